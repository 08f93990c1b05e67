/*
 * pipelined_eval.c -- pipelined_steps.c with the eval_action certificate: a complete C host that plans K independent windows of an
 * EVALUATION rollout (every step returns eval_action, learner.py:318-323) with up to three certified low-precision plan steps of
 * libm3pc_hip.so in flight, each within `eval_tol` of the fp32 step's eval_action under the certificate's delta model
 * (include/m3pc_hip.h: m3pc_plan_step_certified_eval_begin / _eval_end).  The bound of a step goes out with its tail, so a step whose
 * certificates are satisfied at their first read costs the host no second wait.
 *
 * The host brings the model (sizes, state_dict entries, tokenizer statistics), the K raw windows (device) and buffers for
 * the results of every step; it brings NO random numbers: the candidates' normals and the draw's exponentials of step t are
 * m3pc_draw_variates(seed, t), drawn into one of M3PC_SLOTS scratch buffers of the caller.  Step t owns slot t % M3PC_SLOTS:
 * m3pc_plan_step_certified_eval_begin enqueues it and returns at once, and the step begun three steps earlier is resolved
 * (m3pc_plan_step_certified_eval_end) before the next one begins, so three steps overlap on the device while the host only ever
 * waits for the oldest one's certificate.  No HIP call of its own: device memory and the stream are the caller's.
 *
 *   gcc -O2 -Wall -Werror -I include -c examples/pipelined_eval.c
 *   (link with -L<dir of libm3pc_hip.so> -l:libm3pc_hip.so)
 */
#include <stdio.h>
#include <string.h>

#include "m3pc_hip.h"

#define IN_FLIGHT (M3PC_SLOTS - 1)

typedef struct pipelined_eval_io {
    /* model and tokenizers (host) */
    const m3pc_dims* dims;
    const m3pc_named_tensor* weights; /* omtm.state_dict(): every required name */
    int n_weights;
    const float* tok_mean[4]; /* per key (M3PC_STATES ...): `tok_dim[k]` floats each */
    const float* tok_std[4];
    int tok_dim[4];
    int tok_normalize[4];
    /* the windows (device), complete before the call */
    int n_windows;        /* K */
    const float* states;  /* (K,T,S) raw windows, future rows zero (learner.py:348-366) */
    const float* actions; /* (K,T,A) */
    const float* rewards; /* (K,T,1) */
    int n, horizon;       /* cfg.action_samples, the steps' effective horizon */
    int precision;        /* M3PC_PREC_BF16 / M3PC_PREC_BF16X3 (the tier that reaches 1e-4 at a flat softmax) */
    double rtg, lmbda, discount; /* host */
    float temperature;           /* host: cfg.temperature */
    float eval_tol;              /* host: > 0; INFINITY reports the bound only */
    unsigned long long seed;     /* of the library's variates; the step index is the counter */
    /* scratch (device): the variates of the steps in flight, one set per slot */
    float* eps;  /* (M3PC_SLOTS, n, T, A) */
    float* expo; /* (M3PC_SLOTS, n) */
    /* results (device), per step */
    float* sample_actions; /* (K, n, horizon, A) */
    float* scores_low;     /* (K, n) bf16 scores */
    float* merged;         /* (K, n) the vectors the selects ran on */
    float* eval_action;    /* (K, A) */
    int* argmax;           /* (K,) */
    int* sample_idx;       /* (K,) */
    float* sample_action;  /* (K, A) */
    /* results (host) */
    m3pc_cert_record* records;      /* (K,) */
    m3pc_eval_record* eval_records; /* (K,) */
    float delta;               /* the calibrated bound every step went in with */
} pipelined_eval_io;

/* -> 0, or the library's negative code (the message on stderr) */
int pipelined_eval(pipelined_eval_io* io, int device, void* stream) {
    m3pc_handle* h = 0;
    const int n = io->n, T = io->dims->traj_length, S = io->dims->state_dim, A = io->dims->action_dim, H = io->horizon;
    int rc = m3pc_create(io->dims, device, &h);
    if (rc == 0) rc = m3pc_load_weights(h, io->weights, io->n_weights, stream);
    for (int k = 0; k < 4 && rc == 0; ++k)
        rc = m3pc_set_tokenizer(h, k, io->tok_mean[k], io->tok_std[k], io->tok_dim[k], io->tok_normalize[k]);

    m3pc_plan_args args;
    memset(&args, 0, sizeof(args));
    args.mode = M3PC_MODE_RTG;
    args.precision = io->precision;
    args.horizon = H;
    args.n_total = args.n_count = n; /* one rank scores every candidate */
    args.lmbda = io->lmbda;
    args.discount = io->discount;
    args.rtg = io->rtg;

    /* delta: calibrated on window 0 with the variates of step 0 -- one bf16 step for its scores, one full fp32 pass inside
     * m3pc_calibrate_delta (a planner keeps the maximum over the first steps behind a weight load: m3pc_amd/planner.py) */
    if (rc == 0) rc = m3pc_draw_variates(h, io->seed, 0, 0, n, T * A, io->eps, io->expo, stream);
    if (rc == 0)
        rc = m3pc_plan_step(h, &args, io->states, io->actions, io->rewards, io->eps, 0, 0, io->sample_actions, io->scores_low, 0, 0, stream);
    if (rc == 0)
        rc = m3pc_calibrate_delta(h, &args, io->states, io->actions, io->rewards, io->eps, io->scores_low, 1.6f, &io->delta, stream);

    m3pc_cert_args cert;
    memset(&cert, 0, sizeof(cert));
    cert.temperature = io->temperature;
    cert.delta = io->delta;
    cert.grow_delta = 1;
    cert.kmax = n - 1 < 128 ? (n > 1 ? n - 1 : 1) : 128;
    cert.kmin = cert.kmax < 6 ? cert.kmax : 6;
    cert.rmax = n < 32 ? n : 32;
    cert.rfirst = cert.rmax < 2 ? cert.rmax : 2;

    /* the pipeline: the step begun IN_FLIGHT steps ago is resolved before step t begins (its slot's variates are free again
     * one step later: step t draws into slot t % M3PC_SLOTS, last used by step t - M3PC_SLOTS) */
    int begun = 0, ended = 0;
    for (int t = 0; t < io->n_windows + IN_FLIGHT && rc == 0; ++t) {
        if (t >= IN_FLIGHT && ended < begun) {
            rc = m3pc_plan_step_certified_eval_end(h, ended % M3PC_SLOTS, &io->records[ended], &io->eval_records[ended], stream);
            ++ended;
        }
        if (t < io->n_windows && rc == 0) {
            const int slot = t % M3PC_SLOTS;
            float* eps = io->eps + (size_t)slot * n * T * A;
            float* expo = io->expo + (size_t)slot * n;
            args.slot = slot;
            rc = m3pc_draw_variates(h, io->seed, (unsigned long long)t, 0, n, T * A, eps, expo, stream);
            if (rc == 0)
                rc = m3pc_plan_step_certified_eval_begin(h, &args, &cert, io->states + (size_t)t * T * S, io->actions + (size_t)t * T * A,
                                                         io->rewards + (size_t)t * T, eps, expo, 0, 0,
                                                         io->sample_actions + (size_t)t * n * H * A, io->scores_low + (size_t)t * n,
                                                         io->merged + (size_t)t * n, 0, 0, io->eval_action + (size_t)t * A,
                                                         io->argmax + t, io->sample_idx + t, io->sample_action + (size_t)t * A,
                                                         io->eval_tol, stream);
            if (rc == 0) ++begun;
        }
    }
    if (rc != 0) fprintf(stderr, "pipelined_eval: %d: %s\n", rc, m3pc_last_error());
    for (int t = 0; t < ended && rc == 0; ++t) /* a step ends certified: within eval_tol, or on fp32 scores for every candidate */
        if (!io->records[t].certified || !io->eval_records[t].eval_certified) rc = -100 - t;
    /* every device output is complete in stream order; m3pc_destroy synchronises the device (draining any step still begun
     * after an error) before it frees the handle */
    m3pc_destroy(h);
    return rc;
}
