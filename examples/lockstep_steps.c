/*
 * lockstep_steps.c -- a complete C host that plans E environments which step together, one m3pc_plan_steps_certified call of
 * libm3pc_hip.so per round (include/m3pc_hip.h): rtg_guiding, learner.py:271-327, for E windows at once -- one policy pass at
 * batch E, every window's own bf16 candidate pass, the lists, ONE fp32 re-score pass and the merge + select of all windows in one
 * launch each, then each window's certificates.  It is what m3pc_amd/planner.py's action_sample_batch(lockstep="native") runs,
 * from the library alone.
 *
 * The host brings the model (sizes with max_batch >= E, state_dict entries, tokenizer statistics), the raw windows of every round
 * (device) and buffers for the results; it brings NO random numbers: window w of round k plans with the variates of step index
 * k E + w, m3pc_draw_variates(seed, k E + w), drawn into row w of the caller's scratch.  The bound comes from m3pc_calibrate_delta
 * on window 0 of round 0; with grow_delta a round folds back what its last window's record carries.  No HIP call of its own: device
 * memory and the stream are the caller's.
 *
 *   gcc -O2 -Wall -Werror -I include -c examples/lockstep_steps.c
 *   (link with -L<dir of libm3pc_hip.so> -l:libm3pc_hip.so)
 */
#include <stdio.h>
#include <string.h>

#include "m3pc_hip.h"

typedef struct lockstep_steps_io {
    /* model and tokenizers (host) */
    const m3pc_dims* dims; /* max_batch >= n_envs */
    const m3pc_named_tensor* weights; /* omtm.state_dict(): every required name */
    int n_weights;
    const float* tok_mean[4]; /* per key (M3PC_STATES ...): `tok_dim[k]` floats each */
    const float* tok_std[4];
    int tok_dim[4];
    int tok_normalize[4];
    /* the windows (device), complete before the call */
    int n_rounds, n_envs; /* K rounds of E environments */
    const float* states;  /* (K,E,T,S) raw windows, future rows zero (learner.py:348-366) */
    const float* actions; /* (K,E,T,A) */
    const float* rewards; /* (K,E,T,1) */
    const double* rtg;    /* host (K,E): return-to-go per window */
    int n, horizon;       /* cfg.action_samples, the windows' effective horizon */
    double lmbda, discount; /* host */
    float temperature;      /* host: cfg.temperature */
    unsigned long long seed; /* of the library's variates; the step index k E + w is the counter */
    /* scratch (device): the variates of one round */
    float* eps;  /* (E, n, T, A) */
    float* expo; /* (E, n) */
    /* results (device), per round and window */
    float* sample_actions; /* (K, E, n, horizon, A) */
    float* scores_low;     /* (K, E, n) bf16 scores */
    float* merged;         /* (K, E, n) the vectors the selects ran on */
    float* eval_action;    /* (K, E, A) */
    int* argmax;           /* (K, E) */
    int* sample_idx;       /* (K, E) */
    float* sample_action;  /* (K, E, A) */
    /* results (host) */
    m3pc_cert_record* records; /* (K, E) */
    float delta;               /* the calibrated bound round 0 went in with */
} lockstep_steps_io;

/* -> 0, or the library's negative code (the message on stderr) */
int lockstep_steps(lockstep_steps_io* io, int device, void* stream) {
    m3pc_handle* h = 0;
    const int n = io->n, E = io->n_envs, T = io->dims->traj_length, S = io->dims->state_dim, A = io->dims->action_dim, H = io->horizon;
    int rc = m3pc_create(io->dims, device, &h);
    if (rc == 0) rc = m3pc_load_weights(h, io->weights, io->n_weights, stream);
    for (int k = 0; k < 4 && rc == 0; ++k)
        rc = m3pc_set_tokenizer(h, k, io->tok_mean[k], io->tok_std[k], io->tok_dim[k], io->tok_normalize[k]);

    m3pc_plan_args args;
    memset(&args, 0, sizeof(args));
    args.mode = M3PC_MODE_RTG;
    args.precision = M3PC_PREC_BF16;
    args.horizon = H;
    args.n_total = args.n_count = n; /* one rank scores every candidate */
    args.lmbda = io->lmbda;
    args.discount = io->discount;

    /* delta: calibrated on window 0 of round 0 with the variates of step 0 -- one bf16 step for its scores, one full fp32 pass
     * inside m3pc_calibrate_delta (a planner keeps the maximum over the first steps behind a weight load: m3pc_amd/planner.py) */
    args.rtg = io->rtg[0];
    if (rc == 0) rc = m3pc_draw_variates(h, io->seed, 0, 0, n, T * A, io->eps, io->expo, stream);
    if (rc == 0)
        rc = m3pc_plan_step(h, &args, io->states, io->actions, io->rewards, io->eps, 0, 0, io->sample_actions, io->scores_low, 0, 0, stream);
    if (rc == 0)
        rc = m3pc_calibrate_delta(h, &args, io->states, io->actions, io->rewards, io->eps, io->scores_low, 1.6f, &io->delta, stream);
    args.rtg = 0.0; /* (the batch call takes the return-to-go per window) */

    m3pc_cert_args cert;
    memset(&cert, 0, sizeof(cert));
    cert.temperature = io->temperature;
    cert.delta = io->delta;
    cert.grow_delta = 1;
    cert.kmax = n - 1 < 128 ? (n > 1 ? n - 1 : 1) : 128;
    cert.kmin = cert.kmax < 6 ? cert.kmax : 6;
    cert.rmax = n < 32 ? n : 32;
    cert.rfirst = cert.rmax < 2 ? cert.rmax : 2;

    for (int k = 0; k < io->n_rounds && rc == 0; ++k) {
        const size_t w0 = (size_t)k * E; /* the round's first window */
        for (int w = 0; w < E && rc == 0; ++w)
            rc = m3pc_draw_variates(h, io->seed, (unsigned long long)(w0 + w), 0, n, T * A, io->eps + (size_t)w * n * T * A,
                                    io->expo + (size_t)w * n, stream);
        if (rc == 0)
            rc = m3pc_plan_steps_certified(h, &args, &cert, E, io->states + w0 * T * S, io->actions + w0 * T * A, io->rewards + w0 * T,
                                           io->rtg + w0, io->eps, io->expo, 0, 0, io->sample_actions + w0 * n * H * A,
                                           io->scores_low + w0 * n, io->merged + w0 * n, 0, 0, io->eval_action + w0 * A, io->argmax + w0,
                                           io->sample_idx + w0, io->sample_action + w0 * A, io->records + w0, stream);
        /* the records are valid on return: the bound the round's last window came out with goes into the next round */
        if (rc == 0) cert.delta = io->records[w0 + E - 1].delta;
    }
    if (rc != 0) fprintf(stderr, "lockstep_steps: %d: %s\n", rc, m3pc_last_error());
    /* every device output is complete in stream order; m3pc_destroy synchronises the device before it frees the handle */
    m3pc_destroy(h);
    return rc;
}
