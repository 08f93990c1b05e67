/*
 * certified_eval.c -- a complete C host for ONE certified plan step of libm3pc_hip.so (include/m3pc_hip.h) whose eval_action is
 * held to a tolerance: rtg_guiding, learner.py:271-327, with the candidate pass in low precision, the arg-max and the multinomial
 * draw certified to be the fp32 path's, and eval_action (learner.py:318-323: the softmax-weighted mean over ALL candidates, what
 * every eval=True call returns) within `eval_tol` of the fp32 step's under the same delta model -- m3pc_plan_step_certified_eval.
 *
 * The host brings everything in buffers of its own, as in certified_step.c: the model's sizes, its state_dict, the tokenizers'
 * statistics, the raw window, the candidates' standard normals and the draw's Exp(1) variates (device).  The routine creates a
 * handle, loads weights and tokenizers, calibrates delta on this window, makes the ONE call, prints the two records and releases
 * the handle.  No HIP call of its own: device memory and the stream are the caller's.
 *
 * Which precision to ask for: at the nearly flat softmax of rtg guidance (temperature 0.01) bf16's delta leaves a bound no list
 * lowers to 1e-3 -- the step then scores every candidate in fp32 (record.everything = 1) --; M3PC_PREC_BF16X3 certifies 1e-4 with
 * nothing extra re-scored.
 *
 *   gcc -O2 -Wall -Werror -I include -c examples/certified_eval.c
 *   (link with -L<dir of libm3pc_hip.so> -l:libm3pc_hip.so)
 */
#include <stdio.h>
#include <string.h>

#include "m3pc_hip.h"

typedef struct certified_eval_io {
    /* model and tokenizers (host) */
    const m3pc_dims* dims;
    const m3pc_named_tensor* weights; /* omtm.state_dict(): every required name */
    int n_weights;
    const float* tok_mean[4]; /* per key (M3PC_STATES ...): `tok_dim[k]` floats each */
    const float* tok_std[4];
    int tok_dim[4];
    int tok_normalize[4];
    /* the step (device unless stated) */
    const float* states;  /* (T,S) raw window, future rows zero (learner.py:348-366) */
    const float* actions; /* (T,A) */
    const float* rewards; /* (T,1) */
    const float* eps;     /* (n,T,A) standard normals */
    const float* expo;    /* (n,) Exp(1) */
    int n, horizon;       /* cfg.action_samples, the step's effective horizon */
    int precision;        /* host: M3PC_PREC_BF16 or M3PC_PREC_BF16X3 */
    double rtg, lmbda, discount; /* host */
    float temperature;           /* host: cfg.temperature */
    float eval_tol;              /* host: the tolerance on eval_action (> 0; infinity: report the bound only) */
    /* results (device) */
    float* sample_actions; /* (n,horizon,A) */
    float* scores_low;     /* (n,) low-precision scores */
    float* merged;         /* (n,) the vector the select ran on */
    float* eval_action;    /* (A,) */
    int* argmax;           /* (1,) */
    int* sample_idx;       /* (1,) */
    float* sample_action;  /* (A,) */
    /* results (host) */
    m3pc_cert_record record;
    m3pc_eval_record eval_record;
    float delta; /* the calibrated bound the step went in with */
} certified_eval_io;

/* -> 0, or the library's negative code (the message on stderr) */
int certified_eval(certified_eval_io* io, int device, void* stream) {
    m3pc_handle* h = 0;
    int rc = m3pc_create(io->dims, device, &h);
    if (rc == 0) rc = m3pc_load_weights(h, io->weights, io->n_weights, stream);
    for (int k = 0; k < 4 && rc == 0; ++k)
        rc = m3pc_set_tokenizer(h, k, io->tok_mean[k], io->tok_std[k], io->tok_dim[k], io->tok_normalize[k]);

    m3pc_plan_args args;
    memset(&args, 0, sizeof(args));
    args.mode = M3PC_MODE_RTG;
    args.precision = io->precision;
    args.horizon = io->horizon;
    args.n_total = args.n_count = io->n; /* one rank scores every candidate */
    args.lmbda = io->lmbda;
    args.discount = io->discount;
    args.rtg = io->rtg;

    /* delta: one low-precision step for its scores, one full fp32 pass inside m3pc_calibrate_delta (factor 1.6) */
    if (rc == 0)
        rc = m3pc_plan_step(h, &args, io->states, io->actions, io->rewards, io->eps, 0, 0, io->sample_actions, io->scores_low, 0, 0,
                            stream);
    if (rc == 0)
        rc = m3pc_calibrate_delta(h, &args, io->states, io->actions, io->rewards, io->eps, io->scores_low, 1.6f, &io->delta, stream);

    m3pc_cert_args cert;
    memset(&cert, 0, sizeof(cert));
    cert.temperature = io->temperature;
    cert.delta = io->delta;
    cert.grow_delta = 1;
    cert.kmax = io->n - 1 < 128 ? (io->n > 1 ? io->n - 1 : 1) : 128;
    cert.kmin = cert.kmax < 6 ? cert.kmax : 6;
    cert.rmax = io->n < 32 ? io->n : 32;
    cert.rfirst = cert.rmax < 2 ? cert.rmax : 2;
    if (rc == 0)
        rc = m3pc_plan_step_certified_eval(h, &args, &cert, io->states, io->actions, io->rewards, io->eps, io->expo, 0, 0,
                                           io->sample_actions, io->scores_low, io->merged, 0, 0, io->eval_action, io->argmax,
                                           io->sample_idx, io->sample_action, &io->record, io->eval_tol, &io->eval_record, stream);
    if (rc != 0) {
        fprintf(stderr, "certified_eval: %d: %s\n", rc, m3pc_last_error());
    } else {
        const m3pc_cert_record* r = &io->record;
        const m3pc_eval_record* e = &io->eval_record;
        printf("cert record: n_rescored %d n_race %d need_first %d need_race_first %d saturated %d everything %d certified %d rounds %d "
               "delta %g shift %g deviation %g margin %g\n",
               r->n_rescored, r->n_race, r->need_first, r->need_race_first, r->saturated, r->everything, r->certified, r->rounds,
               (double)r->delta, (double)r->shift, (double)r->deviation, (double)r->margin);
        printf("eval record: eval_bound %g (eval_tol %g) need_eval_first %d n_eval %d eval_rounds %d eval_certified %d\n",
               (double)e->eval_bound, (double)io->eval_tol, e->need_eval_first, e->n_eval, e->eval_rounds, e->eval_certified);
        fflush(stdout);
    }
    /* every device output is complete in stream order; m3pc_destroy synchronises the device before it frees the handle */
    m3pc_destroy(h);
    return rc;
}
