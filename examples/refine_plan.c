/*
 * refine_plan.c -- a complete C host for the iterative refinement of a plan with libm3pc_hip.so (include/m3pc_hip.h):
 * m3pc_refine_plan, the CEM / MPPI loop around the model's plan step (score the candidates, keep the top_k, refit mean and std
 * per (step, action), resample, clamp to [-1, 1]), twice in a row: the first refinement starts from the policy's mean, the
 * second is warm-started from the first one's final mean.  The library draws the noise itself (its counter-based generator on
 * (seed, step)), so the host needs no generator, and nothing is read back between the two calls.
 *
 * The host brings the model's sizes, its state_dict as m3pc_named_tensor entries, the four tokenizers' statistics and the raw
 * windows of the two steps (states / actions / rewards, device).  A receding-horizon controller would shift the warm-start mean
 * by the steps that passed between the two windows; with the same horizon it is passed as it is.  No HIP call of its own: device
 * memory and the stream are the caller's.
 *
 *   gcc -O2 -Wall -Werror -I include -c examples/refine_plan.c
 *   (link with -L<dir of libm3pc_hip.so> -l:libm3pc_hip.so)
 */
#include <stdio.h>
#include <string.h>

#include "m3pc_hip.h"

typedef struct refine_plan_io {
    /* model and tokenizers (host) */
    const m3pc_dims* dims;
    const m3pc_named_tensor* weights; /* omtm.state_dict(): every required name */
    int n_weights;
    const float* tok_mean[4]; /* per key (M3PC_STATES ...): `tok_dim[k]` floats each */
    const float* tok_std[4];
    int tok_dim[4];
    int tok_normalize[4];
    /* the two steps (device unless stated) */
    const float* states[2];  /* (T,S) raw window, future rows zero (learner.py:348-366) */
    const float* actions[2]; /* (T,A) */
    const float* rewards[2]; /* (T,1) */
    int n, horizon;          /* cfg.action_samples, the steps' effective horizon */
    int precision;           /* M3PC_PREC_* of the scoring */
    int iterations, top_k, weighting; /* host: the loop (M3PC_REFINE_CEM / M3PC_REFINE_MPPI) */
    float temperature, init_std, min_std;
    double rtg, lmbda, discount; /* host */
    unsigned long long seed, step; /* host: the generator's coordinates of the first call; the second uses step + 1 */
    /* results (device), per call */
    float* mean[2];          /* (iterations + 1, horizon, A) */
    float* std[2];           /* (iterations + 1, horizon, A) */
    float* candidates[2];    /* (n, horizon, A) */
    float* sample_action[2]; /* (A,) */
    float* eval_action[2];   /* (A,) */
} refine_plan_io;

/* -> 0, or the library's negative code (the message on stderr) */
int refine_plan(refine_plan_io* io, int device, void* stream) {
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

    m3pc_refine_args refine;
    memset(&refine, 0, sizeof(refine));
    refine.iterations = io->iterations;
    refine.top_k = io->top_k;
    refine.weighting = io->weighting;
    refine.temperature = io->temperature;
    refine.init_std = io->init_std;
    refine.min_std = io->min_std;
    refine.seed_lo = (unsigned int)io->seed;
    refine.seed_hi = (unsigned int)(io->seed >> 32);

    const float* warm = 0; /* the first call starts from tanh of the policy loc */
    for (int c = 0; c < 2 && rc == 0; ++c) {
        const unsigned long long step = io->step + (unsigned long long)c;
        refine.step_lo = (unsigned int)step;
        refine.step_hi = (unsigned int)(step >> 32);
        rc = m3pc_refine_plan(h, &args, &refine, io->states[c], io->actions[c], io->rewards[c], warm, 0, io->mean[c], io->std[c],
                              io->candidates[c], 0, 0, io->sample_action[c], io->eval_action[c], stream);
        /* the final mean of this call -- row `iterations` of its (iterations + 1, horizon, A) means -- in stream order */
        warm = io->mean[c] + (size_t)io->iterations * io->horizon * io->dims->action_dim;
    }
    if (rc != 0) fprintf(stderr, "refine_plan: %d: %s\n", rc, m3pc_last_error());
    /* every device output is complete in stream order; m3pc_destroy synchronises the device before it frees the handle */
    m3pc_destroy(h);
    return rc;
}
