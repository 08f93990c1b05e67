/*
 * refine_plans.c -- a complete C host for the refinement of a lock-step batch of plans with libm3pc_hip.so (include/m3pc_hip.h):
 * m3pc_refine_plans, the CEM / MPPI loop of m3pc_refine_plan for E environments that step together, as one call per round.  Two
 * rounds, as a receding-horizon (MPPI) controller runs them: the first starts every window from its policy's mean; the second is
 * warm-started from the first one's final means SHIFTED by the one environment step that passed (init_offset = 1): row t of the
 * new plan starts from row t + 1 of the old one, and the last row, which the old plan does not reach, from the policy head.  The
 * library draws the noise itself (window w of round c on the generator's (seed, step + c E + w)), and nothing is read back between
 * the rounds.
 *
 * The host brings the model's sizes (max_batch >= E, max_candidates >= E n), its state_dict as m3pc_named_tensor entries, the four
 * tokenizers' statistics and the raw windows of the two rounds (states / actions / rewards, device).  No HIP call of its own:
 * device memory and the stream are the caller's.
 *
 *   gcc -O2 -Wall -Werror -I include -c examples/refine_plans.c
 *   (link with -L<dir of libm3pc_hip.so> -l:libm3pc_hip.so)
 */
#include <stdio.h>
#include <string.h>

#include "m3pc_hip.h"

#define REFINE_PLANS_MAX_WINDOWS 64

typedef struct refine_plans_io {
    /* model and tokenizers (host) */
    const m3pc_dims* dims;
    const m3pc_named_tensor* weights; /* omtm.state_dict(): every required name */
    int n_weights;
    const float* tok_mean[4]; /* per key (M3PC_STATES ...): `tok_dim[k]` floats each */
    const float* tok_std[4];
    int tok_dim[4];
    int tok_normalize[4];
    /* the two rounds (device unless stated) */
    int n_windows;           /* E <= REFINE_PLANS_MAX_WINDOWS */
    const float* states[2];  /* (E,T,S) raw windows, future rows zero (learner.py:348-366) */
    const float* actions[2]; /* (E,T,A) */
    const float* rewards[2]; /* (E,T,1) */
    const double* rtg[2];    /* host (E,) */
    int n, horizon;          /* cfg.action_samples per window, the rounds' effective horizon */
    int precision;           /* M3PC_PREC_* of the scoring */
    int iterations, top_k, weighting; /* host: the loop (M3PC_REFINE_CEM / M3PC_REFINE_MPPI) */
    float temperature, init_std, min_std;
    double lmbda, discount;  /* host */
    unsigned long long seed, step; /* host: the generator's coordinates; window w of round c draws on step + c E + w */
    /* results (device), per round */
    float* mean[2];          /* (iterations + 1, E, horizon, A) */
    float* std[2];           /* (iterations + 1, E, horizon, A) */
    float* candidates[2];    /* (E, n, horizon, A) */
    float* sample_action[2]; /* (E, A) */
    float* eval_action[2];   /* (E, A) */
} refine_plans_io;

/* -> 0, or the library's negative code (the message on stderr) */
int refine_plans(refine_plans_io* io, int device, void* stream) {
    const int E = io->n_windows;
    if (E < 1 || E > REFINE_PLANS_MAX_WINDOWS) return M3PC_EINVAL;
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
    args.n_total = args.n_count = io->n; /* per window; one rank scores every candidate */
    args.lmbda = io->lmbda;
    args.discount = io->discount;

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

    const float* warm = 0; /* the first round starts from tanh of the policy loc: no init_mean */
    for (int c = 0; c < 2 && rc == 0; ++c) {
        unsigned long long steps[REFINE_PLANS_MAX_WINDOWS];
        for (int w = 0; w < E; ++w) steps[w] = io->step + (unsigned long long)c * (unsigned long long)E + (unsigned long long)w;
        /* warm: (E, horizon, A) with init_stride = horizon rows per window, all of them valid (init_rows = NULL), read from row 1 on */
        rc = m3pc_refine_plans(h, &args, &refine, E, io->states[c], io->actions[c], io->rewards[c], io->rtg[c], warm, io->horizon, 0,
                               c == 0 ? 0 : 1, 0, steps, io->mean[c], io->std[c], io->candidates[c], 0, 0, io->sample_action[c],
                               io->eval_action[c], stream);
        /* the final means of this round -- block `iterations` of its (iterations + 1, E, horizon, A) means -- in stream order */
        warm = io->mean[c] + (size_t)io->iterations * E * io->horizon * io->dims->action_dim;
    }
    if (rc != 0) fprintf(stderr, "refine_plans: %d: %s\n", rc, m3pc_last_error());
    /* every device output is complete in stream order; m3pc_destroy synchronises the device before it frees the handle */
    m3pc_destroy(h);
    return rc;
}
