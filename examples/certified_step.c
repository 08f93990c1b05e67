/*
 * certified_step.c -- a complete C host for ONE certified bf16 plan step of libm3pc_hip.so (include/m3pc_hip.h):
 * rtg_guiding, learner.py:271-327, with the candidate pass in bf16 and both returned actions -- the arg-max behind eval_action
 * (learner.py:318-323) and the multinomial draw behind sample_action (learner.py:324-325) -- certified to be the fp32 path's.
 *
 * The host brings everything in buffers of its own: the model's sizes, its state_dict as m3pc_named_tensor entries, the four
 * tokenizers' statistics, the raw window (states / actions / rewards, device), the candidates' standard normals and the
 * draw's Exp(1) variates (device).  The routine creates a handle, loads weights and tokenizers, calibrates delta on this
 * window (a planner does that on the first steps behind every weight load and keeps the maximum: m3pc_amd/planner.py), makes
 * the ONE call and releases the handle.  No HIP call of its own: device memory and the stream are the caller's.
 *
 *   gcc -O2 -Wall -Werror -I include -c examples/certified_step.c
 *   (link with -L<dir of libm3pc_hip.so> -l:libm3pc_hip.so)
 */
#include <stdio.h>
#include <string.h>

#include "m3pc_hip.h"

typedef struct certified_step_io {
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
    const float* eps;     /* (n,T,A) standard normals: dist.sample((N,)), learner.py:285-287 */
    const float* expo;    /* (n,) Exp(1): torch.multinomial(p, 1) is arg-max p / expo */
    int n, horizon;       /* cfg.action_samples, the step's effective horizon */
    double rtg, lmbda, discount; /* host */
    float temperature;           /* host: cfg.temperature */
    /* results (device) */
    float* sample_actions; /* (n,horizon,A) */
    float* scores_low;     /* (n,) bf16 scores */
    float* merged;         /* (n,) the vector the select ran on */
    float* eval_action;    /* (A,) */
    int* argmax;           /* (1,) */
    int* sample_idx;       /* (1,) */
    float* sample_action;  /* (A,) */
    /* results (host) */
    m3pc_cert_record record;
    float delta; /* the calibrated bound the step went in with */
} certified_step_io;

/* -> 0, or the library's negative code (the message on stderr) */
int certified_step(certified_step_io* io, int device, void* stream) {
    m3pc_handle* h = 0;
    int rc = m3pc_create(io->dims, device, &h);
    if (rc == 0) rc = m3pc_load_weights(h, io->weights, io->n_weights, stream);
    for (int k = 0; k < 4 && rc == 0; ++k)
        rc = m3pc_set_tokenizer(h, k, io->tok_mean[k], io->tok_std[k], io->tok_dim[k], io->tok_normalize[k]);

    m3pc_plan_args args;
    memset(&args, 0, sizeof(args));
    args.mode = M3PC_MODE_RTG;
    args.precision = M3PC_PREC_BF16;
    args.horizon = io->horizon;
    args.n_total = args.n_count = io->n; /* one rank scores every candidate */
    args.lmbda = io->lmbda;
    args.discount = io->discount;
    args.rtg = io->rtg;

    /* delta: one bf16 step for its scores, one full fp32 pass inside m3pc_calibrate_delta (factor 1.6: m3pc_amd/planner.py) */
    if (rc == 0)
        rc = m3pc_plan_step(h, &args, io->states, io->actions, io->rewards, io->eps, 0, 0, io->sample_actions, io->scores_low, 0, 0,
                            stream);
    if (rc == 0)
        rc = m3pc_calibrate_delta(h, &args, io->states, io->actions, io->rewards, io->eps, io->scores_low, 1.6f, &io->delta, stream);

    /* the certified step: 6 candidates by score and 2 by race key in the first pass, up to 128 + 32 through the lists */
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
        rc = m3pc_plan_step_certified(h, &args, &cert, io->states, io->actions, io->rewards, io->eps, io->expo, 0, 0,
                                      io->sample_actions, io->scores_low, io->merged, 0, 0, io->eval_action, io->argmax,
                                      io->sample_idx, io->sample_action, &io->record, stream);
    if (rc != 0) fprintf(stderr, "certified_step: %d: %s\n", rc, m3pc_last_error());
    /* every device output is complete in stream order; m3pc_destroy synchronises the device before it frees the handle */
    m3pc_destroy(h);
    return rc;
}
