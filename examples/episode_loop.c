/*
 * episode_loop.c -- a complete closed loop in C: E environments that step together, their episodes kept in the library's episode
 * store (m3pc_episodes_*, include/m3pc_hip.h) and planned by one m3pc_plan_steps_certified call per round.  It is what
 * m3pc_amd/rollout.py's evaluate_plan(lockstep="native", store=True) runs, from the library alone: the host restates none of the
 * window rules of action_sample (learner.py:342-366) -- the shrinking horizon of an episode's first steps, history_length =
 * T - h + 1 -- and keeps no episode buffer of its own.
 *
 * Per round:  m3pc_episodes_observe (the E observations, host memory)  ->  m3pc_episodes_windows (the (E,T,S) / (E,T,A) / (E,T,1)
 * windows on the device, the round's effective horizon on the host)  ->  m3pc_draw_variates + m3pc_plan_steps_certified (fp32, so
 * that the example needs no calibrated bound; examples/lockstep_steps.c shows the bf16 step)  ->  the E sampled actions read
 * back, the simulator stepped  ->  m3pc_episodes_record (clip to [-1, 1], write, path_length += 1).  At the end the discounted
 * values of replay_buffer.py:234-243 and every environment's blocks come out of the store.
 *
 * The simulator is a toy in this file (toy_reset / toy_step): obs' = tanh(0.8 roll(obs) + 0.5 a), reward = -mean(obs'^2).
 * The one HIP call of the host is the read-back of the actions; device buffers and the stream are the caller's.
 *
 *   gcc -O2 -Wall -Werror -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include -c examples/episode_loop.c
 *   (link with -L<dir of libm3pc_hip.so> -l:libm3pc_hip.so -lamdhip64 -lm)
 */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "m3pc_hip.h"

typedef struct episode_loop_io {
    /* model and tokenizers (host) */
    const m3pc_dims* dims; /* max_batch >= n_envs */
    const m3pc_named_tensor* weights;
    int n_weights;
    const float* tok_mean[4];
    const float* tok_std[4];
    int tok_dim[4];
    int tok_normalize[4];
    /* the loop */
    int n_rounds, n_envs, max_steps; /* n_rounds <= max_steps */
    int n, horizon;                  /* cfg.action_samples, cfg.horizon */
    double lmbda, discount, rtg;
    float temperature;
    unsigned long long seed;
    /* scratch (device) */
    float *states, *actions, *rewards; /* (E,T,S) (E,T,A) (E,T,1): the windows of a round */
    float *eps, *expo;                 /* (E,n,T,A) (E,n) */
    float *sample_actions, *scores_low, *merged; /* (E,n,T,A) (E,n) (E,n) */
    float* sample_action;              /* (E,A) */
    /* scratch (host) */
    float *obs_host, *act_host, *rew_host; /* (E,S) (E,A) (E,) */
    double* rtg_host;                  /* (E,) */
    int* horizons_host;                /* (E,) */
    m3pc_cert_record* records;         /* (E,) */
    /* results */
    float* actions_log;  /* host (K,E,A): the actions as planned, before the clip */
    float* rewards_log;  /* host (K,E) */
    int* horizons_log;   /* host (K,): the effective horizon of every round */
    float* values;       /* device (E, max_steps) */
    float *obs_out, *act_out, *rew_out; /* device (E,max_steps,S) (E,max_steps,A) (E,max_steps) */
    int* path_length;    /* host (E,) */
} episode_loop_io;

static void toy_reset(float* obs, int e, int S) {
    for (int j = 0; j < S; ++j) obs[j] = sinf(0.37f * (float)(e * S + j) + 0.1f);
}

static float toy_step(float* obs, const float* a, int S, int A) {
    float first = obs[0], sum = 0.f;
    for (int j = 0; j < S; ++j) {
        const float next = j + 1 < S ? obs[j + 1] : first;
        obs[j] = tanhf(0.8f * next + 0.5f * a[j % A]);
        sum += obs[j] * obs[j];
    }
    return -sum / (float)S;
}

/* -> 0, or a negative code (the message on stderr) */
int episode_loop(episode_loop_io* io, int device, void* stream) {
    m3pc_handle* h = 0;
    m3pc_episodes* ep = 0;
    const int n = io->n, E = io->n_envs, T = io->dims->traj_length, S = io->dims->state_dim, A = io->dims->action_dim;
    const int M = io->max_steps;
    int rc = m3pc_create(io->dims, device, &h);
    if (rc == 0) rc = m3pc_load_weights(h, io->weights, io->n_weights, stream);
    for (int k = 0; k < 4 && rc == 0; ++k)
        rc = m3pc_set_tokenizer(h, k, io->tok_mean[k], io->tok_std[k], io->tok_dim[k], io->tok_normalize[k]);
    if (rc == 0) rc = m3pc_episodes_create(h, E, M, &ep);
    if (rc == 0) rc = m3pc_episodes_reset(ep, 0, E, 0, 0, 0, stream); /* env_ids NULL: environments 0 .. E-1 */

    m3pc_plan_args args;
    memset(&args, 0, sizeof(args));
    args.mode = M3PC_MODE_RTG;
    args.precision = M3PC_PREC_FP32;
    args.n_total = args.n_count = n;
    args.lmbda = io->lmbda;
    args.discount = io->discount;
    m3pc_cert_args cert; /* (an fp32 step reads the temperature only) */
    memset(&cert, 0, sizeof(cert));
    cert.temperature = io->temperature;
    cert.kmin = cert.kmax = 1;

    for (int e = 0; e < E; ++e) {
        toy_reset(io->obs_host + (size_t)e * S, e, S);
        io->rtg_host[e] = io->rtg;
    }
    for (int k = 0; k < io->n_rounds && rc == 0; ++k) {
        /* host memory is consumed before a call returns: obs_host, act_host and rew_host are free again at once */
        rc = m3pc_episodes_observe(ep, 0, E, io->obs_host, 0, 0, stream);
        if (rc == 0)
            rc = m3pc_episodes_windows(ep, 0, E, M3PC_WINDOW_PLAN, io->horizon, io->states, io->actions, io->rewards, io->horizons_host,
                                       stream);
        if (rc != 0) break;
        /* environments that step together share the effective horizon (a host whose episodes differ in length groups its
         * windows by horizons_host and plans group by group, as m3pc_amd/planner.py's action_sample_batch does) */
        io->horizons_log[k] = args.horizon = io->horizons_host[0];
        for (int w = 0; w < E && rc == 0; ++w)
            rc = m3pc_draw_variates(h, io->seed, (unsigned long long)k * E + w, 0, n, T * A, io->eps + (size_t)w * n * T * A,
                                    io->expo + (size_t)w * n, stream);
        if (rc == 0)
            rc = m3pc_plan_steps_certified(h, &args, &cert, E, io->states, io->actions, io->rewards, io->rtg_host, io->eps, io->expo, 0, 0,
                                           io->sample_actions, io->scores_low, io->merged, 0, 0, 0, 0, 0, io->sample_action, io->records,
                                           stream);
        if (rc != 0) break;
        if (hipMemcpyAsync(io->act_host, io->sample_action, (size_t)E * A * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream) !=
                hipSuccess ||
            hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
            fprintf(stderr, "episode_loop: the read-back of round %d failed\n", k);
            rc = M3PC_EHIP;
            break;
        }
        memcpy(io->actions_log + (size_t)k * E * A, io->act_host, (size_t)E * A * sizeof(float));
        for (int e = 0; e < E; ++e) {
            float clipped[32]; /* (action_dim <= 32) the simulator sees what the store records: np.clip(action, -1, 1) */
            for (int j = 0; j < A; ++j) {
                const float a = io->act_host[(size_t)e * A + j];
                clipped[j] = a < -1.f ? -1.f : (a > 1.f ? 1.f : a);
            }
            io->rew_host[e] = toy_step(io->obs_host + (size_t)e * S, clipped, S, A);
            io->rewards_log[(size_t)k * E + e] = io->rew_host[e];
        }
        rc = m3pc_episodes_record(ep, 0, E, io->act_host, io->rew_host, -1.f, 1.f, 0, stream);
    }
    if (rc == 0) rc = m3pc_episodes_values(ep, 0, E, io->discount, 0, io->values, stream);
    for (int e = 0; e < E && rc == 0; ++e)
        rc = m3pc_episodes_export(ep, e, io->obs_out + (size_t)e * M * S, io->act_out + (size_t)e * M * A, io->rew_out + (size_t)e * M,
                                  io->path_length + e, 1, stream);
    if (rc != 0 && rc != M3PC_EHIP) fprintf(stderr, "episode_loop: %d: %s\n", rc, m3pc_last_error());
    /* both destroys drain the device before they free */
    m3pc_episodes_destroy(ep);
    m3pc_destroy(h);
    return rc;
}
