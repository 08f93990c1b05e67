/*
 * critic_loop.c -- examples/replay_loop.c extended by the IQL trainer: rollout -> replay -> critic -> planner from the library alone
 * (finetune_omtm/finetune.py:281-310).  E toy environments are rolled out into the episode store, their episodes pushed into a replay
 * buffer, N_STEPS IQL steps (ImplicitQLearning.train, finetune_omtm/model.py:286-308) made on transition batches the library draws
 * (m3pc_iql_train), and the trained TwinQ handed to the handle's critic device to device (m3pc_iql_publish_critic): from then on a plan
 * step with M3PC_MODE_CRITIC (m3pc_plan_step and its kin; episode_loop.c shows the planner in this loop) scores its candidates with
 * it, as after m3pc_set_critic.  Here the published critic is checked through the trainer's own evaluation of the same network
 * (m3pc_iql_evaluate), since the example loads no transformer.  The host keeps no batch and copies nothing but the losses.
 *
 * The networks start from a toy initialisation made of exact arithmetic (every weight a multiple of 1/512); the simulator is
 * replay_loop.c's.
 *
 *   gcc -O2 -Wall -Werror -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/critic_loop.c -o critic_loop \
 *       -L<dir of libm3pc_hip.so> -l:libm3pc_hip.so -L/opt/rocm/lib -lamdhip64 -lm
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "m3pc_hip.h"

enum { E = 4, S = 11, A = 3, T = 8, M = 16, L = 8, HIDDEN = 64, BATCH = 24, N_STEPS = 5, ONLINE_CAPACITY = 64 };
static const int LENGTHS[E] = {16, 5, 11, 8};

static float toy_obs(int e, int t, int j) { return (float)((131 * e + 17 * t + 7 * j) % 64 - 32) / 32.f; }
static float toy_action(int e, int t, int j) { return (float)((29 * e + 5 * t + 3 * j) % 80 - 40) / 32.f; }
static float toy_reward(int e, int t) { return (float)((e + 3 * t) % 16 - 8) / 8.f; }

/* one part's tensors: names by the reference's state_dict, values w[i] = ((salt + 37 i) % 129 - 64) / 512 */
enum { MAX_TENSORS = 13 };
static int make_part(const char* const* prefixes, int n_prefix, int in, int out, int with_log_std, int salt, m3pc_named_tensor* list, char names[][32]) {
    static const char* FIELD[6] = {"net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias"};
    int n = 0;
    for (int p = 0; p < n_prefix; ++p) {
        const long long numel[6] = {(long long)HIDDEN * in, HIDDEN, (long long)HIDDEN * HIDDEN, HIDDEN, (long long)out * HIDDEN, out};
        for (int f = 0; f < 6; ++f, ++n) {
            snprintf(names[n], 32, "%s%s", prefixes[p], FIELD[f]);
            float* w = (float*)malloc(sizeof(float) * (size_t)numel[f]);
            if (!w) return -1;
            for (long long i = 0; i < numel[f]; ++i) w[i] = (float)((salt + 31 * n + 37 * i) % 129 - 64) / 512.f;
            list[n].name = names[n];
            list[n].data = w;
            list[n].numel = numel[f];
            list[n].on_device = 0;
        }
    }
    if (with_log_std) {
        float* w = (float*)malloc(sizeof(float) * A);
        if (!w) return -1;
        for (int i = 0; i < A; ++i) w[i] = -0.5f;
        snprintf(names[n], 32, "log_std");
        list[n].name = names[n];
        list[n].data = w;
        list[n].numel = A;
        list[n].on_device = 0;
        ++n;
    }
    return n;
}
static void free_part(m3pc_named_tensor* list, int n) {
    for (int i = 0; i < n; ++i) free((void*)list[i].data);
}

#define HIP_OK(x)                                                          \
    do {                                                                   \
        if ((x) != hipSuccess) {                                           \
            fprintf(stderr, "critic_loop: %s failed\n", #x);               \
            return 2;                                                      \
        }                                                                  \
    } while (0)

int main(void) {
    m3pc_dims dims;
    memset(&dims, 0, sizeof(dims));
    dims.state_dim = S;
    dims.action_dim = A;
    dims.traj_length = T;
    dims.n_embd = 64;
    dims.n_head = 2;
    dims.n_enc_layer = 2;
    dims.n_dec_layer = 1;
    dims.max_candidates = 64;
    dims.max_batch = 1;
    dims.critic_hidden = HIDDEN; /* the planner's critic has the trainer's width */
    m3pc_handle* h = 0;
    m3pc_episodes* ep = 0;
    m3pc_replay* rb = 0;
    m3pc_iql* iql = 0;
    hipStream_t stream = 0;
    HIP_OK(hipSetDevice(0));
    HIP_OK(hipStreamCreate(&stream));
    int rc = m3pc_create(&dims, 0, &h);
    if (rc == 0) rc = m3pc_episodes_create(h, E, M, &ep);
    if (rc == 0) rc = m3pc_replay_create(h, E, M, L, 0, ONLINE_CAPACITY, &rb);
    if (rc == 0) rc = m3pc_iql_create(h, HIDDEN, &iql);
    if (rc == 0) rc = m3pc_episodes_reset(ep, 0, E, 0, 0, 0, stream);

    /* the rollout of replay_loop.c, then episodes in: the online ring now holds every transition */
    float obs[E * S], act[E * A], rew[E], final_obs[E * S];
    int ids[E];
    for (int t = 0; t < M && rc == 0; ++t) {
        int n = 0;
        for (int e = 0; e < E; ++e) {
            if (t >= LENGTHS[e]) continue;
            for (int j = 0; j < S; ++j) obs[n * S + j] = toy_obs(e, t, j);
            for (int j = 0; j < A; ++j) act[n * A + j] = toy_action(e, t, j);
            rew[n] = toy_reward(e, t);
            ids[n++] = e;
        }
        if (n == 0) break;
        rc = m3pc_episodes_observe(ep, ids, n, obs, 0, 0, stream);
        if (rc == 0) rc = m3pc_episodes_record(ep, ids, n, act, rew, -1.f, 1.f, 0, stream);
    }
    for (int e = 0; e < E; ++e)
        for (int j = 0; j < S; ++j) final_obs[e * S + j] = toy_obs(e, LENGTHS[e], j);
    int n_online = 0;
    if (rc == 0) rc = m3pc_replay_push_episodes(rb, ep, 0, E, 0.99, 0, final_obs, 0, 0, stream);
    if (rc == 0) rc = m3pc_replay_counts(rb, 0, 0, &n_online);

    /* load_state_dict, part by part; q_target starts as a copy of qf (model.py:213) */
    static const char* const QP[2] = {"q1.", "q2."};
    static const char* const VP[1] = {"v."};
    static const char* const AP[1] = {"net."};
    m3pc_named_tensor qf[MAX_TENSORS], vf[MAX_TENSORS], actor[MAX_TENSORS];
    static char qn[MAX_TENSORS][32], vn[MAX_TENSORS][32], an[MAX_TENSORS][32];
    const int nq = make_part(QP, 2, S + A, 1, 0, 3, qf, qn), nv = make_part(VP, 1, S, 1, 0, 5, vf, vn), na = make_part(AP, 1, S, A, 1, 7, actor, an);
    if (nq < 0 || nv < 0 || na < 0) return 2;
    float obs_mean[S], obs_std[S];
    for (int j = 0; j < S; ++j) obs_mean[j] = 0.f, obs_std[j] = 1.f;
    if (rc == 0) rc = m3pc_iql_load(iql, M3PC_IQL_QF, qf, nq, obs_mean, obs_std, stream);
    if (rc == 0) rc = m3pc_iql_load(iql, M3PC_IQL_Q_TARGET, qf, nq, 0, 0, stream);
    if (rc == 0) rc = m3pc_iql_load(iql, M3PC_IQL_VF, vf, nv, 0, 0, stream);
    if (rc == 0) rc = m3pc_iql_load(iql, M3PC_IQL_ACTOR, actor, na, 0, 0, stream);
    free_part(qf, nq); /* (host tensors are consumed before m3pc_iql_load returns) */
    free_part(vf, nv);
    free_part(actor, na);

    /* critic_update x N_STEPS (finetune.py:288-290) on the batches the buffer draws for (seed, 0 .. N_STEPS - 1), then the hand-over */
    m3pc_iql_args args;
    memset(&args, 0, sizeof(args));
    args.v_lr = args.q_lr = args.actor_lr = 3e-4;
    args.expectile = 0.7;
    args.beta = 3.0;
    args.discount = 0.99;
    args.tau = 0.005;
    args.actor_t_max = 1000000;
    float *losses, *q_eval, *es, *ea;
    HIP_OK(hipMalloc((void**)&losses, sizeof(float) * N_STEPS * 3));
    HIP_OK(hipMalloc((void**)&q_eval, sizeof(float) * E));
    HIP_OK(hipMalloc((void**)&es, sizeof(float) * E * S));
    HIP_OK(hipMalloc((void**)&ea, sizeof(float) * E * A));
    if (rc == 0) rc = m3pc_iql_train(iql, &args, rb, N_STEPS, BATCH, BATCH, 7ull, 0ull, losses, stream);
    if (rc == 0) rc = m3pc_iql_publish_critic(iql, h, stream);
    /* the value the planner's critic now gives the first (state, action) of every episode */
    for (int e = 0; e < E; ++e) {
        for (int j = 0; j < S; ++j) obs[e * S + j] = toy_obs(e, 0, j);
        for (int j = 0; j < A; ++j) act[e * A + j] = toy_action(e, 0, j);
    }
    HIP_OK(hipMemcpyAsync(es, obs, sizeof(obs), hipMemcpyHostToDevice, stream));
    HIP_OK(hipMemcpyAsync(ea, act, sizeof(act), hipMemcpyHostToDevice, stream));
    if (rc == 0) rc = m3pc_iql_evaluate(iql, M3PC_IQL_Q_MIN, es, ea, E, q_eval, stream);
    long long total_it = 0;
    if (rc == 0) rc = m3pc_iql_get_step(iql, &total_it);
    if (rc != 0) {
        fprintf(stderr, "critic_loop: %d: %s\n", rc, m3pc_last_error());
        return 1;
    }
    float hl[N_STEPS * 3], hq[E];
    HIP_OK(hipMemcpyAsync(hl, losses, sizeof(hl), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(hq, q_eval, sizeof(hq), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    printf("online %d total_it %lld\n", n_online, total_it);
    for (int k = 0; k < N_STEPS; ++k) printf("step %d value_loss %.9g q_loss %.9g actor_loss %.9g\n", k, hl[3 * k], hl[3 * k + 1], hl[3 * k + 2]);
    printf("q_min");
    for (int e = 0; e < E; ++e) printf(" %.9g", hq[e]);
    printf("\n");

    m3pc_iql_destroy(iql);
    m3pc_replay_destroy(rb);
    m3pc_episodes_destroy(ep);
    m3pc_destroy(h);
    void* bufs[] = {losses, q_eval, es, ea};
    for (size_t i = 0; i < sizeof(bufs) / sizeof(bufs[0]); ++i) (void)hipFree(bufs[i]);
    (void)hipStreamDestroy(stream);
    return 0;
}
