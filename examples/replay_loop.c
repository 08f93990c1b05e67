/*
 * replay_loop.c -- examples/episode_loop.c extended by a replay buffer: the rollout -> buffer -> batch path of the fine-tuning loop
 * (finetune_omtm/finetune.py:281-310) from the library alone.  E toy environments are rolled out into the episode store
 * (m3pc_episodes_*), their episodes pushed into a replay buffer device to device (m3pc_replay_push_episodes: ReplayBuffer.online_rollout
 * :223-251 -- values, update_buffer, the online transitions), and one segment batch (traj_sample, :312-366) and one transition batch
 * (trans_sample, :368-420) drawn by the library; the host keeps no episode, restates no rule and copies nothing but the final
 * batches, which it reads back to print their checksums.
 *
 * Neither object needs weights, so the handle is created from its sizes alone and no model is loaded; episode_loop.c shows the
 * planner in this loop.  The simulator and the policy are toys made of exact integer arithmetic (every value a multiple of 1/32), so
 * that any host restating them -- tests/test_replay_gpu.py does, in NumPy -- holds the same bits:
 *   obs[e][t][j] = ((131 e + 17 t + 7 j) % 64 - 32) / 32,  action[e][t][j] = ((29 e + 5 t + 3 j) % 80 - 40) / 32 (clipped to [-1, 1] by
 *   the store),  reward[e][t] = ((e + 3 t) % 16 - 8) / 8;  episode e ends after LENGTHS[e] steps.
 *
 *   gcc -O2 -Wall -Werror -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/replay_loop.c -o replay_loop \
 *       -L<dir of libm3pc_hip.so> -l:libm3pc_hip.so -L/opt/rocm/lib -lamdhip64 -lm
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "m3pc_hip.h"

enum { E = 4, S = 11, A = 3, T = 8, M = 16, L = 8, B_SEG = 6, B_TRANS = 8, ONLINE_CAPACITY = 24 };
static const int LENGTHS[E] = {16, 5, 11, 8}; /* a full episode, one shorter than a segment (not taken as a trajectory), one of exactly L */

static float toy_obs(int e, int t, int j) { return (float)((131 * e + 17 * t + 7 * j) % 64 - 32) / 32.f; }
static float toy_action(int e, int t, int j) { return (float)((29 * e + 5 * t + 3 * j) % 80 - 40) / 32.f; }
static float toy_reward(int e, int t) { return (float)((e + 3 * t) % 16 - 8) / 8.f; }

/* the sum of n values in index order, in double */
static double checksum_f(const float* x, int n) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += (double)x[i];
    return s;
}
static double checksum_d(const double* x, int n) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += x[i];
    return s;
}

#define HIP_OK(x)                                                          \
    do {                                                                   \
        if ((x) != hipSuccess) {                                           \
            fprintf(stderr, "replay_loop: %s failed\n", #x);               \
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
    m3pc_handle* h = 0;
    m3pc_episodes* ep = 0;
    m3pc_replay* rb = 0;
    hipStream_t stream = 0;
    HIP_OK(hipSetDevice(0));
    HIP_OK(hipStreamCreate(&stream));
    int rc = m3pc_create(&dims, 0, &h);
    if (rc == 0) rc = m3pc_episodes_create(h, E, M, &ep);
    /* no offline ring here: a fine-tuning run fills one from its dataset with m3pc_replay_append_transitions (replay_buffer.py:108-125) */
    if (rc == 0) rc = m3pc_replay_create(h, E, M, L, 0, ONLINE_CAPACITY, &rb);
    if (rc == 0) rc = m3pc_episodes_reset(ep, 0, E, 0, 0, 0, stream);

    /* the rollout: per round the live environments observe and record; host rows are consumed before a call returns */
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
    /* what every environment showed after its last step: the next state of its last transition */
    for (int e = 0; e < E; ++e)
        for (int j = 0; j < S; ++j) final_obs[e * S + j] = toy_obs(e, LENGTHS[e], j);

    /* episodes in: values (discount 1/2), update_buffer and the online transitions, one launch, nothing through the host */
    int taken = 0, n_traj = 0, n_online = 0, lens[E];
    if (rc == 0) rc = m3pc_replay_push_episodes(rb, ep, 0, E, 0.5, 0, final_obs, 0, &taken, stream);
    if (rc == 0) rc = m3pc_replay_counts(rb, &n_traj, 0, &n_online);
    if (rc == 0) rc = m3pc_replay_path_lengths(rb, lens, E);
    if (rc != 0) {
        fprintf(stderr, "replay_loop: %d: %s\n", rc, m3pc_last_error());
        return 1;
    }
    printf("taken %d trajectories %d online %d lengths", taken, n_traj, n_online);
    for (int i = 0; i < n_traj; ++i) printf(" %d", lens[i]);
    printf("\n");

    /* batches out: device arrays a training loop on the same GPU would read in place */
    float *states, *actions, *rewards, *ts, *ta, *tr, *ts2, *td;
    double* returns;
    int *seg_traj, *seg_start, *trans_index;
    HIP_OK(hipMalloc((void**)&states, sizeof(float) * B_SEG * L * S));
    HIP_OK(hipMalloc((void**)&actions, sizeof(float) * B_SEG * L * A));
    HIP_OK(hipMalloc((void**)&rewards, sizeof(float) * B_SEG * L));
    HIP_OK(hipMalloc((void**)&returns, sizeof(double) * B_SEG * L));
    HIP_OK(hipMalloc((void**)&seg_traj, sizeof(int) * B_SEG));
    HIP_OK(hipMalloc((void**)&seg_start, sizeof(int) * B_SEG));
    HIP_OK(hipMalloc((void**)&ts, sizeof(float) * B_TRANS * S));
    HIP_OK(hipMalloc((void**)&ta, sizeof(float) * B_TRANS * A));
    HIP_OK(hipMalloc((void**)&tr, sizeof(float) * B_TRANS));
    HIP_OK(hipMalloc((void**)&ts2, sizeof(float) * B_TRANS * S));
    HIP_OK(hipMalloc((void**)&td, sizeof(float) * B_TRANS));
    HIP_OK(hipMalloc((void**)&trans_index, sizeof(int) * B_TRANS));
    const unsigned long long seed = 7;
    rc = m3pc_replay_sample_segments(rb, B_SEG, M3PC_REPLAY_LENGTH, 0, 0, 0, seed, 0, states, actions, rewards, returns, 0, seg_traj, seg_start,
                                     stream);
    if (rc == 0) /* all rows from the online ring: n_online == batch */
        rc = m3pc_replay_sample_transitions(rb, B_TRANS, B_TRANS, 0, 0, seed, 1, ts, ta, tr, ts2, td, trans_index, stream);
    if (rc != 0) {
        fprintf(stderr, "replay_loop: %d: %s\n", rc, m3pc_last_error());
        return 1;
    }
    static float hs[B_SEG * L * S], ha[B_SEG * L * A], hr[B_SEG * L], hts[B_TRANS * S], hta[B_TRANS * A], htr[B_TRANS], hts2[B_TRANS * S],
        htd[B_TRANS];
    static double hv[B_SEG * L];
    static int hi[B_SEG], hk[B_SEG], hx[B_TRANS];
    HIP_OK(hipMemcpyAsync(hs, states, sizeof(hs), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(ha, actions, sizeof(ha), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(hr, rewards, sizeof(hr), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(hv, returns, sizeof(hv), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(hi, seg_traj, sizeof(hi), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(hk, seg_start, sizeof(hk), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(hts, ts, sizeof(hts), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(hta, ta, sizeof(hta), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(htr, tr, sizeof(htr), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(hts2, ts2, sizeof(hts2), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(htd, td, sizeof(htd), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(hx, trans_index, sizeof(hx), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    printf("segment index");
    for (int j = 0; j < B_SEG; ++j) printf(" %d:%d", hi[j], hk[j]);
    printf("\nsegments %.17g %.17g %.17g %.17g\n", checksum_f(hs, B_SEG * L * S), checksum_f(ha, B_SEG * L * A), checksum_f(hr, B_SEG * L),
           checksum_d(hv, B_SEG * L));
    printf("transition index");
    for (int j = 0; j < B_TRANS; ++j) printf(" %d", hx[j]);
    printf("\ntransitions %.17g %.17g %.17g %.17g %.17g\n", checksum_f(hts, B_TRANS * S), checksum_f(hta, B_TRANS * A), checksum_f(htr, B_TRANS),
           checksum_f(hts2, B_TRANS * S), checksum_f(htd, B_TRANS));

    /* the destroys drain the device before they free */
    m3pc_replay_destroy(rb);
    m3pc_episodes_destroy(ep);
    m3pc_destroy(h);
    void* bufs[] = {states, actions, rewards, returns, seg_traj, seg_start, ts, ta, tr, ts2, td, trans_index};
    for (size_t i = 0; i < sizeof(bufs) / sizeof(bufs[0]); ++i) (void)hipFree(bufs[i]);
    (void)hipStreamDestroy(stream);
    return 0;
}
