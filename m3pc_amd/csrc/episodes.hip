// The episode store (include/m3pc_hip.h: m3pc_episodes_*): the rollout histories of n_envs environments on the device and the
// assembly of the (T,S) / (T,A) / (T,1) windows of action_sample (finetune_omtm/learner.py:342-366) and action_piid_sample
// (zeroshot_omtm/learner.py:164-223) there.  The kernels are memory-bound gathers and scatters over a flat element index
// (consecutive lanes take consecutive features of a row: coalesced for any row width, no alignment assumed), without atomics;
// the one reduction (values) is a serial fp64 recurrence per environment: every result is bit-identical from run to run.
// The host half keeps a mirror of the path lengths -- the host makes every call that changes one -- so that no call reads the device.
#include "episodes.h"

namespace m3pc {
namespace {

struct EpisodesP {
    float *obs, *act, *rew;  // (n_envs, M, S) (n_envs, M, A) (n_envs, M)
    int* len;                // (n_envs,) path lengths
    const int* ids;          // (n,) environments of the call, or nullptr: 0 .. n-1
    int n, S, A, T, M;
};

constexpr int EP_THREADS = 256;

__device__ __forceinline__ int env_of(const EpisodesP& p, int i) { return p.ids ? p.ids[i] : i; }

// obs[e, len[e], :] = row i of src (fp64 rows are rounded to nearest even, as NumPy's assignment into a float32 array rounds)
template <typename In>
__global__ __launch_bounds__(EP_THREADS) void ep_observe_kernel(EpisodesP p, const In* src) {
    const long long total = (long long)p.n * p.S;
    for (long long x = (long long)blockIdx.x * EP_THREADS + threadIdx.x; x < total; x += (long long)gridDim.x * EP_THREADS) {
        const int i = (int)(x / p.S), j = (int)(x - (long long)i * p.S);
        const int e = env_of(p, i), pos = p.len[e];
        if (pos < p.M) p.obs[((size_t)e * p.M + pos) * p.S + j] = (float)src[x];
    }
}

// act[e, len[e], :] = clip(a), rew[e, len[e]] = r, len[e] += 1.  One wavefront per environment: its lanes take the A + 1 values of
// the row; every path length of the block is read in front of the barrier and advanced behind it.
// The clip: (a < lo ? lo : a), then (v > hi ? hi : v) -- np.clip's bits, NaN and the sign of a zero included.
__global__ __launch_bounds__(EP_THREADS) void ep_record_kernel(EpisodesP p, const float* actions, const float* rewards, float lo, float hi) {
    const int i = blockIdx.x * (EP_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    int e = 0, pos = p.M;
    if (i < p.n) {
        e = env_of(p, i);
        pos = p.len[e];
    }
    __syncthreads();
    if (pos >= p.M) return;  // (a full episode is refused on the host: never an out-of-range store)
    const size_t row = (size_t)e * p.M + pos;
    for (int j = lane; j <= p.A; j += 64) {
        if (j < p.A) {
            const float a = actions[(size_t)i * p.A + j];
            float v = a < lo ? lo : a;
            v = v > hi ? hi : v;
            p.act[row * p.A + j] = v;
        } else {
            p.rew[row] = rewards[i];
        }
    }
    if (lane == 0) p.len[e] = pos + 1;
}

// the three blocks of every listed environment zeroed (the observation block: rows of the environment's table, when one is given),
// its path length 0
template <typename In>
__global__ __launch_bounds__(EP_THREADS) void ep_reset_kernel(EpisodesP p, const In* table) {
    const long long W = p.S + p.A + 1, per = (long long)p.M * W, total = (long long)p.n * per;
    const long long no = (long long)p.M * p.S, na = (long long)p.M * p.A;
    for (long long x = (long long)blockIdx.x * EP_THREADS + threadIdx.x; x < total; x += (long long)gridDim.x * EP_THREADS) {
        const int i = (int)(x / per);
        const long long r = x - (long long)i * per;
        const size_t e = (size_t)env_of(p, i);
        if (r < no) p.obs[e * no + r] = table ? (float)table[(size_t)i * no + r] : 0.f;
        else if (r < no + na) p.act[e * na + (r - no)] = 0.f;
        else p.rew[e * p.M + (r - no - na)] = 0.f;
        if (r == 0) p.len[e] = 0;
    }
}

// The window of environment e at end = len[e], for the horizon H (learner.py:342-366):
//   h = H if end + H >= T else T - end;  hl = T - h + 1;  lo = end - hl + 1
//   rows t < hl of the three keys = store rows lo + t (row `end` of act / rew is what the store holds there), rows t >= hl zero.
// goal != 0 (zeroshot_omtm/learner.py:164-223): states[t] = obs[lo + t] for t < smart = T - max(0, end + h - M), zero behind.
__global__ __launch_bounds__(EP_THREADS) void ep_windows_kernel(EpisodesP p, int H, int goal, float* states, float* actions, float* rewards) {
    const long long W = p.S + p.A + 1, total = (long long)p.n * p.T * W;
    for (long long x = (long long)blockIdx.x * EP_THREADS + threadIdx.x; x < total; x += (long long)gridDim.x * EP_THREADS) {
        const long long it = x / W;
        const int c = (int)(x - it * W), i = (int)(it / p.T), t = (int)(it - (long long)i * p.T);
        const int e = env_of(p, i), end = p.len[e];
        const int h = end + H >= p.T ? H : p.T - end, hl = p.T - h + 1, lo = end - hl + 1;
        const int over = end + h - p.M, smart = p.T - (over > 0 ? over : 0);
        const int src = lo + t;
        const bool in = src >= 0 && src < p.M;  // (always, for end < M; a full episode is refused on the host)
        const size_t row = (size_t)e * p.M + (in ? src : 0);
        if (c < p.S) states[(size_t)it * p.S + c] = in && t < (goal ? smart : hl) ? p.obs[row * p.S + c] : 0.f;
        else if (c < p.S + p.A) actions[(size_t)it * p.A + (c - p.S)] = in && t < hl ? p.act[row * p.A + (c - p.S)] : 0.f;
        else rewards[it] = in && t < hl ? p.rew[row] : 0.f;
    }
}

// replay_buffer.py:234-243.  V[t] = sum_j rew[t+1+j] gamma^j as the reverse recurrence V[t] = rew[t+1] + gamma V[t+1] in fp64 (product and
// sum rounded separately: the library is built with -ffp-contract=off), stored as fp32; use_avg: fp32(fp64(fp32 V[t]) / (M - t)).
// One thread per environment.
__global__ __launch_bounds__(EP_THREADS) void ep_values_kernel(EpisodesP p, double gamma, int use_avg, float* out) {
    const int i = blockIdx.x * EP_THREADS + threadIdx.x;
    if (i >= p.n) return;
    const float* rew = p.rew + (size_t)env_of(p, i) * p.M;
    float* o = out + (size_t)i * p.M;
    double v = 0.0;
    o[p.M - 1] = 0.f;
    for (int t = p.M - 2; t >= 0; --t) {
        v = (double)rew[t + 1] + gamma * v;
        float f = (float)v;
        if (use_avg) f = (float)((double)f / (double)(p.M - t));
        o[t] = f;
    }
}

int blocks_for(long long total) {
    const long long b = (total + EP_THREADS - 1) / EP_THREADS;
    return (int)(b < 1 ? 1 : (b > (1 << 20) ? (1 << 20) : b));
}

}  // namespace
}  // namespace m3pc

namespace {

int ep_ensure(m3pc_episodes* ep, hipStream_t st) {
    HIPCHK(hipSetDevice(ep->device));
    if (ep->ready) return 0;
    const size_t rows = (size_t)ep->n_envs * ep->M;
    CHK(dmalloc(&ep->obs, rows * ep->S));
    CHK(dmalloc(&ep->act, rows * ep->A));
    CHK(dmalloc(&ep->rew, rows));
    CHK(dmalloc(&ep->len, (size_t)ep->n_envs));
    HIPCHK(hipMemsetAsync(ep->obs, 0, rows * ep->S * sizeof(float), st));
    HIPCHK(hipMemsetAsync(ep->act, 0, rows * ep->A * sizeof(float), st));
    HIPCHK(hipMemsetAsync(ep->rew, 0, rows * sizeof(float), st));
    HIPCHK(hipMemsetAsync(ep->len, 0, (size_t)ep->n_envs * sizeof(int), st));
    ep->ready = true;
    return 0;
}

int ep_stage(m3pc_episodes* ep, const void* src, size_t bytes, const void** dev) { return ep->pool.stage(src, bytes, dev, "m3pc_episodes"); }

// behind the launch that reads them: the call's blocks become free again when `st` has passed this point
int ep_release(m3pc_episodes* ep, hipStream_t st) { return ep->pool.release(st); }

// the ids of one call: n in [1, n_envs], every id in [0, n_envs), none twice.  Before any HIP call.
int ep_check_ids(m3pc_episodes* ep, const int* ids, int n, const char* who) {
    if (n < 1 || n > ep->n_envs) return fail(M3PC_EINVAL, "%s: n %d outside [1, n_envs=%d]", who, n, ep->n_envs);
    if (!ids) return 0;
    if (++ep->call == 0) {
        std::fill(ep->seen.begin(), ep->seen.end(), 0u);
        ep->call = 1;
    }
    for (int i = 0; i < n; ++i) {
        if (ids[i] < 0 || ids[i] >= ep->n_envs) return fail(M3PC_EINVAL, "%s: env_ids[%d] = %d outside [0, n_envs=%d)", who, i, ids[i], ep->n_envs);
        if (ep->seen[ids[i]] == ep->call) return fail(M3PC_EINVAL, "%s: env_ids[%d] = %d is repeated within the call", who, i, ids[i]);
        ep->seen[ids[i]] = ep->call;
    }
    return 0;
}

int ep_check_room(const m3pc_episodes* ep, const int* ids, int n, const char* who) {
    for (int i = 0; i < n; ++i) {
        const int e = ids ? ids[i] : i;
        if (ep->mirror[e] >= ep->M)
            return fail(M3PC_ESTATE, "%s: the episode of environment %d is full (path_length == max_steps = %d)", who, e, ep->M);
    }
    return 0;
}

int ep_params(m3pc_episodes* ep, const int* ids, int n, EpisodesP* p) {
    p->obs = ep->obs;
    p->act = ep->act;
    p->rew = ep->rew;
    p->len = ep->len;
    p->ids = nullptr;
    p->n = n;
    p->S = ep->S;
    p->A = ep->A;
    p->T = ep->T;
    p->M = ep->M;
    if (ids) {
        const void* d = nullptr;
        CHK(ep_stage(ep, ids, (size_t)n * sizeof(int), &d));
        p->ids = (const int*)d;
    }
    return 0;
}

int ep_finish(m3pc_episodes* ep, hipStream_t st, const char* what) {
    const int rc = check_launch(what);
    const int rr = ep_release(ep, st);
    return rc ? rc : rr;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int m3pc_episodes_create(m3pc_handle* h, int n_envs, int max_steps, m3pc_episodes** out) {
    if (!h || !out) return fail(M3PC_EINVAL, "null argument");
    if (n_envs < 1) return fail(M3PC_EINVAL, "m3pc_episodes_create: n_envs %d < 1", n_envs);
    // (the sizes the handle was created with: its m3pc_dims)
    const int T = h->dm.traj_length, S = h->dm.state_dim, A = h->dm.action_dim;
    if (max_steps < T) return fail(M3PC_EINVAL, "m3pc_episodes_create: max_steps %d < T = %d", max_steps, T);
    if (T < 1 || S < 1 || A < 1) return fail(M3PC_EINVAL, "m3pc_episodes_create: the handle has no sizes");
    if ((long long)n_envs * max_steps > (1LL << 31) - 1)
        return fail(M3PC_EINVAL, "m3pc_episodes_create: n_envs * max_steps = %lld rows > 2^31 - 1", (long long)n_envs * max_steps);
    m3pc_episodes* ep = new m3pc_episodes();
    ep->device = h->device;
    ep->S = S;
    ep->A = A;
    ep->T = T;
    ep->n_envs = n_envs;
    ep->M = max_steps;
    ep->mirror.assign((size_t)n_envs, 0);
    ep->seen.assign((size_t)n_envs, 0u);
    *out = ep;
    return 0;
}

int m3pc_episodes_destroy(m3pc_episodes* ep) {
    if (!ep) return 0;
    if (ep->ready || !ep->pool.stages.empty()) {
        (void)hipSetDevice(ep->device);
        (void)hipDeviceSynchronize();
        for (void* b : {(void*)ep->obs, (void*)ep->act, (void*)ep->rew, (void*)ep->len})
            if (b) (void)hipFree(b);
        ep->pool.destroy();
    }
    delete ep;
    return 0;
}

int m3pc_episodes_reset(m3pc_episodes* ep, const int* env_ids, int n, const void* obs_table, int table_f64, int on_device, void* stream) {
    if (!ep) return fail(M3PC_EINVAL, "null argument");
    CHK(ep_check_ids(ep, env_ids, n, "m3pc_episodes_reset"));
    hipStream_t st = (hipStream_t)stream;
    CHK(ep_ensure(ep, st));
    EpisodesP p;
    int rc = ep_params(ep, env_ids, n, &p);
    const void* tab = obs_table;
    if (!rc && obs_table && !on_device)
        rc = ep_stage(ep, obs_table, (size_t)n * ep->M * ep->S * (table_f64 ? sizeof(double) : sizeof(float)), &tab);
    if (rc) {
        ep->pool.held.clear();
        return rc;
    }
    const int blocks = blocks_for((long long)n * ep->M * (ep->S + ep->A + 1));
    if (table_f64) hipLaunchKernelGGL(ep_reset_kernel<double>, dim3(blocks), dim3(EP_THREADS), 0, st, p, (const double*)tab);
    else hipLaunchKernelGGL(ep_reset_kernel<float>, dim3(blocks), dim3(EP_THREADS), 0, st, p, (const float*)tab);
    CHK(ep_finish(ep, st, "episodes_reset"));
    for (int i = 0; i < n; ++i) ep->mirror[env_ids ? env_ids[i] : i] = 0;
    return 0;
}

int m3pc_episodes_observe(m3pc_episodes* ep, const int* env_ids, int n, const void* obs, int obs_f64, int on_device, void* stream) {
    if (!ep || !obs) return fail(M3PC_EINVAL, "null argument");
    CHK(ep_check_ids(ep, env_ids, n, "m3pc_episodes_observe"));
    CHK(ep_check_room(ep, env_ids, n, "m3pc_episodes_observe"));
    hipStream_t st = (hipStream_t)stream;
    CHK(ep_ensure(ep, st));
    EpisodesP p;
    int rc = ep_params(ep, env_ids, n, &p);
    const void* src = obs;
    if (!rc && !on_device) rc = ep_stage(ep, obs, (size_t)n * ep->S * (obs_f64 ? sizeof(double) : sizeof(float)), &src);
    if (rc) {
        ep->pool.held.clear();
        return rc;
    }
    const int blocks = blocks_for((long long)n * ep->S);
    if (obs_f64) hipLaunchKernelGGL(ep_observe_kernel<double>, dim3(blocks), dim3(EP_THREADS), 0, st, p, (const double*)src);
    else hipLaunchKernelGGL(ep_observe_kernel<float>, dim3(blocks), dim3(EP_THREADS), 0, st, p, (const float*)src);
    return ep_finish(ep, st, "episodes_observe");
}

int m3pc_episodes_record(m3pc_episodes* ep, const int* env_ids, int n, const float* actions, const float* rewards, float clip_min,
                         float clip_max, int on_device, void* stream) {
    if (!ep || !actions || !rewards) return fail(M3PC_EINVAL, "null argument");
    CHK(ep_check_ids(ep, env_ids, n, "m3pc_episodes_record"));
    if (!(clip_min <= clip_max)) return fail(M3PC_EINVAL, "m3pc_episodes_record: clip_min %g > clip_max %g (or one of them is NaN)", clip_min, clip_max);
    CHK(ep_check_room(ep, env_ids, n, "m3pc_episodes_record"));
    hipStream_t st = (hipStream_t)stream;
    CHK(ep_ensure(ep, st));
    EpisodesP p;
    int rc = ep_params(ep, env_ids, n, &p);
    const void *a = actions, *r = rewards;
    if (!rc && !on_device) rc = ep_stage(ep, actions, (size_t)n * ep->A * sizeof(float), &a);
    if (!rc && !on_device) rc = ep_stage(ep, rewards, (size_t)n * sizeof(float), &r);
    if (rc) {
        ep->pool.held.clear();
        return rc;
    }
    const int per = EP_THREADS / 64;
    hipLaunchKernelGGL(ep_record_kernel, dim3((n + per - 1) / per), dim3(EP_THREADS), 0, st, p, (const float*)a, (const float*)r, clip_min, clip_max);
    CHK(ep_finish(ep, st, "episodes_record"));
    for (int i = 0; i < n; ++i) ep->mirror[env_ids ? env_ids[i] : i] += 1;
    return 0;
}

int m3pc_episodes_windows(m3pc_episodes* ep, const int* env_ids, int n, int mode, int horizon, float* states, float* actions, float* rewards,
                          int* horizons, void* stream) {
    if (!ep || !states || !actions || !rewards) return fail(M3PC_EINVAL, "null argument");
    CHK(ep_check_ids(ep, env_ids, n, "m3pc_episodes_windows"));
    if (mode != M3PC_WINDOW_PLAN && mode != M3PC_WINDOW_GOAL)
        return fail(M3PC_EINVAL, "m3pc_episodes_windows: mode %d is neither M3PC_WINDOW_PLAN nor M3PC_WINDOW_GOAL", mode);
    if (horizon < 1 || horizon > ep->T) return fail(M3PC_EINVAL, "m3pc_episodes_windows: horizon %d outside [1, T=%d]", horizon, ep->T);
    CHK(ep_check_room(ep, env_ids, n, "m3pc_episodes_windows"));  // (the window's last history row is row path_length)
    hipStream_t st = (hipStream_t)stream;
    CHK(ep_ensure(ep, st));
    EpisodesP p;
    if (int rc = ep_params(ep, env_ids, n, &p)) {
        ep->pool.held.clear();
        return rc;
    }
    hipLaunchKernelGGL(ep_windows_kernel, dim3(blocks_for((long long)n * ep->T * (ep->S + ep->A + 1))), dim3(EP_THREADS), 0, st, p, horizon,
                       mode == M3PC_WINDOW_GOAL ? 1 : 0, states, actions, rewards);
    CHK(ep_finish(ep, st, "episodes_windows"));
    if (horizons)
        for (int i = 0; i < n; ++i) {
            const int end = ep->mirror[env_ids ? env_ids[i] : i];
            horizons[i] = end + horizon >= ep->T ? horizon : ep->T - end;
        }
    return 0;
}

int m3pc_episodes_values(m3pc_episodes* ep, const int* env_ids, int n, double discount, int use_avg, float* values, void* stream) {
    if (!ep || !values) return fail(M3PC_EINVAL, "null argument");
    CHK(ep_check_ids(ep, env_ids, n, "m3pc_episodes_values"));
    if (!(discount >= 0.0 && discount <= 1.7976931348623157e308))
        return fail(M3PC_EINVAL, "m3pc_episodes_values: the discount must be finite and >= 0");
    hipStream_t st = (hipStream_t)stream;
    CHK(ep_ensure(ep, st));
    EpisodesP p;
    if (int rc = ep_params(ep, env_ids, n, &p)) {
        ep->pool.held.clear();
        return rc;
    }
    hipLaunchKernelGGL(ep_values_kernel, dim3((n + EP_THREADS - 1) / EP_THREADS), dim3(EP_THREADS), 0, st, p, discount, use_avg ? 1 : 0, values);
    return ep_finish(ep, st, "episodes_values");
}

int m3pc_episodes_export(m3pc_episodes* ep, int env, float* obs, float* act, float* rew, int* path_length, int on_device, void* stream) {
    if (!ep) return fail(M3PC_EINVAL, "null argument");
    if (env < 0 || env >= ep->n_envs) return fail(M3PC_EINVAL, "m3pc_episodes_export: env %d outside [0, n_envs=%d)", env, ep->n_envs);
    if (path_length) *path_length = ep->mirror[env];
    if (!obs && !act && !rew) return 0;
    hipStream_t st = (hipStream_t)stream;
    CHK(ep_ensure(ep, st));
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const size_t row0 = (size_t)env * ep->M;
    if (obs) HIPCHK(hipMemcpyAsync(obs, ep->obs + row0 * ep->S, (size_t)ep->M * ep->S * sizeof(float), kind, st));
    if (act) HIPCHK(hipMemcpyAsync(act, ep->act + row0 * ep->A, (size_t)ep->M * ep->A * sizeof(float), kind, st));
    if (rew) HIPCHK(hipMemcpyAsync(rew, ep->rew + row0, (size_t)ep->M * sizeof(float), kind, st));
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
