// The replay buffer (include/m3pc_hip.h: m3pc_replay_*): ReplayBuffer of finetune_omtm/replay_buffer.py on the device -- a ring of
// trajectories (update_buffer :272-310, traj_sample :312-366, values_up_bound :161 / :310) and two rings of transitions (the deques of
// :101-102, trans_sample :368-420) -- filled from caller arrays or straight from an episode store (episodes.hip).  The kernels are
// memory-bound gathers and scatters (consecutive lanes take consecutive features of a row: coalesced for any row width, no alignment
// assumed), without atomics; the reductions (the value recurrence, the scan of the path lengths, the column maximum) run in a fixed
// order: every result is bit-identical from run to run.  The library's index draws are exact integer arithmetic on Philox words
// (philox.h), so tests/replay_ref.py restates them bit for bit.  The host half mirrors counts, ring heads and path lengths -- the host
// makes every call that changes one -- so that no call reads the device.
#include "episodes.h"
#include "mtm_loss.h"
#include "philox.h"

namespace m3pc {
namespace {

constexpr int RB_THREADS = 256;
constexpr uint32_t RB_ARRAY_SEGMENTS = 2, RB_ARRAY_ONLINE = 3, RB_ARRAY_OFFLINE = 4;  // the `array` word of the Philox counter

// the trajectory ring: logical index i (0 = oldest) is physical slot (head + i) % C
struct TrajP {
    float *obs, *act, *rew;  // (C, M, S) (C, M, A) (C, M)
    double* val;             // (C, M)
    int* len;                // (C,)
    long long* cum;          // (C + 1,) exclusive scan of the path lengths in logical order
    int C, M, L, S, A, head, count;
};
// one transition ring
struct RingP {
    float *s, *a, *r, *s2, *d;  // (cap, S) (cap, A) (cap,) (cap, S) (cap,)
    int cap, head, count;
};
// one episode of m3pc_replay_push_episodes, made on the host from the mirrors
struct PushD {
    int env, slot, len, nt;  // store environment; physical trajectory slot or -1; path length; transitions of the episode
    long long q;             // the position of its first transition among the call's
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// n trajectories from caller arrays into the slots (slot0 + i) % C
__global__ __launch_bounds__(RB_THREADS) void rb_append_traj_kernel(TrajP p, int n, int slot0, const float* obs, const float* act, const float* rew,
                                                                    const double* val, const int* lens) {
    const long long no = (long long)p.M * p.S, na = (long long)p.M * p.A, per = no + na + 2LL * p.M, total = (long long)n * per;
    for (long long x = (long long)blockIdx.x * RB_THREADS + threadIdx.x; x < total; x += (long long)gridDim.x * RB_THREADS) {
        const int i = (int)(x / per);
        const long long r = x - (long long)i * per;
        const size_t slot = (size_t)((slot0 + i) % p.C);
        if (r < no) p.obs[slot * no + r] = obs[(size_t)i * no + r];
        else if (r < no + na) p.act[slot * na + (r - no)] = act[(size_t)i * na + (r - no)];
        else if (r < no + na + p.M) p.rew[slot * p.M + (r - no - na)] = rew[(size_t)i * p.M + (r - no - na)];
        else p.val[slot * p.M + (r - no - na - p.M)] = val[(size_t)i * p.M + (r - no - na - p.M)];
        if (r == 0) p.len[slot] = lens[i];
    }
}

// n transitions from caller arrays into the slots (slot0 + i) % cap
__global__ __launch_bounds__(RB_THREADS) void rb_append_trans_kernel(RingP g, int S, int A, int n, int slot0, const float* s, const float* a,
                                                                     const float* r, const float* s2, const float* d) {
    const int W = 2 * S + A + 2;
    const long long total = (long long)n * W;
    for (long long x = (long long)blockIdx.x * RB_THREADS + threadIdx.x; x < total; x += (long long)gridDim.x * RB_THREADS) {
        const int i = (int)(x / W), c = (int)(x - (long long)i * W);
        const size_t dst = (size_t)(((long long)slot0 + i) % g.cap);
        if (c < S) g.s[dst * S + c] = s[(size_t)i * S + c];
        else if (c < S + A) g.a[dst * A + (c - S)] = a[(size_t)i * A + (c - S)];
        else if (c == S + A) g.r[dst] = r[i];
        else if (c < 2 * S + A + 1) g.s2[dst * S + (c - S - A - 1)] = s2[(size_t)i * S + (c - S - A - 1)];
        else g.d[dst] = d[i];
    }
}

// Episodes of a store into the buffer, one launch.  Blocks [0, vblocks): one wavefront per episode runs the value recurrence of
// ep_values_kernel (episodes.hip; replay_buffer.py:234-243): V[t] = rew[t+1] + gamma V[t+1] in fp64, rounded to fp32, widened; use_avg:
// (double)(float)V[t] / (M - t), NOT rounded again (float32 array / int64 array is float64 in NumPy, :240-242).  The other blocks: a flat
// index over (episode, row, column), the columns of a row being the S + A + 1 trajectory features and the 2S + A + 2 features of the
// transition (obs[t], act[t], rew[t], obs[t+1] or final_obs, 0).  A transition whose position among the call's is below keep_from has
// already left the ring again when the call is over and is not written: no two threads store to one address.
__global__ __launch_bounds__(RB_THREADS) void rb_push_kernel(TrajP p, RingP on, const float* eobs, const float* eact, const float* erew, int n,
                                                             int vblocks, double gamma, int use_avg, const float* final_obs, long long keep_from,
                                                             int tslot0, const PushD* desc) {
    if ((int)blockIdx.x < vblocks) {
        const int i = blockIdx.x * (RB_THREADS / 64) + (threadIdx.x >> 6);
        if (i >= n || (threadIdx.x & 63) != 0) return;
        const PushD d = desc[i];
        if (d.slot < 0) return;
        const float* rew = erew + (size_t)d.env * p.M;
        double* o = p.val + (size_t)d.slot * p.M;
        double v = 0.0;
        o[p.M - 1] = 0.0;
        for (int t = p.M - 2; t >= 0; --t) {
            v = (double)rew[t + 1] + gamma * v;
            const double f = (double)(float)v;
            o[t] = use_avg ? f / (double)(p.M - t) : f;
        }
        return;
    }
    const int Wt = p.S + p.A + 1, W = Wt + 2 * p.S + p.A + 2;
    const long long per = (long long)p.M * W, total = (long long)n * per;
    const long long stride = (long long)(gridDim.x - vblocks) * RB_THREADS;
    for (long long x = (long long)(blockIdx.x - vblocks) * RB_THREADS + threadIdx.x; x < total; x += stride) {
        const int i = (int)(x / per);
        const long long rem = x - (long long)i * per;
        const int t = (int)(rem / W), c = (int)(rem - (long long)t * W);
        const PushD d = desc[i];
        const size_t src = (size_t)d.env * p.M + t;
        if (c < Wt) {
            if (d.slot < 0) continue;
            const size_t dst = (size_t)d.slot * p.M + t;
            if (c < p.S) p.obs[dst * p.S + c] = eobs[src * p.S + c];
            else if (c < p.S + p.A) p.act[dst * p.A + (c - p.S)] = eact[src * p.A + (c - p.S)];
            else {
                p.rew[dst] = erew[src];
                if (t == 0) p.len[d.slot] = d.len;
            }
            continue;
        }
        if (t >= d.nt || d.q + t < keep_from) continue;
        const int k = c - Wt;
        const size_t dst = (size_t)(((long long)tslot0 + d.q + t) % on.cap);
        if (k < p.S) on.s[dst * p.S + k] = eobs[src * p.S + k];
        else if (k < p.S + p.A) on.a[dst * p.A + (k - p.S)] = eact[src * p.A + (k - p.S)];
        else if (k == p.S + p.A) on.r[dst] = erew[src];
        else if (k < 2 * p.S + p.A + 1) {
            const int f = k - p.S - p.A - 1;
            // (t + 1 < len <= M wherever the store's row is read: without final_obs the episode has len - 1 transitions)
            on.s2[dst * p.S + f] = (t == d.len - 1) ? final_obs[(size_t)i * p.S + f] : eobs[(src + 1) * p.S + f];
        } else on.d[dst] = 0.f;
    }
}

// cum[i] = sum of the path lengths of the logical entries < i, i = 0 .. count, int64.  One wavefront: lane l sums the entries
// [l chunk, (l+1) chunk) serially, the 64 partial sums are scanned across the lanes, then every lane writes its chunk -- a fixed order.
__global__ __launch_bounds__(64) void rb_scan_kernel(TrajP p) {
    const int lane = threadIdx.x, chunk = (p.count + 63) / 64;
    const int lo = lane * chunk < p.count ? lane * chunk : p.count, hi = lo + chunk < p.count ? lo + chunk : p.count;
    long long s = 0;
    for (int k = lo; k < hi; ++k) s += p.len[(p.head + k) % p.C];
    long long inc = s;
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    long long run = inc - s;
    for (int k = lo; k < hi; ++k) {
        p.cum[k] = run;
        run += p.len[(p.head + k) % p.C];
    }
    if (lane == 63) p.cum[p.count] = inc;
}

// A batch of segments, all four keys in one launch; one wavefront per row j.  The (trajectory, start) of the row is the caller's
// (clamped into range: a device index the host cannot check never leads out of the storage) or drawn here from the Philox block j of
// (seed, step), array 2 (the header states the rule).  A segment is L consecutive rows of one trajectory: contiguous in every key.
__global__ __launch_bounds__(RB_THREADS) void rb_segments_kernel(TrajP p, int B, int mode, const int* traj, const int* starts, uint32_t k0,
                                                                 uint32_t k1, uint32_t s0, uint32_t s1, float* states, float* actions,
                                                                 float* rewards, void* returns, int returns_f32, int* out_traj, int* out_start) {
    const int j = blockIdx.x * (RB_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= B) return;
    int i, start = 0;
    uint32_t w[4] = {0, 0, 0, 0};
    if (traj) {
        i = clampi(traj[j], 0, p.count - 1);
    } else {
        philox4x32_10((uint32_t)j, s0, s1, RB_ARRAY_SEGMENTS, k0, k1, w);
        if (mode == M3PC_REPLAY_UNIFORM) {
            i = (int)(((unsigned long long)w[0] * (unsigned long long)p.count) >> 32);
        } else {
            const long long r = (long long)(((unsigned long long)w[0] * (unsigned long long)p.cum[p.count]) >> 32);
            int lo = 0, hi = p.count;  // cum[lo] <= r < cum[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (p.cum[mid] <= r) lo = mid;
                else hi = mid;
            }
            i = lo;
        }
    }
    const size_t slot = (size_t)((p.head + i) % p.C);
    const int len = p.len[slot];
    if (traj) start = clampi(starts[j], 0, len - p.L);
    else start = (int)(((unsigned long long)w[2] * (unsigned long long)(len - p.L + 1)) >> 32);
    const size_t row0 = slot * p.M + start, out0 = (size_t)j * p.L;
    const int ns = p.L * p.S, na = p.L * p.A, total = ns + na + 2 * p.L;
    for (int x = lane; x < total; x += 64) {
        if (x < ns) states[out0 * p.S + x] = p.obs[row0 * p.S + x];
        else if (x < ns + na) actions[out0 * p.A + (x - ns)] = p.act[row0 * p.A + (x - ns)];
        else if (x < ns + na + p.L) rewards[out0 + (x - ns - na)] = p.rew[row0 + (x - ns - na)];
        else {
            const int t = x - ns - na - p.L;
            const double v = p.val[row0 + t];
            if (returns_f32) ((float*)returns)[out0 + t] = (float)v;
            else ((double*)returns)[out0 + t] = v;
        }
    }
    if (lane == 0) {
        if (out_traj) out_traj[j] = i;
        if (out_start) out_start[j] = start;
    }
}

// The keyed bijection of [0, n) behind the library's distinct transition indices (the header defines it): a 4-round balanced Feistel
// network on 2 half bits, cycle-walked into [0, n).
__device__ __forceinline__ uint32_t rb_pi(uint32_t j, uint32_t n, const uint32_t key[4]) {
    if (n <= 1u) return 0u;
    const int bits = 32 - __clz((int)(n - 1u)), half = (bits + 1) >> 1;
    const uint32_t mask = (1u << half) - 1u;
    uint32_t x = j;
    do {
        uint32_t l = x >> half, r = x & mask;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t f = ((r + key[k]) * 0x9E3779B1u) >> (32 - half);
            const uint32_t t = l ^ f;
            l = r;
            r = t;
        }
        x = (l << half) | r;
    } while (x >= n);
    return x;
}

// A batch of transitions, all five keys in one launch: rows [0, n_on) from the online ring, the rest from the offline ring.
__global__ __launch_bounds__(RB_THREADS) void rb_transitions_kernel(RingP on, RingP off, int S, int A, int B, int n_on, const int* given, uint32_t k0,
                                                                    uint32_t k1, uint32_t s0, uint32_t s1, float* state, float* action, float* reward,
                                                                    float* next_state, float* done, int* out_idx) {
    const int W = 2 * S + A + 2;
    const long long total = (long long)B * W;
    for (long long x = (long long)blockIdx.x * RB_THREADS + threadIdx.x; x < total; x += (long long)gridDim.x * RB_THREADS) {
        const int j = (int)(x / W), c = (int)(x - (long long)j * W);
        const bool online = j < n_on;
        const RingP& g = online ? on : off;
        int idx;
        if (given) {
            idx = clampi(given[j], 0, g.count - 1);
        } else {
            uint32_t key[4];
            philox4x32_10(0u, s0, s1, online ? RB_ARRAY_ONLINE : RB_ARRAY_OFFLINE, k0, k1, key);
            idx = (int)rb_pi((uint32_t)(online ? j : j - n_on), (uint32_t)g.count, key);
        }
        const size_t src = (size_t)(((long long)g.head + idx) % g.cap);
        if (c < S) state[(size_t)j * S + c] = g.s[src * S + c];
        else if (c < S + A) action[(size_t)j * A + (c - S)] = g.a[src * A + (c - S)];
        else if (c == S + A) reward[j] = g.r[src];
        else if (c < 2 * S + A + 1) next_state[(size_t)j * S + (c - S - A - 1)] = g.s2[src * S + (c - S - A - 1)];
        else done[j] = g.d[src];
        if (c == 0 && out_idx) out_idx[j] = idx;
    }
}

// out[t] = max over the held trajectories, in logical order, of val[., t]; a NaN stays (numpy.max)
__global__ __launch_bounds__(RB_THREADS) void rb_upbound_kernel(TrajP p, double* out) {
    const int t = blockIdx.x * RB_THREADS + threadIdx.x;
    if (t >= p.M) return;
    double m = p.val[(size_t)p.head * p.M + t];
    for (int i = 1; i < p.count; ++i) {
        const double v = p.val[(size_t)((p.head + i) % p.C) * p.M + t];
        m = (v > m || v != v) ? v : m;
    }
    out[t] = m;
}

int rb_blocks(long long total) {
    const long long b = (total + RB_THREADS - 1) / RB_THREADS;
    return (int)(b < 1 ? 1 : (b > (1 << 20) ? (1 << 20) : b));
}

}  // namespace
}  // namespace m3pc

// One buffer.  Device storage is allocated by the first call that enqueues work: m3pc_replay_create itself makes no HIP call.
struct m3pc_replay {
    int device = 0, S = 0, A = 0, C = 0, M = 0, L = 0;
    float *obs = nullptr, *act = nullptr, *rew = nullptr;
    double* val = nullptr;
    int* len = nullptr;
    long long* cum = nullptr;
    int head = 0, count = 0;
    std::vector<int> lens;  // path lengths by physical slot, as the calls made so far leave them
    bool cum_valid = false; // the device's scan is that of the ring as it stands
    struct Ring {
        float *s = nullptr, *a = nullptr, *r = nullptr, *s2 = nullptr, *d = nullptr;
        int cap = 0, head = 0, count = 0;
    } ring[2];              // M3PC_REPLAY_OFFLINE, M3PC_REPLAY_ONLINE
    bool ready = false;
    m3pc::StagePool pool;
};

namespace m3pc {
// (iql.h) what the trainer checks a buffer against
void replay_sizes(const m3pc_replay* rb, int* S, int* A, int* device) {
    *S = rb->S;
    *A = rb->A;
    *device = rb->device;
}
// (mtm_loss.h)
int replay_segment_length(const m3pc_replay* rb) { return rb->L; }
int replay_check_segments(m3pc_replay* rb, int batch, int mode, const int* traj_index, const int* start_index, int index_on_device,
                          const char* who) {
    if ((traj_index == nullptr) != (start_index == nullptr))
        return fail(M3PC_EINVAL, "%s: traj_index and start_index come together (one of them is null)", who);
    if (batch < 1) return fail(M3PC_EINVAL, "%s: batch %d < 1", who, batch);
    if (mode != M3PC_REPLAY_UNIFORM && mode != M3PC_REPLAY_LENGTH)
        return fail(M3PC_EINVAL, "%s: mode %d is neither M3PC_REPLAY_UNIFORM nor M3PC_REPLAY_LENGTH", who, mode);
    if (rb->count == 0) return fail(M3PC_ESTATE, "%s: the buffer holds no trajectory", who);
    if (traj_index && !index_on_device)
        for (int j = 0; j < batch; ++j) {
            if (traj_index[j] < 0 || traj_index[j] >= rb->count)
                return fail(M3PC_EINVAL, "%s: traj_index[%d] = %d outside [0, count=%d)", who, j, traj_index[j], rb->count);
            const int len = rb->lens[(size_t)((rb->head + traj_index[j]) % rb->C)];
            if (start_index[j] < 0 || start_index[j] > len - rb->L)
                return fail(M3PC_EINVAL, "%s: start_index[%d] = %d outside [0, path_length - segment_length = %d]", who, j, start_index[j],
                            len - rb->L);
        }
    return 0;
}
}  // namespace m3pc

namespace {

int rb_ensure(m3pc_replay* rb) {
    HIPCHK(hipSetDevice(rb->device));
    if (rb->ready) return 0;
    if (rb->C > 0) {
        const size_t rows = (size_t)rb->C * rb->M;
        CHK(dmalloc(&rb->obs, rows * rb->S));
        CHK(dmalloc(&rb->act, rows * rb->A));
        CHK(dmalloc(&rb->rew, rows));
        CHK(dmalloc(&rb->val, rows));
        CHK(dmalloc(&rb->len, (size_t)rb->C));
        CHK(dmalloc(&rb->cum, (size_t)rb->C + 1));
    }
    for (auto& g : rb->ring) {
        if (g.cap <= 0) continue;
        CHK(dmalloc(&g.s, (size_t)g.cap * rb->S));
        CHK(dmalloc(&g.a, (size_t)g.cap * rb->A));
        CHK(dmalloc(&g.r, (size_t)g.cap));
        CHK(dmalloc(&g.s2, (size_t)g.cap * rb->S));
        CHK(dmalloc(&g.d, (size_t)g.cap));
    }
    rb->ready = true;
    return 0;
}

TrajP rb_traj(const m3pc_replay* rb) {
    TrajP p;
    p.obs = rb->obs;
    p.act = rb->act;
    p.rew = rb->rew;
    p.val = rb->val;
    p.len = rb->len;
    p.cum = rb->cum;
    p.C = rb->C;
    p.M = rb->M;
    p.L = rb->L;
    p.S = rb->S;
    p.A = rb->A;
    p.head = rb->head;
    p.count = rb->count;
    return p;
}

RingP rb_ring(const m3pc_replay* rb, int which) {
    const auto& g = rb->ring[which];
    RingP r;
    r.s = g.s;
    r.a = g.a;
    r.r = g.r;
    r.s2 = g.s2;
    r.d = g.d;
    r.cap = g.cap;
    r.head = g.head;
    r.count = g.count;
    return r;
}

// one more entry at the tail of a ring of `cap` slots: the slot it takes; the oldest leaves when the ring is full
int ring_push(int cap, int* head, int* count) {
    if (*count < cap) return (*head + (*count)++) % cap;
    const int slot = *head;
    *head = (*head + 1) % cap;
    return slot;
}

// `total` more entries at the tail
void ring_advance(int cap, int* head, int* count, long long total) {
    const long long over = (long long)*count + total - cap;
    *count = (int)(over > 0 ? cap : *count + total);
    if (over > 0) *head = (int)((*head + over) % cap);
}

int rb_finish(m3pc_replay* rb, hipStream_t st, const char* what) {
    const int rc = check_launch(what);
    const int rr = rb->pool.release(st);
    return rc ? rc : rr;
}

int rb_abandon(m3pc_replay* rb, int rc) {
    rb->pool.held.clear();
    return rc;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int m3pc_replay_create(m3pc_handle* h, int traj_capacity, int max_steps, int segment_length, int offline_capacity, int online_capacity,
                       m3pc_replay** out) {
    if (!h || !out) return fail(M3PC_EINVAL, "null argument");
    if (traj_capacity < 0 || offline_capacity < 0 || online_capacity < 0)
        return fail(M3PC_EINVAL, "m3pc_replay_create: a capacity < 0 (%d, %d, %d)", traj_capacity, offline_capacity, online_capacity);
    if (max_steps < 1) return fail(M3PC_EINVAL, "m3pc_replay_create: max_steps %d < 1", max_steps);
    if (segment_length < 1 || segment_length > max_steps)
        return fail(M3PC_EINVAL, "m3pc_replay_create: segment_length %d outside [1, max_steps=%d]", segment_length, max_steps);
    const int S = h->dm.state_dim, A = h->dm.action_dim;
    if (S < 1 || A < 1) return fail(M3PC_EINVAL, "m3pc_replay_create: the handle has no sizes");
    if ((long long)traj_capacity * max_steps > (1LL << 31) - 1)
        return fail(M3PC_EINVAL, "m3pc_replay_create: traj_capacity * max_steps = %lld rows > 2^31 - 1", (long long)traj_capacity * max_steps);
    m3pc_replay* rb = new m3pc_replay();
    rb->device = h->device;
    rb->S = S;
    rb->A = A;
    rb->C = traj_capacity;
    rb->M = max_steps;
    rb->L = segment_length;
    rb->lens.assign((size_t)traj_capacity, 0);
    rb->ring[M3PC_REPLAY_OFFLINE].cap = offline_capacity;
    rb->ring[M3PC_REPLAY_ONLINE].cap = online_capacity;
    *out = rb;
    return 0;
}

int m3pc_replay_destroy(m3pc_replay* rb) {
    if (!rb) return 0;
    if (rb->ready || !rb->pool.stages.empty()) {
        (void)hipSetDevice(rb->device);
        (void)hipDeviceSynchronize();
        for (void* b : {(void*)rb->obs, (void*)rb->act, (void*)rb->rew, (void*)rb->val, (void*)rb->len, (void*)rb->cum})
            if (b) (void)hipFree(b);
        for (auto& g : rb->ring)
            for (void* b : {(void*)g.s, (void*)g.a, (void*)g.r, (void*)g.s2, (void*)g.d})
                if (b) (void)hipFree(b);
        rb->pool.destroy();
    }
    delete rb;
    return 0;
}

int m3pc_replay_append(m3pc_replay* rb, int n, const float* obs, const float* act, const float* rew, const double* val, const int* lens,
                       int on_device, void* stream) {
    if (!rb || !obs || !act || !rew || !val || !lens) return fail(M3PC_EINVAL, "null argument");
    if (n < 1 || n > rb->C) return fail(M3PC_EINVAL, "m3pc_replay_append: n %d outside [1, traj_capacity=%d]", n, rb->C);
    for (int i = 0; i < n; ++i)
        if (lens[i] < rb->L || lens[i] > rb->M)
            return fail(M3PC_EINVAL, "m3pc_replay_append: lens[%d] = %d outside [segment_length=%d, max_steps=%d]", i, lens[i], rb->L, rb->M);
    hipStream_t st = (hipStream_t)stream;
    CHK(rb_ensure(rb));
    const size_t rows = (size_t)n * rb->M;
    const void *o = obs, *a = act, *r = rew, *v = val, *l = nullptr;
    int rc = rb->pool.stage(lens, (size_t)n * sizeof(int), &l, "m3pc_replay");
    if (!rc && !on_device) rc = rb->pool.stage(obs, rows * rb->S * sizeof(float), &o, "m3pc_replay");
    if (!rc && !on_device) rc = rb->pool.stage(act, rows * rb->A * sizeof(float), &a, "m3pc_replay");
    if (!rc && !on_device) rc = rb->pool.stage(rew, rows * sizeof(float), &r, "m3pc_replay");
    if (!rc && !on_device) rc = rb->pool.stage(val, rows * sizeof(double), &v, "m3pc_replay");
    if (rc) return rb_abandon(rb, rc);
    const int slot0 = (rb->head + rb->count) % rb->C;
    hipLaunchKernelGGL(rb_append_traj_kernel, dim3(rb_blocks((long long)rows * (rb->S + rb->A + 2))), dim3(RB_THREADS), 0, st, rb_traj(rb), n, slot0,
                       (const float*)o, (const float*)a, (const float*)r, (const double*)v, (const int*)l);
    CHK(rb_finish(rb, st, "replay_append"));
    for (int i = 0; i < n; ++i) rb->lens[(size_t)ring_push(rb->C, &rb->head, &rb->count)] = lens[i];
    rb->cum_valid = false;
    return 0;
}

int m3pc_replay_append_transitions(m3pc_replay* rb, int which, int n, const float* state, const float* action, const float* reward,
                                   const float* next_state, const float* done, int on_device, void* stream) {
    if (!rb || !state || !action || !reward || !next_state || !done) return fail(M3PC_EINVAL, "null argument");
    if (which != M3PC_REPLAY_OFFLINE && which != M3PC_REPLAY_ONLINE)
        return fail(M3PC_EINVAL, "m3pc_replay_append_transitions: ring %d is neither M3PC_REPLAY_OFFLINE nor M3PC_REPLAY_ONLINE", which);
    auto& g = rb->ring[which];
    if (n < 1 || n > g.cap) return fail(M3PC_EINVAL, "m3pc_replay_append_transitions: n %d outside [1, capacity=%d]", n, g.cap);
    hipStream_t st = (hipStream_t)stream;
    CHK(rb_ensure(rb));
    const void *s = state, *a = action, *r = reward, *s2 = next_state, *d = done;
    int rc = 0;
    if (!on_device) {
        rc = rb->pool.stage(state, (size_t)n * rb->S * sizeof(float), &s, "m3pc_replay");
        if (!rc) rc = rb->pool.stage(action, (size_t)n * rb->A * sizeof(float), &a, "m3pc_replay");
        if (!rc) rc = rb->pool.stage(reward, (size_t)n * sizeof(float), &r, "m3pc_replay");
        if (!rc) rc = rb->pool.stage(next_state, (size_t)n * rb->S * sizeof(float), &s2, "m3pc_replay");
        if (!rc) rc = rb->pool.stage(done, (size_t)n * sizeof(float), &d, "m3pc_replay");
    }
    if (rc) return rb_abandon(rb, rc);
    const int slot0 = (int)(((long long)g.head + g.count) % g.cap);
    hipLaunchKernelGGL(rb_append_trans_kernel, dim3(rb_blocks((long long)n * (2 * rb->S + rb->A + 2))), dim3(RB_THREADS), 0, st, rb_ring(rb, which),
                       rb->S, rb->A, n, slot0, (const float*)s, (const float*)a, (const float*)r, (const float*)s2, (const float*)d);
    CHK(rb_finish(rb, st, "replay_append_transitions"));
    ring_advance(g.cap, &g.head, &g.count, n);
    return 0;
}

int m3pc_replay_push_episodes(m3pc_replay* rb, m3pc_episodes* ep, const int* env_ids, int n, double discount, int use_avg, const float* final_obs,
                              int final_on_device, int* taken, void* stream) {
    if (!rb || !ep) return fail(M3PC_EINVAL, "null argument");
    if (ep->S != rb->S || ep->A != rb->A || ep->M != rb->M || ep->device != rb->device)
        return fail(M3PC_EINVAL, "m3pc_replay_push_episodes: the store (S %d, A %d, max_steps %d, device %d) does not fit the buffer (%d, %d, %d, %d)",
                    ep->S, ep->A, ep->M, ep->device, rb->S, rb->A, rb->M, rb->device);
    if (n < 1 || n > ep->n_envs) return fail(M3PC_EINVAL, "m3pc_replay_push_episodes: n %d outside [1, n_envs=%d]", n, ep->n_envs);
    if (!(discount >= 0.0 && discount <= 1.7976931348623157e308))
        return fail(M3PC_EINVAL, "m3pc_replay_push_episodes: the discount must be finite and >= 0");
    std::vector<char> seen((size_t)ep->n_envs, 0);
    for (int i = 0; env_ids && i < n; ++i) {
        if (env_ids[i] < 0 || env_ids[i] >= ep->n_envs)
            return fail(M3PC_EINVAL, "m3pc_replay_push_episodes: env_ids[%d] = %d outside [0, n_envs=%d)", i, env_ids[i], ep->n_envs);
        if (seen[(size_t)env_ids[i]]) return fail(M3PC_EINVAL, "m3pc_replay_push_episodes: env_ids[%d] = %d is repeated within the call", i, env_ids[i]);
        seen[(size_t)env_ids[i]] = 1;
    }
    // what the call does, from the mirrors
    auto& on = rb->ring[M3PC_REPLAY_ONLINE];
    std::vector<PushD> desc((size_t)n);
    int head = rb->head, count = rb->count, took = 0;
    long long q = 0;
    for (int i = 0; i < n; ++i) {
        PushD& d = desc[(size_t)i];
        d.env = env_ids ? env_ids[i] : i;
        d.len = ep->mirror[(size_t)d.env];
        d.slot = -1;
        if (rb->C > 0 && d.len >= rb->L) {
            d.slot = ring_push(rb->C, &head, &count);
            ++took;
        }
        d.nt = on.cap > 0 ? (final_obs ? d.len : (d.len > 0 ? d.len - 1 : 0)) : 0;
        d.q = q;
        q += d.nt;
    }
    // (more taken than the ring holds: only the last writer of a slot writes it)
    std::vector<char> used((size_t)(rb->C > 0 ? rb->C : 1), 0);
    for (int i = n - 1; i >= 0; --i) {
        int& s = desc[(size_t)i].slot;
        if (s < 0) continue;
        if (used[(size_t)s]) s = -1;
        else used[(size_t)s] = 1;
    }
    if (taken) *taken = took;
    if (took == 0 && q == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    CHK(rb_ensure(rb));
    if (!ep->ready) return fail(M3PC_ESTATE, "m3pc_replay_push_episodes: the store has path lengths but no storage");
    const void *dd = nullptr, *fo = final_obs;
    int rc = rb->pool.stage(desc.data(), desc.size() * sizeof(PushD), &dd, "m3pc_replay");
    if (!rc && final_obs && !final_on_device) rc = rb->pool.stage(final_obs, (size_t)n * rb->S * sizeof(float), &fo, "m3pc_replay");
    if (rc) return rb_abandon(rb, rc);
    const int per = RB_THREADS / 64, vblocks = took > 0 ? (n + per - 1) / per : 0;
    const long long keep_from = q > on.cap ? q - on.cap : 0;
    const int tslot0 = on.cap > 0 ? (int)(((long long)on.head + on.count) % on.cap) : 0;
    const int cblocks = rb_blocks((long long)n * rb->M * (3 * rb->S + 2 * rb->A + 3));
    hipLaunchKernelGGL(rb_push_kernel, dim3(vblocks + cblocks), dim3(RB_THREADS), 0, st, rb_traj(rb), rb_ring(rb, M3PC_REPLAY_ONLINE), ep->obs, ep->act,
                       ep->rew, n, vblocks, discount, use_avg ? 1 : 0, (const float*)fo, keep_from, tslot0, (const PushD*)dd);
    CHK(rb_finish(rb, st, "replay_push_episodes"));
    for (int i = 0; i < n; ++i)
        if (desc[(size_t)i].slot >= 0) rb->lens[(size_t)desc[(size_t)i].slot] = desc[(size_t)i].len;
    rb->head = head;
    rb->count = count;
    if (took) rb->cum_valid = false;
    if (q > 0) ring_advance(on.cap, &on.head, &on.count, q);
    return 0;
}

int m3pc_replay_sample_segments(m3pc_replay* rb, int batch, int mode, const int* traj_index, const int* start_index, int index_on_device,
                                unsigned long long seed, unsigned long long step, float* states, float* actions, float* rewards, void* returns,
                                int returns_f32, int* out_traj, int* out_start, void* stream) {
    if (!rb || !states || !actions || !rewards || !returns) return fail(M3PC_EINVAL, "null argument");
    CHK(replay_check_segments(rb, batch, mode, traj_index, start_index, index_on_device, "m3pc_replay_sample_segments"));
    hipStream_t st = (hipStream_t)stream;
    CHK(rb_ensure(rb));
    const void *ti = traj_index, *si = start_index;
    if (traj_index && !index_on_device) {
        int rc = rb->pool.stage(traj_index, (size_t)batch * sizeof(int), &ti, "m3pc_replay");
        if (!rc) rc = rb->pool.stage(start_index, (size_t)batch * sizeof(int), &si, "m3pc_replay");
        if (rc) return rb_abandon(rb, rc);
    }
    const TrajP p = rb_traj(rb);
    if (!traj_index && mode == M3PC_REPLAY_LENGTH && !rb->cum_valid) {
        hipLaunchKernelGGL(rb_scan_kernel, dim3(1), dim3(64), 0, st, p);
        if (int rc = check_launch("replay_scan")) return rb_abandon(rb, rc);
        rb->cum_valid = true;
    }
    const int per = RB_THREADS / 64;
    hipLaunchKernelGGL(rb_segments_kernel, dim3((batch + per - 1) / per), dim3(RB_THREADS), 0, st, p, batch, mode, (const int*)ti, (const int*)si,
                       (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step, (uint32_t)(step >> 32), states, actions, rewards, returns,
                       returns_f32 ? 1 : 0, out_traj, out_start);
    return rb_finish(rb, st, "replay_sample_segments");
}

int m3pc_replay_sample_transitions(m3pc_replay* rb, int batch, int n_online, const int* index, int index_on_device, unsigned long long seed,
                                   unsigned long long step, float* state, float* action, float* reward, float* next_state, float* done, int* out_index,
                                   void* stream) {
    if (!rb || !state || !action || !reward || !next_state || !done) return fail(M3PC_EINVAL, "null argument");
    if (batch < 1) return fail(M3PC_EINVAL, "m3pc_replay_sample_transitions: batch %d < 1", batch);
    if (n_online < 0 || n_online > batch) return fail(M3PC_EINVAL, "m3pc_replay_sample_transitions: n_online %d outside [0, batch=%d]", n_online, batch);
    const int want[2] = {batch - n_online, n_online};
    for (int w : {M3PC_REPLAY_ONLINE, M3PC_REPLAY_OFFLINE}) {
        const char* name = w == M3PC_REPLAY_ONLINE ? "online" : "offline";
        if (want[w] > 0 && rb->ring[w].count == 0) return fail(M3PC_ESTATE, "m3pc_replay_sample_transitions: the %s ring is empty", name);
        if (want[w] > rb->ring[w].count)
            return fail(M3PC_EINVAL, "m3pc_replay_sample_transitions: %d rows asked of the %s ring, which holds %d", want[w], name, rb->ring[w].count);
    }
    if (index && !index_on_device)
        for (int j = 0; j < batch; ++j) {
            const int cnt = rb->ring[j < n_online ? M3PC_REPLAY_ONLINE : M3PC_REPLAY_OFFLINE].count;
            if (index[j] < 0 || index[j] >= cnt)
                return fail(M3PC_EINVAL, "m3pc_replay_sample_transitions: index[%d] = %d outside [0, count=%d)", j, index[j], cnt);
        }
    hipStream_t st = (hipStream_t)stream;
    CHK(rb_ensure(rb));
    const void* ix = index;
    if (index && !index_on_device)
        if (int rc = rb->pool.stage(index, (size_t)batch * sizeof(int), &ix, "m3pc_replay")) return rb_abandon(rb, rc);
    hipLaunchKernelGGL(rb_transitions_kernel, dim3(rb_blocks((long long)batch * (2 * rb->S + rb->A + 2))), dim3(RB_THREADS), 0, st,
                       rb_ring(rb, M3PC_REPLAY_ONLINE), rb_ring(rb, M3PC_REPLAY_OFFLINE), rb->S, rb->A, batch, n_online, (const int*)ix, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (uint32_t)step, (uint32_t)(step >> 32), state, action, reward, next_state, done, out_index);
    return rb_finish(rb, st, "replay_sample_transitions");
}

int m3pc_replay_values_up_bound(m3pc_replay* rb, double* out, void* stream) {
    if (!rb || !out) return fail(M3PC_EINVAL, "null argument");
    if (rb->count == 0) return fail(M3PC_ESTATE, "m3pc_replay_values_up_bound: the buffer holds no trajectory");
    hipStream_t st = (hipStream_t)stream;
    CHK(rb_ensure(rb));
    hipLaunchKernelGGL(rb_upbound_kernel, dim3((rb->M + RB_THREADS - 1) / RB_THREADS), dim3(RB_THREADS), 0, st, rb_traj(rb), out);
    return check_launch("replay_values_up_bound");
}

int m3pc_replay_counts(m3pc_replay* rb, int* trajectories, int* offline, int* online) {
    if (!rb) return fail(M3PC_EINVAL, "null argument");
    if (trajectories) *trajectories = rb->count;
    if (offline) *offline = rb->ring[M3PC_REPLAY_OFFLINE].count;
    if (online) *online = rb->ring[M3PC_REPLAY_ONLINE].count;
    return 0;
}

int m3pc_replay_path_lengths(m3pc_replay* rb, int* path_lengths, int capacity) {
    if (!rb || !path_lengths) return fail(M3PC_EINVAL, "null argument");
    if (capacity < rb->count) return fail(M3PC_EINVAL, "m3pc_replay_path_lengths: room for %d of %d path lengths", capacity, rb->count);
    for (int i = 0; i < rb->count; ++i) path_lengths[i] = rb->lens[(size_t)((rb->head + i) % rb->C)];
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
