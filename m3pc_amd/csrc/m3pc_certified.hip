// libm3pc_hip.so -- the certified plan steps of the C ABI (include/m3pc_hip.h): the serial call, the pipelined _begin / _end pair
// and the lock-step batch, each with and without the eval_action certificate, and m3pc_calibrate_delta.  The protocol itself is
// cert_resolve.h: ONE loop (cert_resolve; cert_resolve_eval with the third certificate behind it), driven here by two ops -- a
// single step (StepOps) and a window of a lock-step batch (LsOps).
#include <atomic>
#include <chrono>

#include "m3pc_internal.h"

namespace m3pc {
// one rank, every candidate: what both calls need of m3pc_plan_args before any HIP call
int cert_check_args(const m3pc_plan_args* a, const char* who) {
    if (a->n_total < 1 || a->n_total > 16384) return fail(M3PC_EINVAL, "%s: n_total %d outside [1, 16384]", who, a->n_total);
    if (a->n_begin != 0 || a->n_count != a->n_total)
        return fail(M3PC_EINVAL, "%s plans on one rank: candidates [%d,+%d) are not all n_total=%d", who, a->n_begin, a->n_count, a->n_total);
    if (!precision_ok(a->precision)) return fail(M3PC_EINVAL, "bad precision %d", a->precision);
    if (a->slot < 0 || a->slot >= M3PC_SLOTS) return fail(M3PC_EINVAL, "slot %d outside [0, %d)", a->slot, M3PC_SLOTS);
    return 0;
}
bool cert_any_begun(const m3pc_handle* h) {
    for (int s = 0; s < M3PC_SLOTS; ++s)
        if (h->cstep[s].begun) return true;
    return false;
}
}  // namespace m3pc

#pragma GCC visibility push(default)
extern "C" {

// ---- the certified plan step as one call (learner.py:318-325 on low-precision scores that fp32 re-scores certify)
// The statistics of the kernels that carried seq[0 .. n), read from n consecutive host-mapped 8-float blocks (block i closed by
// seq[i]): ONE BOUNDED spin on the sequence numbers (10 s, the bound of the Python binding's HostStats.wait); on expiry one
// synchronisation of the stream and the device copies.  out: 8 floats per block.
static int cert_wait_blocks(const volatile float* hs, const float* dev, const float* seq, int n, int n_device, hipStream_t st, float* out) {
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    for (int b = 0; b < n; ++b)
        while (hs[8 * b + 4] != seq[b]) {
            if ((++spins & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) {
                if (hipStreamSynchronize(st) != hipSuccess ||
                    hipMemcpy(out, dev, (size_t)n * 8 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
                    return fail(M3PC_EHIP, "the statistics of the certified step reached neither host-mapped memory within 10 s nor the host by a copy");
                for (int v = 0; v < n; ++v)
                    for (int i = n_device; i < 8; ++i) out[8 * v + i] = 0.f;  // (a four-statistics merge leaves the device slots 4..7 alone)
                return 0;
            }
        }
    std::atomic_thread_fence(std::memory_order_acquire);
    for (int i = 0; i < 8 * n; ++i) out[i] = hs[i];
    return 0;
}
static int cert_wait(m3pc_handle* h, int slot, float seq, int n_device, hipStream_t st, float out[8]) {
    return cert_wait_blocks(h->cert_host + 8 * slot, h->cert_stats[slot], &seq, 1, n_device, st, out);
}
static float cert_next_seq(m3pc_handle* h, int slot) {
    h->cert_seq[slot] = h->cert_seq[slot] % 1000000 + 1;
    return (float)h->cert_seq[slot];
}
// the checks of the certified step (serial call and _begin), before any HIP call
static int cert_check_step(const m3pc_plan_args* a, const m3pc_cert_args* c, const char* who) {
    CHK(cert_check_args(a, who));
    const int N = a->n_total, kmin = c->kmin, kmax = c->kmax, R = c->rmax, rfirst = c->rfirst;
    if (a->precision != M3PC_PREC_FP32) {
        if (kmax < 1 || kmax > 1023 || kmin < 1 || kmin > kmax || kmin > N)
            return fail(M3PC_EINVAL, "kmin %d / kmax %d outside 1 <= kmin <= min(kmax, n_total=%d), kmax <= 1023", kmin, kmax, N);
        if (R < 0 || R > 64 || R > N) return fail(M3PC_EINVAL, "rmax %d outside [0, min(64, n_total=%d)]", R, N);
        if (kmax + R > 1023) return fail(M3PC_EINVAL, "kmax %d + rmax %d > 1023 (the merge lists 1024 entries)", kmax, R);
        if (R == 0 ? rfirst != 0 : (rfirst < 1 || rfirst > R)) return fail(M3PC_EINVAL, "rfirst %d outside [1, rmax=%d] (0 with rmax == 0)", rfirst, R);
        if (!(c->delta >= 0.f)) return fail(M3PC_EINVAL, "delta must be >= 0");
    }
    if (!(c->temperature == c->temperature)) return fail(M3PC_EINVAL, "temperature is not a number");
    return 0;
}
// ---- the pieces of a certified step, on the step's tail stream (the caller's stream in the serial call)
using CertStep = m3pc_handle::CertStep;
static int* cert_L(m3pc_handle* h, const CertStep& S) { return S.list ? S.list : h->cert_list[S.a.slot]; }
// A pipelined step's tail runs on a chain stream, beside the candidate passes of its neighbours on the callers' streams.  What
// it runs in the chain workspace of its parity needs no order.  What overflows into the candidate workspace -- a re-score of more
// than max_rescore candidates, the fp32 pass over every candidate (with sa_buf and the handle's top-1 scratch) -- is ordered by
// events: behind every candidate pass enqueued so far (ev_cand of the slot begun last; m3pc_candidate_pass / m3pc_rescore order
// the handle's own streams themselves: ws_sync) and behind the overflow before it, and every later _begin's candidate pass goes
// behind ev_excl.
static int cert_excl_enter(m3pc_handle* h, const CertStep& S) {
    if (!S.async) return 0;
    if (h->cand_last_slot >= 0) HIPCHK(hipStreamWaitEvent(S.tail, h->step_ev[h->cand_last_slot][2], 0));
    if (h->excl_valid) HIPCHK(hipStreamWaitEvent(S.tail, h->ev_excl, 0));
    return 0;
}
static int cert_excl_leave(m3pc_handle* h, const CertStep& S) {
    if (!S.async) return 0;
    HIPCHK(hipEventRecord(h->ev_excl, S.tail));
    h->excl_valid = true;
    return 0;
}
static int cert_rescore(m3pc_handle* h, CertStep& S, int lo, int hi) {  // list positions [lo, hi)
    m3pc_plan_args ra = S.a;
    ra.precision = M3PC_PREC_FP32;
    ra.flags = 0;
    ra.window = 0;
    ra.n_count = hi - lo;
    const bool excl = hi - lo > h->chain[0].max_cand;
    if (excl) CHK(cert_excl_enter(h, S));
    CHK(m3pc_rescore(h, &ra, S.states, S.actions, S.rewards, S.eps, cert_L(h, S) + lo, hi - lo, nullptr, h->cert_f[S.a.slot] + lo, S.tail));
    if (excl) CHK(cert_excl_leave(h, S));
    return 0;
}
static int cert_select(m3pc_handle* h, CertStep& S) {
    return m3pc_select(h, S.merged, S.sample_actions, (long long)S.a.horizon * h->A, S.a.n_total, S.c.temperature, S.expo, S.p, S.eval_action,
                       S.argmax, S.sample_idx, S.sample_action, S.tail);
}
static int cert_merge(m3pc_handle* h, CertStep& S, int n, int r, bool with_select) {
    const int slot = S.a.slot, R = S.c.rmax, N = S.a.n_total, o = R - r;
    int* L = cert_L(h, S);
    float *B = h->cert_b[slot], *F = h->cert_f[slot], *dstats = h->cert_stats[slot], *hstats = h->cert_host_dev + 8 * slot;
    const float temp = S.c.temperature;
    S.seq = cert_next_seq(h, slot);
    ++S.rounds;
    if (R > 0) {
        if (with_select)
            return m3pc_merge_race_select(h, S.scores_low, S.expo, temp, N, L + o, r, n, B + o, F + o, (float)S.cs.delta, S.merged, dstats, hstats,
                                          S.seq, S.sample_actions, (long long)S.a.horizon * h->A, S.p, S.eval_action, S.argmax, S.sample_idx,
                                          S.sample_action, S.tail);
        return m3pc_rescore_merge_race(h, S.scores_low, S.expo, temp, N, L + o, r, n, B + o, F + o, (float)S.cs.delta, S.merged, dstats, hstats,
                                       S.seq, S.tail);
    }
    CHK(m3pc_rescore_merge(h, S.scores_low, N, L, n, B, F, (float)S.cs.delta, S.merged, dstats, hstats, S.seq, S.tail));
    return with_select ? cert_select(h, S) : 0;
}
// The lists are too short.  Window set: the `need` best candidates by low-precision score (descending, ties to the lower
// index) listed behind the race entries in place of the score entries, re-scored in chunks of the re-score workspace.
// Everything: one fp32 candidate pass in the candidate workspace (stream-ordered behind this step's own pass), the best
// entry merged with itself at delta = 0 -- the select then runs on fp32 scores alone.
static int cert_window_set(m3pc_handle* h, CertStep& S, int need, bool everything) {
    const int slot = S.a.slot, R = S.c.rmax, N = S.a.n_total;
    int* L = cert_L(h, S);
    float *B = h->cert_b[slot], *dstats = h->cert_stats[slot], *hstats = h->cert_host_dev + 8 * slot;
    hipStream_t st = S.tail;
    const int cnt = need < N ? need : N;
    if (cnt <= 1024 - 32 && !everything) {
        if (!launch_topk_race(S.scores_low, nullptr, 0.f, N, cnt, 0, R, L, B, st))
            launch_window_stats(S.scores_low, N, L + R, cnt, 1, cnt, 0.f, dstats + 8, nullptr, 0.f, B + R, st, 0);
        CHK(check_launch("plan_step_certified (window set)"));
        const int cap = h->chain[0].max_cand;
        for (int c0 = 0; c0 < cnt; c0 += cap) CHK(cert_rescore(h, S, R + c0, R + (cnt < c0 + cap ? cnt : c0 + cap)));
        S.cs.n_done = cnt;
        CHK(cert_merge(h, S, cnt, S.cs.r_done, false));
        return cert_select(h, S);
    }
    m3pc_plan_args ra = S.a;
    ra.precision = M3PC_PREC_FP32;
    ra.flags = 0;
    ra.window = 0;
    ra.n_count = N;
    float* f32 = h->cert_f32[slot];
    int* top1 = h->cert_top1[slot];
    float* top1v = dstats + 16;
    CHK(cert_excl_enter(h, S));
    CHK(m3pc_candidate_pass(h, &ra, S.states, S.actions, S.rewards, S.eps, nullptr, nullptr, h->sa_buf, f32, nullptr, nullptr, st));
    CHK(cert_excl_leave(h, S));
    if (!launch_topk_race(f32, nullptr, 0.f, N, 1, 0, 0, top1, top1v, st))
        launch_window_stats(f32, N, top1, 1, 1, 1, 0.f, dstats + 8, nullptr, 0.f, top1v, st, 0);
    CHK(check_launch("plan_step_certified (every candidate in fp32)"));
    S.cs.n_done = N;
    S.seq = cert_next_seq(h, slot);
    ++S.rounds;
    CHK(m3pc_rescore_merge(h, f32, N, top1, 1, top1v, top1v, 0.f, S.merged, dstats, hstats, S.seq, st));
    return cert_select(h, S);
}
// first pass, enqueued before anything is read: lists, fp32 re-score of the kmin best by score and the rfirst best by race
// key, merge + certificates + select.  fp32 scores for every candidate: the select alone.
static int cert_first_pass(m3pc_handle* h, CertStep& S) {
    const int slot = S.a.slot, N = S.a.n_total, R = S.c.rmax, kmin = S.c.kmin, kmax = S.c.kmax, rfirst = S.c.rfirst;
    if (S.a.precision == M3PC_PREC_FP32) {
        HIPCHK(hipMemcpyAsync(S.merged, S.scores_low, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, S.tail));
        return m3pc_select(h, S.scores_low, S.sample_actions, (long long)S.a.horizon * h->A, N, S.c.temperature, S.expo, S.p, S.eval_action,
                           S.argmax, S.sample_idx, S.sample_action, S.tail);
    }
    int* L = cert_L(h, S);
    float *B = h->cert_b[slot], *dstats = h->cert_stats[slot];
    S.cs = CertState(N, kmax, R, S.c.grow_delta != 0, kmin, rfirst, (double)S.c.delta);
    S.rounds = 0;
    if (R > 0) CHK(m3pc_topk_race_window(h, S.scores_low, S.expo, S.c.temperature, N, kmax, kmin, R, L, nullptr, B, nullptr, 0.f, S.tail));
    else CHK(m3pc_topk_window(h, S.scores_low, N, kmax, kmin, 0.f, L, dstats + 8, B, nullptr, 0.f, S.tail));
    CHK(cert_rescore(h, S, R - rfirst, R + kmin));
    return cert_merge(h, S, kmin, rfirst, true);
}
// The eval_action certificate of m3pc_plan_step_certified_eval behind the step's last merge + select: the re-scored race entries
// and the listed score entries (kmax of them; behind a window set the list is wholly re-scored), under delta as it stands.
// Launch and wait are two pieces: a pipelined step launches it in advance (step_enqueue_tail) for r / n / delta of the first pass.
static int cert_eval_launch(m3pc_handle* h, CertStep& S, int r, int n, int n_listed, float delta, float* seq_out) {
    const int slot = S.a.slot, R = S.c.rmax;
    h->eval_seq[slot] = h->eval_seq[slot] % 1000000 + 1;
    *seq_out = (float)h->eval_seq[slot];
    return m3pc_eval_bound(h, S.merged, S.a.n_total, cert_L(h, S) + R - r, r, n, n_listed, S.sample_actions, (long long)S.a.horizon * h->A,
                           h->A, S.c.temperature, delta, S.eval_tol, h->cert_stats[slot] + 24, h->eval_host_dev + 8 * slot, *seq_out, S.tail);
}
static int cert_eval_wait(m3pc_handle* h, CertStep& S, float seq, float e8[8]) {
    const int slot = S.a.slot;
    return cert_wait_blocks(h->eval_host + 8 * slot, h->cert_stats[slot] + 24, &seq, 1, 8, S.tail, e8);
}
// the second host-mapped block of every slot, at the first call that asks for the eval certificate
static int eval_host_setup(m3pc_handle* h) {
    if (h->eval_host) return 0;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipHostMalloc((void**)&h->eval_host, (size_t)M3PC_SLOTS * 8 * sizeof(float), hipHostMallocMapped | hipHostMallocCoherent));
    memset(h->eval_host, 0, (size_t)M3PC_SLOTS * 8 * sizeof(float));
    HIPCHK(hipHostGetDevicePointer((void**)&h->eval_host_dev, h->eval_host, 0));
    return 0;
}
// the device work of cert_resolve (cert_resolve.h) for one step: certificate.py's _TicketOps
struct StepOps {
    m3pc_handle* h;
    CertStep& S;
    int read(bool four_only, float* out8) { return cert_wait(h, S.a.slot, S.seq, four_only ? 4 : 8, S.tail, out8); }
    int extend(int lo, int hi) { return cert_rescore(h, S, S.c.rmax + lo, S.c.rmax + hi); }
    int extend_race(int lo, int hi) { return cert_rescore(h, S, S.c.rmax - hi, S.c.rmax - lo); }
    int window_set(int need, bool everything) { return cert_window_set(h, S, need, everything); }
    int merge_select() { return cert_merge(h, S, S.cs.n_done, S.cs.r_done, true); }
    // The bound behind the last merge + select.  A launch made in advance saw r = rfirst, n = kmin and delta as it came in behind the
    // first merge: it is this launch -- same kernel, same inputs, same bits -- exactly when no further merge has been issued (an
    // extension, a raised delta that is acted on and a window set all merge again).  Otherwise it is dropped: launch and wait.
    int eval_read(int n_listed, float* out8) {
        if (S.spec) {
            S.spec = false;
            if (S.rounds == S.spec_rounds && n_listed == S.spec_n_listed && (float)S.cs.delta == S.c.delta)
                return cert_eval_wait(h, S, S.spec_seq, out8);
        }
        float seq;
        CHK(cert_eval_launch(h, S, S.cs.r_done, S.cs.n_done, n_listed, (float)S.cs.delta, &seq));
        return cert_eval_wait(h, S, seq, out8);
    }
};
// The certificates of a step whose first pass is enqueued.  erec: the third certificate under S.eval_tol (cert_resolve_eval);
// erec == NULL: the two certificates alone, nothing else launched, read or allocated
static int cert_resolve_step(m3pc_handle* h, CertStep& S, m3pc_cert_record* rec, m3pc_eval_record* erec = nullptr) {
    const int N = S.a.n_total;
    if (erec) memset(erec, 0, sizeof(*erec));
    if (S.a.precision == M3PC_PREC_FP32) {
        cert_record_fp32(N, rec);
        if (erec) erec->eval_certified = 1;
        return 0;
    }
    memset(rec, 0, sizeof(*rec));
    StepOps ops{h, S};
    if (erec) {
        EvalState es(S.eval_tol);
        CHK(cert_resolve_eval(S.cs, ops, es));
        cert_eval_record(es, erec);
    } else {
        CHK(cert_resolve(S.cs, ops));
    }
    cert_record(S.cs, rec);
    rec->rounds = S.rounds;
    return 0;
}
static void cert_fill(CertStep& S, const m3pc_plan_args* a, const m3pc_cert_args* c, const float* states, const float* actions,
                      const float* rewards, const float* eps, const float* expo, float* sample_actions, float* scores_low, float* merged,
                      int* list, float* p, float* eval_action, int* argmax, int* sample_idx, float* sample_action, hipStream_t tail, bool async,
                      float eval_tol) {
    S.eval_tol = eval_tol;
    S.spec = false;
    S.a = *a;
    S.c = *c;
    S.states = states;
    S.actions = actions;
    S.rewards = rewards;
    S.eps = eps;
    S.expo = expo;
    S.sample_actions = sample_actions;
    S.scores_low = scores_low;
    S.merged = merged;
    S.list = list;
    S.p = p;
    S.eval_action = eval_action;
    S.argmax = argmax;
    S.sample_idx = sample_idx;
    S.sample_action = sample_action;
    S.tail = tail;
    S.async = async;
    S.tail_pending = false;
}

// the serial certified step; with_eval: m3pc_plan_step_certified_eval (eval_tol, erec)
static int cert_step_serial(m3pc_handle* h, const m3pc_plan_args* a, const m3pc_cert_args* c, const float* states, const float* actions,
                            const float* rewards, const float* eps, const float* expo, float* loc, float* std_, float* sample_actions,
                            float* scores_low, float* merged, int* list, float* p, float* eval_action, int* argmax, int* sample_idx,
                            float* sample_action, m3pc_cert_record* rec, bool with_eval, float eval_tol, m3pc_eval_record* erec,
                            void* stream, const char* who) {
    if (!h || !a || !c || !states || !actions || !rewards || !eps || !expo || !sample_actions || !scores_low || !merged || !rec ||
        (with_eval && !erec))
        return fail(M3PC_EINVAL, "null argument");
    CHK(cert_check_step(a, c, who));
    if (with_eval && !(eval_tol > 0.f)) return fail(M3PC_EINVAL, "%s: eval_tol must be > 0 (+inf: report only)", who);
    if (cert_any_begun(h)) return fail(M3PC_ESTATE, "%s with a pipelined step begun (m3pc_plan_step_certified_end first)", who);
    memset(rec, 0, sizeof(*rec));
    if (with_eval) {
        memset(erec, 0, sizeof(*erec));
        if (a->precision != M3PC_PREC_FP32) CHK(eval_host_setup(h));
    }
    CertStep& S = h->cstep[a->slot];
    cert_fill(S, a, c, states, actions, rewards, eps, expo, sample_actions, scores_low, merged, list, p, eval_action, argmax, sample_idx,
              sample_action, (hipStream_t)stream, false, with_eval ? eval_tol : 0.f);

    // learner.py:278-316: policy pass (fp32), candidates, candidate pass in args->precision
    m3pc_plan_args pa = *a;
    pa.flags = a->flags & M3PC_PLAN_PRUNED_POLICY;
    pa.window = 0;
    CHK(m3pc_policy_pass(h, &pa, states, actions, rewards, nullptr, nullptr, stream));
    pa.flags = 0;
    CHK(m3pc_candidate_pass(h, &pa, states, actions, rewards, eps, loc, std_, sample_actions, scores_low, nullptr, nullptr, stream));
    CHK(cert_first_pass(h, S));
    return cert_resolve_step(h, S, rec, with_eval ? erec : nullptr);
}

int m3pc_plan_step_certified(m3pc_handle* h, const m3pc_plan_args* a, const m3pc_cert_args* c, const float* states, const float* actions,
                             const float* rewards, const float* eps, const float* expo, float* loc, float* std_, float* sample_actions,
                             float* scores_low, float* merged, int* list, float* p, float* eval_action, int* argmax, int* sample_idx,
                             float* sample_action, m3pc_cert_record* rec, void* stream) {
    return cert_step_serial(h, a, c, states, actions, rewards, eps, expo, loc, std_, sample_actions, scores_low, merged, list, p, eval_action,
                            argmax, sample_idx, sample_action, rec, false, 0.f, nullptr, stream, "m3pc_plan_step_certified");
}

int m3pc_plan_step_certified_eval(m3pc_handle* h, const m3pc_plan_args* a, const m3pc_cert_args* c, const float* states,
                                  const float* actions, const float* rewards, const float* eps, const float* expo, float* loc, float* std_,
                                  float* sample_actions, float* scores_low, float* merged, int* list, float* p, float* eval_action,
                                  int* argmax, int* sample_idx, float* sample_action, m3pc_cert_record* rec, float eval_tol,
                                  m3pc_eval_record* erec, void* stream) {
    return cert_step_serial(h, a, c, states, actions, rewards, eps, expo, loc, std_, sample_actions, scores_low, merged, list, p, eval_action,
                            argmax, sample_idx, sample_action, rec, true, eval_tol, erec, stream, "m3pc_plan_step_certified_eval");
}

// ---- the certified step in two halves: _begin enqueues, _end resolves (include/m3pc_hip.h: "Pipelined certified steps")
int m3pc_set_step_streams(m3pc_handle* h, void* chain0, void* chain1) {
    if (!h) return fail(M3PC_EINVAL, "null handle");
    if ((chain0 == nullptr) != (chain1 == nullptr) || (chain0 && chain0 == chain1))
        return fail(M3PC_EINVAL, "m3pc_set_step_streams takes two different streams, or two NULLs");
    if (cert_any_begun(h)) return fail(M3PC_ESTATE, "m3pc_set_step_streams with a step begun");
    if (h->step_chain_own) {
        HIPCHK(hipSetDevice(h->device));
        for (int i = 0; i < 2; ++i) {
            HIPCHK(hipStreamSynchronize(h->step_chain[i]));
            HIPCHK(hipStreamDestroy(h->step_chain[i]));
        }
    }
    h->step_chain_own = false;
    h->step_chain[0] = (hipStream_t)chain0;
    h->step_chain[1] = (hipStream_t)chain1;
    return 0;
}
static int step_setup(m3pc_handle* h) {
    if (!h->step_chain[0]) {
        for (int i = 0; i < 2; ++i) {
            HIPCHK(hipStreamCreateWithFlags(&h->step_chain[i], hipStreamNonBlocking));
            ++h->step_streams_created;
        }
        h->step_chain_own = true;
    }
    if (!h->ev_excl) {
        for (int s = 0; s < M3PC_SLOTS; ++s)
            for (int i = 0; i < 4; ++i) HIPCHK(hipEventCreateWithFlags(&h->step_ev[s][i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&h->ev_excl, hipEventDisableTiming));
    }
    return 0;
}
// the tail of a begun step on its chain stream: behind its candidate pass (every part: m3pc_candidate_join), then the first pass
static int step_enqueue_tail(m3pc_handle* h, int slot) {
    CertStep& S = h->cstep[slot];
    HIPCHK(hipStreamWaitEvent(S.tail, h->step_ev[slot][2], 0));
    CHK(m3pc_candidate_join(h, slot, S.tail));
    S.tail_pending = false;
    CHK(cert_first_pass(h, S));
    if (S.eval_tol > 0.f && S.a.precision != M3PC_PREC_FP32) {
        // _eval_begin: the bound goes out right behind the first pass, for the state that pass assumes; _eval_end takes its
        // statistics when the two certificates are satisfied at their first read (StepOps::eval_read), without a second wait
        const int N = S.a.n_total;
        S.spec_n_listed = S.c.kmax < N ? S.c.kmax : N;
        CHK(cert_eval_launch(h, S, S.c.rfirst, S.c.kmin, S.spec_n_listed, S.c.delta, &S.spec_seq));
        S.spec_rounds = S.rounds;
        S.spec = true;
    }
    HIPCHK(hipEventRecord(h->step_ev[slot][3], S.tail));
    return 0;
}

// _begin; with_eval: m3pc_plan_step_certified_eval_begin (eval_tol)
static int cert_step_begin(m3pc_handle* h, const m3pc_plan_args* a, const m3pc_cert_args* c, const float* states, const float* actions,
                           const float* rewards, const float* eps, const float* expo, float* loc, float* std_, float* sample_actions,
                           float* scores_low, float* merged, int* list, float* p, float* eval_action, int* argmax, int* sample_idx,
                           float* sample_action, bool with_eval, float eval_tol, void* stream, const char* who) {
    if (!h || !a || !c || !states || !actions || !rewards || !eps || !expo || !sample_actions || !scores_low || !merged)
        return fail(M3PC_EINVAL, "null argument");
    CHK(cert_check_step(a, c, who));
    if (with_eval && !(eval_tol > 0.f)) return fail(M3PC_EINVAL, "%s: eval_tol must be > 0 (+inf: report only)", who);
    const int slot = a->slot;
    CertStep& S = h->cstep[slot];
    if (S.begun) return fail(M3PC_ESTATE, "%s: the step in slot %d has not been ended", who, slot);
    HIPCHK(hipSetDevice(h->device));
    CHK(step_setup(h));
    if (with_eval && a->precision != M3PC_PREC_FP32) CHK(eval_host_setup(h));
    hipStream_t st = (hipStream_t)stream, chain = h->step_chain[slot & 1];
    hipEvent_t* ev = h->step_ev[slot];
    // the window is complete in `stream` order: the chain stream reads it behind ev_in (M3PC_PLAN_INPUTS_READY: complete already)
    if (!(a->flags & M3PC_PLAN_INPUTS_READY)) {
        HIPCHK(hipEventRecord(ev[0], st));
        HIPCHK(hipStreamWaitEvent(chain, ev[0], 0));
    }
    m3pc_plan_args pa = *a;
    pa.flags = a->flags & M3PC_PLAN_PRUNED_POLICY;
    pa.window = 0;
    CHK(m3pc_policy_pass(h, &pa, states, actions, rewards, nullptr, nullptr, chain));
    HIPCHK(hipEventRecord(ev[1], chain));
    // the pending-tail rule: the tails of the earlier steps of this parity go behind this step's policy pass, oldest first
    for (;;) {
        int o = -1;
        for (int s = 0; s < M3PC_SLOTS; ++s)
            if ((s & 1) == (slot & 1) && h->cstep[s].begun && h->cstep[s].tail_pending && (o < 0 || h->cstep[s].order < h->cstep[o].order))
                o = s;
        if (o < 0) break;
        CHK(step_enqueue_tail(h, o));
    }
    // the candidate pass on the caller's stream: behind the policy pass, behind what overflowed into the candidate workspace, and
    // behind the candidate pass enqueued last (free when the caller plans on one stream)
    HIPCHK(hipStreamWaitEvent(st, ev[1], 0));
    if (h->excl_valid) HIPCHK(hipStreamWaitEvent(st, h->ev_excl, 0));
    if (h->cand_last_slot >= 0) HIPCHK(hipStreamWaitEvent(st, h->step_ev[h->cand_last_slot][2], 0));
    pa.flags = M3PC_PLAN_DEFER_JOIN;
    CHK(m3pc_candidate_pass(h, &pa, states, actions, rewards, eps, loc, std_, sample_actions, scores_low, nullptr, nullptr, stream));
    HIPCHK(hipEventRecord(ev[2], st));
    h->cand_last_slot = slot;
    cert_fill(S, a, c, states, actions, rewards, eps, expo, sample_actions, scores_low, merged, list, p, eval_action, argmax, sample_idx,
              sample_action, chain, true, with_eval ? eval_tol : 0.f);
    S.tail_pending = true;
    S.begun = true;
    S.order = ++h->step_order;
    return 0;
}
int m3pc_plan_step_certified_begin(m3pc_handle* h, const m3pc_plan_args* a, const m3pc_cert_args* c, const float* states,
                                   const float* actions, const float* rewards, const float* eps, const float* expo, float* loc, float* std_,
                                   float* sample_actions, float* scores_low, float* merged, int* list, float* p, float* eval_action,
                                   int* argmax, int* sample_idx, float* sample_action, void* stream) {
    return cert_step_begin(h, a, c, states, actions, rewards, eps, expo, loc, std_, sample_actions, scores_low, merged, list, p, eval_action,
                           argmax, sample_idx, sample_action, false, 0.f, stream, "m3pc_plan_step_certified_begin");
}
int m3pc_plan_step_certified_eval_begin(m3pc_handle* h, const m3pc_plan_args* a, const m3pc_cert_args* c, const float* states,
                                        const float* actions, const float* rewards, const float* eps, const float* expo, float* loc,
                                        float* std_, float* sample_actions, float* scores_low, float* merged, int* list, float* p,
                                        float* eval_action, int* argmax, int* sample_idx, float* sample_action, float eval_tol,
                                        void* stream) {
    return cert_step_begin(h, a, c, states, actions, rewards, eps, expo, loc, std_, sample_actions, scores_low, merged, list, p, eval_action,
                           argmax, sample_idx, sample_action, true, eval_tol, stream, "m3pc_plan_step_certified_eval_begin");
}

// _end; erec: m3pc_plan_step_certified_eval_end -- the step must have been begun with _eval_begin (it carries the tolerance)
static int cert_step_end(m3pc_handle* h, int slot, m3pc_cert_record* rec, bool with_eval, m3pc_eval_record* erec, void* stream,
                         const char* who) {
    if (!h || !rec || (with_eval && !erec)) return fail(M3PC_EINVAL, "null argument");
    if (slot < 0 || slot >= M3PC_SLOTS) return fail(M3PC_EINVAL, "slot %d outside [0, %d)", slot, M3PC_SLOTS);
    CertStep& S = h->cstep[slot];
    if (!S.begun) return fail(M3PC_ESTATE, "%s: no step begun in slot %d", who, slot);
    if (with_eval && !(S.eval_tol > 0.f))
        return fail(M3PC_ESTATE, "%s: the step in slot %d was begun without an eval_tol (m3pc_plan_step_certified_end resolves it)", who, slot);
    HIPCHK(hipSetDevice(h->device));
    S.begun = false;  // (whatever happens below, the slot is free again)
    if (S.tail_pending) CHK(step_enqueue_tail(h, slot));
    const int rounds = S.rounds;
    CHK(cert_resolve_step(h, S, rec, with_eval ? erec : nullptr));
    if (S.rounds != rounds) HIPCHK(hipEventRecord(h->step_ev[slot][3], S.tail));
    HIPCHK(hipStreamWaitEvent((hipStream_t)stream, h->step_ev[slot][3], 0));
    return 0;
}
int m3pc_plan_step_certified_end(m3pc_handle* h, int slot, m3pc_cert_record* rec, void* stream) {
    return cert_step_end(h, slot, rec, false, nullptr, stream, "m3pc_plan_step_certified_end");
}
int m3pc_plan_step_certified_eval_end(m3pc_handle* h, int slot, m3pc_cert_record* rec, m3pc_eval_record* erec, void* stream) {
    return cert_step_end(h, slot, rec, true, erec, stream, "m3pc_plan_step_certified_eval_end");
}

// ---- a lock-step batch of certified plan steps as one call (include/m3pc_hip.h: m3pc_plan_steps_certified): the order of
// m3pc_amd/lockstep.py with the batched kernels of select.hip around ONE fp32 scoring pass, then certificate.py:resolve per window
using Lockstep = m3pc_handle::Lockstep;
static const int LS_ROW = 64 + 1024;  // list entries a window can hold (rmax <= 64 in front of 1024)
static int ls_setup(m3pc_handle* h) {
    Lockstep& W = h->ls;
    if (W.ready) return 0;
    const size_t E = (size_t)(h->dm.max_batch > 0 ? h->dm.max_batch : 1);
    W.cand_rows = h->dm.max_candidates > h->chain[0].max_cand ? h->dm.max_candidates : h->chain[0].max_cand;
    if (!W.list) CHK(dmalloc(&W.list, E * LS_ROW));
    if (!W.b) CHK(dmalloc(&W.b, E * LS_ROW));
    if (!W.f) CHK(dmalloc(&W.f, E * LS_ROW));
    if (!W.stats) CHK(dmalloc(&W.stats, E * 24));
    if (!W.cand) CHK(dmalloc(&W.cand, (size_t)W.cand_rows * h->T * h->A));
    if (!W.fs) CHK(dmalloc(&W.fs, (size_t)W.cand_rows));
    if (!W.widx) CHK(dmalloc(&W.widx, (size_t)W.cand_rows));
    if (!W.host) {
        HIPCHK(hipHostMalloc((void**)&W.host, E * 8 * sizeof(float), hipHostMallocMapped | hipHostMallocCoherent));
        memset(W.host, 0, E * 8 * sizeof(float));
        HIPCHK(hipHostGetDevicePointer((void**)&W.host_dev, W.host, 0));
    }
    // (the eval_action certificate of m3pc_plan_steps_certified_eval: eight statistics per window, device and host-mapped)
    if (!W.estats) CHK(dmalloc(&W.estats, E * 8));
    if (!W.ehost) {
        HIPCHK(hipHostMalloc((void**)&W.ehost, E * 8 * sizeof(float), hipHostMallocMapped | hipHostMallocCoherent));
        memset(W.ehost, 0, E * 8 * sizeof(float));
        HIPCHK(hipHostGetDevicePointer((void**)&W.ehost_dev, W.ehost, 0));
    }
    W.seq_w.assign(E, 0.f);
    W.ready = true;
    return 0;
}
static float ls_next_seq(Lockstep& W) {
    W.seq = W.seq % 1000000 + 1;
    return (float)W.seq;
}
// The device work of cert_resolve (cert_resolve.h) for window w of a lock-step batch: certificate.py's _WindowOps.  The arrays
// are the batch's, as m3pc_plan_steps_certified got them (window w at + w of each); L / B / F: rows of LS list entries.
struct LsOps {
    m3pc_handle* h;
    m3pc_plan_args sa;  // an fp32 scoring call of gathered rows (m3pc_score_actions); n_total / n_count per call
    const float *states, *actions, *rewards, *expo;
    float *sample_actions, *scores_low, *merged, *p, *eval_action, *sample_action, *B, *F;
    int *L, *argmax, *sample_idx;
    int N, R, LS;
    long long row;
    float temp;
    hipStream_t st;
    m3pc_cert_record* records;  // (rounds: the merges issued for a window)
    const float* first;         // the statistics of the first pass's merge, 8 per window, on the host already
    int w;
    bool have;  // first + 8 w are still the statistics of the window's last merge
    CertState cs;
    // m3pc_plan_steps_certified_eval: the tolerance, and whether the window's block of the batched bound launch (r = rfirst,
    // n = kmin, n_listed = spec_n_listed, delta = spec_delta, closed by spec_seq) may still stand for the window's bound
    float eval_tol = 0.f, spec_delta = 0.f, spec_seq = 0.f;
    int spec_n_listed = 0;
    bool spec = false;

    int* Lw() const { return L + (size_t)w * LS; }
    float* Bw() const { return B + (size_t)w * LS; }
    float* Fw() const { return F + (size_t)w * LS; }
    const float* low() const { return scores_low + (size_t)w * N; }
    float* mw() const { return merged + (size_t)w * N; }
    float* scratch() const { return h->ls.stats + 8 * (size_t)h->dm.max_batch + 16 * (size_t)w; }
    float next_seq() { return h->ls.seq_w[w] = ls_next_seq(h->ls); }
    int select(const float* er) {
        const int A = h->A;
        return m3pc_select(h, er, sample_actions + w * N * row, row, N, temp, expo + (size_t)w * N, p ? p + (size_t)w * N : nullptr,
                           eval_action ? eval_action + (size_t)w * A : nullptr, argmax ? argmax + w : nullptr,
                           sample_idx ? sample_idx + w : nullptr, sample_action ? sample_action + (size_t)w * A : nullptr, st);
    }
    int rescore(int lo, int hi) {  // _WindowOps._score: list positions [lo, hi), chunks of max_rescore
        const int cap = h->chain[0].max_cand, T = h->T, S = h->S, A = h->A;
        for (int c0 = lo; c0 < hi; c0 += cap) {
            const int m = hi - c0 < cap ? hi - c0 : cap;
            launch_gather_listed(sample_actions + w * N * row, 1, N, (int)row, Lw(), LS, c0, m, h->ls.cand, nullptr, st);
            sa.n_total = sa.n_count = m;
            CHK(m3pc_score_actions(h, &sa, 1, states + (size_t)w * T * S, actions + (size_t)w * T * A, rewards + (size_t)w * T, h->ls.cand,
                                   nullptr, Fw() + c0, nullptr, nullptr, st));
        }
        return 0;
    }

    int read(bool four_only, float* out8) {
        if (have) {
            have = false;
            memcpy(out8, first + 8 * (size_t)w, 8 * sizeof(float));
            return 0;
        }
        Lockstep& W = h->ls;
        return cert_wait_blocks(W.host + 8 * w, W.stats + 8 * w, &W.seq_w[w], 1, four_only ? 4 : 8, st, out8);
    }
    // The bound behind the window's last merge + select.  The batched launch behind the batched merge is that launch exactly when
    // the window has issued no merge of its own (an earlier window's raised delta makes it merge again first); otherwise the
    // one-window kernel behind its last merge, and a wait.
    int eval_read(int n_listed, float* out8) {
        Lockstep& W = h->ls;
        float seq = spec_seq;
        const bool take = spec && records[w].rounds == 1 && n_listed == spec_n_listed && (float)cs.delta == spec_delta;
        spec = false;
        if (!take) {
            W.eseq = W.eseq % 1000000 + 1;
            seq = (float)W.eseq;
            const int r = cs.r_done;
            CHK(m3pc_eval_bound(h, mw(), N, Lw() + R - r, r, cs.n_done, n_listed, sample_actions + w * N * row, row, h->A, temp, (float)cs.delta,
                                eval_tol, W.estats + 8 * (size_t)w, W.ehost_dev + 8 * (size_t)w, seq, st));
        }
        return cert_wait_blocks(W.ehost + 8 * w, W.estats + 8 * w, &seq, 1, 8, st, out8);
    }
    int extend(int lo, int hi) { return rescore(R + lo, R + hi); }
    int extend_race(int lo, int hi) { return rescore(R - hi, R - lo); }
    int merge_select() {
        const int n = cs.n_done, r = cs.r_done, o = R - r, A = h->A;
        float *dst = h->ls.stats + 8 * (size_t)w, *hst = h->ls.host_dev + 8 * (size_t)w;
        const float seq = next_seq();
        ++records[w].rounds;
        if (R > 0)
            return m3pc_merge_race_select(h, low(), expo + (size_t)w * N, temp, N, Lw() + o, r, n, Bw() + o, Fw() + o, (float)cs.delta, mw(), dst,
                                          hst, seq, sample_actions + w * N * row, row, p ? p + (size_t)w * N : nullptr,
                                          eval_action ? eval_action + (size_t)w * A : nullptr, argmax ? argmax + w : nullptr,
                                          sample_idx ? sample_idx + w : nullptr, sample_action ? sample_action + (size_t)w * A : nullptr, st);
        CHK(m3pc_rescore_merge(h, low(), N, Lw(), n, Bw(), Fw(), (float)cs.delta, mw(), dst, hst, seq, st));
        return select(mw());
    }
    int window_set(int need, bool everything) {
        const int cnt = need < N ? need : N, T = h->T, S = h->S, A = h->A;
        if (cnt <= 1024 - 32 && !everything) {
            if (!launch_topk_race(low(), nullptr, 0.f, N, cnt, 0, R, Lw(), Bw(), st))
                launch_window_stats(low(), N, Lw() + R, cnt, 1, cnt, 0.f, scratch(), nullptr, 0.f, Bw() + R, st, 0);
            CHK(check_launch("plan_steps_certified (window set)"));
            CHK(rescore(R, R + cnt));
            cs.n_done = cnt;
            return merge_select();
        }
        float* f32 = h->cert_f32[sa.slot];
        int* top1 = h->cert_top1[sa.slot];
        float* top1v = scratch() + 8;
        sa.n_total = sa.n_count = N;
        CHK(m3pc_score_actions(h, &sa, 1, states + (size_t)w * T * S, actions + (size_t)w * T * A, rewards + (size_t)w * T,
                               sample_actions + w * N * row, nullptr, f32, nullptr, nullptr, st));
        if (!launch_topk_race(f32, nullptr, 0.f, N, 1, 0, 0, top1, top1v, st))
            launch_window_stats(f32, N, top1, 1, 1, 1, 0.f, scratch(), nullptr, 0.f, top1v, st, 0);
        CHK(check_launch("plan_steps_certified (every candidate in fp32)"));
        cs.n_done = N;  // (r_done stays: the record's n_race is what the loop counted, as in the Python protocol)
        const float seq = next_seq();
        ++records[w].rounds;
        CHK(m3pc_rescore_merge(h, f32, N, top1, 1, top1v, top1v, 0.f, mw(), h->ls.stats + 8 * (size_t)w, h->ls.host_dev + 8 * (size_t)w, seq, st));
        return select(mw());
    }
};

// the lock-step batch; with_eval: m3pc_plan_steps_certified_eval (eval_tol, erecs)
static int ls_steps(m3pc_handle* h, const m3pc_plan_args* a, const m3pc_cert_args* c, int n_windows, const float* states,
                    const float* actions, const float* rewards, const double* rtg, const float* eps, const float* expo, float* loc,
                    float* std_, float* sample_actions, float* scores_low, float* merged, int* list, float* p, float* eval_action,
                    int* argmax, int* sample_idx, float* sample_action, m3pc_cert_record* records, bool with_eval, float eval_tol,
                    m3pc_eval_record* erecs, void* stream, const char* who) {
    if (!h || !a || !c || !states || !actions || !rewards || !rtg || !eps || !expo || !sample_actions || !scores_low || !merged || !records ||
        (with_eval && !erecs))
        return fail(M3PC_EINVAL, "null argument");
    if (with_eval && !(eval_tol > 0.f)) return fail(M3PC_EINVAL, "%s: eval_tol must be > 0 (+inf: report only)", who);
    if (n_windows < 1) return fail(M3PC_EINVAL, "%s: n_windows %d < 1", who, n_windows);
    if (a->returns) return fail(M3PC_EINVAL, "%s takes rtg per window, not a returns row (args->returns must be NULL)", who);
    CHK(cert_check_step(a, c, who));
    if (a->mode < 0 || a->mode > 2) return fail(M3PC_EINVAL, "bad mode %d", a->mode);
    // from here on the handle is read
    const int E = n_windows;
    if (E > h->dm.max_batch) return fail(M3PC_EINVAL, "%s: n_windows %d > max_batch=%d", who, E, h->dm.max_batch);
    if (cert_any_begun(h)) return fail(M3PC_ESTATE, "%s with a pipelined step begun (m3pc_plan_step_certified_end first)", who);
    if (a->mode != M3PC_MODE_RTG && !h->critic_set) return fail(M3PC_ESTATE, "critic weights not set");
    if (a->precision != M3PC_PREC_FP32) {  // (the rows one scoring call can take: what ls_setup sizes the gathered rows by)
        const long long rows = h->dm.max_candidates > h->chain[0].max_cand ? h->dm.max_candidates : h->chain[0].max_cand;
        if ((long long)n_windows * (c->rfirst + c->kmin) > rows)
            return fail(M3PC_ENOMEM, "%s: the first pass re-scores %d x %d candidates, more than max(max_candidates, max_rescore)=%lld", who,
                        n_windows, c->rfirst + c->kmin, rows);
    }
    HIPCHK(hipSetDevice(h->device));
    CHK(ls_setup(h));
    Lockstep& W = h->ls;
    hipStream_t st = (hipStream_t)stream;
    const int N = a->n_total, T = h->T, S = h->S, A = h->A, hz = a->horizon, slot = a->slot;
    const long long row = (long long)hz * A, eps_w = (long long)N * (a->mode == M3PC_MODE_NOISE ? hz : T) * A;
    const float temp = c->temperature;
    memset(records, 0, (size_t)E * sizeof(*records));
    if (with_eval) memset(erecs, 0, (size_t)E * sizeof(*erecs));

    // lockstep.py:57-62: ONE policy pass at batch E, every window's own candidate pass back to back, one join
    m3pc_plan_args pa = *a;
    pa.flags = 0;
    pa.window = 0;
    CHK(m3pc_policy_pass_batch(h, &pa, E, states, actions, rewards, rtg, nullptr, nullptr, stream));
    pa.flags = M3PC_PLAN_DEFER_JOIN;
    for (int w = 0; w < E; ++w) {
        pa.window = w;
        CHK(m3pc_candidate_pass(h, &pa, states + (size_t)w * T * S, actions + (size_t)w * T * A, rewards + (size_t)w * T, eps + w * eps_w,
                                loc ? loc + (size_t)w * T * A : nullptr, std_ ? std_ + (size_t)w * T * A : nullptr, sample_actions + w * N * row,
                                scores_low + (size_t)w * N, nullptr, nullptr, stream));
    }
    CHK(m3pc_candidate_join(h, slot, stream));

    SelectP sel;  // window 0's select; window w at + w of every array
    memset(&sel, 0, sizeof(sel));
    sel.a0 = sample_actions;
    sel.a0_stride = row;
    sel.n = N;
    sel.A = A;
    sel.temperature = temp;
    sel.expo = expo;
    sel.p = p;
    sel.eval_action = eval_action;
    sel.argmax = argmax;
    sel.sample_idx = sample_idx;
    sel.sample_action = sample_action;
    if (a->precision == M3PC_PREC_FP32) {  // fp32 scores for every candidate: the select alone, all windows in one launch
        HIPCHK(hipMemcpyAsync(merged, scores_low, (size_t)E * N * sizeof(float), hipMemcpyDeviceToDevice, st));
        sel.er = scores_low;
        launch_select_batch(sel, E, N, N * row, st);
        for (int w = 0; w < E; ++w) {
            cert_record_fp32(N, records + w);
            if (with_eval) erecs[w].eval_certified = 1;
        }
        return check_launch(who);
    }

    const int R = c->rmax, kmin = c->kmin, kmax = c->kmax, rfirst = c->rfirst, LS = R + 1024, m0 = rfirst + kmin;
    const int kk = kmax + 1 < N ? kmax + 1 : N;
    int* L = list ? list : W.list;  // rows of LS entries, as are B and F
    float *B = W.b, *F = W.f;
    LsOps O;  // the one-window work behind the batched launches: window O.w
    O.h = h;
    O.states = states;
    O.actions = actions;
    O.rewards = rewards;
    O.expo = expo;
    O.sample_actions = sample_actions;
    O.scores_low = scores_low;
    O.merged = merged;
    O.p = p;
    O.eval_action = eval_action;
    O.sample_action = sample_action;
    O.B = B;
    O.F = F;
    O.L = L;
    O.argmax = argmax;
    O.sample_idx = sample_idx;
    O.N = N;
    O.R = R;
    O.LS = LS;
    O.row = row;
    O.temp = temp;
    O.st = st;
    O.records = records;
    // lockstep.py:93-100: the lists of every window (the kmax + 1 best by score, the rmax best by race key) in one launch
    if (!launch_topk_race_batch(scores_low, expo, temp, E, N, N, kk, R, R, L, B, LS, st)) {
        for (O.w = 0; O.w < E; ++O.w)  // (the device refused the LDS of the batched ranking: the one-window launches, same lists)
            if (!launch_topk_race(O.low(), R > 0 ? expo + (size_t)O.w * N : nullptr, temp, N, kk, R, R, O.Lw(), O.Bw(), st))
                launch_window_stats(O.low(), N, O.Lw() + R, kk, kmin, kmax, 0.f, O.scratch(), nullptr, 0.f, O.Bw() + R, st, R);
    }
    // lockstep.py:106-110: list positions [rmax - rfirst, rmax + kmin) of every window, window-major, in ONE fp32 scoring pass
    launch_gather_listed(sample_actions, E, N, (int)row, L, LS, R - rfirst, m0, W.cand, W.widx, st);
    CHK(check_launch(who));
    m3pc_plan_args& sa = O.sa = *a;
    sa.mode = a->mode == M3PC_MODE_RTG ? M3PC_MODE_RTG : M3PC_MODE_CRITIC;
    sa.precision = M3PC_PREC_FP32;
    sa.flags = 0;
    sa.window = 0;
    sa.n_begin = 0;
    sa.n_total = sa.n_count = E * m0;
    CHK(m3pc_score_actions(h, &sa, E, states, actions, rewards, W.cand, W.widx, W.fs, nullptr, nullptr, stream));
    // lockstep.py:111-123: merge + certificates + select of every window in one launch, the statistics to the windows' host blocks
    std::vector<int> n_done(E, kmin), r_done(E, rfirst);
    std::vector<float> d0(E, c->delta), s8((size_t)E * 8);
    const float seq0 = ls_next_seq(W);
    MergeSelectBatchP P;
    memset(&P, 0, sizeof(P));
    P.b = scores_low;
    P.expo = expo;
    P.row_stride = N;
    P.n_total = N;
    P.race = R > 0;
    P.select = 1;
    P.tau = temp;
    P.list = L;
    P.list_scores = B;
    P.list_stride = LS;
    P.rmax = R;
    P.f = W.fs;
    P.f_stride = m0;
    P.f_lo = R - rfirst;
    P.out = merged;
    P.stats = W.stats;
    P.host_stats = W.host_dev;
    P.seq = seq0;
    P.a0 = sample_actions;
    P.a0_wstride = N * row;
    P.a0_stride = row;
    P.A = A;
    P.p = p;
    P.eval_action = eval_action;
    P.argmax = argmax;
    P.sample_idx = sample_idx;
    P.sample_action = sample_action;
    launch_merge_select_batch(P, E, r_done.data(), n_done.data(), d0.data(), st);
    O.eval_tol = eval_tol;
    if (with_eval) {
        // the bound of every window behind the batched merge, for the state it assumes: a window whose certificates are satisfied
        // at their first read takes its block (LsOps::eval_read) -- no launch and, as a rule, no wait of its own
        EvalBoundBatchP Q;
        memset(&Q, 0, sizeof(Q));
        Q.m = merged;
        Q.n_total = N;
        Q.list = L;
        Q.list_stride = LS;
        Q.rmax = R;
        Q.n_listed = O.spec_n_listed = kmax < N ? kmax : N;
        Q.a0 = sample_actions;
        Q.a0_wstride = N * row;
        Q.a0_stride = row;
        Q.A = A;
        Q.tau = temp;
        Q.eval_tol = eval_tol;
        Q.stats = W.estats;
        Q.host_stats = W.ehost_dev;
        W.eseq = W.eseq % 1000000 + 1;
        Q.seq = O.spec_seq = (float)W.eseq;
        O.spec_delta = c->delta;
        launch_eval_bound_batch(Q, E, r_done.data(), n_done.data(), d0.data(), st);
    }
    for (int w = 0; w < E; ++w) {
        W.seq_w[w] = seq0;
        records[w].rounds = 1;
    }
    // (the re-scores into the list's layout, where the one-window merges behind the certificates read them)
    HIPCHK(hipMemcpy2DAsync(F + (R - rfirst), (size_t)LS * sizeof(float), W.fs, (size_t)m0 * sizeof(float), (size_t)m0 * sizeof(float), E,
                            hipMemcpyDeviceToDevice, st));
    CHK(check_launch(who));
    CHK(cert_wait_blocks(W.host, W.stats, W.seq_w.data(), E, R > 0 ? 8 : 4, st, s8.data()));  // the ONE host wait of the first pass: E sequence numbers

    // ---- per window, ascending: the loop of cert_resolve.h with the device work of LsOps.  delta goes from one window to the next.
    O.first = s8.data();
    double delta = (double)c->delta;
    const double delta_first = delta;
    for (int w = 0; w < E; ++w) {
        O.w = w;
        O.have = true;
        O.cs = CertState(N, kmax, R, c->grow_delta != 0, kmin, rfirst, delta);
        if (delta > delta_first) {  // an earlier window raised the bound: this window's certificate again, under it
            CHK(O.merge_select());
            O.have = false;
        }
        if (with_eval) {
            O.spec = true;
            EvalState es(eval_tol);
            CHK(cert_resolve_eval(O.cs, O, es));
            cert_eval_record(es, erecs + w);
        } else {
            CHK(cert_resolve(O.cs, O));
        }
        delta = O.cs.delta;
        cert_record(O.cs, records + w);
    }
    return 0;
}
int m3pc_plan_steps_certified(m3pc_handle* h, const m3pc_plan_args* a, const m3pc_cert_args* c, int n_windows, const float* states,
                              const float* actions, const float* rewards, const double* rtg, const float* eps, const float* expo,
                              float* loc, float* std_, float* sample_actions, float* scores_low, float* merged, int* list, float* p,
                              float* eval_action, int* argmax, int* sample_idx, float* sample_action, m3pc_cert_record* records,
                              void* stream) {
    return ls_steps(h, a, c, n_windows, states, actions, rewards, rtg, eps, expo, loc, std_, sample_actions, scores_low, merged, list, p,
                    eval_action, argmax, sample_idx, sample_action, records, false, 0.f, nullptr, stream, "m3pc_plan_steps_certified");
}
int m3pc_plan_steps_certified_eval(m3pc_handle* h, const m3pc_plan_args* a, const m3pc_cert_args* c, int n_windows, const float* states,
                                   const float* actions, const float* rewards, const double* rtg, const float* eps, const float* expo,
                                   float* loc, float* std_, float* sample_actions, float* scores_low, float* merged, int* list, float* p,
                                   float* eval_action, int* argmax, int* sample_idx, float* sample_action, m3pc_cert_record* records,
                                   float eval_tol, m3pc_eval_record* erecs, void* stream) {
    return ls_steps(h, a, c, n_windows, states, actions, rewards, rtg, eps, expo, loc, std_, sample_actions, scores_low, merged, list, p,
                    eval_action, argmax, sample_idx, sample_action, records, true, eval_tol, erecs, stream, "m3pc_plan_steps_certified_eval");
}

// HipPlanner._calibrate as a call: delta from ONE full fp32 candidate pass over the step's candidates
int m3pc_calibrate_delta(m3pc_handle* h, const m3pc_plan_args* a, const float* states, const float* actions, const float* rewards,
                         const float* eps, const float* scores_low, float factor, float* delta_out, void* stream) {
    if (!h || !a || !states || !actions || !rewards || !eps || !scores_low || !delta_out) return fail(M3PC_EINVAL, "null argument");
    CHK(cert_check_args(a, "m3pc_calibrate_delta"));
    if (!(factor > 0.f)) return fail(M3PC_EINVAL, "factor must be > 0");
    if (cert_any_begun(h)) return fail(M3PC_ESTATE, "m3pc_calibrate_delta with a pipelined step begun (m3pc_plan_step_certified_end first)");
    hipStream_t st = (hipStream_t)stream;
    const int N = a->n_total;
    m3pc_plan_args fa = *a;
    fa.precision = M3PC_PREC_FP32;
    fa.flags = 0;
    fa.window = 0;
    float* f32 = h->cert_f32[a->slot];
    CHK(m3pc_candidate_pass(h, &fa, states, actions, rewards, eps, nullptr, nullptr, h->sa_buf, f32, nullptr, nullptr, stream));
    const float seq = cert_next_seq(h, a->slot);
    launch_deviation_stats(scores_low, f32, N, h->cert_stats[a->slot], h->cert_host_dev + 8 * a->slot, seq, st);
    CHK(check_launch("calibrate_delta"));
    float s8[8];
    CHK(cert_wait(h, a->slot, seq, 8, st, s8));
    *delta_out = cert_delta(factor, s8[1], s8[2]);
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
