// libm3pc_hip_lab.so only (m3pc_amd/build.py: LAB_SOURCES): the kernel-level test / bench hooks declared in
// include/m3pc_hip_debug.h.  The product build does not compile this file.
#include "m3pc_internal.h"
#include "mtm_grad.h"
#include "iql.h"
#include "mtm_opt.h"

#include <vector>

#pragma GCC visibility push(default)
extern "C" {

// streams the handle created for its pipelined certified steps (0 while the caller's pair of m3pc_set_step_streams serves them)
int m3pc_debug_step_streams_created(m3pc_handle* h) { return h ? h->step_streams_created : -1; }
// Lab build only (include/m3pc_hip_debug.h): lets tools/gemm_bench.py time the GEMM kernel on the plan step's shapes.
int m3pc_debug_gemm(int dtype, const void* A, const void* Wt, const float* bias, const float* res, void* C, int M, int N,
                    int K, int gelu, int f32out, int variant, void* stream) {
    static const int ldpad = M3PC_ENV("M3PC_DEBUG_LDPAD") ? atoi(M3PC_ENV("M3PC_DEBUG_LDPAD")) : 0;  // operand row padding (elements)
    GemmP p = gemm_basic(A, K + ldpad, Wt, K + ldpad, M, N, K, bias);
    p.a_padded = 0;  // (a caller's tensor: nothing is known about the memory behind it)
    p.gelu = gelu;
    p.res = res;
    p.ldr = N;
    p.variant = variant;
    if (dtype == DT_BF16 && !f32out)
        p.Cb = (bf16_t*)C;
    else
        p.Cf = (float*)C;
    p.ldc = N;
    if (dtype != DT_BF16 && variant != 1) {  // split-K workspace as the handle provides it (variant 1: none)
        static float* ws = nullptr;
        if (!ws) HIPCHK(hipMalloc((void**)&ws, 64 << 20));
        p.ws = ws;
        p.ws_bytes = 64 << 20;
    }
    if (dtype == DT_X3) {  // A fp32, Wt fp32: split into hi / lo bf16 copies here, as m3pc_load_weights splits the weights
        static bf16_t* wsplit = nullptr;
        static size_t cap = 0;
        const size_t n = (size_t)N * (K + ldpad);
        if (n > cap) {
            if (wsplit) HIPCHK(hipFree(wsplit));
            wsplit = nullptr;
            cap = 0;
            HIPCHK(hipMalloc((void**)&wsplit, 2 * n * sizeof(bf16_t)));
            cap = n;
        }
        launch_f32_split_bf16((const float*)Wt, wsplit, wsplit + n, (long long)n, (hipStream_t)stream);
        p.W = wsplit;
        p.w_lo_off = (long long)n;
        if (launch_gemm_x3(p, (hipStream_t)stream) < 0) return fail(M3PC_EINVAL, "debug_gemm: shape not covered by the x3 kernel");
        return check_launch("debug_gemm");
    }
    launch_gemm(p, dtype, (hipStream_t)stream);
    return check_launch("debug_gemm");
}

// Every GEMM the library launches, on caller tensors, with everything a GemmP can carry (tests/test_gemm_edges_gpu.py).  The
// checks below are the shape rules of the register-staged kernel every problem can fall back to; what the dispatch would launch is
// learnt from a dry walk of the launchers (g_gemm_dry, csrc/kernels.h), so nothing reaches the GPU before the call is known to be
// covered.  Fills `p` (and, for dtype 2, nothing yet of W's split) or returns the error.
static int debug_gemm_fill(const m3pc_debug_gemm_args* a, GemmP& p) {
    if (!a) return fail(M3PC_EINVAL, "debug_gemm_ex: null argument");
    const int dt = a->dtype;
    if (dt != DT_F32 && dt != DT_BF16 && dt != DT_X3) return fail(M3PC_EINVAL, "debug_gemm_ex: dtype %d", dt);
    if (!a->A || !a->W || !a->C) return fail(M3PC_EINVAL, "debug_gemm_ex: null operand");
    if (a->M < 1 || a->M > (1 << 20) || a->N < 32 || a->N > (1 << 16) || a->K < 1 || a->K > (1 << 16)) return fail(M3PC_EINVAL, "debug_gemm_ex: M / N / K out of range");
    const int es = dt == DT_BF16 ? 2 : 4;  // bytes per element of A (x3: fp32 activations; its W copies are bf16)
    if (a->N % 32) return fail(M3PC_EINVAL, "debug_gemm_ex: N %d is not a multiple of 32 (columns would be dropped)", a->N);
    if (((long long)a->K * es) % 128) return fail(M3PC_EINVAL, "debug_gemm_ex: K %d is not a whole number of 128-byte k-tiles (k terms would be dropped)", a->K);
    if (dt == DT_F32 && !a->f32out) return fail(M3PC_EINVAL, "debug_gemm_ex: fp32 operands have fp32 output only");
    const int f32out = dt == DT_F32 || a->f32out;
    const int os = f32out ? 4 : 2;
    const uintptr_t ptrs = (uintptr_t)a->A | (uintptr_t)a->W | (uintptr_t)a->C | (uintptr_t)a->bias | (uintptr_t)a->rowtab | (uintptr_t)a->res |
                           (uintptr_t)a->ws | (uintptr_t)a->ln_g | (uintptr_t)a->ln_b | (uintptr_t)a->ln_out | (uintptr_t)a->a_ln_g |
                           (uintptr_t)a->a_ln_b;
    if (ptrs & 15) return fail(M3PC_EINVAL, "debug_gemm_ex: pointers must be 16-byte aligned");
    if (a->lda < a->K || a->ldw < a->K || a->ldc < a->N || (a->res && a->ldr < a->N) || (a->rowtab && a->rt_ld < a->N))
        return fail(M3PC_EINVAL, "debug_gemm_ex: a leading dimension is below its row length");
    // (x3: W's bf16 copies keep ldw, so their rows need ldw % 8 as well)
    if (((long long)a->lda * es) % 16 || ((long long)a->ldw * (dt == DT_F32 ? 4 : 2)) % 16 || (dt == DT_X3 && a->ldw % 4) || ((long long)a->ldc * os) % 16 ||
        (a->res && a->ldr % 4) || (a->rowtab && a->rt_ld % 4))
        return fail(M3PC_EINVAL, "debug_gemm_ex: rows of a leading dimension leave 16-byte alignment");
    if (a->rowtab && a->rt_mod < 1) return fail(M3PC_EINVAL, "debug_gemm_ex: rowtab with rt_mod %d", a->rt_mod);
    for (const int* m : {a->amap, a->cmap})
        if (m[0] < 0 || m[2] < 0 || (m[0] >= 1 && m[1] < m[0])) return fail(M3PC_EINVAL, "debug_gemm_ex: row map {%d, %d, %d}", m[0], m[1], m[2]);
    if (a->ws && a->ws_bytes < 0) return fail(M3PC_EINVAL, "debug_gemm_ex: negative ws_bytes");
    if (a->ln_out && (!f32out || !a->ln_g || !a->ln_b)) return fail(M3PC_EINVAL, "debug_gemm_ex: ln_out needs fp32 C, ln_g and ln_b");
    if ((a->a_ln_g != nullptr) != (a->a_ln_b != nullptr)) return fail(M3PC_EINVAL, "debug_gemm_ex: a_ln_g and a_ln_b go together");
    const int v = a->variant;
    if (!(v == 0 || (dt == DT_BF16 && (v == 2 || v == 26 || v == 37 || v == 43 || v == 44)) || (dt == DT_F32 && v == 2)))
        return fail(M3PC_EINVAL, "debug_gemm_ex: variant %d of dtype %d is not one this hook drives", v, dt);
    // (a_padded vouches for 127 rows behind A: a ragged 256-row tile of gemm_line_kernel<256>'s persistent form may need up to 255)
    if (v == 44 && a->a_padded && a->M % 256 && 256 - a->M % 256 > 127)
        return fail(M3PC_EINVAL, "debug_gemm_ex: variant 44 with a_padded would read %d rows behind A", 256 - a->M % 256);
    p = gemm_basic(a->A, a->lda, a->W, a->ldw, a->M, a->N, a->K, a->bias);
    p.amap = RowMap{a->amap[0], a->amap[1], a->amap[2]};
    p.cmap = RowMap{a->cmap[0], a->cmap[1], a->cmap[2]};
    p.rowtab = a->rowtab;
    if (a->rowtab) {
        p.rt_mod = a->rt_mod;
        p.rt_ld = a->rt_ld;
    }
    p.gelu = a->gelu ? 1 : 0;
    p.res = a->res;
    p.ldr = a->ldr;
    if (f32out)
        p.Cf = (float*)a->C;
    else
        p.Cb = (bf16_t*)a->C;
    p.ldc = a->ldc;
    p.ws = a->ws;
    p.ws_bytes = a->ws ? a->ws_bytes : 0;
    p.a_padded = a->a_padded ? 1 : 0;
    p.ln_g = a->ln_out ? a->ln_g : nullptr;
    p.ln_b = a->ln_out ? a->ln_b : nullptr;
    p.ln_out = a->ln_out;
    p.a_ln_g = a->a_ln_g;
    p.a_ln_b = a->a_ln_b;
    p.variant = v;
    if (a->a_ln_g && (dt != DT_F32 || !a->ws || v == 2 || !gemm_f32_direct_covers(p)))
        return fail(M3PC_EINVAL, "debug_gemm_ex: a_ln_* on a problem the few-row fp32 kernel does not take (the fold would be dropped)");
    return 0;
}

// the checks and the dry walk: fills p (x3: W still the caller's fp32 tensor) and plan[4] = what the dispatch would launch
static int debug_gemm_plan(const m3pc_debug_gemm_args* a, GemmP& p, int* plan) {
    if (a && a->picked) a->picked[0] = a->picked[1] = a->picked[2] = a->picked[3] = 0;
    if (int rc = debug_gemm_fill(a, p)) return rc;
    const int dt = a->dtype;
    if (dt == DT_X3) p.w_lo_off = (long long)a->N * a->ldw;  // (the hi / lo copies keep W's layout)
    M3PC_GEMM_PICK(0, 0, 0, 0);
    g_gemm_dry = 1;
    const int dry = dt == DT_X3 ? launch_gemm_x3(p, nullptr) : launch_gemm(p, dt, nullptr);
    g_gemm_dry = 0;
    for (int i = 0; i < 4; ++i) plan[i] = g_gemm_picked[i];
    if (dry < 0 || plan[0] == 0) return fail(M3PC_EINVAL, "debug_gemm_ex: no kernel of the dispatch covers this problem (epilogue flags / shape)");
    if (a->N % 64 && plan[0] != 5)  // (only the few-row fp32 kernel has 32-column tiles)
        return fail(M3PC_EINVAL, "debug_gemm_ex: N %d is not a multiple of 64 (kernel %d would drop columns)", a->N, plan[0]);
    const int v = a->variant;
    const int want = dt != DT_BF16 ? 0 : v == 2 ? 8 : v == 26 ? 7 : v == 37 ? 9 : v == 43 ? 10 : v == 44 ? 11 : 0;
    if (want && plan[0] != want) return fail(M3PC_EINVAL, "debug_gemm_ex: variant %d does not take this problem (kernel %d would run)", v, plan[0]);
    return 0;
}

int m3pc_debug_gemm_plan(const m3pc_debug_gemm_args* a) {
    GemmP p;
    int plan[4];
    if (int rc = debug_gemm_plan(a, p, plan)) return rc;
    if (a->picked)
        for (int i = 0; i < 4; ++i) a->picked[i] = plan[i];
    return 0;
}

int m3pc_debug_gemm_ex(const m3pc_debug_gemm_args* a) {
    GemmP p;
    int plan[4];
    if (int rc = debug_gemm_plan(a, p, plan)) return rc;
    hipStream_t st = (hipStream_t)a->stream;
    if (a->dtype == DT_X3) {  // hi / lo copies of W, as m3pc_load_weights keeps them.  (A lab hook's shortcut: the buffer is a
        // function-static that grows and is never freed, W is split again on every call, and calls from two threads would share it)
        static bf16_t* wsplit = nullptr;
        static size_t cap = 0;
        const size_t nw = (size_t)a->N * a->ldw;
        if (nw > cap) {
            if (wsplit) HIPCHK(hipFree(wsplit));
            wsplit = nullptr;
            cap = 0;
            HIPCHK(hipMalloc((void**)&wsplit, 2 * nw * sizeof(bf16_t)));
            cap = nw;
        }
        launch_f32_split_bf16((const float*)a->W, wsplit, wsplit + nw, (long long)nw, st);
        p.W = wsplit;
    }
    M3PC_GEMM_PICK(0, 0, 0, 0);
    if (a->dtype == DT_X3)
        launch_gemm_x3(p, st);
    else
        launch_gemm(p, a->dtype, st);
    if (a->picked)
        for (int i = 0; i < 4; ++i) a->picked[i] = g_gemm_picked[i];
    return check_launch("debug_gemm_ex");
}

int m3pc_debug_gemm_group(const m3pc_debug_gemm_args* a, int n) {
    if (!a || n < 1 || n > 4) return fail(M3PC_EINVAL, "debug_gemm_group: 1..4 problems");
    if (a[0].picked) a[0].picked[0] = a[0].picked[1] = a[0].picked[2] = a[0].picked[3] = 0;
    GemmP ps[4];
    for (int i = 0; i < n; ++i) {
        if (int rc = debug_gemm_fill(a + i, ps[i])) return rc;
        if (a[i].dtype != DT_F32 || !a[i].ws || a[i].variant != 0 || a[i].ln_out || !gemm_f32_direct_covers(ps[i]))
            return fail(M3PC_EINVAL, "debug_gemm_group: problem %d is not one the few-row fp32 kernel covers", i);
    }
    M3PC_GEMM_PICK(0, 0, 0, 0);
    if (!launch_gemm_f32_direct_group(ps, n, (hipStream_t)a[0].stream)) return fail(M3PC_EINVAL, "debug_gemm_group: not covered");
    if (a[0].picked)
        for (int i = 0; i < 4; ++i) a[0].picked[i] = g_gemm_picked[i];
    return check_launch("debug_gemm_group");
}

// Not part of the public header (tools/gemm_bench.py): clock counters of the last probed GEMM workgroup.
// cap > 0: from now on every fused-tail launch of the handle logs the phase stamps of its workgroup 37 into a ring of `cap`
// entries (64 int64 each: wave w at [16 w ..]); cap == 0: copy the ring to out (host, cap_prev * 64 int64), return how many
// launches were logged through *n_logged, and stop logging
int m3pc_debug_stamp_log(m3pc_handle* h, int cap, long long* out, int* n_logged) {
    if (!h) return fail(M3PC_EINVAL, "null handle");
    if (cap > 0) {
        if (h->stamp_log) hipFree(h->stamp_log);
        CHK(dmalloc(&h->stamp_log, (size_t)cap * 64));
        HIPCHK(hipMemset(h->stamp_log, 0, (size_t)cap * 64 * sizeof(long long)));
        h->stamp_cap = cap;
        h->stamp_i = 0;
        return 0;
    }
    if (!h->stamp_log) return fail(M3PC_ESTATE, "stamp log not enabled");
    HIPCHK(hipDeviceSynchronize());
    if (out) HIPCHK(hipMemcpy(out, h->stamp_log, (size_t)h->stamp_cap * 64 * sizeof(long long), hipMemcpyDeviceToHost));
    if (n_logged) *n_logged = h->stamp_i;
    hipFree(h->stamp_log);
    h->stamp_log = nullptr;
    h->stamp_cap = 0;
    return 0;
}

int m3pc_debug_clock(long long* out2) {
    HIPCHK(hipDeviceSynchronize());
    read_clock_probe(out2);
    return 0;
}

// Not part of the public header (tests/test_select_edges_gpu.py): the top-k kernels on their own.
// the statistics kernel of m3pc_calibrate_delta on caller vectors (tests/test_certified_step_gpu.py): stats = {lower median of
// scores_low - f32, largest deviation from it, largest |f32|, 0 ...} on the device, *delta_out as m3pc_calibrate_delta forms it
int m3pc_debug_calibrate_stats(const float* scores_low, const float* f32, int n, float factor, float* stats, float* delta_out,
                               void* stream) {
    if (!scores_low || !f32 || !stats || !delta_out || n < 1 || n > 16384) return fail(M3PC_EINVAL, "bad argument");
    launch_deviation_stats(scores_low, f32, n, stats, nullptr, 0.f, (hipStream_t)stream);
    CHK(check_launch("debug_calibrate_stats"));
    float s8[8];
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    HIPCHK(hipMemcpy(s8, stats, sizeof(s8), hipMemcpyDeviceToHost));
    *delta_out = cert_delta(factor, s8[1], s8[2]);
    return 0;
}
// what no top-k kernel may be given: the bitonic kernel's LDS holds 16384 keys, the selection kernel's registers 16 values per thread,
// and with k > n a rank >= n names no element
static int debug_topk_check(const void* v, const void* out, int n, int k, const char* who) {
    if (!v || !out) return fail(M3PC_EINVAL, "%s: null argument", who);
    if (n < 1 || n > 16384) return fail(M3PC_EINVAL, "%s: n %d outside [1, 16384]", who, n);
    if (k < 1 || k > n) return fail(M3PC_EINVAL, "%s: k %d outside [1, n = %d]", who, k, n);
    return 0;
}
int m3pc_debug_topk(const float* v, int n, int k, int* idx_out, void* stream) {
    CHK(debug_topk_check(v, idx_out, n, k, "debug_topk"));
    launch_topk(v, n, k, idx_out, (hipStream_t)stream);
    return check_launch("debug_topk");
}
int m3pc_debug_select_picked(void) { return g_sel_picked; }
unsigned int m3pc_debug_select_picked_set(int clear) {
    const unsigned int set = g_sel_picked_set;
    if (clear) {
        g_sel_picked_set = 0;
        g_sel_picked = 0;
    }
    return set;
}
// Every top-k kernel of select.hip on caller arrays (tests/test_select_edges_gpu.py): the dispatch or a forced kernel, a score or a
// race source.  Nothing is launched before the arguments are known to be inside what the kernel launched can read and write.
int m3pc_debug_topk_ex(const m3pc_debug_topk_args* a) {
    if (!a) return fail(M3PC_EINVAL, "debug_topk_ex: null argument");
    CHK(debug_topk_check(a->v, a->out, a->n, a->k, "debug_topk_ex"));
    if (a->n_windows < 1 || a->n_windows > 65535) return fail(M3PC_EINVAL, "debug_topk_ex: n_windows %d outside [1, 65535]", a->n_windows);
    if (a->out_stride != 1 && a->out_stride != -1) return fail(M3PC_EINVAL, "debug_topk_ex: out_stride %d is neither 1 nor -1", a->out_stride);
    const int v = a->variant;
    if (v < 0 || v > 6) return fail(M3PC_EINVAL, "debug_topk_ex: variant %d outside [0, 6]", v);
    const bool race_pair = a->expo && (v == 0 || v == 5);  // launch_topk_race: a score list and a race list
    if (v == 5 && !a->expo) return fail(M3PC_EINVAL, "debug_topk_ex: variant 5 ranks a race source");
    if (v != 0 && v != 6 && a->n_windows != 1) return fail(M3PC_EINVAL, "debug_topk_ex: a forced kernel ranks one window");
    if (race_pair) {
        if (a->n_windows != 1) return fail(M3PC_EINVAL, "debug_topk_ex: the race lists of several windows are m3pc_debug_topk_race_batch's");
        if (a->out_stride != -1) return fail(M3PC_EINVAL, "debug_topk_ex: the race list runs backwards (out_stride -1)");
        if (a->k > 64) return fail(M3PC_EINVAL, "debug_topk_ex: %d racers, the selection kernel lists 64", a->k);
        if (a->kk < 1 || a->kk > 1024 || a->kk > a->n) return fail(M3PC_EINVAL, "debug_topk_ex: kk %d outside [1, min(1024, n = %d)]", a->kk, a->n);
        if (v == 5 && a->scores_out) return fail(M3PC_EINVAL, "debug_topk_ex: the selection kernels write no scores");
    } else {
        if (a->kk != 0) return fail(M3PC_EINVAL, "debug_topk_ex: kk belongs to the race dispatch (expo with variant 0 or 5)");
        if (a->scores_out) return fail(M3PC_EINVAL, "debug_topk_ex: scores_out belongs to the race dispatch (expo with variant 0)");
        if (a->expo && v != 3) return fail(M3PC_EINVAL, "debug_topk_ex: of these kernels only the forced selection kernel ranks a race source");
        if (a->out_stride != 1 && v != 3) return fail(M3PC_EINVAL, "debug_topk_ex: only the selection kernel writes backwards");
        if ((v == 1 || v == 2) && a->n > 2048) return fail(M3PC_EINVAL, "debug_topk_ex: the ranking kernels hold 2048 keys, n = %d", a->n);
        if (v == 3 && a->k > 64) return fail(M3PC_EINVAL, "debug_topk_ex: the selection kernel lists 64, k = %d", a->k);
    }
    hipStream_t st = (hipStream_t)a->stream;
    g_sel_picked = 0;
    int first = 0;
    if (race_pair) {
        // out = the list at position rmax = k: out[-1 - i] the i-th racer, out[i] the i-th best score, scores_out alike
        g_sel_force_fallback = v == 5;
        const unsigned int before = g_sel_picked_set;
        g_sel_picked_set = 0;
        (void)launch_topk_race(a->v, a->expo, a->tau, a->n, a->kk, a->k, 0, a->out, a->scores_out, st);
        g_sel_force_fallback = false;
        for (int id = 1; id < 32; ++id)  // (the fallback launches two kernels: the score list's comes first)
            if ((g_sel_picked_set >> id & 1u) && id != g_sel_picked) first = id;
        if (!first) first = g_sel_picked;  // (one kernel ranked both lists, or the selection kernel ranked each)
        g_sel_picked_set |= before;
    } else if (v == 0 || v == 6) {
        if (v == 0 && a->n_windows == 1) launch_topk(a->v, a->n, a->k, a->out, st);
        else launch_topk_batch(a->v, a->n_windows, a->n, a->k, a->out, st);
    } else {
        launch_topk_forced(v, a->v, a->expo, a->tau, a->n, a->k, a->out, a->out_stride, st);
    }
    if (a->picked) {
        a->picked[0] = g_sel_picked;
        a->picked[1] = first;
    }
    return check_launch("debug_topk_ex");
}
int m3pc_debug_window_stats(const float* v, int n_total, const int* idx, int kk, int kmin, int kmax, float window, float* stats,
                            float* host_stats, float seq, float* top_scores, int rr, void* stream) {
    if (!v || !idx || !stats) return fail(M3PC_EINVAL, "debug_window_stats: null argument");
    if (n_total < 1 || n_total > 16384) return fail(M3PC_EINVAL, "debug_window_stats: n_total %d outside [1, 16384]", n_total);
    if (kk < 1 || kk > n_total) return fail(M3PC_EINVAL, "debug_window_stats: kk %d outside [1, n_total = %d]", kk, n_total);
    if (kmin < 1 || kmin > kmax) return fail(M3PC_EINVAL, "debug_window_stats: kmin %d outside [1, kmax = %d]", kmin, kmax);
    if (rr < 0 || rr > 64) return fail(M3PC_EINVAL, "debug_window_stats: rr %d outside [0, 64]", rr);
    if (!(window >= 0.f)) return fail(M3PC_EINVAL, "debug_window_stats: window must be >= 0");
    g_sel_picked = 0;
    launch_window_stats(v, n_total, idx, kk, kmin, kmax, window, stats, host_stats, seq, top_scores, (hipStream_t)stream, rr);
    return check_launch("debug_window_stats");
}
// launch_variates_batch (m3pc_refine_plans' normals) on a caller buffer: window w gets the elements [g0, g1) of the (seed, steps[w])
// normal array, what m3pc_draw_variates gives for that step
int m3pc_debug_variates_batch(unsigned long long seed, const unsigned long long* steps, int n_windows, long long g0, long long g1,
                              float* out, void* stream) {
    if (!steps || !out) return fail(M3PC_EINVAL, "debug_variates_batch: null argument");
    if (n_windows < 1 || n_windows > 65535) return fail(M3PC_EINVAL, "debug_variates_batch: n_windows %d outside [1, 65535]", n_windows);
    if (g0 < 0 || g1 <= g0 || g1 > (1LL << 33)) return fail(M3PC_EINVAL, "debug_variates_batch: [g0, g1) outside the generator's range");
    g_sel_picked = 0;
    launch_variates_batch(seed, steps, n_windows, g0, g1, out, (hipStream_t)stream);
    return check_launch("debug_variates_batch");
}
int m3pc_debug_scatter(const float* src, const int* index, int n, float* dst, int* index_copy, void* stream) {
    if (!src || !index || !dst) return fail(M3PC_EINVAL, "debug_scatter: null argument");
    if (n < 1) return fail(M3PC_EINVAL, "debug_scatter: n %d < 1", n);
    g_sel_picked = 0;
    launch_scatter(src, index, n, dst, index_copy, (hipStream_t)stream);
    return check_launch("debug_scatter");
}

// Not part of the public header (tests/test_lockstep_kernels_gpu.py): the three kernels of a lock-step batch's tail, each alone on
// caller arrays.  The checks are those of the one-window entry points, per window.
int m3pc_debug_topk_race_batch(const float* scores, const float* expo, float temperature, int n_windows, int n_total, int kmax, int kmin,
                               int rmax, int* list, float* list_scores, void* stream) {
    if (!scores || !list || (rmax > 0 && !expo)) return fail(M3PC_EINVAL, "null argument");
    if (n_windows < 1 || n_windows > 65535) return fail(M3PC_EINVAL, "n_windows %d outside [1, 65535]", n_windows);
    if (n_total < 1 || n_total > 16384) return fail(M3PC_EINVAL, "top-k supports n_total <= 16384");
    if (kmax < 1 || kmax > 1023 || kmin < 1 || kmin > kmax) return fail(M3PC_EINVAL, "bad kmin/kmax");
    if (rmax < 0 || rmax > 64 || rmax > n_total) return fail(M3PC_EINVAL, "rmax %d outside [0, min(64, n_total)]", rmax);
    const int kk = kmax + 1 < n_total ? kmax + 1 : n_total;
    if (!launch_topk_race_batch(scores, expo, temperature, n_windows, n_total, n_total, kk, rmax, rmax, list, list_scores,
                                rmax + kmax + 1, (hipStream_t)stream))
        return fail(M3PC_ENOMEM, "the device refused the LDS for the keys of %d candidates", n_total);
    return check_launch("debug_topk_race_batch");
}
int m3pc_debug_gather_listed(const float* sample_actions, const int* list, int n_windows, int n_total, int row_floats, int list_stride,
                             int lo, int hi, float* cand, int* window_index, void* stream) {
    if (!sample_actions || !list || !cand) return fail(M3PC_EINVAL, "null argument");
    if (n_windows < 1 || n_total < 1 || row_floats < 1) return fail(M3PC_EINVAL, "bad sizes");
    if (lo < 0 || hi < lo || hi > list_stride) return fail(M3PC_EINVAL, "slice [%d, %d) outside the list of %d", lo, hi, list_stride);
    if ((long long)n_windows * (hi - lo) > 0x7fffffffLL) return fail(M3PC_EINVAL, "too many rows");
    launch_gather_listed(sample_actions, n_windows, n_total, row_floats, list, list_stride, lo, hi - lo, cand, window_index,
                         (hipStream_t)stream);
    return check_launch("debug_gather_listed");
}
int m3pc_debug_merge_select_batch(const m3pc_debug_tail_args* a) {
    if (!a || !a->scores || !a->list || !a->list_scores || !a->list_rescored || !a->merged || !a->stats || !a->r || !a->n || !a->delta)
        return fail(M3PC_EINVAL, "null argument");
    if (a->race && !a->expo) return fail(M3PC_EINVAL, "race needs expo");
    if (a->n_windows < 1 || a->n_total < 1 || a->n_total > 16384) return fail(M3PC_EINVAL, "bad sizes");
    if (a->rmax < 0 || a->rmax > 64 || a->list_stride < a->rmax + 1 || a->f_lo < 0 || a->f_stride < 1)
        return fail(M3PC_EINVAL, "bad list layout");
    if (a->select && (a->eval_action || a->sample_action) && (!a->a0 || a->A < 1 || a->A > 1024))
        return fail(M3PC_EINVAL, "eval_action / sample_action need a0");
    for (int w = 0; w < a->n_windows; ++w) {
        const int r = a->r[w], n = a->n[w];
        if (n < 1 || r < 0 || r + n > 1024 || n > a->n_total || r > a->n_total || r > a->rmax || (!a->race && r != 0) ||
            n > a->list_stride - a->rmax || a->rmax - r < a->f_lo || a->rmax + n - a->f_lo > a->f_stride)
            return fail(M3PC_EINVAL, "window %d: r %d + n %d outside the list / [1, 1024] / n_total %d", w, r, n, a->n_total);
        if (!(a->delta[w] >= 0.f)) return fail(M3PC_EINVAL, "delta must be >= 0");
    }
    MergeSelectBatchP P;
    memset(&P, 0, sizeof(P));
    P.b = a->scores;
    P.expo = a->expo;
    P.row_stride = a->n_total;
    P.n_total = a->n_total;
    P.race = a->race;
    P.select = a->select;
    P.tau = a->temperature;
    P.list = a->list;
    P.list_scores = a->list_scores;
    P.list_stride = a->list_stride;
    P.rmax = a->rmax;
    P.f = a->list_rescored;
    P.f_stride = a->f_stride;
    P.f_lo = a->f_lo;
    P.out = a->merged;
    P.stats = a->stats;
    P.host_stats = a->host_stats;
    P.seq = a->seq;
    P.a0 = a->a0;
    P.a0_wstride = a->a0_window_stride;
    P.a0_stride = a->a0_stride;
    P.A = a->A;
    P.p = a->p;
    P.eval_action = a->eval_action;
    P.argmax = a->argmax;
    P.sample_idx = a->sample_idx;
    P.sample_action = a->sample_action;
    launch_merge_select_batch(P, a->n_windows, a->r, a->n, a->delta, (hipStream_t)a->stream);
    return check_launch("debug_merge_select_batch");
}
// the eval_action certificate of n_windows windows in one launch (eval_bound_batch_kernel): m3pc_eval_bound's checks, per window
int m3pc_debug_eval_bound_batch(const m3pc_debug_eval_batch_args* a) {
    if (!a || !a->merged || !a->list || !a->a0 || !a->stats || !a->r || !a->n || !a->delta) return fail(M3PC_EINVAL, "null argument");
    if (!(a->eval_tol > 0.f)) return fail(M3PC_EINVAL, "eval_tol must be > 0 (+inf: report only)");
    if (a->n_windows < 1 || a->n_windows > 65535) return fail(M3PC_EINVAL, "n_windows %d outside [1, 65535]", a->n_windows);
    if (a->n_total < 1 || a->n_total > 16384) return fail(M3PC_EINVAL, "n_total %d outside [1, 16384]", a->n_total);
    if (a->A < 1 || a->A > 1024) return fail(M3PC_EINVAL, "A %d outside [1, 1024]", a->A);
    if (a->rmax < 0 || a->rmax > 64 || a->n_listed < 0 || a->rmax + a->n_listed > 1024 || a->rmax + a->n_listed > a->list_stride)
        return fail(M3PC_EINVAL, "rmax %d + n_listed %d outside [0, min(1024, list_stride=%d)]", a->rmax, a->n_listed, a->list_stride);
    if (!(a->temperature == a->temperature)) return fail(M3PC_EINVAL, "temperature is not a number");
    for (int w = 0; w < a->n_windows; ++w) {
        if (a->r[w] < 0 || a->r[w] > a->rmax || a->n[w] < 0 || a->n[w] > a->n_listed)
            return fail(M3PC_EINVAL, "window %d: r %d outside [0, rmax=%d] or n %d outside [0, n_listed=%d]", w, a->r[w], a->rmax, a->n[w],
                        a->n_listed);
        if (!(a->delta[w] >= 0.f)) return fail(M3PC_EINVAL, "delta must be >= 0");
    }
    EvalBoundBatchP P;
    memset(&P, 0, sizeof(P));
    P.m = a->merged;
    P.n_total = a->n_total;
    P.list = a->list;
    P.list_stride = a->list_stride;
    P.rmax = a->rmax;
    P.n_listed = a->n_listed;
    P.a0 = a->a0;
    P.a0_wstride = a->a0_window_stride;
    P.a0_stride = a->a0_stride;
    P.A = a->A;
    P.tau = a->temperature;
    P.eval_tol = a->eval_tol;
    P.stats = a->stats;
    P.host_stats = a->host_stats;
    P.seq = a->seq;
    launch_eval_bound_batch(P, a->n_windows, a->r, a->n, a->delta, (hipStream_t)a->stream);
    return check_launch("debug_eval_bound_batch");
}
// the select of n_windows windows in one launch (the fp32 form of m3pc_plan_steps_certified): m3pc_select's checks, per window
int m3pc_debug_select_batch(const float* scores, const float* a0, long long a0_window_stride, long long a0_stride, int n_windows,
                            int n_total, int A, float temperature, const float* expo, float* p, float* eval_action, int* argmax,
                            int* sample_idx, float* sample_action, void* stream) {
    if (!scores || n_total < 1 || n_total > 16384) return fail(M3PC_EINVAL, "bad argument");
    if (n_windows < 1 || n_windows > 65535) return fail(M3PC_EINVAL, "n_windows %d outside [1, 65535]", n_windows);
    if ((eval_action || sample_action) && (!a0 || A < 1 || A > 1024)) return fail(M3PC_EINVAL, "eval_action / sample_action need a0");
    if ((sample_idx || sample_action) && !expo) return fail(M3PC_EINVAL, "the multinomial draw needs expo");
    SelectP s;
    memset(&s, 0, sizeof(s));
    s.er = scores;
    s.a0 = a0;
    s.a0_stride = a0_stride;
    s.n = n_total;
    s.A = A;
    s.temperature = temperature;
    s.expo = expo;
    s.p = p;
    s.eval_action = eval_action;
    s.argmax = argmax;
    s.sample_idx = sample_idx;
    s.sample_action = sample_action;
    launch_select_batch(s, n_windows, n_total, a0_window_stride, (hipStream_t)stream);
    return check_launch("debug_select_batch");
}

// Not part of the public header (tests/test_block_fused_gpu.py, tools/block_bench.py): the fused layer tail on its own.
//   O (M,512) bf16; res (M,512) fp32 or rowtab (rt_mod,512); Wo (512,512), W1 (2048,512), W2 (512,2048) bf16 in torch
//   Linear layout; stream: scratch of m3pc_debug_block_stream_bytes() bytes (packed when pack != 0);
//   lnB_g0 / lnB_g1 optional (with out_mod / out_grp); Xout (M,512) fp32 optional; Hout (M,512) bf16 optional
long long m3pc_debug_block_stream_bytes(void) { return (long long)block_stream_bytes(); }
int m3pc_debug_block_fused(const void* O, int M, const float* res, const float* rowtab, int rt_mod, const void* Wo, const void* W1,
                           const void* W2, void* stream_buf, int pack, const float* bo, const float* b1, const float* b2,
                           const float* ln2_g, const float* ln2_b, const float* lnA_g, const float* lnA_b, const float* lnB_g0,
                           const float* lnB_b0, const float* lnB_g1, const float* lnB_b1, int out_mod, int out_grp, float* Xout,
                           void* Hout, int variant, void* stream, long long* stamps) {
    hipStream_t st = (hipStream_t)stream;
    if (pack) launch_pack_block_stream((const bf16_t*)Wo, (const bf16_t*)W1, (const bf16_t*)W2, (bf16_t*)stream_buf, st);
    BlockP b;
    memset(&b, 0, sizeof(b));
    b.O = (const bf16_t*)O;
    b.ldo = 512;
    b.M = M;
    b.res = res;
    b.ldr = 512;
    b.rowtab = rowtab;
    b.rt_mod = rt_mod;
    b.wstream = (const bf16_t*)stream_buf;
    b.bo = bo;
    b.b1 = b1;
    b.b2 = b2;
    b.ln2_g = ln2_g;
    b.ln2_b = ln2_b;
    b.Xout = Xout;
    b.ldx = 512;
    b.lnA_g = lnA_g;
    b.lnA_b = lnA_b;
    b.lnB_g[0] = lnB_g0;
    b.lnB_b[0] = lnB_b0;
    b.lnB_g[1] = lnB_g1;
    b.lnB_b[1] = lnB_b1;
    b.out_mod = out_mod;
    b.out_grp = out_grp;
    b.Hout = (bf16_t*)Hout;
    b.ldh = 512;
    b.variant = variant & 15;
    b.x_bf16 = (variant & 16) ? 1 : 0;  // (res and Xout are then (M, 512) bf16 rows)
    b.stamps = stamps;
    if (!launch_block_fused(b, st)) return fail(M3PC_EINVAL, "block_fused: arguments not covered");
    return check_launch("debug_block_fused");
}

// the fused layer tail with the next layer's Q|K|V projection behind it: QKV (M, 1536) bf16 = LN_A(X'') Wqkv^T + bqkv
int m3pc_debug_block_fused_qkv(const void* O, int M, const float* res, const void* Wo, const void* W1, const void* W2, const void* Wqkv,
                               void* stream_buf, const float* bo, const float* b1, const float* b2, const float* ln2_g,
                               const float* ln2_b, const float* lnA_g, const float* lnA_b, const float* bqkv, float* Xout, void* QKV,
                               void* stream, long long* stamps, int x_bf16) {
    hipStream_t st = (hipStream_t)stream;
    launch_pack_block_stream((const bf16_t*)Wo, (const bf16_t*)W1, (const bf16_t*)W2, (bf16_t*)stream_buf, st);
    launch_pack_block_qkv((const bf16_t*)Wqkv, (bf16_t*)stream_buf, st);
    BlockP b;
    memset(&b, 0, sizeof(b));
    b.O = (const bf16_t*)O;
    b.ldo = 512;
    b.M = M;
    b.res = res;
    b.ldr = 512;
    b.wstream = (const bf16_t*)stream_buf;
    b.bo = bo;
    b.b1 = b1;
    b.b2 = b2;
    b.ln2_g = ln2_g;
    b.ln2_b = ln2_b;
    b.Xout = Xout;
    b.ldx = 512;
    b.lnA_g = lnA_g;
    b.lnA_b = lnA_b;
    b.QKVout = (bf16_t*)QKV;
    b.ldq = 1536;
    b.qkv_bytes = (unsigned)((size_t)M * 1536 * 2);
    b.bqkv = bqkv;
    b.stamps = stamps;
    b.x_bf16 = x_bf16 ? 1 : 0;  // (res and Xout are then (M, 512) bf16 rows)
    if (!launch_block_fused(b, st)) return fail(M3PC_EINVAL, "block_fused (qkv): arguments not covered");
    return check_launch("debug_block_fused_qkv");
}

// the decoder form of the fused tail with the two scalar output heads inside: rows of group s = (r % out_mod) / out_grp;
// out0 / out1 (M / 2) floats; Wh (2, 512, 512) bf16, hb1 / hw2 (2, 512), hb2 / hmean / hstd (2) floats (hmean null: no detok)
int m3pc_debug_block_fused_heads(const void* O, int M, const float* rowtab, int rt_mod, const void* Wo, const void* W1, const void* W2,
                                 const void* Wh, void* stream_buf, const float* bo, const float* b1, const float* b2, const float* ln2_g,
                                 const float* ln2_b, const float* lnA_g, const float* lnA_b, const float* lnB_g0, const float* lnB_b0,
                                 const float* lnB_g1, const float* lnB_b1, int out_mod, int out_grp, const float* hb1, const float* hw2,
                                 const float* hb2, const float* hmean, const float* hstd, float* out0, float* out1, void* stream,
                                 long long* stamps) {
    hipStream_t st = (hipStream_t)stream;
    launch_pack_block_stream((const bf16_t*)Wo, (const bf16_t*)W1, (const bf16_t*)W2, (bf16_t*)stream_buf, st);
    launch_pack_block_heads((const bf16_t*)Wh, (const bf16_t*)Wh + 512 * 512, (bf16_t*)stream_buf, st);
    BlockP b;
    memset(&b, 0, sizeof(b));
    b.O = (const bf16_t*)O;
    b.ldo = 512;
    b.M = M;
    b.rowtab = rowtab;
    b.rt_mod = rt_mod;
    b.wstream = (const bf16_t*)stream_buf;
    b.bo = bo;
    b.b1 = b1;
    b.b2 = b2;
    b.ln2_g = ln2_g;
    b.ln2_b = ln2_b;
    b.lnA_g = lnA_g;
    b.lnA_b = lnA_b;
    b.lnB_g[0] = lnB_g0;
    b.lnB_b[0] = lnB_b0;
    b.lnB_g[1] = lnB_g1;
    b.lnB_b[1] = lnB_b1;
    b.out_mod = out_mod;
    b.out_grp = out_grp;
    b.head_out[0] = out0;
    b.head_out[1] = out1;
    for (int s = 0; s < 2; ++s) {
        b.hb1[s] = hb1 + 512 * s;
        b.hw2[s] = hw2 + 512 * s;
        b.hb2[s] = hb2 + s;
        b.hmean[s] = hmean ? hmean + s : nullptr;
        b.hstd[s] = hstd ? hstd + s : nullptr;
    }
    b.stamps = stamps;
    if (!launch_block_fused(b, st)) return fail(M3PC_EINVAL, "block_fused (heads): arguments not covered");
    return check_launch("debug_block_fused_heads");
}

// the fused layer tail with everything BlockP carries (include/m3pc_hip_debug.h)
static int debug_block_fill(const m3pc_debug_block_args* a, BlockP& b, SplitReduceP& r) {
    if (!a) return fail(M3PC_EINVAL, "debug_block: null arguments");
    memset(&b, 0, sizeof(b));
    memset(&r, 0, sizeof(r));
    if (a->picked) a->picked[0] = 0;
    if (a->M <= 0) return fail(M3PC_EINVAL, "debug_block: M = %d", a->M);
    if (!a->O || !a->Wo || !a->W1 || !a->W2 || !a->stream_buf || !a->bo || !a->b1 || !a->b2 || !a->ln2_g || !a->ln2_b)
        return fail(M3PC_EINVAL, "debug_block: O, the layer's weights, biases, norm2 and the stream buffer are required");
    if (!a->res && !a->rowtab) return fail(M3PC_EINVAL, "debug_block: neither res nor rowtab");
    if (a->rowtab && a->rt_mod < 1) return fail(M3PC_EINVAL, "debug_block: rowtab with rt_mod %d", a->rt_mod);
    if (a->res_L < 0 || a->res_nshared < 0) return fail(M3PC_EINVAL, "debug_block: res_L / res_nshared below 0");
    if ((a->Hout || a->head_out[0]) && !a->lnA_g) return fail(M3PC_EINVAL, "debug_block: Hout / heads without lnA");
    if (a->lnA_g && !a->lnA_b) return fail(M3PC_EINVAL, "debug_block: lnA_g without lnA_b");
    for (int s = 0; s < 2; ++s)
        if ((a->lnB_g[s] != nullptr) != (a->lnB_b[s] != nullptr)) return fail(M3PC_EINVAL, "debug_block: lnB_g / lnB_b come in pairs");
    if (a->lnB_g[0] && !a->lnB_g[1]) return fail(M3PC_EINVAL, "debug_block: lnB is two pairs (the kernel's tables hold two)");
    if (a->out_mod < 0 || (a->out_mod > 0 && (a->out_grp < 1 || !a->lnB_g[0]))) return fail(M3PC_EINVAL, "debug_block: out_mod / out_grp / lnB");
    if (a->QKVout && !a->Wqkv) return fail(M3PC_EINVAL, "debug_block: QKVout without Wqkv");
    if (a->head_out[0] && (!a->Wh || !a->hb1 || !a->hw2 || !a->hb2)) return fail(M3PC_EINVAL, "debug_block: heads without their weights");
    if (a->Wqkv && a->Wh) return fail(M3PC_EINVAL, "debug_block: Wqkv and Wh share the stream's tail");
    if (a->qkv_bytes < 0 || a->qkv_bytes > 0xffffffffll) return fail(M3PC_EINVAL, "debug_block: qkv_bytes");
    b.O = (const bf16_t*)a->O;
    b.ldo = a->ldo;
    b.M = a->M;
    b.res = (const float*)a->res;
    b.ldr = a->ldr;
    b.res_L = a->res_L;
    b.res_nshared = a->res_nshared;
    b.rowtab = a->rowtab;
    b.rt_mod = a->rt_mod;
    b.res_nu = a->res_nu;
    b.wstream = (const bf16_t*)a->stream_buf;
    b.bo = a->bo;
    b.b1 = a->b1;
    b.b2 = a->b2;
    b.ln2_g = a->ln2_g;
    b.ln2_b = a->ln2_b;
    b.Xout = (float*)a->Xout;
    b.ldx = a->ldx;
    b.x_bf16 = a->x_bf16 ? 1 : 0;
    b.lnA_g = a->lnA_g;
    b.lnA_b = a->lnA_b;
    for (int s = 0; s < 2; ++s) {
        b.lnB_g[s] = a->lnB_g[s];
        b.lnB_b[s] = a->lnB_b[s];
    }
    b.out_mod = a->out_mod;
    b.out_grp = a->out_grp;
    b.Hout = (bf16_t*)a->Hout;
    b.ldh = a->ldh;
    b.QKVout = (bf16_t*)a->QKVout;
    b.ldq = a->ldq;
    b.qkv_bytes = (unsigned)a->qkv_bytes;
    b.bqkv = a->bqkv;
    for (int s = 0; s < 2; ++s) {
        b.head_out[s] = a->head_out[s];
        if (!a->head_out[0]) continue;
        b.hb1[s] = a->hb1 + 512 * s;
        b.hw2[s] = a->hw2 + 512 * s;
        b.hb2[s] = a->hb2 + s;
        b.hmean[s] = a->hmean ? a->hmean + s : nullptr;
        b.hstd[s] = a->hstd ? a->hstd + s : nullptr;
    }
    b.split = a->split ? 1 : 0;
    if (!block_fused_accepts(b)) return fail(M3PC_EINVAL, "debug_block: arguments not covered (block_fused_accepts)");
    if (b.split) {
        r.slabs = (const float*)a->Xout;
        r.M = a->M;
        r.Xout = a->red_Xout;
        r.ldx = a->red_ldx;
        r.lnA_g = a->red_lnA_g;
        r.lnA_b = a->red_lnA_b;
        for (int s = 0; s < 2; ++s) {
            r.lnB_g[s] = a->red_lnB_g[s];
            r.lnB_b[s] = a->red_lnB_b[s];
        }
        r.out_mod = a->red_out_mod;
        r.out_grp = a->red_out_grp;
        r.Hout = (bf16_t*)a->red_Hout;
        r.ldh = a->red_ldh;
        if (!r.Xout && !r.Hout) return fail(M3PC_EINVAL, "debug_block: the reduce has no output");
        if (r.Xout && (((uintptr_t)r.Xout & 15) || r.ldx < 512 || (r.ldx % 4))) return fail(M3PC_EINVAL, "debug_block: red_Xout / red_ldx");
        if (r.Hout && (((uintptr_t)r.Hout & 15) || r.ldh < 512 || (r.ldh % 8) || !r.lnA_g || !r.lnA_b)) return fail(M3PC_EINVAL, "debug_block: red_Hout / red_ldh / red_lnA");
        if ((r.lnB_g[0] != nullptr) != (r.lnB_b[0] != nullptr) || (r.lnB_g[0] && r.out_mod > 0 && (!r.lnB_g[1] || !r.lnB_b[1])))
            return fail(M3PC_EINVAL, "debug_block: red_lnB");
        if (r.out_mod < 0 || (r.out_mod > 0 && (!r.lnB_g[0] || r.out_mod != 2 * r.out_grp || a->M % r.out_mod != 0)))
            return fail(M3PC_EINVAL, "debug_block: red_out_mod / red_out_grp");
    }
    if (a->picked) a->picked[0] = block_fused_form(b);
    return 0;
}
int m3pc_debug_block_split_n(void) { return block_split_n(); }
int m3pc_debug_block_accepts(const m3pc_debug_block_args* a) {
    BlockP b;
    SplitReduceP r;
    return debug_block_fill(a, b, r);
}
int m3pc_debug_block_ex(const m3pc_debug_block_args* a) {
    BlockP b;
    SplitReduceP r;
    const int rc = debug_block_fill(a, b, r);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)a->stream;
    launch_pack_block_stream((const bf16_t*)a->Wo, (const bf16_t*)a->W1, (const bf16_t*)a->W2, (bf16_t*)a->stream_buf, st);
    if (a->Wqkv) launch_pack_block_qkv((const bf16_t*)a->Wqkv, (bf16_t*)a->stream_buf, st);
    if (a->Wh) launch_pack_block_heads((const bf16_t*)a->Wh, (const bf16_t*)a->Wh + 512 * 512, (bf16_t*)a->stream_buf, st);
    if (!launch_block_fused(b, st)) {
        if (a->picked) a->picked[0] = 0;
        return fail(M3PC_EINVAL, "debug_block: arguments not covered");
    }
    if (b.split) launch_block_split_reduce(r, st);
    return check_launch("debug_block_ex");
}
// where the bf16 residual row of token row r lives in the compact layout (block_res_row_xb; host only, no GPU needed)
int m3pc_debug_block_res_row(int r, int res_L, int res_nshared) {
    if (r < 0 || res_L < 1 || res_nshared < 0 || res_nshared > res_L) return -1;
    return block_res_row_xb(r, res_L, res_nshared);
}

// the embedding kernel (launch_embed) on caller tensors (include/m3pc_hip_debug.h)
static int debug_embed_run(const m3pc_debug_embed_args* a, float* Hf) {
    if (!a) return fail(M3PC_EINVAL, "debug_embed: null arguments");
    g_ew_picked = 0;
    if (a->batch < 1 || a->L < 1 || a->d % 64 != 0 || a->d < 64 || a->d > 1024 || !a->tokmap) return fail(M3PC_EINVAL, "debug_embed: batch / L / d / tokmap");
    const bool block_form = a->d % 256 != 0;  // (launch_embed: embed_kernel, one block per row)
    if (block_form && (a->Xb || a->n_sh || a->n_indep || a->x_first_only || a->x_compact))
        return fail(M3PC_EINVAL, "debug_embed: d %d runs embed_kernel, which has no Xb / n_sh / n_indep / x_first_only / x_compact", a->d);
    if (a->T < 1 || (long long)a->batch * a->L > 0x7fffffffLL) return fail(M3PC_EINVAL, "debug_embed: T / batch * L");
    if (a->n_indep < 0 || a->n_indep > a->L || a->n_sh < 0 || a->n_sh > a->n_indep) return fail(M3PC_EINVAL, "debug_embed: n_indep / n_sh");
    if (!a->X == !a->Xb) return fail(M3PC_EINVAL, "debug_embed: exactly one of X / Xb");
    if (a->x_compact && !(a->Xb && a->x_first_only && a->n_indep > 0)) return fail(M3PC_EINVAL, "debug_embed: x_compact needs Xb, x_first_only and n_indep > 0");
    if ((a->Hb || Hf || a->n_sh) && (!a->ln_g || !a->ln_b)) return fail(M3PC_EINVAL, "debug_embed: Hb / Hf without ln_g / ln_b");
    if (Hf && (a->n_sh || ((uintptr_t)Hf & 15))) return fail(M3PC_EINVAL, "debug_embed: Hf with n_sh, or off 16 bytes");
    if (a->n_sh > 0 && (!a->Hb || !a->Hb_sh)) return fail(M3PC_EINVAL, "debug_embed: n_sh without Hb / Hb_sh");
    {  // the entries of tokmap: a key the call carries, a step inside the table E
        std::vector<int> tm((size_t)a->L * 2);
        HIPCHK(hipMemcpy(tm.data(), a->tokmap, tm.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int j = 0; j < a->L; ++j) {
            const int key = tm[2 * j], t = tm[2 * j + 1];
            if (key < 0 || key > 3 || t < 0 || t >= a->T) return fail(M3PC_EINVAL, "debug_embed: token %d is {key %d, step %d}", j, key, t);
            if (!a->tok[key] || !a->WT[key] || !a->E[key] || a->feat[key] < 1 || (block_form && a->feat[key] > 32))
                return fail(M3PC_EINVAL, "debug_embed: key %d of token %d lacks tok / WT / E or has feat %d", key, j, a->feat[key]);
        }
    }
    EmbedP e;
    memset(&e, 0, sizeof(e));
    for (int k = 0; k < 4; ++k) {
        e.tok[k] = a->tok[k];
        e.bstride[k] = a->bstride[k];
        e.WT[k] = a->WT[k];
        e.E[k] = a->E[k];
        e.feat[k] = a->feat[k];
    }
    e.tokmap = (const int2*)a->tokmap;
    e.batch = a->batch;
    e.L = a->L;
    e.d = a->d;
    e.T = a->T;
    e.X = a->X;
    e.Xb = (bf16_t*)a->Xb;
    e.ln_g = a->ln_g;
    e.ln_b = a->ln_b;
    e.Hf = Hf;
    e.Hb = (bf16_t*)a->Hb;
    e.Hb_sh = (bf16_t*)a->Hb_sh;
    e.n_indep = a->n_indep;
    e.n_sh = a->n_sh;
    e.x_first_only = a->x_first_only ? 1 : 0;
    e.x_compact = a->x_compact ? 1 : 0;
    launch_embed(e, (hipStream_t)a->stream);
    return check_launch("debug_embed");
}
int m3pc_debug_embed(const m3pc_debug_embed_args* a) { return debug_embed_run(a, nullptr); }
int m3pc_debug_embed_ex(const m3pc_debug_embed_ex_args* a) {
    if (!a) return fail(M3PC_EINVAL, "debug_embed_ex: null arguments");
    if (a->picked) a->picked[0] = 0;
    const int rc = debug_embed_run(&a->base, a->Hf);
    if (rc == 0 && a->picked) a->picked[0] = g_ew_picked;
    return rc;
}

// ---- csrc/elementwise.hip, kernel by kernel (include/m3pc_hip_debug.h, "Elementwise kernel ids"; tests/test_elementwise_edges_gpu.py).
// Every hook checks first, fills the kernel's parameter structure, goes through the production launcher and reports what that
// launcher recorded.
int m3pc_debug_elementwise_picked(void) { return g_ew_picked; }
static bool ew_bad_map(const int* m) { return m[0] < 0 || m[2] < 0 || (m[0] >= 1 && m[1] < m[0]); }
static bool ew_bad_d(int d) { return d < 64 || d > 1024 || d % 64 != 0; }
static int ew_done(int* picked, const char* what) {
    if (picked) picked[0] = g_ew_picked;
    return check_launch(what);
}

int m3pc_debug_layernorm(const m3pc_debug_ln_args* a) {
    if (!a) return fail(M3PC_EINVAL, "debug_layernorm: null arguments");
    if (a->picked) a->picked[0] = 0;
    if (!a->X || !a->g1 || !a->b1) return fail(M3PC_EINVAL, "debug_layernorm: X, g1 and b1 are required");
    if (!a->Yf && !a->Yb) return fail(M3PC_EINVAL, "debug_layernorm: neither Yf nor Yb");
    if ((a->g2 != nullptr) != (a->b2 != nullptr)) return fail(M3PC_EINVAL, "debug_layernorm: g2 and b2 go together");
    if (a->rows < 1) return fail(M3PC_EINVAL, "debug_layernorm: rows %d", a->rows);
    if (ew_bad_d(a->d)) return fail(M3PC_EINVAL, "debug_layernorm: d %d is not a multiple of 64 in [64, 1024] (a lane holds at most 16 values)", a->d);
    if (a->ldx < a->d) return fail(M3PC_EINVAL, "debug_layernorm: ldx %d below d %d", a->ldx, a->d);
    if (ew_bad_map(a->xmap)) return fail(M3PC_EINVAL, "debug_layernorm: row map {%d, %d, %d}", a->xmap[0], a->xmap[1], a->xmap[2]);
    if (a->d % 256 == 0 && a->ldx % 4 == 0) {  // layernorm_vec_kernel / layernorm_rows_kernel: 16-byte loads, 16- and 8-byte stores
        const uintptr_t p16 = (uintptr_t)a->X | (uintptr_t)a->g1 | (uintptr_t)a->b1 | (uintptr_t)a->g2 | (uintptr_t)a->b2 | (uintptr_t)a->Yf;
        if ((p16 & 15) || ((uintptr_t)a->Yb & 7)) return fail(M3PC_EINVAL, "debug_layernorm: the 16-byte kernels need X / g / b / Yf on 16 bytes and Yb on 8");
    }
    LnP p;
    memset(&p, 0, sizeof(p));
    p.X = a->X;
    p.ldx = a->ldx;
    p.xmap = RowMap{a->xmap[0], a->xmap[1], a->xmap[2]};
    p.rows = a->rows;
    p.d = a->d;
    p.g1 = a->g1;
    p.b1 = a->b1;
    p.g2 = a->g2;
    p.b2 = a->b2;
    p.Yf = a->Yf;
    p.Yb = (bf16_t*)a->Yb;
    g_ew_picked = 0;
    launch_layernorm(p, (hipStream_t)a->stream);
    return ew_done(a->picked, "debug_layernorm");
}

int m3pc_debug_head_out(const m3pc_debug_head_out_args* a) {
    if (!a) return fail(M3PC_EINVAL, "debug_head_out: null arguments");
    if (a->picked) a->picked[0] = 0;
    if (!a->W || !a->b || !a->Y) return fail(M3PC_EINVAL, "debug_head_out: W, b and Y are required");
    if ((a->mean != nullptr) != (a->stdv != nullptr)) return fail(M3PC_EINVAL, "debug_head_out: mean and stdv go together");
    if (a->rows < 1) return fail(M3PC_EINVAL, "debug_head_out: rows %d", a->rows);
    if (ew_bad_d(a->d)) return fail(M3PC_EINVAL, "debug_head_out: d %d is not a multiple of 64 in [64, 1024]", a->d);
    if (a->D < 1 || a->D > 32) return fail(M3PC_EINVAL, "debug_head_out: D %d outside [1, 32]", a->D);
    if (a->ldx < a->d || a->ldy < a->D) return fail(M3PC_EINVAL, "debug_head_out: ldx %d / ldy %d below d / D", a->ldx, a->ldy);
    if (ew_bad_map(a->ymap)) return fail(M3PC_EINVAL, "debug_head_out: row map {%d, %d, %d}", a->ymap[0], a->ymap[1], a->ymap[2]);
    const bool mfma = a->Xb && head_out_mfma_covers(a->rows, a->d, a->D);  // (as the callers ask before they hand over bf16 rows)
    if (!mfma && !a->X) return fail(M3PC_EINVAL, "debug_head_out: no fp32 rows, and the matrix-core kernel does not cover %d rows of d %d", a->rows, a->d);
    if (mfma && (((uintptr_t)a->Xb & 15) || a->ldx % 8)) return fail(M3PC_EINVAL, "debug_head_out: the matrix-core kernel reads 16 bytes of a bf16 row at a time (Xb, ldx %% 8)");
    HeadOutP p;
    memset(&p, 0, sizeof(p));
    if (mfma) p.Xb = (const bf16_t*)a->Xb;
    else p.X = a->X;
    p.ldx = a->ldx;
    p.rows = a->rows;
    p.d = a->d;
    p.D = a->D;
    p.W = a->W;
    p.b = a->b;
    p.mean = a->mean;
    p.stdv = a->stdv;
    p.Y = a->Y;
    p.ymap = RowMap{a->ymap[0], a->ymap[1], a->ymap[2]};
    p.ldy = a->ldy;
    g_ew_picked = 0;
    launch_head_out(p, (hipStream_t)a->stream);
    return ew_done(a->picked, "debug_head_out");
}

int m3pc_debug_actor_head(const m3pc_debug_actor_args* a) {
    if (!a) return fail(M3PC_EINVAL, "debug_actor_head: null arguments");
    if (a->picked) a->picked[0] = 0;
    if (!a->X || !a->Wmu || !a->bmu || !a->Wls || !a->bls || !a->mu || !a->sd) return fail(M3PC_EINVAL, "debug_actor_head: a required pointer is null");
    if ((a->ln_g != nullptr) != (a->ln_b != nullptr)) return fail(M3PC_EINVAL, "debug_actor_head: ln_g and ln_b go together");
    if (a->rows < 1) return fail(M3PC_EINVAL, "debug_actor_head: rows %d", a->rows);
    if (ew_bad_d(a->d)) return fail(M3PC_EINVAL, "debug_actor_head: d %d is not a multiple of 64 in [64, 1024]", a->d);
    if (a->A < 1 || a->A > 32) return fail(M3PC_EINVAL, "debug_actor_head: A %d outside [1, 32]", a->A);
    if (a->ldx < a->d) return fail(M3PC_EINVAL, "debug_actor_head: ldx %d below d %d", a->ldx, a->d);
    if (ew_bad_map(a->xmap)) return fail(M3PC_EINVAL, "debug_actor_head: row map {%d, %d, %d}", a->xmap[0], a->xmap[1], a->xmap[2]);
    const bool fuses = actor_head_fuses_ln(a->d, a->A);
    if (a->ln_g && !fuses) return fail(M3PC_EINVAL, "debug_actor_head: ln_g at d %d, A %d (actor_head_small_kernel has no LayerNorm: it would be dropped)", a->d, a->A);
    if (fuses) {  // actor_head_kernel: 16-byte loads of the row, the weight rows and the norm's vectors
        const uintptr_t p16 = (uintptr_t)a->X | (uintptr_t)a->Wmu | (uintptr_t)a->Wls | (uintptr_t)a->ln_g | (uintptr_t)a->ln_b;
        if ((p16 & 15) || a->ldx % 4) return fail(M3PC_EINVAL, "debug_actor_head: actor_head_kernel needs X / Wmu / Wls / ln_g / ln_b on 16 bytes and ldx %% 4 == 0");
    }
    ActorP p;
    memset(&p, 0, sizeof(p));
    p.X = a->X;
    p.ldx = a->ldx;
    p.xmap = RowMap{a->xmap[0], a->xmap[1], a->xmap[2]};
    p.rows = a->rows;
    p.d = a->d;
    p.A = a->A;
    p.Wmu = a->Wmu;
    p.bmu = a->bmu;
    p.Wls = a->Wls;
    p.bls = a->bls;
    p.mu = a->mu;
    p.sd = a->sd;
    p.ln_g = a->ln_g;
    p.ln_b = a->ln_b;
    g_ew_picked = 0;
    launch_actor_head(p, (hipStream_t)a->stream);
    return ew_done(a->picked, "debug_actor_head");
}

int m3pc_debug_critic_pack(const float* W1, const float* W2, int SA, int hidden, float* w1f, float* w2f, long long* n_w1f, long long* n_w2f) {
    if (SA < 1 || SA > 32 || (hidden != 64 && hidden != 128 && hidden != 256)) return fail(M3PC_EINVAL, "debug_critic_pack: SA %d / hidden %d", SA, hidden);
    if (n_w1f) *n_w1f = (long long)critic_w1f_floats(hidden);
    if (n_w2f) *n_w2f = (long long)critic_w2f_floats(hidden);
    if (!w1f && !w2f) return 0;
    if (!W1 || !W2 || !w1f || !w2f) return fail(M3PC_EINVAL, "debug_critic_pack: null array");
    critic_pack(W1, W2, SA, hidden, w1f, w2f);
    return 0;
}

int m3pc_debug_critic(const m3pc_debug_critic_args* a) {
    if (!a) return fail(M3PC_EINVAL, "debug_critic: null arguments");
    if (a->picked) a->picked[0] = 0;
    if (!a->states || !a->actions || !a->om || !a->os || !a->q) return fail(M3PC_EINVAL, "debug_critic: a required pointer is null");
    for (int n = 0; n < 2; ++n)
        if (!a->W1[n] || !a->b1[n] || !a->W2[n] || !a->b2[n] || !a->W3[n] || !a->b3[n]) return fail(M3PC_EINVAL, "debug_critic: network %d lacks a tensor", n);
    if (a->rows < 1) return fail(M3PC_EINVAL, "debug_critic: rows %d", a->rows);
    if (a->S < 1 || a->S > 32 || a->A < 1 || a->A > 32) return fail(M3PC_EINVAL, "debug_critic: S %d / A %d outside [1, 32] (S + A <= 64 floats of LDS per row)", a->S, a->A);
    if (a->hidden < 1 || a->hidden > 256) return fail(M3PC_EINVAL, "debug_critic: hidden %d outside [1, 256] (one thread per hidden unit)", a->hidden);
    const int SA = a->S + a->A, Hd = a->hidden;
    const bool mfma = !a->force_scalar && critic_mfma_covers(a->S, a->A, Hd);
    if (mfma) {
        uintptr_t p16 = 0;
        for (int n = 0; n < 2; ++n) p16 |= (uintptr_t)a->b1[n] | (uintptr_t)a->b2[n] | (uintptr_t)a->W3[n];
        if (p16 & 15) return fail(M3PC_EINVAL, "debug_critic: critic_mfma_kernel reads b1 / b2 / W3 16 bytes at a time");
    }
    // per network: W1T (SA, Hd) | W2T (Hd, Hd) | W1F | W2F.  (A lab hook's shortcut: a function-static buffer that grows and is
    // never freed; calls from two threads would share it)
    const size_t n1 = (size_t)SA * Hd, n2 = (size_t)Hd * Hd, nf1 = mfma ? critic_w1f_floats(Hd) : 0, nf2 = mfma ? critic_w2f_floats(Hd) : 0;
    const size_t per = (n1 + n2 + nf1 + nf2 + 3) & ~(size_t)3;  // (every part a multiple of 4 floats but W1T / W2T at odd sizes)
    std::vector<float> host(2 * per + 8, 0.f);
    size_t off[2][4];
    for (int n = 0; n < 2; ++n) {
        size_t o = n * per;
        // the 16-byte parts first, so that they stay on 16 bytes
        off[n][2] = o; o += nf1;
        off[n][3] = o; o += nf2;
        off[n][0] = o; o += n1;
        off[n][1] = o;
        float* w1t = host.data() + off[n][0];
        float* w2t = host.data() + off[n][1];
        for (int c = 0; c < Hd; ++c)
            for (int f = 0; f < SA; ++f) w1t[(size_t)f * Hd + c] = a->W1[n][(size_t)c * SA + f];
        for (int c = 0; c < Hd; ++c)
            for (int k = 0; k < Hd; ++k) w2t[(size_t)k * Hd + c] = a->W2[n][(size_t)c * Hd + k];
        if (mfma) critic_pack(a->W1[n], a->W2[n], SA, Hd, host.data() + off[n][2], host.data() + off[n][3]);
    }
    static float* dev = nullptr;
    static size_t cap = 0;
    hipStream_t st = (hipStream_t)a->stream;
    HIPCHK(hipStreamSynchronize(st));  // (an earlier call on this stream may still read the buffer)
    if (host.size() > cap) {
        if (dev) HIPCHK(hipFree(dev));
        dev = nullptr;
        cap = 0;
        HIPCHK(hipMalloc((void**)&dev, host.size() * sizeof(float)));
        cap = host.size();
    }
    HIPCHK(hipMemcpy(dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    CriticP p;
    memset(&p, 0, sizeof(p));
    p.states = a->states;
    p.actions = a->actions;
    p.rows = a->rows;
    p.S = a->S;
    p.A = a->A;
    p.hidden = Hd;
    p.om = a->om;
    p.os = a->os;
    for (int n = 0; n < 2; ++n) {
        p.W1T[n] = dev + off[n][0];
        p.W2T[n] = dev + off[n][1];
        p.b1[n] = a->b1[n];
        p.b2[n] = a->b2[n];
        p.W3[n] = a->W3[n];
        p.b3[n] = a->b3[n];
        p.W1F[n] = mfma ? dev + off[n][2] : nullptr;
        p.W2F[n] = mfma ? dev + off[n][3] : nullptr;
    }
    p.q = a->q;
    g_ew_picked = 0;
    launch_critic(p, st);
    return ew_done(a->picked, "debug_critic");
}

int m3pc_debug_sample(const m3pc_debug_sample_args* a) {
    if (!a) return fail(M3PC_EINVAL, "debug_sample: null arguments");
    if (a->picked) a->picked[0] = 0;
    if (a->mode < 0 || a->mode > 2) return fail(M3PC_EINVAL, "debug_sample: mode %d", a->mode);
    if (a->T < 1 || a->A < 1 || a->n_count < 1) return fail(M3PC_EINVAL, "debug_sample: T / A / n_count below 1");
    if (a->idx < 0 || a->idx > a->T) return fail(M3PC_EINVAL, "debug_sample: idx %d outside [0, T = %d]", a->idx, a->T);
    if (a->h < a->T - a->idx) return fail(M3PC_EINVAL, "debug_sample: h %d below T - idx = %d (a sampled step would leave its row)", a->h, a->T - a->idx);
    if (!a->cand || !a->eps) return fail(M3PC_EINVAL, "debug_sample: cand and eps are required");
    if (a->idx > 0 && !a->hist_actions) return fail(M3PC_EINVAL, "debug_sample: idx > 0 without hist_actions");
    if ((a->mode <= 1 && !a->loc) || (a->mode == 0 && !a->sd)) return fail(M3PC_EINVAL, "debug_sample: mode %d without loc / sd", a->mode);
    if (a->eps_rows < 1 || a->hist_windows < 1 || (a->hist_windows > 1 && !a->widx)) return fail(M3PC_EINVAL, "debug_sample: eps_rows / hist_windows");
    if (!a->index && (a->n_begin < 0 || (long long)a->n_begin + a->n_count > a->eps_rows))
        return fail(M3PC_EINVAL, "debug_sample: rows [%d, %d + %d) outside the %lld rows of eps", a->n_begin, a->n_begin, a->n_count, a->eps_rows);
    SampleP p;
    memset(&p, 0, sizeof(p));
    p.hist_actions = a->hist_actions;
    p.loc = a->loc;
    p.sd = a->sd;
    p.eps = a->eps;
    p.mode = a->mode;
    p.T = a->T;
    p.A = a->A;
    p.idx = a->idx;
    p.h = a->h;
    p.n_begin = a->n_begin;
    p.n_count = a->n_count;
    p.widx = a->widx;
    p.index = a->index;
    p.cand = a->cand;
    p.sample_actions = a->sample_actions;
    p.loc_out = a->loc_out;
    p.sd_out = a->sd_out;
    g_ew_picked = 0;
    launch_sample(p, (hipStream_t)a->stream);
    return ew_done(a->picked, "debug_sample");
}

int m3pc_debug_score(const m3pc_debug_score_args* a) {
    if (!a) return fail(M3PC_EINVAL, "debug_score: null arguments");
    if (a->picked) a->picked[0] = 0;
    if (!a->rewards || !a->boot || !a->expect_return) return fail(M3PC_EINVAL, "debug_score: rewards, boot and expect_return are required");
    if (a->n < 1 || a->h < 1) return fail(M3PC_EINVAL, "debug_score: n %d / h %d", a->n, a->h);
    if (a->scatter_out && !a->scatter_index) return fail(M3PC_EINVAL, "debug_score: scatter_out without scatter_index");
    ScoreP p;
    memset(&p, 0, sizeof(p));
    p.rewards = a->rewards;
    p.boot = a->boot;
    p.n = a->n;
    p.h = a->h;
    p.boot_scale = a->boot_scale;
    p.gamma = a->gamma;
    p.lmbda = a->lmbda;
    p.expect_return = a->expect_return;
    p.boot_out = a->boot_out;
    p.scatter_index = a->scatter_index;
    p.scatter_out = a->scatter_out;
    g_ew_picked = 0;
    launch_score(p, (hipStream_t)a->stream);
    return ew_done(a->picked, "debug_score");
}

int m3pc_debug_gather_rows(const m3pc_debug_gather_args* a) {
    if (!a) return fail(M3PC_EINVAL, "debug_gather_rows: null arguments");
    if (a->picked) a->picked[0] = 0;
    if (!a->out && !a->outb) return fail(M3PC_EINVAL, "debug_gather_rows: neither out nor outb");
    if (!a->rowsrc || a->batch < 1 || a->rows_per_batch < 1 || (long long)a->batch * a->rows_per_batch > 0x7fffffffLL)
        return fail(M3PC_EINVAL, "debug_gather_rows: rowsrc / batch / rows_per_batch");
    if (ew_bad_d(a->d)) return fail(M3PC_EINVAL, "debug_gather_rows: d %d is not a multiple of 64 in [64, 1024]", a->d);
    if ((((uintptr_t)a->Xe | (uintptr_t)a->table | (uintptr_t)a->out) & 15) || a->xe_bstride % 4 || a->xe_bstride < 0)
        return fail(M3PC_EINVAL, "debug_gather_rows: rows move 16 bytes at a time (Xe, table, out, xe_bstride %% 4)");
    if (a->Xe && a->batch > 1 && a->xe_bstride < (long long)a->xe_rows * a->d)
        return fail(M3PC_EINVAL, "debug_gather_rows: xe_bstride %lld below xe_rows * d = %lld (the batch elements' rows would alias)", a->xe_bstride, (long long)a->xe_rows * a->d);
    for (int i = 0; i < a->rows_per_batch; ++i) {
        const int s = a->rowsrc[i];
        if (s >= 0 ? (!a->Xe || s >= a->xe_rows) : (!a->table || -(long long)s - 1 >= a->table_rows))
            return fail(M3PC_EINVAL, "debug_gather_rows: rowsrc[%d] = %d outside its source (%d rows of Xe, %d of the table)", i, s, a->xe_rows, a->table_rows);
    }
    static int* dsrc = nullptr;  // (a lab hook's shortcut, as in m3pc_debug_gemm_ex)
    static int cap = 0;
    hipStream_t st = (hipStream_t)a->stream;
    HIPCHK(hipStreamSynchronize(st));
    if (a->rows_per_batch > cap) {
        if (dsrc) HIPCHK(hipFree(dsrc));
        dsrc = nullptr;
        cap = 0;
        HIPCHK(hipMalloc((void**)&dsrc, (size_t)a->rows_per_batch * sizeof(int)));
        cap = a->rows_per_batch;
    }
    HIPCHK(hipMemcpy(dsrc, a->rowsrc, (size_t)a->rows_per_batch * sizeof(int), hipMemcpyHostToDevice));
    GatherP p;
    memset(&p, 0, sizeof(p));
    p.Xe = a->Xe;
    p.xe_bstride = a->xe_bstride;
    p.table = a->table;
    p.rowsrc = dsrc;
    p.rows_per_batch = a->rows_per_batch;
    p.batch = a->batch;
    p.d = a->d;
    p.out = a->out;
    p.outb = (bf16_t*)a->outb;
    g_ew_picked = 0;
    launch_gather_rows(p, st);
    return ew_done(a->picked, "debug_gather_rows");
}

static int ew_overlay_check(const char* what, const void* pred, const void* in, const void* out, long long windows, int T, int D, int idx) {
    if (!pred || !in || !out) return fail(M3PC_EINVAL, "%s: null pointer", what);
    if (windows < 1 || T < 1 || D < 1 || windows > (1LL << 40) / ((long long)T * D)) return fail(M3PC_EINVAL, "%s: windows / T / D", what);
    if (idx < 0 || idx > T - 1) return fail(M3PC_EINVAL, "%s: idx %d outside [0, T - 1 = %d]", what, idx, T - 1);
    return 0;
}
int m3pc_debug_goal_overlay(float* pred, const float* states_in, float* states_out, long long windows, int T, int D, int idx,
                            const float* mean, const float* stdv, int normalize, void* stream, int* picked) {
    if (picked) picked[0] = 0;
    CHK(ew_overlay_check("debug_goal_overlay", pred, states_in, states_out, windows, T, D, idx));
    if (normalize && (!mean || !stdv)) return fail(M3PC_EINVAL, "debug_goal_overlay: normalize without mean / stdv");
    g_ew_picked = 0;
    launch_goal_overlay(pred, states_in, states_out, windows * T, T, D, idx, mean, stdv, normalize ? 1 : 0, (hipStream_t)stream);
    return ew_done(picked, "debug_goal_overlay");
}
int m3pc_debug_goal_overlay_rows(const float* pred, const float* states_in, float* states_out, long long windows, int T, int D, int idx,
                                 int nq, void* stream, int* picked) {
    if (picked) picked[0] = 0;
    CHK(ew_overlay_check("debug_goal_overlay_rows", pred, states_in, states_out, windows, T, D, idx));
    const int n_over = idx + 1 + (T - 1 - (idx + 2) > 0 ? T - 1 - (idx + 2) : 0);  // rows t <= idx, then idx + 2 <= t <= T - 2
    if (nq < n_over) return fail(M3PC_EINVAL, "debug_goal_overlay_rows: nq %d below the %d overlay rows of a window", nq, n_over);
    g_ew_picked = 0;
    launch_goal_overlay_rows(pred, states_in, states_out, windows, T, D, idx, nq, (hipStream_t)stream);
    return ew_done(picked, "debug_goal_overlay_rows");
}

// ---- csrc/mtm_grad.hip, kernel by kernel (include/m3pc_hip_debug.h, "MTM-gradient kernel ids"; tests/test_mtm_grad_kernel_edges_gpu.py).
// Every hook checks first (no HIP call before a refusal), fills the kernel's parameter structure, goes through the launcher
// m3pc_mtm_grad uses and reports what that launcher recorded.
static const long long MG_INT_MAX = 0x7fffffffLL;
static void mg_begin(int* picked) {
    if (picked) picked[0] = picked[1] = 0;
    g_mg_picked = 0;
    g_mg_picked_set = 0;
}
static int mg_done(int* picked, const char* what) {
    if (picked) {
        picked[0] = g_mg_picked;
        picked[1] = (int)g_mg_picked_set;
    }
    return check_launch(what);
}
static RMap mg_map(const int* m) { return RMap{m[0], m[1], m[2]}; }
// the largest index of an operand with `outer` rows or columns, -1 if its description is bad
static long long mg_op_last(const m3pc_debug_mg_op& o, int outer, int K) {
    if (!o.p || o.s_o < 0 || o.s_k < 0 || ew_bad_map(o.map) || o.len < 1) return -1;
    const RMap m = mg_map(o.map);
    const long long ro = o.map_k ? outer - 1 : rmap(m, outer - 1), rk = o.map_k ? rmap(m, K - 1) : K - 1;
    if (ro > MG_INT_MAX || rk > MG_INT_MAX || (o.s_o && ro > MG_INT_MAX / o.s_o) || (o.s_k && rk > MG_INT_MAX / o.s_k)) return -1;
    return ro * o.s_o + rk * o.s_k;
}

// a site of the hooks with keep masks (m3pc_debug_mg_drop): refused, or the launch's DropG (thr == 0: off)
static int mg_drop_fill(const m3pc_debug_mg_drop& d, unsigned int array, unsigned long long quads, const char* who, DropG* out) {
    if (!std::isfinite(d.p) || d.p < 0.0 || d.p >= 1.0) return fail(M3PC_EINVAL, "%s: dropout p %g is not a finite number in [0, 1)", who, d.p);
    if (d.site < 0 || d.site > 255) return fail(M3PC_EINVAL, "%s: dropout site %d outside [0, 255]", who, d.site);
    if (quads > (1ull << 32)) return fail(M3PC_EINVAL, "%s: the site has more than 2^32 quads (%llu)", who, quads);
    *out = mg_drop_make(d.p, d.seed, d.draw);
    out->c3 = array | (unsigned int)d.site << 8;
    return 0;
}

static int mg_gemm_hook(const m3pc_debug_mg_gemm_args* a, const m3pc_debug_mg_drop* drop) {
    if (!a) return fail(M3PC_EINVAL, "debug_mg_gemm: null arguments");
    if (a->picked) a->picked[0] = a->picked[1] = 0;
    if (!a->A.p || !a->B.p || !a->C) return fail(M3PC_EINVAL, "debug_mg_gemm: A, B and C are required");
    if (a->M < 1 || a->N < 1 || a->K < 1) return fail(M3PC_EINVAL, "debug_mg_gemm: M %d, N %d, K %d: each must be >= 1", a->M, a->N, a->K);
    const long long la = mg_op_last(a->A, a->M, a->K), lb = mg_op_last(a->B, a->N, a->K);
    if (la < 0 || la >= a->A.len || la > MG_INT_MAX) return fail(M3PC_EINVAL, "debug_mg_gemm: operand A (strides, row map or an index beyond its %lld floats)", a->A.len);
    if (lb < 0 || lb >= a->B.len || lb > MG_INT_MAX) return fail(M3PC_EINVAL, "debug_mg_gemm: operand B (strides, row map or an index beyond its %lld floats)", a->B.len);
    if (ew_bad_map(a->cmap) || a->ldc < a->N || a->ldc > MG_INT_MAX) return fail(M3PC_EINVAL, "debug_mg_gemm: cmap / ldc %lld below N %d", a->ldc, a->N);
    const long long rc = rmap(mg_map(a->cmap), a->M - 1);
    if (rc > MG_INT_MAX / a->ldc || rc * a->ldc + a->N - 1 >= a->c_len)
        return fail(M3PC_EINVAL, "debug_mg_gemm: row %lld of C lies beyond its %lld floats", rc, a->c_len);
    if (a->bias2 && !a->bias) return fail(M3PC_EINVAL, "debug_mg_gemm: bias2 without bias");
    if (a->pos && a->pos_T < 1) return fail(M3PC_EINVAL, "debug_mg_gemm: pos with pos_T %d < 1", a->pos_T);
    GemmG p;
    memset(&p, 0, sizeof(p));
    p.A = GOp{a->A.p, a->A.s_o, a->A.s_k, mg_map(a->A.map), a->A.map_k ? 1 : 0, 0};
    p.B = GOp{a->B.p, a->B.s_o, a->B.s_k, mg_map(a->B.map), a->B.map_k ? 1 : 0, 0};
    p.C = a->C;
    p.ldc = a->ldc;
    p.cmap = mg_map(a->cmap);
    p.M = a->M;
    p.N = a->N;
    p.K = a->K;
    p.bias = a->bias;
    p.bias2 = a->bias2;
    p.pos = a->pos;
    p.pos_T = a->pos ? a->pos_T : 1;
    p.res = a->res;
    p.gelu_aux = a->gelu_aux;
    p.gelu_out = a->gelu_out;
    p.accumulate = a->accumulate ? 1 : 0;
    p.splitk = a->splitk ? 1 : 0;
    if (drop) {
        CHK(mg_drop_fill(*drop, MG_DROP_MATRIX, (unsigned long long)((a->M + 3) / 4) * a->N, "debug_mg_gemm_drop", &p.drop));
        if (p.drop.thr && a->splitk) return fail(M3PC_EINVAL, "debug_mg_gemm_drop: no dropout form of the split-k product");
    }
    mg_begin(a->picked);
    mg_launch_gemm(p, (hipStream_t)a->stream);
    return mg_done(a->picked, "debug_mg_gemm");
}
int m3pc_debug_mg_gemm(const m3pc_debug_mg_gemm_args* a) { return mg_gemm_hook(a, nullptr); }
int m3pc_debug_mg_gemm_drop(const m3pc_debug_mg_gemm_drop_args* a) {
    if (!a) return fail(M3PC_EINVAL, "debug_mg_gemm_drop: null arguments");
    return mg_gemm_hook(&a->g, &a->drop);
}

int m3pc_debug_mg_layernorm(const m3pc_debug_mg_ln_args* a) {
    if (!a) return fail(M3PC_EINVAL, "debug_mg_layernorm: null arguments");
    if (a->picked) a->picked[0] = a->picked[1] = 0;
    if (!a->X || !a->g || !a->st) return fail(M3PC_EINVAL, "debug_mg_layernorm: X, g and st are required");
    if (a->backward ? (!a->dY || !a->dX) : (!a->b || !a->Y)) return fail(M3PC_EINVAL, "debug_mg_layernorm: %s", a->backward ? "backward needs dY and dX" : "forward needs b and Y");
    if (a->rows < 1 || a->d < 1 || (long long)a->rows * a->d > MG_INT_MAX) return fail(M3PC_EINVAL, "debug_mg_layernorm: rows %d, d %d", a->rows, a->d);
    if (ew_bad_map(a->xmap)) return fail(M3PC_EINVAL, "debug_mg_layernorm: row map");
    const long long last = rmap(mg_map(a->xmap), a->rows - 1);
    if (last >= a->x_rows || a->x_rows > MG_INT_MAX / a->d) return fail(M3PC_EINVAL, "debug_mg_layernorm: row %lld of X beyond its x_rows %lld", last, a->x_rows);
    LnG p;
    memset(&p, 0, sizeof(p));
    p.X = a->X;
    p.xmap = mg_map(a->xmap);
    p.g = a->g;
    p.b = a->b;
    p.Y = a->Y;
    p.st = a->st;
    p.dY = a->dY;
    p.dX = a->dX;
    p.rows = a->rows;
    p.d = a->d;
    p.accumulate = a->accumulate ? 1 : 0;
    mg_begin(a->picked);
    if (a->backward)
        mg_launch_ln_bwd(p, (hipStream_t)a->stream);
    else
        mg_launch_ln_fwd(p, (hipStream_t)a->stream);
    return mg_done(a->picked, "debug_mg_layernorm");
}

int m3pc_debug_mg_colsum(const m3pc_debug_mg_colsum_args* a) {
    if (!a) return fail(M3PC_EINVAL, "debug_mg_colsum: null arguments");
    if (a->picked) a->picked[0] = a->picked[1] = 0;
    if (!a->dY || !a->out0 || !a->part) return fail(M3PC_EINVAL, "debug_mg_colsum: dY, out0 and part are required");
    if ((a->X == nullptr) != (a->st == nullptr) || (a->out1 && !a->X)) return fail(M3PC_EINVAL, "debug_mg_colsum: X and st come together, out1 needs them");
    if (a->nseq < 1 || a->n < 1 || a->n > 64) return fail(M3PC_EINVAL, "debug_mg_colsum: nseq %d < 1 or n %d outside [1, 64]", a->nseq, a->n);
    if (a->j0 < 0 || a->L < 1 || (long long)a->j0 + a->n > a->L) return fail(M3PC_EINVAL, "debug_mg_colsum: j0 %d + n %d beyond L %d", a->j0, a->n, a->L);
    if (a->C < 1 || a->ldy < a->C) return fail(M3PC_EINVAL, "debug_mg_colsum: C %d < 1 or ldy %lld below it", a->C, a->ldy);
    const long long total = (long long)a->nseq * a->n, need_rows = (long long)(a->nseq - 1) * a->L + a->j0 + a->n;
    if (total > MG_INT_MAX || need_rows > MG_INT_MAX / a->ldy || a->buf_rows < need_rows)
        return fail(M3PC_EINVAL, "debug_mg_colsum: the rows reach buffer row %lld, buf_rows is %lld", need_rows - 1, a->buf_rows);
    const size_t need = mg_colsum_doubles(total, a->C);
    if (a->part_doubles < 0 || (size_t)a->part_doubles < need)
        return fail(M3PC_EINVAL, "debug_mg_colsum: part holds %lld doubles, %d chunks of 2 C need %zu", a->part_doubles, mg_colsum_chunks(total), need);
    ColG p;
    memset(&p, 0, sizeof(p));
    p.dY = a->dY;
    p.dy_compact = a->dy_compact ? 1 : 0;
    p.ldy = a->ldy;
    p.X = a->X;
    p.st = a->st;
    p.nseq = a->nseq;
    p.L = a->L;
    p.j0 = a->j0;
    p.n = a->n;
    p.sel = a->sel;
    p.C = a->C;
    p.out0 = a->out0;
    p.out1 = a->out1;
    mg_begin(a->picked);
    mg_launch_colsum(p, a->part, (hipStream_t)a->stream);
    return mg_done(a->picked, "debug_mg_colsum");
}

static int mg_attention_hook(const m3pc_debug_mg_attn_args* a, const m3pc_debug_mg_drop* drop) {
    if (!a) return fail(M3PC_EINVAL, "debug_mg_attention: null arguments");
    if (a->picked) a->picked[0] = a->picked[1] = 0;
    if (a->which < 0 || a->which > 3) return fail(M3PC_EINVAL, "debug_mg_attention: which %d outside [0, 3]", a->which);
    if (a->L < 1 || a->L > MG_ATT_MAX_L) return fail(M3PC_EINVAL, "debug_mg_attention: L %d outside [1, %d] (a row of P is held in LDS)", a->L, MG_ATT_MAX_L);
    if (a->B < 1 || a->nh < 1 || a->hd < 1 || a->d < 1 || (long long)a->nh * a->hd != a->d)
        return fail(M3PC_EINVAL, "debug_mg_attention: B %d, n_head %d x head dim %d against d %d", a->B, a->nh, a->hd, a->d);
    if ((long long)a->B * a->nh * a->L * a->L > MG_INT_MAX || (long long)a->B * a->L * 3 * a->d > MG_INT_MAX)
        return fail(M3PC_EINVAL, "debug_mg_attention: the element counts exceed int");
    const bool need_qkv = a->which != 1, need_o = a->which == 0, need_do = a->which == 1 || a->which == 2, need_dqkv = a->which != 0;
    if (!a->P || (need_qkv && !a->QKV) || (need_o && !a->O) || (need_do && !a->dO) || (need_dqkv && !a->dQKV))
        return fail(M3PC_EINVAL, "debug_mg_attention: a pointer kernel %d uses is null", a->which);
    AttG p;
    memset(&p, 0, sizeof(p));
    p.QKV = a->QKV;
    p.P = a->P;
    p.O = a->O;
    p.dO = a->dO;
    p.dQKV = a->dQKV;
    p.B = a->B;
    p.L = a->L;
    p.d = a->d;
    p.nh = a->nh;
    p.hd = a->hd;
    p.scale = a->scale;
    if (drop)
        CHK(mg_drop_fill(*drop, MG_DROP_ATTN, (unsigned long long)a->B * a->nh * a->L * ((a->L + 3) / 4), "debug_mg_attention_drop", &p.drop));
    hipStream_t st = (hipStream_t)a->stream;
    mg_begin(a->picked);
    if (a->which == 0)
        mg_launch_attn_fwd(p, st);
    else if (a->which == 2)
        mg_launch_attn_row(p, st);
    else
        mg_launch_attn_col(p, a->which == 1 ? 0 : 1, st);
    return mg_done(a->picked, "debug_mg_attention");
}
int m3pc_debug_mg_attention(const m3pc_debug_mg_attn_args* a) { return mg_attention_hook(a, nullptr); }
int m3pc_debug_mg_attention_drop(const m3pc_debug_mg_attn_drop_args* a) {
    if (!a) return fail(M3PC_EINVAL, "debug_mg_attention_drop: null arguments");
    return mg_attention_hook(&a->a, &a->drop);
}

int m3pc_debug_mg_drop_rows(const m3pc_debug_mg_drop_rows_args* a) {
    if (!a) return fail(M3PC_EINVAL, "debug_mg_drop_rows: null arguments");
    if (a->picked) a->picked[0] = a->picked[1] = 0;
    if (!a->dX || !a->dY) return fail(M3PC_EINVAL, "debug_mg_drop_rows: dX and dY are required");
    if (a->R < 1 || a->C < 1 || (long long)a->R * a->C > MG_INT_MAX) return fail(M3PC_EINVAL, "debug_mg_drop_rows: R %d, C %d", a->R, a->C);
    DropRowsG p = {a->dX, a->dY, a->R, a->C, {}};
    CHK(mg_drop_fill(a->drop, MG_DROP_MATRIX, (unsigned long long)((a->R + 3) / 4) * a->C, "debug_mg_drop_rows", &p.drop));
    if (!p.drop.thr) return fail(M3PC_EINVAL, "debug_mg_drop_rows: p %g drops nothing: m3pc_mtm_grad makes no such launch", a->drop.p);
    mg_begin(a->picked);
    mg_launch_drop_rows(p, (hipStream_t)a->stream);
    return mg_done(a->picked, "debug_mg_drop_rows");
}

int m3pc_debug_mtm_keep(const m3pc_debug_mg_drop* d, int attention, long long R, int C, unsigned char* keep, void* stream, int* picked) {
    if (picked) picked[0] = picked[1] = 0;
    if (!d || !keep) return fail(M3PC_EINVAL, "debug_mtm_keep: null argument");
    if (R < 1 || C < 1 || R > (1ll << 40)) return fail(M3PC_EINVAL, "debug_mtm_keep: R %lld, C %d", R, C);
    DropG g;
    const unsigned long long quads = attention ? (unsigned long long)R * ((C + 3) / 4) : (unsigned long long)((R + 3) / 4) * C;
    CHK(mg_drop_fill(*d, attention ? MG_DROP_ATTN : MG_DROP_MATRIX, quads, "debug_mtm_keep", &g));
    if (R > MG_INT_MAX / C) return fail(M3PC_EINVAL, "debug_mtm_keep: R %lld x C %d bytes beyond int", R, C);
    mg_begin(picked);
    mg_launch_keep(g, R, C, keep, (hipStream_t)stream);
    return mg_done(picked, "debug_mtm_keep");
}

int m3pc_debug_mg_tokens(const m3pc_debug_mg_tokens_args* a) {
    if (!a) return fail(M3PC_EINVAL, "debug_mg_tokens: null arguments");
    if (a->picked) a->picked[0] = a->picked[1] = 0;
    if (a->which < 0 || a->which > 3) return fail(M3PC_EINVAL, "debug_mg_tokens: which %d outside [0, 3]", a->which);
    if (a->B < 1 || a->T < 1 || a->T > 64 || a->d < 1) return fail(M3PC_EINVAL, "debug_mg_tokens: B %d, d %d, T %d outside [1, 64]", a->B, a->d, a->T);
    int Le = 0;
    for (int k = 0; k < 4; ++k) {
        if (a->T < 64 && (a->bits[k] >> a->T)) return fail(M3PC_EINVAL, "debug_mg_tokens: bits[%d] has a bit at or above T %d", k, a->T);
        if (a->kept[k] != __builtin_popcountll(a->bits[k]) || a->eoff[k] != Le)
            return fail(M3PC_EINVAL, "debug_mg_tokens: kept[%d] %d / eoff[%d] %d inconsistent with bits", k, a->kept[k], k, a->eoff[k]);
        Le += a->kept[k];
    }
    if (a->Le != Le || Le < 1) return fail(M3PC_EINVAL, "debug_mg_tokens: Le %d, the masks keep %d tokens", a->Le, Le);
    if ((long long)a->B * 4 * a->T * a->d > MG_INT_MAX) return fail(M3PC_EINVAL, "debug_mg_tokens: B 4 T d exceeds int");
    if (a->which == 0) {
        if (!a->X || !a->pos) return fail(M3PC_EINVAL, "debug_mg_tokens: embed needs X and pos");
        for (int k = 0; k < 4; ++k)
            if (a->kept[k] && (!a->tok[k] || !a->W[k] || !a->bias[k] || !a->pdim[k] || a->feat[k] < 1))
                return fail(M3PC_EINVAL, "debug_mg_tokens: embed needs tok / W / bias / pdim and feat >= 1 of key %d", k);
    } else if (a->which == 1) {
        if (!a->src || !a->dst) return fail(M3PC_EINVAL, "debug_mg_tokens: gather needs src and dst");
        for (int k = 0; k < 4; ++k)
            if (!a->mtok[k]) return fail(M3PC_EINVAL, "debug_mg_tokens: gather needs mtok of key %d", k);
    } else if (a->which == 2) {
        if (!a->src || !a->dst) return fail(M3PC_EINVAL, "debug_mg_tokens: scatter needs src and dst");
    } else {
        if (a->key < 0 || a->key > 3 || a->kept[a->key] < 1 || a->feat[a->key] < 1 || !a->tok[a->key] || !a->out)
            return fail(M3PC_EINVAL, "debug_mg_tokens: tokv needs a key in [0, 3] with kept >= 1, feat >= 1, its tok and out");
        if ((long long)a->B * a->T * a->feat[a->key] > MG_INT_MAX) return fail(M3PC_EINVAL, "debug_mg_tokens: B T feat exceeds int");
    }
    EmbG p;
    memset(&p, 0, sizeof(p));
    for (int k = 0; k < 4; ++k) {
        p.tok[k] = a->tok[k];
        p.W[k] = a->W[k];
        p.bias[k] = a->bias[k];
        p.pdim[k] = a->pdim[k];
        p.mtok[k] = a->mtok[k];
        p.bits[k] = a->bits[k];
        p.kept[k] = a->kept[k];
        p.eoff[k] = a->eoff[k];
        p.feat[k] = a->feat[k];
    }
    p.pos = a->pos;
    p.B = a->B;
    p.T = a->T;
    p.d = a->d;
    p.Le = a->Le;
    p.X = a->X;
    p.src = a->src;
    p.dst = a->dst;
    hipStream_t st = (hipStream_t)a->stream;
    mg_begin(a->picked);
    if (a->which == 0)
        mg_launch_embed(p, st);
    else if (a->which == 1)
        mg_launch_gather(p, st);
    else if (a->which == 2)
        mg_launch_scatter(p, st);
    else
        mg_launch_tokv(p, a->key, a->out, st);
    return mg_done(a->picked, "debug_mg_tokens");
}

int m3pc_debug_mg_std(const float* ls, float* sd, long long n, void* stream, int* picked) {
    if (picked) picked[0] = picked[1] = 0;
    if (!ls || !sd || n < 1) return fail(M3PC_EINVAL, "debug_mg_std: null pointer or n %lld < 1", n);
    mg_begin(picked);
    mg_launch_std(ls, sd, n, (hipStream_t)stream);
    return mg_done(picked, "debug_mg_std");
}

int m3pc_debug_mg_loss_bwd(const m3pc_debug_mg_loss_bwd_args* a) {
    if (!a) return fail(M3PC_EINVAL, "debug_mg_loss_bwd: null arguments");
    if (a->picked) a->picked[0] = a->picked[1] = 0;
    bool null = !a->mu || !a->sd || !a->ls || !a->eps || !a->dmu || !a->dls;
    for (int j = 0; j < 3; ++j) null = null || !a->pred[j] || !a->dpred[j];
    for (int k = 0; k < 4; ++k) null = null || !a->tgt[k];
    if (null) return fail(M3PC_EINVAL, "debug_mg_loss_bwd: null pointer");
    if (a->batch < 1 || a->S < 1 || a->A < 1 || a->T < 1 || a->T > 64) return fail(M3PC_EINVAL, "debug_mg_loss_bwd: batch %d, S %d, A %d, T %d outside [1, 64]", a->batch, a->S, a->A, a->T);
    for (int k = 0; k < 4; ++k)
        if (a->T < 64 && (a->mask[k] >> a->T)) return fail(M3PC_EINVAL, "debug_mg_loss_bwd: mask[%d] has a bit at or above T %d", k, a->T);
    if (a->flags & ~(M3PC_MTM_NORM_L2 | M3PC_MTM_CLIP_ACTIONS)) return fail(M3PC_EINVAL, "debug_mg_loss_bwd: unknown flag bits 0x%x", a->flags);
    if (a->loss_keys < 0 || a->loss_keys > 15) return fail(M3PC_EINVAL, "debug_mg_loss_bwd: loss_keys %d outside [0, 15]", a->loss_keys);
    if ((long long)a->batch * a->T * ((long long)a->S + 2 + a->A) > MG_INT_MAX) return fail(M3PC_EINVAL, "debug_mg_loss_bwd: batch T (S + 2 + A) exceeds int");
    LossBwdG p;
    memset(&p, 0, sizeof(p));
    for (int j = 0; j < 3; ++j) {
        p.pred[j] = a->pred[j];
        p.dpred[j] = a->dpred[j];
    }
    for (int k = 0; k < 4; ++k) {
        p.tgt[k] = a->tgt[k];
        p.mask[k] = a->mask[k];
    }
    p.mu = a->mu;
    p.sd = a->sd;
    p.ls = a->ls;
    p.eps = a->eps;
    p.dmu = a->dmu;
    p.dls = a->dls;
    p.batch = a->batch;
    p.T = a->T;
    p.S = a->S;
    p.A = a->A;
    p.flags = a->flags;
    p.loss_keys = a->loss_keys;
    p.entropy_reg = a->entropy_reg;
    p.inv_cnt = a->inv_cnt;
    mg_begin(a->picked);
    mg_launch_loss_bwd(p, (hipStream_t)a->stream);
    return mg_done(a->picked, "debug_mg_loss_bwd");
}

// ---- csrc/iql.hip, kernel by kernel (include/m3pc_hip_debug.h, "IQL-trainer kernel ids"; tests/test_iql_kernel_edges_gpu.py).
// Every hook checks first (no HIP call before a refusal), fills the kernel's parameter structure, goes through the launcher
// the trainer uses and reports what that launcher recorded.
static void iql_begin(int* picked) {
    if (picked) picked[0] = picked[1] = 0;
    g_iql_picked = 0;
    g_iql_picked_set = 0;
}
static int iql_done(int* picked, const char* what) {
    if (picked) {
        picked[0] = g_iql_picked;
        picked[1] = (int)g_iql_picked_set;
    }
    return check_launch(what);
}
static bool iql_off16(const void* p) { return ((uintptr_t)p & 15) != 0; }
static NetP iql_net(const m3pc_debug_iql_net& n) { return NetP{n.W1, n.b1, n.W2, n.b2, n.W3, n.b3, n.in, n.out}; }
static bool iql_net_null(const m3pc_debug_iql_net& n) { return !n.W1 || !n.b1 || !n.W2 || !n.b2 || !n.W3 || !n.b3; }
static int iql_common(const m3pc_debug_iql_args* a, const char* who) {
    if (!a) return fail(M3PC_EINVAL, "%s: null arguments", who);
    if (a->picked) a->picked[0] = a->picked[1] = 0;
    if (a->H != 64 && a->H != 128 && a->H != 256) return fail(M3PC_EINVAL, "%s: hidden %d is none of 64, 128, 256", who, a->H);
    if (a->B < 1 || a->B > IQL_MAX_BATCH) return fail(M3PC_EINVAL, "%s: B %d outside [1, %d]", who, a->B, IQL_MAX_BATCH);
    if (a->A < 1 || a->A > 32) return fail(M3PC_EINVAL, "%s: A %d outside [1, 32]", who, a->A);
    if (a->S < 1 || a->S > 64) return fail(M3PC_EINVAL, "%s: S %d outside [1, 64]", who, a->S);
    return 0;
}
static int iql_bad_in(const m3pc_debug_iql_args* a, const m3pc_debug_iql_net& n, const char* who) {
    if (n.in < 1 || n.in > 64 || n.in > a->S + a->A) return fail(M3PC_EINVAL, "%s: in %d outside [1, 64] or above S + A = %d", who, n.in, a->S + a->A);
    if (n.in > a->S && !a->action) return fail(M3PC_EINVAL, "%s: a network is wider than S and action is null", who);
    return 0;
}
static IqlP iql_fill(const m3pc_debug_iql_args* a) {
    IqlP p;
    memset(&p, 0, sizeof(p));
    for (int t = 0; t < 6; ++t) p.net[t] = iql_net(a->net[t]);
    for (int t = 0; t < IQL_NETS; ++t) p.am[t] = iql_net(a->am[t]), p.av[t] = iql_net(a->av[t]);
    p.log_std = a->log_std, p.ls_m = a->ls_m, p.ls_v = a->ls_v;
    p.om = a->om, p.os = a->os;
    p.state = a->state, p.action = a->action, p.reward = a->reward, p.next_state = a->next_state, p.done = a->done;
    p.h1 = a->h1, p.h2 = a->h2, p.out = a->out, p.d3 = a->d3, p.d2 = a->d2, p.d1 = a->d1, p.losses = a->losses;
    iql_set_rows(p, a->B);
    p.H = a->H, p.NT = a->H / 32, p.S = a->S, p.A = a->A;
    p.npass = a->npass;
    for (int f = 0; f < IQL_PASSES; ++f) p.pass_net[f] = a->pass_net[f], p.pass_next[f] = a->pass_next[f] ? 1 : 0;
    p.expectile = a->expectile, p.beta = a->beta, p.gamma = a->gamma, p.omt = a->omt, p.tau = a->tau;
    p.omb1 = a->omb1, p.b2 = a->b2, p.omb2 = a->omb2;
    for (int t = 0; t < IQL_NETS; ++t) p.step_size[t] = a->step_size[t];
    p.sqrt_bc2 = a->sqrt_bc2, p.eps = a->eps;
    return p;
}

int m3pc_debug_iql_forward(const m3pc_debug_iql_args* a) {
    const char* who = "debug_iql_forward";
    CHK(iql_common(a, who));
    if (a->which < 1 || a->which > 3) return fail(M3PC_EINVAL, "%s: layer %d outside [1, 3]", who, a->which);
    if (a->npass < 1 || a->npass > IQL_PASSES) return fail(M3PC_EINVAL, "%s: npass %d outside [1, %d]", who, a->npass, IQL_PASSES);
    for (int f = 0; f < a->npass; ++f) {
        if (a->pass_net[f] < 0 || a->pass_net[f] > 5) return fail(M3PC_EINVAL, "%s: pass_net[%d] %d outside [0, 5]", who, f, a->pass_net[f]);
        const m3pc_debug_iql_net& n = a->net[a->pass_net[f]];
        if (a->which == 1) {
            if (!n.W1 || !n.b1 || !a->om || !a->os || !a->h1 || !(a->pass_next[f] ? a->next_state : a->state)) return fail(M3PC_EINVAL, "%s: null pointer", who);
            CHK(iql_bad_in(a, n, who));
            if (iql_off16(n.b1) || iql_off16(a->h1)) return fail(M3PC_EINVAL, "%s: b1 / h1 off 16 bytes", who);
        } else if (a->which == 2) {
            if (!n.W2 || !n.b2 || !a->h1 || !a->h2) return fail(M3PC_EINVAL, "%s: null pointer", who);
            if (iql_off16(n.W2) || iql_off16(n.b2) || iql_off16(a->h1) || iql_off16(a->h2)) return fail(M3PC_EINVAL, "%s: W2 / b2 / h1 / h2 off 16 bytes", who);
        } else {
            if (!n.W3 || !n.b3 || !a->h2 || !a->out) return fail(M3PC_EINVAL, "%s: null pointer", who);
            if (n.out < 1 || n.out > IQL_OUTW) return fail(M3PC_EINVAL, "%s: out %d outside [1, %d]", who, n.out, IQL_OUTW);
            if (iql_off16(n.W3) || iql_off16(a->h2) || iql_off16(a->out)) return fail(M3PC_EINVAL, "%s: W3 / h2 / out off 16 bytes", who);
        }
    }
    const IqlP p = iql_fill(a);
    iql_begin(a->picked);
    iql_launch_fwd(p, a->which, (hipStream_t)a->stream);
    return iql_done(a->picked, who);
}

int m3pc_debug_iql_loss(const m3pc_debug_iql_args* a) {
    const char* who = "debug_iql_loss";
    CHK(iql_common(a, who));
    if (!a->out || !a->reward || !a->done || !a->action || !a->log_std || !a->ls_m || !a->ls_v || !a->d3) return fail(M3PC_EINVAL, "%s: null pointer", who);
    const IqlP p = iql_fill(a);
    iql_begin(a->picked);
    iql_launch_loss(p, (hipStream_t)a->stream);
    return iql_done(a->picked, who);
}

int m3pc_debug_iql_delta(const m3pc_debug_iql_args* a) {
    const char* who = "debug_iql_delta";
    CHK(iql_common(a, who));
    if (a->which != 1 && a->which != 2) return fail(M3PC_EINVAL, "%s: L %d is neither 1 nor 2", who, a->which);
    for (int t = 0; t < IQL_NETS; ++t) {
        if (!(a->which == 2 ? a->net[t].W3 : a->net[t].W2)) return fail(M3PC_EINVAL, "%s: null pointer", who);
        if (a->which == 2 && (a->net[t].out < 1 || a->net[t].out > IQL_OUTW)) return fail(M3PC_EINVAL, "%s: out %d outside [1, %d]", who, a->net[t].out, IQL_OUTW);
    }
    const float *in = a->which == 2 ? a->d3 : a->d2, *act = a->which == 2 ? a->h2 : a->h1, *o = a->which == 2 ? a->d2 : a->d1;
    if (!in || !act || !o) return fail(M3PC_EINVAL, "%s: null pointer", who);
    if (iql_off16(in) || iql_off16(act) || iql_off16(o)) return fail(M3PC_EINVAL, "%s: a delta or activation buffer off 16 bytes", who);
    const IqlP p = iql_fill(a);
    iql_begin(a->picked);
    iql_launch_delta(p, a->which, (hipStream_t)a->stream);
    return iql_done(a->picked, who);
}

int m3pc_debug_iql_grad(const m3pc_debug_iql_args* a) {
    const char* who = "debug_iql_grad";
    CHK(iql_common(a, who));
    for (int t = 0; t < 6; ++t)
        if (iql_net_null(a->net[t]) || (t < IQL_NETS && (iql_net_null(a->am[t]) || iql_net_null(a->av[t])))) return fail(M3PC_EINVAL, "%s: null pointer", who);
    if (!a->d1 || !a->d2 || !a->d3 || !a->h1 || !a->h2 || !a->om || !a->os) return fail(M3PC_EINVAL, "%s: null pointer", who);
    for (int t = 0; t < IQL_NETS; ++t) {
        CHK(iql_bad_in(a, a->net[t], who));
        if (a->net[t].out < 1 || a->net[t].out > IQL_OUTW) return fail(M3PC_EINVAL, "%s: out %d outside [1, %d]", who, a->net[t].out, IQL_OUTW);
        const int f = t == 0 ? 1 : t + 3;
        if (!(a->pass_next[f] ? a->next_state : a->state)) return fail(M3PC_EINVAL, "%s: null pointer", who);
    }
    const IqlP p = iql_fill(a);
    iql_begin(a->picked);
    iql_launch_grad(p, (hipStream_t)a->stream);
    return iql_done(a->picked, who);
}

int m3pc_debug_iql_eval_out(const float* out, int Bp, int rows, int twin, int width, float* dst, void* stream, int* picked) {
    if (picked) picked[0] = picked[1] = 0;
    if (!out || !dst) return fail(M3PC_EINVAL, "debug_iql_eval_out: null pointer");
    if (rows < 1 || rows > IQL_MAX_BATCH || Bp < rows || Bp % 32 || width < 1 || width > IQL_OUTW)
        return fail(M3PC_EINVAL, "debug_iql_eval_out: rows %d outside [1, %d], Bp %d below it or no multiple of 32, or width %d outside [1, %d]", rows, IQL_MAX_BATCH, Bp, width, IQL_OUTW);
    iql_begin(picked);
    iql_launch_eval_out(out, Bp, rows, twin ? 1 : 0, width, dst, (hipStream_t)stream);
    return iql_done(picked, "debug_iql_eval_out");
}

int m3pc_debug_iql_copy(float* dst, const float* src, long long n, void* stream, int* picked) {
    if (picked) picked[0] = picked[1] = 0;
    if (!dst || !src || n < 1) return fail(M3PC_EINVAL, "debug_iql_copy: null pointer or n %lld < 1", n);
    iql_begin(picked);
    iql_launch_copy(dst, src, n, (hipStream_t)stream);
    return iql_done(picked, "debug_iql_copy");
}

int m3pc_debug_iql_publish(const m3pc_debug_iql_publish_args* a) {
    const char* who = "debug_iql_publish";
    if (!a) return fail(M3PC_EINVAL, "%s: null arguments", who);
    if (a->picked) a->picked[0] = a->picked[1] = 0;
    if (a->H != 64 && a->H != 128 && a->H != 256) return fail(M3PC_EINVAL, "%s: hidden %d is none of 64, 128, 256", who, a->H);
    if (a->S < 1 || a->SA <= a->S || a->SA > 64) return fail(M3PC_EINVAL, "%s: S %d < 1, or S + A = %d not above it or above 64", who, a->S, a->SA);
    if (a->streams && a->SA > 32) return fail(M3PC_EINVAL, "%s: the operand streams cover S + A <= 32, not %d", who, a->SA);
    bool null = !a->om || !a->os || !a->c_om || !a->c_os;
    for (int i = 0; i < 2; ++i) {
        null = null || iql_net_null(a->q[i]) || !a->W1T[i] || !a->b1[i] || !a->W2T[i] || !a->b2[i] || !a->W3[i] || !a->b3[i];
        if (a->streams) null = null || !a->W1F[i] || !a->W2F[i];
    }
    if (null) return fail(M3PC_EINVAL, "%s: null pointer", who);
    for (int i = 0; i < 2; ++i)
        if (a->q[i].in != a->SA || a->q[i].out != 1) return fail(M3PC_EINVAL, "%s: q[%d] has in %d / out %d, a critic has %d / 1", who, i, a->q[i].in, a->q[i].out, a->SA);
    PublishP p;
    memset(&p, 0, sizeof(p));
    for (int i = 0; i < 2; ++i) {
        p.q[i] = iql_net(a->q[i]);
        p.W1T[i] = a->W1T[i], p.b1[i] = a->b1[i], p.W2T[i] = a->W2T[i], p.b2[i] = a->b2[i], p.W3[i] = a->W3[i], p.b3[i] = a->b3[i];
        p.W1F[i] = a->streams ? a->W1F[i] : nullptr, p.W2F[i] = a->streams ? a->W2F[i] : nullptr;
    }
    p.om = a->om, p.os = a->os, p.c_om = a->c_om, p.c_os = a->c_os;
    p.S = a->S, p.SA = a->SA, p.H = a->H;
    p.n_w1f = a->streams ? (long long)critic_w1f_floats(a->H) : 0;
    p.n_w2f = a->streams ? (long long)critic_w2f_floats(a->H) : 0;
    iql_begin(a->picked);
    iql_launch_publish(p, (hipStream_t)a->stream);
    return iql_done(a->picked, who);
}

// kv_fused_kernel alone (tests/test_block_fused_gpu.py): n candidates of Le rows each in Z (n*Le, 512) bf16; group g holds
// the kept[g] rows at offset off[g] of every candidate, embedded with We[g] (512, 512) bf16 + rowtab[g] (kept[g], 512);
// stream_buf: 2 * m3pc_debug_kv_stream_bytes() bytes; KV (n*Le, 1024) bf16
long long m3pc_debug_kv_stream_bytes(void) { return (long long)kv_stream_bytes(); }
int m3pc_debug_attention_bf16(const void* QKV, const void* QKVs, void* O, int batch, int n_own, int n_sh, int kernel, void* stream,
                              long long* stamps) {
    const int d = 512, L = n_own + n_sh;
    AttnP a;
    memset(&a, 0, sizeof(a));
    const char* q = (const char*)QKV;
    const char* qs = (const char*)QKVs;
    a.Q = q;
    a.q_bstride = (long long)n_own * 3 * d;
    a.ldq = 3 * d;
    a.Lq = n_own;
    a.K1 = q + (size_t)d * 2;
    a.V1 = q + (size_t)2 * d * 2;
    a.kv1_bstride = (long long)n_own * 3 * d;
    a.ldkv1 = 3 * d;
    a.L1 = n_own;
    if (n_sh > 0) {  // (run_block: own rows first in the slots, shared rows first in the output)
        a.orow1 = n_sh;
        a.Q2 = qs;
        a.ldq2 = 3 * d;
        a.Lq2 = n_sh;
        a.orow2 = 0;
        a.K2 = qs + (size_t)d * 2;
        a.V2 = qs + (size_t)2 * d * 2;
        a.ldkv2 = 3 * d;
        a.L2 = n_sh;
    }
    a.O = O;
    a.o_bstride = (long long)L * d;
    a.ldo = d;
    a.batch = batch;
    a.n_head = 4;
    a.hd = 128;
    a.scale = 1.0f / sqrtf(128.0f);
    a.stamps = stamps;
    a.no_pipe = kernel;  // (2, 3: timing variants of the pipelined kernel that compute nothing / load nothing)
    launch_attention(a, DT_BF16, (hipStream_t)stream);
    return check_launch("debug_attention_bf16");
}

int m3pc_debug_attention_dec_bf16(const void* Qtab, const void* QKVm, const void* KV, void* O, float* pre, int n, int nq, int Lm, int kernel,
                                  void* stream) {
    return m3pc_debug_attention_dec_le_bf16(Qtab, QKVm, KV, O, pre, n, nq, Lm, 49, kernel, stream);
}

int m3pc_debug_attention_dec_le_bf16(const void* Qtab, const void* QKVm, const void* KV, void* O, float* pre, int n, int nq, int Lm, int Le, int kernel,
                                     void* stream) {
    const int d = 512, nh = 4, hd = 128;
    hipStream_t st = (hipStream_t)stream;
    float* pre_m = pre;
    float* pre_l = pre + nh * nq;
    float* pre_O = pre + 2 * nh * nq;
    AttnP at;
    memset(&at, 0, sizeof(at));
    at.Q = Qtab;
    at.ldq = 3 * d;
    at.Lq = nq;
    at.K2 = (const char*)QKVm + (size_t)d * 2;
    at.V2 = (const char*)QKVm + (size_t)2 * d * 2;
    at.ldkv2 = 3 * d;
    at.L2 = Lm;
    at.n_head = nh;
    at.hd = hd;
    at.scale = 1.0f / sqrtf((float)hd);
    launch_attention_prestats(at, pre_m, pre_l, pre_O, st);
    at.K2 = at.V2 = nullptr;
    at.L2 = 0;
    at.q_bstride = 0;
    at.K1 = KV;
    at.V1 = (const char*)KV + (size_t)d * 2;
    at.kv1_bstride = (long long)Le * 2 * d;
    at.ldkv1 = 2 * d;
    at.L1 = Le;
    at.O = O;
    at.o_bstride = (long long)nq * d;
    at.ldo = d;
    at.batch = n;
    at.pre_m = pre_m;
    at.pre_l = pre_l;
    at.pre_O = pre_O;
    at.no_pipe = kernel;
    launch_attention(at, DT_BF16, st);
    return check_launch("debug_attention_dec_bf16");
}

int m3pc_debug_attention_mix_bf16(const void* Qown, const void* Qsh, const void* KV, const void* QKVm, void* O, int n, int Lq, int Lq2, int kernel,
                                  void* stream) {
    const int d = 512, Le = 49, Lm = 79;
    AttnP at;
    memset(&at, 0, sizeof(at));
    at.Q = Qown;
    at.q_bstride = (long long)Lq * d;
    at.ldq = d;
    at.Lq = Lq;
    at.orow1 = 0;
    at.Q2 = Qsh;
    at.ldq2 = 3 * d;
    at.Lq2 = Lq2;
    at.orow2 = Lq;
    at.K1 = KV;
    at.V1 = (const char*)KV + (size_t)d * 2;
    at.kv1_bstride = (long long)Le * 2 * d;
    at.ldkv1 = 2 * d;
    at.L1 = Le;
    at.K2 = (const char*)QKVm + (size_t)d * 2;
    at.V2 = (const char*)QKVm + (size_t)2 * d * 2;
    at.ldkv2 = 3 * d;
    at.L2 = Lm;
    at.O = O;
    at.o_bstride = (long long)(Lq + Lq2) * d;
    at.ldo = d;
    at.batch = n;
    at.n_head = 4;
    at.hd = 128;
    at.scale = 1.0f / sqrtf(128.0f);
    at.no_pipe = kernel;
    launch_attention(at, DT_BF16, (hipStream_t)stream);
    return check_launch("debug_attention_mix_bf16");
}

// any attention the library launches, on caller tensors (tests/test_attention_gpu.py): fills an AttnP and goes through
// launch_attention's dispatch; shapes the kernels do not cover are refused before anything is launched
int m3pc_debug_attention(int dtype, const void* Q, long long q_bstride, int ldq, int Lq, int orow1, const void* Q2, int ldq2, int Lq2,
                         int orow2, const void* K1, const void* V1, long long kv1_bstride, int ldkv1, int L1, const void* K2,
                         const void* V2, int ldkv2, int L2, const void* Kp, const void* Vp, int ldp, int Lp, float* pre, void* O,
                         long long o_bstride, int ldo, int batch, int n_head, int hd, float scale, int kernel, int* picked,
                         void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (picked) picked[0] = picked[1] = 0;
    if (dtype != DT_F32 && dtype != DT_BF16) return fail(M3PC_EINVAL, "debug_attention: dtype %d", dtype);
    if (hd != 32 && hd != 64 && hd != 128) return fail(M3PC_EINVAL, "debug_attention: head dim %d", hd);
    if (!Q || !K1 || !V1 || !O || batch < 1 || n_head < 1 || Lq < 1 || L1 < 1 || L2 < 0 || Lp < 0 || L1 + L2 > 256 || Lp > 256)
        return fail(M3PC_EINVAL, "debug_attention: shape");
    if (kernel != 0 && kernel != 1) return fail(M3PC_EINVAL, "debug_attention: kernel %d", kernel);
    const int w = n_head * hd, el = dtype == DT_BF16 ? 2 : 4, al = 16 / el;  // (16-byte row fragments)
    if (q_bstride < 0 || kv1_bstride < 0 || o_bstride < 0 || orow1 < 0 || (Q2 && orow2 < 0)) return fail(M3PC_EINVAL, "debug_attention: negative stride / row");
    if (ldq < w || ldkv1 < w || ldo < w || (K2 && ldkv2 < w) || (Q2 && ldq2 < w) || (Lp && ldp < w))
        return fail(M3PC_EINVAL, "debug_attention: leading dimension below n_head * hd");
    if ((ldq | ldkv1 | ldo | (K2 ? ldkv2 : 0) | (Q2 ? ldq2 : 0) | (Lp ? ldp : 0)) % al || (q_bstride | kv1_bstride | o_bstride) % al)
        return fail(M3PC_EINVAL, "debug_attention: strides must be multiples of %d elements", al);
    if (((uintptr_t)Q | (uintptr_t)K1 | (uintptr_t)V1 | (uintptr_t)O | (uintptr_t)Q2 | (uintptr_t)K2 | (uintptr_t)V2 | (uintptr_t)Kp |
         (uintptr_t)Vp | (uintptr_t)pre) & 15)
        return fail(M3PC_EINVAL, "debug_attention: pointers must be 16-byte aligned");
    if ((K2 == nullptr) != (V2 == nullptr) || (L2 > 0) != (K2 != nullptr) || (Lp > 0) != (Kp && Vp && pre) || (Q2 != nullptr) != (Lq2 > 0))
        return fail(M3PC_EINVAL, "debug_attention: optional segments need their pointers and a length");
    // the fp32 kernels know one query segment, no pre-reduced block and no output row offset
    if (dtype == DT_F32 && (Q2 || Lp || orow1)) return fail(M3PC_EINVAL, "debug_attention: Q2 / pre block / orow1 need bf16 rows");
    // the pre-reduced block is per query, shared by the batch, and indexed by the first segment's query slots
    if (Lp && (q_bstride != 0 || Q2)) return fail(M3PC_EINVAL, "debug_attention: a pre block needs batch-shared queries and no Q2");
    AttnP a;
    memset(&a, 0, sizeof(a));
    a.Q = Q;
    a.q_bstride = q_bstride;
    a.ldq = ldq;
    a.Lq = Lq;
    a.orow1 = orow1;
    a.Q2 = Q2;
    a.ldq2 = ldq2;
    a.Lq2 = Q2 ? Lq2 : 0;
    a.orow2 = orow2;
    a.n_head = n_head;
    a.hd = hd;
    a.scale = scale;
    float* pre_m = pre;
    float* pre_l = pre ? pre + (size_t)n_head * Lq : nullptr;
    float* pre_O = pre ? pre + (size_t)2 * n_head * Lq : nullptr;
    if (Lp) {  // (pre: n_head * Lq * (2 + hd) floats; pre_O 16-byte aligned as the pipelined kernels read it)
        if ((2 * n_head * Lq) % 4) return fail(M3PC_EINVAL, "debug_attention: 2 * n_head * Lq must be a multiple of 4");
        a.K2 = Kp;
        a.V2 = Vp;
        a.ldkv2 = ldp;
        a.L2 = Lp;
        launch_attention_prestats(a, pre_m, pre_l, pre_O, st);
        if (picked) picked[1] = 50;
        a.pre_m = pre_m;
        a.pre_l = pre_l;
        a.pre_O = pre_O;
    }
    a.K1 = K1;
    a.V1 = V1;
    a.kv1_bstride = kv1_bstride;
    a.ldkv1 = ldkv1;
    a.L1 = L1;
    a.K2 = K2;
    a.V2 = V2;
    a.ldkv2 = ldkv2;
    a.L2 = L2;
    a.O = O;
    a.o_bstride = o_bstride;
    a.ldo = ldo;
    a.batch = batch;
    a.no_pipe = kernel;
    g_attn_picked = 0;
    launch_attention(a, dtype, st);
    if (picked) picked[0] = g_attn_picked;
    return check_launch("debug_attention");
}

int m3pc_debug_kv_fused(const void* Z, int n, int Le, int kept0, int off0, int kept1, int off1, const void* We0, const void* We1,
                        const void* Wkv, void* stream_buf, const float* rowtab0, const float* rowtab1, const float* ln_g,
                        const float* ln_b, const float* bkv, void* KV, void* stream, long long* stamps) {
    hipStream_t st = (hipStream_t)stream;
    bf16_t* s0 = (bf16_t*)stream_buf;
    bf16_t* s1 = (bf16_t*)((char*)stream_buf + kv_stream_bytes());
    launch_pack_kv_stream((const bf16_t*)We0, (const bf16_t*)Wkv, s0, st);
    if (kept1) launch_pack_kv_stream((const bf16_t*)We1, (const bf16_t*)Wkv, s1, st);
    KvFusedP p;
    memset(&p, 0, sizeof(p));
    p.Z = (const bf16_t*)Z;
    p.ldz = 512;
    p.M[0] = n * kept0;
    p.map[0] = RowMap{kept0, Le, off0};
    p.rowtab[0] = rowtab0;
    p.rt_mod[0] = kept0;
    p.wstream[0] = s0;
    p.M[1] = n * kept1;
    p.map[1] = RowMap{kept1 ? kept1 : 1, Le, off1};
    p.rowtab[1] = rowtab1;
    p.rt_mod[1] = kept1 ? kept1 : 1;
    p.wstream[1] = s1;
    p.ln_g = ln_g;
    p.ln_b = ln_b;
    p.bkv = bkv;
    p.KV = (bf16_t*)KV;
    p.ldkv = 1024;
    p.kv_bytes = (unsigned)((size_t)n * Le * 1024 * 2);
    p.stamps = stamps;
    if (!launch_kv_fused(p, st)) return fail(M3PC_EINVAL, "kv_fused: arguments not covered");
    return check_launch("debug_kv_fused");
}

int m3pc_debug_kv_fused_ex(const m3pc_debug_kv_args* a) {
    if (!a) return fail(M3PC_EINVAL, "debug_kv: null arguments");
    if (!a->Z || !a->Wkv || !a->stream_buf || !a->ln_g || !a->ln_b || !a->bkv || !a->KV) return fail(M3PC_EINVAL, "debug_kv: a required pointer is null");
    if (a->kv_bytes <= 0 || a->kv_bytes > 0xffffffffll) return fail(M3PC_EINVAL, "debug_kv: kv_bytes");
    hipStream_t st = (hipStream_t)a->stream;
    KvFusedP p;
    memset(&p, 0, sizeof(p));
    p.Z = (const bf16_t*)a->Z;
    p.ldz = a->ldz;
    for (int g = 0; g < 2; ++g) {
        p.M[g] = a->M[g];
        if (a->map[g][0] < 0 || a->map[g][2] < 0 || (a->map[g][0] > 0 && a->map[g][1] < a->map[g][0])) return fail(M3PC_EINVAL, "debug_kv: row map of group %d", g);
        p.map[g] = RowMap{a->map[g][0], a->map[g][1], a->map[g][2]};
        p.rowtab[g] = a->rowtab[g];
        p.rt_mod[g] = a->rt_mod[g];
        p.wstream[g] = (const bf16_t*)((char*)a->stream_buf + g * kv_stream_bytes());
        if (a->M[g] > 0 && !a->We[g]) return fail(M3PC_EINVAL, "debug_kv: group %d without its embedding weights", g);
    }
    p.ln_g = a->ln_g;
    p.ln_b = a->ln_b;
    p.bkv = a->bkv;
    p.KV = (bf16_t*)a->KV;
    p.ldkv = a->ldkv;
    p.kv_bytes = (unsigned)a->kv_bytes;
    for (int g = 0; g < 2; ++g)
        if (a->M[g] > 0) launch_pack_kv_stream((const bf16_t*)a->We[g], (const bf16_t*)a->Wkv, (bf16_t*)p.wstream[g], st);
    if (!launch_kv_fused(p, st)) return fail(M3PC_EINVAL, "kv_fused: arguments not covered");
    return check_launch("debug_kv_fused_ex");
}

// which XCD (and CU) every workgroup of a launch on `stream` lands on: out[2 i] = XCC_ID, out[2 i + 1] = HW_ID register
// (tools/xcd_probe.py: maps the bits of a hipExtStreamCreateWithCUMask mask to XCDs)
__global__ void xcc_probe_kernel(int* out) {
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = (int)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11));   // HW_REG_XCC_ID[3:0]
        out[2 * blockIdx.x + 1] = (int)__builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11)); // HW_REG_HW_ID
    }
    // (long enough that the workgroups of the launch spread over everything the stream may use)
    const long long t0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < 1024; ++i) {
        if (__builtin_amdgcn_s_memrealtime() - t0 >= 300) break;
        __builtin_amdgcn_s_sleep(16);
    }
}
int m3pc_debug_xcc_probe(int* out, int n_blocks, void* stream) {
    hipLaunchKernelGGL(xcc_probe_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, out);
    return check_launch("xcc_probe");
}

int m3pc_debug_clock_big(long long* out4) {
    HIPCHK(hipDeviceSynchronize());
    read_big_probe(out4);
    return 0;
}


// ---- csrc/mtm_opt.hip: mo_adamw_kernel alone on caller arrays and a caller segment table, through the launcher the trainer uses
// (tests/test_mtm_opt_kernel_edges_gpu.py).  The tables are uploaded here and freed when the launch has finished: the call waits.
int m3pc_debug_mtm_adamw(const m3pc_debug_mtm_adamw_args* a) {
    if (!a) return fail(M3PC_EINVAL, "debug_mtm_adamw: null arguments");
    if (a->n < 1 || a->n > 4096) return fail(M3PC_EINVAL, "debug_mtm_adamw: n %d outside [1, 4096]", a->n);
    if (!a->p || !a->g_off || !a->s_off || !a->numel || !a->decay || !a->active || !a->grad || !a->exp_avg || !a->exp_avg_sq || !a->steps_in ||
        !a->steps_out)
        return fail(M3PC_EINVAL, "debug_mtm_adamw: null pointer");
    if (a->steps_in == a->steps_out) return fail(M3PC_EINVAL, "debug_mtm_adamw: steps_in and steps_out are one array");
    std::vector<MoSeg> seg((size_t)a->n);
    for (int i = 0; i < a->n; ++i) {
        if (!a->p[i]) return fail(M3PC_EINVAL, "debug_mtm_adamw: p[%d] is null", i);
        if (a->numel[i] < 1 || a->numel[i] > (1ll << 30)) return fail(M3PC_EINVAL, "debug_mtm_adamw: numel[%d] = %lld outside [1, 2^30]", i, a->numel[i]);
        if (a->g_off[i] < 0 || a->g_off[i] + a->numel[i] > a->grad_floats)
            return fail(M3PC_EINVAL, "debug_mtm_adamw: g_off[%d] + numel leaves the %lld floats of grad", i, a->grad_floats);
        if (a->s_off[i] < 0 || a->s_off[i] + a->numel[i] > a->state_floats)
            return fail(M3PC_EINVAL, "debug_mtm_adamw: s_off[%d] + numel leaves the %lld floats of the moments", i, a->state_floats);
        seg[i].p = a->p[i];
        seg[i].b = a->b ? (bf16_t*)a->b[i] : nullptr;
        seg[i].g_off = a->g_off[i];
        seg[i].s_off = a->s_off[i];
        seg[i].numel = a->numel[i];
        seg[i].decay = a->decay[i] ? 1 : 0;
        seg[i].head_key = a->active[i] ? -1 : 0;  // (with loss_keys 0 below: key 0 is outside)
    }
    std::vector<int2> blk;
    mo_block_table(a->numel, a->n, blk);
    MoSeg* d_seg = nullptr;
    int2* d_blk = nullptr;
    hipStream_t st = (hipStream_t)a->stream;
    CHK(dmalloc((char**)&d_seg, seg.size() * sizeof(MoSeg)));
    if (int rc = dmalloc((char**)&d_blk, blk.size() * sizeof(int2))) {
        (void)hipFree(d_seg);
        return rc;
    }
    hipError_t e = hipMemcpy(d_seg, seg.data(), seg.size() * sizeof(MoSeg), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_blk, blk.data(), blk.size() * sizeof(int2), hipMemcpyHostToDevice);
    int rc = 0;
    if (e == hipSuccess) {
        MoAdamP p;
        memset(&p, 0, sizeof(p));
        p.seg = d_seg;
        p.blk = d_blk;
        p.n_blocks = (int)blk.size();
        p.grad = a->grad;
        p.exp_avg = a->exp_avg;
        p.exp_avg_sq = a->exp_avg_sq;
        p.steps_in = a->steps_in;
        p.steps_out = a->steps_out;
        p.loss_keys = 0;
        p.write_bf16 = a->write_bf16;
        p.lr_t = a->lr_t;
        p.wd = a->weight_decay;
        p.beta1 = a->beta1;
        p.beta2 = a->beta2;
        p.eps = a->eps;
        p.omb1 = (float)(1.0 - a->beta1);
        p.b2 = (float)a->beta2;
        p.omb2 = (float)(1.0 - a->beta2);
        mo_launch_adamw(p, st);
        rc = check_launch("debug_mtm_adamw");
        e = hipStreamSynchronize(st);
    }
    (void)hipFree(d_seg);
    (void)hipFree(d_blk);
    if (e != hipSuccess) return fail(M3PC_EHIP, "debug_mtm_adamw: %s", hipGetErrorString(e));
    if (a->n_blocks) *a->n_blocks = (int)blk.size();
    return rc;
}


}  // extern "C"
#pragma GCC visibility pop
