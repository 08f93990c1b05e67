/*
 * m3pc_hip_debug.h -- kernel-level test and bench hooks of the LAB build (libm3pc_hip_lab.so,
 * `python -m m3pc_amd.build --lab`, compiled with -DM3PC_LAB).  The product library libm3pc_hip.so
 * exports none of these and reads no environment variable; the lab build additionally honours the
 * A/B switches M3PC_NO_* / M3PC_GEMM_VARIANT / M3PC_TWO_STREAM / ... listed in DESIGN.md section 7.
 * Users: tests/test_gemm_kernels_gpu.py, tests/test_gemm_edges_gpu.py, tests/test_bf16x3_gpu.py, tests/test_attention_gpu.py,
 * tests/test_block_fused_gpu.py, tests/test_block_edges_gpu.py, tests/test_block_ref_cpu.py, tests/test_lockstep_kernels_gpu.py,
 * tests/test_block_shared_xb_gpu.py, tests/test_block_shared_xb_cpu.py, tests/test_embed_shared_xb_gpu.py,
 * tests/test_elementwise_edges_gpu.py, tests/test_elementwise_ref_cpu.py, tests/test_select_edges_gpu.py, tests/test_select_ref_cpu.py,
 * tools/*.py.
 */
#ifndef M3PC_HIP_DEBUG_H
#define M3PC_HIP_DEBUG_H

#ifdef __cplusplus
extern "C" {
#endif

/* one GEMM launch of the library's dispatch on caller tensors (dtype 0 fp32 / 1 bf16 operands / 2 split-bf16: A and W fp32,
 * W split into hi / lo bf16 copies inside the call, gemm_x3.hip; variant 1 there: no split-K workspace):
 * C = epilogue(A (M,K) W (N,K)^T + bias [gelu] [+ res]); variant selects a kernel configuration (0: dispatch) */
int m3pc_debug_gemm(int dtype, const void* A, const void* Wt, const float* bias, const float* res, void* C, int M, int N,
                    int K, int gelu, int f32out, int variant, void* stream);
/* one GEMM of the library on caller tensors with everything a production call can pass (GemmP, csrc/kernels.h), through
 * launch_gemm's / launch_gemm_x3's dispatch:
 *     C[cmap(r)] = [res[cmap(r)] +] [gelu](A[amap(r)] (K) . W (N, K)^T + bias + rowtab[(r % rt_mod) rt_ld ..])      r < M
 * a row map {rpg, gstride, off} sends logical row r to physical row (r / rpg) gstride + r % rpg + off (rpg 0: identity); cmap
 * applies to C and res alike, and res may be C itself.  dtype 0: fp32 operands, 1: bf16 operands, 2: split-bf16 (A and W fp32, W is
 * split into its hi / lo bf16 copies inside the call).  f32out: C is fp32 (always for dtype 0), else bf16.  ws / ws_bytes: the
 * split-K slab workspace (null: K is never split, and the few-row fp32 kernel of gemm_f32_direct.hip is not used).  a_padded: 127
 * readable rows follow A's last row.  ln_g / ln_b / ln_out: the LayerNorm that consumes C (N columns, contiguous rows); bit 2 of
 * picked[3] says whether the launch applied it -- when not, ln_out is untouched and the caller runs the LayerNorm itself.
 * a_ln_g / a_ln_b: A is LayerNorm(A rows) (K columns), normalised on the operand load.  variant: 0 = dispatch; bf16 operands: 2 /
 * 26 / 37 / 43 / 44 force launch_tile<128, 128, 2, 2, 64> (the double buffer on 64-byte LDS rows) / the ring without peeling / gemm_big / gemm_line 128 / gemm_line 256;
 * fp32 operands: 2 = never the few-row kernel.
 * Refused with M3PC_EINVAL before anything is launched (the register-staged kernel every shape can fall back to sets the shape
 * rules): N % 64 (N % 32 where the few-row fp32 kernel, id 5 / 6, takes the problem), K * sizeof(operand) % 128 (x3: K % 32), a pointer not on 16 bytes, a leading dimension below its row length or
 * whose rows leave 16 bytes, rowtab with rt_mod < 1, a row map that is neither rpg == 0 nor rpg >= 1 with gstride >= rpg (off >= 0),
 * bf16 output of fp32 operands, an epilogue no launcher of the dispatch instantiates (id 0), ln_out without fp32 C / ln_g / ln_b,
 * a_ln_* on a problem gemm_f32_direct_covers rejects (or without ws, or with
 * variant 2: the fold would be dropped silently), any other variant, a forced variant whose launcher does not take the problem, and
 * variant 44 with a_padded where the ragged 256-row tile would read more than the 127 rows a_padded vouches for.
 * picked (4 ints, optional): [0] kernel id, [1] split count S (1: K not split), [2] the peel row (0: off), [3] bits: 1 persistent
 * form (gemm_line.hip: look-alike tiles, tile origin in the scalar offset), 2 the split-K reduce applied the LayerNorm, 4 grouped.
 * GEMM kernel ids (tests/test_gemm_edges_gpu.py reaches every id of this list):
 *   gemm.hip:            1 gemm_kernel<float, 64, 64>;  2 gemm_kernel<float, 128, 128>;  3 gemm_kernel<bf16, 64, 64>;
 *                        4 gemm_kernel<bf16, 128, 128>   (S > 1: followed by splitk_reduce_kernel / splitk_reduce_ln_kernel)
 *   gemm_f32_direct.hip: 5 gemm_f32_direct_kernel<1, 16>;  6 gemm_f32_direct_group_kernel
 *   gemm_glds.hip:       7 gemm_glds_ring3_kernel;  8 gemm_glds_kernel via launch_tile<128, 128, 2, 2, 64> (variant 2)
 *   gemm_big.hip:        9 gemm_big_kernel
 *   gemm_line.hip:       10 gemm_line_kernel<128>;  11 gemm_line_kernel<256>
 *   gemm_x3.hip:         12 gemm_x3_kernel<64, 64>;  13 gemm_x3_kernel<128, 128>
 *   not listed, not reachable through this hook: the lab-only experimental tilings gemm_ring.hip (variants 7-19), gemm_persist.hip (9),
 *   gemm_rs.hip (36), gemm_glds_ring3w_kernel (31), launch_tile's 128-byte-row instance (3, 20-24, 27) and the timing variants of gemm_big.hip / gemm_line.hip (38-42, 45, 46) */
typedef struct m3pc_debug_gemm_args {
    int dtype;
    const void* A;
    int lda;
    int amap[3]; /* rpg, gstride, off */
    const void* W;
    int ldw;
    int M, N, K;
    const float* bias; /* optional */
    const float* rowtab; /* optional */
    int rt_mod, rt_ld;
    int gelu;
    const float* res; /* optional; may be C */
    int ldr;
    void* C;
    int f32out;
    int ldc;
    int cmap[3];
    float* ws; /* optional */
    long long ws_bytes;
    int a_padded;
    const float* ln_g;
    const float* ln_b;
    float* ln_out;
    const float* a_ln_g;
    const float* a_ln_b;
    int variant;
    void* stream;
    int* picked; /* optional: 4 ints */
} m3pc_debug_gemm_args;
int m3pc_debug_gemm_ex(const m3pc_debug_gemm_args* a);
/* the same checks and the same walk of the dispatch without launching anything (no GPU needed): the refusals, and `picked` as
 * m3pc_debug_gemm_ex would report it */
int m3pc_debug_gemm_plan(const m3pc_debug_gemm_args* a);
/* n <= 4 fp32 problems in ONE launch (launch_gemm_f32_direct_group, kernel id 6): every problem must be one the few-row kernel
 * covers, with ws set; stream and picked are those of a[0] */
int m3pc_debug_gemm_group(const m3pc_debug_gemm_args* a, int n);
/* clock probes of the last probed GEMM workgroup: {shader clocks, 100-MHz ticks} / gemm_big phase timers */
int m3pc_debug_clock(long long* out2);
int m3pc_debug_clock_big(long long* out4);
/* the top-k kernels on their own, through launch_topk's dispatch: indices of the k largest of v (n), descending, ties to the lower
 * index.  Refused with M3PC_EINVAL before anything is launched: a null v / idx_out, n outside [1, 16384], k outside [1, n]. */
int m3pc_debug_topk(const float* v, int n, int k, int* idx_out, void* stream);
/* ---- the selection and certificate kernels of csrc/select.hip, one by one (tests/test_select_edges_gpu.py reaches every id of this
 * list; tests/select_ref.py holds the references).  Every launcher of select.hip records the id of the kernel it launches:
 * Selection kernel ids:
 *   1 select_kernel;  2 select_batch_kernel;  3 topk_kernel;  4 topk_batch_kernel;  5 topk_select_kernel;
 *   6 topk_select_batch_kernel;  7 topk_rank_blocks_kernel;  8 topk_rank_blocks_batch_kernel;  9 topk_rank_blocks2_kernel;
 *   10 topk_rank_blocks2_dyn_kernel;  11 topk_rank_batch_kernel;  12 topk_rank_kernel;  13 window_stats_kernel;
 *   14 rescore_merge_kernel;  15 merge_select_kernel;  16 merge_select_batch_kernel;  17 deviation_stats_kernel;
 *   18 eval_bound_kernel;  19 eval_bound_batch_kernel;  20 scatter_kernel;  21 gather_listed_kernel;  22 variates_kernel;
 *   23 variates_batch_kernel
 * (end of the selection kernel ids)
 * Reached through: m3pc_select (1), m3pc_debug_select_batch (2), m3pc_debug_topk_ex (3 .. 10, 12), m3pc_debug_topk_race_batch (11),
 * m3pc_debug_window_stats (13), m3pc_rescore_merge / m3pc_rescore_merge_race (14), m3pc_merge_race_select (15),
 * m3pc_debug_merge_select_batch (16), m3pc_debug_calibrate_stats (17), m3pc_eval_bound (18), m3pc_debug_eval_bound_batch (19),
 * m3pc_debug_scatter (20), m3pc_debug_gather_listed (21), m3pc_draw_variates (22), m3pc_debug_variates_batch (23).
 * The id of the select.hip kernel the calling thread launched last (0: none), for the entry points without a `picked` argument: */
int m3pc_debug_select_picked(void);
/* the set of ids launched by the calling thread since the set was last cleared, bit `id` for kernel id (m3pc_topk_window launches
 * two kernels); clear != 0 empties the set and the last id */
unsigned int m3pc_debug_select_picked_set(int clear);
/* one top-k of n_windows rows of v (n_windows, n): the ranks r < k, descending value, ties to the lower index, -0.0 equal to +0.0;
 * the element of rank r goes to out[r * out_stride] (window w: out + w k).
 *   variant 0, no expo: launch_topk (one window) or launch_topk_batch.  out_stride 1.
 *   variants 1 .. 4: topk_rank_kernel, topk_rank_blocks_kernel, topk_select_kernel, topk_kernel forced, one window, where that kernel
 *     is legal: n <= 2048;  n <= 2048;  k <= 64 and n <= 16384;  n <= 16384.  With expo (variant 3 only) the value ranked is the race
 *     key tau v - log expo; out_stride -1 (variant 3 only) writes rank r to out[-r].
 *   variant 0 with expo: launch_topk_race, one window.  `out` is the list at position rmax: out[-1 - i] = the i-th best by race key,
 *     i < k <= 64 (out_stride must be -1), out[i] = the i-th best by value, i < kk <= min(1024, n); scores_out (optional, same layout)
 *     = v[winner].
 *   variant 5: the same call through launch_topk_race's branch for a device that refuses the LDS opt-in -- launch_topk for the
 *     values, topk_select_kernel for the race keys -- taken without asking the device to refuse anything.  No scores_out.
 *   variant 6: launch_topk_batch for every n_windows, one window included (variant 0 sends one window to launch_topk).
 * Refused with M3PC_EINVAL before anything is launched: a null v / out, n outside [1, 16384], k outside [1, n], n_windows outside
 * [1, 65535], an out_stride other than 1 / -1, a variant outside [0, 6], a forced kernel outside its shapes (above) or with several
 * windows, k > 64 on the selection kernel, expo / out_stride -1 / scores_out / kk where the variant has no use for it, kk outside
 * [1, min(1024, n)] where it has.
 * picked (2 ints, optional): [0] the kernel launched last, [1] the kernel that ranked the values when two lists were made (variant 0
 * with expo: the one kernel; variant 5: launch_topk's), else 0. */
typedef struct m3pc_debug_topk_args {
    const float* v;
    const float* expo; /* optional */
    float tau;
    int n_windows, n, k;
    int* out;
    int out_stride;
    float* scores_out; /* optional */
    int kk;            /* with expo and variant 0 / 5, else 0 */
    int variant;
    int* picked; /* optional: 2 ints */
    void* stream;
} m3pc_debug_topk_args;
int m3pc_debug_topk_ex(const m3pc_debug_topk_args* a);
/* window_stats_kernel through launch_window_stats: idx = the kk best entries of v (n_total), best first; stats (device, 4 floats) =
 * {n = min(clamp(cnt, kmin, kmax), kk), v[idx[0]] - v[idx[n]] (infinity when n == kk), v[idx[0]], cnt = #{i: v[i] >= v[idx[0]] -
 * window}}; host_stats (optional): 5 floats a kernel can store to, closed by seq in slot 4; top_scores (optional): top_scores[i] =
 * v[idx[i]] for i in [-rr, kk) -- rr race entries in front of idx.  Refused: a null v / idx / stats, n_total outside [1, 16384], kk
 * outside [1, n_total], kmin outside [1, kmax], rr outside [0, 64], a window that is not >= 0. */
int m3pc_debug_window_stats(const float* v, int n_total, const int* idx, int kk, int kmin, int kmax, float window, float* stats,
                            float* host_stats, float seq, float* top_scores, int rr, void* stream);
/* scatter_kernel through launch_scatter: dst[index[i]] = src[i], index_copy[i] = index[i] (optional), i < n.  Refused: a null src /
 * index / dst, n < 1.  The caller keeps the entries of index (device memory) inside dst. */
int m3pc_debug_scatter(const float* src, const int* index, int n, float* dst, int* index_copy, void* stream);
/* variates_batch_kernel through launch_variates_batch (the normals of m3pc_refine_plans): out (n_windows, g1 - g0), window w = the
 * elements [g0, g1) of the standard-normal array of (seed, steps[w]) -- m3pc_draw_variates' eps for that step, flat.  steps is a HOST
 * array.  Refused: a null steps / out, n_windows outside [1, 65535], g0 < 0, g1 <= g0, g1 > 2^33. */
int m3pc_debug_variates_batch(unsigned long long seed, const unsigned long long* steps, int n_windows, long long g0, long long g1,
                              float* out, void* stream);
/* the statistics kernel of m3pc_calibrate_delta on caller vectors: stats (device, 8 floats) = {lower median c of scores_low - f32,
 * max |scores_low - f32 - c|, max |f32|, 0 ...}; *delta_out (host) = max(factor * stats[1], 1e-6 * stats[2], 1e-30).  n <= 16384.
 * Synchronises the stream. */
int m3pc_debug_calibrate_stats(const float* scores_low, const float* f32, int n, float factor, float* stats, float* delta_out,
                               void* stream);
/* ---- the tail of a lock-step batch of certified plan steps (csrc/select.hip), each kernel alone on caller device arrays.  Every
 * kernel takes its window from the grid and runs the device functions of the one-window kernels: window w's results are those of
 * the one-window entry points on row w, bit for bit (tests/test_lockstep_kernels_gpu.py).
 * The lists of n_windows windows in one launch: scores / expo (n_windows, n_total); per window the layout of m3pc_topk_race_window,
 * list[w][rmax + i] = the i-th best by score (i < min(kmax + 1, n_total)), list[w][rmax - 1 - i] = the i-th best by race key (i < rmax),
 * rows of rmax + kmax + 1 entries, list_scores (optional) in the same layout; rmax 0: m3pc_topk_window's list (expo unused).
 * Descending, ties to the lower index.  n_total <= 16384, kmax <= 1023, rmax <= min(64, n_total). */
int m3pc_debug_topk_race_batch(const float* scores, const float* expo, float temperature, int n_windows, int n_total, int kmax, int kmin,
                               int rmax, int* list, float* list_scores, void* stream);
/* what the lists name, for one m3pc_score_actions call: cand[w m + i] = sample_actions[w][list[w][lo + i]] (rows of row_floats = h A
 * floats; sample_actions (n_windows, n_total, row_floats), list rows of list_stride entries) and window_index[w m + i] = w (int32,
 * optional), m = hi - lo, window-major.  An entry outside [0, n_total) leaves its row of cand untouched. */
int m3pc_debug_gather_listed(const float* sample_actions, const int* list, int n_windows, int n_total, int row_floats, int list_stride,
                             int lo, int hi, float* cand, int* window_index, void* stream);
/* merge + certificate statistics + select of n_windows windows in one launch: m3pc_merge_race_select per window (race != 0), or
 * m3pc_rescore_merge followed by m3pc_select (race == 0: r[w] = 0, four statistics, expo optional and used by the select alone);
 * select == 0: the merge alone.  Window w uses r[w] race and n[w] score entries, the slice [rmax - r[w], rmax + n[w]) of its list and
 * list_scores (rows of list_stride), their fp32 re-scores list_rescored[w f_stride + j - f_lo] for list position j (f_stride =
 * list_stride and f_lo = 0: the list's layout), and delta[w]; r / n / delta are HOST arrays.  scores / expo / merged / p
 * (n_windows, n_total); stats (n_windows, 8) device; host_stats (optional): n_windows blocks of 8 floats a kernel can store to, each
 * closed by seq in slot 4, written last at system scope; a0: window w's first actions at a0 + w a0_window_stride, candidate j's at
 * + j a0_stride (A floats); eval_action / sample_action (n_windows, A), argmax / sample_idx (n_windows,) int32, each optional. */
typedef struct m3pc_debug_tail_args {
    const float* scores;
    const float* expo;
    int race, select;
    float temperature;
    int n_windows, n_total;
    const int* list;
    const float* list_scores;
    const float* list_rescored;
    int rmax, list_stride, f_stride, f_lo;
    const int* r;       /* host */
    const int* n;       /* host */
    const float* delta; /* host */
    float* merged;
    float* stats;
    float* host_stats;
    float seq;
    const float* a0;
    long long a0_window_stride, a0_stride;
    int A;
    float* p;
    float* eval_action;
    int* argmax;
    int* sample_idx;
    float* sample_action;
    void* stream;
} m3pc_debug_tail_args;
int m3pc_debug_merge_select_batch(const m3pc_debug_tail_args* a);
/* m3pc_select of n_windows windows in one launch (select_batch_kernel, the fp32 form of m3pc_plan_steps_certified): scores / expo / p
 * (n_windows, n_total); a0 as above; eval_action / sample_action (n_windows, A), argmax / sample_idx (n_windows,) int32; p, the four
 * outputs and expo optional as in m3pc_select.  Window w's results are m3pc_select's on row w, bit for bit.  n_total <= 16384. */
int m3pc_debug_select_batch(const float* scores, const float* a0, long long a0_window_stride, long long a0_stride, int n_windows,
                            int n_total, int A, float temperature, const float* expo, float* p, float* eval_action, int* argmax,
                            int* sample_idx, float* sample_action, void* stream);
/* m3pc_eval_bound of n_windows windows in one launch (eval_bound_batch_kernel, behind the batched merge of
 * m3pc_plan_steps_certified_eval): window w reads row w of merged (n_windows, n_total), the slice of its list row (rows of list_stride
 * int32) from rmax - r[w] on -- r[w] re-scored race entries, then n_listed score entries of which the first n[w] are re-scored --,
 * its first actions at a0 + w a0_window_stride (candidate j's at + j a0_stride, A floats) and delta[w]; r / n / delta are HOST arrays;
 * n_listed, temperature and eval_tol are shared.  stats (n_windows, 8) device; host_stats (optional): n_windows blocks of 8 floats a
 * kernel can store to, each closed by seq in slot 4, written last at system scope.  Window w's eight floats are m3pc_eval_bound's on
 * that window's rows, bit for bit (tests/test_eval_bound_batch_gpu.py).  rmax + n_listed <= min(1024, list_stride). */
typedef struct m3pc_debug_eval_batch_args {
    const float* merged;
    int n_windows, n_total;
    const int* list;
    int rmax, list_stride, n_listed;
    const int* r;       /* host */
    const int* n;       /* host */
    const float* delta; /* host */
    const float* a0;
    long long a0_window_stride, a0_stride;
    int A;
    float temperature, eval_tol;
    float* stats;
    float* host_stats;
    float seq;
    void* stream;
} m3pc_debug_eval_batch_args;
int m3pc_debug_eval_bound_batch(const m3pc_debug_eval_batch_args* a);
/* the fused layer tail (block_fused.hip) on caller tensors; see csrc/m3pc_debug.hip for the argument layout */
long long m3pc_debug_block_stream_bytes(void);
int m3pc_debug_block_fused(const void* O, int M, const float* res, const float* rowtab, int rt_mod, const void* Wo, const void* W1,
                           const void* W2, void* stream_buf, int pack, const float* bo, const float* b1, const float* b2,
                           const float* ln2_g, const float* ln2_b, const float* lnA_g, const float* lnA_b, const float* lnB_g0,
                           const float* lnB_b0, const float* lnB_g1, const float* lnB_b1, int out_mod, int out_grp, float* Xout,
                           void* Hout, int variant, void* stream, long long* stamps);
/* the same with the next layer's Q|K|V projection behind the tail: QKV (M, 1536) bf16 = LN_A(X'') Wqkv^T + bqkv */
int m3pc_debug_block_fused_qkv(const void* O, int M, const float* res, const void* Wo, const void* W1, const void* W2, const void* Wqkv,
                               void* stream_buf, const float* bo, const float* b1, const float* b2, const float* ln2_g,
                               const float* ln2_b, const float* lnA_g, const float* lnA_b, const float* bqkv, float* Xout, void* QKV,
                               void* stream, long long* stamps, int x_bf16);  /* x_bf16: res / Xout are (M, 512) bf16 rows (round 6);
                                                                                 m3pc_debug_block_fused: bit 16 of `variant` */
/* the decoder form with the two scalar output heads inside the tail (see csrc/m3pc_debug.hip for the argument layout) */
int m3pc_debug_block_fused_heads(const void* O, int M, const float* rowtab, int rt_mod, const void* Wo, const void* W1, const void* W2,
                                 const void* Wh, void* stream_buf, const float* bo, const float* b1, const float* b2, const float* ln2_g,
                                 const float* ln2_b, const float* lnA_g, const float* lnA_b, const float* lnB_g0, const float* lnB_b0,
                                 const float* lnB_g1, const float* lnB_b1, int out_mod, int out_grp, const float* hb1, const float* hw2,
                                 const float* hb2, const float* hmean, const float* hstd, float* out0, float* out1, void* stream,
                                 long long* stamps);
/* one launch of the fused layer tail with everything a production call can pass (BlockP, csrc/kernels.h), through
 * launch_block_fused's checks and dispatch; the weight stream is packed inside the call (Wo (512, 512), W1 (2048, 512), W2 (512, 2048),
 * optional Wqkv (1536, 512) or Wh (2, 512, 512): bf16, torch Linear layout; stream_buf: m3pc_debug_block_stream_bytes() bytes on 1 KiB).
 *     X'  = residual(r) + bo + O[r] Wo^T          residual(r): res[r] (ldr; bf16 rows when x_bf16); with res_L > 0 the rows come in
 *                                                 sequences of res_L and row j < res_nshared of every sequence is read from sequence 0
 *                                                 (x_bf16: res is the compact block of m3pc_debug_block_res_row, and Xout is not res);
 *                                                 with rowtab: rowtab[w], w = r % rt_mod, and for w < res_nu the row of its own stored
 *                                                 behind the table, rowtab[rt_mod + (r / rt_mod) res_nu + w]
 *     X'' = X' + b2 + gelu(LN2(X') W1^T + b1) W2^T     -> Xout (ldx; fp32, bf16 when x_bf16; may be res)
 *     Hout[orow(r)] = bf16(LN_B[s]?(LN_A(X'')))   (ldh) out_mod > 0: s = (r % out_mod) / out_grp, orow = s (M / out_mod) out_grp +
 *                                                 (r / out_mod) out_grp + r % out_grp; out_mod 0 with lnB_g[0]: LN_B[0] for every row
 *     QKVout[r] = bf16(bf16(LN_A(X'')) Wqkv^T + bqkv)  (ldq >= 1536; qkv_bytes: the size of the buffer, stores behind it are dropped)
 *     head_out[s][i] = detok(hw2_s . gelu(Wh_s bf16(LN_B[s](LN_A(X''))) + hb1_s) + hb2_s) for the i-th row of group s (hb1 / hw2
 *                                                 (2, 512), hb2 / hmean / hstd (2) floats; hmean null: no de-tokenisation)
 * split: four workgroups per tile write fp32 partials to the block_split_n() = 4 slabs of M rows behind Xout (ldx 512), and
 * block_split_reduce_kernel follows: red_Xout (red_ldx) = their sum, red_Hout (red_ldh) = bf16(LN_B?(LN_A(sum))) with red_lnA_* /
 * red_lnB_* / red_out_mod / red_out_grp as above.
 * Refused with M3PC_EINVAL before anything is launched: whatever block_fused_accepts refuses (tests/test_block_ref_cpu.py lists the
 * refusals), a missing weight the form needs, and reduce arguments block_split_reduce_kernel does not cover (red_ldx % 4, red_ldh % 8,
 * red_Hout without red_lnA_*, red_out_mod != 2 red_out_grp or not dividing M, neither output).
 * picked (1 int, optional): the instance launched.  Block forms (tests/test_block_edges_gpu.py reaches every value of this list):
 *   0 block_fused_kernel<0, 0>;  1 block_fused_kernel<0, 1> (next Q|K|V);  2 block_fused_kernel<0, 2> (heads);
 *   3 block_fused_kernel<0, 3> + block_split_reduce_kernel;  16 block_fused_kernel<0, 0, 1>;  17 block_fused_kernel<0, 1, 1>
 * (the timing variants DBG 1..7 compute wrong results by design and are not reachable through this hook) */
typedef struct m3pc_debug_block_args {
    const void* O;
    int ldo;
    int M;
    const void* res; /* fp32 rows, bf16 rows when x_bf16; or rowtab */
    int ldr;
    int res_L, res_nshared;
    const float* rowtab;
    int rt_mod, res_nu;
    const void* Wo;
    const void* W1;
    const void* W2;
    const void* Wqkv; /* optional: with QKVout */
    const void* Wh;   /* optional: with head_out */
    void* stream_buf;
    const float* bo;
    const float* b1;
    const float* b2;
    const float* ln2_g;
    const float* ln2_b;
    const float* lnA_g;
    const float* lnA_b;
    const float* lnB_g[2];
    const float* lnB_b[2];
    void* Xout; /* optional; with split: the slabs */
    int ldx;
    int x_bf16;
    void* Hout; /* optional */
    int ldh;
    int out_mod, out_grp;
    void* QKVout; /* optional */
    int ldq;
    long long qkv_bytes;
    const float* bqkv;
    const float* hb1;
    const float* hw2;
    const float* hb2;
    const float* hmean; /* optional */
    const float* hstd;
    float* head_out[2]; /* optional */
    int split;
    float* red_Xout; /* optional */
    int red_ldx;
    void* red_Hout; /* optional */
    int red_ldh;
    const float* red_lnA_g;
    const float* red_lnA_b;
    const float* red_lnB_g[2];
    const float* red_lnB_b[2];
    int red_out_mod, red_out_grp;
    void* stream;
    int* picked; /* optional: 1 int */
} m3pc_debug_block_args;
int m3pc_debug_block_ex(const m3pc_debug_block_args* a);
/* the same checks without packing or launching anything (no GPU needed): the refusals, and `picked` as m3pc_debug_block_ex reports it */
int m3pc_debug_block_accepts(const m3pc_debug_block_args* a);
int m3pc_debug_block_split_n(void);
/* x_bf16 with res_L > 0 (forms 16 / 17): `res` is the compact block -- the res_nshared shared rows once, then the res_L - res_nshared
 * own rows of sequence 0, 1, ... -- and this is the row of it that token row r takes as its residual (-1: arguments out of range).
 * Host only, no GPU needed (tests/test_block_shared_xb_cpu.py) */
int m3pc_debug_block_res_row(int r, int res_L, int res_nshared);
/* the embedding kernel (launch_embed; d % 64 == 0, d <= 1024 as a handle takes it: the wave-per-row kernel embed_rows_kernel at d = 256,
 * 512, 768 or 1024, the block-per-row embed_kernel at every other d) on caller tensors: token j of batch element
 * b is key tokmap[2 j] at step t = tokmap[2 j + 1], its row X[b L + j] = tok[key][b bstride[key] + t feat[key] ..] WT[key] + E[key][t]
 * (WT (feat, d), E (T, d) fp32; no normalisation, no window index), stored as fp32 (X) or bf16 (Xb); with ln_g / ln_b also
 * LayerNorm(row) as bf16 to Hb (n_sh > 0: tokens j < n_sh once to Hb_sh[j], the others to Hb[b (L - n_sh) + j - n_sh]).  The first
 * n_indep tokens do not depend on b; x_first_only: their X rows are stored for b = 0 only; x_compact (with Xb, x_first_only,
 * n_indep > 0): Xb holds those n_indep rows once and behind them the L - n_indep own rows of b = 0, 1, ... (m3pc_debug_block_res_row).
 * Refused with M3PC_EINVAL before anything is launched: d % 64, d < 64, d > 1024, a token's key outside [0, 3], with feat < 1 (or
 * above 32 where embed_kernel runs: its LDS row) or without tok / WT / E, a token step outside [0, T), and, where embed_kernel runs, what that kernel does
 * not implement: Xb, n_sh, n_indep, x_first_only, x_compact.  The checks of d and of embed_kernel's options come first and need no
 * GPU; tokmap (device memory) is then copied back for the checks of its entries.  The kernel launched: m3pc_debug_elementwise_picked. */
typedef struct m3pc_debug_embed_args {
    const float* tok[4];
    long long bstride[4];
    const float* WT[4];
    const float* E[4];
    int feat[4];
    const int* tokmap; /* (L, 2) int32 */
    int batch, L, d, T;
    float* X;
    void* Xb;
    const float* ln_g; /* optional */
    const float* ln_b;
    void* Hb;    /* optional */
    void* Hb_sh; /* with n_sh > 0 */
    int n_indep, n_sh, x_first_only, x_compact;
    void* stream;
} m3pc_debug_embed_args;
int m3pc_debug_embed(const m3pc_debug_embed_args* a);
/* the same launch with what EmbedP carries beside it: Hf (optional, with ln_g / ln_b), the LayerNorm rows in fp32 (batch L, d) -- what
 * holds the fused norm to its fp32 bound and not only through the bf16 rounding of Hb (not with n_sh) -- and picked (1 int, optional).
 * Both entry points copy tokmap back with a synchronous hipMemcpy on every call: do not time a kernel through them. */
typedef struct m3pc_debug_embed_ex_args {
    m3pc_debug_embed_args base;
    float* Hf;
    int* picked;
} m3pc_debug_embed_ex_args;
int m3pc_debug_embed_ex(const m3pc_debug_embed_ex_args* a);
/* the fused decoder input (kv_fused_kernel) on caller tensors */
long long m3pc_debug_kv_stream_bytes(void);
int m3pc_debug_kv_fused(const void* Z, int n, int Le, int kept0, int off0, int kept1, int off1, const void* We0, const void* We1,
                        const void* Wkv, void* stream_buf, const float* rowtab0, const float* rowtab1, const float* ln_g,
                        const float* ln_b, const float* bkv, void* KV, void* stream, long long* stamps);
/* the same with everything KvFusedP carries: group g holds M[g] rows (0: absent; group 1 only with group 0), its row r is row
 * (r / rpg) gstride + r % rpg + off of Z (ldz) and of KV (ldkv) under map[g] = {rpg, gstride, off} (rpg 0: identity), embedded with
 * We[g] (512, 512) bf16 + rowtab[g][r % rt_mod[g]]; Wkv (1024, 512) bf16; stream_buf: 2 * m3pc_debug_kv_stream_bytes() bytes.
 * kv_bytes: the size of the KV buffer from its base (stores behind it are dropped).  Refusals: launch_kv_fused's. */
typedef struct m3pc_debug_kv_args {
    const void* Z;
    int ldz;
    int M[2];
    int map[2][3];
    const float* rowtab[2];
    int rt_mod[2];
    const void* We[2];
    const void* Wkv;
    void* stream_buf;
    const float* ln_g;
    const float* ln_b;
    const float* bkv;
    void* KV;
    int ldkv;
    long long kv_bytes;
    void* stream;
} m3pc_debug_kv_args;
int m3pc_debug_kv_fused_ex(const m3pc_debug_kv_args* a);
/* the bf16 attention of an encoder layer of the candidate pass on caller tensors: QKV (batch, n_own, 1536) per-candidate rows
 * [Q | K | V] and, when n_sh > 0, QKVs (n_sh, 1536) rows shared by the batch (first layer: history tokens); O (batch, n_own + n_sh, 512),
 * shared rows first.  4 heads of 128.  kernel: 0 = what the library picks, 1 = never the pipelined kernel, 2 / 3 = the pipelined kernel
 * without its arithmetic / without its loads (timing only).
 * stamps: optional 16 int64 (device): shader-clock stamps of one workgroup's third item in the pipelined kernel */
int m3pc_debug_attention_bf16(const void* QKV, const void* QKVs, void* O, int batch, int n_own, int n_sh, int kernel, void* stream,
                              long long* stamps);
/* the decoder's bf16 attention of an rtg_guiding candidate pass: Qtab (nq <= 32, 1536) the batch-shared query rows [Q | . | .], QKVm (Lm, 1536)
 * the masked tokens' rows [. | K | V] (their block of the softmax is pre-reduced into `pre`: 4 * nq * (2 + 128) floats of scratch), KV (n, 49, 1024)
 * the candidates' own [K | V] rows; O (n, nq, 512).  kernel as m3pc_debug_attention_bf16 */
int m3pc_debug_attention_dec_bf16(const void* Qtab, const void* QKVm, const void* KV, void* O, float* pre, int n, int nq, int Lm, int kernel,
                                  void* stream);
/* the same with Le own [K | V] rows per candidate (KV (n, Le, 1024)) and nq <= 64: the T = 64 decoder is Le = 97, nq = 64 */
int m3pc_debug_attention_dec_le_bf16(const void* Qtab, const void* QKVm, const void* KV, void* O, float* pre, int n, int nq, int Lm, int Le,
                                     int kernel, void* stream);
/* the decoder's bf16 attention of a critic_lambda_guiding candidate pass: Qown (n, Lq <= 4, 512) the candidates' own query rows, Qsh (Lq2, 1536)
 * the batch-shared query rows [Q | . | .], KV (n, 49, 1024) the candidates' own [K | V] rows, QKVm (79, 1536) the batch-shared rows [. | K | V];
 * O (n, Lq + Lq2, 512), own rows first.  kernel as m3pc_debug_attention_bf16 */
int m3pc_debug_attention_mix_bf16(const void* Qown, const void* Qsh, const void* KV, const void* QKVm, void* O, int n, int Lq, int Lq2, int kernel,
                                  void* stream);
/* any attention of the library on caller tensors, through launch_attention's dispatch.  dtype 0: fp32 rows, 1: bf16 rows.
 * Queries Q (row i of batch element b at Q + b q_bstride + i ldq; q_bstride 0: shared by the batch), Lq rows, output rows orow1 + i;
 * optional batch-shared second query segment Q2 (Lq2 rows, output rows orow2 + i; bf16 only).  Keys / values: K1, V1 per batch
 * element (L1 rows), optional batch-shared K2, V2 (L2 rows), optional batch-shared pre-reduced block Kp, Vp (Lp rows, bf16 only,
 * batch-shared queries and no Q2) reduced by the prestats kernel into `pre` (n_head * Lq * (2 + hd) floats of scratch).  O row r of
 * batch element b at O + b o_bstride + r ldo; head h owns columns [h hd, (h + 1) hd) of every row.  kernel: 0 = dispatch, 1 = never the
 * pipelined kernels.  Shapes no kernel covers return M3PC_EINVAL before anything is launched: hd not 32 / 64 / 128, L1 < 1, Lq < 1,
 * L1 + L2 > 256, Lp > 256, orow1 / Q2 / a pre block with fp32 rows, pointers not 16-byte aligned, strides not multiples of 16 bytes.
 * picked (2 ints, optional): [0] the id of the attention kernel launched, [1] 50 if the prestats kernel ran, else 0.
 * Kernel ids (tests/test_attention_gpu.py reaches every id of this list except the A/B-only ones):
 *   fp32 (attn.hip):   1 attn_pair_kernel<4>;  2 / 3 / 4 attn_split_kernel hd 32 / 64 / 128;
 *                      5 + 3 a + c: attn_kernel<HDT, NCH>, a = 0 / 1 / 2 for hd 32 / 64 / 128, c = 0 / 1 / 2 for NCH 1 / 2 / 4  (5..13)
 *   bf16 (attn_bf16.hip): 20 pipe<49, 0>;  21 pipe<17, 32>;  22 pipe_dec<49>;  23 pipe_mix<49, 79>;  24 pipe_wide<97, 0, 97, 0, false>;
 *                      25 pipe_wide<33, 64, 33, 64, false>;  26 pipe_wide<0, 64, 97, 0, true>;  27 / 28 / 29 pack2 hd 32 / 64 / 128;
 *                      30 + 3 a + f: direct<HDT, ., .>, f = 0 / 1 / 2 for <1, 2> / <2, 2> / <2, 4>  (30..38);
 *                      39 / 40 / 41 attn_bf16_kernel<HDT, 4> hd 32 / 64 / 128;
 *                      A/B-only (M3PC_NO_ATTN_DIRECT): 42 + 2 a + c attn_bf16_kernel<HDT, NCH>, c = 0 / 1 for NCH 1 / 2  (42..47)
 *   prestats:          50 attn_prestats_kernel */
int m3pc_debug_attention(int dtype, const void* Q, long long q_bstride, int ldq, int Lq, int orow1, const void* Q2, int ldq2, int Lq2,
                         int orow2, const void* K1, const void* V1, long long kv1_bstride, int ldkv1, int L1, const void* K2,
                         const void* V2, int ldkv2, int L2, const void* Kp, const void* Vp, int ldp, int Lp, float* pre, void* O,
                         long long o_bstride, int ldo, int batch, int n_head, int hd, float scale, int kernel, int* picked,
                         void* stream);
/* ---- the streaming and small reduction kernels of csrc/elementwise.hip, each alone on caller tensors, through its production
 * launcher (launch_layernorm, launch_head_out, ...): the launcher's dispatch decides which kernel runs and the hook reports it.
 * Every argument structure mirrors the kernel's parameter structure in csrc/kernels.h; a row map is {rpg, gstride, off} as in
 * m3pc_debug_gemm_ex.  picked (1 int, optional; 0 while nothing was launched): the id of the kernel launched.
 * Elementwise kernel ids (tests/test_elementwise_edges_gpu.py reaches every id of this list):
 *   1 embed_kernel;  2 embed_rows_kernel<1>;  3 embed_rows_kernel<2>;  4 embed_rows_kernel<3>;  5 embed_rows_kernel<4>;
 *   6 gather_rows_kernel;  7 layernorm_kernel;  8 layernorm_vec_kernel;  9 layernorm_rows_kernel<1, 2>;
 *   10 layernorm_rows_kernel<2, 2>;  11 layernorm_rows_kernel<3, 2>;  12 layernorm_rows_kernel<4, 2>;  13 head_out_kernel;
 *   14 head_out_mfma_kernel;  15 actor_head_kernel<4>;  16 actor_head_kernel<8>;  17 actor_head_small_kernel;  18 sample_kernel;
 *   19 critic_kernel;  20 critic_mfma_kernel<2>;  21 critic_mfma_kernel<4>;  22 critic_mfma_kernel<8>;  23 score_kernel;
 *   24 tokenize_kernel;  25 detokenize_kernel;  26 goal_overlay_kernel;  27 goal_overlay_rows_kernel
 * (not listed, no id: the A/B-only instances layernorm_rows_kernel<NV, 4> of M3PC_LN_RPW=4, and the weight-load helpers
 * f32_to_bf16_kernel, fill_kernel, transpose_f32_kernel and embed_table_kernel, which no hook drives)
 * The id of the elementwise kernel the calling thread launched last, for the entry points without a `picked` argument
 * (m3pc_debug_embed, m3pc_tokenize, m3pc_detokenize): */
int m3pc_debug_elementwise_picked(void);
/* LayerNorm (LnP): Y[r] = LN2?(LN1(X[xmap(r)] (ldx))), r < rows, eps 1e-5, biased variance; Yf fp32 and / or Yb bf16, contiguous
 * rows of d.  Refused with M3PC_EINVAL before anything is launched: a null X / g1 / b1, neither output, g2 without b2 (or b2 alone),
 * rows < 1, d % 64, d < 64, d > 1024 (a lane holds at most 16 values), ldx < d, a row map that is neither rpg == 0 nor rpg >= 1
 * with gstride >= rpg (off >= 0), and, where the 16-byte kernels run (d % 256 == 0 and ldx % 4 == 0), X / g1 / b1 / g2 / b2 / Yf
 * off 16 bytes or Yb off 8 bytes. */
typedef struct m3pc_debug_ln_args {
    const float* X;
    int ldx;
    int xmap[3];
    int rows, d;
    const float* g1;
    const float* b1;
    const float* g2; /* optional */
    const float* b2;
    float* Yf; /* optional */
    void* Yb;  /* optional */
    void* stream;
    int* picked;
} m3pc_debug_ln_args;
int m3pc_debug_layernorm(const m3pc_debug_ln_args* a);
/* an output head's last Linear with the de-tokeniser (HeadOutP): Y[ymap(r)] (ldy)[f] = (x[r] . W[f] + b[f]) stdv[f] + mean[f],
 * f < D (mean null: no de-tokeniser); W (D, d) fp32.  The rows come as fp32 X or bf16 Xb (or both): as the library's callers do,
 * the hook passes Xb on only where head_out_mfma_covers(rows, d, D) holds (d = 512, D <= 32, rows >= 2048: head_out_mfma_kernel),
 * and X otherwise.  Refused: no rows the chosen kernel can read (Xb alone where the matrix-core kernel does not cover, X alone is
 * always fine), null W / b / Y, mean without stdv or stdv alone, rows < 1, d % 64, d < 64, d > 1024, D outside [1, 32], ldx < d,
 * ldy < D, a bad row map, and for the matrix-core kernel Xb off 16 bytes or ldx % 8. */
typedef struct m3pc_debug_head_out_args {
    const float* X; /* optional */
    const void* Xb; /* optional */
    int ldx;
    int rows, d, D;
    const float* W;
    const float* b;
    const float* mean; /* optional */
    const float* stdv;
    float* Y;
    int ymap[3];
    int ldy;
    void* stream;
    int* picked;
} m3pc_debug_head_out_args;
int m3pc_debug_head_out(const m3pc_debug_head_out_args* a);
/* the actor head (ActorP): mu[r] = x . Wmu^T + bmu, sd[r] = exp(-5 + 3.5 (tanh(x . Wls^T + bls) + 1)), x = LN?(X[xmap(r)] (ldx));
 * Wmu / Wls (A, d), mu / sd (rows, A).  Refused: a null operand, rows < 1, d % 64, d < 64, d > 1024, A outside [1, 32], ldx < d, a
 * bad row map, ln_g without ln_b (or ln_b alone), ln_g where actor_head_fuses_ln(d, A) is false (actor_head_small_kernel has no
 * LayerNorm), and, where actor_head_kernel runs (d % 256 == 0, A <= 8), X / Wmu / Wls / ln_g / ln_b off 16 bytes or ldx % 4. */
typedef struct m3pc_debug_actor_args {
    const float* X;
    int ldx;
    int xmap[3];
    int rows, d, A;
    const float* Wmu;
    const float* bmu;
    const float* Wls;
    const float* bls;
    float* mu;
    float* sd;
    const float* ln_g; /* optional */
    const float* ln_b;
    void* stream;
    int* picked;
} m3pc_debug_actor_args;
int m3pc_debug_actor_head(const m3pc_debug_actor_args* a);
/* TwinQ (CriticP): q[r] = min over the two networks of W3 . relu(W2 relu(W1 [(s - om) / os | a] + b1) + b2) + b3.  W1[net]
 * (hidden, S + A) and W2[net] (hidden, hidden) are HOST arrays in torch Linear layout: the hook transposes them for critic_kernel
 * and packs them with critic_pack for critic_mfma_kernel inside the call (function-static device buffers, as m3pc_debug_gemm_ex
 * keeps its split of W); everything else is device memory.  force_scalar: never the matrix-core kernel.  Refused: a null operand,
 * rows < 1, S or A outside [1, 32] (the scalar kernel's LDS row holds S + A <= 64), hidden outside [1, 256] (one thread per hidden
 * unit), and, where the matrix-core kernel runs (S + A <= 32, hidden 64 / 128 / 256, not forced), b1 / b2 / W3 off 16 bytes. */
typedef struct m3pc_debug_critic_args {
    const float* states;
    const float* actions;
    int rows, S, A, hidden;
    const float* om;
    const float* os;
    const float* W1[2]; /* host */
    const float* b1[2];
    const float* W2[2]; /* host */
    const float* b2[2];
    const float* W3[2];
    const float* b3[2];
    float* q;
    int force_scalar;
    void* stream;
    int* picked;
} m3pc_debug_critic_args;
int m3pc_debug_critic(const m3pc_debug_critic_args* a);
/* critic_pack on host arrays (no GPU needed): W1 (hidden, SA), W2 (hidden, hidden) -> w1f (n_w1f floats), w2f (n_w2f floats, its
 * 1024 floats of read-ahead padding zeroed).  w1f / w2f null: only the sizes are reported.  Refused: SA outside [1, 32], hidden not
 * 64 / 128 / 256. */
int m3pc_debug_critic_pack(const float* W1, const float* W2, int SA, int hidden, float* w1f, float* w2f, long long* n_w1f,
                           long long* n_w2f);
/* candidate construction (SampleP).  eps_rows: the rows of eps (mode 0: of T A floats, else of h A); hist_windows: the windows of
 * hist_actions (1 without widx).  index / widx are device arrays whose entries the caller keeps below eps_rows / hist_windows.
 * Refused: mode outside 0 / 1 / 2, T or A < 1, n_count < 1, idx outside [0, T], h < T - idx (sampled steps would leave their row),
 * n_begin < 0 or n_begin + n_count > eps_rows without index, a null cand / eps, hist_actions null with idx > 0, loc null in modes
 * 0 / 1, sd null in mode 0. */
typedef struct m3pc_debug_sample_args {
    const float* hist_actions;
    const float* loc;
    const float* sd;
    const float* eps;
    int mode, T, A, idx, h, n_begin, n_count;
    const int* widx;  /* optional */
    const int* index; /* optional */
    float* cand;
    float* sample_actions; /* optional */
    float* loc_out;        /* optional */
    float* sd_out;         /* optional */
    long long eps_rows;
    int hist_windows;
    void* stream;
    int* picked;
} m3pc_debug_sample_args;
int m3pc_debug_sample(const m3pc_debug_sample_args* a);
/* TD(lambda) scoring (ScoreP).  Refused: a null rewards / boot / expect_return, n < 1, h < 1, scatter_out without scatter_index. */
typedef struct m3pc_debug_score_args {
    const float* rewards;
    const float* boot;
    int n, h;
    float boot_scale, gamma;
    double lmbda;
    float* expect_return;
    float* boot_out;          /* optional */
    const int* scatter_index; /* optional */
    float* scatter_out;
    void* stream;
    int* picked;
} m3pc_debug_score_args;
int m3pc_debug_score(const m3pc_debug_score_args* a);
/* row gather (GatherP): out[b, i] = Xe[b, rowsrc[i]] (rowsrc[i] >= 0) or table[-rowsrc[i] - 1].  rowsrc is a HOST array: the hook
 * checks every entry against xe_rows / table_rows and uploads it.  Refused: neither output, batch or rows_per_batch < 1, d % 64,
 * d < 64, d > 1024, an entry of rowsrc outside its source (or a source that is null), xe_bstride % 4 or below xe_rows d where batch > 1
 * (the batch elements' rows would alias), Xe / table / out off 16 bytes (outb takes 2-byte stores: any address). */
typedef struct m3pc_debug_gather_args {
    const float* Xe;
    long long xe_bstride;
    const float* table;
    const int* rowsrc; /* host */
    int rows_per_batch, batch, d;
    float* out; /* optional */
    void* outb; /* optional */
    int xe_rows, table_rows;
    void* stream;
    int* picked;
} m3pc_debug_gather_args;
int m3pc_debug_gather_rows(const m3pc_debug_gather_args* a);
/* the goal overlays (launch_goal_overlay / launch_goal_overlay_rows): windows of T rows of D floats; pred is de-tokenised in place
 * (normalize) and written over rows t <= idx and idx + 2 <= t <= T - 2 of states_out, the other rows come from states_in; the rows
 * form reads the nq overlay rows of each window from pred (windows nq, D) instead.  Refused: a null pointer, windows / T / D < 1,
 * idx outside [0, T - 1], normalize without mean / stdv, nq below the number of overlay rows. */
int m3pc_debug_goal_overlay(float* pred, const float* states_in, float* states_out, long long windows, int T, int D, int idx,
                            const float* mean, const float* stdv, int normalize, void* stream, int* picked);
int m3pc_debug_goal_overlay_rows(const float* pred, const float* states_in, float* states_out, long long windows, int T, int D, int idx,
                                 int nq, void* stream, int* picked);
/* ---- the kernels of csrc/mtm_grad.hip (the gradient of the masked-trajectory loss), each alone on caller tensors, through the
 * launchers m3pc_mtm_grad itself uses (csrc/mtm_grad.h: mg_launch_*): grid geometry, the `vec` decision of the product and the chunk
 * count of the column sums are the production ones.  Every argument structure mirrors the kernel's parameter structure in
 * csrc/mtm_grad.h; a row map is {rpg, gstride, off}.  picked (2 ints, optional; 0 while nothing was launched): [0] the id of the
 * kernel launched last, [1] the set of ids the call launched (bit id).  Every refusal is M3PC_EINVAL and comes before any HIP call.
 * MTM-gradient kernel ids (tests/test_mtm_grad_kernel_edges_gpu.py reaches every id of this list):
 *   1 mg_gemm_kernel<false>;  2 mg_gemm_kernel<true>;  3 mg_ln_fwd_kernel;  4 mg_ln_bwd_kernel;  5 mg_colsum_kernel;
 *   6 mg_colsum_fin_kernel;  7 mg_attn_fwd_kernel;  8 mg_attn_col_kernel;  9 mg_attn_row_kernel;  10 mg_embed_kernel;
 *   11 mg_gather_kernel;  12 mg_scatter_kernel;  13 mg_tokv_kernel;  14 mg_std_kernel;  15 mg_loss_bwd_kernel
 * (end of the MTM-gradient kernel ids) */
/* one operand of the product (GOp): element (o, k) is p[row(o) s_o + k s_k], or p[o s_o + row(k) s_k] with map_k; len: the floats
 * behind p (the hook refuses a product that would read beyond them) */
typedef struct m3pc_debug_mg_op {
    const float* p;
    long long s_o, s_k;
    int map[3];
    int map_k;
    long long len;
} m3pc_debug_mg_op;
/* the product (GemmG): C[cmap(m) ldc + n] (+)= epilogue(sum_k A(m, k) B(k, n)), epilogue = ((acc + (bias[n] + bias2[n])) +
 * pos[(m % pos_T) N + n]) + res[at], times gelu'(gelu_aux[at]); gelu_out[at] = gelu(C).  res, gelu_aux, gelu_out share C's layout
 * and c_len floats.  splitk: mg_gemm_kernel<true>.  Refused: a null A.p / B.p / C, M / N / K < 1, negative strides, a bad row map
 * (rpg < 0, off < 0, gstride < rpg), bias2 without bias, pos with pos_T < 1, ldc < N, an operand or C index beyond len / c_len or
 * beyond int. */
typedef struct m3pc_debug_mg_gemm_args {
    m3pc_debug_mg_op A, B;
    float* C;
    long long ldc, c_len;
    int cmap[3];
    int M, N, K;
    const float* bias;
    const float* bias2;
    const float* pos;
    int pos_T;
    const float* res;
    const float* gelu_aux;
    float* gelu_out;
    int accumulate, splitk;
    void* stream;
    int* picked;
} m3pc_debug_mg_gemm_args;
int m3pc_debug_mg_gemm(const m3pc_debug_mg_gemm_args* a);
/* LayerNorm (LnG), eps 1e-5, biased variance.  backward 0: Y[r] = LN(X[xmap(r)]) g + b and st[r] = (mean, rstd), r < rows;
 * backward 1: dX[xmap(r)] (+)= rstd (g' - mean(g') - xhat mean(g' xhat)), g' = dY[r] g, from the st given.  x_rows: the rows of X
 * (and of dX).  Refused: rows / d < 1, rows d beyond int, a bad row map, xmap(rows - 1) >= x_rows, a null X / g / st, forward
 * without b / Y, backward without dY / dX. */
typedef struct m3pc_debug_mg_ln_args {
    int backward;
    const float* X;
    int xmap[3];
    long long x_rows;
    const float* g;
    const float* b;
    float* Y;
    float* st;
    const float* dY;
    float* dX;
    int rows, d, accumulate;
    void* stream;
    int* picked;
} m3pc_debug_mg_ln_args;
int m3pc_debug_mg_layernorm(const m3pc_debug_mg_ln_args* a);
/* column sums, both stages (ColG): out0[c] = sum over the rows (s, j), s < nseq, j < n, bit j of sel, of dY[row][c]; with X / st
 * out1[c] = the same sum of dY xhat.  The buffer row is s L + j0 + j, the compact row s n + j (dY: the compact row with dy_compact;
 * st: always).  part: part_doubles doubles of scratch; buf_rows: the rows of X, and of dY unless compact.  Refused: a null dY / out0 /
 * part, X without st or st without X, out1 without X, nseq < 1, n outside [1, 64], j0 < 0, j0 + n > L, C < 1, ldy < C, buf_rows
 * below (nseq - 1) L + j0 + n, part_doubles below chunks 2 C (chunks = ceil(nseq n / 64)), counts beyond int. */
typedef struct m3pc_debug_mg_colsum_args {
    const float* dY;
    int dy_compact;
    long long ldy;
    const float* X;
    const float* st;
    int nseq, L, j0, n;
    unsigned long long sel;
    int C;
    double* part;
    long long part_doubles, buf_rows;
    float* out0;
    float* out1;
    void* stream;
    int* picked;
} m3pc_debug_mg_colsum_args;
int m3pc_debug_mg_colsum(const m3pc_debug_mg_colsum_args* a);
/* the four attention kernels (AttG).  which 0: mg_attn_fwd_kernel (QKV -> P, O); 1: mg_attn_col_kernel dV = P^T dO; 2:
 * mg_attn_row_kernel (P, dO, QKV -> dS over P, dQ); 3: mg_attn_col_kernel dK = dS^T Q scale.  QKV, dQKV (B L, 3 d); O, dO (B L, d);
 * P (B, nh, L, L).  Refused: which outside [0, 3], B < 1, L outside [1, 256], nh / hd < 1, nh hd != d, B nh L L or B L 3 d beyond
 * int, a null pointer the kernel uses. */
typedef struct m3pc_debug_mg_attn_args {
    int which;
    const float* QKV;
    float* P;
    float* O;
    const float* dO;
    float* dQKV;
    int B, L, d, nh, hd;
    float scale;
    void* stream;
    int* picked;
} m3pc_debug_mg_attn_args;
int m3pc_debug_mg_attention(const m3pc_debug_mg_attn_args* a);
/* the token-layout kernels (EmbG).  which 0: mg_embed_kernel (tok, W, bias, pdim, pos -> X); 1: mg_gather_kernel (src, mtok -> dst);
 * 2: mg_scatter_kernel (src -> dst); 3: mg_tokv_kernel (tok[key] -> out).  Refused: which outside [0, 3], B < 1, T outside [1, 64],
 * d < 1, a bit of bits[k] at or above T, kept[k] != popcount(bits[k]), eoff[k] != kept[0] + .. + kept[k - 1], Le != their sum or
 * < 1, B 4 T d beyond int, a null pointer the kernel uses (embed: tok / W / bias / pdim of every key with kept > 0 and feat >= 1
 * there; gather: mtok of every key), tokv with key outside [0, 3], kept[key] < 1 or feat[key] < 1. */
typedef struct m3pc_debug_mg_tokens_args {
    int which;
    const float* tok[4];
    const float* W[4];
    const float* bias[4];
    const float* pdim[4];
    const float* pos;
    const float* mtok[4];
    unsigned long long bits[4];
    int kept[4], eoff[4], feat[4];
    int B, T, d, Le;
    float* X;
    const float* src;
    float* dst;
    int key;
    float* out;
    void* stream;
    int* picked;
} m3pc_debug_mg_tokens_args;
int m3pc_debug_mg_tokens(const m3pc_debug_mg_tokens_args* a);
/* sd[i] = exp(-5 + 3.5 (tanh(ls[i]) + 1)), i < n.  Refused: a null pointer, n < 1. */
int m3pc_debug_mg_std(const float* ls, float* sd, long long n, void* stream, int* picked);
/* the loss backward (LossBwdG): dpred of the three scalar heads, dmu and d log_std of the action head.  Refused: a null pointer,
 * batch / S / A < 1, T outside [1, 64], a mask bit at or above T, unknown flag bits, loss_keys outside [0, 15], batch T (S + 2 + A)
 * beyond int. */
typedef struct m3pc_debug_mg_loss_bwd_args {
    const float* pred[3];
    const float* mu;
    const float* sd;
    const float* ls;
    const float* tgt[4];
    const float* eps;
    float* dpred[3];
    float* dmu;
    float* dls;
    unsigned long long mask[4];
    int batch, T, S, A, flags, loss_keys;
    float entropy_reg, inv_cnt;
    void* stream;
    int* picked;
} m3pc_debug_mg_loss_bwd_args;
int m3pc_debug_mg_loss_bwd(const m3pc_debug_mg_loss_bwd_args* a);
/* ---- the kernels of csrc/mtm_dropout.hip: the product and the attention kernels above with the keep masks of a dropout site, dY = dX k
 * over rows, and the mask itself (csrc/mtm_grad.h, DROPOUT: sites, counter layout, arithmetic order).  The hooks go through the same
 * launchers: with p == 0 (or p < 2^-32, which drops nothing) the launch is the one without dropout and reports its id.
 * MTM-dropout kernel ids (tests/test_mtm_dropout_kernel_edges_gpu.py reaches every id of this list):
 *   16 mg_gemm_drop_kernel;  17 mg_attn_fwd_drop_kernel;  18 mg_attn_col_drop_kernel;  19 mg_attn_row_drop_kernel;
 *   20 mg_drop_rows_kernel;  21 mg_keep_kernel
 * (end of the MTM-dropout kernel ids) */
/* a site: an element is kept iff its Philox word of (seed, draw, site) is >= floor(p 2^32); kept elements are multiplied by
 * (float)(1 / (1 - p)).  Refused by every hook: p not finite or outside [0, 1), site outside [0, 255], more than 2^32 quads. */
typedef struct m3pc_debug_mg_drop {
    double p;
    unsigned long long seed, draw;
    int site;
} m3pc_debug_mg_drop;
/* the product with the mask of a matrix site of extent (M, N) on element (m, n): ((acc + bias + bias2) + pos) k + res; with gelu_out
 * C stays unmasked and gelu_out = gelu(C) k; with gelu_aux (acc k) gelu'(aux).  Refused too: splitk with p >= 2^-32. */
typedef struct m3pc_debug_mg_gemm_drop_args {
    m3pc_debug_mg_gemm_args g;
    m3pc_debug_mg_drop drop;
} m3pc_debug_mg_gemm_drop_args;
int m3pc_debug_mg_gemm_drop(const m3pc_debug_mg_gemm_drop_args* a);
/* the attention kernels with site 0 of a layer.  which 0: P keeps the undropped probability and carries "dropped" in its sign bit, O =
 * (P k) V; 1: dV = (|P| k)^T dO; 2: dP = (dO V^T) k, dS = |P| (dP - sum dP |P|) over P, dQ; 3: dK, the launch without dropout. */
typedef struct m3pc_debug_mg_attn_drop_args {
    m3pc_debug_mg_attn_args a;
    m3pc_debug_mg_drop drop;
} m3pc_debug_mg_attn_drop_args;
int m3pc_debug_mg_attention_drop(const m3pc_debug_mg_attn_drop_args* a);
/* dY[r][c] = dX[r][c] k(r, c) over (R, C) compact rows (dY may be dX).  Refused too: a null dX / dY, R / C < 1, R C beyond int, p < 2^-32. */
typedef struct m3pc_debug_mg_drop_rows_args {
    const float* dX;
    float* dY;
    int R, C;
    m3pc_debug_mg_drop drop;
    void* stream;
    int* picked;
} m3pc_debug_mg_drop_rows_args;
int m3pc_debug_mg_drop_rows(const m3pc_debug_mg_drop_rows_args* a);
/* keep[r C + c] = 0 / 1 (device bytes): attention 0, the matrix site of extent (R, C); 1, R = B n_head L attention rows of C = L keys */
int m3pc_debug_mtm_keep(const m3pc_debug_mg_drop* d, int attention, long long R, int C, unsigned char* keep, void* stream, int* picked);
/* ---- the kernels of csrc/iql.hip (the IQL trainer), each alone on caller tensors, through the launchers m3pc_iql_train_step,
 * _evaluate, _load, _export and _publish_critic themselves use (csrc/iql.h: iql_launch_*): grid geometry, the tile count of the
 * gradient grid and the block count of the copies are the production ones.  The caller owns every buffer; no hook creates a trainer.
 * picked (2 ints, optional; 0 while nothing was launched): [0] the id of the kernel launched last, [1] the set of ids the call
 * launched (bit id).  Every refusal is M3PC_EINVAL and comes before any HIP call.
 * IQL-trainer kernel ids (tests/test_iql_kernel_edges_gpu.py reaches every id of this list):
 *   1 iql_fwd1_kernel;  2 iql_fwd2_kernel;  3 iql_fwd3_kernel;  4 iql_loss_kernel;  5 iql_delta_kernel<2>;  6 iql_delta_kernel<1>;
 *   7 iql_grad_kernel;  8 iql_eval_out_kernel;  9 iql_copy_kernel;  10 iql_publish_kernel
 * (end of the IQL-trainer kernel ids) */
/* one network (NetP), torch layout: W1 (H, in), b1 (H), W2 (H, H), b2 (H), W3 (out, H), b3 (out) */
typedef struct m3pc_debug_iql_net {
    float* W1;
    float* b1;
    float* W2;
    float* b2;
    float* W3;
    float* b3;
    int in, out;
} m3pc_debug_iql_net;
/* IqlP, flat.  net[0..3] = V, Q1, Q2, actor (the trained networks, in that order in d3 / d2 / d1), net[4..5] = the targets of Q1 / Q2;
 * am / av their Adam moments.  Bp = B rounded up to 32.  h1, h2 (pass, Bp, H); out (pass, Bp, 32); d3 (4, Bp, 32); d2, d1 (4, Bp, H).
 * The backward of trained network t reads forward pass 1, 4, 5, 6 for t = 0, 1, 2, 3.  Feature k of layer 1 is (s[k] - om[k]) / os[k]
 * for k < S and action[k - S] beyond; s is next_state where pass_next is set.  Adam (csrc/iql.h): omb1 = 1 - beta1, b2 = beta2,
 * omb2 = 1 - beta2 in fp32; step_size[t] = lr / (1 - beta1^t), sqrt_bc2 = sqrt(1 - beta2^t) and eps in fp64; omt = 1 - tau.
 * Common refusals: a null structure, hidden not 64 / 128 / 256, B outside [1, 1024], A outside [1, 32], S outside [1, 64]. */
typedef struct m3pc_debug_iql_args {
    m3pc_debug_iql_net net[6];
    m3pc_debug_iql_net am[4];
    m3pc_debug_iql_net av[4];
    float* log_std;
    float* ls_m;
    float* ls_v;
    const float* om;
    const float* os;
    const float* state;
    const float* action;
    const float* reward;
    const float* next_state;
    const float* done;
    float* h1;
    float* h2;
    float* out;
    float* d3;
    float* d2;
    float* d1;
    float* losses; /* optional */
    int B, H, S, A;
    int npass, pass_net[7], pass_next[7];
    float expectile, beta, gamma, omt, tau, omb1, b2, omb2;
    double step_size[4], sqrt_bc2, eps;
    int which; /* forward: the layer 1, 2, 3; delta: L = 2, 1 */
    void* stream;
    int* picked;
} m3pc_debug_iql_args;
/* layer `which` of passes [0, npass) (network pass_net[f]).  1: state / next_state / action, om, os -> h1; 2: h1 -> h2; 3: h2 -> out
 * (tanh where pass_net[f] is 3).  Refused: which outside [1, 3], npass outside [1, 7], pass_net[f] outside [0, 5], a null pointer the
 * layer uses (layer 1: action only where a network is wider than S), in outside [1, 64] or above S + A (layer 1), out outside [1, 32]
 * (layer 3), b1 / h1 (layer 1), W2 / b2 / h1 / h2 (layer 2), W3 / h2 / out (layer 3) off 16 bytes. */
int m3pc_debug_iql_forward(const m3pc_debug_iql_args* a);
/* out (7 passes: next_v, v, q1t, q2t, q1, q2, mu), reward, done, action, log_std -> d3 (all four networks, rows < Bp, 32 columns),
 * losses (optional), and the Adam step of log_std / ls_m / ls_v with step_size[3].  Refused: a null pointer but losses. */
int m3pc_debug_iql_loss(const m3pc_debug_iql_args* a);
/* which 2: d2 = (W3^T d3) relu'(h2); which 1: d1 = (W2^T d2) relu'(h1); of the four trained networks.  Refused: which not 1 or 2, a null
 * W3 (W2) of net[0..3], out outside [1, 32], a null or 16-byte-unaligned d3 / h2 / d2 (d2 / h1 / d1). */
int m3pc_debug_iql_delta(const m3pc_debug_iql_args* a);
/* the gradients of the four trained networks from d1 / d2 / d3, h1 / h2 and the layer-1 features, Adam on every element, and the soft
 * update of net[4] / net[5].  Refused: a null tensor of net[0..5], am[0..3] or av[0..3], in outside [1, 64] or above S + A, out outside
 * [1, 32], a null d1 / d2 / d3 / h1 / h2 / om / os / state (next_state where pass_next of a backward's pass is set; action where a
 * network is wider than S). */
int m3pc_debug_iql_grad(const m3pc_debug_iql_args* a);
/* dst[r width + c] = out[r 32 + c], or with twin the smaller of that and out[(Bp + r) 32 + c].  Refused: a null pointer, rows outside
 * [1, 1024], Bp below rows or no multiple of 32, width outside [1, 32]. */
int m3pc_debug_iql_eval_out(const float* out, int Bp, int rows, int twin, int width, float* dst, void* stream, int* picked);
/* dst[i] = src[i], i < n.  Refused: a null pointer, n < 1. */
int m3pc_debug_iql_copy(float* dst, const float* src, long long n, void* stream, int* picked);
/* PublishP: q[0] / q[1] (in = SA, out = 1) -> W1T (SA, H), b1, W2T (H, H), b2, W3 (H), b3 (1) of each, om / os (S) -> c_om / c_os, and with
 * streams the operand streams W1F / W2F of critic_pack (m3pc_debug_critic_pack gives their lengths).  Refused: a null pointer (W1F / W2F
 * only with streams), hidden not 64 / 128 / 256, S < 1, SA <= S, SA > 64, in != SA, out != 1, streams with SA > 32. */
typedef struct m3pc_debug_iql_publish_args {
    m3pc_debug_iql_net q[2];
    float* W1T[2];
    float* b1[2];
    float* W2T[2];
    float* b2[2];
    float* W3[2];
    float* b3[2];
    float* W1F[2];
    float* W2F[2];
    const float* om;
    const float* os;
    float* c_om;
    float* c_os;
    int S, SA, H, streams;
    void* stream;
    int* picked;
} m3pc_debug_iql_publish_args;
int m3pc_debug_iql_publish(const m3pc_debug_iql_publish_args* a);
/* ---- csrc/mtm_opt.hip: mo_adamw_kernel (the AdamW launch of m3pc_mtm_opt_step) alone, on caller-given device arrays and a caller-given
 * segment table, through the launcher the trainer uses (csrc/mtm_opt.h: arithmetic order, block table, step-count arrays).  Segment i:
 * weight p[i] (device, numel[i] floats), gradient at grad + g_off[i], moments at exp_avg / exp_avg_sq + s_off[i], b[i] (optional; device,
 * 2 numel[i] bf16: hi | lo) written when write_bf16.  p, b, g_off, s_off, numel, decay, active are HOST arrays of n; steps_in / steps_out
 * DEVICE arrays of n int64 (distinct).  An inactive segment (active[i] == 0) keeps every bit and its step count.  n_blocks (optional out):
 * the workgroups launched.  The call waits for the launch.  Refused (M3PC_EINVAL, before any HIP call): a null pointer (b, n_blocks
 * and stream excepted), n outside [1, 4096], numel outside [1, 2^30], an offset + numel beyond grad_floats / state_floats, steps_in == steps_out. */
typedef struct m3pc_debug_mtm_adamw_args {
    int n;
    float* const* p;
    void* const* b;
    const long long* g_off;
    const long long* s_off;
    const long long* numel;
    const int* decay;
    const int* active;
    const float* grad;
    long long grad_floats;
    float* exp_avg;
    float* exp_avg_sq;
    long long state_floats;
    const long long* steps_in;
    long long* steps_out;
    int write_bf16;
    double lr_t, weight_decay, beta1, beta2, eps;
    void* stream;
    int* n_blocks;
} m3pc_debug_mtm_adamw_args;
int m3pc_debug_mtm_adamw(const m3pc_debug_mtm_adamw_args* a);
/* in-kernel phase stamps of workgroup 37 of every fused-tail launch as the step runs: cap > 0 starts a ring of cap entries
 * (64 int64 each), cap == 0 copies it to `out` (host), reports the number of launches logged and stops */
int m3pc_debug_stamp_log(m3pc_handle* h, int cap, long long* out, int* n_logged);
/* how many streams the handle has created for m3pc_plan_step_certified_begin (0: the pair of m3pc_set_step_streams serves them) */
int m3pc_debug_step_streams_created(m3pc_handle* h);
/* XCD / CU of every workgroup of a launch on `stream`: out[2 i] = XCC_ID, out[2 i + 1] = HW_ID */
int m3pc_debug_xcc_probe(int* out, int n_blocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* M3PC_HIP_DEBUG_H */
