// The gradient of the masked-trajectory loss (include/m3pc_hip.h: m3pc_mtm_grad*): Learner.compute_mtm_loss / omtm.forward_loss and
// loss.backward() through the whole model on the device, one gradient tensor per parameter.  Eval-mode model unless
// m3pc_mtm_grad_set_dropout switched the training-mode one on: DROPOUT, below.
//
// LAUNCHES of one call (n = layers of a stack; a "product" is one mg_gemm_kernel launch):
//   forward   tokenize x4; mg_embed_kernel (encoder rows); per layer: LayerNorm, Q|K|V product, mg_attn_fwd_kernel (keeps the
//             probabilities), out_proj product (+ residual), LayerNorm, linear1 product (keeps the pre-GELU rows and writes the GELU
//             rows beside them), linear2 product (+ residual); stack norm; mg_gather_kernel (decoder embedding inputs: kept rows and
//             mask tokens); four decoder-embedding products; the decoder layers and norm; per scalar head LayerNorm + two products,
//             the action head two products + mg_std_kernel; the two launches of mtm_loss.hip for the record.
//   backward  mg_loss_bwd_kernel (dpred, dmu, d log_std); per head of a key in loss_keys and for the action head: dX and dW products,
//             LayerNorm backward; stack norm backward; per layer, last to first: linear2 dX (times gelu') and dW, linear1 dX and dW,
//             LayerNorm backward, out_proj dX and dW, attention backward (three launches), Q|K|V dX and dW, LayerNorm backward; the
//             decoder-embedding dX and dW products; mg_scatter_kernel (kept rows back to encoder rows); the encoder the same way;
//             mg_tokv_kernel + a dW product (encoder embedding weights).  Every bias, LayerNorm weight / bias, per-dim encoding and mask token
//             is a column sum over rows: mg_colsum_kernel + mg_colsum_fin_kernel.
// What the forward keeps per layer and row: the layer input, both LayerNorm outputs and their (mean, rstd), Q|K|V, the attention
// output, the post-attention residual, the pre-GELU and the GELU rows; per (head, query, key) the attention probability.
//
// PRODUCTS.  mg_gemm_kernel: one wavefront per 32 x 32 output tile on v_mfma_f32_32x32x2_f32; both operands are read through
// (outer stride, k stride, row map), so Y = X W^T, dX = dY W and dW = dY^T X read X, dY and W where the forward left them; indices
// beyond M, N or K load zeros, so every extent may be ragged.  An element's K sum is one chain of fp32 fmas in ascending blocks of 16 k;
// in the dW form (K = rows) the four wavefronts of a workgroup share a tile, wavefront w taking the k blocks w, w + 4, ..., and
// wavefront 0 adds the partial tiles of wavefronts 1, 2, 3 in that order.
//
// REDUCTION ORDERS.  No floating-point atomics.  dW: the four chains above, rows ascending within each.  Column sums: rows in blocks of 64, each
// block summed in ascending order in float64 by the thread that owns the column, then the blocks in ascending order in float64,
// rounded to fp32 once.  LayerNorm and softmax rows: the 64-lane xor butterfly.  Attention backward: one wavefront per query row (dS,
// dQ: keys ascending) or key row (dV, dK: queries ascending).  The gradient buffers are zeroed at the start of every call, and nothing reads rows beyond `batch`.
//
// BYTES per batch element (fp32 words x 4), with L = 4 T, n = n_enc_layer + n_dec_layer:
//   saved      n L (8 d + 2 ff + 4 + n_head L)  +  L (5 d + 4)  +  T (9 d + 6)  [heads]  +  T (3 S + 6 A + 5)  [batch, eps, head outputs]
//   backward   L (7 d + ff)  +  T (2 d + S + 2 + 2 A)
//   float64    7 T doubles (the returns of a replay draw, the six row sums of the record)
// in all 4 [n L (8 d + 2 ff + 4 + n_head L) + L (12 d + ff + 4) + T (11 d + 4 S + 8 A + 13)] + 56 T bytes, each buffer rounded up to 256
// bytes; and, once per object, the gradient of every parameter and the column-sum partials (2 ceil(max_batch L / 64) max(3 d, ff) doubles).
//
// DROPOUT (m3pc_mtm_grad_set_dropout, p > 0; kernels in mtm_dropout.hip, device bodies in mtm_grad_body.h).  The four sites of a
// training-mode nn.TransformerEncoderLayer(norm_first=True), site id 4 layer + s, layers counted encoder first as `lay` is:
//   s 0  attention probabilities (B, nh, L, L)   O = (P * k) V;  dV = (P * k)^T dO;  dP = (dO V^T) * k, softmax backward on the undropped P
//   s 1  dropout1, out_proj output (R, d)        X1 = Xin + (O Wo^T + b) * k;  dY = dX * k feeds the dX and dW products and the bias sum
//   s 2  the FFN's dropout (R, ff)               Fact = gelu(Fpre) * k (stored dropped);  dF = ((dX W2) * k) gelu'(Fpre)
//   s 3  dropout2, linear2 output (R, d)         Xout = X1 + (Fact W2^T + b) * k;  backward as s 1
// k is scale = (float)(1.0 / (1.0 - p)) where the element is kept, 0 where it is dropped; kept iff its Philox word >= thr,
// thr = (uint32) floor(p 2^32), both computed on the host in double.  The keep-mask stream is a pure function of (seed, draw, site,
// logical element) (philox.h: key = seed, counter = (quad, draw lo, draw hi, array | site << 8)):
//   matrix sites (array 5)   quad = (row >> 2) C + col, word = row & 3; row: the row of the site's (R, C) activation
//   attention (array 6)      quad = ((b nh + h) L + i) ceil(L / 4) + (j >> 2), word = j & 3
// so nothing depends on batch, max_batch, the tiling or the workspace.  ARITHMETIC ORDER, exactly:
//   product, forward form      v = ((acc + (bias + bias2)) + pos);  v = kept ? __fmul_rn(v, scale) : 0;  v = v + res
//   product with gelu_out      C = v unmasked;  gelu_out = kept ? __fmul_rn(gelu(v), scale) : 0
//   product with gelu_aux      v = kept ? __fmul_rn(acc, scale) : 0;  v = v * gelu'(gelu_aux)
//   mg_drop_rows_kernel        dY = kept ? __fmul_rn(dX, scale) : 0
//   attention forward          the stored P keeps the undropped probability and carries "dropped" in its sign bit (P >= 0, so the bit
//                              is free); O sums (kept ? __fmul_rn(P, scale) : 0) V, keys ascending
//   attention backward         dV sums (kept ? __fmul_rn(|P|, scale) : 0) dO, queries ascending;  dP = kept ? __fmul_rn(dO . V_j, scale) : 0,
//                              then dS = |P| (dP - sum_j dP |P|) over P as without dropout; the dK launch is the one without dropout
// One Philox call serves the four accumulators a lane holds of one column (rows 4 q .. 4 q + 3), and four keys of one attention row:
// lane q of the row's wavefront draws quad q once and leaves the four bits in LDS.  No new buffer: dY of dropout2 goes to dO (free
// until the out_proj dX product writes it) and dY of dropout1 to dH (free between the LayerNorm backward that read it and the Q|K|V dX
// product).  Refused before any HIP call: more than 64 layers, a site of more than 2^32 quads.  With p == 0 no launch differs.
#pragma once
#include "m3pc_internal.h"

namespace m3pc {
// ------------------------------------------------------------------------------------------------ parameter structures
// (mtm_grad.hip holds the kernels; mg_run and the lab hooks of m3pc_debug.hip fill these and go through the launchers below)
// row r of a compact run -> row of the buffer: rpg rows per group, groups gstride rows apart, from row off (rpg == 0: r itself)
struct RMap {
    int rpg, gstride, off;
};
__host__ __device__ __forceinline__ long long rmap(const RMap& m, int r) {
    return m.rpg == 0 ? (long long)r : (long long)(r / m.rpg) * m.gstride + (r % m.rpg) + m.off;
}

// a dropout site of one launch (DROPOUT above); thr == 0: off
struct DropG {
    unsigned int thr;
    float scale;
    unsigned int k0, k1;  // seed lo, hi
    unsigned int d0, d1;  // draw lo, hi
    unsigned int c3;      // array | site << 8
};
constexpr unsigned int MG_DROP_MATRIX = 5, MG_DROP_ATTN = 6;  // (philox.h: the arrays)

// C[m][n] = sum_k A(m, k) B(k, n): element (o, k) of an operand is p[row(o) * s_o + k * s_k], or p[o * s_o + row(k) * s_k] with map_k
struct GOp {
    const float* p;
    long long s_o, s_k;
    RMap map;
    int map_k;
    int vec;  // k-contiguous, not row-mapped on k, 16-byte aligned rows: four k per load (mg_launch_gemm decides it)
};
struct GemmG {
    GOp A, B;
    float* C;
    long long ldc;
    RMap cmap;              // on m
    int M, N, K;
    const float *bias, *bias2;  // + bias[n] + bias2[n]
    const float* pos;       // + pos[(m % pos_T) * N + n]
    int pos_T;
    const float* res;       // + res[row(m) * ldc + n]
    const float* gelu_aux;  // * gelu'(gelu_aux[row(m) * ldc + n])
    float* gelu_out;        // gelu_out[row(m) * ldc + n] = gelu(C)
    int accumulate;         // C += instead of C =
    int splitk;             // the four wavefronts of a workgroup share a tile (mg_gemm_kernel<true>)
    DropG drop;             // the site's keep mask on element (m, n) of an (M, N) activation (never with splitk)
};

struct LnG {
    const float* X;   // rows xmap(r), ld d
    RMap xmap;
    const float *g, *b;
    float* Y;         // forward: compact rows
    float* st;        // (rows, 2): mean, rstd
    const float* dY;  // backward: compact rows
    float* dX;        // backward: rows xmap(r)
    int rows, d, accumulate;
};

// rows (s, j): s < nseq, j < n, bit j of sel set; the buffer row is s L + j0 + j, the compact row s n + j.
//   out0[c] = sum dY[row][c];  with X: out1[c] = sum dY[row][c] xhat[row][c]  (LayerNorm: bias and weight)
struct ColG {
    const float* dY;
    int dy_compact;
    long long ldy;
    const float* X;   // buffer rows, ld C
    const float* st;  // compact rows
    int nseq, L, j0, n;
    unsigned long long sel;
    int C;
    double* part;     // (chunks, 2, C)
    float *out0, *out1;
    int chunks;
};

struct AttG {
    const float* QKV;  // (B L, 3 d)
    float* P;          // (B, nh, L, L): probabilities, then dS
    float* O;          // forward out (B L, d)
    const float* dO;   // (B L, d)
    float* dQKV;       // (B L, 3 d)
    int B, L, d, nh, hd;
    float scale;
    DropG drop;        // site 0 of the layer: forward, dV and the row kernel
};

// dY[r][c] = dX[r][c] * k(r, c) over (R, C) compact rows
struct DropRowsG {
    const float* dX;
    float* dY;
    int R, C;
    DropG drop;
};

struct EmbG {
    const float *tok[4], *W[4], *bias[4], *pdim[4], *pos, *mtok[4];
    unsigned long long bits[4];
    int kept[4], eoff[4], feat[4];
    int B, T, d, Le;
    float* X;          // (B Le, d)  encoder rows (embed: out)
    const float* src;  // gather: EncN (B Le, d); scatter: dZin (B 4T, d)
    float* dst;        // gather: Zin (B 4T, d); scatter: dEncN (B Le, d)
};

struct LossBwdG {
    const float *pred[3], *mu, *sd, *ls, *tgt[4], *eps;
    float *dpred[3], *dmu, *dls;
    unsigned long long mask[4];
    int batch, T, S, A, flags, loss_keys;
    float entropy_reg, inv_cnt;  // 1 / (batch * hidden action timesteps * A)
    const float* entropy_reg_p;  // optional device scalar read in place of entropy_reg (the trainer's temperature, mtm_opt.h)
};

// ------------------------------------------------------------------------------------------------ launchers
// The grid geometry, the `vec` decision of the product, the chunk count of the column sums and their scratch size exist here once.
// The longest attention row the kernels hold in LDS (sp[4][MG_ATT_MAX_L]).
constexpr int MG_ATT_MAX_L = 256;
// decides A.vec / B.vec; no launch when M or N is 0
void mg_launch_gemm(GemmG& p, hipStream_t st);
void mg_launch_ln_fwd(const LnG& p, hipStream_t st);
void mg_launch_ln_bwd(const LnG& p, hipStream_t st);
// blocks of 64 rows (s, j) of a column sum, and the doubles of scratch its two stages need
inline int mg_colsum_chunks(long long total) { return (int)((total + 63) / 64); }
inline size_t mg_colsum_doubles(long long total, int C) { return (size_t)mg_colsum_chunks(total) * 2 * (size_t)C; }
// sets p.part = scratch (mg_colsum_doubles(nseq n, C) doubles) and p.chunks; both stages.  No launch when nseq n is 0.
void mg_launch_colsum(ColG& p, double* scratch, hipStream_t st);
void mg_launch_attn_fwd(const AttG& p, hipStream_t st);
void mg_launch_attn_col(const AttG& p, int which, hipStream_t st);
void mg_launch_attn_row(const AttG& p, hipStream_t st);
void mg_launch_embed(const EmbG& p, hipStream_t st);
void mg_launch_gather(const EmbG& p, hipStream_t st);
void mg_launch_scatter(const EmbG& p, hipStream_t st);
void mg_launch_tokv(const EmbG& p, int k, float* out, hipStream_t st);
void mg_launch_std(const float* ls, float* sd, long long n, hipStream_t st);
void mg_launch_loss_bwd(const LossBwdG& p, hipStream_t st);
// mtm_dropout.hip: what the launchers above call when p.drop.thr != 0, and the two kernels without a counterpart
void mg_launch_gemm_drop(const GemmG& p, hipStream_t st);
void mg_launch_attn_fwd_drop(const AttG& p, hipStream_t st);
void mg_launch_attn_col_drop(const AttG& p, hipStream_t st);  // (dV only)
void mg_launch_attn_row_drop(const AttG& p, hipStream_t st);
void mg_launch_drop_rows(const DropRowsG& p, hipStream_t st);
// keep[r * C + c] = 0 / 1 of a matrix site (array 5: extent (R, C)) or of attention (array 6: R = B nh L rows of C = L keys)
void mg_launch_keep(const DropG& d, long long R, int C, unsigned char* keep, hipStream_t st);
// thr, scale and the key / draw words of (p, seed, draw); c3 is left 0 for the caller to set per site.  (The limits of a gradient
// call -- layers, quads -- are checked by mg_precheck[_replay], in mtm_grad.hip.)
DropG mg_drop_make(double p, unsigned long long seed, unsigned long long draw);
}  // namespace m3pc

// ------------------------------------------------------------------------------------------------ the object
// (mtm_grad.hip fills it; mtm_opt.hip reads the parameter list, the gradient arena and the record of the last call)
struct m3pc_mtm_grad {
    m3pc_handle* h = nullptr;
    int max_batch = 0;
    bool ready = false, have_grad = false;
    bool consumed = false;       // the optimizer of mtm_opt.h has applied the gradients of the last call
    int last_loss_keys = 0;      // loss_keys of the last gradient call
    struct Par {
        std::string name;
        long long numel;
        size_t off;
    };
    std::vector<Par> par;
    std::map<std::string, int> idx;
    size_t grad_floats = 0;
    float* arena = nullptr;  // every fp32 buffer below
    double* arena64 = nullptr;
    float* grad = nullptr;
    struct Lay {
        float *Xin, *Hn1, *QKV, *P, *O, *X1, *Hn2, *Fpre, *Fact, *st1, *st2;
    };
    std::vector<Lay> lay;  // encoder layers, then decoder layers
    float *XencOut, *EncN, *st_enc, *Zin, *XdecOut, *DecN, *st_dec;
    m3pc::MtmStage s;  // tok, raw, eps out of arena; raw_returns, part out of arena64
    float *Hh[3], *st_h[3], *Hpre[3], *Hact[3], *pred[3], *mu, *ls, *sd;
    float *dX, *dH, *dQKV, *dF, *dO, *dpred[3], *dmu, *dls, *dh1, *dh2, *rec;
    double* colpart;
    // dropout (host state; DROPOUT above): every gradient call with drop_p > 0 uses drop_draw and advances it by one
    double drop_p = 0.0;
    unsigned long long drop_seed = 0, drop_draw = 0;
};

namespace m3pc {
// m3pc_mtm_grad / m3pc_mtm_grad_replay behind their null checks, under the caller's name `who`, in the three parts every entry makes in
// this order (the trainer of mtm_opt.hip: the first for all its steps, the second once, the third per step).
// 1. Every refusal of the call and bits[k], the mask of key k.  No HIP call, and a pure function of the arguments and of host state that
//    neither a gradient call, a replay draw nor an optimizer step writes (the handle's m3pc_dims, weights_loaded and tok_set; the
//    buffer's sizes, count and path lengths): what holds before the first of a run of steps holds before each of them.
int mg_precheck(const struct m3pc_mtm_grad* g, int batch, const unsigned char* const masks[4], int flags, int loss_keys, const char* who,
                unsigned long long bits[4]);
int mg_precheck_replay(const struct m3pc_mtm_grad* g, m3pc_replay* rb, int batch, int mode, const int* traj_index, const int* start_index,
                       int index_on_device, const unsigned char* const masks[4], int flags, int loss_keys, const char* who,
                       unsigned long long bits[4]);
// 2. The object's arenas, at the first call.
int mg_ensure(struct m3pc_mtm_grad* g);
// 3. The launches.  entropy_reg_p: optional device scalar read in place of entropy_reg.  The record lands in g->rec, and in `record`
//    too when given.  mg_run_replay draws the batch (and, with eps null, the normals) into the object's staging rows first.
int mg_run(struct m3pc_mtm_grad* g, int batch, const float* states, const float* actions, const float* rewards, const void* returns, int returns_f64,
           const unsigned long long bits[4], const float* eps, float entropy_reg, const float* entropy_reg_p, int flags, int loss_keys,
           float* record, hipStream_t st);
int mg_run_replay(struct m3pc_mtm_grad* g, m3pc_replay* rb, int batch, int mode, const int* traj_index, const int* start_index, int index_on_device,
                  unsigned long long seed, unsigned long long step, const unsigned long long bits[4], const float* eps, float entropy_reg,
                  const float* entropy_reg_p, int flags, int loss_keys, float* record, int* out_traj, int* out_start, hipStream_t st,
                  const char* who);
}  // namespace m3pc

