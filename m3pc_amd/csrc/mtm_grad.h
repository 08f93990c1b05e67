// The gradient of the masked-trajectory loss (include/m3pc_hip.h: m3pc_mtm_grad*): Learner.compute_mtm_loss / omtm.forward_loss and
// loss.backward() through the whole model on the device, one gradient tensor per parameter.  Eval-mode model: no dropout.
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
// bytes; and, once per object, the gradient of every parameter and the column-sum partials (2 (max_batch L / 64 + 2) max(3 d, ff) doubles).
#pragma once
#include "m3pc_internal.h"

struct m3pc_replay;
namespace m3pc {
int replay_segment_length(const m3pc_replay* rb);
}  // namespace m3pc
