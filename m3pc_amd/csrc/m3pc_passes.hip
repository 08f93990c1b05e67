// The forward passes of libm3pc_hip.so: the layer tail (GEMM chain or fused kernel), one transformer block (run_block), the encoder,
// the full decoder + heads (forward_impl: omtm.forward, mtm_model.py:593-716), the exactly pruned decoder and the candidate pass
// (learner.py:288-316).  Host side; see m3pc_internal.h.
#include "m3pc_internal.h"

namespace m3pc {

// ---------------------------------------------------------------------------------- layer tail
// Everything of a layer behind its attention (whose output rows are in h->O):
//     X' = residual + out_proj(O);  X'' = X' + linear2(gelu(linear1(norm2(X'))))
// Where the residual rows come from:
struct TailRes {
    const float* rows = nullptr;   // (M, d) rows (in place when the block output goes to the same rows), or
    const float* table = nullptr;  // (mod, d): row r takes table[r % mod] (decoder rows of masked query tokens, shared by the batch)
    int mod = 0;
    int nu = 0;                    // fused tail only, BlockP::res_nu: the first nu of every mod rows have rows of their own behind the table
};

// The tail as a GEMM chain -> Xout (fp32).  norm2 is folded into linear1's operand load (few-row fp32), else applied on the split-K
// reduce of the out-proj GEMM, else a launch of its own.  next_ln: the LayerNorm that follows on Xout, or null; -> whether
// linear2's split-K reduce applied it.
static bool chain_tail(m3pc_handle* h, const std::string& pfx, int rows, int dt, hipStream_t st, const TailRes& res, float* Xout,
                       const LnP* next_ln) {
    const int d = h->d, ff = h->ff;
    GemmP p = gemm_basic(h->O, d, Wop(h, pfx + ".self_attn.out_proj.weight", dt), d, rows, d, d, W(h, pfx + ".self_attn.out_proj.bias").f);
    if (res.table) {
        p.rowtab = res.table;
        p.rt_mod = res.mod;
        p.rt_ld = d;
    } else {
        p.res = res.rows;
        p.ldr = d;
    }
    gemm_out(p, DT_F32, Xout, d);
    const LnP ln = ln_rows(h, Xout, rows, W(h, pfx + ".norm2.weight").f, W(h, pfx + ".norm2.bias").f, h->Hn, dt);
    GemmP p1 = gemm_basic(h->Hn, d, Wop(h, pfx + ".linear1.weight", dt), d, rows, ff, d, W(h, pfx + ".linear1.bias").f);
    p1.gelu = 1;
    gemm_out(p1, dt, h->F, ff);
    GemmP t = p1;
    t.A = Xout;
    t.a_ln_g = ln.g1;
    t.a_ln_b = ln.b1;
    if (can_fold_ln(h, t, dt)) {
        gemm(h, p, dt, st);
        gemm(h, t, dt, st);
    } else {
        if (dt == DT_F32) {
            p.ln_g = ln.g1;
            p.ln_b = ln.b1;
            p.ln_out = ln.Yf;
        }
        if (!gemm(h, p, dt, st)) launch_layernorm(ln, st);
        gemm(h, p1, dt, st);
    }
    GemmP p2 = gemm_basic(h->F, ff, Wop(h, pfx + ".linear2.weight", dt), ff, rows, d, ff, W(h, pfx + ".linear2.bias").f);
    p2.res = Xout;
    p2.ldr = d;
    gemm_out(p2, DT_F32, Xout, d);
    if (dt == DT_F32 && next_ln && next_ln->Yf && !next_ln->Yb && !next_ln->g2 && next_ln->X == Xout && next_ln->xmap.rpg == 0 &&
        next_ln->rows == rows) {
        p2.ln_g = next_ln->g1;
        p2.ln_b = next_ln->b1;
        p2.ln_out = next_ln->Yf;
    }
    return gemm(h, p2, dt, st) != 0;
}

// Which tail a layer of `rows` rows takes, by the rows of the WHOLE step (m3pc_internal.h: FUSED_MIN_ROWS): the fused kernel with one
// workgroup per tile, its split form (four per tile + a reduce; the slabs of its partials must fit the F buffer), or the chain
enum TailForm { TAIL_CHAIN = 0, TAIL_SPLIT = 1, TAIL_FULL = 2 };
static TailForm tail_form(m3pc_handle* h, const std::string& pfx, int rows, int dt) {
    const PassSwitches& sw = pass_switches();
    if (dt != DT_BF16 || sw.no_block_fused || !h->wstream.count(pfx)) return TAIL_CHAIN;
    const double step_rows = (double)rows * h->pass_scale;
    if (step_rows >= (double)FUSED_MIN_ROWS) return TAIL_FULL;
    if (!sw.no_block_split && step_rows >= (double)SPLIT_MIN_ROWS && (long long)rows * block_split_n() * h->d <= h->R * 4LL * h->d)
        return TAIL_SPLIT;
    return TAIL_CHAIN;
}

// The tail as one launch (block_fused.hip), in `form` (not TAIL_CHAIN).  `b` arrives holding what is the caller's, as for the full
// form: the consumer of the block output (lnA / lnB / out_mod / out_grp with Hout, or QKVout, or head_*) and Xout.  In the split form
// that consumer goes to the reduce launch behind the kernel.  extra: flops per row of what the consumer adds to the launch.
// -> false: the kernel does not cover the arguments, nothing was launched.
static bool fused_tail(m3pc_handle* h, const std::string& pfx, int rows, int dt, hipStream_t st, TailForm form, const TailRes& res,
                       BlockP& b, double extra) {
    const int d = h->d;
    b.O = (const bf16_t*)h->O;
    b.ldo = d;
    b.M = rows;
    if (res.table) {
        b.rowtab = res.table;
        b.rt_mod = res.mod;
        b.res_nu = res.nu;
    } else {
        b.res = res.rows;
        b.ldr = d;
    }
    b.wstream = h->wstream[pfx];
    b.bo = W(h, pfx + ".self_attn.out_proj.bias").f;
    b.b1 = W(h, pfx + ".linear1.bias").f;
    b.b2 = W(h, pfx + ".linear2.bias").f;
    b.ln2_g = W(h, pfx + ".norm2.weight").f;
    b.ln2_b = W(h, pfx + ".norm2.bias").f;
    SplitReduceP r{};
    if (form == TAIL_SPLIT) {  // few tiles: four workgroups per tile, the consumer's LayerNorms on the reduce of their partials
        r.slabs = (const float*)h->F;
        r.M = rows;
        r.Xout = b.Xout;
        r.ldx = b.ldx;
        r.lnA_g = b.lnA_g;
        r.lnA_b = b.lnA_b;
        for (int s = 0; s < 2; ++s) {
            r.lnB_g[s] = b.lnB_g[s];
            r.lnB_b[s] = b.lnB_b[s];
        }
        r.out_mod = b.out_mod;
        r.out_grp = b.out_grp;
        r.Hout = b.Hout;
        r.ldh = b.ldh;
        b.split = 1;
        b.Xout = (float*)h->F;
        b.ldx = d;
        b.Hout = nullptr;
        b.ldh = 0;
    }
    if (h->stamp_log) {
        b.stamps = h->stamp_log + 64 * (h->stamp_i++ % h->stamp_cap);
        b.stamp_block = 37;
    }
    bool ok;
    {
        GemmTimer t(h, st, 2.0 * rows * ((double)d * d + 2.0 * d * h->ff + extra), dt, 1);  // (algorithmic: the split form's repeated out-proj is not counted)
        ok = launch_block_fused(b, st);
    }
    if (ok && form == TAIL_SPLIT) launch_block_split_reduce(r, st);
    return ok;
}

// can the fused tail apply next_ln (full rows of Xout -> bf16 rows)?
static bool tail_fuses_ln(const LnP* next_ln, const float* Xout, int rows) {
    return next_ln && next_ln->Yb && !next_ln->Yf && !next_ln->g2 && next_ln->X == Xout && next_ln->xmap.rpg == 0 && next_ln->rows == rows;
}

// ---------------------------------------------------------------------------------- transformer block
// Q|K|V + attention of the first layer of a candidate pass: the first n_sh tokens are the same for every candidate (history), so
// their norm1 rows and Q|K|V projections exist once (n_sh rows behind the compact per-candidate rows in Hn / QKV, written by the
// embedding kernel) and only the L - n_sh candidate-specific rows go through the big GEMM.  Attention still produces all L output
// rows per candidate: queries and keys are read from the two segments (own rows first, then the shared ones; softmax is
// order-independent up to rounding).
static void shared_rows_attention(m3pc_handle* h, const BlockArgs& a, int dt, hipStream_t st) {
    const int d = h->d, n_sh = a.n_sh, n_own = a.L - n_sh;
    const size_t es = dtype_size(dt);
    char* hn_sh = (char*)h->Hn + (size_t)a.batch * n_own * d * es;
    char* qkv_sh = (char*)h->QKV + (size_t)a.batch * n_own * 3 * d * es;
    const void* w = Wop(h, a.pfx + ".self_attn.in_proj_weight", dt);
    const float* bias = W(h, a.pfx + ".self_attn.in_proj_bias").f;
    GemmP p = gemm_basic(h->Hn, d, w, d, a.batch * n_own, 3 * d, d, bias);
    gemm_out(p, dt, h->QKV, 3 * d);
    gemm(h, p, dt, st);
    p = gemm_basic(hn_sh, d, w, d, n_sh, 3 * d, d, bias);
    gemm_out(p, dt, qkv_sh, 3 * d);
    gemm(h, p, dt, st);
    AttnP at = attn_basic(h, a.batch, a.L);
    const char* q = (const char*)h->QKV;
    at.Q = q;
    at.q_bstride = (long long)n_own * 3 * d;
    at.ldq = 3 * d;
    at.Lq = n_own;
    at.orow1 = n_sh;
    at.Q2 = qkv_sh;
    at.ldq2 = 3 * d;
    at.Lq2 = n_sh;
    at.orow2 = 0;
    at.K1 = q + (size_t)d * es;
    at.V1 = q + (size_t)2 * d * es;
    at.kv1_bstride = (long long)n_own * 3 * d;
    at.ldkv1 = 3 * d;
    at.L1 = n_own;
    at.K2 = qkv_sh + (size_t)d * es;
    at.V2 = qkv_sh + (size_t)2 * d * es;
    at.ldkv2 = 3 * d;
    at.L2 = n_sh;
    launch_attention(at, dt, st);
}

int run_block(m3pc_handle* h, const BlockArgs& a, int dt, hipStream_t st, PieceState& ps) {
    const int d = h->d, rows = a.batch * a.L;
    const std::string& pfx = a.pfx;
    bool ln1_done = ps.ln;
    const bool qkv_done = ps.qkv;
    ps.ln = ps.qkv = false;
    if (a.n_sh > 0) {
        shared_rows_attention(h, a, dt, st);  // (norm1 of the first layer comes from the embedding kernel)
    } else {
        const LnP ln = ln_rows(h, a.X, rows, W(h, pfx + ".norm1.weight").f, W(h, pfx + ".norm1.bias").f, h->Hn, dt);
        // norm1 in front of the Q|K|V projection: folded into that GEMM's operand load in the few-row fp32 passes
        GemmP pqkv = gemm_basic(h->Hn, d, Wop(h, pfx + ".self_attn.in_proj_weight", dt), d, rows, 3 * d, d,
                                W(h, pfx + ".self_attn.in_proj_bias").f);
        gemm_out(pqkv, dt, h->QKV, 3 * d);
        if (!ln1_done) {
            GemmP t = pqkv;
            t.A = a.X;
            t.a_ln_g = ln.g1;
            t.a_ln_b = ln.b1;
            if (can_fold_ln(h, t, dt)) {
                pqkv = t;
                ln1_done = true;
            }
        }
        if (!ln1_done && !qkv_done) launch_layernorm(ln, st);
        if (!qkv_done) gemm(h, pqkv, dt, st);
        AttnP at = attn_basic(h, a.batch, a.L);
        const char* q = (const char*)h->QKV;
        at.Q = q;
        at.q_bstride = (long long)a.L * 3 * d;
        at.ldq = 3 * d;
        at.Lq = a.L;
        at.K1 = q + (size_t)d * dtype_size(dt);
        at.V1 = q + (size_t)2 * d * dtype_size(dt);
        at.kv1_bstride = (long long)a.L * 3 * d;
        at.ldkv1 = 3 * d;
        at.L1 = a.L;
        launch_attention(at, dt, st);
    }
    if (a.x_bf16 && !ln1_done && !qkv_done) return fail(M3PC_EINVAL, "%s: norm1 of a bf16 residual stream has no kernel", pfx.c_str());
    // many-row bf16 passes: everything after the attention is one launch (block_fused.hip)
    const TailForm form = tail_form(h, pfx, rows, dt);
    TailRes res;
    res.rows = a.X;
    float* const Xout = a.Xnext ? a.Xnext : a.X;
    if (form != TAIL_CHAIN) {
        BlockP b{};
        const bool fuse_ln = tail_fuses_ln(a.next_ln, Xout, rows);
        // norm1 of the next layer never leaves the kernel: its Q|K|V rows do
        const bool fuse_qkv = form == TAIL_FULL && fuse_ln && a.next_qkv && !pass_switches().no_qkv_fused &&
                              a.next_ln->Yb == (bf16_t*)h->Hn && (size_t)rows * 3 * d * 2 < 0x7fffffffull;
        if (a.x_bf16 && !(fuse_ln && (fuse_qkv || a.x_dead)))
            return fail(M3PC_EINVAL, "%s: a bf16 residual stream needs the consumer of the block output inside the tail", pfx.c_str());
        if (a.res_nshared > 0) {
            b.res_L = a.L;
            b.res_nshared = a.res_nshared;
        }
        b.x_bf16 = a.x_bf16 ? 1 : 0;
        if (fuse_ln) {
            b.lnA_g = a.next_ln->g1;
            b.lnA_b = a.next_ln->b1;
        }
        if (fuse_qkv) {
            b.QKVout = (bf16_t*)h->QKV;
            b.ldq = 3 * d;
            b.qkv_bytes = (unsigned)((size_t)rows * 3 * d * 2);
            b.bqkv = W(h, *a.next_qkv + ".self_attn.in_proj_bias").f;
        } else if (fuse_ln) {
            b.Hout = a.next_ln->Yb;
            b.ldh = d;
        }
        if (!(fuse_ln && a.x_dead)) {
            b.Xout = Xout;
            b.ldx = d;
        }
        if (fused_tail(h, pfx, rows, dt, st, form, res, b, fuse_qkv ? 3.0 * d * d : 0.0)) {
            ps.ln = fuse_ln;
            ps.qkv = fuse_qkv;
            return check_launch(pfx.c_str());
        }
    }
    if (a.Xnext || a.res_nshared || a.x_bf16) return fail(M3PC_EINVAL, "%s: the fused layer tail did not take a pass set up for it", pfx.c_str());
    ps.ln = chain_tail(h, pfx, rows, dt, st, res, a.X, a.next_ln);
    return check_launch(pfx.c_str());
}


int run_encoder(m3pc_handle* h, Plan* pl, const TokIn& in, int batch, int dt, hipStream_t st, bool bf16_out_only,
                int n_indep, int layer_from, int layer_to, PieceState* ln_state) {
    const PassSwitches& sw = pass_switches();
    const int Le = pl->Le, d = h->d, nl = h->dm.n_enc_layer;
    // first-layer pruning (shared_rows_attention): whole 32-query tiles of shared tokens, bf16 candidate passes only
    int n_sh = 0;
    if (dt == DT_BF16 && batch >= 64 && d % 256 == 0 && d <= 1024 && n_indep >= 32 && !sw.no_prune1) n_sh = (n_indep / 32) * 32;
    // Round 6: the residual stream in bf16 between the layers (X: embedding -> layer tails; half of a tile's residual bytes in and
    // of its X'' bytes out; oracle/lowprec_study.py "bf16_res": the bf16 deviation delta x 0.95-1.25) -- when every layer of this
    // pass takes the full-tile fused tail with its consumer inside (next Q|K|V, or encoder.norm with X'' dead), so that nothing
    // but the tails ever reads X.  Decided from the pass's shape alone: the pieces of a pass enqueued layer by layer agree.
    bool xb16 = dt == DT_BF16 && bf16_out_only && !sw.no_bf16_residual && !sw.no_fused_anything && block_fused_supported(d, h->ff) &&
                (double)batch * Le * h->pass_scale >= (double)FUSED_MIN_ROWS && (size_t)batch * Le * 3 * d * 2 < 0x7fffffffull &&
                (unsigned long long)batch * Le * d * 2 < 0x80000000ull;
    for (int i = 0; i < nl && xb16; ++i) xb16 = h->wstream.count("encoder.layers." + std::to_string(i)) != 0;
    // The history rows of the bf16 residual stream stored once per pass (each half its own copy, in its own workspace rows) and
    // the candidates' own rows compactly behind them (block_res_row_xb): the embedding writes n_indep + batch (Le - n_indep) rows
    // instead of batch Le, and the first layer's tail reads those.  The block lives behind the full bf16 rows the first tail writes
    // (X'' goes to h->X as before, so nothing changes from the second layer on): a candidate owns 2 T fp32 rows of X, i.e. 4 T bf16
    // rows, of which the stream takes Le.  Decided from the pass's shape alone, like xb16.  M3PC_NO_SHARED_XB=1: the full rows.
    const long long xc_rows = (long long)n_indep + (long long)batch * (Le - n_indep);  // rows of the compact block
    const bool xb_shared = xb16 && n_sh > 0 && !sw.no_shared_xb && n_indep < Le &&
                           (long long)batch * Le + xc_rows <= (long long)batch * 4 * h->T &&
                           (h->X - h->cur->X) / d + (long long)batch * 2 * h->T <= h->R;
    bf16_t* const Xc = (bf16_t*)h->X + (size_t)batch * Le * d;
    if (layer_from <= 0) {
        EmbedP e{};
        e.n_indep = n_indep;
        e.n_sh = n_sh;
        e.Hb_sh = n_sh ? (bf16_t*)((char*)h->Hn + (size_t)batch * (Le - n_sh) * d * 2) : nullptr;
        for (int k = 0; k < 4; ++k) {
            e.tok[k] = in.ptr[k];
            e.bstride[k] = in.bstride[k];
            e.wstride[k] = in.wstride[k];
            e.normalize[k] = in.normalize[k];
            e.mean[k] = h->tok_mean[k];
            e.stdv[k] = h->tok_std[k];
            e.WT[k] = h->WT[k];
            e.E[k] = h->Eenc[k];
            e.feat[k] = h->feat[k];
        }
        e.x_first_only = e.x_compact = xb_shared ? 1 : 0;
        if (xb16) e.Xb = xb_shared ? Xc : (bf16_t*)h->X;
        e.widx = in.widx;
        e.tokmap = pl->d_tokmap;
        e.batch = batch;
        e.L = Le;
        e.d = d;
        e.T = h->T;
        e.X = h->X;
        e.ln_g = W(h, "encoder.layers.0.norm1.weight").f;  // first layer's norm1 fused into the embedding
        e.ln_b = W(h, "encoder.layers.0.norm1.bias").f;
        if (dt == DT_BF16)
            e.Hb = (bf16_t*)h->Hn;
        else
            e.Hf = (float*)h->Hn;
        launch_embed(e, st);
    }
    // encoder.norm: the candidate pass consumes the encoder output only as a bf16 GEMM operand
    const LnP ln = ln_rows(h, h->X, batch * Le, W(h, "encoder.norm.weight").f, W(h, "encoder.norm.bias").f,
                           bf16_out_only ? (void*)h->Z : (void*)h->EncOut, bf16_out_only ? DT_BF16 : DT_F32);
    PieceState ps = layer_from <= 0 || !ln_state ? PieceState{} : *ln_state;
    for (int i = layer_from > 0 ? layer_from : 0; i < nl && i < layer_to; ++i) {
        const std::string pfx = "encoder.layers." + std::to_string(i), nq = "encoder.layers." + std::to_string(i + 1);
        LnP nxt = ln;  // what follows layer i on X: norm1 of layer i+1 (-> Hn) or encoder.norm (-> EncOut / Z)
        if (i + 1 < nl) nxt = ln_rows(h, h->X, batch * Le, W(h, nq + ".norm1.weight").f, W(h, nq + ".norm1.bias").f, h->Hn, dt);
        BlockArgs b{pfx, h->X, batch, Le};
        b.n_sh = i == 0 ? n_sh : 0;
        b.next_ln = &nxt;
        b.x_dead = i + 1 == nl && bf16_out_only;
        b.next_qkv = i + 1 < nl ? &nq : nullptr;
        b.x_bf16 = xb16;
        if (xb_shared && i == 0) {  // the first tail reads the compact block and writes the full rows to X, where the stream stays
            b.X = (float*)Xc;
            b.Xnext = h->X;
            b.res_nshared = n_indep;
        }
        CHK(run_block(h, b, dt, st, ps));
    }
    if (ln_state) *ln_state = ps;
    if (layer_to >= nl && !ps.ln) launch_layernorm(ln, st);
    return check_launch("encoder");
}

// decoder-embed of rows of one key: Y[cmap rows] = Z[amap rows] W_dec_k^T + E_dec_k[r % mod]
static GemmP dec_embed_p(m3pc_handle* h, int k, const void* Zop, RowMap amap, float* Yout, RowMap cmap, int M, int mod, int dt,
                         const float* table) {
    const int d = h->d;
    GemmP p = gemm_basic(Zop, d, Wop(h, std::string("decoder_embed_dict.") + KEYN[k] + ".weight", dt), d, M, d, d, nullptr);
    p.amap = amap;
    p.cmap = cmap;
    p.rowtab = table ? table : h->Edec[k];
    p.rt_mod = mod;
    p.rt_ld = d;
    gemm_out(p, DT_F32, Yout, d);
    return p;
}
void dec_embed(m3pc_handle* h, int k, const void* Zop, RowMap amap, float* Yout, RowMap cmap, int M, int mod, int dt,
               hipStream_t st, const float* table) {
    gemm(h, dec_embed_p(h, k, Zop, amap, Yout, cmap, M, mod, dt, table), dt, st);
}

// Full (un-pruned) decoder on `batch` sequences: Z (4T rows each, operand dtype) -> Y (fp32) after all layers.
int run_decoder_full(m3pc_handle* h, const void* Zop, int batch, int dt, hipStream_t st) {
    const int T = h->T, d = h->d;
    bool grouped = false;
    if (dt == DT_F32 && !pass_switches().no_group && h->allow_splitk) {  // few-row fp32 pass: the four modality GEMMs as one launch
        GemmP ps[4];
        for (int k = 0; k < 4; ++k) {
            RowMap m{T, 4 * T, k * T};
            ps[k] = dec_embed_p(h, k, Zop, m, h->Y, m, batch * T, T, dt, nullptr);
        }
        GemmTimer t(h, st, 4 * 2.0 * batch * T * (double)d * d, dt);
        grouped = launch_gemm_f32_direct_group(ps, 4, st);
    }
    for (int k = 0; k < 4 && !grouped; ++k) {
        RowMap m{T, 4 * T, k * T};
        dec_embed(h, k, Zop, m, h->Y, m, batch * T, T, dt, st);
    }
    for (int i = 0; i < h->dm.n_dec_layer; ++i) {
        const std::string pfx = "decoder.layers." + std::to_string(i);
        PieceState ps{false, false};  // every layer runs its own norm1 and Q|K|V
        CHK(run_block(h, BlockArgs{pfx, h->Y, batch, 4 * T}, dt, st, ps));
    }
    return check_launch("decoder");
}

// Output head of key k (not actions) on `rows` logical rows of Ysrc selected by xmap:
// decoder.norm -> head LN -> Linear+GELU -> Linear(D_k) [-> de-tokenize]
int run_head(m3pc_handle* h, int k, const float* Ysrc, RowMap xmap, int rows, float* out, int ldy, bool detok, int dt,
             hipStream_t st) {
    const std::string kn = KEYN[k];
    LnP ln = ln_rows(h, Ysrc, rows, W(h, "decoder.norm.weight").f, W(h, "decoder.norm.bias").f, h->Hn, dt);
    ln.xmap = xmap;
    ln.g2 = W(h, "output_head_dict." + kn + ".0.weight").f;
    ln.b2 = W(h, "output_head_dict." + kn + ".0.bias").f;
    launch_layernorm(ln, st);
    return run_head_tail(h, k, h->Hn, rows, out, ldy, detok, dt, st);
}

// ... from the head's LayerNorm output (rows, d) in the operand dtype on: Linear+GELU -> Linear(D_k) [-> de-tokenize]
int run_head_tail(m3pc_handle* h, int k, const void* ln_rows, int rows, float* out, int ldy, bool detok, int dt, hipStream_t st) {
    const int d = h->d;
    const std::string kn = KEYN[k];
    GemmP p = gemm_basic(ln_rows, d, Wop(h, "output_head_dict." + kn + ".1.weight", dt), d, rows, d, d,
                         W(h, "output_head_dict." + kn + ".1.bias").f);
    p.gelu = 1;
    // many-row bf16 passes: the gelu'd hidden rows cross HBM in bf16 and the last Linear runs on the matrix cores (round 6)
    // (chosen by the size of the WHOLE step, never by a shard's rows: sharded scores stay bit-identical to the unsharded ones)
    const long long step_rows = (long long)((double)rows * h->pass_scale + 0.5);
    const bool hb = dt == DT_BF16 && !pass_switches().no_head_out_mfma &&
                    head_out_mfma_covers((int)(step_rows < 0x7fffffff ? step_rows : 0x7fffffff), d, h->feat[k]);
    gemm_out(p, hb ? DT_BF16 : DT_F32, h->G, d);
    gemm(h, p, dt, st);
    HeadOutP ho{};
    if (hb) ho.Xb = (const bf16_t*)h->G;
    else ho.X = h->G;
    ho.ldx = d;
    ho.rows = rows;
    ho.d = d;
    ho.D = h->feat[k];
    ho.W = W(h, "output_head_dict." + kn + ".3.weight").f;
    ho.b = W(h, "output_head_dict." + kn + ".3.bias").f;
    if (detok && h->tok_norm[k]) {
        ho.mean = h->tok_mean[k];
        ho.stdv = h->tok_std[k];
    }
    ho.Y = out;
    ho.ldy = ldy;
    launch_head_out(ho, st);
    return check_launch("head");
}

// Generic forward on `batch` sequences; outputs raw head values (no de-tokenization)
int forward_impl(m3pc_handle* h, Plan* pl, const TokIn& in, int batch, float* out_states, float* out_rewards,
                 float* out_returns, float* out_mu, float* out_std, int dt, hipStream_t st) {
    const int T = h->T, d = h->d;
    if ((long long)batch * 4 * T > h->R) return fail(M3PC_ENOMEM, "batch %d exceeds workspace (max_batch=%d)", batch, h->dm.max_batch);
    CHK(run_encoder(h, pl, in, batch, dt, st));
    GatherP g = gather_basic(h, h->EncOut, pl->Le, h->mask_tokens, pl->d_dec_rowsrc, 4 * T, batch);
    if (dt == DT_BF16)
        g.outb = (bf16_t*)h->Z;
    else
        g.out = (float*)h->Z;
    launch_gather_rows(g, st);
    CHK(run_decoder_full(h, h->Z, batch, dt, st));
    float* outs[4] = {out_states, nullptr, out_rewards, out_returns};
    for (int k = 0; k < 4; ++k) {
        if (k == M3PC_ACTIONS || !outs[k]) continue;
        RowMap m{T, 4 * T, k * T};
        CHK(run_head(h, k, h->Y, m, batch * T, outs[k], h->feat[k], false, dt, st));
    }
    if (out_mu && out_std) {
        // decoder.norm of the action rows, then the actor head: one launch when the head kernel can normalise its rows itself
        const bool fuse = actor_head_fuses_ln(d, h->A);
        const RowMap am{T, 4 * T, M3PC_ACTIONS * T};
        const float* ng = W(h, "decoder.norm.weight").f;
        const float* nb = W(h, "decoder.norm.bias").f;
        if (!fuse) {
            LnP ln = ln_rows(h, h->Y, batch * T, ng, nb, h->G, DT_F32);
            ln.xmap = am;
            launch_layernorm(ln, st);
        }
        ActorP a{};
        a.X = fuse ? h->Y : h->G;
        a.ldx = d;
        if (fuse) {
            a.xmap = am;
            a.ln_g = ng;
            a.ln_b = nb;
        }
        a.rows = batch * T;
        a.d = d;
        a.A = h->A;
        a.Wmu = W(h, "output_head_dict.actions.mu.weight").f;
        a.bmu = W(h, "output_head_dict.actions.mu.bias").f;
        a.Wls = W(h, "output_head_dict.actions.log_std.weight").f;
        a.bls = W(h, "output_head_dict.actions.log_std.bias").f;
        a.mu = out_mu;
        a.sd = out_std;
        launch_actor_head(a, st);
    }
    return check_launch("forward");
}


// ---------------------------------------------------------------------------------- pruned decoder
// The exactly pruned decoder (mtm_model.py:663-716 restricted to what the caller reads) behind an encoder pass over `n`
// sequences of plan `pl` (encoder output in Z [bf16] / EncOut [fp32]), stage by stage: decoder inputs and K|V of the un-masked
// tokens, the queries of set `q` (shared table rows when every query token is masked, per-sequence rows else), attention over
// own + masked keys, out-proj / FFN on the n * nq query rows, then
//   TAIL_HEADS: decoder.norm + the output head of each group's key -> h->pred[s] (n * grp, D_k) de-tokenised
//   TAIL_X:     the fp32 block output rows (n * nq, d) -> *xrows (the caller applies decoder.norm / the action head)
struct PrunedCtx {
    m3pc_handle* h;
    Plan* pl;
    Plan::Query& q;
    SharedTables& tb;
    int n, dt;
    hipStream_t st;
    int tail;
    const std::string pfx;  // the decoder layer
    const void* enc_op;     // encoder output rows in the operand dtype
    float* Y1;              // (n*nq, d) decoder residual of the query tokens (EncOut is dead: Z/Y hold its uses)
    const float* n1_g;      // the layer's norm1
    const float* n1_b;
    // Some query tokens un-masked, as a prefix (Query::nu): the fused decoder input still serves K|V, the nu per-sequence
    // query rows get their decoder inputs / Q projection from few-row GEMMs of their own, and the fused tail takes their
    // residual rows from behind the shared table (many-row bf16 passes only: the choice goes by the size of the whole step)
    bool kv_fusable, mixp;
    // the query stage's: where the attention finds its queries, where the tail its residual rows
    const void* Qp = nullptr;
    long long q_bstride = 0;
    int ldq = 0;
    TailRes res;
    // the tail stage's: what it left for the heads
    enum { HEADS_DONE, HEADS_LN_ROWS, HEADS_X } heads = HEADS_X;  // inside the tail / their LayerNorm rows in Hn / the block output in Y1

    LnP norm1(const float* X, int rows) const { return ln_rows(h, X, rows, n1_g, n1_b, h->Hn, dt); }
};

static void pruned_routes(PrunedCtx& c) {
    m3pc_handle* h = c.h;
    const PassSwitches& sw = pass_switches();
    const Plan* pl = c.pl;
    const int d = h->d, n = c.n, nq = c.q.nq;
    c.kv_fusable = c.dt == DT_BF16 && !sw.no_kv_fused && (double)n * pl->Le * h->pass_scale >= 512.0 && h->kvstream[0] &&
                   (pl->kept[0] || pl->kept[1]) && !pl->kept[2] && !pl->kept[3];
    c.mixp = c.kv_fusable && !c.q.all_masked && c.q.nu > 0 && !sw.no_mix_prefix && !sw.no_block_fused && h->wstream.count(c.pfx) &&
             (double)n * nq * h->pass_scale >= (double)FUSED_MIN_ROWS && (long long)nq + (long long)n * c.q.nu <= h->R &&
             // (the fused tail's own limits for this layout, block_fused_accepts(): 32-bit buffer offsets of the residual
             // table [shared rows | n nu per-sequence rows] and of the rows it writes -- decided HERE, before the pass is laid
             // out for that kernel, so that a pass it would refuse takes the generic per-sequence path instead of failing)
             (unsigned long long)(nq + (unsigned long long)n * c.q.nu) * d * 4 < 0xfffffff0ull &&
             (unsigned long long)n * nq * d * 4 < 0x80000000ull;
}

// decoder inputs (-> Y) and K|V (-> QKV) of the un-masked tokens
static void pruned_kv(PrunedCtx& c) {
    m3pc_handle* h = c.h;
    Plan* pl = c.pl;
    const int d = h->d, n = c.n, Le = pl->Le, dt = c.dt;
    if (c.kv_fusable && (c.q.all_masked || c.mixp)) {
        // embedding, norm1 and the K|V projection in one launch (kv_fused_kernel): the fp32 rows Y are consumed by nothing
        // else when every scored token is masked
        KvFusedP kp{};
        kp.Z = (const bf16_t*)h->Z;
        kp.ldz = d;
        int g = 0;
        for (int k = 0; k < 2; ++k) {
            if (!pl->kept[k]) continue;
            kp.M[g] = n * pl->kept[k];
            kp.map[g] = RowMap{pl->kept[k], Le, pl->enc_off[k]};
            kp.rowtab[g] = pl->edec_kept[k];
            kp.rt_mod[g] = pl->kept[k];
            kp.wstream[g] = h->kvstream[k];
            ++g;
        }
        kp.ln_g = c.n1_g;
        kp.ln_b = c.n1_b;
        kp.bkv = W(h, c.pfx + ".self_attn.in_proj_bias").f + d;
        kp.KV = (bf16_t*)h->QKV;
        kp.ldkv = 2 * d;
        kp.kv_bytes = (unsigned)((size_t)n * Le * 2 * d * 2);
        GemmTimer t(h, c.st, 2.0 * n * Le * (3.0 * d * d), dt, 2);
        if (launch_kv_fused(kp, c.st)) return;
    }
    // few-row fp32 pass (re-score, pruned policy pass): the decoder-embedding GEMMs of the kept keys as ONE launch
    bool grouped = false;
    int nk = 0;
    GemmP ps[4];
    for (int k = 0; k < 4; ++k) {
        if (!pl->kept[k]) continue;
        RowMap mm{pl->kept[k], Le, pl->enc_off[k]};
        ps[nk++] = dec_embed_p(h, k, c.enc_op, mm, h->Y, mm, n * pl->kept[k], pl->kept[k], dt, pl->edec_kept[k]);
    }
    if (dt == DT_F32 && !pass_switches().no_group && h->allow_splitk && nk >= 2) {
        GemmTimer t(h, c.st, 2.0 * n * Le * (double)d * d, dt);
        grouped = launch_gemm_f32_direct_group(ps, nk, c.st);
    }
    for (int k = 0; k < nk && !grouped; ++k) gemm(h, ps[k], dt, c.st);
    // K|V of the un-masked tokens: in_proj rows [d, 3d); norm1 rides on the operand load in the few-row fp32 pass
    const char* wkv = (const char*)Wop(h, c.pfx + ".self_attn.in_proj_weight", dt) + (size_t)d * d * dtype_size(dt);
    GemmP p = gemm_basic(h->Hn, d, wkv, d, n * Le, 2 * d, d, W(h, c.pfx + ".self_attn.in_proj_bias").f + d);
    gemm_out(p, dt, h->QKV, 2 * d);
    GemmP t = p;
    t.A = h->Y;
    t.a_ln_g = c.n1_g;
    t.a_ln_b = c.n1_b;
    if (can_fold_ln(h, t, dt))
        p = t;
    else
        launch_layernorm(c.norm1(h->Y, n * Le), c.st);
    gemm(h, p, dt, c.st);
}

// norm1 + the Q rows of in_proj of `rows` per-sequence residual rows X -> qbuf (behind K|V in the same buffer)
static void pruned_q_proj(PrunedCtx& c, const float* X, int rows, int rows_per_seq) {
    m3pc_handle* h = c.h;
    const int d = h->d;
    char* qbuf = (char*)h->QKV + (size_t)c.n * c.pl->Le * 2 * d * dtype_size(c.dt);
    launch_layernorm(c.norm1(X, rows), c.st);
    GemmP p = gemm_basic(h->Hn, d, Wop(h, c.pfx + ".self_attn.in_proj_weight", c.dt), d, rows, d, d, W(h, c.pfx + ".self_attn.in_proj_bias").f);
    gemm_out(p, c.dt, qbuf, d);
    gemm(h, p, c.dt, c.st);
    c.Qp = qbuf;
    c.q_bstride = (long long)rows_per_seq * d;
    c.ldq = d;
}

// the queries and the residual rows of their tail, in three forms
static int pruned_queries(PrunedCtx& c) {
    m3pc_handle* h = c.h;
    const int d = h->d, n = c.n, nq = c.q.nq, Le = c.pl->Le;
    if (c.mixp) {
        // [shared residual table (nq rows)] [per-sequence residual rows of the nu un-masked queries (n nu)]
        const int nu = c.q.nu, kq = c.q.nu_key;
        float* Rcomb = h->X;  // (the encoder residual stream is dead by now)
        float* Yu = Rcomb + (size_t)nq * d;
        HIPCHK(hipMemcpyAsync(Rcomb, c.tb.Yq, (size_t)nq * d * sizeof(float), hipMemcpyDeviceToDevice, c.st));
        // decoder inputs of the nu query tokens of every sequence: Z rows nu_enc0 .. of the sequence, the key's embedding
        RowMap am{nu, Le, c.q.nu_enc0};
        dec_embed(h, kq, c.enc_op, am, Yu, rowmap_identity(), n * nu, nu, c.dt, c.st, c.pl->edec_kept[kq] + (size_t)c.q.nu_kept0 * d);
        pruned_q_proj(c, Yu, n * nu, nu);
        c.res.table = Rcomb;
        c.res.mod = nq;
        c.res.nu = nu;
    } else if (c.q.all_masked) {
        c.Qp = c.tb.QKVq;
        c.q_bstride = 0;
        c.ldq = 3 * d;
        c.res.table = c.tb.Yq;
        c.res.mod = nq;
    } else {
        float* Yq_rows = h->X;  // per-candidate residual rows (n*nq, d); the encoder residual stream is dead by now
        GatherP g = gather_basic(h, h->Y, Le, c.tb.Yall, c.q.d_q_rowsrc_mix, nq, n);
        g.out = Yq_rows;
        launch_gather_rows(g, c.st);
        pruned_q_proj(c, Yq_rows, n * nq, nq);
        c.res.rows = Yq_rows;
    }
    return 0;
}

static void pruned_attention(const PrunedCtx& c) {
    m3pc_handle* h = c.h;
    const Plan::Query& q = c.q;
    const SharedTables& tb = c.tb;
    const int d = h->d, nq = q.nq, Le = c.pl->Le;
    const size_t es = dtype_size(c.dt);
    const char* kvu = (const char*)h->QKV;
    AttnP at = attn_basic(h, c.n, nq);
    at.Q = c.Qp;
    at.q_bstride = c.q_bstride;
    at.ldq = c.ldq;
    at.K1 = kvu;
    at.V1 = kvu + (size_t)d * es;
    at.kv1_bstride = (long long)Le * 2 * d;
    at.ldkv1 = 2 * d;
    at.L1 = Le;
    at.K2 = (const char*)tb.QKVm + (size_t)d * es;
    at.V2 = (const char*)tb.QKVm + (size_t)2 * d * es;
    at.ldkv2 = 3 * d;
    at.L2 = c.pl->Lm;
    at.Lq = nq;
    if (c.mixp) {  // queries [0, nu) per sequence, the others from the shared table behind them
        at.Lq = q.nu;
        at.orow1 = 0;
        if (nq > q.nu) {
            at.Q2 = (const char*)tb.QKVq + (size_t)q.nu * 3 * d * es;
            at.ldq2 = 3 * d;
            at.Lq2 = nq - q.nu;
            at.orow2 = q.nu;
        }
    }
    if (c.dt == DT_BF16 && q.all_masked && tb.pre_m) {
        // the masked tokens' keys meet the same (shared) queries for every candidate: that block of the softmax
        // was reduced when the tables were built, only the candidate's own Le keys are visited here
        at.K2 = at.V2 = nullptr;
        at.L2 = 0;
        at.pre_m = tb.pre_m;
        at.pre_l = tb.pre_l;
        at.pre_O = tb.pre_O;
    }
    launch_attention(at, c.dt, c.st);
}

// out-proj, norm2 and FFN of the query rows -> Y1, or straight on to the heads' LayerNorm rows / the heads themselves (c.heads)
static int pruned_tail(PrunedCtx& c) {
    m3pc_handle* h = c.h;
    const Plan::Query& q = c.q;
    const int d = h->d, rows = c.n * q.nq;
    const bool want_heads = c.tail == TAIL_HEADS;
    const TailForm form = tail_form(h, c.pfx, rows, c.dt);
    if (form != TAIL_CHAIN) {
        // decoder.norm and the two heads' LayerNorms inside the launch (or on the split form's reduce): the rows of head s land in
        // the s-th block of n*grp rows of Hn
        BlockP b{};
        if (want_heads) {
            b.lnA_g = W(h, "decoder.norm.weight").f;
            b.lnA_b = W(h, "decoder.norm.bias").f;
            for (int s = 0; s < 2; ++s) {  // (one group: LN_B[0] for every row; the kernel's tables still hold two)
                const int ks = q.qkeys[s < q.n_groups ? s : 0];
                b.lnB_g[s] = W(h, std::string("output_head_dict.") + KEYN[ks] + ".0.weight").f;
                b.lnB_b[s] = W(h, std::string("output_head_dict.") + KEYN[ks] + ".0.bias").f;
            }
            if (q.n_groups == 2) {
                b.out_mod = q.nq;
                b.out_grp = q.grp;
            }
        }
        // both scored keys have scalar heads (rtg_guiding: rewards, returns): the heads run inside the full tail, on workgroups
        // that each own rows of one key; else the heads' LayerNorm rows go to Hn and the heads are launches of their own
        const bool fuse_heads = want_heads && q.n_groups == 2 && form == TAIL_FULL && !pass_switches().no_head_fused &&
                                q.qkeys[0] == M3PC_REWARDS && q.qkeys[1] == M3PC_RETURNS && h->feat[M3PC_REWARDS] == 1 &&
                                h->feat[M3PC_RETURNS] == 1;
        if (fuse_heads) {
            for (int s = 0; s < 2; ++s) {
                const std::string hp = std::string("output_head_dict.") + KEYN[q.qkeys[s]];
                b.head_out[s] = h->pred[s];
                b.hb1[s] = W(h, hp + ".1.bias").f;
                b.hw2[s] = W(h, hp + ".3.weight").f;
                b.hb2[s] = W(h, hp + ".3.bias").f;
                if (h->tok_norm[q.qkeys[s]]) {
                    b.hmean[s] = h->tok_mean[q.qkeys[s]];
                    b.hstd[s] = h->tok_std[q.qkeys[s]];
                }
            }
        } else if (want_heads) {
            b.Hout = (bf16_t*)h->Hn;
            b.ldh = d;
        } else {
            b.Xout = c.Y1;
            b.ldx = d;
        }
        if (fused_tail(h, c.pfx, rows, c.dt, c.st, form, c.res, b, fuse_heads ? (double)d * d : 0.0)) {
            c.heads = fuse_heads || !want_heads ? PrunedCtx::HEADS_DONE : PrunedCtx::HEADS_LN_ROWS;
            return 0;
        }
    }
    if (c.mixp) return fail(M3PC_EINVAL, "pruned_decoder: the fused layer tail did not take a pass set up for it");
    chain_tail(h, c.pfx, rows, c.dt, c.st, c.res, c.Y1, nullptr);
    c.heads = want_heads ? PrunedCtx::HEADS_X : PrunedCtx::HEADS_DONE;
    return 0;
}

// few-row fp32 pass with scalar heads only (the re-score of an rtg_guiding step): both heads on the block output in ONE launch
static bool pruned_scalar_heads(PrunedCtx& c) {
    m3pc_handle* h = c.h;
    const Plan::Query& q = c.q;
    const int d = h->d, n = c.n, hh = q.grp;
    bool scalar = c.dt == DT_F32 && h->allow_splitk && !pass_switches().no_head_f32_fused && h->cur && h->cur->head_part &&
                  n * hh <= h->cur->head_rows && q.n_groups >= 1 && q.n_groups <= 2;
    for (int s = 0; s < q.n_groups && scalar; ++s) scalar = h->feat[q.qkeys[s]] == 1 && q.qkeys[s] != M3PC_ACTIONS;
    if (!scalar) return false;
    HeadFusedP hp{};
    hp.X = c.Y1;
    hp.ldx = d;
    hp.rows = n * hh;
    hp.d = d;
    hp.n_heads = q.n_groups;
    hp.grp = hh;
    hp.row_mod = q.nq;
    hp.gA = W(h, "decoder.norm.weight").f;
    hp.bA = W(h, "decoder.norm.bias").f;
    for (int s = 0; s < q.n_groups; ++s) {
        const std::string hn = std::string("output_head_dict.") + KEYN[q.qkeys[s]];
        hp.gB[s] = W(h, hn + ".0.weight").f;
        hp.bB[s] = W(h, hn + ".0.bias").f;
        hp.W1[s] = W(h, hn + ".1.weight").f;
        hp.b1[s] = W(h, hn + ".1.bias").f;
        hp.w2[s] = W(h, hn + ".3.weight").f;
        hp.b2[s] = W(h, hn + ".3.bias").f;
        if (h->tok_norm[q.qkeys[s]]) {
            hp.mean[s] = h->tok_mean[q.qkeys[s]];
            hp.stdv[s] = h->tok_std[q.qkeys[s]];
        }
        hp.out[s] = h->pred[s];
    }
    hp.part = h->cur->head_part;
    hp.ticket = h->cur->head_ticket;
    GemmTimer t(h, c.st, q.n_groups * 2.0 * n * hh * (double)d * d, c.dt);
    return launch_head_f32_fused(hp, c.st);
}

// heads of the scored keys -> pred[s] (n*grp, D_k), de-tokenized
static int pruned_heads(PrunedCtx& c) {
    m3pc_handle* h = c.h;
    const Plan::Query& q = c.q;
    const int d = h->d, n = c.n, hh = q.grp;
    if (c.heads == PrunedCtx::HEADS_DONE || (c.heads == PrunedCtx::HEADS_X && pruned_scalar_heads(c))) return 0;
    for (int s = 0; s < q.n_groups; ++s) {
        const int k = q.qkeys[s];
        if (c.heads == PrunedCtx::HEADS_LN_ROWS)
            CHK(run_head_tail(h, k, (const char*)h->Hn + (size_t)s * n * hh * d * dtype_size(c.dt), n * hh, h->pred[s], h->feat[k], true,
                              c.dt, c.st));
        else
            CHK(run_head(h, k, c.Y1, RowMap{hh, q.nq, s * hh}, n * hh, h->pred[s], h->feat[k], true, c.dt, c.st));
    }
    return 0;
}

static int pruned_stages(PrunedCtx& c) {
    pruned_routes(c);
    pruned_kv(c);
    CHK(pruned_queries(c));
    pruned_attention(c);
    CHK(pruned_tail(c));
    return pruned_heads(c);
}

int pruned_decoder(m3pc_handle* h, Plan* pl, Plan::Query& q, SharedTables& tb, int n, int dt, hipStream_t st, int tail,
                   float** xrows) {
    CHK(ensure_edec(h, pl, st));
    const std::string pfx = "decoder.layers.0";
    PrunedCtx c{h, pl, q, tb, n, dt, st, tail, pfx, dt == DT_BF16 ? h->Z : (const void*)h->EncOut, h->EncOut,
                W(h, pfx + ".norm1.weight").f, W(h, pfx + ".norm1.bias").f};
    if (xrows) *xrows = c.Y1;
    int rc = pruned_stages(c);
    if (rc == 0) rc = check_launch("pruned_decoder");
    if (rc != 0 && h->cur && h->cur->head_ticket)  // (an error behind the fused heads' launch: no count may survive in its tickets)
        (void)hipMemsetAsync(h->cur->head_ticket, 0, (size_t)2 * ((h->cur->head_rows + 31) / 32) * sizeof(int), st);
    return rc;
}

// ---------------------------------------------------------------------------------- candidate pass
// widx (optional, device (n,)): candidate c belongs to history window widx[c] of states (., T, S) / rewards (., T, 1);
// without it all candidates share window 0 and the history tokens are computed once (first-layer sharing).
// stage_from / stage_to / ln_state: the pass can be enqueued in pieces -- stage k < n_enc_layer is encoder layer k (the
// embedding goes with stage 0), stage n_enc_layer everything behind the encoder -- so that the pieces of two candidate halves
// can be enqueued alternately (m3pc_plan_step)
int candidate_pass(m3pc_handle* h, const m3pc_plan_args* a, const float* states, const float* rewards, int n,
                   const float* sample_actions, float* expect_return, float* pred_rewards, float* pred_boot, int dt,
                   hipStream_t st, const int* widx, int stage_from, int stage_to, PieceState* ln_state) {
    const int T = h->T, d = h->d, hh = a->horizon, idx = T - hh;
    const size_t es = dtype_size(dt);
    struct ScaleScope {
        m3pc_handle* h;
        ~ScaleScope() { h->pass_scale = 1.0; }
    } scale_scope{h};
    h->pass_scale = !widx && a->n_total > n ? (double)a->n_total / (double)n : 1.0;
    Plan* pl = nullptr;
    CHK(get_mask_plan(h, 1, idx, &pl));  // fd mask (finetune_omtm/masks.py:30-44)
    const int qi = a->mode == M3PC_MODE_RTG ? 0 : 1;
    CHK(build_query(h, pl, qi, hh));
    CHK(build_tables(h, pl, qi, dt, st));
    Plan::Query& q = pl->query[qi];
    SharedTables& tb = q.tab[dt];
    const int Le = pl->Le, nq = q.nq;
    if ((long long)n * Le > h->R || (long long)n * nq > h->R) return fail(M3PC_ENOMEM, "n_count %d exceeds workspace", n);

    TokIn in{};
    in.ptr[M3PC_STATES] = states;
    in.normalize[M3PC_STATES] = h->tok_norm[M3PC_STATES];
    in.ptr[M3PC_ACTIONS] = h->cand;
    in.bstride[M3PC_ACTIONS] = (long long)T * h->A;
    in.normalize[M3PC_ACTIONS] = h->tok_norm[M3PC_ACTIONS];
    in.ptr[M3PC_REWARDS] = rewards;
    in.ptr[M3PC_RETURNS] = h->rtok;
    in.widx = widx;
    in.wstride[M3PC_STATES] = (long long)T * h->S;
    in.wstride[M3PC_REWARDS] = T;
    // encoder order is states 0..idx, actions 0..T-1: everything before actions[idx] is history, shared by all candidates
    // of one window
    const int nl_enc = h->dm.n_enc_layer;
    if (stage_from < nl_enc) CHK(run_encoder(h, pl, in, n, dt, st, dt == DT_BF16, widx ? 0 : (idx + 1) + idx, stage_from, stage_to, ln_state));
    if (stage_to <= nl_enc) return check_launch("candidate_pass");

    CHK(pruned_decoder(h, pl, q, tb, n, dt, st, TAIL_HEADS, nullptr));
    const float* rw;
    const float* boot;
    float boot_scale;
    if (a->mode == M3PC_MODE_RTG) {
        rw = h->pred[0];
        boot = h->pred[1];
        boot_scale = 1000.0f;  // learner.py:305
    } else {
        if (!h->critic_set) return fail(M3PC_ESTATE, "critic weights not set");
        CriticP c{};
        c.states = h->pred[0];
        c.actions = sample_actions;
        c.rows = n * hh;
        c.S = h->S;
        c.A = h->A;
        c.hidden = h->dm.critic_hidden;
        c.om = h->c_om;
        c.os = h->c_os;
        for (int i = 0; i < 2; ++i) {
            c.W1T[i] = h->cW1T[i];
            c.b1[i] = h->cb1[i];
            c.W2T[i] = h->cW2T[i];
            c.b2[i] = h->cb2[i];
            c.W3[i] = h->cW3[i];
            c.b3[i] = h->cb3[i];
            c.W1F[i] = h->cW1F[i];
            c.W2F[i] = h->cW2F[i];
        }
        c.q = h->qv;
        launch_critic(c, st);
        rw = h->pred[1];
        boot = h->qv;
        boot_scale = 1.0f;
    }
    ScoreP sc{};
    sc.rewards = rw;
    sc.boot = boot;
    sc.n = n;
    sc.h = hh;
    sc.boot_scale = boot_scale;
    sc.gamma = (float)a->discount;
    sc.lmbda = a->lmbda;
    sc.expect_return = expect_return;
    sc.boot_out = pred_boot;
    sc.scatter_index = h->score_scatter_index;  // (m3pc_rescore_listed: the scores also go straight to their candidates' slots)
    sc.scatter_out = h->score_scatter_out;
    launch_score(sc, st);
    if (pred_rewards) HIPCHK(hipMemcpyAsync(pred_rewards, rw, (size_t)n * hh * sizeof(float), hipMemcpyDeviceToDevice, st));
    return check_launch("candidate_pass");
}


}  // namespace m3pc
