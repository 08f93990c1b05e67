// libm3pc_hip.so -- host side of the C ABI declared in include/m3pc_hip.h.
//
// Data layout in HBM (one handle = one GPU):
//   weights   fp32 arena in state_dict layout + bf16 copies of every GEMM weight ([N][K], K contiguous)
//   tables    per key: transposed encoder-embed weight (D_k,d); E_enc/E_dec (T,d) = bias + per-dim + pos
//   plans     per mask pattern: token maps, and -- for the candidate pass -- the candidate-independent
//             part of the decoder (inputs, K/V and Q of every masked token), computed once per weight load
//   workspace activations for R = max(max_candidates*2T, max_batch*4T) token rows:
//             X, Y (fp32 residual streams), Hn, QKV, O, F (operand dtype), EncOut (fp32)
//
// Candidate pass ("pass 2", learner.py:288-293) is exactly pruned: decoder rows of masked tokens do not
// depend on the candidate, so only the 2h scored tokens are pushed through out-proj/FFN/heads and only the
// un-masked tokens through the K/V projection.
#include <atomic>
#include <chrono>

#include "m3pc_internal.h"

namespace m3pc {
thread_local char g_err[512] = "";
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace m3pc

namespace {

int find_tensor(const m3pc_named_tensor* list, int n, const std::string& name) {
    for (int i = 0; i < n; ++i)
        if (list[i].name && name == list[i].name) return i;
    return -1;
}


}  // namespace


// =====================================================================================================
static int fill_rtok(m3pc_handle* h, const double* rtg, int n_windows, hipStream_t st);

// the library is built with -fvisibility=hidden: the C ABI below (include/m3pc_hip.h, and in the lab build m3pc_hip_debug.h) is
// everything it exports
#pragma GCC visibility push(default)
extern "C" {

const char* m3pc_last_error(void) { return g_err; }
int m3pc_abi_version(void) { return M3PC_ABI_VERSION; }

int m3pc_create(const m3pc_dims* dims, int device, m3pc_handle** out) {
    if (!dims || !out) return fail(M3PC_EINVAL, "null argument");
    const m3pc_dims& D = *dims;
    if (D.n_embd % 64 || D.n_embd > 1024 || D.n_head <= 0 || D.n_embd % D.n_head)
        return fail(M3PC_EINVAL, "n_embd must be a multiple of 64 (<=1024) and divisible by n_head");
    const int hd = D.n_embd / D.n_head;
    if (hd != 32 && hd != 64 && hd != 128) return fail(M3PC_EINVAL, "head_dim %d unsupported (32, 64, 128)", hd);
    if (D.state_dim < 1 || D.state_dim > 32 || D.action_dim < 1 || D.action_dim > 32)
        return fail(M3PC_EINVAL, "state_dim/action_dim must be in [1,32]");
    if (D.traj_length < 1 || D.traj_length > 64) return fail(M3PC_EINVAL, "traj_length must be in [1,64]");
    if (D.n_dec_layer != 1) return fail(M3PC_EINVAL, "n_dec_layer must be 1 (every shipped m3pc config)");
    if (D.n_enc_layer < 1 || D.max_candidates < 1 || D.max_batch < 1) return fail(M3PC_EINVAL, "bad sizes");
    if (D.critic_hidden < 0 || D.critic_hidden > 256) return fail(M3PC_EINVAL, "critic_hidden must be <= 256");
    if (D.max_goal_batch < 0) return fail(M3PC_EINVAL, "max_goal_batch must be >= 0");
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<m3pc_handle> h(new m3pc_handle());
    h->dm = D;
    h->device = device;
    h->d = D.n_embd;
    h->nh = D.n_head;
    h->hd = hd;
    h->T = D.traj_length;
    h->S = D.state_dim;
    h->A = D.action_dim;
    h->ff = 4 * D.n_embd;
    h->feat[0] = D.state_dim;
    h->feat[1] = D.action_dim;
    h->feat[2] = 1;
    h->feat[3] = 1;
    declare_weights(h.get());
    for (auto& kv : h->w) {
        CHK(dmalloc(&kv.second.f, (size_t)kv.second.numel));
        if (kv.second.gemm) {
            CHK(dmalloc(&kv.second.b, 2 * (size_t)kv.second.numel));  // hi | lo (Tensor::b)
            h->gemm_w.push_back({kv.second.f, &kv.second});
        }
    }
    std::sort(h->gemm_w.begin(), h->gemm_w.end());
    const int d = h->d, T = h->T;
    for (int k = 0; k < 4; ++k) {
        CHK(dmalloc(&h->WT[k], (size_t)h->feat[k] * d));
        CHK(dmalloc(&h->Eenc[k], (size_t)T * d));
        CHK(dmalloc(&h->Edec[k], (size_t)T * d));
        CHK(dmalloc(&h->tok_mean[k], 32));
        CHK(dmalloc(&h->tok_std[k], 32));
    }
    CHK(dmalloc(&h->mask_tokens, (size_t)4 * d));
    // candidate workspace: max_candidates candidates of 2T token rows (or max_batch generic forwards of 4T)
    {
        const long long r1 = (long long)D.max_candidates * 2 * T, r2 = (long long)D.max_batch * 4 * T;
        const long long r3 = (long long)D.max_goal_batch * 2 * T;  // (a goal window keeps at most 2T - 1 tokens, reads at most T)
        long long R = r1 > r2 ? r1 : r2;
        if (r3 > R) R = r3;
        if (R < 4 * T) R = 4 * T;
        CHK(alloc_ws(h.get(), h->base, R, D.max_candidates > D.max_goal_batch ? D.max_candidates : D.max_goal_batch, 64LL << 20));
        if (D.max_goal_batch > 0) CHK(dmalloc(&h->goal_ws, (size_t)D.max_goal_batch * T * h->S));
    }
    // chain workspaces: fp32 re-scores (<= max_rescore candidates) / policy passes (batch <= max_batch)
    {
        const int mr = D.max_rescore > 0 ? D.max_rescore : 64;
        long long R = (long long)mr * 2 * T;
        if (R < 4 * T) R = 4 * T;
        for (int par = 0; par < 2; ++par) {
            CHK(alloc_ws(h.get(), h->chain[par], R, mr, 32LL << 20));
            CHK(alloc_ws(h.get(), h->pchain[par], (long long)D.max_batch * 4 * T, 1, 32LL << 20));
        }
    }
    for (int s = 0; s < M3PC_SLOTS; ++s) {
        CHK(dmalloc(&h->slot[s].loc, (size_t)D.max_batch * T * h->A + 64));
        CHK(dmalloc(&h->slot[s].sd, (size_t)D.max_batch * T * h->A + 64));
        CHK(dmalloc(&h->slot[s].rtok, (size_t)D.max_batch * T));
    }
    CHK(dmalloc(&h->sel_scratch, 64));
    CHK(dmalloc(&h->d_topk, 1024));
    CHK(dmalloc(&h->er_top, 1024));
    CHK(dmalloc(&h->sa_buf, (size_t)(D.max_candidates > h->chain[0].max_cand ? D.max_candidates : h->chain[0].max_cand) * T * h->A));
    CHK(dmalloc(&h->sa_chain[0], (size_t)h->chain[0].max_cand * T * h->A));
    CHK(dmalloc(&h->sa_chain[1], (size_t)h->chain[0].max_cand * T * h->A));
    CHK(dmalloc(&h->refine_noise, (size_t)D.max_candidates * T * h->A));
    CHK(dmalloc(&h->refine_scores, (size_t)D.max_candidates));
    CHK(dmalloc(&h->refine_elites, (size_t)D.max_candidates));
    for (int s = 0; s < M3PC_SLOTS; ++s) {
        CHK(dmalloc(&h->cert_list[s], 64 + 1024));
        CHK(dmalloc(&h->cert_b[s], 64 + 1024));
        CHK(dmalloc(&h->cert_f[s], 64 + 1024));
        CHK(dmalloc(&h->cert_stats[s], 32));
        CHK(dmalloc(&h->cert_f32[s], (size_t)D.max_candidates));
        CHK(dmalloc(&h->cert_top1[s], 4));
    }
    HIPCHK(hipHostMalloc((void**)&h->cert_host, (size_t)M3PC_SLOTS * 8 * sizeof(float), hipHostMallocMapped | hipHostMallocCoherent));
    memset(h->cert_host, 0, (size_t)M3PC_SLOTS * 8 * sizeof(float));
    HIPCHK(hipHostGetDevicePointer((void**)&h->cert_host_dev, h->cert_host, 0));
    bind_ws(h.get(), &h->base);
    bind_slot(h.get(), 0);
    // ONE extra stream per device for all handles of the process: a process has four hardware queues, and with more
    // streams than that two of them share a queue and stop overlapping (a second planner must not cost the first its halves)
    {
        static std::map<int, hipStream_t> shared_aux;
        static std::mutex shared_aux_mutex;  // (handles of different threads may be created at the same time)
        std::lock_guard<std::mutex> lock(shared_aux_mutex);
        hipStream_t& sa = shared_aux[device];
#ifdef M3PC_LAB  // (tools/cu_mask_probe.py: the candidate passes' second stream confined to a CU mask, comma-separated hex words)
        if (!sa)
            if (const char* e = M3PC_ENV("M3PC_AUX_CU_MASK")) {
                std::vector<uint32_t> words;
                for (const char* q = e; *q;) {
                    words.push_back((uint32_t)strtoul(q, nullptr, 16));
                    while (*q && *q != ',') ++q;
                    if (*q == ',') ++q;
                }
                HIPCHK(hipExtStreamCreateWithCUMask(&sa, (uint32_t)words.size(), words.data()));
            }
#endif
        if (!sa) HIPCHK(hipStreamCreateWithFlags(&sa, hipStreamNonBlocking));
        h->aux = sa;
    }
    HIPCHK(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    for (int s = 0; s < M3PC_SLOTS; ++s)
        for (int i = 0; i < 3; ++i) HIPCHK(hipEventCreateWithFlags(&h->slot_join[s][i], hipEventDisableTiming));
    for (int i = 0; i < 3; ++i) HIPCHK(hipEventCreateWithFlags(&h->aux_tail[i], hipEventDisableTiming));
    if (const char* e = M3PC_ENV("M3PC_TWO_STREAM")) h->two_stream = atoi(e) != 0;
    h->auxs.push_back(h->aux);
    h->ev_joins.push_back(h->ev_join);
    // (lab: more than two candidate parts.  Streams are created only when asked for: a process has four hardware queues,
    // with more streams than that two of them share a queue and the halves no longer overlap)
    if (const char* e = M3PC_ENV("M3PC_STREAM_SPLIT")) {
        for (const char* q = e; *q;) {
            h->stream_split.push_back(atoi(q));
            while (*q && *q != ',') ++q;
            if (*q == ',') ++q;
        }
        for (size_t i = 1; i < h->stream_split.size() && i < 3; ++i) {
            hipStream_t s2;
            hipEvent_t e2;
            HIPCHK(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
            HIPCHK(hipEventCreateWithFlags(&e2, hipEventDisableTiming));
            h->auxs.push_back(s2);
            h->ev_joins.push_back(e2);
        }
    }
    if (D.critic_hidden > 0) {
        const int Hd = D.critic_hidden, SA = h->S + h->A;
        for (int i = 0; i < 2; ++i) {
            CHK(dmalloc(&h->cW1T[i], (size_t)SA * Hd));
            CHK(dmalloc(&h->cb1[i], Hd));
            CHK(dmalloc(&h->cW2T[i], (size_t)Hd * Hd));
            CHK(dmalloc(&h->cb2[i], Hd));
            CHK(dmalloc(&h->cW3[i], Hd));
            CHK(dmalloc(&h->cb3[i], 4));
            if (critic_mfma_covers(h->S, h->A, Hd)) {
                CHK(dmalloc(&h->cW1F[i], critic_w1f_floats(Hd)));
                CHK(dmalloc(&h->cW2F[i], critic_w2f_floats(Hd)));
            }
        }
        CHK(dmalloc(&h->c_om, 32));
        CHK(dmalloc(&h->c_os, 32));
    }
    *out = h.release();
    return 0;
}

int m3pc_destroy(m3pc_handle* h) {
    if (!h) return 0;
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    for (auto& kv : h->w) {
        hipFree(kv.second.f);
        if (kv.second.b) hipFree(kv.second.b);
    }
    for (int k = 0; k < 4; ++k) {
        hipFree(h->WT[k]);
        hipFree(h->Eenc[k]);
        hipFree(h->Edec[k]);
        hipFree(h->tok_mean[k]);
        hipFree(h->tok_std[k]);
    }
    hipFree(h->mask_tokens);
    free_ws(h->base);
    for (int par = 0; par < 2; ++par) {
        free_ws(h->chain[par]);
        free_ws(h->pchain[par]);
    }
    for (int s = 0; s < M3PC_SLOTS; ++s) {
        hipFree(h->slot[s].loc);
        hipFree(h->slot[s].sd);
        hipFree(h->slot[s].rtok);
    }
    void* bufs[] = {h->sel_scratch, h->d_topk, h->er_top, h->sa_buf, h->sa_chain[0], h->sa_chain[1], h->c_om, h->c_os, h->goal_ws,
                    h->refine_noise, h->refine_scores, h->refine_elites};
    for (int s = 0; s < M3PC_SLOTS; ++s) {
        void* cb[] = {h->cert_list[s], h->cert_b[s], h->cert_f[s], h->cert_stats[s], h->cert_f32[s], h->cert_top1[s]};
        for (void* b : cb)
            if (b) hipFree(b);
        for (int i = 0; i < 4; ++i)
            if (h->step_ev[s][i]) hipEventDestroy(h->step_ev[s][i]);
    }
    if (h->ev_excl) hipEventDestroy(h->ev_excl);
    if (h->step_chain_own)
        for (int i = 0; i < 2; ++i)
            if (h->step_chain[i]) hipStreamDestroy(h->step_chain[i]);
    if (h->cert_host) hipHostFree(h->cert_host);
    if (h->eval_host) hipHostFree(h->eval_host);
    {
        void* lb[] = {h->ls.list, h->ls.b, h->ls.f, h->ls.stats, h->ls.cand, h->ls.fs, h->ls.widx};
        for (void* b : lb)
            if (b) hipFree(b);
        if (h->ls.host) hipHostFree(h->ls.host);
    }
    for (size_t i = 1; i < h->auxs.size(); ++i) {
        hipStreamDestroy(h->auxs[i]);
        hipEventDestroy(h->ev_joins[i]);
    }
    for (int s = 0; s < M3PC_SLOTS; ++s)
        for (int i = 0; i < 3; ++i)
            if (h->slot_join[s][i]) hipEventDestroy(h->slot_join[s][i]);
    for (int i = 0; i < 3; ++i)
        if (h->aux_tail[i]) hipEventDestroy(h->aux_tail[i]);
    if (h->aux) hipStreamSynchronize(h->aux);  // (shared by the handles of the device: not destroyed)
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    if (h->ev_join) hipEventDestroy(h->ev_join);
    for (void* b : bufs)
        if (b) hipFree(b);
    for (int i = 0; i < 2; ++i) {
        void* cb[] = {h->cW1T[i], h->cb1[i], h->cW2T[i], h->cb2[i], h->cW3[i], h->cb3[i], h->cW1F[i], h->cW2F[i]};
        for (void* b : cb)
            if (b) hipFree(b);
    }
    for (auto& kv : h->plans) {
        Plan* pl = kv.second.get();
        hipFree(pl->d_tokmap);
        hipFree(pl->d_dec_rowsrc);
        hipFree(pl->d_masked_rowsrc);
        for (int k = 0; k < 4; ++k)
            if (pl->edec_own[k]) hipFree(pl->edec_own[k]);
        for (int q = 0; q < N_QUERY; ++q) {
            if (pl->query[q].d_q_rowsrc_tab) hipFree(pl->query[q].d_q_rowsrc_tab);
            if (pl->query[q].d_q_rowsrc_mix) hipFree(pl->query[q].d_q_rowsrc_mix);
            for (int pr = 0; pr < 2; ++pr) free_tables(pl->query[q].tab[pr]);
        }
    }
    for (auto& e : h->ev) {
        hipEventDestroy(e.a);
        hipEventDestroy(e.b);
    }
    for (int k = 0; k < 4; ++k)
        if (h->kvstream[k]) hipFree(h->kvstream[k]);
    for (auto& kv : h->wstream)
        if (kv.second) hipFree(kv.second);
    delete h;
    return 0;
}

int m3pc_load_weights(m3pc_handle* h, const m3pc_named_tensor* tensors, int n, void* stream) {
    if (!h || !tensors) return fail(M3PC_EINVAL, "null argument");
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(h->device));
    CHK(ws_sync(h, st));  // (deferred candidate parts still read the weights this call is about to replace)
    // The first call must bring every tensor; later calls may bring any subset (fine-tuning changes the weights between
    // rollouts, finetune.py:306): only what depends on a tensor that came is re-derived.
    const bool first = !h->weights_loaded;
    std::vector<std::string> dirty;
    for (auto& kv : h->w) {
        const int i = find_tensor(tensors, n, kv.first);
        if (i < 0) {
            if (first) return fail(M3PC_EINVAL, "state_dict is missing '%s'", kv.first.c_str());
            continue;
        }
        if (tensors[i].numel != kv.second.numel)
            return fail(M3PC_EINVAL, "'%s' has %lld elements, expected %lld", kv.first.c_str(), tensors[i].numel, kv.second.numel);
        HIPCHK(hipMemcpyAsync(kv.second.f, tensors[i].data, (size_t)kv.second.numel * sizeof(float),
                              tensors[i].on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        if (kv.second.gemm) launch_f32_split_bf16(kv.second.f, kv.second.b, kv.second.b + kv.second.numel, kv.second.numel, st);
        kv.second.loaded = true;
        dirty.push_back(kv.first);
    }
    auto is_dirty = [&](const std::string& name) {
        for (const std::string& d : dirty)
            if (d == name) return true;
        return false;
    };
    long long* ls = h->load_stats;
    ls[0] = (long long)dirty.size();
    ls[1] = ls[2] = ls[3] = 0;
    if (block_fused_supported(h->d, h->ff)) {  // fragment streams of the fused layer tails (block_fused.hip)
        // nxt: the layer whose Q|K|V projection rides behind this layer's tail (the next encoder layer), or ""
        auto pack = [&](const std::string& pfx, const std::string& nxt) -> int {
            const bool own = is_dirty(pfx + ".self_attn.out_proj.weight") || is_dirty(pfx + ".linear1.weight") || is_dirty(pfx + ".linear2.weight");
            const bool qkv = !nxt.empty() && is_dirty(nxt + ".self_attn.in_proj_weight");
            if (!own && !qkv) return 0;
            bf16_t*& ws = h->wstream[pfx];
            if (!ws) CHK(dmalloc((char**)&ws, block_stream_bytes()));
            if (own)
                launch_pack_block_stream(W(h, pfx + ".self_attn.out_proj.weight").b, W(h, pfx + ".linear1.weight").b,
                                         W(h, pfx + ".linear2.weight").b, ws, st);
            if (qkv) launch_pack_block_qkv(W(h, nxt + ".self_attn.in_proj_weight").b, ws, st);
            ++ls[1];
            return 0;
        };
        for (int i = 0; i < h->dm.n_enc_layer; ++i)
            CHK(pack("encoder.layers." + std::to_string(i), i + 1 < h->dm.n_enc_layer ? "encoder.layers." + std::to_string(i + 1) : ""));
        for (int i = 0; i < h->dm.n_dec_layer; ++i) CHK(pack("decoder.layers." + std::to_string(i), ""));
        // behind the decoder layer's own fragments: the first Linear of the two scalar output heads rtg_guiding scores
        // (rewards, returns: learner.py:294-305), consumed by the fused tail's head phases
        if (h->dm.n_dec_layer >= 1 && h->wstream.count("decoder.layers.0")) {
            const std::string w0 = std::string("output_head_dict.") + KEYN[M3PC_REWARDS] + ".1.weight";
            const std::string w1 = std::string("output_head_dict.") + KEYN[M3PC_RETURNS] + ".1.weight";
            if (is_dirty(w0) || is_dirty(w1)) {
                launch_pack_block_heads(W(h, w0).b, W(h, w1).b, h->wstream["decoder.layers.0"], st);
                ++ls[1];
            }
        }
        if (h->dm.n_dec_layer >= 1)
            for (int k = 0; k < 4; ++k) {
                const std::string we = std::string("decoder_embed_dict.") + KEYN[k] + ".weight";
                if (!(is_dirty(we) || is_dirty("decoder.layers.0.self_attn.in_proj_weight"))) continue;
                if (!h->kvstream[k]) CHK(dmalloc((char**)&h->kvstream[k], kv_stream_bytes()));
                launch_pack_kv_stream(W(h, we).b, W(h, "decoder.layers.0.self_attn.in_proj_weight").b + (size_t)h->d * h->d,
                                      h->kvstream[k], st);
                ++ls[2];
            }
    }
    // small derived tables, on the device: transposed encoder-embed weights, E_enc / E_dec = (bias + per-dim) + pos, mask tokens
    const int d = h->d, T = h->T;
    const bool pos_dirty = is_dirty("pos_embed");
    for (int k = 0; k < 4; ++k) {
        const std::string kn = KEYN[k];
        if (is_dirty("encoder_embed_dict." + kn + ".weight"))
            launch_transpose_f32(W(h, "encoder_embed_dict." + kn + ".weight").f, h->WT[k], d, h->feat[k], st);
        for (int pass = 0; pass < 2; ++pass) {
            const std::string side = pass == 0 ? "encoder" : "decoder";
            if (pos_dirty || is_dirty(side + "_embed_dict." + kn + ".bias") || is_dirty(side + "_per_dim_encoding." + kn))
                launch_embed_table(W(h, side + "_embed_dict." + kn + ".bias").f, W(h, side + "_per_dim_encoding." + kn).f,
                                   W(h, "pos_embed").f, pass == 0 ? h->Eenc[k] : h->Edec[k], T, d, st);
        }
        if (is_dirty("mask_token_dict." + kn))
            HIPCHK(hipMemcpyAsync(h->mask_tokens + (size_t)k * d, W(h, "mask_token_dict." + kn).f, d * sizeof(float),
                                  hipMemcpyDeviceToDevice, st));
    }
    // the candidate-independent decoder tables of every cached plan hang on the decoder side of the model
    bool dec_dirty = pos_dirty;
    for (const std::string& nme : dirty)
        if (nme.rfind("decoder", 0) == 0 || nme.rfind("mask_token_dict", 0) == 0) dec_dirty = true;
    if (dec_dirty) {
        invalidate_tables(h);
        ls[3] = 1;
    }
    for (int sl = 0; sl < M3PC_SLOTS; ++sl) {
        h->slot[sl].policy_valid = false;
        h->slot[sl].n_windows = 0;
    }
    HIPCHK(hipStreamSynchronize(st));  // the caller's tensors may go away when the call returns
    h->weights_loaded = true;
    return check_launch("load_weights");
}

int m3pc_load_stats(m3pc_handle* h, long long* out4) {
    if (!h || !out4) return fail(M3PC_EINVAL, "null argument");
    for (int i = 0; i < 4; ++i) out4[i] = h->load_stats[i];
    return 0;
}

int m3pc_set_tokenizer(m3pc_handle* h, int key, const float* mean, const float* std_, int dim, int normalize) {
    if (!h || key < 0 || key > 3 || !mean || !std_) return fail(M3PC_EINVAL, "bad argument");
    if (dim != h->feat[key]) return fail(M3PC_EINVAL, "tokenizer '%s' has dim %d, expected %d", KEYN[key], dim, h->feat[key]);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpy(h->tok_mean[key], mean, dim * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->tok_std[key], std_, dim * sizeof(float), hipMemcpyHostToDevice));
    h->h_mean[key].assign(mean, mean + dim);
    h->h_std[key].assign(std_, std_ + dim);
    h->tok_norm[key] = normalize ? 1 : 0;
    h->tok_set[key] = true;
    return 0;
}

int m3pc_set_critic(m3pc_handle* h, const m3pc_named_tensor* tensors, int n, const float* obs_mean, const float* obs_std,
                    void* stream) {
    if (!h || !tensors || !obs_mean || !obs_std) return fail(M3PC_EINVAL, "null argument");
    if (h->dm.critic_hidden <= 0) return fail(M3PC_EINVAL, "handle was created without a critic");
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(h->device));
    // device tensors are read after everything already queued on the caller's stream (an optimizer step that has just
    // updated qf, finetune.py:288-290): the blocking copies below are not ordered behind a non-blocking stream by themselves
    HIPCHK(hipStreamSynchronize(st));
    const int Hd = h->dm.critic_hidden, SA = h->S + h->A;
    auto fetch = [&](const std::string& name, long long numel, std::vector<float>& out) -> int {
        const int i = find_tensor(tensors, n, name);
        if (i < 0) return fail(M3PC_EINVAL, "critic state_dict is missing '%s'", name.c_str());
        if (tensors[i].numel != numel) return fail(M3PC_EINVAL, "'%s' has %lld elements, expected %lld", name.c_str(), tensors[i].numel, numel);
        out.resize((size_t)numel);
        HIPCHK(hipMemcpy(out.data(), tensors[i].data, (size_t)numel * sizeof(float),
                         tensors[i].on_device ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
        return 0;
    };
    for (int qn = 0; qn < 2; ++qn) {
        const std::string q = qn == 0 ? "q1" : "q2";
        std::vector<float> w1, b1, w2, b2, w3, b3;
        CHK(fetch(q + ".net.0.weight", (long long)Hd * SA, w1));
        CHK(fetch(q + ".net.0.bias", Hd, b1));
        CHK(fetch(q + ".net.2.weight", (long long)Hd * Hd, w2));
        CHK(fetch(q + ".net.2.bias", Hd, b2));
        CHK(fetch(q + ".net.4.weight", Hd, w3));
        CHK(fetch(q + ".net.4.bias", 1, b3));
        std::vector<float> w1t((size_t)SA * Hd), w2t((size_t)Hd * Hd);
        for (int c = 0; c < Hd; ++c)
            for (int f = 0; f < SA; ++f) w1t[(size_t)f * Hd + c] = w1[(size_t)c * SA + f];
        for (int c = 0; c < Hd; ++c)
            for (int k = 0; k < Hd; ++k) w2t[(size_t)k * Hd + c] = w2[(size_t)c * Hd + k];
        HIPCHK(hipMemcpy(h->cW1T[qn], w1t.data(), w1t.size() * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->cb1[qn], b1.data(), b1.size() * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->cW2T[qn], w2t.data(), w2t.size() * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->cb2[qn], b2.data(), b2.size() * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->cW3[qn], w3.data(), w3.size() * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->cb3[qn], b3.data(), sizeof(float), hipMemcpyHostToDevice));
        if (h->cW1F[qn]) {
            std::vector<float> w1f(critic_w1f_floats(Hd)), w2f(critic_w2f_floats(Hd));
            critic_pack(w1.data(), w2.data(), SA, Hd, w1f.data(), w2f.data());
            HIPCHK(hipMemcpy(h->cW1F[qn], w1f.data(), w1f.size() * sizeof(float), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(h->cW2F[qn], w2f.data(), w2f.size() * sizeof(float), hipMemcpyHostToDevice));
        }
    }
    HIPCHK(hipMemcpy(h->c_om, obs_mean, h->S * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->c_os, obs_std, h->S * sizeof(float), hipMemcpyHostToDevice));
    h->critic_set = true;
    return 0;
}

int m3pc_tokenize(m3pc_handle* h, int key, const void* in, int in_f64, float* out, long long rows, void* stream) {
    if (!h || key < 0 || key > 3 || !in || !out) return fail(M3PC_EINVAL, "bad argument");
    if (!h->tok_set[key]) return fail(M3PC_ESTATE, "tokenizer '%s' not set", KEYN[key]);
    HIPCHK(hipSetDevice(h->device));
    launch_tokenize(in, in_f64, out, rows, h->feat[key], h->tok_mean[key], h->tok_std[key], h->tok_norm[key], (hipStream_t)stream);
    return check_launch("tokenize");
}

int m3pc_detokenize(m3pc_handle* h, int key, const float* in, float* out, long long rows, void* stream) {
    if (!h || key < 0 || key > 3 || !in || !out) return fail(M3PC_EINVAL, "bad argument");
    if (!h->tok_set[key]) return fail(M3PC_ESTATE, "tokenizer '%s' not set", KEYN[key]);
    HIPCHK(hipSetDevice(h->device));
    launch_detokenize(in, out, rows, h->feat[key], h->tok_mean[key], h->tok_std[key], h->tok_norm[key], (hipStream_t)stream);
    return check_launch("detokenize");
}

int m3pc_forward(m3pc_handle* h, int batch, const float* const tokens[4], const unsigned char* const masks[4],
                 float* out_states, float* out_rewards, float* out_returns, float* out_mu, float* out_std, int precision,
                 void* stream) {
    if (!h || !tokens || !masks) return fail(M3PC_EINVAL, "null argument");
    if (!h->weights_loaded) return fail(M3PC_ESTATE, "weights not loaded");
    if (batch < 1 || batch > h->dm.max_batch) return fail(M3PC_EINVAL, "batch %d outside [1, max_batch=%d]", batch, h->dm.max_batch);
    if (!precision_ok(precision)) return fail(M3PC_EINVAL, "bad precision %d", precision);
    if ((out_mu == nullptr) != (out_std == nullptr)) return fail(M3PC_EINVAL, "out_mu and out_std go together");
    HIPCHK(hipSetDevice(h->device));
    Plan* pl = nullptr;
    CHK(get_plan(h, masks, &pl));
    TokIn in;
    memset(&in, 0, sizeof(in));
    for (int k = 0; k < 4; ++k) {
        if (pl->kept[k] && !tokens[k]) return fail(M3PC_EINVAL, "tokens[%s] is null but its mask keeps tokens", KEYN[k]);
        in.ptr[k] = tokens[k];
        in.bstride[k] = (long long)h->T * h->feat[k];
    }
    h->allow_splitk = true;
    CHK(ws_sync(h, (hipStream_t)stream));
    X3Scope x3(h, precision == M3PC_PREC_BF16X3);
    return forward_impl(h, pl, in, batch, out_states, out_rewards, out_returns, out_mu, out_std, pass_dt(precision),
                        (hipStream_t)stream);
}

// Zero-shot goal reaching, both forwards of action_piid_sample (zeroshot_omtm/learner.py:151-261) in one call on RAW windows:
// path inference under the pi mask -> the inferred observations over the window rows [0, idx] and [idx+2, T-2] (240-246) ->
// inverse dynamics under the fid mask -> the action distribution.  fp32, in the policy workspace.
int m3pc_goal_step(m3pc_handle* h, int batch, const float* states, const float* actions, const float* rewards, const double* rtg,
                   const unsigned char* const masks_pi[4], const unsigned char* const masks_fid[4], int idx, float* inferred,
                   float* window_states, float* out_mu, float* out_std, void* stream) {
    if (!h || !states || !actions || !rewards || !rtg || !masks_pi || !masks_fid || !inferred || !window_states || !out_mu || !out_std)
        return fail(M3PC_EINVAL, "null argument");
    if (!h->weights_loaded) return fail(M3PC_ESTATE, "weights not loaded");
    for (int k = 0; k < 4; ++k)
        if (!h->tok_set[k]) return fail(M3PC_ESTATE, "tokenizer '%s' not set", KEYN[k]);
    if (batch < 1 || batch > h->dm.max_batch) return fail(M3PC_EINVAL, "batch %d outside [1, max_batch=%d]", batch, h->dm.max_batch);
    const int T = h->T;
    if (idx < 0 || idx >= T) return fail(M3PC_EINVAL, "idx %d outside [0, T=%d)", idx, T);
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(h->device));
    Plan *pi = nullptr, *fid = nullptr;
    CHK(get_plan(h, masks_pi, &pi));
    CHK(get_plan(h, masks_fid, &fid));
    bind_slot(h, 0);
    h->slot[0].policy_valid = false;
    h->slot[0].n_windows = 0;
    CHK(fill_rtok(h, rtg, batch, st));
    TokIn in;
    memset(&in, 0, sizeof(in));
    const float* src[4] = {states, actions, rewards, h->rtok};
    for (int k = 0; k < 4; ++k) {
        in.ptr[k] = src[k];
        in.bstride[k] = (long long)T * h->feat[k];
        in.normalize[k] = k == M3PC_RETURNS ? 0 : h->tok_norm[k];
    }
    h->allow_splitk = true;
    WsScope ws(h, true, true);
    CHK(forward_impl(h, pi, in, batch, inferred, nullptr, nullptr, nullptr, nullptr, DT_F32, st));
    launch_goal_overlay(inferred, states, window_states, (long long)batch * T, T, h->S, idx, h->tok_mean[M3PC_STATES],
                        h->tok_std[M3PC_STATES], h->tok_norm[M3PC_STATES], st);
    in.ptr[M3PC_STATES] = window_states;
    CHK(forward_impl(h, fid, in, batch, nullptr, nullptr, nullptr, out_mu, out_std, DT_F32, st));
    return check_launch("goal_step");
}

// m3pc_goal_step for many windows: the same two forwards, exactly pruned to what the reference reads of them, in the
// arithmetic of the candidate pass (bf16 MFMA or fp32), in the candidate workspace.
//   path inference (pi mask): the states head is read at the window rows t <= idx and idx+2 <= t <= T-2 only
//   (zeroshot_omtm/learner.py:240-246) -- those decoder tokens are the queries; inverse dynamics (fid mask): the action
//   distribution is read at token idx only (learner.py:250-256) -- ONE query per window, a masked token, so its query row is
//   shared by the batch.  Neither mask keeps a rewards or returns token (zeroshot_omtm/masks.py:30-47, 72-91): those rows
//   of the window never enter, which is why the call does not take them.
// goal_mode M3PC_GOAL_ID: action_id_sample (learner.py:60-149) -- the second forward alone, under the gid mask (= pi mask).
// plan tables, query set and candidate-independent decoder rows of one goal forward (cached per idx / weights)
static int goal_prepare(m3pc_handle* h, int kind, int qi, int idx, int dt, hipStream_t st, Plan** pl_out, Plan::Query** q_out) {
    const int T = h->T;
    Plan* pl = nullptr;
    CHK(get_mask_plan(h, kind, idx, &pl));
    std::vector<int> toks;
    if (qi == 2) {
        for (int t = 0; t < T; ++t)
            if (t <= idx || (t >= idx + 2 && t < T - 1)) toks.push_back(M3PC_STATES * T + t);
    } else {
        toks.push_back(M3PC_ACTIONS * T + idx);
    }
    CHK(build_query_list(h, pl, qi, T - idx, toks, 1, qi == 2 ? M3PC_STATES : M3PC_ACTIONS, 0));
    CHK(build_tables(h, pl, qi, dt, st));
    CHK(ensure_edec(h, pl, st));
    if (pl_out) *pl_out = pl;
    if (q_out) *q_out = &pl->query[qi];
    return 0;
}

static int goal_forward(m3pc_handle* h, int kind, int qi, int idx, const float* states, const float* actions, int n, int dt,
                        hipStream_t st, int tail, float** xrows) {
    const int T = h->T;
    Plan* pl = nullptr;
    Plan::Query* qp = nullptr;
    CHK(goal_prepare(h, kind, qi, idx, dt, st, &pl, &qp));
    Plan::Query& q = *qp;
    if ((long long)n * pl->Le > h->R || (long long)n * q.nq > h->R) return fail(M3PC_ENOMEM, "batch %d exceeds workspace", n);
    TokIn in;
    memset(&in, 0, sizeof(in));
    in.ptr[M3PC_STATES] = states;
    in.bstride[M3PC_STATES] = (long long)T * h->S;
    in.normalize[M3PC_STATES] = h->tok_norm[M3PC_STATES];
    in.ptr[M3PC_ACTIONS] = actions;
    in.bstride[M3PC_ACTIONS] = (long long)T * h->A;
    in.normalize[M3PC_ACTIONS] = h->tok_norm[M3PC_ACTIONS];
    CHK(run_encoder(h, pl, in, n, dt, st, dt == DT_BF16, 0));
    return pruned_decoder(h, pl, q, q.tab[dt], n, dt, st, tail, xrows);
}

int m3pc_goal_step_batch(m3pc_handle* h, int batch, const float* states, const float* actions, int idx, int goal_mode,
                         int precision, float* window_states, float* out_mu, float* out_std, void* stream) {
    if (!h || !states || !actions || !out_mu || !out_std) return fail(M3PC_EINVAL, "null argument");
    if (!h->weights_loaded) return fail(M3PC_ESTATE, "weights not loaded");
    for (int k = 0; k < 2; ++k)
        if (!h->tok_set[k]) return fail(M3PC_ESTATE, "tokenizer '%s' not set", KEYN[k]);
    if (batch < 1 || batch > h->dm.max_goal_batch) return fail(M3PC_EINVAL, "batch %d outside [1, max_goal_batch=%d]", batch, h->dm.max_goal_batch);
    if (!precision_ok(precision)) return fail(M3PC_EINVAL, "bad precision %d", precision);
    if (goal_mode != M3PC_GOAL_PIID && goal_mode != M3PC_GOAL_ID) return fail(M3PC_EINVAL, "bad goal_mode %d", goal_mode);
    const int T = h->T, d = h->d;
    if (idx < 0 || idx >= T) return fail(M3PC_EINVAL, "idx %d outside [0, T=%d)", idx, T);
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(h->device));
    const int dt = pass_dt(precision);
    X3Scope x3(h, precision == M3PC_PREC_BF16X3);
    bind_ws(h, &h->base);
    CHK(ws_sync(h, st));
    // kernels chosen by the row count (split-K, the few-row fp32 kernels) stay off: a window's result must not depend on
    // which other windows share its call (environment sharding, m3pc_amd/dist.py)
    h->allow_splitk = false;
    h->pass_scale = 1.0;
    int nq_a = 0;
    for (int t = 0; t < T; ++t) nq_a += (t <= idx || (t >= idx + 2 && t < T - 1)) ? 1 : 0;
    float* const ws_all = window_states ? window_states : h->goal_ws;
    // windows [c0, c0 + cnt) on stream s, in the workspace rows of those windows (set_view: 2T rows per window)
    auto run_part = [&](int c0, int cnt, hipStream_t s) -> int {
        set_view(h, c0, cnt);
        const float* st_p = states + (size_t)c0 * T * h->S;
        const float* ac_p = actions + (size_t)c0 * T * h->A;
        const float* second = st_p;
        if (goal_mode == M3PC_GOAL_PIID) {
            CHK(goal_forward(h, 2, 2, idx, st_p, ac_p, cnt, dt, s, TAIL_HEADS, nullptr));
            float* ws = ws_all + (size_t)c0 * T * h->S;
            launch_goal_overlay_rows(h->pred[0], st_p, ws, cnt, T, h->S, idx, nq_a, s);
            second = ws;
        } else if (window_states) {
            HIPCHK(hipMemcpyAsync(window_states + (size_t)c0 * T * h->S, st_p, (size_t)cnt * T * h->S * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        float* xr = nullptr;
        CHK(goal_forward(h, goal_mode == M3PC_GOAL_PIID ? 3 : 2, 3, idx, second, ac_p, cnt, dt, s, TAIL_X, &xr));
        // decoder.norm of the one query row per window, then the action head (mtm_model.py:705, 313-321), fp32
        const bool fuse_ln = actor_head_fuses_ln(d, h->A);  // (the head kernel normalises its rows itself: one launch fewer)
        if (!fuse_ln) {
            LnP ln;
            memset(&ln, 0, sizeof(ln));
            ln.X = xr;
            ln.ldx = d;
            ln.rows = cnt;
            ln.d = d;
            ln.g1 = W(h, "decoder.norm.weight").f;
            ln.b1 = W(h, "decoder.norm.bias").f;
            ln.Yf = h->G;
            launch_layernorm(ln, s);
        }
        ActorP ac;
        memset(&ac, 0, sizeof(ac));
        ac.X = fuse_ln ? xr : h->G;
        if (fuse_ln) {
            ac.ln_g = W(h, "decoder.norm.weight").f;
            ac.ln_b = W(h, "decoder.norm.bias").f;
        }
        ac.ldx = d;
        ac.rows = cnt;
        ac.d = d;
        ac.A = h->A;
        ac.Wmu = W(h, "output_head_dict.actions.mu.weight").f;
        ac.bmu = W(h, "output_head_dict.actions.mu.bias").f;
        ac.Wls = W(h, "output_head_dict.actions.log_std.weight").f;
        ac.bls = W(h, "output_head_dict.actions.log_std.bias").f;
        ac.mu = out_mu + (size_t)c0 * h->A;
        ac.sd = out_std + (size_t)c0 * h->A;
        launch_actor_head(ac, s);
        return 0;
    };
    // Many windows in bf16: two halves on two streams, as the candidate pass runs its halves -- the encoder launches of the
    // whole call are 2.5 and 3 rounds of fused-tail tiles, and the other half's attention / embedding kernels (HBM-bound) run
    // beside a half's tiles.  The kernel choice goes by the size of the whole call (pass_scale): same bits either way.
    int rc = 0;
    if (h->two_stream && dt == DT_BF16 && batch >= 2048 && !h->prof_serial) {
        const int n0 = ((batch / 2 + 63) / 64) * 64;
        // what is built once per (weights, idx) -- plan tables, query sets, the shared decoder rows -- before the streams fork
        if (goal_mode == M3PC_GOAL_PIID) CHK(goal_prepare(h, 2, 2, idx, dt, st, nullptr, nullptr));
        CHK(goal_prepare(h, goal_mode == M3PC_GOAL_PIID ? 3 : 2, 3, idx, dt, st, nullptr, nullptr));
        HIPCHK(hipEventRecord(h->ev_fork, st));
        HIPCHK(hipStreamWaitEvent(h->aux, h->ev_fork, 0));
        h->pass_scale = (double)batch / (double)n0;
        rc = run_part(0, n0, st);
        h->pass_scale = (double)batch / (double)(batch - n0);
        if (rc == 0) rc = run_part(n0, batch - n0, h->aux);
        HIPCHK(hipEventRecord(h->ev_join, h->aux));
        HIPCHK(hipStreamWaitEvent(st, h->ev_join, 0));
    } else {
        rc = run_part(0, batch, st);
    }
    h->pass_scale = 1.0;
    set_view(h, 0, h->base.max_cand);
    if (rc) return rc;
    return check_launch("goal_step_batch");
}

// common argument checks of the plan-step entry points; binds the step's slot
static int plan_check(m3pc_handle* h, const m3pc_plan_args* a, bool need_critic) {
    if (!h->weights_loaded) return fail(M3PC_ESTATE, "weights not loaded");
    for (int k = 0; k < 4; ++k)
        if (!h->tok_set[k]) return fail(M3PC_ESTATE, "tokenizer '%s' not set", KEYN[k]);
    const int T = h->T;
    if (a->horizon < 1 || a->horizon > T) return fail(M3PC_EINVAL, "horizon %d outside [1, T=%d]", a->horizon, T);
    if (a->mode < 0 || a->mode > 2) return fail(M3PC_EINVAL, "bad mode %d", a->mode);
    if (!precision_ok(a->precision)) return fail(M3PC_EINVAL, "bad precision %d", a->precision);
    if (a->slot < 0 || a->slot >= M3PC_SLOTS) return fail(M3PC_EINVAL, "slot %d outside [0, %d)", a->slot, M3PC_SLOTS);
    if (a->flags & ~(M3PC_PLAN_DEFER_JOIN | M3PC_PLAN_PRUNED_POLICY))  // (also what a caller built against the shorter ABI v2 structure would hand over)
        return fail(M3PC_EINVAL, "unknown m3pc_plan_args::flags 0x%x (is the caller's structure the ABI v%d one?)", a->flags, M3PC_ABI_VERSION);
    if (need_critic && a->mode != M3PC_MODE_RTG && !h->critic_set) return fail(M3PC_ESTATE, "critic weights not set");
    HIPCHK(hipSetDevice(h->device));
    bind_slot(h, a->slot);
    return 0;
}

// PASS 1 of a plan step (learner.py:278-284): the returns tokens of the window, then the return-conditioned policy at
// batch 1 under the rcbc mask (finetune_omtm/masks.py:7-27), always fp32, in the chain workspace; leaves loc / sd / rtok in
// the step's slot.
int m3pc_policy_pass(m3pc_handle* h, const m3pc_plan_args* a, const float* states, const float* actions, const float* rewards,
                     float* loc, float* std_, void* stream) {
    if (!h || !a || !states || !actions || !rewards) return fail(M3PC_EINVAL, "null argument");
    CHK(plan_check(h, a, false));
    hipStream_t st = (hipStream_t)stream;
    const int T = h->T, hh = a->horizon, idx = T - hh;
    if (a->returns) {
        // the caller's returns row (learner.py:272-293 consumes whatever trajectory["returns"] holds): tokenised as
        // ContinuousTokenizer.encode does, in the row's own dtype, then cast (continuous.py:74-79)
        launch_tokenize(a->returns, a->returns_f64, h->rtok, T, 1, h->tok_mean[M3PC_RETURNS], h->tok_std[M3PC_RETURNS],
                        h->tok_norm[M3PC_RETURNS], st);
    } else {
        // constant return-to-go: float64 normalisation then cast (learner.py:371-374, continuous.py:74-79)
        double rt = a->rtg;
        if (h->tok_norm[M3PC_RETURNS]) rt = (rt - (double)h->h_mean[M3PC_RETURNS][0]) / (double)h->h_std[M3PC_RETURNS][0];
        launch_fill(h->rtok, (float)rt, T, st);
    }
    Plan* pl = nullptr;
    CHK(get_mask_plan(h, 0, idx, &pl));
    TokIn in;
    memset(&in, 0, sizeof(in));
    in.ptr[M3PC_STATES] = states;
    in.normalize[M3PC_STATES] = h->tok_norm[M3PC_STATES];
    in.ptr[M3PC_ACTIONS] = actions;
    in.normalize[M3PC_ACTIONS] = h->tok_norm[M3PC_ACTIONS];
    in.ptr[M3PC_REWARDS] = rewards;
    in.normalize[M3PC_REWARDS] = h->tok_norm[M3PC_REWARDS];
    in.ptr[M3PC_RETURNS] = h->rtok;
    h->allow_splitk = true;
    int rc;
    if ((a->flags & M3PC_PLAN_PRUNED_POLICY) && !loc && !std_ && idx > 0) {
        // the policy head at the action tokens idx .. T-1 only (masked under the rcbc mask for idx > 0): query set 4 of the plan
        WsScope ws(h, true, true, a->slot);
        std::vector<int> toks;
        for (int t = idx; t < T; ++t) toks.push_back(M3PC_ACTIONS * T + t);
        rc = build_query_list(h, pl, 4, hh, toks, 1, M3PC_ACTIONS, 0);
        if (!rc) rc = build_tables(h, pl, 4, DT_F32, st);
        if (!rc && !pl->query[4].all_masked) rc = fail(M3PC_EINVAL, "policy pass: an action token at t >= idx is not masked");
        if (!rc) rc = run_encoder(h, pl, in, 1, DT_F32, st, false, 0);
        float* xr = nullptr;
        if (!rc) rc = pruned_decoder(h, pl, pl->query[4], pl->query[4].tab[DT_F32], 1, DT_F32, st, TAIL_X, &xr);
        if (!rc) {  // decoder.norm of the h query rows, then the action head (mtm_model.py:705, 313-321)
            const int d = h->d;
            const bool fuse_ln = actor_head_fuses_ln(d, h->A);
            if (!fuse_ln) {
                LnP ln;
                memset(&ln, 0, sizeof(ln));
                ln.X = xr;
                ln.ldx = d;
                ln.rows = hh;
                ln.d = d;
                ln.g1 = W(h, "decoder.norm.weight").f;
                ln.b1 = W(h, "decoder.norm.bias").f;
                ln.Yf = h->G;
                launch_layernorm(ln, st);
            }
            ActorP ac;
            memset(&ac, 0, sizeof(ac));
            ac.X = fuse_ln ? xr : h->G;
            if (fuse_ln) {
                ac.ln_g = W(h, "decoder.norm.weight").f;
                ac.ln_b = W(h, "decoder.norm.bias").f;
            }
            ac.ldx = d;
            ac.rows = hh;
            ac.d = d;
            ac.A = h->A;
            ac.Wmu = W(h, "output_head_dict.actions.mu.weight").f;
            ac.bmu = W(h, "output_head_dict.actions.mu.bias").f;
            ac.Wls = W(h, "output_head_dict.actions.log_std.weight").f;
            ac.bls = W(h, "output_head_dict.actions.log_std.bias").f;
            ac.mu = h->loc + (size_t)idx * h->A;
            ac.sd = h->sd + (size_t)idx * h->A;
            launch_actor_head(ac, st);
            if (hipMemsetAsync(h->loc, 0, (size_t)idx * h->A * sizeof(float), st) != hipSuccess ||
                hipMemsetAsync(h->sd, 0, (size_t)idx * h->A * sizeof(float), st) != hipSuccess)
                rc = fail(M3PC_EHIP, "hipMemsetAsync failed in the pruned policy pass");
        }
    } else {
        WsScope ws(h, true, true, a->slot);
        rc = forward_impl(h, pl, in, 1, nullptr, nullptr, nullptr, h->loc, h->sd, DT_F32, st);
    }
    h->allow_splitk = false;
    if (rc) return rc;
    h->slot[a->slot].policy_valid = true;
    h->slot[a->slot].n_windows = 1;
    if (loc) HIPCHK(hipMemcpyAsync(loc, h->loc, (size_t)T * h->A * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (std_) HIPCHK(hipMemcpyAsync(std_, h->sd, (size_t)T * h->A * sizeof(float), hipMemcpyDeviceToDevice, st));
    return check_launch("policy_pass");
}

// Candidates + PASS 2 + scoring of a plan step (learner.py:285-316) from the slot's policy head, in the candidate workspace.
int m3pc_candidate_pass(m3pc_handle* h, const m3pc_plan_args* a, const float* states, const float* actions, const float* rewards,
                        const float* eps, float* loc, float* std_, float* sample_actions, float* expect_return,
                        float* pred_rewards, float* pred_boot, void* stream) {
    if (!h || !a || !states || !actions || !rewards || !eps || !sample_actions || !expect_return)
        return fail(M3PC_EINVAL, "null argument");
    CHK(plan_check(h, a, true));
    if (a->window < 0 || a->window >= h->slot[a->slot].n_windows)
        return fail(M3PC_ESTATE, "m3pc_candidate_pass: slot %d holds %d policy pass(es), window %d asked for (m3pc_policy_pass[_batch] first)",
                    a->slot, h->slot[a->slot].n_windows, a->window);
    const int T = h->T;
    if (a->n_count < 1 || a->n_begin < 0 || a->n_begin + a->n_count > a->n_total)
        return fail(M3PC_EINVAL, "candidate range [%d,+%d) outside n_total=%d", a->n_begin, a->n_count, a->n_total);
    if (a->n_count > h->dm.max_candidates) return fail(M3PC_ENOMEM, "n_count %d > max_candidates %d", a->n_count, h->dm.max_candidates);
    hipStream_t st = (hipStream_t)stream;
    const int hh = a->horizon, idx = T - hh;
    bind_ws(h, &h->base);
    h->allow_splitk = false;

    // candidates of [c0, c0 + cnt) (relative to n_begin), on the stream of the part that scores them
    auto sample = [&](int c0, int cnt, hipStream_t s) {
        SampleP sp;
        memset(&sp, 0, sizeof(sp));
        sp.hist_actions = actions;
        sp.loc = h->loc + (size_t)a->window * T * h->A;
        sp.sd = h->sd + (size_t)a->window * T * h->A;
        sp.eps = eps;
        sp.mode = a->mode == M3PC_MODE_NOISE ? 1 : 0;
        sp.T = T;
        sp.A = h->A;
        sp.idx = idx;
        sp.h = hh;
        sp.n_begin = a->n_begin + c0;
        sp.n_count = cnt;
        sp.cand = h->base.cand + (size_t)c0 * T * h->A;
        sp.sample_actions = sample_actions + (size_t)c0 * hh * h->A;
        if (c0 == 0) {  // the caller's copies of the policy head ride on the first launch
            sp.loc_out = loc;
            sp.sd_out = std_;
        }
        launch_sample(sp, s);
    };

    // PASS 2 + scoring.  Large bf16 batches are cut into two candidate halves that run the same kernel chain
    // on two HIP streams over disjoint workspace halves.  The fused layer tails work in 128-row tiles, one per CU:
    // 1024 candidates are 392 tiles = two rounds on 256 CUs with the second round half empty, a half is 196 tiles =
    // one round, and the other half's attention / projection kernels run on the CUs it leaves free.  Candidates are
    // independent, results are identical to the one-stream order.
    const int dt = pass_dt(a->precision);
    X3Scope x3(h, a->precision == M3PC_PREC_BF16X3);
    const int n = a->n_count;
    h->slot_join_n[a->slot] = 0;
    // (only when one half alone fills the chip with fused-tail tiles: more than 256 tiles of 128 rows in the whole pass)
    if (h->two_stream && dt == DT_BF16 && n >= 512 && (long long)n * (2 * T - hh + 1) > 256 * 128) {
        // part sizes: M3PC_STREAM_SPLIT=a,b,c (lab) or two halves
        std::vector<int> parts;
        if (!h->stream_split.empty()) {
            int left = n;
            for (int v : h->stream_split)
                if (v > 0 && v < left && parts.size() + 1 < h->auxs.size() + 1) {
                    parts.push_back(v);
                    left -= v;
                }
            parts.push_back(left);
        } else {
            int n0 = ((n / 2 + 127) / 128) * 128;
            parts = {n0, n - n0};
        }
        // M3PC_PLAN_DEFER_JOIN: the caller's stream does not wait for the other parts (m3pc_candidate_join does, for the
        // consumer), and a pass of the same part sizes as the deferred ones before it starts without waiting for them either:
        // per stream it touches the rows that stream's own earlier work touched.
        const bool defer = (a->flags & M3PC_PLAN_DEFER_JOIN) != 0 && !h->prof_serial && parts.size() <= 4;
        if (!(defer && parts == h->defer_parts)) CHK(ws_sync(h, st));
        HIPCHK(hipEventRecord(h->ev_fork, st));
        int rc = 0;
        // enqueued stage by stage, alternating between the parts: the host needs ~1.5 us per launch, and a part whose 45
        // launches are all enqueued behind the other part's starts that much later on the device -- and ends that much later,
        // with the other stream idle.  (With the profiling brackets in serial mode: one part after the other.)
        const int n_stage = h->dm.n_enc_layer + 1;
        PieceState lnst[4];
        for (int stg = 0; stg < (h->prof_serial ? 1 : n_stage) && rc == 0; ++stg) {
            int c0 = 0;
            for (size_t i = 0; i < parts.size() && rc == 0; ++i) {
                hipStream_t s = i == 0 || h->prof_serial ? st : h->auxs[i - 1];
                if (stg == 0) {
                    if (s != st) HIPCHK(hipStreamWaitEvent(s, h->ev_fork, 0));
                    sample(c0, parts[i], s);
                }
                set_view(h, c0, parts[i]);
                rc = candidate_pass(h, a, states, rewards, parts[i], sample_actions + (size_t)c0 * hh * h->A, expect_return + c0,
                                    pred_rewards ? pred_rewards + (size_t)c0 * hh : nullptr,
                                    pred_boot ? pred_boot + (size_t)c0 * hh : nullptr, dt, s, nullptr,
                                    h->prof_serial ? 0 : stg, h->prof_serial ? 1 << 30 : stg + 1, &lnst[i]);
                if (s != st && stg == n_stage - 1 && rc == 0) {
                    if (defer) {
                        HIPCHK(hipEventRecord(h->slot_join[a->slot][i - 1], s));
                        HIPCHK(hipEventRecord(h->aux_tail[i - 1], s));
                        h->aux_unjoined[i - 1] = true;
                        h->slot_join_n[a->slot] = (int)i;
                    } else {
                        HIPCHK(hipEventRecord(h->ev_joins[i - 1], s));
                        HIPCHK(hipStreamWaitEvent(st, h->ev_joins[i - 1], 0));
                    }
                }
                c0 += parts[i];
            }
        }
        if (defer && rc == 0) h->defer_parts = parts;
        set_view(h, 0, h->dm.max_candidates);
        return rc;
    }
    CHK(ws_sync(h, st));
    sample(0, n, st);
    return candidate_pass(h, a, states, rewards, n, sample_actions, expect_return, pred_rewards, pred_boot, dt, st);
}

int m3pc_candidate_join(m3pc_handle* h, int slot, void* stream) {
    if (!h) return fail(M3PC_EINVAL, "null handle");
    if (slot < 0 || slot >= M3PC_SLOTS) return fail(M3PC_EINVAL, "slot %d outside [0, %d)", slot, M3PC_SLOTS);
    for (int i = 0; i < h->slot_join_n[slot]; ++i) HIPCHK(hipStreamWaitEvent((hipStream_t)stream, h->slot_join[slot][i], 0));
    h->slot_join_n[slot] = 0;
    return 0;
}

// m3pc_policy_pass + m3pc_candidate_pass on one stream
int m3pc_plan_step(m3pc_handle* h, const m3pc_plan_args* a, const float* states, const float* actions, const float* rewards,
                   const float* eps, float* loc, float* std_, float* sample_actions, float* expect_return,
                   float* pred_rewards, float* pred_boot, void* stream) {
    if (!h || !a || !states || !actions || !rewards || !eps || !sample_actions || !expect_return)
        return fail(M3PC_EINVAL, "null argument");
    if (a->mode >= 0 && a->mode <= 2 && a->mode != M3PC_MODE_RTG && !h->critic_set) return fail(M3PC_ESTATE, "critic weights not set");
    if (a->n_count < 1 || a->n_begin < 0 || a->n_begin + a->n_count > a->n_total)
        return fail(M3PC_EINVAL, "candidate range [%d,+%d) outside n_total=%d", a->n_begin, a->n_count, a->n_total);
    if (a->n_count > h->dm.max_candidates) return fail(M3PC_ENOMEM, "n_count %d > max_candidates %d", a->n_count, h->dm.max_candidates);
    CHK(m3pc_policy_pass(h, a, states, actions, rewards, nullptr, nullptr, stream));
    return m3pc_candidate_pass(h, a, states, actions, rewards, eps, loc, std_, sample_actions, expect_return, pred_rewards,
                               pred_boot, stream);
}

// fills h->rtok[w * T + t] with window w's normalised return-to-go (float64 normalisation then cast: learner.py:371-374,
// continuous.py:74-79)
static int fill_rtok(m3pc_handle* h, const double* rtg, int n_windows, hipStream_t st) {
    for (int w = 0; w < n_windows; ++w) {
        double rt = rtg[w];
        if (h->tok_norm[M3PC_RETURNS]) rt = (rt - (double)h->h_mean[M3PC_RETURNS][0]) / (double)h->h_std[M3PC_RETURNS][0];
        launch_fill(h->rtok + (size_t)w * h->T, (float)rt, h->T, st);
    }
    return 0;
}

int m3pc_score_actions(m3pc_handle* h, const m3pc_plan_args* a, int n_windows, const float* states, const float* actions,
                       const float* rewards, const float* cand, const int* window_index, float* expect_return,
                       float* pred_rewards, float* pred_boot, void* stream) {
    if (!h || !a || !states || !actions || !rewards || !cand || !expect_return) return fail(M3PC_EINVAL, "null argument");
    if (!h->weights_loaded) return fail(M3PC_ESTATE, "weights not loaded");
    for (int k = 0; k < 4; ++k)
        if (!h->tok_set[k]) return fail(M3PC_ESTATE, "tokenizer '%s' not set", KEYN[k]);
    const int T = h->T, n = a->n_count;
    if (a->horizon < 1 || a->horizon > T) return fail(M3PC_EINVAL, "horizon %d outside [1, T=%d]", a->horizon, T);
    if (a->mode != M3PC_MODE_RTG && a->mode != M3PC_MODE_CRITIC) return fail(M3PC_EINVAL, "mode must be RTG or CRITIC scoring");
    if (!precision_ok(a->precision)) return fail(M3PC_EINVAL, "bad precision %d", a->precision);
    if (n < 1 || (n > h->dm.max_candidates && !(a->precision == M3PC_PREC_FP32 && n <= h->chain[0].max_cand)))
        return fail(M3PC_ENOMEM, "n_count %d outside [1, max_candidates=%d]", n, h->dm.max_candidates);
    if (n_windows < 1 || (n_windows > 1 && !window_index)) return fail(M3PC_EINVAL, "n_windows > 1 needs window_index");
    if (a->mode == M3PC_MODE_CRITIC && !h->critic_set) return fail(M3PC_ESTATE, "critic weights not set");
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(h->device));
    const int dt = pass_dt(a->precision);
    const bool fp32 = a->precision == M3PC_PREC_FP32;
    X3Scope x3(h, a->precision == M3PC_PREC_BF16X3);
    // few-row fp32 calls (the re-score of a batched plan) run in the chain workspace, like m3pc_rescore
    WsScope ws(h, fp32 && n <= h->chain[0].max_cand, false, a->slot);
    if (h->cur == &h->base) CHK(ws_sync(h, st));
    SampleP sp;
    memset(&sp, 0, sizeof(sp));
    sp.hist_actions = actions;
    sp.eps = cand;
    sp.mode = 2;
    sp.T = T;
    sp.A = h->A;
    sp.idx = T - a->horizon;
    sp.h = a->horizon;
    sp.n_count = n;
    sp.widx = window_index;
    sp.cand = h->cand;
    launch_sample(sp, st);
    // (split-K is row-count dependent: only where the caller does not rely on sharding exactness, i.e. the fp32 re-scores)
    h->allow_splitk = fp32;
    const int rc = candidate_pass(h, a, states, rewards, n, cand, expect_return, pred_rewards, pred_boot, dt, st, window_index);
    h->allow_splitk = false;
    return rc;
}

// PASS 1 of E windows at once (learner.py:278-284 per window): return-conditioned policy, batch E, rcbc mask, fp32, in the
// policy workspace; the slot then holds E policy heads (loc / sd rows [w T, (w+1) T)) and E rows of returns tokens.
int m3pc_policy_pass_batch(m3pc_handle* h, const m3pc_plan_args* a, int n_windows, const float* states, const float* actions,
                           const float* rewards, const double* rtg, float* loc, float* std_, void* stream) {
    if (!h || !a || !states || !actions || !rewards || !rtg) return fail(M3PC_EINVAL, "null argument");
    if (!h->weights_loaded) return fail(M3PC_ESTATE, "weights not loaded");
    for (int k = 0; k < 4; ++k)
        if (!h->tok_set[k]) return fail(M3PC_ESTATE, "tokenizer '%s' not set", KEYN[k]);
    const int T = h->T, E = n_windows;
    if (E < 1 || E > h->dm.max_batch) return fail(M3PC_ENOMEM, "n_windows %d outside [1, max_batch=%d]", E, h->dm.max_batch);
    if (a->horizon < 1 || a->horizon > T) return fail(M3PC_EINVAL, "horizon %d outside [1, T=%d]", a->horizon, T);
    if (a->mode < 0 || a->mode > 2) return fail(M3PC_EINVAL, "bad mode %d", a->mode);
    if (a->slot < 0 || a->slot >= M3PC_SLOTS) return fail(M3PC_EINVAL, "slot %d outside [0, %d)", a->slot, M3PC_SLOTS);
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(h->device));
    const int idx = T - a->horizon, A = h->A;
    bind_slot(h, a->slot);
    CHK(fill_rtok(h, rtg, E, st));
    Plan* pl = nullptr;
    CHK(get_mask_plan(h, 0, idx, &pl));
    TokIn in;
    memset(&in, 0, sizeof(in));
    in.ptr[M3PC_STATES] = states;
    in.bstride[M3PC_STATES] = (long long)T * h->S;
    in.normalize[M3PC_STATES] = h->tok_norm[M3PC_STATES];
    in.ptr[M3PC_ACTIONS] = actions;
    in.bstride[M3PC_ACTIONS] = (long long)T * A;
    in.normalize[M3PC_ACTIONS] = h->tok_norm[M3PC_ACTIONS];
    in.ptr[M3PC_REWARDS] = rewards;
    in.bstride[M3PC_REWARDS] = T;
    in.normalize[M3PC_REWARDS] = h->tok_norm[M3PC_REWARDS];
    in.ptr[M3PC_RETURNS] = h->rtok;
    in.bstride[M3PC_RETURNS] = T;
    h->allow_splitk = true;
    {
        WsScope ws(h, true, true, a->slot);
        const int rc = forward_impl(h, pl, in, E, nullptr, nullptr, nullptr, h->loc, h->sd, DT_F32, st);
        h->allow_splitk = false;
        if (rc) return rc;
    }
    h->slot[a->slot].policy_valid = E == 1;  // (m3pc_rescore works on a single-window slot; batched callers re-score with m3pc_score_actions)
    h->slot[a->slot].n_windows = E;
    if (loc) HIPCHK(hipMemcpyAsync(loc, h->loc, (size_t)E * T * A * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (std_) HIPCHK(hipMemcpyAsync(std_, h->sd, (size_t)E * T * A * sizeof(float), hipMemcpyDeviceToDevice, st));
    return check_launch("policy_pass_batch");
}

int m3pc_plan_step_batch(m3pc_handle* h, const m3pc_plan_args* a, int n_windows, const float* states, const float* actions,
                         const float* rewards, const double* rtg, const float* eps, const int* window_index, float* loc,
                         float* std_, float* sample_actions, float* expect_return, void* stream) {
    if (!h || !a || !states || !actions || !rewards || !rtg || !eps || !window_index || !sample_actions || !expect_return)
        return fail(M3PC_EINVAL, "null argument");
    const int T = h->T, E = n_windows, N = a->n_total;
    if (!precision_ok(a->precision)) return fail(M3PC_EINVAL, "bad precision %d", a->precision);
    if (E >= 1 && (N < 1 || (long long)E * N > h->dm.max_candidates))
        return fail(M3PC_ENOMEM, "n_windows * n_total = %lld > max_candidates %d", (long long)E * N, h->dm.max_candidates);
    if (a->mode >= 0 && a->mode <= 2 && a->mode != M3PC_MODE_RTG && !h->critic_set) return fail(M3PC_ESTATE, "critic weights not set");
    CHK(m3pc_policy_pass_batch(h, a, n_windows, states, actions, rewards, rtg, nullptr, nullptr, stream));
    hipStream_t st = (hipStream_t)stream;
    const int hh = a->horizon, idx = T - hh, A = h->A;
    h->slot[a->slot].policy_valid = false;
    CHK(ws_sync(h, st));
    // candidates of window w: rows [w N, (w+1) N) of cand / sample_actions, drawn from window w's policy head and eps block
    for (int w = 0; w < E; ++w) {
        SampleP sp;
        memset(&sp, 0, sizeof(sp));
        sp.hist_actions = actions + (size_t)w * T * A;
        sp.loc = h->loc + (size_t)w * T * A;
        sp.sd = h->sd + (size_t)w * T * A;
        const size_t per = a->mode == M3PC_MODE_NOISE ? (size_t)hh * A : (size_t)T * A;
        sp.eps = eps + (size_t)w * N * per;
        sp.mode = a->mode == M3PC_MODE_NOISE ? 1 : 0;
        sp.T = T;
        sp.A = A;
        sp.idx = idx;
        sp.h = hh;
        sp.n_count = N;
        sp.cand = h->cand + (size_t)w * N * T * A;
        sp.sample_actions = sample_actions + (size_t)w * N * hh * A;
        sp.loc_out = loc ? loc + (size_t)w * T * A : nullptr;
        sp.sd_out = std_ ? std_ + (size_t)w * T * A : nullptr;
        launch_sample(sp, st);
    }
    const int dt = pass_dt(a->precision);
    X3Scope x3(h, a->precision == M3PC_PREC_BF16X3);
    return candidate_pass(h, a, states, rewards, E * N, sample_actions, expect_return, nullptr, nullptr, dt, st, window_index);
}

int m3pc_rescore(m3pc_handle* h, const m3pc_plan_args* a, const float* states, const float* actions, const float* rewards,
                 const float* eps, const int* index, int n, float* sample_actions, float* expect_return, void* stream) {
    if (!h || !a || !states || !actions || !rewards || !eps || !index || !expect_return) return fail(M3PC_EINVAL, "null argument");
    if (!h->weights_loaded) return fail(M3PC_ESTATE, "weights not loaded");
    if (a->slot < 0 || a->slot >= M3PC_SLOTS) return fail(M3PC_EINVAL, "slot %d outside [0, %d)", a->slot, M3PC_SLOTS);
    if (!h->slot[a->slot].policy_valid) return fail(M3PC_ESTATE, "m3pc_rescore needs a preceding m3pc_plan_step / m3pc_policy_pass on slot %d", a->slot);
    const int T = h->T;
    if (a->horizon < 1 || a->horizon > T || a->mode < 0 || a->mode > 2) return fail(M3PC_EINVAL, "bad horizon/mode");
    // runs in the chain workspace when it fits (so that it can be enqueued beside a candidate pass), else in the candidate one
    const bool in_chain = n <= h->chain[0].max_cand;
    if (n < 1 || (!in_chain && n > h->dm.max_candidates))
        return fail(M3PC_ENOMEM, "n %d outside [1, max(max_rescore=%d, max_candidates=%d)]", n, h->chain[0].max_cand, h->dm.max_candidates);
    if (a->mode != M3PC_MODE_RTG && !h->critic_set) return fail(M3PC_ESTATE, "critic weights not set");
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(h->device));
    bind_slot(h, a->slot);
    WsScope ws(h, in_chain, false, a->slot);
    if (!in_chain) CHK(ws_sync(h, st));
    float* sa = sample_actions ? sample_actions : (in_chain ? h->sa_chain[a->slot & 1] : h->sa_buf);
    SampleP sp;
    memset(&sp, 0, sizeof(sp));
    sp.hist_actions = actions;
    sp.loc = h->loc;
    sp.sd = h->sd;
    sp.eps = eps;
    sp.mode = a->mode == M3PC_MODE_NOISE ? 1 : 0;
    sp.T = T;
    sp.A = h->A;
    sp.idx = T - a->horizon;
    sp.h = a->horizon;
    sp.n_count = n;
    sp.index = index;
    sp.cand = h->cand;
    sp.sample_actions = sa;
    launch_sample(sp, st);
    h->allow_splitk = true;
    const int rc = candidate_pass(h, a, states, rewards, n, sa, expect_return, nullptr, nullptr, DT_F32, st);
    h->allow_splitk = false;
    return rc;
}

int m3pc_rescore_topk(m3pc_handle* h, const m3pc_plan_args* a, const float* states, const float* actions,
                      const float* rewards, const float* eps, float* expect_return, int k, int* topk_index, void* stream) {
    if (!h || !a || !expect_return) return fail(M3PC_EINVAL, "null argument");
    if (a->n_total < 1 || a->n_total > 16384) return fail(M3PC_EINVAL, "top-k supports n_total <= 16384");
    if (k < 1 || k > a->n_total || (k > h->dm.max_candidates && k > h->chain[0].max_cand) || k > 1024)
        return fail(M3PC_EINVAL, "k %d outside [1, min(n_total, max(max_candidates, max_rescore), 1024)]", k);
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(h->device));
    launch_topk(expect_return, a->n_total, k, h->d_topk, st);
    CHK(m3pc_rescore(h, a, states, actions, rewards, eps, h->d_topk, k, nullptr, h->er_top, stream));
    launch_scatter(h->er_top, h->d_topk, k, expect_return, topk_index, st);
    return check_launch("rescore_topk");
}

int m3pc_topk_window(m3pc_handle* h, const float* expect_return, int n_total, int kmax, int kmin, float window, int* topk_index,
                     float* stats, float* top_scores, float* host_stats, float seq, void* stream) {
    if (!h || !expect_return || !topk_index || !stats) return fail(M3PC_EINVAL, "null argument");
    if (n_total < 1 || n_total > 16384) return fail(M3PC_EINVAL, "top-k supports n_total <= 16384");
    if (kmax < 1 || kmax > 1023 || kmin < 1 || kmin > kmax || !(window >= 0.f)) return fail(M3PC_EINVAL, "bad kmin/kmax/window");
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(h->device));
    const int kk = kmax + 1 < n_total ? kmax + 1 : n_total;
    launch_topk(expect_return, n_total, kk, topk_index, st);
    launch_window_stats(expect_return, n_total, topk_index, kk, kmin, kmax, window, stats, host_stats, seq, top_scores, st);
    return check_launch("topk_window");
}

int m3pc_topk_race_window(m3pc_handle* h, const float* expect_return, const float* expo, float temperature, int n_total, int kmax,
                          int kmin, int rmax, int* list, float* stats, float* list_scores, float* host_stats, float seq, void* stream) {
    if (!h || !expect_return || !expo || !list) return fail(M3PC_EINVAL, "null argument");
    if (n_total < 1 || n_total > 16384) return fail(M3PC_EINVAL, "top-k supports n_total <= 16384");
    if (kmax < 1 || kmax > 1023 || kmin < 1 || kmin > kmax) return fail(M3PC_EINVAL, "bad kmin/kmax");
    if (!stats && host_stats) return fail(M3PC_EINVAL, "host_stats needs stats");
    if (rmax < 1 || rmax > 64 || rmax > n_total) return fail(M3PC_EINVAL, "rmax %d outside [1, min(64, n_total)]", rmax);
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(h->device));
    const int kk = kmax + 1 < n_total ? kmax + 1 : n_total;
    const bool scored = launch_topk_race(expect_return, expo, temperature, n_total, kk, rmax, rmax, list, list_scores, st);
    // the statistics of the score part (and, beyond 2048 candidates, the listed scores) are a launch of their own: skipped when the
    // caller wants neither (the planner's certificate works on the merge's statistics)
    if (stats || (list_scores && !scored)) {
        if (!stats) stats = h->sel_scratch;
        launch_window_stats(expect_return, n_total, list + rmax, kk, kmin, kmax, 0.f, stats, host_stats, seq,
                            list_scores ? list_scores + rmax : nullptr, st, rmax);
    }
    return check_launch("topk_race_window");
}

int m3pc_rescore_merge(m3pc_handle* h, const float* scores, int n_total, const int* index, int n, const float* top_scores,
                       const float* top_rescored, float delta, float* merged, float* stats, float* host_stats, float seq,
                       void* stream) {
    if (!h || !scores || !index || !top_scores || !top_rescored || !merged || !stats) return fail(M3PC_EINVAL, "null argument");
    if (n_total < 1 || n < 1 || n > 1024 || n > n_total) return fail(M3PC_EINVAL, "n %d outside [1, min(1024, n_total)]", n);
    if (!(delta >= 0.f)) return fail(M3PC_EINVAL, "delta must be >= 0");
    HIPCHK(hipSetDevice(h->device));
    launch_rescore_merge(scores, n_total, index, 0, n, top_scores, top_rescored, delta, nullptr, 0.f, merged, stats, host_stats, seq,
                         (hipStream_t)stream);
    return check_launch("rescore_merge");
}

int m3pc_rescore_merge_race(m3pc_handle* h, const float* scores, const float* expo, float temperature, int n_total, const int* list,
                            int r, int n, const float* list_scores, const float* list_rescored, float delta, float* merged,
                            float* stats, float* host_stats, float seq, void* stream) {
    if (!h || !scores || !expo || !list || !list_scores || !list_rescored || !merged || !stats) return fail(M3PC_EINVAL, "null argument");
    if (n_total < 1 || n < 1 || r < 0 || r + n > 1024 || n > n_total || r > n_total)
        return fail(M3PC_EINVAL, "r %d + n %d outside [1, 1024] / n_total %d", r, n, n_total);
    if (!(delta >= 0.f)) return fail(M3PC_EINVAL, "delta must be >= 0");
    HIPCHK(hipSetDevice(h->device));
    launch_rescore_merge(scores, n_total, list, r, n, list_scores, list_rescored, delta, expo, temperature, merged, stats, host_stats,
                         seq, (hipStream_t)stream);
    return check_launch("rescore_merge_race");
}

int m3pc_merge_race_select(m3pc_handle* h, const float* scores, const float* expo, float temperature, int n_total, const int* list,
                           int r, int n, const float* list_scores, const float* list_rescored, float delta, float* merged,
                           float* stats, float* host_stats, float seq, const float* a0, long long a0_stride, float* p,
                           float* eval_action, int* argmax, int* sample_idx, float* sample_action, void* stream) {
    if (!h || !scores || !expo || !list || !list_scores || !list_rescored || !merged || !stats) return fail(M3PC_EINVAL, "null argument");
    if (n_total < 1 || n < 1 || r < 0 || r + n > 1024 || n > n_total || r > n_total)
        return fail(M3PC_EINVAL, "r %d + n %d outside [1, 1024] / n_total %d", r, n, n_total);
    if (!(delta >= 0.f)) return fail(M3PC_EINVAL, "delta must be >= 0");
    if ((eval_action || sample_action) && !a0) return fail(M3PC_EINVAL, "eval_action / sample_action need a0");
    HIPCHK(hipSetDevice(h->device));
    SelectP s;
    memset(&s, 0, sizeof(s));
    s.er = merged;
    s.a0 = a0;
    s.a0_stride = a0_stride;
    s.n = n_total;
    s.A = h->A;
    s.temperature = temperature;
    s.expo = expo;
    s.p = p;
    s.eval_action = eval_action;
    s.argmax = argmax;
    s.sample_idx = sample_idx;
    s.sample_action = sample_action;
    launch_merge_select(scores, n_total, list, r, n, list_scores, list_rescored, delta, expo, temperature, merged, stats, host_stats,
                        seq, s, (hipStream_t)stream);
    return check_launch("merge_race_select");
}

int m3pc_rescore_listed(m3pc_handle* h, const m3pc_plan_args* a, const float* states, const float* actions, const float* rewards,
                        const float* eps, const int* index, int n, float* expect_return, void* stream) {
    if (!h || !a || !expect_return || !index) return fail(M3PC_EINVAL, "null argument");
    if (n < 1 || n > 1024) return fail(M3PC_EINVAL, "n %d outside [1, 1024]", n);
    h->score_scatter_index = index;
    h->score_scatter_out = expect_return;
    const int rc = m3pc_rescore(h, a, states, actions, rewards, eps, index, n, nullptr, h->er_top, stream);
    h->score_scatter_index = nullptr;
    h->score_scatter_out = nullptr;
    if (rc) return rc;
    return check_launch("rescore_listed");
}

int m3pc_select(m3pc_handle* h, const float* expect_return, const float* a0, long long a0_stride, int n, float temperature,
                const float* expo, float* p, float* eval_action, int* argmax, int* sample_idx, float* sample_action,
                void* stream) {
    if (!h || !expect_return || n < 1) return fail(M3PC_EINVAL, "bad argument");
    if ((eval_action || sample_action) && !a0) return fail(M3PC_EINVAL, "eval_action / sample_action need a0");
    if ((sample_idx || sample_action) && !expo) return fail(M3PC_EINVAL, "the multinomial draw needs expo");
    HIPCHK(hipSetDevice(h->device));
    SelectP s;
    memset(&s, 0, sizeof(s));
    s.er = expect_return;
    s.a0 = a0;
    s.a0_stride = a0_stride;
    s.n = n;
    s.A = h->A;
    s.temperature = temperature;
    s.expo = expo;
    s.p = p;
    s.eval_action = eval_action;
    s.argmax = argmax;
    s.sample_idx = sample_idx;
    s.sample_action = sample_action;
    launch_select(s, (hipStream_t)stream);
    return check_launch("select");
}

int m3pc_eval_bound(m3pc_handle* h, const float* merged, int n_total, const int* list, int r, int n, int n_listed, const float* a0,
                    long long a0_stride, int A, float temperature, float delta, float eval_tol, float* stats, float* host_stats,
                    float seq, void* stream) {
    if (!h || !merged || !list || !a0 || !stats) return fail(M3PC_EINVAL, "null argument");
    if (!(eval_tol > 0.f)) return fail(M3PC_EINVAL, "eval_tol must be > 0 (+inf: report only)");
    if (!(delta >= 0.f)) return fail(M3PC_EINVAL, "delta must be >= 0");
    if (n_total < 1 || n_total > 16384) return fail(M3PC_EINVAL, "n_total %d outside [1, 16384]", n_total);
    if (A < 1 || A > 1024) return fail(M3PC_EINVAL, "A %d outside [1, 1024]", A);
    if (r < 0 || n_listed < 0 || r + n_listed > 1024) return fail(M3PC_EINVAL, "r %d + n_listed %d outside [0, 1024]", r, n_listed);
    if (n < 0 || n > n_listed) return fail(M3PC_EINVAL, "n %d outside [0, n_listed=%d]", n, n_listed);
    if (!(temperature == temperature)) return fail(M3PC_EINVAL, "temperature is not a number");
    HIPCHK(hipSetDevice(h->device));
    launch_eval_bound(merged, n_total, list, r, n, n_listed, a0, a0_stride, A, temperature, delta, eval_tol, stats, host_stats, seq,
                      (hipStream_t)stream);
    return check_launch("eval_bound");
}

// ---- the certified plan step as one call (learner.py:318-325 on low-precision scores that fp32 re-scores certify)
// The statistics of the kernel that carried `seq`, read from the slot's host-mapped block: a BOUNDED spin on the sequence number
// (10 s, the bound of the Python binding's HostStats.wait); on expiry one synchronisation of the stream and the device copy.
static int cert_wait_block(const volatile float* hs, const float* dev, float seq, int n_device, hipStream_t st, float out[8]) {
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    while (hs[4] != seq) {
        if ((++spins & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) {
            if (hipStreamSynchronize(st) != hipSuccess ||
                hipMemcpy(out, dev, 8 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
                return fail(M3PC_EHIP, "the statistics of the certified step reached neither host-mapped memory within 10 s nor the host by a copy");
            for (int i = n_device; i < 8; ++i) out[i] = 0.f;  // (a four-statistics merge leaves the device slots 4..7 alone)
            return 0;
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    for (int i = 0; i < 8; ++i) out[i] = hs[i];
    return 0;
}
static int cert_wait(m3pc_handle* h, int slot, float seq, int n_device, hipStream_t st, float out[8]) {
    return cert_wait_block(h->cert_host + 8 * slot, h->cert_stats[slot], seq, n_device, st, out);
}
static float cert_next_seq(m3pc_handle* h, int slot) {
    h->cert_seq[slot] = h->cert_seq[slot] % 1000000 + 1;
    return (float)h->cert_seq[slot];
}
// max(factor x the largest deviation from the median, 1e-6 x the scores' scale, 1e-30): the host arithmetic of
// HipPlanner._calibrate (doubles of the device's floats), rounded once to the float the ABI carries
static float cert_delta(float factor, float deviation, float f_max) {
    double d = (double)factor * (double)deviation;
    if (1e-6 * (double)f_max > d) d = 1e-6 * (double)f_max;
    if (1e-30 > d) d = 1e-30;
    return (float)d;
}
// one rank, every candidate: what both calls need of m3pc_plan_args before any HIP call
static int cert_check_args(const m3pc_plan_args* a, const char* who) {
    if (a->n_total < 1 || a->n_total > 16384) return fail(M3PC_EINVAL, "%s: n_total %d outside [1, 16384]", who, a->n_total);
    if (a->n_begin != 0 || a->n_count != a->n_total)
        return fail(M3PC_EINVAL, "%s plans on one rank: candidates [%d,+%d) are not all n_total=%d", who, a->n_begin, a->n_count, a->n_total);
    if (!precision_ok(a->precision)) return fail(M3PC_EINVAL, "bad precision %d", a->precision);
    if (a->slot < 0 || a->slot >= M3PC_SLOTS) return fail(M3PC_EINVAL, "slot %d outside [0, %d)", a->slot, M3PC_SLOTS);
    return 0;
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
static bool cert_any_begun(const m3pc_handle* h) {
    for (int s = 0; s < M3PC_SLOTS; ++s)
        if (h->cstep[s].begun) return true;
    return false;
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
            return m3pc_merge_race_select(h, S.scores_low, S.expo, temp, N, L + o, r, n, B + o, F + o, (float)S.delta, S.merged, dstats, hstats,
                                          S.seq, S.sample_actions, (long long)S.a.horizon * h->A, S.p, S.eval_action, S.argmax, S.sample_idx,
                                          S.sample_action, S.tail);
        return m3pc_rescore_merge_race(h, S.scores_low, S.expo, temp, N, L + o, r, n, B + o, F + o, (float)S.delta, S.merged, dstats, hstats,
                                       S.seq, S.tail);
    }
    CHK(m3pc_rescore_merge(h, S.scores_low, N, L, n, B, F, (float)S.delta, S.merged, dstats, hstats, S.seq, S.tail));
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
        S.n_done = cnt;
        CHK(cert_merge(h, S, cnt, S.r_done, false));
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
    S.n_done = N;
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
    S.delta = (double)S.c.delta;  // (1.5 x a float deviation needs 25 bits: kept as the double the Python protocol keeps)
    S.rounds = 0;
    S.n_done = kmin;
    S.r_done = rfirst;
    if (R > 0) CHK(m3pc_topk_race_window(h, S.scores_low, S.expo, S.c.temperature, N, kmax, kmin, R, L, nullptr, B, nullptr, 0.f, S.tail));
    else CHK(m3pc_topk_window(h, S.scores_low, N, kmax, kmin, 0.f, L, dstats + 8, B, nullptr, 0.f, S.tail));
    CHK(cert_rescore(h, S, R - rfirst, R + kmin));
    return cert_merge(h, S, kmin, rfirst, true);
}
// m3pc_amd/certificate.py:resolve -- read the certificates; raise delta when the re-scored set deviates by more than it
// allows; re-score what a certificate asks for; stop when both are satisfied or every candidate has been scored in fp32
// The eval_action certificate of m3pc_plan_step_certified_eval behind the step's last merge + select: the re-scored race entries
// and the listed score entries (kmax of them; behind a window set the list is wholly re-scored), under delta as it stands.
static int cert_eval_bound(m3pc_handle* h, CertStep& S, int n_listed, float eval_tol, float e8[8]) {
    const int slot = S.a.slot, R = S.c.rmax;
    float* dstats = h->cert_stats[slot] + 24;
    h->eval_seq[slot] = h->eval_seq[slot] % 1000000 + 1;
    const float seq = (float)h->eval_seq[slot];
    CHK(m3pc_eval_bound(h, S.merged, S.a.n_total, cert_L(h, S) + R - S.r_done, S.r_done, S.n_done, n_listed, S.sample_actions,
                        (long long)S.a.horizon * h->A, h->A, S.c.temperature, (float)S.delta, eval_tol, dstats, h->eval_host_dev + 8 * slot,
                        seq, S.tail));
    return cert_wait_block(h->eval_host + 8 * slot, dstats, seq, 8, S.tail, e8);
}
// eval_tol / erec: the third certificate (m3pc_plan_step_certified_eval); erec == NULL: the two certificates alone, nothing else
// launched, read or allocated
static int cert_resolve(m3pc_handle* h, CertStep& S, m3pc_cert_record* rec, float eval_tol = 0.f, m3pc_eval_record* erec = nullptr) {
    const int slot = S.a.slot, N = S.a.n_total, R = S.c.rmax, kmax = S.c.kmax;
    memset(rec, 0, sizeof(*rec));
    if (erec) memset(erec, 0, sizeof(*erec));
    if (S.a.precision == M3PC_PREC_FP32) {
        rec->n_rescored = N;
        rec->everything = rec->certified = 1;
        if (erec) erec->eval_certified = 1;
        return 0;
    }
    const int n_device = R > 0 ? 8 : 4;
    bool saturated = false, everything = false;
    int need = 0, need_race = 0;
    float s8[8];
    bool first = true;
    for (;;) {  // (one turn without erec; with it, a turn per extension the eval certificate asks for)
        for (;; first = false) {
            CHK(cert_wait(h, slot, S.seq, everything || R == 0 ? 4 : n_device, S.tail, s8));
            need = (int)s8[2];
            need_race = (int)s8[5];
            if (first) {
                rec->need_first = need;
                rec->need_race_first = need_race;
            }
            bool redo = false;
            if (S.c.grow_delta && 1.5 * (double)s8[1] > S.delta && !everything) {
                S.delta = 1.5 * (double)s8[1];
                redo = S.n_done < N;
            }
            if (everything || S.n_done >= N) break;
            if (!redo) {
                if (need > S.n_done && saturated) {  // the window set's certificate still asks for more: every candidate in fp32
                    CHK(cert_window_set(h, S, N, true));
                    everything = true;
                    continue;
                }
                if (need > S.n_done) {
                    if (need <= kmax) {
                        CHK(cert_rescore(h, S, R + S.n_done, R + need));
                        S.n_done = need;
                        redo = true;
                    } else {
                        CHK(cert_window_set(h, S, need, false));
                        saturated = true;
                        everything = S.n_done >= N;
                        continue;
                    }
                }
                if (need_race > S.r_done) {
                    if (need_race <= R) {
                        CHK(cert_rescore(h, S, R - need_race, R - S.r_done));
                        S.r_done = need_race;
                        redo = true;
                    } else {  // more racers than the race list holds: every candidate in fp32
                        CHK(cert_window_set(h, S, N, true));
                        saturated = everything = true;
                        continue;
                    }
                }
            }
            if (!redo) break;
            CHK(cert_merge(h, S, S.n_done, S.r_done, true));
        }
        first = false;
        if (!erec) break;
        if (everything || S.n_done >= N) {  // the select ran on fp32 scores alone
            erec->eval_bound = 0.f;
            erec->eval_certified = 1;
            break;
        }
        float e8[8];
        const int n_listed = saturated ? S.n_done : (kmax < N ? kmax : N);
        CHK(cert_eval_bound(h, S, n_listed, eval_tol, e8));
        const int need_eval = (int)e8[1];
        if (++erec->eval_rounds == 1) erec->need_eval_first = need_eval;
        erec->eval_bound = e8[0];
        if (need_eval <= S.n_done) {
            erec->eval_certified = 1;
            break;
        }
        if (need_eval <= n_listed) {  // score entries [n_done, need_eval), merge + select again, every certificate read again
            CHK(cert_rescore(h, S, R + S.n_done, R + need_eval));
            erec->n_eval += need_eval - S.n_done;
            S.n_done = need_eval;
            CHK(cert_merge(h, S, S.n_done, S.r_done, true));
        } else {  // the list cannot reach the tolerance: every candidate in fp32
            CHK(cert_window_set(h, S, N, true));
            everything = true;
        }
    }
    rec->n_rescored = S.n_done;
    rec->n_race = S.r_done;
    rec->saturated = saturated;
    rec->everything = everything;
    rec->certified = everything || S.n_done >= N || (need <= S.n_done && need_race <= S.r_done);
    rec->rounds = S.rounds;
    rec->delta = (float)S.delta;
    rec->shift = s8[0];
    rec->deviation = s8[1];
    rec->margin = s8[3];
    return 0;
}
static void cert_fill(CertStep& S, const m3pc_plan_args* a, const m3pc_cert_args* c, const float* states, const float* actions,
                      const float* rewards, const float* eps, const float* expo, float* sample_actions, float* scores_low, float* merged,
                      int* list, float* p, float* eval_action, int* argmax, int* sample_idx, float* sample_action, hipStream_t tail, bool async) {
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
        if (!h->eval_host && a->precision != M3PC_PREC_FP32) {  // the second host-mapped block of every slot, at the first such call
            HIPCHK(hipSetDevice(h->device));
            HIPCHK(hipHostMalloc((void**)&h->eval_host, (size_t)M3PC_SLOTS * 8 * sizeof(float), hipHostMallocMapped | hipHostMallocCoherent));
            memset(h->eval_host, 0, (size_t)M3PC_SLOTS * 8 * sizeof(float));
            HIPCHK(hipHostGetDevicePointer((void**)&h->eval_host_dev, h->eval_host, 0));
        }
    }
    CertStep& S = h->cstep[a->slot];
    cert_fill(S, a, c, states, actions, rewards, eps, expo, sample_actions, scores_low, merged, list, p, eval_action, argmax, sample_idx,
              sample_action, (hipStream_t)stream, false);

    // learner.py:278-316: policy pass (fp32), candidates, candidate pass in args->precision
    m3pc_plan_args pa = *a;
    pa.flags = a->flags & M3PC_PLAN_PRUNED_POLICY;
    pa.window = 0;
    CHK(m3pc_policy_pass(h, &pa, states, actions, rewards, nullptr, nullptr, stream));
    pa.flags = 0;
    CHK(m3pc_candidate_pass(h, &pa, states, actions, rewards, eps, loc, std_, sample_actions, scores_low, nullptr, nullptr, stream));
    CHK(cert_first_pass(h, S));
    return cert_resolve(h, S, rec, eval_tol, with_eval ? erec : nullptr);
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
    HIPCHK(hipEventRecord(h->step_ev[slot][3], S.tail));
    return 0;
}

int m3pc_plan_step_certified_begin(m3pc_handle* h, const m3pc_plan_args* a, const m3pc_cert_args* c, const float* states,
                                   const float* actions, const float* rewards, const float* eps, const float* expo, float* loc, float* std_,
                                   float* sample_actions, float* scores_low, float* merged, int* list, float* p, float* eval_action,
                                   int* argmax, int* sample_idx, float* sample_action, void* stream) {
    if (!h || !a || !c || !states || !actions || !rewards || !eps || !expo || !sample_actions || !scores_low || !merged)
        return fail(M3PC_EINVAL, "null argument");
    CHK(cert_check_step(a, c, "m3pc_plan_step_certified_begin"));
    const int slot = a->slot;
    CertStep& S = h->cstep[slot];
    if (S.begun) return fail(M3PC_ESTATE, "m3pc_plan_step_certified_begin: the step in slot %d has not been ended", slot);
    HIPCHK(hipSetDevice(h->device));
    CHK(step_setup(h));
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
              sample_action, chain, true);
    S.tail_pending = true;
    S.begun = true;
    S.order = ++h->step_order;
    return 0;
}

int m3pc_plan_step_certified_end(m3pc_handle* h, int slot, m3pc_cert_record* rec, void* stream) {
    if (!h || !rec) return fail(M3PC_EINVAL, "null argument");
    if (slot < 0 || slot >= M3PC_SLOTS) return fail(M3PC_EINVAL, "slot %d outside [0, %d)", slot, M3PC_SLOTS);
    CertStep& S = h->cstep[slot];
    if (!S.begun) return fail(M3PC_ESTATE, "m3pc_plan_step_certified_end: no step begun in slot %d", slot);
    HIPCHK(hipSetDevice(h->device));
    S.begun = false;  // (whatever happens below, the slot is free again)
    if (S.tail_pending) CHK(step_enqueue_tail(h, slot));
    const int rounds = S.rounds;
    CHK(cert_resolve(h, S, rec));
    if (S.rounds != rounds) HIPCHK(hipEventRecord(h->step_ev[slot][3], S.tail));
    HIPCHK(hipStreamWaitEvent((hipStream_t)stream, h->step_ev[slot][3], 0));
    return 0;
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
    W.seq_w.assign(E, 0.f);
    W.ready = true;
    return 0;
}
static float ls_next_seq(Lockstep& W) {
    W.seq = W.seq % 1000000 + 1;
    return (float)W.seq;
}
// cert_wait for the windows [w0, w1): ONE bounded spin until block w holds the sequence number issued last for window w (seq_w),
// for all of them; on expiry one synchronisation of the stream and the device copies.  out: 8 floats per window.
static int ls_wait(m3pc_handle* h, int w0, int w1, int n_device, hipStream_t st, float* out) {
    Lockstep& W = h->ls;
    const volatile float* hs = W.host;
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    for (int w = w0; w < w1; ++w)
        while (hs[8 * w + 4] != W.seq_w[w]) {
            if ((++spins & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) {
                if (hipStreamSynchronize(st) != hipSuccess ||
                    hipMemcpy(out, W.stats + 8 * w0, (size_t)(w1 - w0) * 8 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
                    return fail(M3PC_EHIP, "the statistics of the lock-step batch reached neither host-mapped memory within 10 s nor the host by a copy");
                for (int v = 0; v < w1 - w0; ++v)
                    for (int i = n_device; i < 8; ++i) out[8 * v + i] = 0.f;
                return 0;
            }
        }
    std::atomic_thread_fence(std::memory_order_acquire);
    for (int i = 8 * w0; i < 8 * w1; ++i) out[i - 8 * w0] = hs[i];
    return 0;
}

int m3pc_plan_steps_certified(m3pc_handle* h, const m3pc_plan_args* a, const m3pc_cert_args* c, int n_windows, const float* states,
                              const float* actions, const float* rewards, const double* rtg, const float* eps, const float* expo,
                              float* loc, float* std_, float* sample_actions, float* scores_low, float* merged, int* list, float* p,
                              float* eval_action, int* argmax, int* sample_idx, float* sample_action, m3pc_cert_record* records,
                              void* stream) {
    static const char* who = "m3pc_plan_steps_certified";
    if (!h || !a || !c || !states || !actions || !rewards || !rtg || !eps || !expo || !sample_actions || !scores_low || !merged || !records)
        return fail(M3PC_EINVAL, "null argument");
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
            records[w].n_rescored = N;
            records[w].everything = records[w].certified = 1;
        }
        return check_launch(who);
    }

    const int R = c->rmax, kmin = c->kmin, kmax = c->kmax, rfirst = c->rfirst, LS = R + 1024, m0 = rfirst + kmin;
    const int kk = kmax + 1 < N ? kmax + 1 : N, cap = h->chain[0].max_cand;
    int* L = list ? list : W.list;  // rows of LS entries, as are B and F
    float *B = W.b, *F = W.f;
    auto Lw = [&](int w) { return L + (size_t)w * LS; };
    auto Bw = [&](int w) { return B + (size_t)w * LS; };
    auto Fw = [&](int w) { return F + (size_t)w * LS; };
    auto low = [&](int w) { return scores_low + (size_t)w * N; };
    auto scratch = [&](int w) { return W.stats + 8 * (size_t)h->dm.max_batch + 16 * (size_t)w; };
    // lockstep.py:93-100: the lists of every window (the kmax + 1 best by score, the rmax best by race key) in one launch
    if (!launch_topk_race_batch(scores_low, expo, temp, E, N, N, kk, R, R, L, B, LS, st)) {
        for (int w = 0; w < E; ++w)  // (the device refused the LDS of the batched ranking: the one-window launches, same lists)
            if (!launch_topk_race(low(w), R > 0 ? expo + (size_t)w * N : nullptr, temp, N, kk, R, R, Lw(w), Bw(w), st))
                launch_window_stats(low(w), N, Lw(w) + R, kk, kmin, kmax, 0.f, scratch(w), nullptr, 0.f, Bw(w) + R, st, R);
    }
    // lockstep.py:106-110: list positions [rmax - rfirst, rmax + kmin) of every window, window-major, in ONE fp32 scoring pass
    launch_gather_listed(sample_actions, E, N, (int)row, L, LS, R - rfirst, m0, W.cand, W.widx, st);
    CHK(check_launch(who));
    m3pc_plan_args sa = *a;
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
    for (int w = 0; w < E; ++w) {
        W.seq_w[w] = seq0;
        records[w].rounds = 1;
    }
    // (the re-scores into the list's layout, where the one-window merges behind the certificates read them)
    HIPCHK(hipMemcpy2DAsync(F + (R - rfirst), (size_t)LS * sizeof(float), W.fs, (size_t)m0 * sizeof(float), (size_t)m0 * sizeof(float), E,
                            hipMemcpyDeviceToDevice, st));
    CHK(check_launch(who));
    CHK(ls_wait(h, 0, E, R > 0 ? 8 : 4, st, s8.data()));  // the ONE host wait of the first pass: E sequence numbers

    // ---- per window, ascending: certificate.py:resolve with the device work of _WindowOps
    auto select_w = [&](int w, const float* er) -> int {
        return m3pc_select(h, er, sample_actions + w * N * row, row, N, temp, expo + (size_t)w * N, p ? p + (size_t)w * N : nullptr,
                           eval_action ? eval_action + (size_t)w * A : nullptr, argmax ? argmax + w : nullptr,
                           sample_idx ? sample_idx + w : nullptr, sample_action ? sample_action + (size_t)w * A : nullptr, stream);
    };
    auto merge_w = [&](int w, int n, int r, double delta) -> int {  // _WindowOps.merge_select
        const int o = R - r;
        float *mw = merged + (size_t)w * N, *dst = W.stats + 8 * (size_t)w, *hst = W.host_dev + 8 * (size_t)w;
        W.seq_w[w] = ls_next_seq(W);
        ++records[w].rounds;
        if (R > 0)
            return m3pc_merge_race_select(h, low(w), expo + (size_t)w * N, temp, N, Lw(w) + o, r, n, Bw(w) + o, Fw(w) + o, (float)delta, mw, dst,
                                          hst, W.seq_w[w], sample_actions + w * N * row, row, p ? p + (size_t)w * N : nullptr,
                                          eval_action ? eval_action + (size_t)w * A : nullptr, argmax ? argmax + w : nullptr,
                                          sample_idx ? sample_idx + w : nullptr, sample_action ? sample_action + (size_t)w * A : nullptr, stream);
        CHK(m3pc_rescore_merge(h, low(w), N, Lw(w), n, Bw(w), Fw(w), (float)delta, mw, dst, hst, W.seq_w[w], stream));
        return select_w(w, mw);
    };
    auto rescore_w = [&](int w, int lo, int hi) -> int {  // _WindowOps._score: list positions [lo, hi), chunks of max_rescore
        for (int c0 = lo; c0 < hi; c0 += cap) {
            const int m = hi - c0 < cap ? hi - c0 : cap;
            launch_gather_listed(sample_actions + w * N * row, 1, N, (int)row, Lw(w), LS, c0, m, W.cand, nullptr, st);
            sa.n_total = sa.n_count = m;
            CHK(m3pc_score_actions(h, &sa, 1, states + (size_t)w * T * S, actions + (size_t)w * T * A, rewards + (size_t)w * T, W.cand, nullptr,
                                   Fw(w) + c0, nullptr, nullptr, stream));
        }
        return 0;
    };
    auto window_set_w = [&](int w, int need, bool everything, double delta) -> int {  // _WindowOps.window_set
        const int cnt = need < N ? need : N;
        if (cnt <= 1024 - 32 && !everything) {
            if (!launch_topk_race(low(w), nullptr, 0.f, N, cnt, 0, R, Lw(w), Bw(w), st))
                launch_window_stats(low(w), N, Lw(w) + R, cnt, 1, cnt, 0.f, scratch(w), nullptr, 0.f, Bw(w) + R, st, 0);
            CHK(check_launch("plan_steps_certified (window set)"));
            CHK(rescore_w(w, R, R + cnt));
            n_done[w] = cnt;
            return merge_w(w, cnt, r_done[w], delta);
        }
        float* f32 = h->cert_f32[slot];
        int* top1 = h->cert_top1[slot];
        float *top1v = scratch(w) + 8, *mw = merged + (size_t)w * N;
        sa.n_total = sa.n_count = N;
        CHK(m3pc_score_actions(h, &sa, 1, states + (size_t)w * T * S, actions + (size_t)w * T * A, rewards + (size_t)w * T,
                               sample_actions + w * N * row, nullptr, f32, nullptr, nullptr, stream));
        if (!launch_topk_race(f32, nullptr, 0.f, N, 1, 0, 0, top1, top1v, st))
            launch_window_stats(f32, N, top1, 1, 1, 1, 0.f, scratch(w), nullptr, 0.f, top1v, st, 0);
        CHK(check_launch("plan_steps_certified (every candidate in fp32)"));
        n_done[w] = N;  // (r_done stays: the record's n_race is what resolve counted, as in the Python protocol)
        W.seq_w[w] = ls_next_seq(W);
        ++records[w].rounds;
        CHK(m3pc_rescore_merge(h, f32, N, top1, 1, top1v, top1v, 0.f, mw, W.stats + 8 * (size_t)w, W.host_dev + 8 * (size_t)w, W.seq_w[w], stream));
        return select_w(w, mw);
    };

    double delta = (double)c->delta;  // (1.5 x a float deviation needs 25 bits: the double the Python protocol keeps)
    const double delta_first = delta;
    for (int w = 0; w < E; ++w) {
        m3pc_cert_record* rec = records + w;
        float* s = s8.data() + 8 * (size_t)w;
        bool have = true;  // the statistics of the window's last merge are on the host already
        if (delta > delta_first) {  // an earlier window raised the bound: this window's certificate again, under it
            CHK(merge_w(w, n_done[w], r_done[w], delta));
            have = false;
        }
        bool saturated = false, everything = false;
        int need = 0, need_race = 0;
        for (bool first = true;; first = false) {
            if (!have) CHK(ls_wait(h, w, w + 1, everything || R == 0 ? 4 : 8, st, s));
            have = false;
            need = (int)s[2];
            need_race = (int)s[5];
            if (first) {
                rec->need_first = need;
                rec->need_race_first = need_race;
            }
            bool redo = false;
            if (c->grow_delta && 1.5 * (double)s[1] > delta && !everything) {
                delta = 1.5 * (double)s[1];
                redo = n_done[w] < N;
            }
            if (everything || n_done[w] >= N) break;
            if (!redo) {
                if (need > n_done[w] && saturated) {  // the window set's certificate still asks for more: every candidate in fp32
                    CHK(window_set_w(w, N, true, delta));
                    everything = true;
                    continue;
                }
                if (need > n_done[w]) {
                    if (need <= kmax) {
                        CHK(rescore_w(w, R + n_done[w], R + need));
                        n_done[w] = need;
                        redo = true;
                    } else {
                        CHK(window_set_w(w, need, false, delta));
                        saturated = true;
                        everything = n_done[w] >= N;
                        continue;
                    }
                }
                if (need_race > r_done[w]) {
                    if (need_race <= R) {
                        CHK(rescore_w(w, R - need_race, R - r_done[w]));
                        r_done[w] = need_race;
                        redo = true;
                    } else {  // more racers than the race list holds: every candidate in fp32
                        CHK(window_set_w(w, N, true, delta));
                        saturated = everything = true;
                        continue;
                    }
                }
            }
            if (!redo) break;
            CHK(merge_w(w, n_done[w], r_done[w], delta));
        }
        rec->n_rescored = n_done[w];
        rec->n_race = r_done[w];
        rec->saturated = saturated;
        rec->everything = everything;
        rec->certified = everything || n_done[w] >= N || (need <= n_done[w] && need_race <= r_done[w]);
        rec->delta = (float)delta;
        rec->shift = s[0];
        rec->deviation = s[1];
        rec->margin = s[3];
    }
    return 0;
}

int m3pc_draw_variates(m3pc_handle* h, unsigned long long seed, unsigned long long step, int n_begin, int n_count, int row_elems,
                       float* eps, float* expo, void* stream) {
    if (!h) return fail(M3PC_EINVAL, "null handle");
    if (n_begin < 0 || n_count < 1 || row_elems < 1 || (long long)n_begin + n_count > (1LL << 31) - 1 ||
        ((long long)n_begin + n_count) * row_elems > (1LL << 33))
        return fail(M3PC_EINVAL, "m3pc_draw_variates: rows [%d,+%d) of %d elements outside the generator's range", n_begin, n_count, row_elems);
    HIPCHK(hipSetDevice(h->device));
    launch_variates(seed, step, 0, (long long)n_begin * row_elems, ((long long)n_begin + n_count) * row_elems, eps, (hipStream_t)stream);
    launch_variates(seed, step, 1, n_begin, (long long)n_begin + n_count, expo, (hipStream_t)stream);
    return check_launch("draw_variates");
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

// ---- CEM / MPPI refinement of a plan (include/m3pc_hip.h: m3pc_refit_resample, m3pc_refine_plan; kernels: refine.hip)
static bool finite_nonneg(float v) { return v >= 0.f && v <= 3.402823466e+38f; }
// weighting / temperature / min_std of a refit, before any HIP call
static int refine_check_refit(int weighting, float temperature, float min_std, const char* who) {
    if (weighting != M3PC_REFINE_CEM && weighting != M3PC_REFINE_MPPI)
        return fail(M3PC_EINVAL, "%s: weighting %d is neither M3PC_REFINE_CEM nor M3PC_REFINE_MPPI", who, weighting);
    if (weighting == M3PC_REFINE_MPPI && !finite_nonneg(temperature)) return fail(M3PC_EINVAL, "%s: temperature must be finite and >= 0", who);
    if (!finite_nonneg(min_std)) return fail(M3PC_EINVAL, "%s: min_std must be finite and >= 0", who);
    return 0;
}

int m3pc_refit_resample(m3pc_handle* h, const float* cand, int n, int horizon, const float* scores, const int* elites, int k, int weighting,
                        float temperature, float min_std, const float* noise, float* mean, float* std_, float* cand_out, void* stream) {
    if (!h || !cand || !elites || !mean || !std_) return fail(M3PC_EINVAL, "null argument");
    if (n < 1 || n > 16384) return fail(M3PC_EINVAL, "m3pc_refit_resample: n %d outside [1, 16384]", n);
    if (k < 1 || k > n) return fail(M3PC_EINVAL, "m3pc_refit_resample: k %d outside [1, n=%d]", k, n);
    if (horizon < 1) return fail(M3PC_EINVAL, "m3pc_refit_resample: horizon %d < 1", horizon);
    CHK(refine_check_refit(weighting, temperature, min_std, "m3pc_refit_resample"));
    if (weighting == M3PC_REFINE_MPPI && !scores) return fail(M3PC_EINVAL, "m3pc_refit_resample: M3PC_REFINE_MPPI needs scores");
    if ((noise == nullptr) != (cand_out == nullptr)) return fail(M3PC_EINVAL, "m3pc_refit_resample: noise and cand_out are given together or not at all");
    if (horizon > h->T) return fail(M3PC_EINVAL, "horizon %d outside [1, T=%d]", horizon, h->T);
    const long long total = (long long)n * horizon * h->A;
    if (total > (1LL << 30)) return fail(M3PC_EINVAL, "m3pc_refit_resample: %lld candidate elements > 2^30", total);
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    RefitP rp;
    memset(&rp, 0, sizeof(rp));
    rp.cand = cand;
    rp.elite = elites;
    rp.scores = scores;
    rp.n = n;
    rp.k = k;
    rp.C = horizon * h->A;
    rp.weighting = weighting;
    rp.tau = temperature;
    rp.min_std = min_std;
    rp.mean = mean;
    rp.std = std_;
    launch_refit(rp, st);
    if (noise) {
        ResampleP sp;
        memset(&sp, 0, sizeof(sp));
        sp.mean = mean;
        sp.std = std_;
        sp.noise = noise;
        sp.out = cand_out;
        sp.total = (int)total;
        sp.C = rp.C;
        sp.A = h->A;
        launch_resample(sp, st);
    }
    return check_launch("refit_resample");
}

int m3pc_refine_plan(m3pc_handle* h, const m3pc_plan_args* a, const m3pc_refine_args* r, const float* states, const float* actions,
                     const float* rewards, const float* init_mean, const float* noise, float* mean, float* std_, float* candidates,
                     float* scores, int* elites, float* sample_action, float* eval_action, void* stream) {
    if (!h || !a || !r || !states || !actions || !rewards || !mean || !std_ || !candidates) return fail(M3PC_EINVAL, "null argument");
    CHK(cert_check_args(a, "m3pc_refine_plan"));
    if (a->mode != M3PC_MODE_RTG && a->mode != M3PC_MODE_CRITIC) return fail(M3PC_EINVAL, "m3pc_refine_plan: mode must be RTG or CRITIC scoring");
    if (a->horizon < 1) return fail(M3PC_EINVAL, "m3pc_refine_plan: horizon %d < 1", a->horizon);
    if (a->flags & ~M3PC_PLAN_PRUNED_POLICY)
        return fail(M3PC_EINVAL, "m3pc_refine_plan: m3pc_plan_args::flags 0x%x holds more than M3PC_PLAN_PRUNED_POLICY", a->flags);
    if (r->iterations < 1 || r->iterations > M3PC_REFINE_MAX_ITER)
        return fail(M3PC_EINVAL, "m3pc_refine_plan: iterations %d outside [1, %d]", r->iterations, M3PC_REFINE_MAX_ITER);
    if (r->top_k < 1 || r->top_k > a->n_total) return fail(M3PC_EINVAL, "m3pc_refine_plan: top_k %d outside [1, n_total=%d]", r->top_k, a->n_total);
    CHK(refine_check_refit(r->weighting, r->temperature, r->min_std, "m3pc_refine_plan"));
    if (!finite_nonneg(r->init_std)) return fail(M3PC_EINVAL, "m3pc_refine_plan: init_std must be finite and >= 0");
    if (cert_any_begun(h)) return fail(M3PC_ESTATE, "m3pc_refine_plan with a pipelined step begun (m3pc_plan_step_certified_end first)");
    if (a->mode == M3PC_MODE_CRITIC && !h->critic_set) return fail(M3PC_ESTATE, "critic weights not set");
    const int N = a->n_total, k = r->top_k, T = h->T, hh = a->horizon;
    if (N > h->dm.max_candidates) return fail(M3PC_ENOMEM, "n_total %d > max_candidates %d", N, h->dm.max_candidates);
    if (hh > T) return fail(M3PC_EINVAL, "horizon %d outside [1, T=%d]", hh, T);
    hipStream_t st = (hipStream_t)stream;
    const int C = hh * h->A;
    const long long total = (long long)N * C;  // (<= max_candidates * T * A: what the workspace holds)

    // learner.py:278-284: the policy pass; leaves the slot's policy head and returns tokens (the scoring reads the latter)
    m3pc_plan_args pa = *a;
    pa.window = 0;
    CHK(m3pc_policy_pass(h, &pa, states, actions, rewards, nullptr, nullptr, stream));
    pa.flags = 0;

    const unsigned long long seed = ((unsigned long long)r->seed_hi << 32) | r->seed_lo, step = ((unsigned long long)r->step_hi << 32) | r->step_lo;
    // the noise of iteration `it`: the caller's slice, or that slice of the (seed, step) array drawn into the handle's buffer
    auto noise_of = [&](int it) -> const float* {
        if (noise) return noise + (size_t)it * total;
        launch_variates(seed, step, 0, (long long)it * total, (long long)(it + 1) * total, h->refine_noise, st);
        return h->refine_noise;
    };
    ResampleP sp;
    memset(&sp, 0, sizeof(sp));
    sp.out = candidates;
    sp.total = (int)total;
    sp.C = C;
    sp.A = h->A;
    // distribution 0: the caller's mean or tanh of the policy head over the last h steps, std = init_std; candidates from it
    sp.mean = init_mean;
    sp.loc = h->loc + (size_t)(T - hh) * h->A;
    sp.std_const = r->init_std;
    sp.noise = noise_of(0);
    sp.mean_out = mean;
    sp.std_out = std_;
    launch_resample(sp, st);
    CHK(check_launch("refine_plan"));
    sp.mean_out = sp.std_out = nullptr;
    for (int it = 0; it < r->iterations; ++it) {
        float* er = scores ? scores + (size_t)it * N : h->refine_scores;
        int* top = elites ? elites + (size_t)it * k : h->refine_elites;
        CHK(m3pc_score_actions(h, &pa, 1, states, actions, rewards, candidates, nullptr, er, nullptr, nullptr, stream));
        launch_topk(er, N, k, top, st);
        RefitP rp;
        memset(&rp, 0, sizeof(rp));
        rp.cand = candidates;
        rp.elite = top;
        rp.scores = er;
        rp.n = N;
        rp.k = k;
        rp.C = C;
        rp.weighting = r->weighting;
        rp.tau = r->temperature;
        rp.min_std = r->min_std;
        rp.mean = mean + (size_t)(it + 1) * C;
        rp.std = std_ + (size_t)(it + 1) * C;
        launch_refit(rp, st);
        sp.mean = rp.mean;
        sp.std = rp.std;
        sp.noise = noise_of(it + 1);
        if (it == r->iterations - 1) {  // what cem_guiding returns: candidate 0's first action, the final mean's first action
            sp.sample_action = sample_action;
            sp.eval_action = eval_action;
        }
        launch_resample(sp, st);
        CHK(check_launch("refine_plan"));
    }
    return 0;
}

#ifdef M3PC_LAB  // ---- kernel-level test / bench hooks: libm3pc_hip_lab.so only, declared in include/m3pc_hip_debug.h
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

// Not part of the public header (tests/test_gemm_kernels_gpu.py): the top-k kernels on their own.
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
int m3pc_debug_topk(const float* v, int n, int k, int* idx_out, void* stream) {
    launch_topk(v, n, k, idx_out, (hipStream_t)stream);
    return check_launch("debug_topk");
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
int m3pc_debug_embed(const m3pc_debug_embed_args* a) {
    if (!a) return fail(M3PC_EINVAL, "debug_embed: null arguments");
    if (a->batch < 1 || a->L < 1 || a->d % 256 != 0 || a->d < 256 || a->d > 1024 || !a->tokmap) return fail(M3PC_EINVAL, "debug_embed: batch / L / d / tokmap");
    if (a->n_indep < 0 || a->n_indep > a->L || a->n_sh < 0 || a->n_sh > a->n_indep) return fail(M3PC_EINVAL, "debug_embed: n_indep / n_sh");
    if (!a->X == !a->Xb) return fail(M3PC_EINVAL, "debug_embed: exactly one of X / Xb");
    if (a->x_compact && !(a->Xb && a->x_first_only && a->n_indep > 0)) return fail(M3PC_EINVAL, "debug_embed: x_compact needs Xb, x_first_only and n_indep > 0");
    if ((a->Hb || a->n_sh) && (!a->ln_g || !a->ln_b)) return fail(M3PC_EINVAL, "debug_embed: Hb without ln_g / ln_b");
    if (a->n_sh > 0 && (!a->Hb || !a->Hb_sh)) return fail(M3PC_EINVAL, "debug_embed: n_sh without Hb / Hb_sh");
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
    e.Hb = (bf16_t*)a->Hb;
    e.Hb_sh = (bf16_t*)a->Hb_sh;
    e.n_indep = a->n_indep;
    e.n_sh = a->n_sh;
    e.x_first_only = a->x_first_only ? 1 : 0;
    e.x_compact = a->x_compact ? 1 : 0;
    launch_embed(e, (hipStream_t)a->stream);
    return check_launch("debug_embed");
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

#endif  // M3PC_LAB

int m3pc_profile_enable(m3pc_handle* h, int enable) {
    if (!h) return fail(M3PC_EINVAL, "null handle");
    h->prof = enable == 1 || enable == 2;
    h->prof_serial = enable == 2 || enable == 3;
    return 0;
}

int m3pc_profile_read(m3pc_handle* h, int precision, long long* launches, double* gemm_ms, double* gemm_flops, int reset) {
    if (!h) return fail(M3PC_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    double ms = 0, fl = 0;
    long long cnt = 0;
    for (size_t i = 0; i < h->ev_used; ++i) {
        if (precision == M3PC_PROF_LAYER_TAIL) {
            if (h->ev[i].kind != 1) continue;
        } else if (precision >= 0 && h->ev[i].dt != gemm_dt(precision)) {
            continue;
        }
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, h->ev[i].a, h->ev[i].b));
        ms += t;
        fl += h->ev[i].flops;
        ++cnt;
    }
    if (launches) *launches = cnt;
    if (gemm_ms) *gemm_ms = ms;
    if (gemm_flops) *gemm_flops = fl;
    if (reset) h->ev_used = 0;
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
