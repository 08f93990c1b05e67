// The shared front end of the masked-trajectory calls (mtm_batch.h).  Host code only.
#include "iql.h"
#include "mtm_loss.h"

namespace m3pc {

int mb_check(const m3pc_dims& dm, int max_batch, int batch, const unsigned char* const masks[4], int flags, int loss_keys, const char* who,
             bool refuse_all_hidden, unsigned long long bits[4]) {
    if (batch < 1 || batch > max_batch) return fail(M3PC_EINVAL, "%s: batch %d outside [1, max_batch=%d]", who, batch, max_batch);
    if (flags & ~(M3PC_MTM_NORM_L2 | M3PC_MTM_CLIP_ACTIONS)) return fail(M3PC_EINVAL, "%s: unknown flag bits 0x%x", who, flags);
    if (loss_keys < 0 || loss_keys > 15) return fail(M3PC_EINVAL, "%s: loss_keys %d outside [0, 15]", who, loss_keys);
    const int T = dm.traj_length;
    if (T < 1 || T > 64) return fail(M3PC_EINVAL, "%s: traj_length %d outside [1, 64]", who, T);
    unsigned long long any = 0;
    for (int k = 0; k < 4; ++k) {
        if (!masks[k]) return fail(M3PC_EINVAL, "%s: null mask of '%s'", who, KEYN[k]);
        bits[k] = 0;
        for (int t = 0; t < T; ++t) {
            if (masks[k][t] > 1) return fail(M3PC_EINVAL, "%s: mask byte %d of '%s' is %d, not 0 or 1", who, t, KEYN[k], (int)masks[k][t]);
            bits[k] |= (unsigned long long)masks[k][t] << t;
        }
        any |= bits[k];
    }
    if (refuse_all_hidden && !any) return fail(M3PC_EINVAL, "%s: mask keeps no token", who);
    return 0;
}

int mb_fits(const m3pc_handle* h, const m3pc_replay* rb, const char* who) {
    int S = 0, A = 0, dev = 0;
    replay_sizes(rb, &S, &A, &dev);
    const int L = replay_segment_length(rb);
    if (S != h->dm.state_dim || A != h->dm.action_dim || dev != h->device || L != h->dm.traj_length)
        return fail(M3PC_EINVAL, "%s: the buffer (S %d, A %d, segment_length %d, device %d) does not fit the handle (%d, %d, T %d, %d)", who,
                    S, A, L, dev, h->dm.state_dim, h->dm.action_dim, h->dm.traj_length, h->device);
    return 0;
}

int mb_state(const m3pc_handle* h, const char* who) {
    if (!h->weights_loaded) return fail(M3PC_ESTATE, "%s: weights not loaded", who);
    for (int k = 0; k < 4; ++k)
        if (!h->tok_set[k]) return fail(M3PC_ESTATE, "%s: tokenizer '%s' not set", who, KEYN[k]);
    return 0;
}

int mb_draw(m3pc_handle* h, const MtmStage& s, m3pc_replay* rb, int batch, int mode, const int* traj_index, const int* start_index,
            int index_on_device, unsigned long long seed, unsigned long long step, const float** eps, int* out_traj, int* out_start,
            hipStream_t st, const char* who) {
    CHK(m3pc_replay_sample_segments(rb, batch, mode, traj_index, start_index, index_on_device, seed, step, s.raw[0], s.raw[1], s.raw[2],
                                    s.raw_returns, 0, out_traj, out_start, (void*)st));
    if (!*eps) {
        launch_variates(seed, step, 0, 0, (long long)batch * h->T * h->A, s.eps, st);
        CHK(check_launch((std::string(who) + " variates").c_str()));
        *eps = s.eps;
    }
    return 0;
}

void mb_tokenize(m3pc_handle* h, const MtmStage& s, int batch, const float* states, const float* actions, const float* rewards, const void* returns,
                 int returns_f64, hipStream_t st) {
    const long long rows = (long long)batch * h->T;
    const void* raw[4] = {states, actions, rewards, returns};
    for (int k = 0; k < 4; ++k)
        launch_tokenize(raw[k], k == M3PC_RETURNS ? (returns_f64 ? 1 : 0) : 0, s.tok[k], rows, h->feat[k], h->tok_mean[k], h->tok_std[k],
                        h->tok_norm[k], st);
}

void mb_loss(const m3pc_handle* h, const MtmStage& s, int batch, const float* const pred[5], const float* const tgt[4],
             const unsigned long long bits[4], const float* eps, float entropy_reg, const float* entropy_reg_p, int flags, int loss_keys,
             float* record, hipStream_t st) {
    MtmLossP p;
    memset(&p, 0, sizeof(p));
    for (int j = 0; j < 3; ++j) p.pred[j] = pred[j];
    p.mu = pred[3];
    p.sd = pred[4];
    for (int k = 0; k < 4; ++k) {
        p.tgt[k] = tgt[k];
        p.mask[k] = bits[k];
    }
    p.eps = eps;
    p.batch = batch;
    p.T = h->T;
    p.S = h->S;
    p.A = h->A;
    p.flags = flags;
    p.loss_keys = loss_keys;
    p.entropy_reg = entropy_reg;
    p.entropy_reg_p = entropy_reg_p;
    p.part = s.part;
    p.record = record;
    launch_mtm_loss(p, st);
}

int nt_check(const m3pc_named_tensor* tensors, int n, const std::function<long long(const char*)>& numel_of, const char* who, const char* noun) {
    for (int i = 0; i < n; ++i) {
        const m3pc_named_tensor& t = tensors[i];
        if (!t.name || !t.data) return fail(M3PC_EINVAL, "%s: entry %d has no name or no data", who, i);
        const long long numel = numel_of(t.name);
        if (numel < 0) return fail(M3PC_EINVAL, "%s: '%s' is not a %s", who, t.name, noun);
        if (t.numel != numel) return fail(M3PC_EINVAL, "%s: '%s' has %lld elements, expected %lld", who, t.name, t.numel, numel);
    }
    return 0;
}

int nt_copy(const m3pc_named_tensor* tensors, int n, bool to_caller, const std::function<float*(const char*)>& at, hipStream_t st) {
    for (int i = 0; i < n; ++i) {
        const m3pc_named_tensor& t = tensors[i];
        float* ours = at(t.name);
        const size_t bytes = (size_t)t.numel * sizeof(float);
        if (to_caller)
            HIPCHK(hipMemcpyAsync(const_cast<float*>(t.data), ours, bytes, t.on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
        else
            HIPCHK(hipMemcpyAsync(ours, t.data, bytes, t.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    }
    return 0;
}

}  // namespace m3pc
