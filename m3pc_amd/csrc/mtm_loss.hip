// The masked-trajectory loss (include/m3pc_hip.h: m3pc_mtm_loss_terms, m3pc_mtm_loss, m3pc_mtm_loss_replay).  mtm_loss.h states the
// arithmetic, the reduction order and the record.  Two launches behind the forward's.
#include "device_util.h"
#include "mtm_loss.h"

namespace m3pc {
namespace {

constexpr int ML_THREADS = 256;

// Normal(mu, sd).log_prob(x) minus TanhTransform.log_abs_det_jacobian(x, .): what TransformedDistribution.log_prob adds up for the
// pre-tanh value x
__device__ __forceinline__ float squashed_log_prob(float x, float mu, float sd) {
    const float var = sd * sd;
    const float d = x - mu;
    const float normal = ((-(d * d)) / (2.0f * var) - logf(sd)) - 0.91893853320467274178f;  // log(sqrt(2 pi))
    const float y = -2.0f * x;
    const float softplus = y > 20.0f ? y : log1pf(expf(y));
    const float ladj = 2.0f * ((0.69314718055994530942f - x) - softplus);
    return normal - ladj;
}

// One wavefront per row r = (b, t); lanes run over the features of one key after the other (S, A <= 32 today; the loops take any
// width).  Lane 0 writes the row's six sums.
__global__ __launch_bounds__(ML_THREADS) void mtm_loss_rows_kernel(MtmLossP p) {
    const int r = blockIdx.x * (ML_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int rows = p.batch * p.T;
    if (r >= rows) return;  // (whole wavefronts leave: the butterflies below run with all 64 lanes)
    double out[MTM_LOSS_PART];
    // states, rewards, returns
    const int keys[3] = {M3PC_STATES, M3PC_REWARDS, M3PC_RETURNS};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int D = j == 0 ? p.S : 1;
        const float* tg = p.tgt[keys[j]] + (size_t)r * D;
        const float* pr = p.pred[j] + (size_t)r * D;
        float nrm = 1.0f;
        if (p.flags & M3PC_MTM_NORM_L2) {
            double n2 = 0.0;
            for (int d = lane; d < D; d += 64) {
                const float t = tg[d];
                n2 += (double)(t * t);
            }
            nrm = sqrtf((float)wave_sum_f64(n2));
        }
        double acc = 0.0;
        for (int d = lane; d < D; d += 64) {
            float t = tg[d];
            if (p.flags & M3PC_MTM_NORM_L2) t = t / nrm;
            const float df = pr[d] - t;
            acc += (double)(df * df);
        }
        out[j] = wave_sum_f64(acc);
    }
    // actions: the squared error of the mean, the likelihood of the target, the sampled entropy
    const float lo = (float)(-1.0 + 1e-6), hi = (float)(1.0 - 1e-6);
    double a_se = 0.0, a_lp = 0.0, a_lq = 0.0;
    for (int d = lane; d < p.A; d += 64) {
        const size_t i = (size_t)r * p.A + d;
        const float mu = p.mu[i], sd = p.sd[i], a = p.tgt[M3PC_ACTIONS][i];
        const float df = tanhf(mu) - a;
        a_se += (double)(df * df);
        float ac = a;
        if ((p.flags & M3PC_MTM_CLIP_ACTIONS) && a == a) ac = fminf(fmaxf(a, lo), hi);  // (torch.clip keeps a NaN)
        const float z = 0.5f * (log1pf(ac) - log1pf(-ac));
        a_lp += (double)squashed_log_prob(z, mu, sd);
        const float u = mu + p.eps[i] * sd;
        a_lq += (double)squashed_log_prob(u, mu, sd);
    }
    out[3] = wave_sum_f64(a_se);
    out[4] = wave_sum_f64(a_lp);
    out[5] = wave_sum_f64(a_lq);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < MTM_LOSS_PART; ++j) p.part[(size_t)r * MTM_LOSS_PART + j] = out[j];
    }
}

// One workgroup: thread i adds the rows i, i + ML_THREADS, ... in that order, then block_sum_f64.  Thread 0 forms the record.
__global__ __launch_bounds__(ML_THREADS) void mtm_loss_reduce_kernel(MtmLossP p) {
    __shared__ double sv[ML_THREADS / 64];
    const int rows = p.batch * p.T;
    const int keys[3] = {M3PC_STATES, M3PC_REWARDS, M3PC_RETURNS};
    double acc[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) acc[j] = 0.0;
    for (int r = threadIdx.x; r < rows; r += ML_THREADS) {
        const int t = r % p.T;
        const double* q = p.part + (size_t)r * MTM_LOSS_PART;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double m = (double)((p.mask[keys[j]] >> t) & 1ull), s = q[j];
            acc[3 * j] += s;
            acc[3 * j + 1] += s * m;
            acc[3 * j + 2] += s * (1.0 - m);
        }
        const bool vis = (p.mask[M3PC_ACTIONS] >> t) & 1ull;
        acc[9] += q[3] * (vis ? 1.0 : 0.0);
        if (!vis) {
            acc[10] += q[4];
            acc[11] += q[5];
        }
    }
#pragma unroll
    for (int j = 0; j < 12; ++j) acc[j] = block_sum_f64(acc[j], sv);
    if (threadIdx.x != 0) return;
    const double B = (double)p.batch, T = (double)p.T;
    double loss[4];
    float* rec = p.record;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int k = keys[j];
        const double D = j == 0 ? (double)p.S : 1.0, n_vis = (double)__popcll(p.mask[k]);
        loss[k] = acc[3 * j] / (B * T * D);
        rec[3 * k] = (float)loss[k];
        rec[3 * k + 1] = (float)(acc[3 * j + 2] / (T - n_vis) / B);  // masked_loss: the hidden tokens
        rec[3 * k + 2] = (float)(acc[3 * j + 1] / n_vis / B);        // masked_c_loss: the visible ones
    }
    loss[M3PC_ACTIONS] = acc[9] / (B * T * (double)p.A);
    rec[3 * M3PC_ACTIONS] = (float)loss[M3PC_ACTIONS];
    rec[3 * M3PC_ACTIONS + 1] = 0.f;
    rec[3 * M3PC_ACTIONS + 2] = 0.f;
    const double n_hid = T - (double)__popcll(p.mask[M3PC_ACTIONS]);
    const double cnt = B * n_hid * (double)p.A;
    const double ll = acc[10] / cnt, entropy = -(acc[11] / cnt);
    double total = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if ((p.loss_keys >> k) & 1) total += loss[k];
    total -= ll + (double)(p.entropy_reg_p ? *p.entropy_reg_p : p.entropy_reg) * entropy;
    rec[12] = (float)entropy;
    rec[13] = (float)(-ll);
    rec[14] = (float)total;
}

}  // namespace

void launch_mtm_loss(const MtmLossP& p, hipStream_t st) {
    const int rows = p.batch * p.T, per = ML_THREADS / 64;
    hipLaunchKernelGGL(mtm_loss_rows_kernel, dim3((rows + per - 1) / per), dim3(ML_THREADS), 0, st, p);
    hipLaunchKernelGGL(mtm_loss_reduce_kernel, dim3(1), dim3(ML_THREADS), 0, st, p);
}

void mtm_loss_free(m3pc_handle* h) {
    auto& m = h->ml;
    for (void* b : {(void*)m.s.tok[0], (void*)m.s.tok[1], (void*)m.s.tok[2], (void*)m.s.tok[3], (void*)m.head[0], (void*)m.head[1],
                    (void*)m.head[2], (void*)m.head[3], (void*)m.head[4], (void*)m.s.raw[0], (void*)m.s.raw[1], (void*)m.s.raw[2], (void*)m.s.eps,
                    (void*)m.s.raw_returns, (void*)m.s.part})
        if (b) (void)hipFree(b);
    m = m3pc_handle::MtmLoss();
}

}  // namespace m3pc

namespace {

// the scratch of the three calls, at the first of them
int ml_ensure(m3pc_handle* h) {
    HIPCHK(hipSetDevice(h->device));
    auto& m = h->ml;
    if (m.ready) return 0;
    const size_t rows = (size_t)h->dm.max_batch * h->T;
    for (int k = 0; k < 4; ++k) CHK(dmalloc(&m.s.tok[k], rows * h->feat[k]));
    const int hw[5] = {h->S, 1, 1, h->A, h->A};
    for (int j = 0; j < 5; ++j) CHK(dmalloc(&m.head[j], rows * hw[j]));
    for (int k = 0; k < 3; ++k) CHK(dmalloc(&m.s.raw[k], rows * h->feat[k]));
    CHK(dmalloc(&m.s.eps, rows * h->A));
    CHK(dmalloc(&m.s.raw_returns, rows));
    CHK(dmalloc(&m.s.part, rows * MTM_LOSS_PART));
    m.ready = true;
    return 0;
}

// tokenise the raw batch, omtm.forward under the masks, the loss: everything behind the refusals
int ml_run(m3pc_handle* h, int batch, const float* states, const float* actions, const float* rewards, const void* returns, int returns_f64,
           const unsigned char* const masks[4], const unsigned long long bits[4], const float* eps, float entropy_reg, int flags,
           int loss_keys, int precision, float* record, float* const outs[5], hipStream_t st) {
    auto& m = h->ml;
    mb_tokenize(h, m.s, batch, states, actions, rewards, returns, returns_f64, st);
    CHK(check_launch("mtm_loss tokenize"));
    Plan* pl = nullptr;
    CHK(get_plan(h, masks, &pl));
    TokIn in;
    memset(&in, 0, sizeof(in));
    for (int k = 0; k < 4; ++k) {
        in.ptr[k] = m.s.tok[k];
        in.bstride[k] = (long long)h->T * h->feat[k];
    }
    float* head[5];
    for (int j = 0; j < 5; ++j) head[j] = outs[j] ? outs[j] : m.head[j];
    h->allow_splitk = true;
    CHK(ws_sync(h, st));
    {
        X3Scope x3(h, precision == M3PC_PREC_BF16X3);
        CHK(forward_impl(h, pl, in, batch, head[0], head[1], head[2], head[3], head[4], pass_dt(precision), st));
    }
    mb_loss(h, m.s, batch, head, m.s.tok, bits, eps, entropy_reg, nullptr, flags, loss_keys, record, st);
    return check_launch("mtm_loss");
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int m3pc_mtm_loss_terms(m3pc_handle* h, int batch, const float* pred_states, const float* pred_rewards, const float* pred_returns,
                        const float* mu, const float* std_, const float* const targets[4], const unsigned char* const masks[4],
                        const float* eps, float entropy_reg, int flags, int loss_keys, float* record, void* stream) {
    if (!h || !pred_states || !pred_rewards || !pred_returns || !mu || !std_ || !targets || !masks || !eps || !record)
        return fail(M3PC_EINVAL, "m3pc_mtm_loss_terms: null argument");
    for (int k = 0; k < 4; ++k)
        if (!targets[k]) return fail(M3PC_EINVAL, "m3pc_mtm_loss_terms: null targets of '%s'", KEYN[k]);
    unsigned long long bits[4];
    CHK(mb_check(h->dm, h->dm.max_batch, batch, masks, flags, loss_keys, "m3pc_mtm_loss_terms", false, bits));
    CHK(ml_ensure(h));
    const float* pred[5] = {pred_states, pred_rewards, pred_returns, mu, std_};
    mb_loss(h, h->ml.s, batch, pred, targets, bits, eps, entropy_reg, nullptr, flags, loss_keys, record, (hipStream_t)stream);
    return check_launch("mtm_loss");
}

int m3pc_mtm_loss(m3pc_handle* h, int batch, const float* states, const float* actions, const float* rewards, const void* returns,
                  int returns_f64, const unsigned char* const masks[4], const float* eps, float entropy_reg, int flags, int loss_keys,
                  int precision, float* record, float* out_states, float* out_rewards, float* out_returns, float* out_mu, float* out_std,
                  void* stream) {
    const char* who = "m3pc_mtm_loss";
    if (!h || !states || !actions || !rewards || !returns || !masks || !eps || !record) return fail(M3PC_EINVAL, "%s: null argument", who);
    unsigned long long bits[4];
    CHK(mb_check(h->dm, h->dm.max_batch, batch, masks, flags, loss_keys, who, false, bits));
    if (!precision_ok(precision)) return fail(M3PC_EINVAL, "%s: bad precision %d", who, precision);
    CHK(mb_state(h, who));
    CHK(ml_ensure(h));
    float* const outs[5] = {out_states, out_rewards, out_returns, out_mu, out_std};
    return ml_run(h, batch, states, actions, rewards, returns, returns_f64, masks, bits, eps, entropy_reg, flags, loss_keys, precision, record,
                  outs, (hipStream_t)stream);
}

int m3pc_mtm_loss_replay(m3pc_handle* h, m3pc_replay* rb, int batch, int mode, const int* traj_index, const int* start_index,
                         int index_on_device, unsigned long long seed, unsigned long long step, const unsigned char* const masks[4],
                         const float* eps, float entropy_reg, int flags, int loss_keys, int precision, float* record, int* out_traj,
                         int* out_start, void* stream) {
    const char* who = "m3pc_mtm_loss_replay";
    if (!h || !rb || !masks || !record) return fail(M3PC_EINVAL, "%s: null argument", who);
    unsigned long long bits[4];
    CHK(mb_check(h->dm, h->dm.max_batch, batch, masks, flags, loss_keys, who, false, bits));
    if (!precision_ok(precision)) return fail(M3PC_EINVAL, "%s: bad precision %d", who, precision);
    CHK(mb_fits(h, rb, who));
    CHK(replay_check_segments(rb, batch, mode, traj_index, start_index, index_on_device, who));
    CHK(mb_state(h, who));
    CHK(ml_ensure(h));
    const MtmStage& s = h->ml.s;
    hipStream_t st = (hipStream_t)stream;
    CHK(mb_draw(h, s, rb, batch, mode, traj_index, start_index, index_on_device, seed, step, &eps, out_traj, out_start, st, who));
    float* const outs[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    return ml_run(h, batch, s.raw[0], s.raw[1], s.raw[2], s.raw_returns, 1, masks, bits, eps, entropy_reg, flags, loss_keys, precision, record,
                  outs, st);
}

}  // extern "C"
#pragma GCC visibility pop

