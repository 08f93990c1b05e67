// The optimizers of the masked-trajectory model: mo_adamw_kernel, mo_temperature_kernel, their launchers and the C ABI of
// m3pc_mtm_opt_* / m3pc_mtm_train* / m3pc_mtm_weights_export.  Launches, arithmetic order and determinism: mtm_opt.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_util.h"
#include "mtm_loss.h"
#include "mtm_grad.h"
#include "mtm_opt.h"

namespace m3pc {
namespace {

// one element: the fp32 moment recurrences, then decay and step as one float64 expression rounded once (mtm_opt.h, ARITHMETIC)
__device__ __forceinline__ float mo_elem(const MoAdamP& p, double step_size, double sqrt_bc2, double keep, float w, float g, float& m, float& v) {
    m = __fadd_rn(m, __fmul_rn(p.omb1, __fsub_rn(g, m)));
    v = __fadd_rn(__fmul_rn(p.b2, v), __fmul_rn(__fmul_rn(p.omb2, g), g));
    const double denom = sqrt((double)v) / sqrt_bc2 + p.eps;
    return (float)((double)w * keep - step_size * (double)m / denom);
}

__device__ __forceinline__ unsigned int bf16_bits(bf16_t x) { return (unsigned int)__builtin_bit_cast(unsigned short, x); }

__global__ __launch_bounds__(256) void mo_adamw_kernel(MoAdamP p) {
    __shared__ double sc[3];  // lr_t / bc1, sqrt(bc2), 1 - lr_t wd
    if ((int)blockIdx.x >= p.n_blocks) return;
    const int2 bc = p.blk[blockIdx.x];
    const MoSeg s = p.seg[bc.x];
    const bool active = s.head_key < 0 || ((p.loss_keys >> s.head_key) & 1);
    const long long t0 = p.steps_in[bc.x];
    if (bc.y == 0 && threadIdx.x == 0) p.steps_out[bc.x] = active ? t0 + 1 : t0;
    if (!active) return;  // (the whole workgroup: weight, moments and bf16 copies keep their bits)
    if (threadIdx.x == 0) {
        const double t = (double)(t0 + 1);
        sc[0] = p.lr_t / (1.0 - pow(p.beta1, t));
        sc[1] = sqrt(1.0 - pow(p.beta2, t));
        sc[2] = s.decay ? 1.0 - p.lr_t * p.wd : 1.0;
    }
    __syncthreads();
    const double step_size = sc[0], sqrt_bc2 = sc[1], keep = sc[2];
    float* W = s.p;
    const float* G = p.grad + s.g_off;
    float* M = p.exp_avg + s.s_off;
    float* V = p.exp_avg_sq + s.s_off;
    bf16_t* hi = p.write_bf16 ? s.b : nullptr;
    bf16_t* lo = hi ? hi + s.numel : nullptr;
    const bool vec = ((((uintptr_t)W) | ((uintptr_t)G) | ((uintptr_t)M) | ((uintptr_t)V)) & 15) == 0;
    const bool bvec = hi && (((uintptr_t)hi) & 7) == 0 && (s.numel & 3) == 0;
    const long long c0 = (long long)bc.y * MO_CHUNK;
#pragma unroll
    for (int it = 0; it < MO_CHUNK / 1024; ++it) {
        const long long x = c0 + it * 1024 + threadIdx.x * 4;
        if (x >= s.numel) break;
        if (vec && x + 4 <= s.numel) {
            const float4 w4 = *(const float4*)(W + x), g4 = *(const float4*)(G + x);
            float4 m4 = *(const float4*)(M + x), v4 = *(const float4*)(V + x);
            float4 o;
            o.x = mo_elem(p, step_size, sqrt_bc2, keep, w4.x, g4.x, m4.x, v4.x);
            o.y = mo_elem(p, step_size, sqrt_bc2, keep, w4.y, g4.y, m4.y, v4.y);
            o.z = mo_elem(p, step_size, sqrt_bc2, keep, w4.z, g4.z, m4.z, v4.z);
            o.w = mo_elem(p, step_size, sqrt_bc2, keep, w4.w, g4.w, m4.w, v4.w);
            *(float4*)(M + x) = m4;
            *(float4*)(V + x) = v4;
            *(float4*)(W + x) = o;
            if (hi) {
                const float of[4] = {o.x, o.y, o.z, o.w};
                bf16_t h4[4], l4[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    h4[j] = (bf16_t)of[j];
                    l4[j] = (bf16_t)(of[j] - (float)h4[j]);
                }
                if (bvec) {
                    *(uint2*)(hi + x) = make_uint2(bf16_bits(h4[0]) | (bf16_bits(h4[1]) << 16), bf16_bits(h4[2]) | (bf16_bits(h4[3]) << 16));
                    *(uint2*)(lo + x) = make_uint2(bf16_bits(l4[0]) | (bf16_bits(l4[1]) << 16), bf16_bits(l4[2]) | (bf16_bits(l4[3]) << 16));
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        hi[x + j] = h4[j];
                        lo[x + j] = l4[j];
                    }
                }
            }
        } else {
            for (int j = 0; j < 4 && x + j < s.numel; ++j) {
                float m = M[x + j], v = V[x + j];
                const float o = mo_elem(p, step_size, sqrt_bc2, keep, W[x + j], G[x + j], m, v);
                M[x + j] = m;
                V[x + j] = v;
                W[x + j] = o;
                if (hi) {
                    const bf16_t hb = (bf16_t)o;
                    hi[x + j] = hb;
                    lo[x + j] = (bf16_t)(o - (float)hb);
                }
            }
        }
    }
}

__global__ void mo_temperature_kernel(MoTempP p) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double log_t = p.state[0], m = p.state[1], v = p.state[2];
    const double t = p.state[3] + 1.0;
    const double g = exp(log_t) * ((double)p.record[12] - p.target_entropy);
    m = m + (g - m) * (1.0 - p.beta1);
    v = v * p.beta2 + ((1.0 - p.beta2) * g) * g;
    const double step_size = p.lr / (1.0 - pow(p.beta1, t));
    const double denom = sqrt(v) / sqrt(1.0 - pow(p.beta2, t)) + p.eps;
    log_t = log_t - (step_size * m) / denom;
    const double temp = exp(log_t);
    p.state[0] = log_t;
    p.state[1] = m;
    p.state[2] = v;
    p.state[3] = t;
    *p.temp_f = (float)temp;
    if (p.train_record) {
        p.train_record[0] = p.lr_t;
        p.train_record[1] = temp;
        p.train_record[2] = log_t;
    }
}

}  // namespace

void mo_launch_adamw(const MoAdamP& p, hipStream_t st) {
    if (p.n_blocks <= 0) return;
    hipLaunchKernelGGL(mo_adamw_kernel, dim3((unsigned)p.n_blocks), dim3(256), 0, st, p);
}
void mo_launch_temperature(const MoTempP& p, hipStream_t st) { hipLaunchKernelGGL(mo_temperature_kernel, dim3(1), dim3(64), 0, st, p); }

}  // namespace m3pc

struct m3pc_mtm_opt {
    struct m3pc_mtm_grad* g = nullptr;
    m3pc_mtm_opt_args a;
    std::vector<MoSeg> seg;  // in the order of g->par
    std::vector<int2> blk;
    bool ready = false;
    float* arena = nullptr;  // exp_avg | exp_avg_sq, each laid out as the gradient arena
    MoSeg* d_seg = nullptr;
    int2* d_blk = nullptr;
    long long* d_steps = nullptr;  // 2 x n: the launches alternate (cur: the one the next launch reads)
    int cur = 0;
    double* d_temp = nullptr;      // log_t, exp_avg, exp_avg_sq, step count | train_record scratch (3)
    float* d_temp_f = nullptr;
    m3pc_mtm_opt_state st0;        // until the storage exists: what it starts from; afterwards only sched_step is kept here
};

namespace m3pc {
namespace {

using Opt = struct m3pc_mtm_opt;

bool ends_with(const std::string& s, const char* suf) {
    const size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}
// omtm.configure_optimizers on this architecture: the weights of Linear / MultiheadAttention modules decay; biases, LayerNorm weights
// (the heads' .0.weight included), per-dim encodings and mask tokens do not
bool mo_decays(const std::string& name) {
    if (!ends_with(name, "weight")) return false;
    if (name.find(".norm") != std::string::npos || ends_with(name, ".0.weight")) return false;
    return true;
}
int mo_head_key(const std::string& name) {
    const int keys[3] = {M3PC_STATES, M3PC_REWARDS, M3PC_RETURNS};
    for (int k : keys)
        if (name.rfind(std::string("output_head_dict.") + KEYN[k] + ".", 0) == 0) return k;
    return -1;
}

int mo_check_args(const m3pc_mtm_opt_args* a, const char* who) {
    if (!a) return fail(M3PC_EINVAL, "%s: null args", who);
    if (!(a->learning_rate >= 0.0) || !std::isfinite(a->learning_rate)) return fail(M3PC_EINVAL, "%s: learning_rate %g is not a finite number >= 0", who, a->learning_rate);
    if (!(a->weight_decay >= 0.0) || !std::isfinite(a->weight_decay)) return fail(M3PC_EINVAL, "%s: weight_decay %g is not a finite number >= 0", who, a->weight_decay);
    if (!(a->beta1 >= 0.0 && a->beta1 < 1.0)) return fail(M3PC_EINVAL, "%s: beta1 %g outside [0, 1)", who, a->beta1);
    if (!(a->beta2 >= 0.0 && a->beta2 < 1.0)) return fail(M3PC_EINVAL, "%s: beta2 %g outside [0, 1)", who, a->beta2);
    if (!(a->eps > 0.0) || !std::isfinite(a->eps)) return fail(M3PC_EINVAL, "%s: eps %g is not a finite number > 0", who, a->eps);
    if (a->num_train_steps < 1) return fail(M3PC_EINVAL, "%s: num_train_steps %lld < 1", who, a->num_train_steps);
    if (a->warmup_steps < 0 || (a->warmup_steps > 0 && a->warmup_steps >= a->num_train_steps))
        return fail(M3PC_EINVAL, "%s: warmup_steps %lld outside [0, num_train_steps=%lld)", who, a->warmup_steps, a->num_train_steps);
    if (!(a->temp_learning_rate >= 0.0) || !std::isfinite(a->temp_learning_rate)) return fail(M3PC_EINVAL, "%s: temp_learning_rate %g is not a finite number >= 0", who, a->temp_learning_rate);
    if (!(a->temp_beta1 >= 0.0 && a->temp_beta1 < 1.0)) return fail(M3PC_EINVAL, "%s: temp_beta1 %g outside [0, 1)", who, a->temp_beta1);
    if (!(a->temp_beta2 >= 0.0 && a->temp_beta2 < 1.0)) return fail(M3PC_EINVAL, "%s: temp_beta2 %g outside [0, 1)", who, a->temp_beta2);
    if (!(a->temp_eps > 0.0) || !std::isfinite(a->temp_eps)) return fail(M3PC_EINVAL, "%s: temp_eps %g is not a finite number > 0", who, a->temp_eps);
    if (!std::isfinite(a->target_entropy)) return fail(M3PC_EINVAL, "%s: target_entropy is not finite", who);
    if (!std::isfinite(a->init_log_temperature)) return fail(M3PC_EINVAL, "%s: init_log_temperature is not finite", who);
    return 0;
}

double mo_lr(const m3pc_mtm_opt_args& a, long long s) {
    const double pi = 3.141592653589793;
    double lam;
    if (a.warmup_steps > 0) {
        if (s < a.warmup_steps) {
            lam = (double)s / (double)a.warmup_steps;
        } else {
            const double u = (double)(s - a.warmup_steps);
            lam = 0.5 * (1.0 + cos(u / (double)(a.num_train_steps - a.warmup_steps) * pi));
        }
    } else {
        lam = 0.5 * (1.0 + cos((double)s / (double)a.num_train_steps * pi));
    }
    return a.learning_rate * lam;
}

int mo_ensure(Opt* o) {
    m3pc_handle* h = o->g->h;
    HIPCHK(hipSetDevice(h->device));
    if (o->ready) return 0;
    const size_t n = o->seg.size(), nf = o->g->grad_floats;
    if (!o->arena) CHK(dmalloc(&o->arena, 2 * nf));
    if (!o->d_seg) CHK(dmalloc((char**)&o->d_seg, n * sizeof(MoSeg)));
    if (!o->d_blk) CHK(dmalloc((char**)&o->d_blk, std::max<size_t>(1, o->blk.size()) * sizeof(int2)));
    if (!o->d_steps) CHK(dmalloc(&o->d_steps, 2 * n));
    if (!o->d_temp) CHK(dmalloc(&o->d_temp, 8));
    if (!o->d_temp_f) CHK(dmalloc(&o->d_temp_f, 64));
    for (size_t i = 0; i < n; ++i) {  // (the handle's tensors exist since m3pc_create)
        const Tensor& t = h->w.at(o->g->par[i].name);
        o->seg[i].p = t.f;
        o->seg[i].b = t.gemm ? t.b : nullptr;
    }
    // once per object, synchronous: the tables, zeroed moments and step counts, the temperature's state
    HIPCHK(hipMemcpy(o->d_seg, o->seg.data(), n * sizeof(MoSeg), hipMemcpyHostToDevice));
    if (!o->blk.empty()) HIPCHK(hipMemcpy(o->d_blk, o->blk.data(), o->blk.size() * sizeof(int2), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(o->arena, 0, 2 * nf * sizeof(float)));
    HIPCHK(hipMemset(o->d_steps, 0, 2 * n * sizeof(long long)));
    const double t4[8] = {o->st0.log_temperature, o->st0.temp_exp_avg, o->st0.temp_exp_avg_sq, (double)o->st0.temp_step, 0, 0, 0, 0};
    const float tf = (float)exp(o->st0.log_temperature);
    HIPCHK(hipMemcpy(o->d_temp, t4, sizeof(t4), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(o->d_temp_f, &tf, sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
    o->cur = 0;
    o->ready = true;
    return 0;
}

// what every stepping entry refuses alike, before any HIP call
int mo_step_state(const Opt* o, const char* who) {
    if (cert_any_begun(o->g->h)) return fail(M3PC_ESTATE, "%s: a certified step is between _begin and _end on the handle", who);
    return 0;
}

// one optimizer step on the gradients and the record of the gradient call just made; last: write the bf16 copies and re-derive
int mo_step(Opt* o, bool last, double* train_record, hipStream_t st, const char* who) {
    struct m3pc_mtm_grad* g = o->g;
    m3pc_handle* h = g->h;
    const int n = (int)o->seg.size();
    const double lr_t = mo_lr(o->a, o->st0.sched_step);
    MoAdamP p;
    memset(&p, 0, sizeof(p));
    p.seg = o->d_seg;
    p.blk = o->d_blk;
    p.n_blocks = (int)o->blk.size();
    p.grad = g->grad;
    p.exp_avg = o->arena;
    p.exp_avg_sq = o->arena + g->grad_floats;
    p.steps_in = o->d_steps + (size_t)o->cur * n;
    p.steps_out = o->d_steps + (size_t)(1 - o->cur) * n;
    p.loss_keys = g->last_loss_keys;
    p.write_bf16 = last ? 1 : 0;
    p.lr_t = lr_t;
    p.wd = o->a.weight_decay;
    p.beta1 = o->a.beta1;
    p.beta2 = o->a.beta2;
    p.eps = o->a.eps;
    p.omb1 = (float)(1.0 - o->a.beta1);
    p.b2 = (float)o->a.beta2;
    p.omb2 = (float)(1.0 - o->a.beta2);
    mo_launch_adamw(p, st);
    o->cur = 1 - o->cur;
    MoTempP t;
    memset(&t, 0, sizeof(t));
    t.state = o->d_temp;
    t.temp_f = o->d_temp_f;
    t.record = g->rec;
    t.train_record = train_record;
    t.lr_t = lr_t;
    t.target_entropy = o->a.target_entropy;
    t.lr = o->a.temp_learning_rate;
    t.beta1 = o->a.temp_beta1;
    t.beta2 = o->a.temp_beta2;
    t.eps = o->a.temp_eps;
    mo_launch_temperature(t, st);
    CHK(check_launch(who));
    o->st0.sched_step += 1;
    g->consumed = true;
    if (last) {
        std::vector<std::string> dirty;
        for (int i = 0; i < n; ++i)
            if (o->seg[i].head_key < 0 || ((g->last_loss_keys >> o->seg[i].head_key) & 1)) dirty.push_back(g->par[i].name);
        CHK(derive_weights(h, dirty, true, st));
        CHK(check_launch(who));
    }
    return 0;
}

// the parameter `name` in the gradient object's list, or null
const m3pc_mtm_grad::Par* mo_par(const Opt* o, const char* name) {
    auto it = o->g->idx.find(name);
    return it == o->g->idx.end() ? nullptr : &o->g->par[it->second];
}
int mo_find(const Opt* o, const m3pc_named_tensor* tensors, int n, const char* who) {
    return nt_check(tensors, n, [o](const char* name) { return mo_par(o, name) ? mo_par(o, name)->numel : -1ll; }, who, "parameter");
}
// exp_avg (which = 1) or exp_avg_sq (2) of the listed parameters, to the caller's tensors or from them
int mo_copy(Opt* o, int which, const m3pc_named_tensor* tensors, int n, bool to_caller, hipStream_t st) {
    float* base = o->arena + (which == 2 ? o->g->grad_floats : 0);
    return nt_copy(tensors, n, to_caller, [&](const char* name) { return base + mo_par(o, name)->off; }, st);
}

}  // namespace
}  // namespace m3pc

#pragma GCC visibility push(default)
extern "C" {

int m3pc_mtm_opt_create(struct m3pc_mtm_grad* g, const m3pc_mtm_opt_args* args, struct m3pc_mtm_opt** out) {
    if (!g || !out) return fail(M3PC_EINVAL, "m3pc_mtm_opt_create: null argument (g or out)");
    CHK(mo_check_args(args, "m3pc_mtm_opt_create"));
    Opt* o = new Opt();
    o->g = g;
    o->a = *args;
    o->st0.sched_step = 0;
    o->st0.temp_step = 0;
    o->st0.log_temperature = args->init_log_temperature;
    o->st0.temp_exp_avg = 0.0;
    o->st0.temp_exp_avg_sq = 0.0;
    std::vector<long long> numel;
    for (const auto& par : g->par) {
        MoSeg s;
        memset(&s, 0, sizeof(s));
        s.g_off = (long long)par.off;
        s.s_off = (long long)par.off;
        s.numel = par.numel;
        s.decay = mo_decays(par.name) ? 1 : 0;
        s.head_key = mo_head_key(par.name);
        o->seg.push_back(s);
        numel.push_back(par.numel);
    }
    mo_block_table(numel.data(), (int)numel.size(), o->blk);
    *out = o;
    return 0;
}

int m3pc_mtm_opt_destroy(struct m3pc_mtm_opt* o) {
    if (!o) return 0;
    if (o->arena || o->d_seg || o->d_blk || o->d_steps || o->d_temp || o->d_temp_f) {
        (void)hipSetDevice(o->g->h->device);
        (void)hipDeviceSynchronize();
        void* bufs[] = {o->arena, o->d_seg, o->d_blk, o->d_steps, o->d_temp, o->d_temp_f};
        for (void* b : bufs)
            if (b) (void)hipFree(b);
    }
    delete o;
    return 0;
}

int m3pc_mtm_lr(const m3pc_mtm_opt_args* args, long long sched_step, double* lr) {
    if (!lr) return fail(M3PC_EINVAL, "m3pc_mtm_lr: null lr");
    CHK(mo_check_args(args, "m3pc_mtm_lr"));
    if (sched_step < 0) return fail(M3PC_EINVAL, "m3pc_mtm_lr: sched_step %lld < 0", sched_step);
    *lr = mo_lr(*args, sched_step);
    return 0;
}

int m3pc_mtm_opt_decays(struct m3pc_mtm_opt* o, const char* name, int* decays) {
    if (decays) *decays = -1;
    if (!o || !name || !decays) return fail(M3PC_EINVAL, "m3pc_mtm_opt_decays: null argument");
    auto it = o->g->idx.find(name);
    if (it == o->g->idx.end()) return fail(M3PC_EINVAL, "m3pc_mtm_opt_decays: name '%s' is not a parameter", name);
    *decays = o->seg[it->second].decay;
    return 0;
}

int m3pc_mtm_opt_step(struct m3pc_mtm_opt* o, void* stream) {
    if (!o) return fail(M3PC_EINVAL, "m3pc_mtm_opt_step: null opt");
    if (!o->g->have_grad) return fail(M3PC_ESTATE, "m3pc_mtm_opt_step: no gradient call was made");
    if (o->g->consumed) return fail(M3PC_ESTATE, "m3pc_mtm_opt_step: the gradients of the last gradient call were already applied");
    CHK(mo_step_state(o, "m3pc_mtm_opt_step"));
    hipStream_t st = (hipStream_t)stream;
    CHK(mo_ensure(o));
    CHK(ws_sync(o->g->h, st));  // (deferred candidate parts still read the weights this call is about to move)
    return mo_step(o, true, nullptr, st, "m3pc_mtm_opt_step");
}

int m3pc_mtm_train_step(struct m3pc_mtm_opt* o, int batch, const float* states, const float* actions, const float* rewards, const void* returns,
                        int returns_f64, const unsigned char* const masks[4], const float* eps, int flags, int loss_keys, float* record,
                        double* train_record, void* stream) {
    if (!o) return fail(M3PC_EINVAL, "m3pc_mtm_train_step: null opt");
    if (!states || !actions || !rewards || !returns || !masks || !eps)
        return fail(M3PC_EINVAL, "m3pc_mtm_train_step: null argument (states, actions, rewards, returns, masks or eps)");
    unsigned long long bits[4];
    CHK(mg_precheck(o->g, batch, masks, flags, loss_keys, "m3pc_mtm_train_step", bits));
    CHK(mo_step_state(o, "m3pc_mtm_train_step"));
    hipStream_t st = (hipStream_t)stream;
    CHK(mo_ensure(o));
    CHK(ws_sync(o->g->h, st));
    CHK(mg_ensure(o->g));
    CHK(mg_run(o->g, batch, states, actions, rewards, returns, returns_f64, bits, eps, 0.f, o->d_temp_f, flags, loss_keys, record, st));
    return mo_step(o, true, train_record, st, "m3pc_mtm_train_step");
}

int m3pc_mtm_train(struct m3pc_mtm_opt* o, m3pc_replay* rb, int n_steps, int batch, int mode, unsigned long long seed, unsigned long long step0,
                   const unsigned char* const* masks, int flags, int loss_keys, float* records, double* train_records, void* stream) {
    if (!o) return fail(M3PC_EINVAL, "m3pc_mtm_train: null opt");
    if (!rb || !masks) return fail(M3PC_EINVAL, "m3pc_mtm_train: null argument (rb or masks)");
    if (n_steps < 1) return fail(M3PC_EINVAL, "m3pc_mtm_train: n_steps %d < 1", n_steps);
    std::vector<unsigned long long> bits(4 * (size_t)n_steps);  // (every step is refused or accepted before the first one runs: mtm_grad.h)
    for (int i = 0; i < n_steps; ++i)
        CHK(mg_precheck_replay(o->g, rb, batch, mode, nullptr, nullptr, 0, masks + 4 * (size_t)i, flags, loss_keys, "m3pc_mtm_train", &bits[4 * (size_t)i]));
    CHK(mo_step_state(o, "m3pc_mtm_train"));
    hipStream_t st = (hipStream_t)stream;
    CHK(mo_ensure(o));
    CHK(ws_sync(o->g->h, st));
    CHK(mg_ensure(o->g));
    for (int i = 0; i < n_steps; ++i) {
        CHK(mg_run_replay(o->g, rb, batch, mode, nullptr, nullptr, 0, seed, step0 + (unsigned long long)i, &bits[4 * (size_t)i], nullptr, 0.f,
                          o->d_temp_f, flags, loss_keys, records ? records + (size_t)i * M3PC_MTM_LOSS_FLOATS : nullptr, nullptr, nullptr, st,
                          "m3pc_mtm_train"));
        CHK(mo_step(o, i + 1 == n_steps, train_records ? train_records + 3 * (size_t)i : nullptr, st, "m3pc_mtm_train"));
    }
    return 0;
}

int m3pc_mtm_opt_export(struct m3pc_mtm_opt* o, int which, const m3pc_named_tensor* tensors, int n, long long* steps, void* stream) {
    if (!o || !tensors || n < 0) return fail(M3PC_EINVAL, "m3pc_mtm_opt_export: null argument (opt or tensors) or n < 0");
    if (which != 1 && which != 2) return fail(M3PC_EINVAL, "m3pc_mtm_opt_export: which %d is not 1 (exp_avg) or 2 (exp_avg_sq)", which);
    CHK(mo_find(o, tensors, n, "m3pc_mtm_opt_export"));
    hipStream_t st = (hipStream_t)stream;
    CHK(mo_ensure(o));
    CHK(mo_copy(o, which, tensors, n, true, st));
    if (steps) {  // (host out: waits for the stream)
        const size_t ns = o->seg.size();
        std::vector<long long> all(ns);
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(all.data(), o->d_steps + (size_t)o->cur * ns, ns * sizeof(long long), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) steps[i] = all[o->g->idx.at(tensors[i].name)];
    }
    return 0;
}

int m3pc_mtm_opt_load(struct m3pc_mtm_opt* o, int which, const m3pc_named_tensor* tensors, int n, const long long* steps, void* stream) {
    if (!o || !tensors || n < 0) return fail(M3PC_EINVAL, "m3pc_mtm_opt_load: null argument (opt or tensors) or n < 0");
    if (which != 1 && which != 2) return fail(M3PC_EINVAL, "m3pc_mtm_opt_load: which %d is not 1 (exp_avg) or 2 (exp_avg_sq)", which);
    CHK(mo_find(o, tensors, n, "m3pc_mtm_opt_load"));
    if (steps)
        for (int i = 0; i < n; ++i)
            if (steps[i] < 0) return fail(M3PC_EINVAL, "m3pc_mtm_opt_load: steps[%d] = %lld < 0", i, steps[i]);
    hipStream_t st = (hipStream_t)stream;
    CHK(mo_ensure(o));
    CHK(mo_copy(o, which, tensors, n, false, st));
    HIPCHK(hipStreamSynchronize(st));  // the caller's tensors may go away when the call returns
    if (steps) {
        const size_t ns = o->seg.size();
        std::vector<long long> all(ns);
        long long* cur = o->d_steps + (size_t)o->cur * ns;
        HIPCHK(hipMemcpy(all.data(), cur, ns * sizeof(long long), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) all[o->g->idx.at(tensors[i].name)] = steps[i];
        HIPCHK(hipMemcpy(cur, all.data(), ns * sizeof(long long), hipMemcpyHostToDevice));
    }
    return 0;
}

int m3pc_mtm_weights_export(m3pc_handle* h, const m3pc_named_tensor* tensors, int n, void* stream) {
    if (!h || !tensors || n < 0) return fail(M3PC_EINVAL, "m3pc_mtm_weights_export: null argument (h or tensors) or n < 0");
    auto numel_of = [h](const char* name) {
        auto it = h->w.find(name);
        return it == h->w.end() ? -1ll : it->second.numel;
    };
    CHK(nt_check(tensors, n, numel_of, "m3pc_mtm_weights_export", "tensor of the model"));
    if (!h->weights_loaded) return fail(M3PC_ESTATE, "m3pc_mtm_weights_export: weights not loaded");
    HIPCHK(hipSetDevice(h->device));
    return nt_copy(tensors, n, true, [h](const char* name) { return h->w.at(name).f; }, (hipStream_t)stream);
}

int m3pc_mtm_opt_get_state(struct m3pc_mtm_opt* o, m3pc_mtm_opt_state* out) {
    if (!o || !out) return fail(M3PC_EINVAL, "m3pc_mtm_opt_get_state: null argument");
    *out = o->st0;
    out->temperature = (double)(float)exp(o->st0.log_temperature);
    if (o->ready) {
        double t4[4];
        HIPCHK(hipSetDevice(o->g->h->device));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(t4, o->d_temp, sizeof(t4), hipMemcpyDeviceToHost));
        out->log_temperature = t4[0];
        out->temp_exp_avg = t4[1];
        out->temp_exp_avg_sq = t4[2];
        out->temp_step = (long long)t4[3];
        float tf = 0.f;
        HIPCHK(hipMemcpy(&tf, o->d_temp_f, sizeof(float), hipMemcpyDeviceToHost));
        out->temperature = (double)tf;
    }
    return 0;
}

int m3pc_mtm_opt_set_state(struct m3pc_mtm_opt* o, const m3pc_mtm_opt_state* in) {
    if (!o || !in) return fail(M3PC_EINVAL, "m3pc_mtm_opt_set_state: null argument");
    if (in->sched_step < 0) return fail(M3PC_EINVAL, "m3pc_mtm_opt_set_state: sched_step %lld < 0", in->sched_step);
    if (in->temp_step < 0) return fail(M3PC_EINVAL, "m3pc_mtm_opt_set_state: temp_step %lld < 0", in->temp_step);
    if (!std::isfinite(in->log_temperature) || !std::isfinite(in->temp_exp_avg) || !(in->temp_exp_avg_sq >= 0.0) || !std::isfinite(in->temp_exp_avg_sq))
        return fail(M3PC_EINVAL, "m3pc_mtm_opt_set_state: log_temperature / temp_exp_avg not finite or temp_exp_avg_sq not a finite number >= 0");
    o->st0 = *in;
    if (o->ready) {
        const double t4[4] = {in->log_temperature, in->temp_exp_avg, in->temp_exp_avg_sq, (double)in->temp_step};
        const float tf = (float)exp(in->log_temperature);
        HIPCHK(hipSetDevice(o->g->h->device));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(o->d_temp, t4, sizeof(t4), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(o->d_temp_f, &tf, sizeof(float), hipMemcpyHostToDevice));
    }
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
