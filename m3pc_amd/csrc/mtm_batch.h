// The front end the masked-trajectory calls share (m3pc_mtm_loss*, m3pc_mtm_grad*, m3pc_mtm_train*): what a batch call accepts, how a
// raw or replay-drawn batch becomes tokenised rows and a loss record, and how a list of named tensors is checked and copied.
// mtm_batch.hip holds the functions; it has no kernel of its own.  m3pc_internal.h includes this file: nothing of the handle is named here.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>

#include "../../include/m3pc_hip.h"

namespace m3pc {

// The staging buffers of one caller, each sized for max_batch * T rows: m3pc_handle::MtmLoss allocates them one by one, m3pc_mtm_grad
// slices them out of its arenas (mtm_grad.h: BYTES).
struct MtmStage {
    float *tok[4] = {nullptr, nullptr, nullptr, nullptr};  // the tokenised batch, in key order
    float *raw[3] = {nullptr, nullptr, nullptr}, *eps = nullptr;  // a replay draw: states, actions, rewards; the library's normals
    double *raw_returns = nullptr, *part = nullptr;        // its float64 returns; the per-row partial sums of the loss
};

// ---- refusals: pure functions of host state, no HIP call.  Every message starts with "<who>: ".
// In this order: batch, flags, loss_keys, traj_length, per key a null mask or a byte that is not 0 or 1, and with refuse_all_hidden
// "mask keeps no token".  bits[k]: the mask of key k, bit t = token t visible.
int mb_check(const m3pc_dims& dm, int max_batch, int batch, const unsigned char* const masks[4], int flags, int loss_keys, const char* who,
             bool refuse_all_hidden, unsigned long long bits[4]);
// the buffer's S, A, segment length and device are the handle's
int mb_fits(const m3pc_handle* h, const m3pc_replay* rb, const char* who);
// the weights are loaded and the four tokenizers set
int mb_state(const m3pc_handle* h, const char* who);

// ---- launches, on the caller's stream
// m3pc_replay_sample_segments into s.raw / s.raw_returns; *eps == nullptr: array 0 of the generator of m3pc_draw_variates at (seed, step),
// batch * T rows of A normals, into s.eps, and *eps = s.eps
int mb_draw(m3pc_handle* h, const MtmStage& s, m3pc_replay* rb, int batch, int mode, const int* traj_index, const int* start_index,
            int index_on_device, unsigned long long seed, unsigned long long step, const float** eps, int* out_traj, int* out_start,
            hipStream_t st, const char* who);
// the four keys of a raw batch into s.tok (the caller checks the launches)
void mb_tokenize(m3pc_handle* h, const MtmStage& s, int batch, const float* states, const float* actions, const float* rewards, const void* returns,
                 int returns_f64, hipStream_t st);
// the two launches of mtm_loss.hip: pred = states, rewards, returns, mu, std; entropy_reg_p: optional device scalar read in place of entropy_reg
void mb_loss(const m3pc_handle* h, const MtmStage& s, int batch, const float* const pred[5], const float* const tgt[4],
             const unsigned long long bits[4], const float* eps, float entropy_reg, const float* entropy_reg_p, int flags, int loss_keys,
             float* record, hipStream_t st);

// ---- lists of named tensors
// every entry has a name and data, numel_of(name) >= 0 (else "'<name>' is not a <noun>") and that many elements
int nt_check(const m3pc_named_tensor* tensors, int n, const std::function<long long(const char*)>& numel_of, const char* who, const char* noun);
// entry i and the device floats at(name): to the caller's tensors (to_caller) or from them
int nt_copy(const m3pc_named_tensor* tensors, int n, bool to_caller, const std::function<float*(const char*)>& at, hipStream_t st);

}  // namespace m3pc
