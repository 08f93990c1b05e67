/*
 * mtm_loss.c -- the validation loss of the fine-tuning loop (finetune_omtm/finetune.py:346-370: learner.compute_mtm_loss on a batch of
 * the buffer, logged as eval/loss*) from the library alone: fill a replay buffer, then per evaluation ONE call, m3pc_mtm_loss_replay,
 * which draws a segment batch at (seed, step), tokenises it, runs the model under the masks and writes the loss record -- the batch
 * never leaves the device, and the host restates nothing of the loss (the early return of learner.py:488-504, the clip, the mean over
 * the action dimension, the sampled entropy: include/m3pc_hip.h).
 *
 * The caller brings the model (weights by state_dict name, the four tokenizers), the trajectories and the masks -- masks are drawn by
 * the caller, as for m3pc_forward (m3pc_amd/masks.py: create_random_autoregressive_mask mirrors the reference's drawer).  eps = NULL:
 * the normals of the sampled entropy come from the library's generator at the same (seed, step).
 *
 *   gcc -O2 -Wall -Werror -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include -c examples/mtm_loss.c
 *   (link with -L<dir of libm3pc_hip.so> -l:libm3pc_hip.so -lamdhip64 -lm)
 */
#include <stdio.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "m3pc_hip.h"

typedef struct mtm_loss_io {
    /* model and tokenizers (host) */
    const m3pc_dims* dims; /* max_batch >= batch */
    const m3pc_named_tensor* weights;
    int n_weights;
    const float* tok_mean[4];
    const float* tok_std[4];
    int tok_dim[4];
    int tok_normalize[4];
    /* the buffer: n_traj trajectories of max_steps rows (host), path lengths >= traj_length */
    int n_traj, max_steps;
    const float *obs, *act, *rew; /* (n_traj, max_steps, S) (n_traj, max_steps, A) (n_traj, max_steps) */
    const double* val;            /* (n_traj, max_steps) */
    const int* lens;              /* (n_traj,) */
    /* the evaluations */
    int n_evals, batch;
    const unsigned char* masks[4]; /* (T,) 0/1 bytes each, the same for every evaluation here */
    float entropy_reg;             /* exp(log_temperature) */
    unsigned long long seed;
    float* record_dev; /* device scratch, M3PC_MTM_LOSS_FLOATS floats */
    /* results */
    float* records; /* host (n_evals, M3PC_MTM_LOSS_FLOATS) */
} mtm_loss_io;

/* -> 0, or a negative code (the message on stderr) */
int mtm_loss_example(mtm_loss_io* io, int device, void* stream) {
    static const char* names[4] = {"states", "actions", "rewards", "returns"};
    m3pc_handle* h = 0;
    m3pc_replay* rb = 0;
    const int T = io->dims->traj_length;
    int rc = m3pc_create(io->dims, device, &h);
    if (rc == 0) rc = m3pc_load_weights(h, io->weights, io->n_weights, stream);
    for (int k = 0; k < 4 && rc == 0; ++k)
        rc = m3pc_set_tokenizer(h, k, io->tok_mean[k], io->tok_std[k], io->tok_dim[k], io->tok_normalize[k]);
    /* segment_length == T: the loss call refuses a buffer that cuts other segments than the model takes */
    if (rc == 0) rc = m3pc_replay_create(h, io->n_traj, io->max_steps, T, 0, 0, &rb);
    if (rc == 0) rc = m3pc_replay_append(rb, io->n_traj, io->obs, io->act, io->rew, io->val, io->lens, 0, stream);
    for (int k = 0; k < io->n_evals && rc == 0; ++k) {
        /* the fine-tuning form: the clip, no l2 norm, loss_keys = states alone (the reference returns behind its first key) */
        rc = m3pc_mtm_loss_replay(h, rb, io->batch, M3PC_REPLAY_LENGTH, 0, 0, 0, io->seed, (unsigned long long)k, io->masks, 0, io->entropy_reg,
                                  M3PC_MTM_CLIP_ACTIONS, 1 << M3PC_STATES, M3PC_PREC_FP32, io->record_dev, 0, 0, stream);
        if (rc != 0) break;
        float* rec = io->records + (size_t)k * M3PC_MTM_LOSS_FLOATS;
        if (hipMemcpyAsync(rec, io->record_dev, M3PC_MTM_LOSS_FLOATS * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
            hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
            fprintf(stderr, "mtm_loss: the read-back of evaluation %d failed\n", k);
            rc = M3PC_EHIP;
            break;
        }
        printf("eval %d total %.9g entropy %.9g nll %.9g", k, rec[14], rec[12], rec[13]);
        for (int j = 0; j < 4; ++j) printf(" | %s loss %.9g masked %.9g masked_c %.9g", names[j], rec[3 * j], rec[3 * j + 1], rec[3 * j + 2]);
        printf("\n");
    }
    if (rc != 0 && rc != M3PC_EHIP) fprintf(stderr, "mtm_loss: %d: %s\n", rc, m3pc_last_error());
    /* both destroys drain the device before they free */
    m3pc_replay_destroy(rb);
    m3pc_destroy(h);
    return rc;
}
