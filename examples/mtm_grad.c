/*
 * mtm_grad.c -- the backward pass of the fine-tuning loop (finetune_omtm/learner.py:506-538: mtm_update's loss.backward()) from the
 * library alone: fill a replay buffer, create a gradient object on the handle, then ONE call, m3pc_mtm_grad_replay, which draws a
 * segment batch at (seed, step), tokenises it, runs the model under the masks, writes the loss record and differentiates `total`
 * through the whole model; m3pc_mtm_grad_export then hands out the gradients the caller names, in the torch layout of their
 * parameters.  The batch never leaves the device.  The optimizer is the caller's.
 *
 * The model differentiated here is the eval-mode one; m3pc_mtm_grad_set_dropout(g, p, seed, draw) before the call would switch on the
 * training-mode model's dropout under the library's own keep-mask stream (include/m3pc_hip.h; examples/mtm_train.c sets it).
 *
 *   gcc -O2 -Wall -Werror -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include -c examples/mtm_grad.c
 *   (link with -L<dir of libm3pc_hip.so> -l:libm3pc_hip.so -lamdhip64 -lm)
 */
#include <stdio.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "m3pc_hip.h"

typedef struct mtm_grad_io {
    /* model and tokenizers (host) */
    const m3pc_dims* dims;
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
    /* the gradient call */
    int batch;
    const unsigned char* masks[4]; /* (T,) 0/1 bytes each */
    float entropy_reg;             /* exp(log_temperature) */
    unsigned long long seed, step;
    float* record_dev; /* device scratch, M3PC_MTM_LOSS_FLOATS floats */
    /* results: the record and two gradients (host), by state_dict name */
    float* record;
    const char* grad_name[2];
    float* grad[2];
    long long grad_numel[2];
} mtm_grad_io;

/* -> 0, or a negative code (the message on stderr) */
int mtm_grad_example(mtm_grad_io* io, int device, void* stream) {
    m3pc_handle* h = 0;
    m3pc_replay* rb = 0;
    struct m3pc_mtm_grad* g = 0;
    const int T = io->dims->traj_length;
    int rc = m3pc_create(io->dims, device, &h);
    if (rc == 0) rc = m3pc_load_weights(h, io->weights, io->n_weights, stream);
    for (int k = 0; k < 4 && rc == 0; ++k)
        rc = m3pc_set_tokenizer(h, k, io->tok_mean[k], io->tok_std[k], io->tok_dim[k], io->tok_normalize[k]);
    if (rc == 0) rc = m3pc_replay_create(h, io->n_traj, io->max_steps, T, 0, 0, &rb);
    if (rc == 0) rc = m3pc_replay_append(rb, io->n_traj, io->obs, io->act, io->rew, io->val, io->lens, 0, stream);
    /* the object owns its workspace (allocated by the first gradient call) and reads the handle's weights at each call */
    if (rc == 0) rc = m3pc_mtm_grad_create(h, io->batch, &g);
    /* the fine-tuning form: the clip, no l2 norm, loss_keys = states alone; eps = NULL: the library's normals at (seed, step) */
    if (rc == 0)
        rc = m3pc_mtm_grad_replay(g, rb, io->batch, M3PC_REPLAY_LENGTH, 0, 0, 0, io->seed, io->step, io->masks, 0, io->entropy_reg,
                                  M3PC_MTM_CLIP_ACTIONS, 1 << M3PC_STATES, io->record_dev, 0, 0, stream);
    if (rc == 0) {
        m3pc_named_tensor out[2];
        for (int i = 0; i < 2; ++i) {
            out[i].name = io->grad_name[i];
            out[i].data = io->grad[i];
            out[i].numel = io->grad_numel[i];
            out[i].on_device = 0;
        }
        rc = m3pc_mtm_grad_export(g, out, 2, stream);
    }
    if (rc == 0) {
        if (hipMemcpyAsync(io->record, io->record_dev, M3PC_MTM_LOSS_FLOATS * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
            hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
            fprintf(stderr, "mtm_grad: the read-back failed\n");
            rc = M3PC_EHIP;
        } else {
            printf("total %.9g entropy %.9g nll %.9g", io->record[14], io->record[12], io->record[13]);
            for (int i = 0; i < 2; ++i) printf(" | d/d %s [0] = %.9g", io->grad_name[i], io->grad[i][0]);
            printf("\n");
        }
    }
    if (rc != 0 && rc != M3PC_EHIP) fprintf(stderr, "mtm_grad: %d: %s\n", rc, m3pc_last_error());
    /* the destroys drain the device before they free; the gradient object goes before its handle */
    m3pc_mtm_grad_destroy(g);
    m3pc_replay_destroy(rb);
    m3pc_destroy(h);
    return rc;
}
