/*
 * mtm_train.c -- the model half of the fine-tuning loop (finetune_omtm/learner.py:506-538: mtm_update) from the library alone: fill a
 * replay buffer, create a gradient object and an optimizer object on the handle, then ONE call, m3pc_mtm_train, which takes three
 * whole training steps -- each draws a segment batch at (seed, step0 + i), differentiates the loss under the device's own
 * temperature, steps AdamW over every parameter under the cosine schedule and steps the float64 log_temperature -- and leaves the
 * handle's weights, and every form the plan step reads, moved.  Nothing crosses the host until the records are read back.
 *
 * mtm_train_example trains the eval-mode model; mtm_train_example_dropout(..., p, dropout_seed) the training-mode one, with
 * dropout p at the four sites of every transformer layer under the library's own keep-mask stream (include/m3pc_hip.h: not
 * torch's generator): step i of the call drops under draw i.
 *
 *   gcc -O2 -Wall -Werror -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include -c examples/mtm_train.c
 *   (link with -L<dir of libm3pc_hip.so> -l:libm3pc_hip.so -lamdhip64 -lm)
 */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "m3pc_hip.h"

#define MTM_TRAIN_STEPS 3

typedef struct mtm_train_io {
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
    /* the training call */
    int batch;
    const unsigned char* masks[4]; /* (T,) 0/1 bytes each: the same masks at every step */
    double learning_rate, weight_decay;
    long long num_train_steps;
    unsigned long long seed, step0;
    float* records_dev;        /* device scratch, MTM_TRAIN_STEPS x M3PC_MTM_LOSS_FLOATS floats */
    double* train_records_dev; /* device scratch, MTM_TRAIN_STEPS x 3 doubles */
    /* results (host): the records, {lr, temperature, log_temperature} per step, and one trained weight by state_dict name */
    float* records;
    double* train_records;
    const char* weight_name;
    float* weight;
    long long weight_numel;
} mtm_train_io;

/* -> 0, or a negative code (the message on stderr).  dropout_p 0: the eval-mode model. */
int mtm_train_example_dropout(mtm_train_io* io, int device, void* stream, double dropout_p, unsigned long long dropout_seed) {
    m3pc_handle* h = 0;
    m3pc_replay* rb = 0;
    struct m3pc_mtm_grad* g = 0;
    struct m3pc_mtm_opt* opt = 0;
    const int T = io->dims->traj_length;
    const unsigned char* masks[4 * MTM_TRAIN_STEPS];
    m3pc_mtm_opt_args a;
    memset(&a, 0, sizeof(a));
    a.learning_rate = io->learning_rate;
    a.weight_decay = io->weight_decay;
    a.beta1 = 0.9;
    a.beta2 = 0.999;
    a.eps = 1e-8;
    a.num_train_steps = io->num_train_steps;
    a.warmup_steps = 0; /* learner.py:50-51 */
    a.temp_learning_rate = 1e-4;
    a.temp_beta1 = 0.9;
    a.temp_beta2 = 0.999;
    a.temp_eps = 1e-8;
    a.target_entropy = -(double)io->dims->action_dim;
    a.init_log_temperature = log(0.1);
    for (int i = 0; i < 4 * MTM_TRAIN_STEPS; ++i) masks[i] = io->masks[i % 4];
    int rc = m3pc_create(io->dims, device, &h);
    if (rc == 0) rc = m3pc_load_weights(h, io->weights, io->n_weights, stream);
    for (int k = 0; k < 4 && rc == 0; ++k)
        rc = m3pc_set_tokenizer(h, k, io->tok_mean[k], io->tok_std[k], io->tok_dim[k], io->tok_normalize[k]);
    if (rc == 0) rc = m3pc_replay_create(h, io->n_traj, io->max_steps, T, 0, 0, &rb);
    if (rc == 0) rc = m3pc_replay_append(rb, io->n_traj, io->obs, io->act, io->rew, io->val, io->lens, 0, stream);
    if (rc == 0) rc = m3pc_mtm_grad_create(h, io->batch, &g);
    if (rc == 0) rc = m3pc_mtm_opt_create(g, &a, &opt);
    /* host state of the gradient object: every gradient call from here on uses the current draw (0, 1, 2 below) and advances it */
    if (rc == 0 && dropout_p > 0.0) rc = m3pc_mtm_grad_set_dropout(g, dropout_p, dropout_seed, 0);
    /* the fine-tuning form: the clip, no l2 norm, loss_keys = states alone (the rewards / returns heads are left alone, as torch's
     * AdamW leaves parameters without a gradient) */
    if (rc == 0)
        rc = m3pc_mtm_train(opt, rb, MTM_TRAIN_STEPS, io->batch, M3PC_REPLAY_LENGTH, io->seed, io->step0, masks, M3PC_MTM_CLIP_ACTIONS,
                            1 << M3PC_STATES, io->records_dev, io->train_records_dev, stream);
    if (rc == 0) {
        m3pc_named_tensor out;
        out.name = io->weight_name;
        out.data = io->weight;
        out.numel = io->weight_numel;
        out.on_device = 0;
        rc = m3pc_mtm_weights_export(h, &out, 1, stream);
    }
    if (rc == 0) {
        if (hipMemcpyAsync(io->records, io->records_dev, MTM_TRAIN_STEPS * M3PC_MTM_LOSS_FLOATS * sizeof(float), hipMemcpyDeviceToHost,
                           (hipStream_t)stream) != hipSuccess ||
            hipMemcpyAsync(io->train_records, io->train_records_dev, MTM_TRAIN_STEPS * 3 * sizeof(double), hipMemcpyDeviceToHost,
                           (hipStream_t)stream) != hipSuccess ||
            hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
            fprintf(stderr, "mtm_train: the read-back failed\n");
            rc = M3PC_EHIP;
        } else {
            for (int i = 0; i < MTM_TRAIN_STEPS; ++i)
                printf("step %d: total %.9g entropy %.9g | lr %.9g temperature %.12g\n", i, io->records[i * M3PC_MTM_LOSS_FLOATS + 14],
                       io->records[i * M3PC_MTM_LOSS_FLOATS + 12], io->train_records[3 * i], io->train_records[3 * i + 1]);
            printf("%s [0] = %.9g\n", io->weight_name, io->weight[0]);
        }
    }
    if (rc != 0 && rc != M3PC_EHIP) fprintf(stderr, "mtm_train: %d: %s\n", rc, m3pc_last_error());
    /* the destroys drain the device before they free: the optimizer before its gradient object, that before the handle */
    m3pc_mtm_opt_destroy(opt);
    m3pc_mtm_grad_destroy(g);
    m3pc_replay_destroy(rb);
    m3pc_destroy(h);
    return rc;
}

int mtm_train_example(mtm_train_io* io, int device, void* stream) { return mtm_train_example_dropout(io, device, stream, 0.0, 0); }
