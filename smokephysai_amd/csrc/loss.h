#pragma once
#include "common.h"

namespace smk {

// The loss terms of train.py's batch_losses (reconstruction MSE, chaos-feature MSE, PhysicsRegularizer's mass-conservation and
// continuity terms) as one forward (two partial-sum launches + a one-workgroup finish) and one backward launch.
constexpr int LOSS_THREADS = 256;
constexpr int LOSS_PLANE_CHUNK = 2048;     // elements of one pred / target plane per workgroup
constexpr int LOSS_SEQ_CHUNK = 1024;       // pixels of one sequence per workgroup (each walked through all T frames)

struct LossShape {
    int planes, plane_elems;               // pred / target: [planes][plane_elems]
    int n_chaos;
    int seq_batch, seq_T;                  // sequence: [seq_batch][seq_T][seq_plane], or seq_batch = 0
    long long seq_plane;
};
int64_t loss_plane_chunks(int plane_elems);            // workgroups per plane
int64_t loss_seq_chunks(long long seq_plane);          // workgroups per sequence
int64_t loss_workspace_doubles(const LossShape &s);

hipError_t launch_train_loss_forward(const float *pred, const float *target, const float *chaos_pred, const float *chaos_target,
                                     const float *sequence, const LossShape &s, double w_chaos, double w_physics, double w_mass,
                                     double w_continuity, float *out, float *mass_diff, double *workspace, hipStream_t st);
hipError_t launch_train_loss_backward(const float *pred, const float *target, const float *mass_diff, const float *chaos_pred,
                                      const float *chaos_target, const LossShape &s, const float *grad_out, double w_chaos,
                                      double w_physics, double w_mass, float *d_pred, float *d_chaos, hipStream_t st);

}  // namespace smk
