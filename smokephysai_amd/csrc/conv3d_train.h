// Training passes of the 3-D encoder (SPEC_3D.md section 11): the two Conv3d blocks' forward, data and weight gradients and the train-mode
// BatchNorm3d + ReLU (+ token pooling) phases, all on channels-last activations [B][D][H][W][C].  No reference counterpart (the reference's
// encoder is 2-D: smokephys_net.py:24-32); the rules are torch's, stated in the specification.
#pragma once
#include "common.h"

namespace smk {

constexpr int C3T_TH = 8, C3T_TW = 16;                        // a workgroup's tile of one plane: 8 x 16 voxels (= conv3d_march.hip's)
constexpr size_t C3T_W2_BYTES = (size_t)27 * 64 * 128 * 4;    // re-laid conv2 weights [tap][cin][cout] (forward and data gradient alike)
constexpr size_t C3T_W1_BYTES = (size_t)49 * 8 * 64 * 4;      // re-laid conv1 weights [kz * 7 + ky][8 kx slots][64]

inline bool conv3d_train_shape_ok(long long B, long long D, long long H, long long W) {
    if (B < 1 || D < 1 || H < C3T_TH || W < C3T_TW || H % C3T_TH || W % C3T_TW) return false;
    const long long tiles = B * D * (H / C3T_TH) * (W / C3T_TW);
    return tiles < (1LL << 31) && B * D * H * W < (1LL << 40);
}
int conv3d_wgrad_streams(long long tiles);                    // voxel streams per output group: a function of the shape alone
size_t conv3d_wgrad_workspace_bytes(int B, int D, int H, int W);

hipError_t launch_conv3d_cl_train_forward(const float *a1, const float *w2, const float *bias, int B, int D, int H, int W, float *z2, void *ws,
                                          hipStream_t st);
hipError_t launch_conv3d_cl_dgrad(const float *dz2, const float *w2, int B, int D, int H, int W, float *da1, void *ws, hipStream_t st);
hipError_t launch_conv3d_cl_wgrad(const float *dz2, const float *a1, int B, int D, int H, int W, float *dw, float *db, void *ws, hipStream_t st);
hipError_t launch_conv3d_s7_train_forward(const float *vol, const float *w1, const float *bias, int B, int D, int H, int W, float *z1, void *ws,
                                          hipStream_t st);
// dvol [B][D][H][W] = the data gradient of conv1 from dz1 [B][D][H][W][64]; ws holds the re-laid weights [343 taps][64] (87,808 B)
hipError_t launch_conv3d_s7_dgrad(const float *dz1, const float *w1, int B, int D, int H, int W, float *dvol, void *ws, hipStream_t st);

size_t bn_cl_workspace_bytes(long long M, int C);
// phase: smk_bn_phase.  pooled = 0: out / dout are [M][C]; pooled = 1: out = token SUMS [B][1024][C], dout = token gradients [B][1024][C]
hipError_t launch_bn_cl_phase(int phase, const float *z, const float *dout, int B, int D, int H, int W, int C, int pooled, const float *gamma,
                              const float *beta, double eps, float *mean, float *var, float *rstd, float *out, float *dz, float *dgamma,
                              float *dbeta, double count, void *ws, hipStream_t st);

}  // namespace smk
