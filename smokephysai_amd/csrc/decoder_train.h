#pragma once
#include "common.h"

namespace smk {

// SmokePhysNet.reconstruction_head under autograd (csrc/decoder_train.hip): the two ConvTranspose2d(k4, s2, p1) layers and the
// Conv2d(16, 1, 3, p1) + Sigmoid, forward and backward, with BatchNorm left to the training-mode kernels of norm.hip.
// Shape rules (checked by the callers in api.hip): COUT in {16, 32}; CIN a multiple of 16 (COUT 32) or 32 (COUT 16); H, W multiples of 16;
// 1 <= B <= 65535.  tok: the ConvT input (forward, wgrad) / data gradient (dgrad) is token-major [B][H*W][CIN] instead of NCHW.
bool convt_train_shape_ok(int B, int CIN, int COUT, int H, int W);
hipError_t launch_convt_train_forward(const float *x, const float *w, const float *bias, int B, int CIN, int COUT, int H, int W, bool tok,
                                      float *z, hipStream_t st);
hipError_t launch_convt_train_dgrad(const float *dz, const float *w, int B, int CIN, int COUT, int H, int W, bool tok, float *dx,
                                    hipStream_t st);
size_t convt_train_wgrad_workspace_bytes(int B, int CIN, int COUT, int H, int W);
hipError_t launch_convt_train_wgrad(const float *dz, const float *x, int B, int CIN, int COUT, int H, int W, bool tok, float *dw, float *db,
                                    void *workspace, hipStream_t st);

// Conv2d(16, 1, 3, padding 1) + Sigmoid: x [B][16][H][W] -> y [B][H][W]; H % 8 == 0, W % 32 == 0.
bool conv3_train_shape_ok(int B, int H, int W);
hipError_t launch_conv3_sigmoid_train_forward(const float *x, const float *w, const float *bias, int B, int H, int W, float *y, hipStream_t st);
size_t conv3_sigmoid_train_workspace_bytes(int B, int H, int W);
hipError_t launch_conv3_sigmoid_train_backward(const float *dy, const float *y, const float *x, const float *w, int B, int H, int W, float *dx,
                                               float *dw, float *db, void *workspace, hipStream_t st);

}  // namespace smk
