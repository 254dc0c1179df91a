#pragma once
#include "common.h"

namespace smk {

// SmokePhysNet.input_encoder's two convolutions under autograd (csrc/encoder_train.hip); NCHW fp32 in and out.
// Training: z2 = conv2(a1) + bias alone (Conv2d(64, 128, 3, padding = 1); NCHW fp32 in and out; H % 8 == 0, W % 16 == 0); `workspace` holds
// the split weights (conv2_train_workspace_bytes), rebuilt from `weight` [128][64][3][3] in the same call.
size_t conv2_train_workspace_bytes();
// dX = the data gradient of the same convolution from dz [B][128][H][W] (same workspace size, its own contents)
hipError_t launch_conv2_train_dgrad(const float *dz, const float *weight, int B, int H, int W, float *dx, void *workspace, hipStream_t st);
// Training passes of the FIRST convolution (Conv2d(1, 64, 7, padding = 3)), fp32 on the vector ALUs: z1 = conv(x) + bias (W % 4 == 0) and
// dW [64][7][7] / db [64] from dz [B][64][H][W] and x [B][H][W] (H % 4 == 0, W % 64 == 0; workspace conv1_wgrad_workspace_bytes()).
size_t conv1_wgrad_workspace_bytes();
hipError_t launch_conv1_train_forward(const float *x, const float *weight, const float *bias, int B, int H, int W, float *z1, hipStream_t st);
hipError_t launch_conv1_train_wgrad(const float *dz, const float *x, int B, int H, int W, float *dw, float *db, void *workspace, hipStream_t st);
// dX [B][H][W] = the data gradient of the first convolution from dz [B][64][H][W] and weight [64][7][7] (W % 4 == 0, B <= 65535; no workspace)
hipError_t launch_conv1_train_dgrad(const float *dz, const float *weight, int B, int H, int W, float *dx, hipStream_t st);
// dW [128][64][3][3] (and db [128] unless NULL) of the same convolution from dz and a1; workspace: conv2_wgrad_workspace_bytes(conv2_wgrad_streams())
size_t conv2_wgrad_workspace_bytes(int nstreams);
int conv2_wgrad_streams();
hipError_t launch_conv2_train_wgrad(const float *dz, const float *a1, int B, int H, int W, float *dw, float *db, void *workspace, hipStream_t st);
hipError_t launch_conv2_train_forward(const float *a1, const float *weight, const float *bias, int B, int H, int W, float *z2, void *workspace,
                                      hipStream_t st);

}  // namespace smk
