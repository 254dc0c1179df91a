#pragma once
#include "common.h"

namespace smk {
constexpr int QUALITY_MAX_WINDOW = 31;
size_t quality_lds_bytes(int k);
int64_t quality_tiles(int H, int W);         // output tiles per plane: one (ssim, sqerr) fp64 pair of workspace each
hipError_t launch_image_quality(const float *pred, int64_t pred_stride, const float *target, int64_t target_stride, int n, int H,
                                int W, int k, float c1, float c2, void *workspace, double *ssim_sum, double *sqerr_sum,
                                hipStream_t st);
// d(sum_i plane_grad[i] * mean SSIM of plane i) / d pred -> dpred [n][H][W] (plane stride dpred_stride), every element written once;
// workspace: 3 * n * H * W floats (the coefficient planes a, b, c between the two launches)
hipError_t launch_image_quality_backward(const float *pred, int64_t pred_stride, const float *target, int64_t target_stride, int n,
                                         int H, int W, int k, float c1, float c2, const float *plane_grad, void *workspace,
                                         float *dpred, int64_t dpred_stride, hipStream_t st);
}  // namespace smk
