#pragma once
#include "common.h"

namespace smk {
constexpr int QUALITY_MAX_WINDOW = 31;
size_t quality_lds_bytes(int k);
int64_t quality_tiles(int H, int W);         // output tiles per plane: one (ssim, sqerr) fp64 pair of workspace each
hipError_t launch_image_quality(const float *pred, int64_t pred_stride, const float *target, int64_t target_stride, int n, int H,
                                int W, int k, float c1, float c2, void *workspace, double *ssim_sum, double *sqerr_sum,
                                hipStream_t st);
}  // namespace smk
