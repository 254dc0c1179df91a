#pragma once
#include "common.h"

namespace smk {
constexpr int FLOW_MIN_DIM = 32, FLOW_MAX_DIM = 1024, FLOW_MAX_LEVELS = 3;
constexpr int LK_MAX_CORNERS = 100, LK_MAX_LEVEL = 2;

int flow_levels(int H, int W);                              // Farneback pyramid depth K (1..3); 0 for an unsupported shape
void flow_level_size(int H, int W, int level, int *h, int *w);
size_t farneback_workspace_bytes(int n, int H, int W);
size_t warp_workspace_bytes(int n, int H, int W);
size_t lk_workspace_bytes(int n, int H, int W);

hipError_t launch_flow_level_image(const uint8_t *frames, int n, int H, int W, int level, float *out, void *ws, hipStream_t st);
hipError_t launch_flow_poly_exp(const float *img, int n, int h, int w, float *coef, hipStream_t st);
hipError_t launch_flow_iteration(const float *coef0, const float *coef1, float *flow, int n, int h, int w, void *ws, hipStream_t st);
hipError_t launch_flow_farneback(const uint8_t *prev, const uint8_t *next, int n, int H, int W, float *flow, void *ws, hipStream_t st);
hipError_t launch_warp_frames(const uint8_t *prev, const float *flow, const uint8_t *next, int n, int H, int W, uint8_t *pred,
                              double *mse, void *ws, hipStream_t st);
hipError_t launch_flow_min_eigen(const uint8_t *frames, int n, int H, int W, float *eig, hipStream_t st);
hipError_t launch_good_features(const float *eig, int n, int H, int W, float *pts, int32_t *counts, void *ws, hipStream_t st);
hipError_t launch_lk_track(const uint8_t *prev, const uint8_t *next, int n, int H, int W, const float *pts, const int32_t *counts,
                           float *out_pts, uint8_t *status, void *ws, hipStream_t st);
hipError_t launch_lk_scatter(const float *pts, const float *out_pts, const uint8_t *status, const int32_t *counts, int n, int H, int W,
                             float *flow, hipStream_t st);
hipError_t launch_flow_lucas_kanade(const uint8_t *prev, const uint8_t *next, int n, int H, int W, float *flow, void *ws, hipStream_t st);
}  // namespace smk
