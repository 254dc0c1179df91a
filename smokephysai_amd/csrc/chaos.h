#pragma once
#include "common.h"

namespace smk {
hipError_t launch_chaos_stats(const float *frames, int64_t stride, int n, int H, int W, float *means, int32_t *box_counts,
                              int32_t *hist, hipStream_t st);
hipError_t launch_diff_norms(const float *frames, int64_t stride, int n_pairs, int n_cells, float *norms, hipStream_t st);
hipError_t launch_chaos_features(const float *norms, const int32_t *box_counts, const int32_t *hist, int S, const int32_t *pos,
                                 const int32_t *hist_len, int F, int n_groups, double *features, double *means, hipStream_t st);
// chaos_nd.hip: the same reductions for n volumes [D][H][W] (D == 1: frames), many workgroups per volume; workspace of
// volume_stats_workspace(n, D*H*W) bytes; norms may be NULL
int64_t volume_stats_workspace(int n, int64_t cells);
hipError_t launch_volume_stats(const float *vols, int64_t stride, int n, int D, int H, int W, float *means, int32_t *box_counts,
                               int32_t *hist, float *norms, void *workspace, hipStream_t st);
}  // namespace smk
