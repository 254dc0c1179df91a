#pragma once
#include "common.h"

namespace smk {

// Training-mode BatchNorm2d (batch statistics) + ReLU + P x P mean pooling over an NCHW fp32 tensor -- the encoder's
// norm / activation / pool blocks under autograd (smokephys_net.py:24-32,87-91; train.py:88-89).
struct BnTrainArgs {
    const float *z;              // [B][C][H][W] convolution output
    const float *gamma, *beta;   // [C]
    int B, C, H, W, pool;        // bn_pool_built(pool); pool > 1 needs W == 32 * pool and H * W % bn_chunk_floats(pool) == 0
    float eps;
    float *part;                 // workspace: [C][nchunks][2] partial sums (bn_train_workspace_floats)
    // forward
    float *out;                  // [B][C][H/pool][W/pool]
    float *mean, *var, *rstd;    // [C]: batch mean, biased batch variance, 1 / sqrt(var + eps)
    // backward
    const float *dout;           // [B][C][H/pool][W/pool]
    float *dz;                   // [B][C][H][W]
    float *dgamma, *dbeta;       // [C]
    // cross-rank statistics (SyncBatchNorm): element count of the GLOBAL batch per channel for the dz formula; 0 = B * H * W
    float count;
};

// THE statement of the tiling: floats of one (b, c) plane per workgroup.  bn_check (api.hip), the workspace size and every launch grid
// derive from these; BnShape<P> is the same number at compile time.  Pool 1, 2, 4: 4,096 floats (with pooling: 64 / 16 rows of cells);
// pool 8: 16,384 (8 rows of cells); pool 16 and 32: ONE row of cells, P rows x 32 P columns.
constexpr bool bn_pool_built(int pool) { return pool == 1 || pool == 2 || pool == 4 || pool == 8 || pool == 16 || pool == 32; }
constexpr int bn_chunk_floats(int pool) { return pool == 8 ? 16384 : pool == 16 ? 8192 : pool == 32 ? 32768 : 4096; }
inline long long bn_chunks_per_plane(int H, int W, int pool) {      // whole chunks, but for pool 1 from given statistics (smk_bn_relu_pool_phase)
    return ((long long)H * W + bn_chunk_floats(pool) - 1) / bn_chunk_floats(pool);
}
template <int P> struct BnShape {
    static constexpr int CHUNK = bn_chunk_floats(P);         // floats of one plane per workgroup
    static constexpr int NK = CHUNK / (256 * 4);             // float4 per thread
    static constexpr int G = P >= 16 ? 8 : 1;                // pool 16 / 32: a thread issues its loads of z eight rows at a time, then works on them
};

long long bn_train_workspace_floats(int B, int C, int H, int W, int pool);
hipError_t launch_bn_relu_pool_forward(const BnTrainArgs &a, hipStream_t st);
hipError_t launch_bn_relu_pool_backward(const BnTrainArgs &a, hipStream_t st);
// The same passes one at a time, for statistics that span several processes (the caller all-reduces between them):
//   stats:  z -> mean / var / rstd of THIS process's batch;   apply: out from given mean / rstd;
//   sums:   dout, z, given mean / rstd -> dgamma / dbeta of this process;   dz: from given TOTAL dgamma / dbeta and a.count.
hipError_t launch_bn_stats(const BnTrainArgs &a, hipStream_t st);
hipError_t launch_bn_relu_pool_apply(const BnTrainArgs &a, hipStream_t st);
hipError_t launch_bn_relu_pool_backward_sums(const BnTrainArgs &a, hipStream_t st);
hipError_t launch_bn_relu_pool_backward_dz(const BnTrainArgs &a, hipStream_t st);

}  // namespace smk
