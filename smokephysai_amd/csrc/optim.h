#pragma once
#include "common.h"

namespace smk {

// Gradient clip + AdamW over a HOST table of tensors (smk_opt_tensor), as multi-tensor launches: the descriptors of up to OPT_BATCH
// tensors travel by value in the kernel arguments (no device allocation, no host-to-device copy whose source could be overwritten before
// it runs).  Work is cut into chunks of OPT_CHUNK elements counted from element 0 of each tensor, one workgroup per chunk.
constexpr int OPT_CHUNK = 8192;      // elements per workgroup: 256 threads x 8 x float4
constexpr int OPT_BATCH = 64;        // tensors per launch (the AdamW descriptor block is 2.8 KB of a 4 KB kernarg)
constexpr int OPT_THREADS = 256;

struct AdamCoef {
    float lr_wd;       // lr * weight_decay
    float w1;          // 1 - beta1
    float beta2, w2;   // beta2, 1 - beta2
    float step;        // lr / bias_correction1
    float rsq_bc2;     // sqrt(bias_correction2)
    float eps;
};

int64_t opt_chunks(const smk_opt_tensor *t, int n_tensors);      // sum over tensors of ceil(n / OPT_CHUNK); -1 for a negative n
hipError_t launch_grad_norm(const smk_opt_tensor *t, int n_tensors, float max_norm, float *out, double *partial, hipStream_t st);
hipError_t launch_adamw(const smk_opt_tensor *t, int n_tensors, const AdamCoef &c, const float *grad_scale, int write_grad,
                        hipStream_t st);

}  // namespace smk
