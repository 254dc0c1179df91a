#pragma once
// What the fused inference encoder (encoder.hip) and the training convolutions (encoder_train.hip) share: the 8 x 16 output tile
// with its a1 halo, the split-bf16 operand types and the priorities of the 16x16x32 K loops.  Device code only.
#include "common.h"

namespace smk {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

constexpr int B3_TH = 8, B3_TW = 16;                     // output tile
constexpr int B3_AW = B3_TW + 2, B3_APIX = (B3_TH + 2) * B3_AW;   // a1 halo tile: 10 x 18 = 180 pixels
constexpr int S16_A1_BYTES = B3_APIX * 128;              // one plane (hi or lo) of the swizzled a1 image: 23,040

#ifndef S16_PRIO_CONV1
#define S16_PRIO_CONV1 0
#define S16_PRIO_KLOOP 1
#endif

__device__ __forceinline__ void split_bf16(float v, __bf16 &hi, __bf16 &lo) {
    hi = (__bf16)v;
    lo = (__bf16)(v - (float)hi);
}

}  // namespace smk
