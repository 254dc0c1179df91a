#pragma once
#include <mutex>
#include <vector>

#include "common.h"

namespace smk {

// Folded / re-laid-out encoder weights on the device (library-owned).
struct EncoderDev {
    float *w1;    // [64][49]           conv1 weights
    float *s1, *t1;   // [64]           folded BN1 scale / shift (conv bias included)
    float *w2t;   // [9][64][128]       conv2 weights, [tap][c][o]
    float *s2, *t2;   // [128]
    // split-bf16 copies for the bf16 MFMA kernels (value = hi + lo, each a bf16):
    unsigned short *w1p;   // [2 hi/lo][64 ch][64 k], k = 8*ki + kj (ki = 7 or kj = 7: zero)
    signed char *w2i;      // [18 k-steps = tap*2 + c/32][2 limbs h|l][128 o][32 c] int8: w = sw2[o] * (256 h + l)
    float *sw2;            // [128] per-output-channel weight scale of the int8 limbs
    int *wsum;             // [2][128] 128 * sum_k of the h / l weight limbs (offset correction of the unsigned activations)
    unsigned short *w2q;   // [36 k-steps = tap*4 + c/16][2 hi/lo][128 o][16 c]  (B fragments, 1 KiB per wave load)
    unsigned short *w2s;   // [18 k-steps = tap*2 + c/32][2 hi/lo][128 o][32 c]  (16x16x32 B fragments: 16 o x 64 B = 1 KiB)
};

// Per-handle state of the tile-skip path (encoder.hip, "tile skip"): lazily built, guarded by mu, released with the handle.
struct EncoderSkip {
    std::mutex mu;
    // zero-response tables [form: bf16x3 | bf16 | i8x3][H: 64 | 128 | 256 | 512 | 1024][layout: NCHW | tokens]; at 512 and 1024 a
    // table holds per-tile partial sums, which have one layout: only [..][..][0] is used there
    float *table[3][5][2] = {};
    int *ws = nullptr;                // workspace: tiles run (written by the main kernel), band masks for ws_bands bands
    size_t ws_bands = 0;
    std::vector<void *> retired;      // outgrown workspaces (captured graphs may still name them)
    int64_t last_total = 0;           // tiles of the last forward ...
    const int *last_count = nullptr;  // ... and where the device keeps how many of them ran (null: direct path, all ran)
    void release();                   // frees the device memory (the handle's device is current)
};
hipError_t encoder_skip_stats(EncoderSkip &sk, int64_t *tiles_total, int64_t *tiles_run, hipStream_t st);

// Per-handle buffer of the frames beyond 256^2 (encoder.hip, "frames beyond 256^2"): per tile and channel the un-normalised sum of
// the tile's 128 activations, [B][H/8][W/16][128] fp32 (1 MB per 512^2 frame, 4 MB per 1024^2 frame).  Independent of the skip state:
// the direct path writes it too.  Grown on demand under mu; outgrown buffers are kept until the handle is destroyed (a captured graph
// may still name them).  Calls on one handle share it, as they share the skip workspace: one stream at a time.
struct EncoderPartials {
    std::mutex mu;
    float *buf = nullptr;
    size_t floats = 0;
    std::vector<void *> retired;
    // The buffer for B frames of H x W in *out, or null in *out when the frame size pools inside a tile (H <= 256).
    // hipErrorStreamCaptureUnsupported: the stream is capturing and the buffer is missing or too small (nothing is allocated inside a
    // capture; an eager call of the same shape creates it).
    hipError_t acquire(int B, int H, int W, hipStream_t st, float **out);
    void release();
};

hipError_t launch_fold_weights(const smk_encoder_weights &w, const EncoderDev &e, hipStream_t st);
hipError_t launch_conv1_only(const float *frames, int64_t fstride, int B, int H, int W, const EncoderDev &e, float *act,
                             hipStream_t st);
// partials (every fused form below): EncoderPartials::acquire's buffer for this call; null for H <= 256.
hipError_t launch_encoder_f32(const float *frames, int64_t fstride, int B, int H, int W, const EncoderDev &e,
                              float *features, hipStream_t st, float *partials = nullptr);

// x3 = true: split-bf16 (hi*hi + hi*lo + lo*hi, ~fp32 accuracy); false: single-pass bf16.
// tokens = true: features written token-major [B][32*32][128] (coalesced; the layout feature_proj consumes).
// skip (all three persistent MFMA forms below): the handle's tile-skip state, or null to run every tile.
hipError_t launch_encoder_bf16(const float *frames, int64_t fstride, int B, int H, int W, const EncoderDev &e,
                               float *features, bool x3, bool tokens, hipStream_t st, EncoderSkip *skip = nullptr,
                               float *partials = nullptr);
// split-bf16 on the 16x16x32 MFMA shape (same arithmetic and tiles; higher sustained clock under the power limit)
hipError_t launch_encoder_b16(const float *frames, int64_t fstride, int B, int H, int W, const EncoderDev &e,
                              float *features, bool tokens, hipStream_t st, EncoderSkip *skip = nullptr, float *partials = nullptr);

// int8 two-limb fixed point (activations scaled per tile, weights per output channel), exact i32 accumulation.
hipError_t launch_encoder_i8(const float *frames, int64_t fstride, int B, int H, int W, const EncoderDev &e,
                             float *features, bool tokens, hipStream_t st, EncoderSkip *skip = nullptr, float *partials = nullptr);

}  // namespace smk
