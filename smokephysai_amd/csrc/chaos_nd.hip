// Chaos statistics of n volumes [D][H][W] (SPEC_3D.md section 9: the n-axis form of smoke_simulator.py:47-140's reductions), with many
// workgroups per volume and no size ceiling.  D == 1 is the 2-axis instance: s x s boxes on [H][W], the rule of chaos.hip.
//   mean      : fp64 sum over all voxels / cells, rounded once to fp32 (chaos.hip:3)
//   box counts: cubes of edge s = 2,4,8,16,32 of (vol > mean) on the (D/s) x (H/s) x (W/s) grid (:89-124; upper remainders ignored)
//   histogram : torch.histogram(bins=256, range=(0,1)) counts (:134-135): outside [0,1] dropped, 1.0 -> bin 255
//   norms     : ||vol[i+1] - vol[i]||_2 (:73-79), fp64 accumulation, fp32 result
// Two launches (a memset of the integer outputs in front):
//   k_vol_reduce : P workgroups per volume, each streams one contiguous chunk (16-byte loads where the addresses allow) and leaves an fp64
//                  partial sum, an fp64 partial of the squared difference to the next volume, and its histogram (per-wave LDS histograms for
//                  the bins 1..255; bin 0 -- nine voxels in ten of a smoke volume -- is a per-thread register count), flushed with integer adds.
//   k_vol_boxes  : every workgroup rebuilds the mean from the P partials in ascending order (the same order everywhere), takes one
//                  32-aligned brick, forms the level-2 flags from 16-byte loads, reduces them level by level in LDS and issues at most five
//                  integer adds.  A box whose far corner passes the extent does not exist: its flag is 0 and it is never counted, and then
//                  neither is any larger box that contains it.  The first workgroup of a volume also writes its mean and its norm.
// Determinism: integer adds commute; every fp64 sum has one order (thread-strided within a chunk, the shuffle tree, waves ascending, chunks
// ascending).  No float atomics.
#include "chaos.h"

namespace smk {

namespace {

constexpr int VS_NT = 256;                                    // threads per workgroup, both kernels
constexpr int VS_MAX_P = 256;                                 // chunks per volume at most (= VS_NT: k_vol_boxes loads one partial per thread)
constexpr int VS_MIN_CHUNK = 16384;                           // cells per chunk at least

// the fixed partition of a volume: a function of the cell count alone
inline int vs_chunks(int64_t cells) {
    int64_t p = (cells + VS_MIN_CHUNK - 1) / VS_MIN_CHUNK;
    return (int)(p < 1 ? 1 : (p > VS_MAX_P ? VS_MAX_P : p));
}
inline int vs_chunk_cells(int64_t cells, int P) {
    return (int)(((cells + P - 1) / P + 3) / 4 * 4);          // a multiple of 4: chunk starts keep the volume's 16-byte alignment
}

__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

__device__ __forceinline__ int wave_sum32(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// block-wide sum of one double per thread (4 waves), fixed order; valid in thread 0
__device__ __forceinline__ double block_sum4(double v, double *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = wave_sum64(v);
    __syncthreads();                                          // red may still be read from the previous use
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

struct F4 {
    float v[4];
};

// four consecutive cells from cell index i of a volume; cells at or past `end` read as NaN (no bin, no sum: the callers test i + j < end)
__device__ __forceinline__ F4 load4(const float *__restrict__ p, int i, int end, bool vec) {
    F4 r;
    if (vec && i + 3 < end) {
        const float4 q = *reinterpret_cast<const float4 *>(p + i);
        r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) r.v[j] = i + j < end ? p[i + j] : 0.f;
    }
    return r;
}

template <bool NORMS>
__global__ __launch_bounds__(VS_NT) void k_vol_reduce(const float *__restrict__ vols, int64_t stride, int n, int cells, int P, int chunk,
                                                      int vec, int32_t *__restrict__ hist, double *__restrict__ psum,
                                                      double *__restrict__ psq) {
    __shared__ int lhist[4][256];
    __shared__ double red[4];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int v = blockIdx.x % n, c = blockIdx.x / n;          // volume fastest: the chunk c of v + 1 is read by two workgroups close in time
    const float *a = vols + (size_t)v * stride;
    const bool pair = NORMS && v + 1 < n;
    const float *b = pair ? a + stride : a;
    for (int k = tid; k < 4 * 256; k += VS_NT) (&lhist[0][0])[k] = 0;
    __syncthreads();
    const int begin = c * chunk;                               // c * chunk < cells + 4 P: no overflow below 2^31 - 1024 cells (checked by the caller)
    const int end = begin + chunk < cells ? begin + chunk : cells;
    double s = 0.0, q = 0.0;
    int zeros = 0;
    constexpr int U = 4;                                       // 16-byte loads in flight per thread and stream
    for (int i0 = begin + tid * 4; i0 < end; i0 += U * VS_NT * 4) {
        F4 xa[U], xb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * VS_NT * 4;
            xa[u] = load4(a, i, end, vec);
            if (pair) xb[u] = load4(b, i, end, vec);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * VS_NT * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (i + j >= end) continue;
                const float x = xa[u].v[j];
                s += (double)x;
                if (pair) {
                    const double d = (double)xb[u].v[j] - (double)x;
                    q += d * d;
                }
                if (x >= 0.f && x <= 1.f) {
                    int bin = (int)(x * 256.0f);               // exact: power-of-two scale
                    bin = bin > 255 ? 255 : bin;
                    if (bin == 0) ++zeros;
                    else atomicAdd(&lhist[wave][bin], 1);
                }
            }
        }
    }
    zeros = wave_sum32(zeros);
    if ((tid & 63) == 0 && zeros) atomicAdd(&lhist[wave][0], zeros);
    const double ts = block_sum4(s, red);
    if (tid == 0) psum[(size_t)v * P + c] = ts;
    if (NORMS) {
        const double tq = block_sum4(q, red);
        if (tid == 0 && pair) psq[(size_t)v * P + c] = tq;
    }
    __syncthreads();
    const int h = lhist[0][tid] + lhist[1][tid] + lhist[2][tid] + lhist[3][tid];      // VS_NT == 256 bins
    if (h) atomicAdd(&hist[(size_t)v * 256 + tid], h);
}

// Brick geometry in level-2 boxes.  3-D: 16 x 16 x 16 boxes of 2 x 2 x 2 cells (a 32^3 brick).  2-D: 1 x 64 x 128 boxes of 1 x 2 x 2 cells
// (a 128 x 256 brick): the same 32768 cells per workgroup.
template <bool IS3D>
struct Brick {
    static constexpr int NZ2 = IS3D ? 16 : 1, NY2 = IS3D ? 16 : 64, NX2 = IS3D ? 16 : 128;
    static constexpr int CZ = IS3D ? 32 : 1, CY = 2 * NY2, CX = 2 * NX2;              // cells
    static constexpr int ZS = IS3D ? 1 : 0;                                           // the z extent halves per level only in 3-D
};

template <bool IS3D>
__global__ __launch_bounds__(VS_NT) void k_vol_boxes(const float *__restrict__ vols, int64_t stride, int n, int D, int H, int W, int P,
                                                     int vec, int nbz, int nby, int nbx, const double *__restrict__ psum,
                                                     const double *__restrict__ psq, float *__restrict__ means,
                                                     int32_t *__restrict__ box_counts, float *__restrict__ norms) {
    using B = Brick<IS3D>;
    __shared__ unsigned char f0[B::NZ2 * B::NY2 * B::NX2];     // levels 2, 8, 32
    __shared__ unsigned char f1[B::NZ2 * B::NY2 * B::NX2 / 4]; // levels 4, 16 (a quarter of level 2 in 2-D, an eighth in 3-D)
    __shared__ double part[VS_MAX_P];
    __shared__ float smean;
    __shared__ int lcount[5];
    const int tid = threadIdx.x;
    unsigned id = blockIdx.x;
    const int bx = id % nbx; id /= nbx;
    const int by = id % nby; id /= nby;
    const int bz = id % nbz;
    const int v = id / nbz;
    const bool first = bx == 0 && by == 0 && bz == 0;
    const float *f = vols + (size_t)v * stride;
    const int cells = D * H * W;

    // the mean, from the partials in ascending order
    if (tid < P) part[tid] = psum[(size_t)v * P + tid];
    if (tid < 5) lcount[tid] = 0;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int c = 0; c < P; ++c) t += part[c];
        const float m = (float)(t / (double)cells);
        smean = m;
        if (first) means[v] = m;
    }
    __syncthreads();
    const float mean = smean;
    if (first && norms != nullptr && v + 1 < n) {              // workgroup-uniform
        if (tid < P) part[tid] = psq[(size_t)v * P + tid];
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int c = 0; c < P; ++c) t += part[c];
            norms[v] = (float)sqrt(t);
        }
    }

    // level 2: a unit is two boxes side by side in x = four cells of 2 (1 in 2-D) planes x 2 rows
    const int z0 = bz * B::CZ, y0 = by * B::CY, x0 = bx * B::CX;
    const int nz2 = D >> B::ZS, ny2 = H >> 1, nx2 = W >> 1;    // level-2 boxes of the volume (2-D: nz2 = D = 1)
    constexpr int UX = B::NX2 / 2, UNITS = B::NZ2 * B::NY2 * UX;
    int cnt = 0;
#pragma unroll 2
    for (int u = tid; u < UNITS; u += VS_NT) {
        const int ux = u % UX, uy = (u / UX) % B::NY2, uz = u / (UX * B::NY2);
        const int gz2 = (z0 >> B::ZS) + uz, gy2 = (y0 >> 1) + uy, gx2 = (x0 >> 1) + 2 * ux;
        bool a0 = false, a1 = false;
        if (gz2 < nz2 && gy2 < ny2 && gx2 < nx2) {             // the left box exists: its 2 x 2 (x 2) cells are inside the volume
            const bool two = gx2 + 1 < nx2;                    // and so does the right one
            const int x = 2 * gx2;
#pragma unroll
            for (int dz = 0; dz <= B::ZS; ++dz)
#pragma unroll
                for (int dy = 0; dy < 2; ++dy) {
                    const int row = (((gz2 << B::ZS) + dz) * H + 2 * gy2 + dy) * W + x;      // < cells < 2^31
                    if (vec && two) {
                        const float4 q = *reinterpret_cast<const float4 *>(f + row);
                        a0 |= q.x > mean || q.y > mean;
                        a1 |= q.z > mean || q.w > mean;
                    } else {
                        a0 |= f[row] > mean || f[row + 1] > mean;
                        if (two) a1 |= f[row + 2] > mean || f[row + 3] > mean;
                    }
                }
        }
        f0[(uz * B::NY2 + uy) * B::NX2 + 2 * ux] = a0;
        f0[(uz * B::NY2 + uy) * B::NX2 + 2 * ux + 1] = a1;
        cnt += (int)a0 + (int)a1;
    }
    cnt = wave_sum32(cnt);
    if ((tid & 63) == 0 && cnt) atomicAdd(&lcount[0], cnt);
    __syncthreads();

    // levels 4, 8, 16, 32: a box has a set cell iff one of its half-size boxes has; a box that does not exist whole is not counted and
    // passes 0 upwards (every box that contains it passes the extent too)
    unsigned char *src = f0, *dst = f1;
    int sz = B::NZ2, sy = B::NY2, sx = B::NX2;                 // extent of the source level in this brick
#pragma unroll
    for (int lvl = 1; lvl < 5; ++lvl) {
        const int s = 2 << lvl;                                // box edge in cells
        const int tz = IS3D ? sz >> 1 : 1, ty = sy >> 1, tx = sx >> 1;
        const int gz = IS3D ? D / s : 1, gy = H / s, gx = W / s;                       // boxes of the volume at this level
        const int oz = IS3D ? z0 / s : 0, oy = y0 / s, ox = x0 / s;                    // this brick's first box
        int c2 = 0;
        for (int k = tid; k < tz * ty * tx; k += VS_NT) {
            const int kx = k % tx, ky = (k / tx) % ty, kz = k / (tx * ty);
            unsigned char any = 0;
#pragma unroll
            for (int dz = 0; dz <= B::ZS; ++dz)
#pragma unroll
                for (int dy = 0; dy < 2; ++dy) {
                    const unsigned char *p = src + (((kz << B::ZS) + dz) * sy + 2 * ky + dy) * sx + 2 * kx;
                    any |= p[0] | p[1];
                }
            if (oz + kz >= gz || oy + ky >= gy || ox + kx >= gx) any = 0;
            dst[k] = any;
            c2 += any;
        }
        c2 = wave_sum32(c2);
        if ((tid & 63) == 0 && c2) atomicAdd(&lcount[lvl], c2);
        __syncthreads();
        unsigned char *t = src; src = dst; dst = t;
        sz = tz; sy = ty; sx = tx;
    }
    if (tid < 5 && lcount[tid]) atomicAdd(&box_counts[(size_t)v * 5 + tid], lcount[tid]);
}

}  // namespace

int64_t volume_stats_workspace(int n, int64_t cells) {
    const int P = vs_chunks(cells);
    return (int64_t)(2 * n - 1) * P * (int64_t)sizeof(double);   // [n][P] sums, then [n-1][P] squared differences
}

hipError_t launch_volume_stats(const float *vols, int64_t stride, int n, int D, int H, int W, float *means, int32_t *box_counts,
                               int32_t *hist, float *norms, void *workspace, hipStream_t st) {
    const int64_t cells64 = (int64_t)D * H * W;
    const int P = vs_chunks(cells64), chunk = vs_chunk_cells(cells64, P), cells = (int)cells64;
    if ((int64_t)P * chunk + 4096 >= (1LL << 31)) return hipErrorInvalidValue;
    double *psum = (double *)workspace, *psq = psum + (size_t)n * P;
    // 16-byte loads: the base, the volume stride and every row start (box kernel) keep the alignment
    const int vec_a = ((uintptr_t)vols & 15) == 0 && stride % 4 == 0;
    const int vec_b = vec_a && W % 4 == 0;
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)n * 256 * sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(box_counts, 0, (size_t)n * 5 * sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    const long long ga = (long long)n * P;
    if (ga > 0x7fffffffLL) return hipErrorInvalidValue;
    if (norms != nullptr && n > 1)
        hipLaunchKernelGGL(k_vol_reduce<true>, dim3((unsigned)ga), dim3(VS_NT), 0, st, vols, stride, n, cells, P, chunk, vec_a, hist, psum, psq);
    else
        hipLaunchKernelGGL(k_vol_reduce<false>, dim3((unsigned)ga), dim3(VS_NT), 0, st, vols, stride, n, cells, P, chunk, vec_a, hist, psum, psq);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (D == 1) {
        using B = Brick<false>;
        const int nby = cdiv(H, B::CY), nbx = cdiv(W, B::CX);
        const long long gb = (long long)n * nby * nbx;
        if (gb > 0x7fffffffLL) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_vol_boxes<false>, dim3((unsigned)gb), dim3(VS_NT), 0, st, vols, stride, n, D, H, W, P, vec_b, 1, nby, nbx, psum,
                           psq, means, box_counts, norms);
    } else {
        using B = Brick<true>;
        const int nbz = cdiv(D, B::CZ), nby = cdiv(H, B::CY), nbx = cdiv(W, B::CX);
        const long long gb = (long long)n * nbz * nby * nbx;
        if (gb > 0x7fffffffLL) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_vol_boxes<true>, dim3((unsigned)gb), dim3(VS_NT), 0, st, vols, stride, n, D, H, W, P, vec_b, nbz, nby, nbx, psum,
                           psq, means, box_counts, norms);
    }
    return hipGetLastError();
}

}  // namespace smk
