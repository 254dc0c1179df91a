// Modified Gram-Schmidt over the T tangent states of every grid: the kernels behind smk_tangent_orthonormalize and
// smk_tangent3d_orthonormalize.  DESIGN.md section 3.13.
//
// The rule, per grid, for j = 0 .. T-1 (what physics/fluid_tangent.py's _gram_schmidt computes, in the right-looking order: a finished
// vector is removed from all later ones at once, which does the same operations on every vector in the same sequence):
//     n_j = sqrt(sum (double)x (double)x) over the whole state of vector j;  norms[b * T + j] = n_j
//     vector j /= (float)n_j (true fp32 divide) unless n_j is 0 or not finite (as fp64 or as fp32)
//     for i > j:  c = sum (double)q (double)x over (vector j, vector i);  x <- x - (float)c * q  (one rounded multiply, one rounded subtract)
//
// One kernel body serves both dimensions: it is written over a row map (a state is a list of rows (pointer, columns); vector t of grid b
// is state b * T + t, the same row `stride` elements further per vector), and the two maps are the renorm kernels' (ft_row of
// csrc/fluid_tangent.hip, ft3_row of csrc/fluid_tangent3d.h).  Every sum is smk_tangent_renorm's two-level fp64 sum: a workgroup owns a run
// of consecutive rows, wave w its rows w, w + 4, ..., lane l their columns l, l + 64, ...; a thread adds its terms in that order, the 256
// threads are folded by halves, and the runs are added in ascending order by one thread.  No atomics; bit-identical from call to call; a
// grid's result does not depend on its batch mates.
//
// Launches: 2 T (tangent_qr.h: tq_launches).  k_tq_sumsq forms the runs' sums of squares of vector 0; then per vector j k_tq_scale_dots adds
// them, reports the norm, scales its rows and writes the runs' dot products with the T-1-j later vectors, and (for j < T-1) k_tq_update
// adds those, updates the later vectors' rows and forms the runs' sums of squares of vector j + 1.  T = 1 is smk_tangent_renorm's two
// kernels, operation for operation.
#include "tangent_qr.h"

#include "fluid_trace.h"
#include "fluid_trace3d.h"

namespace smk {

namespace {

struct TqRow {
    float *p;            // the row's first column in the first state asked for
    int cols;
    size_t stride;       // elements from this row to the same row of the grid's next vector
};

// ft_row (csrc/fluid_tangent.hip): 4H + 1 rows -- u's H + 1 of W, v's H of W + 1, p's H of W, density's H of W.
struct Map2 {
    Geom g;
    float *tu, *tv, *tp, *td;
    __device__ __forceinline__ int64_t rows() const { return 4 * g.H + 1; }
    __device__ __forceinline__ TqRow row(int bt, int64_t r64) const {
        int r = (int)r64;
        if (r <= g.H) return {tu + (size_t)bt * g.su + (size_t)r * g.pc, g.W, g.su};
        r -= g.H + 1;
        if (r < g.H) return {tv + (size_t)bt * g.sv + (size_t)r * g.pv, g.W + 1, g.sv};
        r -= g.H;
        if (r < g.H) return {tp + (size_t)bt * g.sc + (size_t)r * g.pc, g.W, g.sc};
        r -= g.H;
        return {td + (size_t)bt * g.sc + (size_t)r * g.pc, g.W, g.sc};
    }
};

// ft3_row (csrc/fluid_tangent3d.h): u's D (H + 1) rows, v's D H, w's (D + 1) H, p's D H, density's D H, planes before rows.
struct Map3 {
    Geom3 g;
    float *tu, *tv, *tw, *tp, *td;
    __device__ __forceinline__ int64_t rows() const { return ft3_rows(g.D, g.H); }
    __device__ __forceinline__ TqRow row(int bt, int64_t r) const {
        const Ft3Row q = ft3_row(g.D, g.H, g.W, g.pc, g.pv, r);
        float *base = q.field == 0 ? tu : q.field == 1 ? tv : q.field == 2 ? tw : q.field == 3 ? tp : td;
        const size_t stride = q.field == 0 ? g.su : q.field == 1 ? g.sv : q.field == 2 ? g.sw : g.sc;
        return {base + (size_t)bt * stride + q.offset, q.cols, stride};
    }
};

// Per grid b the workspace holds T * P doubles (P = gridDim.x runs): the runs' sums of squares of the current vector, then for the i-th
// later vector (i = 0 .. T-2) the runs' dot products with it.
__device__ __forceinline__ double *tq_work(double *work, int b, int T, int P) { return work + (size_t)b * T * P; }

// The runs' sums of squares of vector 0 (k_tangent_sumsq on state b * T).
template <class Map>
__global__ __launch_bounds__(TQ_NT) void k_tq_sumsq(Map m, int T, int rpg, double *__restrict__ work) {
    __shared__ double part[TQ_NT];
    const int b = blockIdx.y, p = blockIdx.x, P = gridDim.x, tid = threadIdx.x;
    const int64_t rows = m.rows(), r0 = (int64_t)p * rpg, r1 = r0 + rpg < rows ? r0 + rpg : rows;
    double acc = 0.0;
    for (int64_t r = r0 + (tid >> 6); r < r1; r += TQ_NT / 64) {
        const TqRow row = m.row(b * T, r);
        for (int c = tid & 63; c < row.cols; c += 64) {
            const double x = (double)row.p[c];
            acc = acc + x * x;
        }
    }
    part[tid] = acc;
    for (int s = TQ_NT / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (tid < s) part[tid] = part[tid] + part[tid + s];
    }
    if (tid == 0) tq_work(work, b, T, P)[p] = part[0];
}

// Vector j of grid b: every workgroup adds the P sums of squares in ascending order (all get the same words), the first one reports the
// norm, each divides its own rows by (float)norm with a true fp32 divide -- unless the norm is 0 or not finite (as fp64 or as fp32): then
// the rows stay as they are -- and sums, in fp64, the products of its rows with the same rows of the N = T-1-j later vectors.
template <class Map, int N>
__global__ __launch_bounds__(TQ_NT) void k_tq_scale_dots(Map m, int T, int j, int rpg, double *__restrict__ work, double *__restrict__ norms) {
    __shared__ double part[N > 0 ? N : 1][TQ_NT];
    __shared__ double total;
    const int b = blockIdx.y, p = blockIdx.x, P = gridDim.x, tid = threadIdx.x;
    double *const base = tq_work(work, b, T, P);
    if (tid == 0) {
        double t = 0.0;
        for (int c = 0; c < P; ++c) t = t + base[c];
        total = sqrt(t);
        if (p == 0) norms[(size_t)b * T + j] = total;
    }
    __syncthreads();
    const double norm = total;
    const float d = (float)norm;
    const bool scale = norm > 0.0 && isfinite(norm) && isfinite(d);            // (workgroup-uniform; NaN fails the first test)
    if (N == 0 && !scale) return;
    const int64_t rows = m.rows(), r0 = (int64_t)p * rpg, r1 = r0 + rpg < rows ? r0 + rpg : rows;
    double acc[N > 0 ? N : 1];
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = 0.0;
    for (int64_t r = r0 + (tid >> 6); r < r1; r += TQ_NT / 64) {
        const TqRow row = m.row(b * T + j, r);
        for (int c = tid & 63; c < row.cols; c += 64) {
            float x[N > 0 ? N : 1];                                             // (all loads before the store: the rows may not alias, the compiler cannot know)
#pragma unroll
            for (int i = 0; i < N; ++i) x[i] = row.p[(size_t)(i + 1) * row.stride + c];
            float q = row.p[c];
            if (scale) {
                q = __fdiv_rn(q, d);
                row.p[c] = q;
            }
#pragma unroll
            for (int i = 0; i < N; ++i) acc[i] = acc[i] + (double)q * (double)x[i];
        }
    }
    if (N == 0) return;
#pragma unroll
    for (int i = 0; i < N; ++i) part[i][tid] = acc[i];
    for (int s = TQ_NT / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (tid < s) {
#pragma unroll
            for (int i = 0; i < N; ++i) part[i][tid] = part[i][tid] + part[i][tid + s];
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) base[(size_t)(i + 1) * P + p] = part[i][0];
    }
}

// The N = T-1-j >= 1 vectors after vector j of grid b: every workgroup adds the P partial dot products of each in ascending order, turns
// the sums into fp32 coefficients and takes (float)c * q from its own rows of each later vector, then sums the squares of what is left of
// vector j + 1 for the next round.
template <class Map, int N>
__global__ __launch_bounds__(TQ_NT) void k_tq_update(Map m, int T, int j, int rpg, double *__restrict__ work) {
    __shared__ double part[TQ_NT];
    __shared__ float coef[N];
    const int b = blockIdx.y, p = blockIdx.x, P = gridDim.x, tid = threadIdx.x;
    double *const base = tq_work(work, b, T, P);
    if (tid < N) {
        double t = 0.0;
        for (int c = 0; c < P; ++c) t = t + base[(size_t)(tid + 1) * P + c];
        coef[tid] = (float)t;
    }
    __syncthreads();
    float cf[N];
#pragma unroll
    for (int i = 0; i < N; ++i) cf[i] = coef[i];
    const int64_t rows = m.rows(), r0 = (int64_t)p * rpg, r1 = r0 + rpg < rows ? r0 + rpg : rows;
    double acc = 0.0;
    for (int64_t r = r0 + (tid >> 6); r < r1; r += TQ_NT / 64) {
        const TqRow row = m.row(b * T + j, r);
        for (int c = tid & 63; c < row.cols; c += 64) {
            const float q = row.p[c];
            float x[N];                                                         // (all loads before the stores, as in k_tq_scale_dots)
#pragma unroll
            for (int i = 0; i < N; ++i) x[i] = row.p[(size_t)(i + 1) * row.stride + c];
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const float prod = cf[i] * q;                                   // (-ffp-contract=off: a rounded multiply, then a rounded subtract)
                x[i] = x[i] - prod;
                row.p[(size_t)(i + 1) * row.stride + c] = x[i];
            }
            acc = acc + (double)x[0] * (double)x[0];
        }
    }
    part[tid] = acc;
    for (int s = TQ_NT / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (tid < s) part[tid] = part[tid] + part[tid + s];
    }
    if (tid == 0) base[p] = part[0];
}

template <class Map, int N>
void tq_round(const Map &m, dim3 grid, int T, int j, int rpg, double *work, double *norms, hipStream_t st) {
    hipLaunchKernelGGL((k_tq_scale_dots<Map, N>), grid, dim3(TQ_NT), 0, st, m, T, j, rpg, work, norms);
    if constexpr (N > 0) hipLaunchKernelGGL((k_tq_update<Map, N>), grid, dim3(TQ_NT), 0, st, m, T, j, rpg, work);
}

template <class Map>
hipError_t tq_launch(const Map &m, int B, int T, int runs, int rpg, double *norms, double *work, hipStream_t st) {
    const dim3 grid((unsigned)runs, (unsigned)B);
    hipLaunchKernelGGL(k_tq_sumsq<Map>, grid, dim3(TQ_NT), 0, st, m, T, rpg, work);
    for (int j = 0; j < T; ++j) {
        switch (T - 1 - j) {
            case 0: tq_round<Map, 0>(m, grid, T, j, rpg, work, norms, st); break;
            case 1: tq_round<Map, 1>(m, grid, T, j, rpg, work, norms, st); break;
            case 2: tq_round<Map, 2>(m, grid, T, j, rpg, work, norms, st); break;
            case 3: tq_round<Map, 3>(m, grid, T, j, rpg, work, norms, st); break;
            case 4: tq_round<Map, 4>(m, grid, T, j, rpg, work, norms, st); break;
            case 5: tq_round<Map, 5>(m, grid, T, j, rpg, work, norms, st); break;
            case 6: tq_round<Map, 6>(m, grid, T, j, rpg, work, norms, st); break;
            default: tq_round<Map, 7>(m, grid, T, j, rpg, work, norms, st); break;
        }
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_tangent_orthonormalize(const Geom &g, int T, float *tu, float *tv, float *tp, float *td, double *norms, double *work,
                                         hipStream_t st) {
    return tq_launch(Map2{g, tu, tv, tp, td}, g.B, T, ft_groups(g.H), ft_rows_per_group(g.H), norms, work, st);
}

hipError_t launch3_tangent_orthonormalize(const Geom3 &g, int T, float *tu, float *tv, float *tw, float *tp, float *td, double *norms,
                                          double *work, hipStream_t st) {
    return tq_launch(Map3{g, tu, tv, tw, tp, td}, g.B, T, ft3_groups(g.D, g.H), ft3_rows_per_group(g.D, g.H), norms, work, st);
}

}  // namespace smk

using namespace smk;

namespace {

// The renorm entry points' limits (csrc/fluid_tangent.hip: ft_shape_ok, csrc/fluid_tangent3d.hip: ft3_shape_ok) and T <= 8.
bool tq_shape_ok(int32_t B, int32_t T, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v) {
    return fluid2d_shape_ok(B, H, W, pitch_c, pitch_v) && T >= 1 && T <= TQ_MAX_T && (int64_t)B * T <= 65535;
}
bool tq3_shape_ok(int32_t B, int32_t T, int32_t D, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v) {
    return fluid3d_shape_ok(B, D, H, W, pitch_c, pitch_v) && T >= 1 && T <= TQ_MAX_T && (int64_t)B * T * (D + 1) <= 65535;
}
const char *const TQ_SHAPE = "B >= 1, 1 <= T <= 8, B * T <= 65535, 3 <= H, W <= 32766, pitch_c >= W, pitch_v >= W + 1";
const char *const TQ3_SHAPE = "B >= 1, 1 <= T <= 8, B * T * (D + 1) <= 65535, 3 <= D, H, W <= 32766, pitch_c >= W, pitch_v >= W + 1, one grid's field below 2^31 elements";

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int64_t smk_tangent_orthonormalize_workspace(int32_t B, int32_t T, int32_t H, int32_t W) {
    if (!tq_shape_ok(B, T, H, W, W, W + 1)) return -1;
    return (int64_t)B * T * ft_groups(H) * (int64_t)sizeof(double);
}

int smk_tangent_orthonormalize(float *tu, float *tv, float *tp, float *td, double *norms, int32_t B, int32_t T, int32_t H, int32_t W,
                               int32_t pitch_c, int32_t pitch_v, void *workspace, int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(tu && tv && tp && td && norms, "tangent_orthonormalize: null pointer");
    SMK_REQUIRE(tq_shape_ok(B, T, H, W, pitch_c, pitch_v), TQ_SHAPE);
    SMK_REQUIRE(workspace && workspace_bytes >= smk_tangent_orthonormalize_workspace(B, T, H, W),
                "tangent_orthonormalize: workspace smaller than smk_tangent_orthonormalize_workspace(B, T, H, W) bytes");
    SMK_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)norms & 7) == 0,
                "tangent_orthonormalize: workspace and norms must be 8-byte aligned");
    Geom g = fluid2d_geom(B * T, H, W, pitch_c, pitch_v, 0.0, 0.0);
    g.B = B;                                                                    // the launch's grids; a grid's T states lie su / sv / sc apart
    return check_launch(launch_tangent_orthonormalize(g, T, tu, tv, tp, td, norms, (double *)workspace, (hipStream_t)stream),
                        "tangent_orthonormalize");
}

int64_t smk_tangent3d_orthonormalize_workspace(int32_t B, int32_t T, int32_t D, int32_t H, int32_t W) {
    if (!tq3_shape_ok(B, T, D, H, W, W, W + 1)) return -1;
    return (int64_t)B * T * ft3_groups(D, H) * (int64_t)sizeof(double);
}

int smk_tangent3d_orthonormalize(float *tu, float *tv, float *tw, float *tp, float *td, double *norms, int32_t B, int32_t T, int32_t D,
                                 int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v, void *workspace, int64_t workspace_bytes,
                                 void *stream) {
    SMK_REQUIRE(tu && tv && tw && tp && td && norms, "tangent3d_orthonormalize: null pointer");
    SMK_REQUIRE(tq3_shape_ok(B, T, D, H, W, pitch_c, pitch_v), TQ3_SHAPE);
    SMK_REQUIRE(workspace && workspace_bytes >= smk_tangent3d_orthonormalize_workspace(B, T, D, H, W),
                "tangent3d_orthonormalize: workspace smaller than smk_tangent3d_orthonormalize_workspace(B, T, D, H, W) bytes");
    SMK_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)norms & 7) == 0,
                "tangent3d_orthonormalize: workspace and norms must be 8-byte aligned");
    const Geom3 g = fluid3d_geom(B, D, H, W, pitch_c, pitch_v, 0.0);
    return check_launch(launch3_tangent_orthonormalize(g, T, tu, tv, tw, tp, td, norms, (double *)workspace, (hipStream_t)stream),
                        "tangent3d_orthonormalize");
}

}  // extern "C"
#pragma GCC visibility pop
