// What the plans of the moving cameras share (orbit_plan.h, camera_plan.h): the azimuth rule and the number of samples on a ray.  Plain
// C++ for host and device, as they are.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VIEW_HD __host__ __device__ inline
#else
#define VIEW_HD inline
#endif

namespace smk {

// The angle rule: r = remainder(azimuth, 360) in double; a multiple of 90 gives exactly (1,0), (0,1), (-1,0) or (0,-1), anything else
// cos / sin of r * pi / 180 in double; both cast to fp32 once.  Host only.
inline void orbit_cos_sin(double azimuth_deg, float *c, float *s) {
    const double r = remainder(azimuth_deg, 360.0);            // [-180, 180]
    const double q = r / 90.0;
    if (q == -2.0 || q == 2.0) { *c = -1.f; *s = 0.f; return; }
    if (q == -1.0) { *c = 0.f; *s = -1.f; return; }
    if (q == 0.0) { *c = 1.f; *s = 0.f; return; }
    if (q == 1.0) { *c = 0.f; *s = 1.f; return; }
    const double rad = r * (3.14159265358979323846 / 180.0);
    *c = (float)cos(rad);
    *s = (float)sin(rad);
}

// S: the smallest integer >= sqrt(q) with the parity of D; q: the sum of the squared extents a ray can cross (integer arithmetic: no
// rounding to argue about)
VIEW_HD int ray_samples(long long q, int D) {
    long long s = (long long)sqrt((double)q);
    while (s * s < q) ++s;
    while (s > 0 && (s - 1) * (s - 1) >= q) --s;
    if (((s - D) & 1) != 0) ++s;
    return (int)s;
}

}  // namespace smk
