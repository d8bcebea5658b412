// What the two surface extractions of a TSDF volume share (tsdf.hip: the zero crossings along the axes; tsdf_mesh.hip:
// the crossings along all seven edge directions, with faces): the arguments, the gradient, and the point and the normal
// of one crossing.  One device function each, so that an axis edge gives the same bits in both.
#pragma once
#include "compaction.hpp"

#pragma clang fp contract(off)

namespace pds {

struct TsdfExtractArgs {
    float origin[3];
    float voxel_size, min_weight;
    int nx, ny, nz, total;
};

// The central-difference gradient of the tsdf at voxel c = (i, j, k); false: one of the six voxels is outside or unobserved
__device__ __forceinline__ bool tsdf_gradient(const TsdfExtractArgs& a, const float* __restrict__ tsdf,
                                              const float* __restrict__ weight, int c, int i, int j, int k,
                                              float (&g)[3]) {
    if (i < 1 || i + 1 >= a.nx || j < 1 || j + 1 >= a.ny || k < 1 || k + 1 >= a.nz) return false;
    const int stride[3] = {1, a.nx, a.nx * a.ny};
    bool observed = true;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        observed = observed && weight[c + stride[m]] >= a.min_weight && weight[c - stride[m]] >= a.min_weight;
        g[m] = tsdf[c + stride[m]] - tsdf[c - stride[m]];
    }
    return observed;
}

// The surface point on the edge from voxel (i, j, k) along direction d (a bit mask: bit m = one step along axis m) at the
// share r of the edge
__device__ __forceinline__ void tsdf_surface_point(const TsdfExtractArgs& a, int i, int j, int k, int d, float r,
                                                   float* rec) {
    const float at[3] = {(float)i + 0.5f + ((d & 1) ? r : 0.f), (float)j + 0.5f + ((d & 2) ? r : 0.f),
                         (float)k + 0.5f + ((d & 4) ? r : 0.f)};
#pragma unroll
    for (int m = 0; m < 3; ++m) rec[m] = fmaf(a.voxel_size, at[m], a.origin[m]);
}

// Its normal: the normalised (1 - r) g(v) + r g(nb), v = (i, j, k) and nb its neighbour along d; NaN where a gradient
// does not exist or the sum is zero or not finite
__device__ __forceinline__ void tsdf_surface_normal(const TsdfExtractArgs& a, const float* __restrict__ tsdf,
                                                    const float* __restrict__ weight, int v, int nb, int i, int j, int k,
                                                    int d, float r, float* rec) {
    float gv[3], gn[3], g[3];
    bool ok = tsdf_gradient(a, tsdf, weight, v, i, j, k, gv);
    ok = tsdf_gradient(a, tsdf, weight, nb, i + (d & 1), j + ((d >> 1) & 1), k + ((d >> 2) & 1), gn) && ok;
    float largest = 0.f;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        g[m] = ok ? fmaf(r, gn[m], (1.f - r) * gv[m]) : 0.f;
        largest = fmaxf(largest, fabsf(g[m]));
    }
    // scaled by its largest component first: the squares of a tiny gradient do not vanish
    ok = ok && largest > 0.f && largest < __builtin_inff() && g[0] == g[0] && g[1] == g[1] && g[2] == g[2];
    const float s0 = g[0] / largest, s1 = g[1] / largest, s2 = g[2] / largest;
    const float length = sqrtf(fmaf(s0, s0, fmaf(s1, s1, s2 * s2)));
    rec[0] = ok ? s0 / length : __builtin_nanf("");
    rec[1] = ok ? s1 / length : __builtin_nanf("");
    rec[2] = ok ? s2 / length : __builtin_nanf("");
}

}  // namespace pds
