// What the two surface extractions of a TSDF volume share (tsdf.hip: the zero crossings along the axes; tsdf_mesh.hip:
// the crossings along all seven edge directions, with faces): the arguments, the walk over the voxels, the edges of a
// quad that carry a crossing, the gradient, and the point and the normal of one crossing.  One device function each, so
// that an axis edge gives the same bits in both.  (tsdf_integrate_kernel and quad_cells of the mesh keep their own
// written-out walks on purpose; each says why.)  And what the plain and the coloured integration share: the sample of a
// voxel and the running average (tsdf.hip, tsdf_color.hip).
#pragma once
#include "compaction.hpp"

#pragma clang fp contract(off)

namespace pds {

struct TsdfExtractArgs {
    float origin[3];
    float voxel_size, min_weight;
    int nx, ny, nz, total;
};

// ---------------------------------------------------------------------------------------------- integrate
// What the two integrations share (tsdf.hip: tsdf_integrate; tsdf_color.hip: tsdf_color_integrate), so that both make the
// same decisions and give tsdf and weight the same bits.
// What voxel (i, j, k) receives from this frame: false = the voxel is skipped; t the truncated distance, wt its weight,
// pixel = py * w + px the source pixel the Z was read from
template <bool CONF>
__device__ __forceinline__ bool tsdf_sample(const TsdfIntegrateArgs& a, const float* __restrict__ zbuf,
                                            const float* __restrict__ wbuf, int i, int j, int k, int h, int w, float& t,
                                            float& wt, int& pixel) {
    const float fi = (float)i, fj = (float)j, fk = (float)k;
    const float zc = fmaf(a.A[6], fi, fmaf(a.A[7], fj, fmaf(a.A[8], fk, a.b[2])));
    if (!(zc > 0.f)) return false;
    const float xc = fmaf(a.A[0], fi, fmaf(a.A[1], fj, fmaf(a.A[2], fk, a.b[0])));
    const float yc = fmaf(a.A[3], fi, fmaf(a.A[4], fj, fmaf(a.A[5], fk, a.b[1])));
    const float x = xc / zc, y = yc / zc;
    const float u = fmaf(a.camera[0], x, fmaf(a.camera[4], y, a.camera[2]));
    const float v = fmaf(a.camera[1], y, a.camera[3]);
    if (!(isfinite(u) && isfinite(v))) return false;
    // floats below 2^31 convert exactly
    const float fu = floorf(u + 0.5f), fv = floorf(v + 0.5f);
    if (!(fu >= 0.f && fu < 2147483648.f && fv >= 0.f && fv < 2147483648.f)) return false;
    const int px = (int)fu, py = (int)fv;
    if (px >= w || py >= h) return false;
    pixel = py * w + px;
    const float Z = zbuf[pixel];
    if (!(Z == Z)) return false;
    const float sdf = Z - zc;
    if (sdf < -a.truncation) return false;
    t = fminf(1.f, sdf / a.truncation);
    wt = 1.f;
    if constexpr (CONF) {
        wt = wbuf[pixel];
        if (!(wt > 0.f)) return false;   // (a NaN confidence fails too)
    }
    return true;
}

__device__ __forceinline__ void tsdf_update(float max_weight, float t, float wt, float& value, float& weight) {
    const float sum = weight + wt;
    value = fmaf(value, weight, t * wt) / sum;
    weight = fminf(sum, max_weight);
}

// ---------------------------------------------------------------------------------------------- extract
// Voxel (i, j, k) of a volume [nz, ny, nx], x fastest, and the walk along the flat index
struct VoxelAt {
    int i, j, k;
    __device__ __forceinline__ static VoxelAt from_flat(int v, int nx, int ny) {
        const int rest = v / nx;
        return {v % nx, rest % ny, rest / ny};
    }
    __device__ __forceinline__ void next(int nx, int ny) {
        if (++i == nx) {
            i = 0;
            if (++j == ny) {
                j = 0;
                ++k;
            }
        }
    }
};

// Which edges of the quad [v0, v0 + n) carry a crossing (both ends observed, signs differ: decided on the stored bits).
// Per voxel of the quad a byte of the result: bit d - 1 = the edge from the voxel along direction d does (d a bit mask:
// bit m = one step along axis m).  DIRS: bit d - 1 = direction d is looked at; the others cost nothing.
// -> value: the voxels' own tsdf (1.f beyond n), at: the first voxel.
// The form is kept on purpose (docs/LAB_NOTES.md, the notes on the compaction scaffold): one branch loads both tensors,
// and the outputs stay locals until the end.  With two load_quad calls tsdf_mesh_count measured 3 % slower, the outputs
// local or not; this form gives it the instruction stream it had before quad_edges.
template <bool VEC, unsigned DIRS>
__device__ __forceinline__ unsigned quad_edges(const TsdfExtractArgs& a, const float* __restrict__ tsdf,
                                               const float* __restrict__ weight, int v0, int n, float (&value)[4],
                                               VoxelAt& at) {
    float own[4], held[4];
    if (VEC && n == 4) {
        const float4 t4 = *reinterpret_cast<const float4*>(tsdf + v0);
        const float4 w4 = *reinterpret_cast<const float4*>(weight + v0);
        own[0] = t4.x; own[1] = t4.y; own[2] = t4.z; own[3] = t4.w;
        held[0] = w4.x; held[1] = w4.y; held[2] = w4.z; held[3] = w4.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            own[e] = e < n ? tsdf[v0 + e] : 1.f;
            held[e] = e < n ? weight[v0 + e] : 0.f;
        }
    }
    const VoxelAt first = VoxelAt::from_flat(v0, a.nx, a.ny);
    VoxelAt c = first;
    const int sy = a.nx, sz = a.nx * a.ny;
    unsigned packed = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (e < n) {
            if (held[e] >= a.min_weight) {
                const bool negative = own[e] < 0.f;
                const bool in_x = c.i + 1 < a.nx, in_y = c.j + 1 < a.ny, in_z = c.k + 1 < a.nz;
#pragma unroll
                for (int d = 1; d < 8; ++d) {
                    // (d is a constant once unrolled: a direction outside DIRS leaves no code)
                    if ((DIRS >> (d - 1) & 1) && (!(d & 1) || in_x) && (!(d & 2) || in_y) && (!(d & 4) || in_z)) {
                        const int nb = v0 + e + (d & 1) + ((d & 2) ? sy : 0) + ((d & 4) ? sz : 0);
                        if (weight[nb] >= a.min_weight && (tsdf[nb] < 0.f) != negative) packed |= 1u << (8 * e + d - 1);
                    }
                }
            }
            c.next(a.nx, a.ny);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) value[e] = own[e];
    at = first;
    return packed;
}

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
