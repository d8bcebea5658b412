// What the raycast of a TSDF volume and the colour of a raycast share (tsdf_raycast.hip: tsdf_raycast; tsdf_color.hip:
// tsdf_color_render): the ray of a pixel, the cell of a grid position, the eight corners of a cell, whether they are
// observed, and the lerp.  One device function each, so that the colour is read in the cell the normal was taken from.
#pragma once
#include "common.hpp"

#pragma clang fp contract(off)

namespace pds {

// Step 1 of tsdf_raycast.hip: the ray of pixel (px, py) in the camera frame, dir = (x, y, 1), and in grid coordinates,
// g(s) = o + s d.  pose: M (9), o (3) of the entry
__device__ __forceinline__ void raycast_ray(const TsdfRaycastArgs& a, const float* pose, int px, int py, float& x,
                                            float& y, float (&d)[3], float (&o)[3]) {
    y = ((float)py - a.camera[3]) / a.camera[1];
    x = fmaf(-a.camera[4], y, (float)px - a.camera[2]) / a.camera[0];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        d[m] = fmaf(pose[3 * m], x, fmaf(pose[3 * m + 1], y, pose[3 * m + 2]));
        o[m] = pose[9 + m];
    }
}

// The cell of grid position g and the position within it; -> the index of the cell's first corner.  Every n_a >= 2
__device__ __forceinline__ int raycast_cell(const TsdfRaycastArgs& a, const float (&g)[3], float (&f)[3]) {
    // (fmaxf drops a NaN: whatever g is, the eight corners lie inside the volume)
    const float ci = fminf(fmaxf(floorf(g[0]), 0.f), (float)(a.nx - 2));
    const float cj = fminf(fmaxf(floorf(g[1]), 0.f), (float)(a.ny - 2));
    const float ck = fminf(fmaxf(floorf(g[2]), 0.f), (float)(a.nz - 2));
    f[0] = g[0] - ci;
    f[1] = g[1] - cj;
    f[2] = g[2] - ck;
    return ((int)ck * a.ny + (int)cj) * a.nx + (int)ci;   // (3 * nx * ny * nz < 2^31)
}

// corner e: bit 0 = +x, bit 1 = +y, bit 2 = +z
__device__ __forceinline__ void raycast_corners(const float* __restrict__ t, int base, int sy, int sz, float (&v)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = t[base + (e & 1) + (e >> 1 & 1) * sy + (e >> 2) * sz];
}

__device__ __forceinline__ bool raycast_observed(const float (&w)[8], float min_weight) {
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 8; ++e) ok = ok && w[e] >= min_weight;   // (a NaN weight fails)
    return ok;
}

__device__ __forceinline__ float lerp(float t, float a, float b) { return fmaf(t, b - a, a); }

// the trilinear interpolant over the eight corners, in x, then y, then z
__device__ __forceinline__ float raycast_value(const float (&v)[8], const float (&f)[3]) {
    const float c00 = lerp(f[0], v[0], v[1]), c10 = lerp(f[0], v[2], v[3]);
    const float c01 = lerp(f[0], v[4], v[5]), c11 = lerp(f[0], v[6], v[7]);
    return lerp(f[2], lerp(f[1], c00, c10), lerp(f[1], c01, c11));
}

}  // namespace pds
