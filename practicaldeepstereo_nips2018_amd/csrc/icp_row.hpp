// The point-to-plane row of one source pixel (steps 1 - 7 of icp.hip's text), shared by icp.hip and icp_color.hip so that
// the geometric half of the colour system is the same device code and gives the same bits.  Include it below
// `#pragma clang fp contract(off)`: every multiply-add here is an explicit fmaf.
#pragma once

#include "common.hpp"

namespace pds {

namespace {

// What step 3 leaves behind for a photometric row: the transformed point and its projection before rounding.  Written only
// where there is a row; a caller that reads none of it pays nothing.
struct IcpProjection {
    float q[3];
    float u, v;
};

// The row of pixel `pixel` of entry `entry` (global); false: none
__device__ __forceinline__ bool icp_row(const IcpArgs& a, const float* __restrict__ T,
                                        const float* __restrict__ disparity, const unsigned char* __restrict__ valid,
                                        const float* __restrict__ confidence, const float* __restrict__ normals,
                                        const float* __restrict__ model_depth, const float* __restrict__ model_normals,
                                        int entry, int pixel, float (&row)[7], IcpProjection& projection) {
    const int p = entry * (a.h * a.w) + pixel;   // (batch * h * w < 2^31)
    // 1.
    const Point3 P = reproject_one(a.r, valid, confidence, p, disparity[p], a.h, a.w);
    if (!(P.x == P.x)) return false;
    // 2.
    float q[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) q[m] = fmaf(T[3 * m], P.x, fmaf(T[3 * m + 1], P.y, fmaf(T[3 * m + 2], P.z, T[9 + m])));
    if (!(q[2] > 0.f && isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]))) return false;
    // 3.
    const float x = q[0] / q[2], y = q[1] / q[2];
    const float u = fmaf(a.camera[0], x, fmaf(a.camera[4], y, a.camera[2]));
    const float v = fmaf(a.camera[1], y, a.camera[3]);
    const float fu = floorf(u + 0.5f), fv = floorf(v + 0.5f);
    if (!(fu >= 0.f && fu < (float)a.wm && fv >= 0.f && fv < (float)a.hm)) return false;   // (a NaN fails)
    const int px = (int)fu, py = (int)fv;
    // 4.
    const size_t at = (size_t)(a.model_batch == 1 ? 0 : entry) * ((size_t)a.hm * a.wm) + (size_t)py * a.wm + px;
    const float Z = model_depth[at];
    const float n[3] = {model_normals[3 * at], model_normals[3 * at + 1], model_normals[3 * at + 2]};
    if (!(Z == Z && n[0] == n[0] && n[1] == n[1] && n[2] == n[2])) return false;
    const float ym = (fv - a.camera[3]) / a.camera[1];
    const float xm = fmaf(-a.camera[4], ym, fu - a.camera[2]) / a.camera[0];
    // 5.
    const float e[3] = {Z * xm - q[0], Z * ym - q[1], Z - q[2]};
    const float ee = fmaf(e[0], e[0], fmaf(e[1], e[1], e[2] * e[2]));
    if (!(ee <= a.max_distance * a.max_distance)) return false;
    // 6.
    if (normals) {
        const float* nf = normals + 3 * (size_t)p;
        const float f0 = nf[0], f1 = nf[1], f2 = nf[2];
        if (!(f0 == f0 && f1 == f1 && f2 == f2)) return false;
        float s[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) s[m] = fmaf(T[3 * m], f0, fmaf(T[3 * m + 1], f1, T[3 * m + 2] * f2));
        if (!(fmaf(s[0], n[0], fmaf(s[1], n[1], s[2] * n[2])) >= a.min_cosine)) return false;
    }
    // 7.
    row[0] = fmaf(q[1], n[2], -(q[2] * n[1]));
    row[1] = fmaf(q[2], n[0], -(q[0] * n[2]));
    row[2] = fmaf(q[0], n[1], -(q[1] * n[0]));
    row[3] = n[0];
    row[4] = n[1];
    row[5] = n[2];
    row[6] = fmaf(n[0], e[0], fmaf(n[1], e[1], n[2] * e[2]));
    projection.q[0] = q[0];
    projection.q[1] = q[1];
    projection.q[2] = q[2];
    projection.u = u;
    projection.v = v;
    return true;
}

}  // namespace

}  // namespace pds
