// The reprojection of ONE pixel, shared by rectification.hip (pds_reproject_fwd: the dense [B, H, W, 3] output) and
// point_cloud.hip (pds_point_cloud_fwd: the same points, packed).  Both files call this one device function and are built
// with the same flags, so a packed point is bit for bit the point the dense output holds at that pixel.
#pragma once
#include <hip/hip_runtime.h>

namespace pds {

struct ReprojectArgs {
    float matrix[16];               // row-major 4x4
    float min_confidence;
    int first;                      // (launcher-internal) first pixel of the scalar tail
};

struct Point3 {
    float x, y, z;
};

__device__ __forceinline__ Point3 reproject_one(const ReprojectArgs& a, const unsigned char* __restrict__ valid,
                                                const float* __restrict__ confidence, int p, float d, int h, int w) {
    const float* M = a.matrix;
    const int x = p % w, y = (p / w) % h;
    const float fx = (float)x, fy = (float)y;
    const float X = M[0] * fx + M[1] * fy + M[2] * d + M[3];
    const float Y = M[4] * fx + M[5] * fy + M[6] * d + M[7];
    const float Z = M[8] * fx + M[9] * fy + M[10] * d + M[11];
    const float W = M[12] * fx + M[13] * fy + M[14] * d + M[15];
    bool ok = isfinite(d) && d > 0.f && W > 0.f;
    if (valid) ok = ok && valid[p] != 0;
    if (confidence) ok = ok && confidence[p] >= a.min_confidence;   // (a NaN confidence fails too)
    Point3 r;
    if (ok) {
        r.x = X / W;
        r.y = Y / W;
        r.z = Z / W;
    } else {
        r.x = r.y = r.z = __builtin_nanf("");
    }
    return r;
}

}  // namespace pds
