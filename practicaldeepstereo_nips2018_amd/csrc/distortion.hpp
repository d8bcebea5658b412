// The Brown-Conrady distortion polynomial of ONE normalised point, shared by rectification.hip (pds_rectify_maps_fwd: fp64,
// as OpenCV's initUndistortRectifyMap) and register_depth.hip (pds_register_depth_fwd: fp32, the forward projection into
// a distorted target camera).  T is the float type; the order of the operations is the one rectify_maps_kernel has
// always had, so its fp64 maps keep every bit.
#pragma once
#include <hip/hip_runtime.h>

namespace pds {

// (x, y) -> (xd, yd); k = k1, k2, p1, p2, k3
template <typename T>
__device__ __forceinline__ void distort_point(const T* __restrict__ k, T x, T y, T& xd, T& yd) {
    const T k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4];
    const T r2 = x * x + y * y;
    const T kr = T(1) + ((k3 * r2 + k2) * r2 + k1) * r2;
    xd = x * kr + T(2) * p1 * x * y + p2 * (r2 + T(2) * x * x);
    yd = y * kr + p1 * (r2 + T(2) * y * y) + T(2) * p2 * x * y;
}

}  // namespace pds
