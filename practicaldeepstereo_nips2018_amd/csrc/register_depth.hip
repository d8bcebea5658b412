// Depth registration (pds_register_depth_fwd; not in the reference): a z-buffered forward warp.  Every kept pixel of
// `reproject` is carried into another camera -- the raw left frame, the right view, a colour camera -- and the nearest
// point that lands on a target pixel wins (OpenCV rgbd::registerDepth, ROS depth_image_proc/register, RealSense align).
//
// Per source pixel p (raster index within its batch entry b), in fp32:
//   1. (X, Y, Z) = reproject_one(M', ...) -- reproject.hpp, the device function behind pds_reproject_fwd and
//      pds_point_cloud_fwd, so the kept pixels and their Z are the ones `reproject` gives for M' (d finite and > 0, W > 0,
//      valid, confidence).  M' = [[R, t], [0, 0, 0, 1]] * matrix is composed by the host in fp64 and rounded once.
//      Dropped unless Z is finite and Z > 0.
//   2. x = X / Z, y = Y / Z, r2 = x^2 + y^2.  Dropped when 1 + 3 k1 r2 + 5 k2 r2^2 + 7 k3 r2^3 <= 0 (evaluated as
//      1 + ((7 k3 r2 + 5 k2) r2 + 3 k1) r2): that is d(r kr)/dr, and where it is not positive the radial model has folded
//      back -- a point far outside the field of view would land inside the image.  OpenCV's projectPoints has no such guard.
//   3. (xd, yd) = distort_point (distortion.hpp, the polynomial of pds_rectify_maps_fwd, here in fp32);
//      u = fx xd + skew yd + cx, v = fy yd + cy.  Dropped if u or v is not finite.
//   4. footprint: splat 1: the pixel (floorf(u + 0.5f), floorf(v + 0.5f)); splat 2: {floorf(u), floorf(u) + 1} x
//      {floorf(v), floorf(v) + 1}.  Footprint pixels outside [0, wt) x [0, ht) are skipped one by one.
//   5. every footprint pixel receives key = (uint64(float_as_uint(Z)) << 32) | uint32(p) by a 64-bit unsigned atomic
//      minimum at device scope (the targets of one image are hit from every XCD).  Z > 0 and finite: its bits order as
//      its value.  So the nearest point wins, among equal depths the smaller source index, and -- the minimum of integers
//      not depending on arrival order -- the result has the same bits on every run.  No floating-point atomic.
//
// On the caller's stream, in stream order, and NO workgroup waits on another:
//   clear    hipMemsetAsync of the key buffer uint64 [batch, ht, wt] with 0xFF ("empty" = all ones, which no key can be:
//            its upper half would be a NaN)
//   scatter  one workgroup of 256 threads per tile of kRegisterDepthTile = 1024 flat source pixels (batch * h * w taken
//            as one row).  Each thread loads one float4 of disparity (VEC) into LDS; then thread t takes the pixels
//            t, t + 256, t + 512, t + 768 of the tile, so that the 64 lanes of a wave hold 64 CONSECUTIVE source pixels
//            and one atomic wave-instruction falls on neighbouring keys of (mostly) one target row.
//   resolve  one workgroup of 256 threads per 1024 target pixels, four per thread: two 16-byte loads of keys, one
//            16-byte store of depth and of index and one 4-byte store of valid (VEC), plain vector stores.
// VEC = false is the scalar form for pointers that are not 16-byte aligned; the last total % 4 pixels go scalar in
// either form.
#include "common.hpp"
#include "distortion.hpp"

namespace pds {

namespace {

constexpr int kRdThreads = 256;
static_assert(kRegisterDepthTile == 4 * kRdThreads, "four pixels per thread");
constexpr unsigned long long kRdEmpty = ~0ull;

__device__ __forceinline__ void put_key(unsigned long long* __restrict__ plane, int yi, int xi, int ht, int wt,
                                        unsigned long long key) {
    if (yi >= 0 && yi < ht && xi >= 0 && xi < wt) atomicMin(plane + ((size_t)yi * wt + xi), key);
}

template <int SPLAT>
__device__ __forceinline__ void scatter_one(const RegisterDepthArgs& a, const unsigned char* __restrict__ valid,
                                            const float* __restrict__ confidence, unsigned long long* __restrict__ keys,
                                            int p, float d, int h, int w, int ht, int wt) {
    const Point3 q = reproject_one(a.r, valid, confidence, p, d, h, w);
    const float Z = q.z;
    if (!(Z > 0.f && Z < __builtin_inff())) return;   // (the NaN of a rejected pixel fails too)
    const float x = q.x / Z, y = q.y / Z;
    const float r2 = x * x + y * y;
    const float k1 = a.distortion[0], k2 = a.distortion[1], k3 = a.distortion[4];
    if (!(1.f + ((7.f * k3 * r2 + 5.f * k2) * r2 + 3.f * k1) * r2 > 0.f)) return;   // folded back (or NaN)
    float xd, yd;
    distort_point<float>(a.distortion, x, y, xd, yd);
    const float u = a.camera[0] * xd + a.camera[4] * yd + a.camera[2];
    const float v = a.camera[1] * yd + a.camera[3];
    if (!(isfinite(u) && isfinite(v))) return;
    const int hw = h * w;
    const int b = p / hw;
    const unsigned long long key = ((unsigned long long)__float_as_uint(Z) << 32) | (unsigned)(p - b * hw);
    unsigned long long* plane = keys + (size_t)b * ht * wt;
    // floats below 2^31 convert exactly (the largest is 2^31 - 128, so that + 1 still fits)
    if constexpr (SPLAT == 1) {
        const float fu = floorf(u + 0.5f), fv = floorf(v + 0.5f);
        if (!(fu >= 0.f && fu < 2147483648.f && fv >= 0.f && fv < 2147483648.f)) return;
        put_key(plane, (int)fv, (int)fu, ht, wt, key);
    } else {
        const float fu = floorf(u), fv = floorf(v);
        if (!(fu >= -1.f && fu < 2147483648.f && fv >= -1.f && fv < 2147483648.f)) return;
        const int x0 = (int)fu, y0 = (int)fv;
        put_key(plane, y0, x0, ht, wt, key);
        put_key(plane, y0, x0 + 1, ht, wt, key);
        put_key(plane, y0 + 1, x0, ht, wt, key);
        put_key(plane, y0 + 1, x0 + 1, ht, wt, key);
    }
}

// ---------------------------------------------------------------------------------------------- scatter
template <bool VEC, int SPLAT>
__global__ __launch_bounds__(kRdThreads) void register_depth_scatter_kernel(
    RegisterDepthArgs a, const float* __restrict__ disparity, const unsigned char* __restrict__ valid,
    const float* __restrict__ confidence, unsigned long long* __restrict__ keys, int total, int h, int w, int ht,
    int wt) {
    __shared__ alignas(16) float s_d[kRegisterDepthTile];
    const int t = threadIdx.x;
    const long long tile0 = (long long)blockIdx.x * kRegisterDepthTile;   // < total
    const long long first = tile0 + 4 * t;
    const int n = first >= total ? 0 : (total - first < 4 ? (int)(total - first) : 4);
    if (VEC && n == 4) {
        *reinterpret_cast<float4*>(s_d + 4 * t) = *reinterpret_cast<const float4*>(disparity + first);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) s_d[4 * t + k] = disparity[first + k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long p = tile0 + k * kRdThreads + t;
        if (p < total) scatter_one<SPLAT>(a, valid, confidence, keys, (int)p, s_d[k * kRdThreads + t], h, w, ht, wt);
    }
}

// ---------------------------------------------------------------------------------------------- resolve
template <bool VEC>
__global__ __launch_bounds__(kRdThreads) void register_depth_resolve_kernel(const unsigned long long* __restrict__ keys,
                                                                            float* __restrict__ depth,
                                                                            int* __restrict__ index,
                                                                            unsigned char* __restrict__ valid_out,
                                                                            float fill_value, int total) {
    const long long first = (long long)blockIdx.x * kRegisterDepthTile + 4 * (int)threadIdx.x;
    if (first >= total) return;
    const int n = total - first < 4 ? (int)(total - first) : 4;
    unsigned long long key[4];
    if (VEC && n == 4) {
        const ulonglong2 lo = *reinterpret_cast<const ulonglong2*>(keys + first);
        const ulonglong2 hi = *reinterpret_cast<const ulonglong2*>(keys + first + 2);
        key[0] = lo.x; key[1] = lo.y; key[2] = hi.x; key[3] = hi.y;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) key[k] = k < n ? keys[first + k] : kRdEmpty;
    }
    float z[4];
    int source[4];
    unsigned char hit[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        hit[k] = key[k] != kRdEmpty;
        z[k] = hit[k] ? __uint_as_float((unsigned)(key[k] >> 32)) : fill_value;
        source[k] = hit[k] ? (int)(unsigned)key[k] : -1;
    }
    if (VEC && n == 4) {
        *reinterpret_cast<float4*>(depth + first) = make_float4(z[0], z[1], z[2], z[3]);
        if (index) *reinterpret_cast<int4*>(index + first) = make_int4(source[0], source[1], source[2], source[3]);
        if (valid_out) *reinterpret_cast<uchar4*>(valid_out + first) = make_uchar4(hit[0], hit[1], hit[2], hit[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < n) {
                depth[first + k] = z[k];
                if (index) index[first + k] = source[k];
                if (valid_out) valid_out[first + k] = hit[k];
            }
        }
    }
}

bool aligned_to(const void* p, unsigned bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

}  // namespace

size_t register_depth_workspace_bytes(long long target_pixels) {
    return ((size_t)target_pixels * sizeof(unsigned long long) + 255) & ~(size_t)255;
}

int launch_register_depth(const RegisterDepthArgs& a, const float* disparity, const unsigned char* valid,
                          const float* confidence, float* depth, int* index, unsigned char* valid_out, int batch, int h,
                          int w, int ht, int wt, void* workspace, hipStream_t s) {
    const int total = batch * h * w, targets = batch * ht * wt;
    unsigned long long* keys = static_cast<unsigned long long*>(workspace);
    if (hipMemsetAsync(keys, 0xFF, (size_t)targets * sizeof(unsigned long long), s) != hipSuccess) {
        (void)hipGetLastError();
        return set_error(-1, "register_depth: clearing the key buffer failed");
    }

    const int scatter_tiles = (int)(((long long)total + kRegisterDepthTile - 1) / kRegisterDepthTile);
    const bool vec_in = aligned_to(disparity, 16);
    int probe = probe_before("register_depth_scatter", s);
#define PDS_RD_SCATTER(V, S)                                                                                           \
    hipLaunchKernelGGL((register_depth_scatter_kernel<V, S>), dim3(scatter_tiles), dim3(kRdThreads), 0, s, a,          \
                       disparity, valid, confidence, keys, total, h, w, ht, wt)
    if (vec_in) {
        if (a.splat == 1) PDS_RD_SCATTER(true, 1);
        else PDS_RD_SCATTER(true, 2);
    } else {
        if (a.splat == 1) PDS_RD_SCATTER(false, 1);
        else PDS_RD_SCATTER(false, 2);
    }
#undef PDS_RD_SCATTER
    probe_after(probe, scatter_tiles, s);
    if (int rc = check_launch("register_depth_scatter")) return rc;

    const int resolve_tiles = (int)(((long long)targets + kRegisterDepthTile - 1) / kRegisterDepthTile);
    const bool vec_out = aligned_to(keys, 16) && aligned_to(depth, 16) && (!index || aligned_to(index, 16)) &&
                         (!valid_out || aligned_to(valid_out, 4));
    probe = probe_before("register_depth_resolve", s);
    if (vec_out)
        hipLaunchKernelGGL(register_depth_resolve_kernel<true>, dim3(resolve_tiles), dim3(kRdThreads), 0, s, keys, depth,
                           index, valid_out, a.fill_value, targets);
    else
        hipLaunchKernelGGL(register_depth_resolve_kernel<false>, dim3(resolve_tiles), dim3(kRdThreads), 0, s, keys,
                           depth, index, valid_out, a.fill_value, targets);
    probe_after(probe, resolve_tiles, s);
    return check_launch("register_depth_resolve");
}

}  // namespace pds
