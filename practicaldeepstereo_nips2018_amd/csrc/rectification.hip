// Rectification maps, remap and 3-D reprojection (pds_rectify_maps_fwd, pds_remap_fwd, pds_reproject_fwd; not in the
// reference).
//
// rectify_maps: one thread per output pixel, fp64 throughout as OpenCV's initUndistortRectifyMap, rounded once to fp32.
// It runs once per rig, so nothing about it is tuned.
//
// remap: the per-frame path.  One thread takes four consecutive output pixels of a row: their map entries are one float4
// of map_x and one of map_y, the tap addresses and bilinear weights are computed once and reused for every image of the
// batch, and each of the three output planes gets one float4 store per image.  Taps are plain byte (uint8 NHWC) or dword
// (float32 NCHW) loads: the footprint of four pixels is a 2 x 5 patch that no two threads share enough of to pay for LDS.
// It runs at 13-25 % of the HBM floor; a form with one thread per plane (3 * batch times the threads) was no faster
// (DESIGN.md section 3.7).
// VEC = false is the scalar form for rows whose width is not a multiple of 4 (or pointers that are not 16-byte aligned).
//
// reproject: four flat pixels per thread, (X, Y, Z, W) = M (x, y, d, 1) in fp32; three float4 stores of interleaved xyz
// (48 B, 16-byte aligned because 4 pixels * 12 B = 48 B) and one float4 of depth.  The last numel % 4 pixels go scalar.
//
// Every index fits in 32 bits (checked by the entry points in api.hip).
#include "common.hpp"
#include "distortion.hpp"

namespace pds {

namespace {

constexpr int kRectThreads = 256;
constexpr int kRectMaxBlocks = 2048;   // grid-stride beyond (cdna_hip_programming.md Guideline 11)

int rect_grid(long long items) {
    const long long blocks = (items + kRectThreads - 1) / kRectThreads;
    return (int)(blocks < kRectMaxBlocks ? (blocks > 0 ? blocks : 1) : kRectMaxBlocks);
}

// ---------------------------------------------------------------------------------------------- rectification maps
__global__ __launch_bounds__(kRectThreads) void rectify_maps_kernel(RectifyMapsArgs a, float* __restrict__ map_x,
                                                                    float* __restrict__ map_y, int h, int w) {
    const int total = h * w;
    for (int i = blockIdx.x * kRectThreads + threadIdx.x; i < total; i += gridDim.x * kRectThreads) {
        const double u = (double)(i % w), v = (double)(i / w);
        const double* P = a.inverse_projection;
        double x = P[0] * u + P[1] * v + P[2];
        double y = P[3] * u + P[4] * v + P[5];
        const double z = P[6] * u + P[7] * v + P[8];
        x /= z;
        y /= z;
        double xd, yd;
        distort_point<double>(a.distortion, x, y, xd, yd);   // (distortion.hpp, shared with register_depth.hip)
        map_x[i] = (float)(a.camera[0] * xd + a.camera[4] * yd + a.camera[2]);
        map_y[i] = (float)(a.camera[1] * yd + a.camera[3]);
    }
}

// ---------------------------------------------------------------------------------------------- remap
// The taps of one output pixel: offsets of (x0, y0) / (x0 + 1, y0) / (x0, y0 + 1) / (x0 + 1, y0 + 1) within one image
// plane (-1: outside, reads the border value) and the bilinear weights.
struct Taps {
    int o00, o01, o10, o11;
    float ax, ay;
};

template <int LAYOUT>
__device__ __forceinline__ Taps make_taps(float mx, float my, int h_in, int w_in) {
    Taps t;
    if (!(isfinite(mx) && isfinite(my))) {
        t.o00 = t.o01 = t.o10 = t.o11 = -1;
        t.ax = t.ay = 0.f;
        return t;
    }
    // past one pixel outside, every tap is outside: clamping there keeps floorf's result in int range and changes no tap
    mx = fminf(fmaxf(mx, -2.f), (float)w_in + 1.f);
    my = fminf(fmaxf(my, -2.f), (float)h_in + 1.f);
    const float fx = floorf(mx), fy = floorf(my);
    const int x0 = (int)fx, y0 = (int)fy;
    t.ax = mx - fx;
    t.ay = my - fy;
    const bool cx0 = x0 >= 0 && x0 < w_in, cx1 = x0 + 1 >= 0 && x0 + 1 < w_in;
    const bool cy0 = y0 >= 0 && y0 < h_in, cy1 = y0 + 1 >= 0 && y0 + 1 < h_in;
    const int step = LAYOUT == 1 ? 3 : 1;   // uint8 NHWC: 3 bytes per pixel
    const int r0 = y0 * w_in, r1 = r0 + w_in;
    t.o00 = cy0 && cx0 ? (r0 + x0) * step : -1;
    t.o01 = cy0 && cx1 ? (r0 + x0 + 1) * step : -1;
    t.o10 = cy1 && cx0 ? (r1 + x0) * step : -1;
    t.o11 = cy1 && cx1 ? (r1 + x0 + 1) * step : -1;
    return t;
}

template <int LAYOUT>
__device__ __forceinline__ float tap(const void* __restrict__ plane, int offset, float border) {
    if (offset < 0) return border;
    if constexpr (LAYOUT == 1)
        return (float)static_cast<const unsigned char*>(plane)[offset];
    else
        return static_cast<const float*>(plane)[offset];
}

// plane: image b's channel c (float NCHW) or image b's first byte + c (uint8 NHWC)
template <int LAYOUT>
__device__ __forceinline__ float sample(const void* __restrict__ plane, const Taps& t, float border) {
    const float p00 = tap<LAYOUT>(plane, t.o00, border), p01 = tap<LAYOUT>(plane, t.o01, border);
    const float p10 = tap<LAYOUT>(plane, t.o10, border), p11 = tap<LAYOUT>(plane, t.o11, border);
    return (1.f - t.ay) * ((1.f - t.ax) * p00 + t.ax * p01) + t.ay * ((1.f - t.ax) * p10 + t.ax * p11);
}

template <int LAYOUT>
__device__ __forceinline__ const void* plane_of(const void* image, int b, int c, int in_plane) {
    if constexpr (LAYOUT == 1)
        return static_cast<const unsigned char*>(image) + b * 3 * in_plane + c;   // in_plane: pixels per image
    else
        return static_cast<const float*>(image) + (b * 3 + c) * in_plane;
}

template <int LAYOUT, bool VEC>
__global__ __launch_bounds__(kRectThreads) void remap_kernel(const void* __restrict__ image,
                                                             const float* __restrict__ map_x,
                                                             const float* __restrict__ map_y, float* __restrict__ out,
                                                             int batch, int h_in, int w_in, int h_out, int w_out,
                                                             float border, int reverse_channels) {
    const int quads = (w_out + 3) >> 2;
    const int total = h_out * quads;
    const int in_plane = h_in * w_in, out_plane = h_out * w_out;
    for (int i = blockIdx.x * kRectThreads + threadIdx.x; i < total; i += gridDim.x * kRectThreads) {
        const int y = i / quads, x = (i - y * quads) << 2;
        const int base = y * w_out + x;
        const int n = VEC ? 4 : min(4, w_out - x);
        float mx[4], my[4];
        if constexpr (VEC) {
            const float4 vx = *reinterpret_cast<const float4*>(map_x + base);
            const float4 vy = *reinterpret_cast<const float4*>(map_y + base);
            mx[0] = vx.x; mx[1] = vx.y; mx[2] = vx.z; mx[3] = vx.w;
            my[0] = vy.x; my[1] = vy.y; my[2] = vy.z; my[3] = vy.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                mx[k] = k < n ? map_x[base + k] : 0.f;
                my[k] = k < n ? map_y[base + k] : 0.f;
            }
        }
        Taps t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = make_taps<LAYOUT>(mx[k], my[k], h_in, w_in);
        for (int b = 0; b < batch; ++b) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const void* plane = plane_of<LAYOUT>(image, b, reverse_channels ? 2 - c : c, in_plane);
                float* dst = out + (b * 3 + c) * out_plane + base;
                if constexpr (VEC) {
                    float4 v;
                    v.x = sample<LAYOUT>(plane, t[0], border);
                    v.y = sample<LAYOUT>(plane, t[1], border);
                    v.z = sample<LAYOUT>(plane, t[2], border);
                    v.w = sample<LAYOUT>(plane, t[3], border);
                    *reinterpret_cast<float4*>(dst) = v;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < n) dst[k] = sample<LAYOUT>(plane, t[k], border);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- reprojection
// (reproject_one, Point3: reproject.hpp, shared with point_cloud.hip)
template <bool VEC>
__global__ __launch_bounds__(kRectThreads) void reproject_kernel(ReprojectArgs a, const float* __restrict__ disparity,
                                                                 const unsigned char* __restrict__ valid,
                                                                 const float* __restrict__ confidence,
                                                                 float* __restrict__ points, float* __restrict__ depth,
                                                                 int total, int h, int w) {
    // VEC: groups of four pixels from 0; scalar: pixels from a.first (the tail the vector launch left)
    const int end = VEC ? total >> 2 : total;
    for (int i = (VEC ? 0 : a.first) + blockIdx.x * kRectThreads + threadIdx.x; i < end; i += gridDim.x * kRectThreads) {
        if constexpr (VEC) {
            const int p = i << 2;
            const float4 d4 = *reinterpret_cast<const float4*>(disparity + p);
            const Point3 q0 = reproject_one(a, valid, confidence, p, d4.x, h, w);
            const Point3 q1 = reproject_one(a, valid, confidence, p + 1, d4.y, h, w);
            const Point3 q2 = reproject_one(a, valid, confidence, p + 2, d4.z, h, w);
            const Point3 q3 = reproject_one(a, valid, confidence, p + 3, d4.w, h, w);
            if (points) {
                float4* dst = reinterpret_cast<float4*>(points + 3 * p);
                dst[0] = make_float4(q0.x, q0.y, q0.z, q1.x);
                dst[1] = make_float4(q1.y, q1.z, q2.x, q2.y);
                dst[2] = make_float4(q2.z, q3.x, q3.y, q3.z);
            }
            if (depth) *reinterpret_cast<float4*>(depth + p) = make_float4(q0.z, q1.z, q2.z, q3.z);
        } else {
            const Point3 q = reproject_one(a, valid, confidence, i, disparity[i], h, w);
            if (points) {
                points[3 * i] = q.x;
                points[3 * i + 1] = q.y;
                points[3 * i + 2] = q.z;
            }
            if (depth) depth[i] = q.z;
        }
    }
}

}  // namespace

int launch_rectify_maps(const RectifyMapsArgs& a, float* map_x, float* map_y, int h, int w, hipStream_t s) {
    hipLaunchKernelGGL(rectify_maps_kernel, dim3(rect_grid((long long)h * w)), dim3(kRectThreads), 0, s, a, map_x,
                       map_y, h, w);
    return check_launch("rectify_maps");
}

int launch_remap(const void* image, int layout, const float* map_x, const float* map_y, float* out, int batch, int h_in,
                 int w_in, int h_out, int w_out, float border, int reverse_channels, hipStream_t s) {
    const bool vec = w_out % 4 == 0 && aligned16(map_x) && aligned16(map_y) && aligned16(out);
    const int grid = rect_grid((long long)h_out * ((w_out + 3) / 4));
#define PDS_REMAP(L, V)                                                                                                 \
    hipLaunchKernelGGL((remap_kernel<L, V>), dim3(grid), dim3(kRectThreads), 0, s, image, map_x, map_y, out, batch,   \
                       h_in, w_in, h_out, w_out, border, reverse_channels)
    if (layout == 1) {
        if (vec) PDS_REMAP(1, true);
        else PDS_REMAP(1, false);
    } else {
        if (vec) PDS_REMAP(0, true);
        else PDS_REMAP(0, false);
    }
#undef PDS_REMAP
    return check_launch("remap");
}

int launch_reproject(const ReprojectArgs& a, const float* disparity, const unsigned char* valid, const float* confidence,
                     float* points, float* depth, int total, int h, int w, hipStream_t s) {
    const bool vec = aligned16(disparity) && (!points || aligned16(points)) && (!depth || aligned16(depth));
    const int main = vec ? total & ~3 : 0;
    if (main > 0)
        hipLaunchKernelGGL(reproject_kernel<true>, dim3(rect_grid(main / 4)), dim3(kRectThreads), 0, s, a, disparity,
                           valid, confidence, points, depth, main, h, w);
    if (main < total) {
        // the tail (or everything, unaligned): the scalar form on the pixels from `main` on
        const int rest = total - main;
        ReprojectArgs tail = a;
        tail.first = main;
        hipLaunchKernelGGL(reproject_kernel<false>, dim3(rect_grid(rest)), dim3(kRectThreads), 0, s, tail, disparity,
                           valid, confidence, points, depth, total, h, w);
    }
    return check_launch("reproject");
}

}  // namespace pds
