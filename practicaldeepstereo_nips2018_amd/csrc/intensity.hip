// Intensity pyramid (pds_intensity_pyramid_fwd; not in the reference): the luma of an image and up to three halvings of it
// in one launch, the frame and model images of photometric tracking (tracking.py: track_color).
//
// Everything is fp32, contraction off:
//   level 0      L = fmaf(0.299f, c0, fmaf(0.587f, c1, 0.114f * c2)) of the pixel's three channels, taken as they are (a
//                uint8 channel converts exactly); a NaN channel gives NaN
//   level l + 1  ((a00 + a01) + (a10 + a11)) * 0.25f over the four children (row, column) of level l; NaN propagates
// Sizes floor (h >> l, w >> l), so a pixel of level l covers exactly the level-0 pixels [x 2^l, (x + 1) 2^l) and no
// workgroup needs another's: the pixel centres are those of pyramid.hip (2 x' + 0.5).
//
// One workgroup of 256 threads owns a 32 x 32 block of the image, aligned to 32:
//   staging   thread t takes the four pixels (row t / 8, columns 4 (t % 8) ..).  VEC (w % 4 == 0 and the pointers allow):
//             float32 [b, 3, h, w]: one 16-byte load per channel plane; float32 [b, h, w, 3]: the 48 bytes of the four
//             pixels as three 16-byte loads; uint8 [b, h, w, 3]: their 12 bytes as three 4-byte loads (there is no more
//             to fetch); level 0 leaves as one 16-byte store.  Scalar accesses otherwise.  The luma goes to LDS with one
//             16-byte store, rows kStride0 = 48 floats apart.
//   levels    1: every thread one pixel from two 8-byte LDS reads; 2: wave 0; 3: threads 0 .. 15 -- the strides and the
//             bank argument are those of pyramid.hip.
// No atomics, no workspace, no workgroup reads what another wrote: the same bits on every run and stream.
#include "common.hpp"

#pragma clang fp contract(off)

namespace pds {

namespace {

constexpr int kIntensityBlock = 32;
constexpr int kIntensityThreads = 256;
constexpr int kStride0 = 48, kStride1 = 24, kStride2 = 8;
static_assert(kIntensityBlock * kIntensityBlock == 4 * kIntensityThreads, "four pixels per thread");

struct IntensityArgs {
    float* out[kIntensityLevels];   // level k: [batch, h >> k, w >> k]
    int levels, h, w, tiles_x, tiles_y;
};

__device__ __forceinline__ float luma(float c0, float c1, float c2) { return fmaf(0.299f, c0, fmaf(0.587f, c1, 0.114f * c2)); }

// pixel (y, x) of the level above the one whose rows are `stride` apart in `from`
__device__ __forceinline__ float quarter_at(const float* from, int stride, int y, int x) {
    const float2 top = *reinterpret_cast<const float2*>(from + (2 * y) * stride + 2 * x);
    const float2 bottom = *reinterpret_cast<const float2*>(from + (2 * y + 1) * stride + 2 * x);
    return ((top.x + top.y) + (bottom.x + bottom.y)) * 0.25f;
}

// LAYOUT 0: float32 [b, 3, h, w]; 1: uint8 [b, h, w, 3]; 2: float32 [b, h, w, 3]
template <int LAYOUT, bool VEC>
__global__ __launch_bounds__(kIntensityThreads) void intensity_pyramid_kernel(IntensityArgs a,
                                                                              const void* __restrict__ image) {
    __shared__ __attribute__((aligned(16))) float level0[kIntensityBlock * kStride0];
    __shared__ __attribute__((aligned(16))) float level1[(kIntensityBlock / 2) * kStride1];
    __shared__ __attribute__((aligned(16))) float level2[(kIntensityBlock / 4) * kStride2];
    const int per_image = a.tiles_x * a.tiles_y;
    const int b = (int)blockIdx.x / per_image, t = (int)blockIdx.x - b * per_image;
    const int ty = t / a.tiles_x;
    const int y0 = ty * kIntensityBlock, x0 = (t - ty * a.tiles_x) * kIntensityBlock;
    const int tid = (int)threadIdx.x;
    const float nan = __builtin_nanf("");

    {
        const int row = tid >> 3, col = (tid & 7) * 4;
        const int y = y0 + row, x = x0 + col;
        float l[4] = {nan, nan, nan, nan};
        if (y < a.h && x < a.w) {
            const size_t plane = (size_t)a.h * a.w;
            const size_t p = ((size_t)b * a.h + y) * a.w + x;   // the pixel among batch * h * w
            float c[4][3];
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j][0] = c[j][1] = c[j][2] = nan;
            if constexpr (VEC) {   // (w % 4 == 0 and x % 4 == 0: the four pixels are inside the row together)
                if constexpr (LAYOUT == 0) {
                    const float* from = static_cast<const float*>(image) + (size_t)b * 3 * plane + ((size_t)y * a.w + x);
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const float4 q = *reinterpret_cast<const float4*>(from + k * plane);
                        c[0][k] = q.x, c[1][k] = q.y, c[2][k] = q.z, c[3][k] = q.w;
                    }
                } else if constexpr (LAYOUT == 1) {
                    const unsigned* from = reinterpret_cast<const unsigned*>(static_cast<const unsigned char*>(image) + 3 * p);
                    const unsigned w0 = from[0], w1 = from[1], w2 = from[2];
                    const unsigned char bytes[12] = {
                        (unsigned char)w0, (unsigned char)(w0 >> 8), (unsigned char)(w0 >> 16), (unsigned char)(w0 >> 24),
                        (unsigned char)w1, (unsigned char)(w1 >> 8), (unsigned char)(w1 >> 16), (unsigned char)(w1 >> 24),
                        (unsigned char)w2, (unsigned char)(w2 >> 8), (unsigned char)(w2 >> 16), (unsigned char)(w2 >> 24)};
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int k = 0; k < 3; ++k) c[j][k] = (float)bytes[3 * j + k];
                } else {
                    const float4* from = reinterpret_cast<const float4*>(static_cast<const float*>(image) + 3 * p);
                    const float4 q0 = from[0], q1 = from[1], q2 = from[2];
                    const float values[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int k = 0; k < 3; ++k) c[j][k] = values[3 * j + k];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (x + j < a.w) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            if constexpr (LAYOUT == 0)
                                c[j][k] = static_cast<const float*>(image)[((size_t)b * 3 + k) * plane + ((size_t)y * a.w + x + j)];
                            else if constexpr (LAYOUT == 1)
                                c[j][k] = (float)static_cast<const unsigned char*>(image)[3 * (p + j) + k];
                            else
                                c[j][k] = static_cast<const float*>(image)[3 * (p + j) + k];
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) l[j] = luma(c[j][0], c[j][1], c[j][2]);
            if constexpr (VEC) {
                *reinterpret_cast<float4*>(a.out[0] + p) = make_float4(l[0], l[1], l[2], l[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x + j < a.w) a.out[0][p + j] = l[j];
            }
        }
        if (a.levels < 2) return;   // (uniform over the workgroup)
        *reinterpret_cast<float4*>(level0 + row * kStride0 + col) = make_float4(l[0], l[1], l[2], l[3]);
    }
    __syncthreads();

    // level 1: 16 x 16, every thread one pixel
    {
        const int ly = tid >> 4, lx = tid & 15;
        const float value = quarter_at(level0, kStride0, ly, lx);
        level1[ly * kStride1 + lx] = value;
        const int h1 = a.h >> 1, w1 = a.w >> 1, y = (y0 >> 1) + ly, x = (x0 >> 1) + lx;
        if (y < h1 && x < w1) a.out[1][((size_t)b * h1 + y) * w1 + x] = value;
    }
    if (a.levels < 3) return;
    __syncthreads();

    // level 2: 8 x 8, wave 0
    if (tid < 64) {
        const int ly = tid >> 3, lx = tid & 7;
        const float value = quarter_at(level1, kStride1, ly, lx);
        level2[ly * kStride2 + lx] = value;
        const int h2 = a.h >> 2, w2 = a.w >> 2, y = (y0 >> 2) + ly, x = (x0 >> 2) + lx;
        if (y < h2 && x < w2) a.out[2][((size_t)b * h2 + y) * w2 + x] = value;
    }
    if (a.levels < 4) return;
    __syncthreads();

    // level 3: 4 x 4
    if (tid < 16) {
        const int ly = tid >> 2, lx = tid & 3;
        const float value = quarter_at(level2, kStride2, ly, lx);
        const int h3 = a.h >> 3, w3 = a.w >> 3, y = (y0 >> 3) + ly, x = (x0 >> 3) + lx;
        if (y < h3 && x < w3) a.out[3][((size_t)b * h3 + y) * w3 + x] = value;
    }
}

template <int LAYOUT>
void launch_layout(bool vec, int groups, hipStream_t s, const IntensityArgs& a, const void* image) {
    if (vec)
        hipLaunchKernelGGL((intensity_pyramid_kernel<LAYOUT, true>), dim3(groups), dim3(kIntensityThreads), 0, s, a, image);
    else
        hipLaunchKernelGGL((intensity_pyramid_kernel<LAYOUT, false>), dim3(groups), dim3(kIntensityThreads), 0, s, a, image);
}

}  // namespace

int intensity_groups(int batch, int h, int w) {
    const long long groups = (long long)batch * ((h + kIntensityBlock - 1) / kIntensityBlock) *
                             ((w + kIntensityBlock - 1) / kIntensityBlock);
    return groups > (1LL << 24) ? 0 : (int)groups;   // (256 threads each: a launch holds at most 2^32 threads)
}

// batch * h * w fits int (checked by the entry point), so the number of blocks does
int launch_intensity_pyramid(const void* image, int layout, float* const* out, int levels, int batch, int h, int w,
                             hipStream_t s) {
    IntensityArgs a = {};
    for (int k = 0; k < levels; ++k) a.out[k] = out[k];
    a.levels = levels;
    a.h = h;
    a.w = w;
    a.tiles_x = (w + kIntensityBlock - 1) / kIntensityBlock;
    a.tiles_y = (h + kIntensityBlock - 1) / kIntensityBlock;
    const int groups = intensity_groups(batch, h, w);
    // uint8: the 12 bytes of four pixels begin at 3 p, p % 4 == 0, a multiple of 4 from a 4-byte aligned base; the
    // float layouts begin at a multiple of 16 bytes from a 16-byte aligned base
    const bool vec = w % 4 == 0 && aligned16(out[0]) && (layout == 1 ? ((uintptr_t)image & 3u) == 0 : aligned16(image));
    const int probe = probe_before("intensity_pyramid", s);
    if (layout == 0)
        launch_layout<0>(vec, groups, s, a, image);
    else if (layout == 1)
        launch_layout<1>(vec, groups, s, a, image);
    else
        launch_layout<2>(vec, groups, s, a, image);
    probe_after(probe, groups, s);
    return check_launch("intensity_pyramid");
}

}  // namespace pds
