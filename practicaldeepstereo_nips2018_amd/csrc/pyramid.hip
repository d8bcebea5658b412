// Edge- and hole-aware disparity pyramid (pds_disparity_pyramid_fwd; not in the reference): up to three halvings of a
// disparity map in one launch, the frame side of coarse-to-fine tracking (tracking.py).
//
// A pixel of level l is formed from its four children at level l - 1, taken in the order (0,0), (0,1), (1,0), (1,1)
// (row, column).  Everything is fp32, contraction off:
//   eligible   at level 0: isfinite(d) && d > 0, valid != 0 where given, confidence >= min_confidence where given (a NaN
//              fails): the mask of reproject_one less its matrix test.  Above level 0: the child is not NaN
//   reference  m = the largest eligible child: the foreground wins, a block astride a depth edge does not average across it
//   members    the eligible children with m - c <= max_difference (one subtraction)
//   value      the sum of the members in child order (from 0.f) divided by their count; NaN without a member
// Sizes floor (h >> l, w >> l), so a pixel of level l covers exactly the level-0 pixels [x 2^l, (x + 1) 2^l) and no
// workgroup needs another's.  Values stay in the units of the source.
//
// One workgroup of 256 threads owns a 32 x 32 block of the source, aligned to 32:
//   staging   thread t takes the four pixels (row t / 8, columns 4 (t % 8) ..) -- one 16-byte load per tensor where
//             w % 4 == 0 and the pointers allow (VEC), scalar loads otherwise -- applies the eligibility and stores the
//             value or NaN into LDS with one 16-byte store.  Rows are kStride0 = 48 floats apart.
//   level 1   thread t forms pixel (t / 16, t % 16) from two 8-byte LDS reads (rows 2 y and 2 y + 1 at column 2 x).  The
//             compiler pairs them into one ds_read2_b64, which is serviced per 16 contiguous lanes with banks of
//             (address / 4) % 32: such a group is one output row, 32 consecutive floats, every bank once.  Were the two
//             reads issued apart (ds_read_b64: per half wave, banks % 64), the next output row begins 2 kStride0 = 96 = 32
//             (mod 64) floats further and a half wave still touches every bank once; a stride of 32 would make that 2-way.
//   level 2   threads 0 .. 63 (wave 0), from level 1 in LDS at kStride1 = 24: 16 lanes are two output rows 48 floats
//             apart, [0, 16) and [16, 32) mod 32 (apart: 0, 48, 32, 16 mod 64 for the four rows of a half wave): no
//             conflict either way; level 3: threads 0 .. 15 from level 2 at stride 8 (2-way, one instruction).
// Every level is stored to LDS for the next and, inside the image, to its output.  No atomics, no workspace, no workgroup
// reads what another wrote: the same bits on every run and stream.
#include "common.hpp"

#pragma clang fp contract(off)

namespace pds {

namespace {

constexpr int kPyramidBlock = 32;
constexpr int kPyramidThreads = 256;
constexpr int kStride0 = 48, kStride1 = 24, kStride2 = 8;
static_assert(kPyramidBlock * kPyramidBlock == 4 * kPyramidThreads, "four source pixels per thread");

struct PyramidArgs {
    float* out[kPyramidLevels];   // level k + 1 of the source: [batch, h >> (k + 1), w >> (k + 1)]
    float min_confidence, max_difference;
    int levels, h, w, tiles_x, tiles_y;
};

__device__ __forceinline__ float halve(float c0, float c1, float c2, float c3, float max_difference) {
    const float c[4] = {c0, c1, c2, c3};
    float m = __builtin_nanf("");
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (c[i] == c[i] && !(m >= c[i])) m = c[i];   // (a NaN m gives way to the first eligible child)
    float sum = 0.f;
    int n = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (c[i] == c[i] && m - c[i] <= max_difference) {
            sum += c[i];
            ++n;
        }
    }
    return n ? sum / (float)n : __builtin_nanf("");
}

// pixel (y, x) of the level whose rows are `stride` apart in `from`
__device__ __forceinline__ float halve_at(const float* from, int stride, int y, int x, float max_difference) {
    const float2 top = *reinterpret_cast<const float2*>(from + (2 * y) * stride + 2 * x);
    const float2 bottom = *reinterpret_cast<const float2*>(from + (2 * y + 1) * stride + 2 * x);
    return halve(top.x, top.y, bottom.x, bottom.y, max_difference);
}

// FIRST: the source is level 0 (its eligibility; valid and confidence are read); otherwise a level above it (not NaN)
template <bool FIRST, bool VEC>
__global__ __launch_bounds__(kPyramidThreads) void disparity_pyramid_kernel(PyramidArgs a,
                                                                            const float* __restrict__ disparity,
                                                                            const unsigned char* __restrict__ valid,
                                                                            const float* __restrict__ confidence) {
    __shared__ __attribute__((aligned(16))) float level0[kPyramidBlock * kStride0];
    __shared__ __attribute__((aligned(16))) float level1[(kPyramidBlock / 2) * kStride1];
    __shared__ __attribute__((aligned(16))) float level2[(kPyramidBlock / 4) * kStride2];
    const int per_image = a.tiles_x * a.tiles_y;
    const int b = (int)blockIdx.x / per_image, t = (int)blockIdx.x - b * per_image;
    const int ty = t / a.tiles_x;
    const int y0 = ty * kPyramidBlock, x0 = (t - ty * a.tiles_x) * kPyramidBlock;
    const int tid = (int)threadIdx.x;
    const float nan = __builtin_nanf("");

    {
        const int row = tid >> 3, col = (tid & 7) * 4;
        const int y = y0 + row, x = x0 + col;
        float d[4] = {nan, nan, nan, nan};
        if (y < a.h && x < a.w) {
            const size_t p = ((size_t)b * a.h + y) * a.w + x;
            unsigned char v[4] = {1, 1, 1, 1};
            float c[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (VEC) {   // (w % 4 == 0 and x % 4 == 0: the four pixels are inside the row together)
                const float4 q = *reinterpret_cast<const float4*>(disparity + p);
                d[0] = q.x, d[1] = q.y, d[2] = q.z, d[3] = q.w;
                if (FIRST && valid) {
                    const uchar4 u = *reinterpret_cast<const uchar4*>(valid + p);
                    v[0] = u.x, v[1] = u.y, v[2] = u.z, v[3] = u.w;
                }
                if (FIRST && confidence) {
                    const float4 u = *reinterpret_cast<const float4*>(confidence + p);
                    c[0] = u.x, c[1] = u.y, c[2] = u.z, c[3] = u.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (x + j < a.w) {
                        d[j] = disparity[p + j];
                        if (FIRST && valid) v[j] = valid[p + j];
                        if (FIRST && confidence) c[j] = confidence[p + j];
                    }
                }
            }
            if constexpr (FIRST) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    bool ok = isfinite(d[j]) && d[j] > 0.f && v[j] != 0;
                    if (confidence) ok = ok && c[j] >= a.min_confidence;   // (a NaN confidence fails too)
                    d[j] = ok ? d[j] : nan;
                }
            }
        }
        *reinterpret_cast<float4*>(level0 + row * kStride0 + col) = make_float4(d[0], d[1], d[2], d[3]);
    }
    __syncthreads();

    // level 1: 16 x 16, every thread one pixel
    {
        const int ly = tid >> 4, lx = tid & 15;
        const float value = halve_at(level0, kStride0, ly, lx, a.max_difference);
        level1[ly * kStride1 + lx] = value;
        const int h1 = a.h >> 1, w1 = a.w >> 1, y = (y0 >> 1) + ly, x = (x0 >> 1) + lx;
        if (y < h1 && x < w1) a.out[0][((size_t)b * h1 + y) * w1 + x] = value;
    }
    if (a.levels < 2) return;   // (uniform over the workgroup)
    __syncthreads();

    // level 2: 8 x 8, wave 0
    if (tid < 64) {
        const int ly = tid >> 3, lx = tid & 7;
        const float value = halve_at(level1, kStride1, ly, lx, a.max_difference);
        level2[ly * kStride2 + lx] = value;
        const int h2 = a.h >> 2, w2 = a.w >> 2, y = (y0 >> 2) + ly, x = (x0 >> 2) + lx;
        if (y < h2 && x < w2) a.out[1][((size_t)b * h2 + y) * w2 + x] = value;
    }
    if (a.levels < 3) return;
    __syncthreads();

    // level 3: 4 x 4
    if (tid < 16) {
        const int ly = tid >> 2, lx = tid & 3;
        const float value = halve_at(level2, kStride2, ly, lx, a.max_difference);
        const int h3 = a.h >> 3, w3 = a.w >> 3, y = (y0 >> 3) + ly, x = (x0 >> 3) + lx;
        if (y < h3 && x < w3) a.out[2][((size_t)b * h3 + y) * w3 + x] = value;
    }
}

}  // namespace

int pyramid_groups(int batch, int h, int w) {
    const long long groups = (long long)batch * ((h + kPyramidBlock - 1) / kPyramidBlock) *
                             ((w + kPyramidBlock - 1) / kPyramidBlock);
    return groups > 0x7fffffffLL ? 0 : (int)groups;
}

// batch * h * w fits int (checked by the entry point), so the number of blocks does
int launch_disparity_pyramid(const float* disparity, const unsigned char* valid, const float* confidence,
                             float min_confidence, float max_difference, float* const* out, int levels, int source_level,
                             int batch, int h, int w, hipStream_t s) {
    PyramidArgs a = {};
    for (int k = 0; k < levels; ++k) a.out[k] = out[k];
    a.min_confidence = min_confidence;
    a.max_difference = max_difference;
    a.levels = levels;
    a.h = h;
    a.w = w;
    a.tiles_x = (w + kPyramidBlock - 1) / kPyramidBlock;
    a.tiles_y = (h + kPyramidBlock - 1) / kPyramidBlock;
    const int groups = pyramid_groups(batch, h, w);
    const bool first = source_level == 0;
    const bool vec = w % 4 == 0 && ((uintptr_t)disparity & 15) == 0 &&
                     (!first || ((!valid || ((uintptr_t)valid & 3) == 0) && (!confidence || ((uintptr_t)confidence & 15) == 0)));
    const int probe = probe_before("disparity_pyramid", s);
    if (first) {
        if (vec)
            hipLaunchKernelGGL((disparity_pyramid_kernel<true, true>), dim3(groups), dim3(kPyramidThreads), 0, s, a,
                               disparity, valid, confidence);
        else
            hipLaunchKernelGGL((disparity_pyramid_kernel<true, false>), dim3(groups), dim3(kPyramidThreads), 0, s, a,
                               disparity, valid, confidence);
    } else {
        if (vec)
            hipLaunchKernelGGL((disparity_pyramid_kernel<false, true>), dim3(groups), dim3(kPyramidThreads), 0, s, a,
                               disparity, nullptr, nullptr);
        else
            hipLaunchKernelGGL((disparity_pyramid_kernel<false, false>), dim3(groups), dim3(kPyramidThreads), 0, s, a,
                               disparity, nullptr, nullptr);
    }
    probe_after(probe, groups, s);
    return check_launch("disparity_pyramid");
}

}  // namespace pds
