// Left-right consistency check and background fill (pds_left_right_check_fwd; not in the reference).
//
// A left pixel (b, y, x) with d = DL[b,y,x] points at k = floorf(((float)x - d) + 0.5f) of the right view and is valid
// iff d is finite, 0 <= k < w and |d - DR[b,y,k]| <= max_difference; a right pixel points at k = floorf(((float)x + d)
// + 0.5f) and is compared with DL[b,y,k].  No multiply: fp-contraction cannot change the result.  The fill gives every
// invalid pixel min(D[l], D[r]) of the nearest valid pixels l < x < r on its row (the one that exists if only one does;
// a row without a valid pixel is copied).
//
// Everything happens along a row, so one workgroup takes one row of both views.  Its 256 threads own contiguous
// segments of ceil(w / 256) pixels: a thread computes the masks of its segment and its first and last valid pixel of
// either view; an exclusive max-scan of the last valid pixels (wave shuffles, then the waves' totals through LDS) gives
// every segment its nearest valid pixel to the left, an exclusive min-scan of the first valid pixels the nearest one to
// the right.  The fill then walks the segment once, closing each run of invalid pixels at the valid pixel that ends it.
// Both rows are staged in LDS when they fit (w <= kStagedMaxWidth, 32 KiB); wider rows are gathered from global memory.
#include "common.hpp"

namespace pds {

namespace {

constexpr int kCheckThreads = 256;
constexpr int kCheckWaves = kCheckThreads / 64;
constexpr int kStagedMaxWidth = 4096;

// the check of pixel x of one view: `own` is that view's row, `other` the other view's
template <bool RIGHT>
__device__ __forceinline__ bool consistent(const float* own, const float* other, int x, int w, float max_difference) {
    const float d = own[x];
    const float k = floorf((RIGHT ? (float)x + d : (float)x - d) + 0.5f);
    if (!(isfinite(d) && k >= 0.f && k < (float)w)) return false;
    return fabsf(d - other[(int)k]) <= max_difference;
}

// fill of one view's segment [x0, x1): l = the nearest valid pixel left of the segment (-1: none), r_after = the nearest
// valid pixel right of it (w: none)
template <bool RIGHT>
__device__ __forceinline__ void fill_segment(const float* own, const float* other, float* __restrict__ out, int x0,
                                             int x1, int l, int r_after, int w, float max_difference) {
    int run = -1;   // first pixel of the pending run of invalid pixels
    for (int x = x0; x < x1; ++x) {
        if (consistent<RIGHT>(own, other, x, w, max_difference)) {
            if (run >= 0) {
                const float v = l >= 0 ? fminf(own[l], own[x]) : own[x];
                for (int y = run; y < x; ++y) out[y] = v;
                run = -1;
            }
            out[x] = own[x];
            l = x;
        } else if (run < 0) {
            run = x;
        }
    }
    if (run >= 0) {
        if (l < 0 && r_after >= w) {   // no valid pixel on the row
            for (int y = run; y < x1; ++y) out[y] = own[y];
        } else {
            const float v = l < 0 ? own[r_after] : r_after >= w ? own[l] : fminf(own[l], own[r_after]);
            for (int y = run; y < x1; ++y) out[y] = v;
        }
    }
}

// one workgroup per row (b, y)
template <bool STAGED>
__global__ __launch_bounds__(kCheckThreads) void left_right_check_kernel(const float* __restrict__ dl,
                                                                        const float* __restrict__ dr,
                                                                        unsigned char* __restrict__ lv,
                                                                        unsigned char* __restrict__ rv,
                                                                        float* __restrict__ lf, float* __restrict__ rf,
                                                                        int w, float max_difference) {
    extern __shared__ float rows[];                // STAGED: [2][w], the left row then the right row
    __shared__ int totals[4][kCheckWaves];
    const size_t base = (size_t)blockIdx.x * w;
    const float* L = dl + base;
    const float* R = dr + base;
    if constexpr (STAGED) {
        for (int x = threadIdx.x; x < w; x += kCheckThreads) {
            rows[x] = L[x];
            rows[w + x] = R[x];
        }
        __syncthreads();
        L = rows;
        R = rows + w;
    }
    const int seg = (w + kCheckThreads - 1) / kCheckThreads;
    const int x0 = min((int)threadIdx.x * seg, w), x1 = min(x0 + seg, w);
    int first_l = w, last_l = -1, first_r = w, last_r = -1;
    for (int x = x0; x < x1; ++x) {
        const bool vl = consistent<false>(L, R, x, w, max_difference);
        const bool vr = consistent<true>(R, L, x, w, max_difference);
        lv[base + x] = vl;
        rv[base + x] = vr;
        if (vl) {
            first_l = last_l < 0 ? x : first_l;
            last_l = x;
        }
        if (vr) {
            first_r = last_r < 0 ? x : first_r;
            last_r = x;
        }
    }
    if (!lf && !rf) return;   // (uniform: kernel arguments)

    // inclusive scans within the wave: the last valid pixel up to this lane (max), the first one from it on (min)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int pl = last_l, pr = last_r, sl = first_l, sr = first_r;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int tpl = __shfl_up(pl, off, 64), tpr = __shfl_up(pr, off, 64);
        const int tsl = __shfl_down(sl, off, 64), tsr = __shfl_down(sr, off, 64);
        if (lane >= off) {
            pl = max(pl, tpl);
            pr = max(pr, tpr);
        }
        if (lane + off < 64) {
            sl = min(sl, tsl);
            sr = min(sr, tsr);
        }
    }
    if (lane == 63) {
        totals[0][wave] = pl;
        totals[1][wave] = pr;
    }
    if (lane == 0) {
        totals[2][wave] = sl;
        totals[3][wave] = sr;
    }
    // exclusive: the neighbouring lane's inclusive value, then the other waves' totals
    int left_l = __shfl_up(pl, 1, 64), left_r = __shfl_up(pr, 1, 64);
    int right_l = __shfl_down(sl, 1, 64), right_r = __shfl_down(sr, 1, 64);
    if (lane == 0) left_l = left_r = -1;
    if (lane == 63) right_l = right_r = w;
    __syncthreads();
    for (int q = 0; q < wave; ++q) {
        left_l = max(left_l, totals[0][q]);
        left_r = max(left_r, totals[1][q]);
    }
    for (int q = wave + 1; q < kCheckWaves; ++q) {
        right_l = min(right_l, totals[2][q]);
        right_r = min(right_r, totals[3][q]);
    }
    if (lf) fill_segment<false>(L, R, lf + base, x0, x1, left_l, right_l, w, max_difference);
    if (rf) fill_segment<true>(R, L, rf + base, x0, x1, left_r, right_r, w, max_difference);
}

}  // namespace

int launch_left_right_check(const float* dl, const float* dr, unsigned char* lv, unsigned char* rv, float* lf,
                            float* rf, int rows, int w, float max_difference, hipStream_t s) {
    if (w <= kStagedMaxWidth)
        hipLaunchKernelGGL(left_right_check_kernel<true>, dim3(rows), dim3(kCheckThreads), 2 * (size_t)w * sizeof(float),
                           s, dl, dr, lv, rv, lf, rf, w, max_difference);
    else
        hipLaunchKernelGGL(left_right_check_kernel<false>, dim3(rows), dim3(kCheckThreads), 0, s, dl, dr, lv, rv, lf, rf,
                           w, max_difference);
    return check_launch("left_right_check");
}

}  // namespace pds
