// Hole-aware median filter of a disparity map (pds_median_filter_fwd; not in the reference).
//
// Per image: W(p) = the eligible pixels (finite, and valid != 0 where a mask is given) of the k x k window around p,
// clipped at the border; n = |W(p)|; median(p) = the value of rank (n - 1) / 2 among them (the LOWER median: no two
// samples are averaged).  An eligible pixel receives median(p); a pixel that is not eligible receives it only with
// fill_holes and n >= min_valid, fill_value otherwise (include/pds_hip.h).
//
// One launch, no atomics, no traffic between workgroups.  A workgroup of 256 threads owns a tile of kMedianTileW x
// kMedianTileH = 64 x 16 pixels:
//   staging    the tile plus a halo of r = k / 2 pixels goes to LDS once, as the ORDERED INTEGER KEY of the value
//              (key = bits ^ ((bits >> 31) & 0x7fffffff): signed integer order == fp32 order, so v_min_i32 / v_max_i32
//              select and no floating-point mode -- denormals, -0.0 -- can touch a value) or kMissing = INT_MAX where the
//              pixel is not eligible or lies outside the image.  The finiteness test and the mask byte are paid here,
//              once per pixel.  No finite value has the key INT_MAX or INT_MIN (both are NaN patterns).
//   selection  a thread produces four neighbouring pixels of one row.  Per pixel a forgetful selection (Perrot, Domas,
//              Couturier 2014) over registers with compile-time indices: with K = k * k = 2 c + 1 samples, keep c + 2 of
//              them, drop their minimum and their maximum (neither can be the median), take the next sample in, until
//              three are left; the middle one is the sample of rank c.  A step over s registers costs 3 s / 2 - 1
//              compare-exchanges (pairs, then the minimum of the lower and the maximum of the upper halves).
//   holes      the rank wanted, (n - 1) / 2, moves with n; the rank selected is fixed.  With M = K - n missing samples,
//              c - (n - 1) / 2 = ceil(M / 2) of them are replaced by INT_MIN ("-inf") and the rest stay INT_MAX
//              ("+inf"): the sample of rank (n - 1) / 2 among the n real ones then sits at rank c of all K.  In the
//              order the samples are taken, the 1st, 3rd, 5th ... missing one becomes -inf: a counter, no indexing.
//              A tile whose staged pixels are all eligible (the common case inside a surface) skips that counter: the
//              decision is uniform over the workgroup (__syncthreads_or).
//   stores     float4 / uchar4 where w % 4 == 0 and the pointers are 16- / 4-byte aligned (VEC), scalar otherwise.
#include "common.hpp"

namespace pds {

namespace {

constexpr int kMedianTileW = 64;
constexpr int kMedianTileH = 16;
constexpr int kMedianThreads = 256;
constexpr int kMedianPerThread = 4;              // neighbouring pixels of one row per thread
constexpr int kMissing = 0x7fffffff;             // "+inf": not eligible, or outside the image
constexpr int kMinusInf = (int)0x80000000u;

static_assert(kMedianTileW / kMedianPerThread * kMedianTileH == kMedianThreads, "one thread per four pixels of the tile");

__device__ __forceinline__ int key_of(float v) {
    const int b = __float_as_int(v);
    return b ^ ((b >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float value_of(int key) { return __int_as_float(key ^ ((key >> 31) & 0x7fffffff)); }

__device__ __forceinline__ void compare_exchange(int& lo, int& hi) {
    const int a = lo, b = hi;
    lo = min(a, b);
    hi = max(a, b);
}

// sample i of the window in the order they are taken; HOLES: every odd missing sample becomes -inf (see above)
template <bool HOLES>
__device__ __forceinline__ int take(int key, int& missing) {
    if constexpr (HOLES) {
        const bool miss = key == kMissing;
        missing += miss ? 1 : 0;
        return miss && (missing & 1) ? kMinusInf : key;
    } else {
        return key;
    }
}

// The key of rank K / 2 among the K = k * k samples at window[dy * stride + dx]; `missing` receives K - n.
template <int KS, bool HOLES>
__device__ __forceinline__ int select_median(const int* window, int stride, int& missing) {
    constexpr int K = KS * KS, C = K / 2, S = C + 2;
    int a[S];
    missing = 0;
#pragma unroll
    for (int i = 0; i < S; ++i) a[i] = take<HOLES>(window[(i / KS) * stride + i % KS], missing);
#pragma unroll
    for (int s = S; s >= 3; --s) {
        // the smaller of every pair (i, s - 1 - i) to the lower half, then the minimum to a[0], the maximum to a[s - 1]
#pragma unroll
        for (int i = 0; i < s / 2; ++i) compare_exchange(a[i], a[s - 1 - i]);
#pragma unroll
        for (int i = 1; i < (s + 1) / 2; ++i) compare_exchange(a[0], a[i]);
#pragma unroll
        for (int i = s / 2; i < s - 1; ++i) compare_exchange(a[i], a[s - 1]);
        if (s > 3) {
            // a[0] and a[s - 1] are forgotten: the next sample takes the place of a[0], the set is a[0 .. s - 2]
            const int next = S + (S - s);
            a[0] = take<HOLES>(window[(next / KS) * stride + next % KS], missing);
        }
    }
    return a[1];
}

template <int KS, bool VEC, bool HOLES>
__device__ __forceinline__ void median_outputs(const int* tile, int stride, int tx, int ty, float* __restrict__ filtered,
                                               unsigned char* __restrict__ ok, size_t row, int x, int w, int fill_holes,
                                               int min_valid, float fill) {
    constexpr int R = KS / 2, K = KS * KS;
    float out[kMedianPerThread] = {fill, fill, fill, fill};
    unsigned char good[kMedianPerThread] = {0, 0, 0, 0};
    // One selection at a time (not unrolled: four interleaved selections of 7 x 7 need more than 256 registers); the
    // results go to their slots by compile-time index all the same, so nothing lives in scratch.
#pragma unroll 1
    for (int j = 0; j < kMedianPerThread; ++j) {
        const int* window = tile + ty * stride + tx * kMedianPerThread + j;   // its top left corner
        int missing;
        const int median = select_median<KS, HOLES>(window, stride, missing);
        bool keep = true;
        if constexpr (HOLES) {
            const bool eligible = window[R * stride + R] != kMissing;
            keep = eligible || (fill_holes && K - missing >= min_valid);
        }
        const float value = keep ? value_of(median) : fill;
#pragma unroll
        for (int slot = 0; slot < kMedianPerThread; ++slot) {
            out[slot] = slot == j ? value : out[slot];
            good[slot] = slot == j ? (unsigned char)keep : good[slot];
        }
    }
    if constexpr (VEC) {
        // (w % 4 == 0 and x % 4 == 0: the four pixels are inside the row together)
        *reinterpret_cast<float4*>(filtered + row + x) = make_float4(out[0], out[1], out[2], out[3]);
        if (ok) *reinterpret_cast<uchar4*>(ok + row + x) = make_uchar4(good[0], good[1], good[2], good[3]);
    } else {
#pragma unroll
        for (int j = 0; j < kMedianPerThread; ++j) {
            if (x + j < w) {
                filtered[row + x + j] = out[j];
                if (ok) ok[row + x + j] = good[j];
            }
        }
    }
}

// grid: batch * tiles_y * tiles_x workgroups
template <int KS, bool VEC>
__global__ __launch_bounds__(kMedianThreads) void median_filter_kernel(const float* __restrict__ disparity,
                                                                       const unsigned char* __restrict__ valid,
                                                                       float* __restrict__ filtered,
                                                                       unsigned char* __restrict__ ok, int h, int w,
                                                                       int tiles_x, int tiles_y, int fill_holes,
                                                                       int min_valid, float fill) {
    constexpr int R = KS / 2, LW = kMedianTileW + 2 * R, LH = kMedianTileH + 2 * R;
    __shared__ int tile[LH * LW];
    const int t = blockIdx.x % (tiles_x * tiles_y), b = blockIdx.x / (tiles_x * tiles_y);
    const int y0 = (t / tiles_x) * kMedianTileH, x0 = (t % tiles_x) * kMedianTileW;
    const size_t image = (size_t)b * h * w;

    int holes = 0;
    for (int i = threadIdx.x; i < LH * LW; i += kMedianThreads) {
        const int gy = y0 - R + i / LW, gx = x0 - R + i % LW;
        int key = kMissing;
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
            const size_t p = image + (size_t)gy * w + gx;
            const float v = disparity[p];
            if (isfinite(v) && (!valid || valid[p] != 0)) key = key_of(v);
        }
        holes |= key == kMissing;
        tile[i] = key;
    }
    const bool any_hole = __syncthreads_or(holes) != 0;   // (the barrier between staging and selection as well)

    const int tx = threadIdx.x % (kMedianTileW / kMedianPerThread), ty = threadIdx.x / (kMedianTileW / kMedianPerThread);
    const int x = x0 + tx * kMedianPerThread, y = y0 + ty;
    if (y >= h || x >= w) return;
    const size_t row = image + (size_t)y * w;
    if (any_hole)
        median_outputs<KS, VEC, true>(tile, LW, tx, ty, filtered, ok, row, x, w, fill_holes, min_valid, fill);
    else
        median_outputs<KS, VEC, false>(tile, LW, tx, ty, filtered, ok, row, x, w, fill_holes, min_valid, fill);
}

template <int KS>
void launch_median_k(bool vec, int grid, hipStream_t s, const float* disparity, const unsigned char* valid,
                     float* filtered, unsigned char* ok, int h, int w, int tiles_x, int tiles_y, int fill_holes,
                     int min_valid, float fill) {
    if (vec)
        hipLaunchKernelGGL((median_filter_kernel<KS, true>), dim3(grid), dim3(kMedianThreads), 0, s, disparity, valid,
                           filtered, ok, h, w, tiles_x, tiles_y, fill_holes, min_valid, fill);
    else
        hipLaunchKernelGGL((median_filter_kernel<KS, false>), dim3(grid), dim3(kMedianThreads), 0, s, disparity, valid,
                           filtered, ok, h, w, tiles_x, tiles_y, fill_holes, min_valid, fill);
}

}  // namespace

// batch * h * w fits int (checked by the entry point), so the number of tiles does
int launch_median_filter(const float* disparity, const unsigned char* valid, float* filtered, unsigned char* ok,
                         int batch, int h, int w, int kernel_size, int fill_holes, int min_valid, float fill,
                         hipStream_t s) {
    const int tiles_x = (w + kMedianTileW - 1) / kMedianTileW, tiles_y = (h + kMedianTileH - 1) / kMedianTileH;
    const long long grid = (long long)batch * tiles_x * tiles_y;
    if (grid > 0x7fffffffLL) return set_error(-1, "median_filter: %lld tiles do not fit one launch", grid);
    const bool vec = w % 4 == 0 && ((uintptr_t)filtered & 15) == 0 && (!ok || ((uintptr_t)ok & 3) == 0);
    if (kernel_size == 3)
        launch_median_k<3>(vec, (int)grid, s, disparity, valid, filtered, ok, h, w, tiles_x, tiles_y, fill_holes,
                           min_valid, fill);
    else if (kernel_size == 5)
        launch_median_k<5>(vec, (int)grid, s, disparity, valid, filtered, ok, h, w, tiles_x, tiles_y, fill_holes,
                           min_valid, fill);
    else
        launch_median_k<7>(vec, (int)grid, s, disparity, valid, filtered, ok, h, w, tiles_x, tiles_y, fill_holes,
                           min_valid, fill);
    return check_launch("median_filter");
}

}  // namespace pds
