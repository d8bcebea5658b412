// Speckle filter: sizes of the 4-connected regions of similar disparity (pds_speckle_filter_fwd; not in the reference).
//
// A pixel is eligible iff its disparity is finite and its `valid` byte (if given) is non-zero; two eligible horizontal or
// vertical neighbours are linked iff fabsf(D[p] - D[q]) <= max_difference (one fp32 subtraction, no multiply: contraction
// cannot change it); a region is a connected component under these links.  Labels are pixel indices within one image and
// every union hooks the larger root onto the smaller one, so the root of a region is its smallest pixel index whatever
// the order in which the integer atomics land: sizes, keep and filtered are exact and reproducible.
//
// Block-based union-find (Komura; Playne & Hawick) in four launches on the caller's stream, none of which waits for
// another workgroup:
//   speckle_tile_kernel    one workgroup per 64 x 32 tile.  A wave takes a row: a ballot of "not linked to the left" gives
//                          every pixel the first pixel of its run as label and every run its length without any union;
//                          runs are then united with the row above by atomicMin union-find in LDS, the roots' pixels
//                          counted in LDS (one add per run), and the workspace receives, per pixel, the image index of its
//                          tile-local root (-1: not eligible) and, at root pixels, the local count (0 elsewhere).
//   speckle_seam_kernel    one thread per pixel pair across a tile seam: union in global memory (agent-scope loads,
//                          atomicMin; the loop is repeated only when the atomic found that its target was no root any
//                          more, never to wait for somebody).
//   speckle_count_kernel   every tile-local root that is not the region's root adds its count to the region's root (a few
//                          hundred adds for a background of half a million pixels, not one per pixel) and points at it.
//   speckle_output_kernel  per pixel: tile-local root -> region root -> count; writes sizes / keep / filtered, four pixels
//                          per thread where the row width and the pointers allow 16-byte accesses.
#include "common.hpp"

namespace pds {

namespace {

constexpr int kTileW = 64;                       // one wave per row
constexpr int kTileH = 32;
constexpr int kTileThreads = 256;
constexpr int kTileWaves = kTileThreads / 64;
constexpr int kTileRows = kTileH / kTileWaves;   // rows of one wave
constexpr int kSpeckleThreads = 256;
constexpr int kSpeckleMaxGrid = 256 * 64;

static_assert(kTileW == 64, "a tile row is one wave");

__device__ __forceinline__ int lds_load(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ int agent_load(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int find_lds(const int* L, int a) {
    for (int p = lds_load(L + a); p != a; p = lds_load(L + a)) a = p;
    return a;
}

// unites the trees of a and b: the larger root is hooked onto the smaller one; when the atomic finds that its target had
// been hooked elsewhere meanwhile, the walk goes on from where it points now
__device__ __forceinline__ void union_lds(int* L, int a, int b) {
    for (;;) {
        a = find_lds(L, a);
        b = find_lds(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(L + a, b);   // a > b
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ int find_global(const int* L, int a) {
    for (int p = agent_load(L + a); p != a; p = agent_load(L + a)) a = p;
    return a;
}

__device__ __forceinline__ void union_global(int* L, int a, int b) {
    for (;;) {
        a = find_global(L, a);
        b = find_global(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(L + a, b);
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ bool linked(float a, float b, float max_difference) {
    return fabsf(a - b) <= max_difference;   // false when either is NaN
}

// the disparity of an eligible pixel, NaN otherwise
__device__ __forceinline__ float eligible_value(const float* __restrict__ d, const unsigned char* __restrict__ valid,
                                                size_t i) {
    const float v = d[i];
    const bool ok = isfinite(v) && (!valid || valid[i] != 0);
    return ok ? v : __builtin_nanf("");
}

// grid: batch * tiles_y * tiles_x workgroups
__global__ __launch_bounds__(kTileThreads) void speckle_tile_kernel(const float* __restrict__ disparity,
                                                                    const unsigned char* __restrict__ valid,
                                                                    int* __restrict__ labels, int* __restrict__ counts,
                                                                    int h, int w, int tiles_x, int tiles_y,
                                                                    float max_difference) {
    __shared__ float val[kTileH * kTileW];
    __shared__ int lab[kTileH * kTileW];
    __shared__ int cnt[kTileH * kTileW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x % (tiles_x * tiles_y), b = blockIdx.x / (tiles_x * tiles_y);
    const int y0 = (tile / tiles_x) * kTileH, x0 = (tile % tiles_x) * kTileW;
    const size_t image = (size_t)b * h * w;
    const int gx = x0 + lane;

    float v[kTileRows];
    int len[kTileRows];   // length of the run this pixel starts (0: it starts none, or is not eligible)
#pragma unroll
    for (int i = 0; i < kTileRows; ++i) {
        const int r = wave * kTileRows + i, gy = y0 + r;
        v[i] = gy < h && gx < w ? eligible_value(disparity, valid, image + (size_t)gy * w + gx) : __builtin_nanf("");
        const float left = __shfl_up(v[i], 1, 64);
        const bool link_left = lane > 0 && linked(v[i], left, max_difference);
        const unsigned long long starts = __ballot(!link_left);   // bit 0 is always set
        const int start = 63 - __clzll(starts & (~0ull >> (63 - lane)));
        const unsigned long long rest = lane == 63 ? 0ull : starts >> (lane + 1);
        len[i] = link_left || !(v[i] == v[i]) ? 0 : rest ? __ffsll(rest) : 64 - lane;
        val[r * kTileW + lane] = v[i];
        lab[r * kTileW + lane] = r * kTileW + start;
        cnt[r * kTileW + lane] = 0;
    }
    __syncthreads();

    // unions with the row above; the link (r, c) - (r - 1, c) adds nothing when both pixels are linked to their left
    // neighbours and those are linked to each other
#pragma unroll
    for (int i = 0; i < kTileRows; ++i) {
        const int r = wave * kTileRows + i;
        if (r == 0) continue;   // (wave-uniform)
        const float up = val[(r - 1) * kTileW + lane];
        const float left = __shfl_up(v[i], 1, 64), up_left = __shfl_up(up, 1, 64);
        const bool link_up = linked(v[i], up, max_difference);
        const bool left_link_up = __shfl_up((int)link_up, 1, 64) != 0;
        const bool implied = lane > 0 && left_link_up && linked(v[i], left, max_difference) &&
                             linked(up, up_left, max_difference);
        if (link_up && !implied) union_lds(lab, r * kTileW + lane, (r - 1) * kTileW + lane);
    }
    __syncthreads();

    int root[kTileRows];
#pragma unroll
    for (int i = 0; i < kTileRows; ++i) {
        root[i] = find_lds(lab, (wave * kTileRows + i) * kTileW + lane);
        if (len[i] > 0) atomicAdd(cnt + root[i], len[i]);
    }
    __syncthreads();

#pragma unroll
    for (int i = 0; i < kTileRows; ++i) {
        const int r = wave * kTileRows + i, gy = y0 + r;
        if (gy >= h || gx >= w) continue;
        const int p = gy * w + gx, local = r * kTileW + lane;
        const bool ok = v[i] == v[i];
        labels[image + p] = ok ? (y0 + root[i] / kTileW) * w + x0 + root[i] % kTileW : -1;
        counts[image + p] = ok && root[i] == local ? cnt[local] : 0;
    }
}

// One thread per pixel pair across a seam of one image: first the h * (tiles_x - 1) pairs (y, 64 k - 1) | (y, 64 k), then
// the w * (tiles_y - 1) pairs (32 k - 1, x) | (32 k, x).  A pair whose link is implied by the previous pair along the seam
// and the two links beside it is skipped when those two lie inside tiles (the tile pass has made them): at a tile corner
// nothing is skipped, which keeps the skips of the two seam directions from relying on each other.
__global__ __launch_bounds__(kSpeckleThreads) void speckle_seam_kernel(const float* __restrict__ disparity,
                                                                       int* labels, int h, int w, int tiles_x,
                                                                       int tiles_y, float max_difference, int batch) {
    const int across = h * (tiles_x - 1), per_image = across + w * (tiles_y - 1);
    const long long total = (long long)per_image * batch;
    for (long long i = (long long)blockIdx.x * kSpeckleThreads + threadIdx.x; i < total;
         i += (long long)gridDim.x * kSpeckleThreads) {
        const int b = (int)(i / per_image), j = (int)(i % per_image);
        const size_t image = (size_t)b * h * w;
        const float* D = disparity + image;
        int* L = labels + image;
        int p, q, back;      // the pair, and the step to the previous pair along the seam
        bool inside;         // the previous pair lies in the same two tiles
        if (j < across) {
            const int y = j % h, x = (j / h + 1) * kTileW;
            p = y * w + x - 1;
            q = p + 1;
            back = w;
            inside = y % kTileH != 0;
        } else {
            const int k = j - across, x = k % w, y = (k / w + 1) * kTileH;
            p = (y - 1) * w + x;
            q = p + w;
            back = 1;
            inside = x % kTileW != 0;
        }
        // eligibility as the tile pass saw it (the tile pass wrote these labels in an earlier launch; a stale positive
        // value is still positive)
        if (agent_load(L + p) < 0 || agent_load(L + q) < 0) continue;
        const float dp = D[p], dq = D[q];
        if (!linked(dp, dq, max_difference)) continue;
        if (inside && agent_load(L + p - back) >= 0 && agent_load(L + q - back) >= 0) {
            const float ep = D[p - back], eq = D[q - back];
            if (linked(ep, eq, max_difference) && linked(dp, ep, max_difference) && linked(dq, eq, max_difference))
                continue;
        }
        union_global(L, p, q);
    }
}

// total = batch * h * w
__global__ __launch_bounds__(kSpeckleThreads) void speckle_count_kernel(int* labels, int* counts, int hw, int total) {
    for (int i = blockIdx.x * kSpeckleThreads + threadIdx.x; i < total; i += gridDim.x * kSpeckleThreads) {
        const int c = counts[i];
        if (c <= 0) continue;                    // not a tile-local root
        const int p = i % hw;
        int* L = labels + (i - p);
        const int parent = agent_load(L + p);
        if (parent == p) continue;               // a region root: it only receives
        const int r = find_global(L, parent);    // no union in this launch: r stays the root
        atomicAdd(counts + (i - p) + r, c);
        __hip_atomic_store(L + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // walks through p get shorter
    }
}

__device__ __forceinline__ int region_size(const int* __restrict__ L, const int* __restrict__ C, int p) {
    int r = L[p];
    if (r < 0) return 0;
    for (int n = L[r]; n != r; n = L[r]) r = n;   // at most two steps after the count pass
    return C[r];
}

// VEC: groups of four pixels (w % 4 == 0, so a group never crosses an image); scalar: one pixel per thread.  A thread
// reads disparity[p] and then writes filtered[p] itself, so the two may be the same buffer (no __restrict__ on them).
template <bool VEC>
__global__ __launch_bounds__(kSpeckleThreads) void speckle_output_kernel(const float* disparity,
                                                                         const int* __restrict__ labels,
                                                                         const int* __restrict__ counts,
                                                                         unsigned char* __restrict__ keep,
                                                                         float* filtered, int* __restrict__ sizes,
                                                                         int hw, int total, int max_size, float fill) {
    const int end = VEC ? total >> 2 : total;
    for (int i = blockIdx.x * kSpeckleThreads + threadIdx.x; i < end; i += gridDim.x * kSpeckleThreads) {
        if constexpr (VEC) {
            const int g = i << 2, p = g % hw;
            const int* L = labels + (g - p);
            const int* C = counts + (g - p);
            const int s0 = region_size(L, C, p), s1 = region_size(L, C, p + 1), s2 = region_size(L, C, p + 2),
                      s3 = region_size(L, C, p + 3);
            const bool k0 = s0 > max_size, k1 = s1 > max_size, k2 = s2 > max_size, k3 = s3 > max_size;
            *reinterpret_cast<uchar4*>(keep + g) = make_uchar4(k0, k1, k2, k3);
            if (sizes) *reinterpret_cast<int4*>(sizes + g) = make_int4(s0, s1, s2, s3);
            if (filtered) {
                const float4 d = *reinterpret_cast<const float4*>(disparity + g);
                *reinterpret_cast<float4*>(filtered + g) =
                    make_float4(k0 ? d.x : fill, k1 ? d.y : fill, k2 ? d.z : fill, k3 ? d.w : fill);
            }
        } else {
            const int p = i % hw;
            const int s = region_size(labels + (i - p), counts + (i - p), p);
            const bool k = s > max_size;
            keep[i] = k;
            if (sizes) sizes[i] = s;
            if (filtered) filtered[i] = k ? disparity[i] : fill;
        }
    }
}

int speckle_grid(long long items) {
    const long long blocks = (items + kSpeckleThreads - 1) / kSpeckleThreads;
    return (int)(blocks < 1 ? 1 : blocks > kSpeckleMaxGrid ? kSpeckleMaxGrid : blocks);
}

bool speckle_aligned(const void* p, unsigned mask) { return ((uintptr_t)p & mask) == 0; }

}  // namespace

// the grid-stride loops count in int: the last stride beyond the last pixel must stay below 2^31
size_t speckle_max_pixels() { return 0x7fffffffu - (size_t)kSpeckleMaxGrid * kSpeckleThreads; }

size_t speckle_workspace_bytes(int batch, int h, int w) {
    return (size_t)batch * h * w * 2 * sizeof(int) + 256;   // labels, counts
}

int launch_speckle_filter(const float* disparity, const unsigned char* valid, unsigned char* keep, float* filtered,
                          int* sizes, int batch, int h, int w, float max_difference, int max_size, float fill,
                          void* workspace, hipStream_t s) {
    const int total = batch * h * w, hw = h * w;
    const int tiles_x = (w + kTileW - 1) / kTileW, tiles_y = (h + kTileH - 1) / kTileH;
    int* labels = reinterpret_cast<int*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
    int* counts = labels + (((size_t)total + 3) & ~(size_t)3);
    hipLaunchKernelGGL(speckle_tile_kernel, dim3(batch * tiles_x * tiles_y), dim3(kTileThreads), 0, s, disparity, valid,
                       labels, counts, h, w, tiles_x, tiles_y, max_difference);
    const long long pairs = ((long long)h * (tiles_x - 1) + (long long)w * (tiles_y - 1)) * batch;
    if (pairs > 0) {
        hipLaunchKernelGGL(speckle_seam_kernel, dim3(speckle_grid(pairs)), dim3(kSpeckleThreads), 0, s, disparity,
                           labels, h, w, tiles_x, tiles_y, max_difference, batch);
        hipLaunchKernelGGL(speckle_count_kernel, dim3(speckle_grid(total)), dim3(kSpeckleThreads), 0, s, labels, counts,
                           hw, total);
    }
    const bool vec = w % 4 == 0 && speckle_aligned(keep, 3) && (!sizes || speckle_aligned(sizes, 15)) &&
                     (!filtered || (speckle_aligned(filtered, 15) && speckle_aligned(disparity, 15)));
    if (vec)
        hipLaunchKernelGGL(speckle_output_kernel<true>, dim3(speckle_grid(total / 4)), dim3(kSpeckleThreads), 0, s,
                           disparity, labels, counts, keep, filtered, sizes, hw, total, max_size, fill);
    else
        hipLaunchKernelGGL(speckle_output_kernel<false>, dim3(speckle_grid(total)), dim3(kSpeckleThreads), 0, s,
                           disparity, labels, counts, keep, filtered, sizes, hw, total, max_size, fill);
    return check_launch("speckle_filter");
}

}  // namespace pds
