// Packed, coloured point cloud (pds_point_cloud_fwd; not in the reference): an ordered stream compaction fused with the
// reprojection and the colour gather.  The kept pixels of `reproject` are written packed, in raster order within a
// batch entry and the entries in batch order, with their colours, their pixel indices and the offsets of the entries.
//
// A pixel is kept iff the point reproject_one (reproject.hpp, the function behind pds_reproject_fwd) gives for it has an
// x that is not NaN -- the pixels a caller's ~isnan(points[..., 0]) keeps of the dense output -- and its depth lies in
// [min_depth, max_depth] (a bound of -inf / +inf is absent).  The packed xyz are that function's result, bit for bit.
//
// Three launches on the caller's stream, and NO workgroup ever waits on another (no look-back, no flag, no spin: a
// compaction that spins hangs when its predecessor is not resident, and the machine with it):
//   count    one workgroup of 256 threads per tile of kPointCloudTile = 1024 flat pixels (batch * h * w taken as one
//            row of pixels), four pixels per thread from one float4 of disparity; wave64 __ballot + popcount, the four
//            wave totals meet in LDS; one int per tile
//   scan     ONE workgroup of 1024 threads turns the tile counts into exclusive offsets in place, 1024 tiles at a time
//            with a carry (any number of tiles), and writes offsets[0] = 0 and offsets[batch] = the TRUE total
//   scatter  per tile again: the predicate is evaluated a second time, the rank of a kept pixel within its tile is
//            mbcnt over the four ballots + the wave prefix from LDS + the kept pixels before it in its own quad; xyz, rgb
//            and the pixel index are staged in LDS at their rank and leave as contiguous runs [tile_offset, tile_offset +
//            n): 16-byte stores wherever the OUTPUT address is 16-byte aligned (the staging is shifted by the run's
//            misalignment, so that an aligned store reads an aligned LDS address), element stores for the head and the
//            tail of the run.  Only rows below `capacity` are written.  The thread that owns the first pixel of batch
//            entry b = 1 .. batch - 1 writes offsets[b].
// Integer arithmetic only in the ordering: the result is the same on every run.
// VEC = false is the scalar load form for a disparity pointer that is not 16-byte aligned; the last total % 4 pixels
// are loaded one by one in either form (they belong to the last tile, whose order they share).
//
// pds_triangle_mesh_fwd (triangle_mesh.hip) takes its vertices from these three launches: launch_point_cloud_ranked is
// the same call whose scatter (its RANKS = true form, an instantiation of its own: the RANKS = false form behind
// pds_point_cloud_fwd is the kernel it was before) also writes the dense rank map -- per pixel its packed row, or -1
// where the pixel is not kept -- and launch_compaction_scan is the scan kernel, which the face counts go through again.
#include "compaction.hpp"

namespace pds {

namespace {

constexpr int kPcScanThreads = 1024;
constexpr int kPcScanWaves = kPcScanThreads / 64;

struct PointCloudArgs {
    ReprojectArgs r;
    float min_depth, max_depth;   // -inf / +inf: no bound
};

__device__ __forceinline__ bool kept(const PointCloudArgs& a, const Point3& q) {
    return q.x == q.x && (a.min_depth == -__builtin_inff() || q.z >= a.min_depth) &&
           (a.max_depth == __builtin_inff() || q.z <= a.max_depth);
}

// The quad of this thread: its first pixel and how many of its four pixels exist (0: none)
__device__ __forceinline__ int quad_of(int total, int& p0) {
    const long long first = (long long)blockIdx.x * kPointCloudTile + 4 * (int)threadIdx.x;
    if (first >= total) {
        p0 = 0;
        return 0;
    }
    p0 = (int)first;
    return total - p0 < 4 ? total - p0 : 4;
}

template <bool VEC>
__device__ __forceinline__ void load_quad(const float* __restrict__ disparity, int p0, int n, float (&d)[4]) {
    if (VEC && n == 4) {
        const float4 v = *reinterpret_cast<const float4*>(disparity + p0);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = k < n ? disparity[p0 + k] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------- count
template <bool VEC>
__global__ __launch_bounds__(kPcThreads) void point_cloud_count_kernel(PointCloudArgs a,
                                                                       const float* __restrict__ disparity,
                                                                       const unsigned char* __restrict__ valid,
                                                                       const float* __restrict__ confidence,
                                                                       int* __restrict__ tile_count, int total, int h,
                                                                       int w) {
    __shared__ int wave_total[kPcWaves];
    int p0;
    const int n = quad_of(total, p0);
    float d[4];
    load_quad<VEC>(disparity, p0, n, d);
    int count = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        bool keep = false;
        if (k < n) keep = kept(a, reproject_one(a.r, valid, confidence, p0 + k, d[k], h, w));
        count += __popcll(__ballot(keep));
    }
    if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
#pragma unroll
        for (int k = 0; k < kPcWaves; ++k) sum += wave_total[k];
        tile_count[blockIdx.x] = sum;
    }
}

// ---------------------------------------------------------------------------------------------- scan
// tiles[i]: the count of tile i on entry, the number of kept pixels in the tiles before it on exit
__global__ __launch_bounds__(kPcScanThreads) void point_cloud_scan_kernel(int* __restrict__ tiles, int count,
                                                                          int* __restrict__ offsets, int batch) {
    __shared__ int wave_sum[kPcScanWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int base = 0; base < count; base += kPcScanThreads) {
        const int i = base + tid;
        const int v = i < count ? tiles[i] : 0;
        int inclusive = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(inclusive, off, 64);
            if (lane >= off) inclusive += t;
        }
        if (lane == 63) wave_sum[wave] = inclusive;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < kPcScanWaves; ++k) {
            const int s = wave_sum[k];
            before += k < wave ? s : 0;
            all += s;
        }
        if (i < count) tiles[i] = carry + before + inclusive - v;
        carry += all;
        __syncthreads();   // (wave_sum is written again by the next 1024 tiles)
    }
    if (tid == 0) {
        offsets[0] = 0;
        offsets[batch] = carry;
    }
}

// ---------------------------------------------------------------------------------------------- scatter
// COLORS 0: none, 1: float32 NCHW image -> float32 rows, 2: uint8 NHWC image -> uint8 rows
// RANKS: also write rank_map[p] = the packed row of pixel p (capacity or not), -1 where p is not kept
template <bool VEC, int COLORS, bool RANKS>
__global__ __launch_bounds__(kPcThreads) void point_cloud_scatter_kernel(
    PointCloudArgs a, const float* __restrict__ disparity, const unsigned char* __restrict__ valid,
    const float* __restrict__ confidence, const void* __restrict__ image, const int* __restrict__ tile_offset,
    float* __restrict__ points, void* __restrict__ colors, int* __restrict__ index, int* __restrict__ offsets,
    long long capacity, int batch, int total, int h, int w, int* __restrict__ rank_map) {
    constexpr int T = kPointCloudTile;
    constexpr int kRgbBytes = COLORS == 1 ? 12 * T + 16 : COLORS == 2 ? 3 * T + 16 : 16;
    __shared__ alignas(16) unsigned char s_xyz[12 * T + 16];
    __shared__ alignas(16) unsigned char s_rgb[kRgbBytes];
    __shared__ alignas(16) unsigned char s_idx[4 * T + 16];
    __shared__ int wave_total[kPcWaves];

    const int base = tile_offset[blockIdx.x];   // kept pixels in the tiles before this one
    unsigned char* xyz_out = reinterpret_cast<unsigned char*>(points) + 12ll * base;
    unsigned char* rgb_out = static_cast<unsigned char*>(colors) + (COLORS == 1 ? 12ll : 3ll) * base;
    unsigned char* idx_out = reinterpret_cast<unsigned char*>(index) + 4ll * base;
    const int xyz_shift = (int)((uintptr_t)xyz_out & 15), rgb_shift = (int)((uintptr_t)rgb_out & 15),
              idx_shift = (int)((uintptr_t)idx_out & 15);

    int p0;
    const int n = quad_of(total, p0);
    float d[4];
    load_quad<VEC>(disparity, p0, n, d);
    Point3 q[4];
    bool keep[4];
    int before = 0, wave_n = 0;   // kept pixels of the lower lanes of this wave; of the whole wave
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        keep[k] = false;
        if (k < n) {
            q[k] = reproject_one(a.r, valid, confidence, p0 + k, d[k], h, w);
            keep[k] = kept(a, q[k]);
        }
        const unsigned long long ballot = __ballot(keep[k]);
        before += __builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
        wave_n += __popcll(ballot);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wave_total[wave] = wave_n;
    __syncthreads();
    int rank = before, tile_n = 0;
#pragma unroll
    for (int k = 0; k < kPcWaves; ++k) {
        const int s = wave_total[k];
        rank += k < wave ? s : 0;
        tile_n += s;
    }

    if (n > 0) {
        const int hw = h * w;
        int b = p0 / hw, pixel = p0 - b * hw;   // batch entry and pixel within it
        [[maybe_unused]] int row[4] = {-1, -1, -1, -1};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < n) {
                if (pixel == 0 && b > 0) offsets[b] = base + rank;   // entry b begins at this pixel
                if constexpr (RANKS) row[k] = keep[k] ? base + rank : -1;
                if (keep[k]) {
                    float* xyz = reinterpret_cast<float*>(s_xyz + xyz_shift) + 3 * rank;
                    xyz[0] = q[k].x;
                    xyz[1] = q[k].y;
                    xyz[2] = q[k].z;
                    if constexpr (COLORS == 1) {
                        const float* src = static_cast<const float*>(image) + (size_t)b * 3 * hw + pixel;
                        float* rgb = reinterpret_cast<float*>(s_rgb + rgb_shift) + 3 * rank;
                        rgb[0] = src[0];
                        rgb[1] = src[hw];
                        rgb[2] = src[2 * (size_t)hw];
                    } else if constexpr (COLORS == 2) {
                        const unsigned char* src = static_cast<const unsigned char*>(image) + 3 * (size_t)(p0 + k);
                        unsigned char* rgb = s_rgb + rgb_shift + 3 * rank;
                        rgb[0] = src[0];
                        rgb[1] = src[1];
                        rgb[2] = src[2];
                    }
                    if (index) reinterpret_cast<int*>(s_idx + idx_shift)[rank] = pixel;
                    ++rank;
                }
                if (++pixel == hw) {
                    pixel = 0;
                    ++b;
                }
            }
        }
        if constexpr (RANKS) {   // (rank_map is 16-byte aligned and p0 a multiple of 4)
            if (n == 4) {
                *reinterpret_cast<int4*>(rank_map + p0) = make_int4(row[0], row[1], row[2], row[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < n) rank_map[p0 + k] = row[k];
            }
        }
    }
    __syncthreads();

    // rows [base, base + tile_n) of the outputs, as far as they lie below capacity
    const long long room = capacity - base;
    const int rows = room <= 0 ? 0 : (room < tile_n ? (int)room : tile_n);
    store_run<4>(s_xyz, xyz_out, xyz_shift, 12 * rows);
    if constexpr (COLORS == 1) store_run<4>(s_rgb, rgb_out, rgb_shift, 12 * rows);
    if constexpr (COLORS == 2) store_run<1>(s_rgb, rgb_out, rgb_shift, 3 * rows);
    if (index) store_run<4>(s_idx, idx_out, idx_shift, 4 * rows);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

size_t point_cloud_workspace_bytes(long long total) {
    const size_t tiles = (size_t)((total + kPointCloudTile - 1) / kPointCloudTile);
    return ((tiles * sizeof(int) + 255) & ~(size_t)255) + 256;
}

int launch_compaction_scan(const char* name, int* tiles, int count, int* offsets, int batch, hipStream_t s) {
    const int probe = probe_before(name, s);
    hipLaunchKernelGGL(point_cloud_scan_kernel, dim3(1), dim3(kPcScanThreads), 0, s, tiles, count, offsets, batch);
    probe_after(probe, 1, s);
    return check_launch(name);
}

int launch_point_cloud_ranked(const ReprojectArgs& r, float min_depth, float max_depth, const float* disparity,
                              const unsigned char* valid, const float* confidence, const void* image, int image_layout,
                              float* points, void* colors, int* index, int* offsets, long long capacity, int batch,
                              int h, int w, void* workspace, int* rank_map, hipStream_t s) {
    const int total = batch * h * w;
    const int tiles = (int)(((long long)total + kPointCloudTile - 1) / kPointCloudTile);
    int* tile_words = static_cast<int*>(workspace);
    PointCloudArgs a;
    a.r = r;
    a.min_depth = min_depth;
    a.max_depth = max_depth;
    const bool vec = aligned16(disparity);

    int probe = probe_before("point_cloud_count", s);
    if (vec)
        hipLaunchKernelGGL(point_cloud_count_kernel<true>, dim3(tiles), dim3(kPcThreads), 0, s, a, disparity, valid,
                           confidence, tile_words, total, h, w);
    else
        hipLaunchKernelGGL(point_cloud_count_kernel<false>, dim3(tiles), dim3(kPcThreads), 0, s, a, disparity, valid,
                           confidence, tile_words, total, h, w);
    probe_after(probe, tiles, s);
    if (int rc = check_launch("point_cloud_count")) return rc;

    if (int rc = launch_compaction_scan("point_cloud_scan", tile_words, tiles, offsets, batch, s)) return rc;

    const int mode = colors ? (image_layout == 1 ? 2 : 1) : 0;
    probe = probe_before("point_cloud_scatter", s);
#define PDS_SCATTER(V, C)                                                                                              \
    do {                                                                                                               \
        if (rank_map)                                                                                                  \
            hipLaunchKernelGGL((point_cloud_scatter_kernel<V, C, true>), dim3(tiles), dim3(kPcThreads), 0, s, a,      \
                               disparity, valid, confidence, image, tile_words, points, colors, index, offsets,        \
                               capacity, batch, total, h, w, rank_map);                                                \
        else                                                                                                           \
            hipLaunchKernelGGL((point_cloud_scatter_kernel<V, C, false>), dim3(tiles), dim3(kPcThreads), 0, s, a,     \
                               disparity, valid, confidence, image, tile_words, points, colors, index, offsets,        \
                               capacity, batch, total, h, w, nullptr);                                                 \
    } while (0)
    if (vec) {
        if (mode == 0) PDS_SCATTER(true, 0);
        else if (mode == 1) PDS_SCATTER(true, 1);
        else PDS_SCATTER(true, 2);
    } else {
        if (mode == 0) PDS_SCATTER(false, 0);
        else if (mode == 1) PDS_SCATTER(false, 1);
        else PDS_SCATTER(false, 2);
    }
#undef PDS_SCATTER
    probe_after(probe, tiles, s);
    return check_launch("point_cloud_scatter");
}

int launch_point_cloud(const ReprojectArgs& r, float min_depth, float max_depth, const float* disparity,
                       const unsigned char* valid, const float* confidence, const void* image, int image_layout,
                       float* points, void* colors, int* index, int* offsets, long long capacity, int batch, int h, int w,
                       void* workspace, hipStream_t s) {
    return launch_point_cloud_ranked(r, min_depth, max_depth, disparity, valid, confidence, image, image_layout, points,
                                     colors, index, offsets, capacity, batch, h, w, workspace, nullptr, s);
}

}  // namespace pds
