// Packed, coloured point cloud (pds_point_cloud_fwd; not in the reference): an ordered stream compaction fused with the
// reprojection and the colour gather.  The kept pixels of `reproject` are written packed, in raster order within a
// batch entry and the entries in batch order, with their colours, their pixel indices and the offsets of the entries.
//
// A pixel is kept iff the point reproject_one (reproject.hpp, the function behind pds_reproject_fwd) gives for it has an
// x that is not NaN -- the pixels a caller's ~isnan(points[..., 0]) keeps of the dense output -- and its depth lies in
// [min_depth, max_depth] (a bound of -inf / +inf is absent).  The packed xyz are that function's result, bit for bit.
//
// Three launches on the caller's stream, an ordered compaction on the scaffold of compaction.hpp (the tile, the ranks, the
// staged runs and the three rules -- integer-only order, no workgroup waits on another, `capacity` -- are stated there):
//   count    one workgroup per tile of kPointCloudTile = 1024 flat pixels (batch * h * w taken as one row of pixels),
//            four pixels per thread from one float4 of disparity; wave64 __ballot + popcount; one int per tile
//   scan     ONE workgroup of 1024 threads turns the tile counts into exclusive offsets in place, 1024 tiles at a time
//            with a carry (any number of tiles), and writes offsets[0] = 0 and offsets[batch] = the TRUE total
//   scatter  per tile again: the predicate is evaluated a second time, the rank of a kept pixel within its tile is
//            mbcnt over the four ballots + the wave prefix + the kept pixels before it in its own quad; xyz, rgb and the
//            pixel index are staged at their rank and leave as runs.  The thread that owns the first pixel of batch
//            entry b = 1 .. batch - 1 writes offsets[b].
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
    const int n = tile_quad(total, blockIdx.x, p0);
    float d[4];
    load_quad<VEC>(disparity, p0, n, 0.f, d);
    int count = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        bool keep = false;
        if (k < n) keep = kept(a, reproject_one(a.r, valid, confidence, p0 + k, d[k], h, w));
        count += __popcll(__ballot(keep));
    }
    store_tile_count(count, wave_total, &tile_count[blockIdx.x]);
}

// ---------------------------------------------------------------------------------------------- scan
// tiles[i]: the count of tile i on entry, the number of kept pixels in the tiles before it on exit
__global__ __launch_bounds__(kPcScanThreads) void point_cloud_scan_kernel(int* __restrict__ tiles, int count,
                                                                          int* __restrict__ offsets, int batch) {
    __shared__ int scan_sums[kPcScanWaves];
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
        if (lane == 63) scan_sums[wave] = inclusive;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < kPcScanWaves; ++k) {
            const int s = scan_sums[k];
            before += k < wave ? s : 0;
            all += s;
        }
        if (i < count) tiles[i] = carry + before + inclusive - v;
        carry += all;
        __syncthreads();   // (scan_sums is written again by the next 1024 tiles)
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
    const StagedRun<float> xyz(s_xyz, points, 3, base);
    const StagedRun<std::conditional_t<COLORS == 2, unsigned char, float>> rgb(s_rgb, colors, 3, base);
    const StagedRun<int> idx(s_idx, index, 1, base);

    int p0;
    const int n = tile_quad(total, blockIdx.x, p0);
    float d[4];
    load_quad<VEC>(disparity, p0, n, 0.f, d);
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
        before += lower_lanes(ballot);
        wave_n += __popcll(ballot);
    }
    int tile_n;
    int rank = tile_ranks(before, wave_n, wave_total, tile_n);

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
                    float* point = xyz.at(rank);
                    point[0] = q[k].x;
                    point[1] = q[k].y;
                    point[2] = q[k].z;
                    if constexpr (COLORS == 1) {
                        const float* src = static_cast<const float*>(image) + (size_t)b * 3 * hw + pixel;
                        float* color = rgb.at(rank);
                        color[0] = src[0];
                        color[1] = src[hw];
                        color[2] = src[2 * (size_t)hw];
                    } else if constexpr (COLORS == 2) {
                        const unsigned char* src = static_cast<const unsigned char*>(image) + 3 * (size_t)(p0 + k);
                        unsigned char* color = rgb.at(rank);
                        color[0] = src[0];
                        color[1] = src[1];
                        color[2] = src[2];
                    }
                    if (index) *idx.at(rank) = pixel;
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

    const int rows = rows_below(capacity, base, tile_n);
    xyz.store(rows);
    if constexpr (COLORS != 0) rgb.store(rows);
    if (index) idx.store(rows);
}

// The scatter form of (VEC, RANKS) for colour mode 0, 1 or 2
template <bool VEC, bool RANKS>
auto scatter_form(int mode) {
    return mode == 0   ? point_cloud_scatter_kernel<VEC, 0, RANKS>
           : mode == 1 ? point_cloud_scatter_kernel<VEC, 1, RANKS>
                       : point_cloud_scatter_kernel<VEC, 2, RANKS>;
}

}  // namespace

size_t point_cloud_workspace_bytes(long long total) {
    return round_up_256((size_t)compaction_tiles(total) * sizeof(int)) + 256;
}

int launch_compaction_scan(const char* name, int* tiles, int count, int* offsets, int batch, hipStream_t s) {
    return launch_probed(name, point_cloud_scan_kernel, 1, kPcScanThreads, s, tiles, count, offsets, batch);
}

int launch_point_cloud_ranked(const ReprojectArgs& r, float min_depth, float max_depth, const float* disparity,
                              const unsigned char* valid, const float* confidence, const void* image, int image_layout,
                              float* points, void* colors, int* index, int* offsets, long long capacity, int batch,
                              int h, int w, void* workspace, int* rank_map, hipStream_t s) {
    const int total = batch * h * w;
    const int tiles = compaction_tiles(total);
    int* tile_words = static_cast<int*>(workspace);
    PointCloudArgs a;
    a.r = r;
    a.min_depth = min_depth;
    a.max_depth = max_depth;
    const bool vec = aligned16(disparity);

    if (int rc = launch_probed("point_cloud_count", vec ? point_cloud_count_kernel<true> : point_cloud_count_kernel<false>,
                               tiles, kPcThreads, s, a, disparity, valid, confidence, tile_words, total, h, w))
        return rc;
    if (int rc = launch_compaction_scan("point_cloud_scan", tile_words, tiles, offsets, batch, s)) return rc;

    const int mode = colors ? (image_layout == 1 ? 2 : 1) : 0;
    const auto scatter = vec ? (rank_map ? scatter_form<true, true>(mode) : scatter_form<true, false>(mode))
                             : (rank_map ? scatter_form<false, true>(mode) : scatter_form<false, false>(mode));
    return launch_probed("point_cloud_scatter", scatter, tiles, kPcThreads, s, a, disparity, valid, confidence, image,
                         tile_words, points, colors, index, offsets, capacity, batch, total, h, w, rank_map);
}

int launch_point_cloud(const ReprojectArgs& r, float min_depth, float max_depth, const float* disparity,
                       const unsigned char* valid, const float* confidence, const void* image, int image_layout,
                       float* points, void* colors, int* index, int* offsets, long long capacity, int batch, int h, int w,
                       void* workspace, hipStream_t s) {
    return launch_point_cloud_ranked(r, min_depth, max_depth, disparity, valid, confidence, image, image_layout, points,
                                     colors, index, offsets, capacity, batch, h, w, workspace, nullptr, s);
}

}  // namespace pds
