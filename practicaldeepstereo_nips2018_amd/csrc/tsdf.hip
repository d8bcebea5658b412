// TSDF fusion (pds_tsdf_integrate_fwd, pds_tsdf_extract_fwd; not in the reference): disparity maps of a moving rig are
// integrated into one dense truncated-signed-distance volume, and the volume's zero crossings are extracted as a packed
// cloud with normals (KinectFusion; Open3D TSDFVolume.integrate / extract_point_cloud).
//
// The volume: tsdf and weight, float32 [nz, ny, nx], x fastest; voxel v = (k * ny + j) * nx + i.
//
// integrate, per batch entry, two launches on the caller's stream (entry after entry, so the result is that of the
// entries integrated in order):
//   tsdf_depth      per source pixel: Z = reproject_one(...).z (reproject.hpp, the device function behind
//                   pds_reproject_fwd: the same pixels are kept), NaN where the pixel is dropped or Z is not finite and
//                   positive; beside it the pixel's confidence when the weights are taken from it.  One workgroup of 256
//                   threads per 1024 pixels, one float4 of disparity per thread (VEC).
//   tsdf_integrate  per voxel, in fp32 (tsdf_sample below): p_c = A (i, j, k) + b, the projection, the rounding of
//                   pds_register_depth_fwd's splat 1, sdf = Z - z_c, t = min(1, sdf / truncation), the running average.
//                   Whether a voxel is updated does not depend on its old state, and a voxel that is not updated is
//                   neither read nor written: the traffic is that of the updated share of the volume.
//                   Work: the volume as ONE row of nx * ny * nz voxels, cut into quads of four consecutive voxels (x
//                   fastest) that begin on a 16-byte boundary of the state tensors (VEC: both tensors share one
//                   misalignment `shift`, quad q = voxels [4 q - shift, 4 q - shift + 4); the first and the last quad may be
//                   partial).  One quad per thread and step, 256 threads, a grid-stride loop over at most
//                   kTsdfIntegrateMaxGroups workgroups.  A quad whose four voxels are all updated -- the inside of the
//                   band -- is one 16-byte load and store per tensor; a mixed quad -- the rim of the band -- goes voxel by
//                   voxel.  VEC = false (the two tensors disagree in their misalignment): every quad goes voxel by voxel.
//                   No atomics; no workgroup waits on another; each voxel belongs to one thread.
//   Every multiply-add below is an explicit fmaf and contraction is off, so that both forms of a kernel give the same bits.
//
// extract, an ordered compaction on the scaffold of compaction.hpp (the tile, the ranks, the staged runs and the three
// rules are stated there), tiles of kPointCloudTile = 1024 voxels, four consecutive voxels per thread, candidate 3 v + a
// (axis a = 0, 1, 2: the edge from v to its neighbour along +x, +y, +z; direction d = 1 << a of quad_edges):
//   tsdf_extract_count    candidates per tile
//   tsdf_extract_scan     launch_compaction_scan: exclusive offsets of the tiles, offsets[0] = 0, offsets[1] = the TRUE count
//   tsdf_extract_scatter  the candidates are found again, ranked (scan of the threads' counts within a wave), staged and
//                         stored: first points and index, then -- the same LDS again -- the normals.
// Observed (weight >= min_weight), the sign (tsdf < 0) and the order are decided on the stored bits.
#include "tsdf_surface.hpp"

#pragma clang fp contract(off)

namespace pds {

namespace {

constexpr int kTsdfThreads = 256;
static_assert(kTsdfDepthTile == 4 * kTsdfThreads && kTsdfQuadsPerGroup == kTsdfThreads, "one quad per thread");
static_assert(kTsdfDepthTile == kPointCloudTile && kTsdfThreads == kPcThreads, "tsdf_depth takes its quads from tile_quad");

// ---------------------------------------------------------------------------------------------- depth
template <bool VEC>
__global__ __launch_bounds__(kTsdfThreads) void tsdf_depth_kernel(ReprojectArgs r, const float* __restrict__ disparity,
                                                                  const unsigned char* __restrict__ valid,
                                                                  const float* __restrict__ confidence,
                                                                  float* __restrict__ zbuf, float* __restrict__ wbuf,
                                                                  int hw, int h, int w) {
    int p0;
    const int n = tile_quad(hw, blockIdx.x, p0);
    if (n == 0) return;
    float d[4];
    load_quad<VEC>(disparity, p0, n, 0.f, d);
    float z[4], c[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        z[e] = c[e] = __builtin_nanf("");
        if (e < n) {
            const float Z = reproject_one(r, valid, confidence, p0 + e, d[e], h, w).z;
            if (Z > 0.f && Z < __builtin_inff()) z[e] = Z;   // (the NaN of a dropped pixel fails too)
            if (wbuf) c[e] = confidence[p0 + e];
        }
    }
    // (zbuf and wbuf are 16-byte aligned and p0 a multiple of 4)
    if (n == 4) {
        *reinterpret_cast<float4*>(zbuf + p0) = make_float4(z[0], z[1], z[2], z[3]);
        if (wbuf) *reinterpret_cast<float4*>(wbuf + p0) = make_float4(c[0], c[1], c[2], c[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e < n) {
                zbuf[p0 + e] = z[e];
                if (wbuf) wbuf[p0 + e] = c[e];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- integrate
// (tsdf_sample and tsdf_update: tsdf_surface.hpp, shared with tsdf_color.hip)
template <bool VEC, bool CONF>
__global__ __launch_bounds__(kTsdfThreads) void tsdf_integrate_kernel(TsdfIntegrateArgs a,
                                                                      const float* __restrict__ zbuf,
                                                                      const float* __restrict__ wbuf,
                                                                      float* __restrict__ tsdf,
                                                                      float* __restrict__ weight, int nx, int ny,
                                                                      int total, int shift, int quads, int h, int w) {
    for (int q = blockIdx.x * kTsdfThreads + (int)threadIdx.x; q < quads; q += gridDim.x * kTsdfThreads) {
        const int first = 4 * q - shift;   // (3 * total < 2^31: no overflow)
        const int lo = first < 0 ? 0 : first, hi = first + 4 < total ? first + 4 : total;
        // The walk is written out here, not VoxelAt (tsdf_surface.hpp): with it three carries of the kernel were encoded
        // differently and it measured 0.1 to 0.3 us slower in four series (docs/LAB_NOTES.md).  It begins at lo, not at
        // first: the first quad may begin before the volume.
        int i = lo % nx, rest = lo / nx;
        int j = rest % ny, k = rest / ny;
        float t[4], wt[4];
        bool update[4];
        int pixel;   // (where the Z was read: of use to the coloured kernel only)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            update[e] = false;
            if (first + e >= lo && first + e < hi) {
                update[e] = tsdf_sample<CONF>(a, zbuf, wbuf, i, j, k, h, w, t[e], wt[e], pixel);
                if (++i == nx) {
                    i = 0;
                    if (++j == ny) {
                        j = 0;
                        ++k;
                    }
                }
            }
        }
        if (VEC && update[0] && update[1] && update[2] && update[3]) {
            // (all four updated: the quad lies inside the volume, and first is a multiple of 4 behind `shift`)
            float4 value = *reinterpret_cast<const float4*>(tsdf + first);
            float4 held = *reinterpret_cast<const float4*>(weight + first);
            tsdf_update(a.max_weight, t[0], wt[0], value.x, held.x);
            tsdf_update(a.max_weight, t[1], wt[1], value.y, held.y);
            tsdf_update(a.max_weight, t[2], wt[2], value.z, held.z);
            tsdf_update(a.max_weight, t[3], wt[3], value.w, held.w);
            *reinterpret_cast<float4*>(tsdf + first) = value;
            *reinterpret_cast<float4*>(weight + first) = held;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (update[e]) {
                    float value = tsdf[first + e], held = weight[first + e];
                    tsdf_update(a.max_weight, t[e], wt[e], value, held);
                    tsdf[first + e] = value;
                    weight[first + e] = held;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- extract
// (TsdfExtractArgs, VoxelAt, quad_edges, tsdf_gradient and the point and the normal of a crossing: tsdf_surface.hpp,
// shared with tsdf_mesh.hip)
constexpr unsigned kAxisDirs = 0x0b;   // the directions d = 1, 2, 4 of quad_edges: one step along x, y, z

// The leaving extraction (pds_tsdf_extract_leaving_fwd): the same two kernels with Args = TsdfLeavingArgs, which keep of
// quad_edges' result the edges that do not survive a shift of the volume.  The edge from v to n survives iff both v and n
// land inside the shifted volume: `lands` holds, per axis, the range of the voxels that do (tsdf_shift_range of the
// input).  With Args = TsdfExtractArgs, the default, nothing of this is compiled: pds_tsdf_extract_fwd keeps its code.
struct TsdfLeavingArgs : TsdfExtractArgs {
    TsdfShiftRange lands;
};

// bit 8 e + d - 1 (d = 1, 2, 4) = the edge from voxel e of the quad [at, at + n) along d does not survive
__device__ __forceinline__ unsigned leaving_edges(const TsdfShiftRange& r, VoxelAt at, int n, int nx, int ny) {
    unsigned mask = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (e < n) {
            const int c[3] = {at.i, at.j, at.k};
            bool lands = true, next[3];
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                lands = lands && c[m] >= r.lo[m] && c[m] < r.hi[m];
                next[m] = c[m] + 1 < r.hi[m];   // (the neighbour along m differs from the voxel in c[m] alone)
            }
#pragma unroll
            for (int m = 0; m < 3; ++m)
                if (!(lands && next[m])) mask |= 1u << (8 * e + (1 << m) - 1);
            at.next(nx, ny);
        }
    }
    return mask;
}

template <bool VEC, class Args = TsdfExtractArgs>
__global__ __launch_bounds__(kPcThreads) void tsdf_extract_count_kernel(Args a,
                                                                        const float* __restrict__ tsdf,
                                                                        const float* __restrict__ weight,
                                                                        int* __restrict__ tile_count) {
    __shared__ int wave_total[kPcWaves];
    int v0;
    float value[4];
    VoxelAt at;
    const int n = tile_quad(a.total, blockIdx.x, v0);
    unsigned packed = quad_edges<VEC, kAxisDirs>(a, tsdf, weight, v0, n, value, at);
    if constexpr (std::is_same<Args, TsdfLeavingArgs>::value) packed &= leaving_edges(a.lands, at, n, a.nx, a.ny);
    const int mine = __popc(packed);
    store_tile_count(wave_count(mine), wave_total, &tile_count[blockIdx.x]);
}

template <bool VEC, class Args = TsdfExtractArgs>
__global__ __launch_bounds__(kPcThreads) void tsdf_extract_scatter_kernel(
    Args a, const float* __restrict__ tsdf, const float* __restrict__ weight,
    const int* __restrict__ tile_offset, float* __restrict__ points, float* __restrict__ normals,
    int* __restrict__ index, long long capacity) {
    constexpr int kMost = 3 * kPointCloudTile;   // candidates of one tile
    __shared__ alignas(16) unsigned char s_rec[12 * kMost + 16];   // the points, then the normals
    __shared__ alignas(16) unsigned char s_idx[4 * kMost + 16];
    __shared__ int wave_total[kPcWaves];

    const int base = tile_offset[blockIdx.x];   // surface points in the tiles before this one
    int v0;
    float value[4];
    VoxelAt at0;
    const int n = tile_quad(a.total, blockIdx.x, v0);
    unsigned packed = quad_edges<VEC, kAxisDirs>(a, tsdf, weight, v0, n, value, at0);
    if constexpr (std::is_same<Args, TsdfLeavingArgs>::value) packed &= leaving_edges(a.lands, at0, n, a.nx, a.ny);
    const int mine = __popc(packed), before = wave_exclusive(mine);
    int tile_n;
    const int first_rank = tile_ranks(before, before + mine, wave_total, tile_n);
    if (tile_n == 0) return;   // (the whole workgroup: most tiles of a volume hold no surface)
    const int rows = rows_below(capacity, base, tile_n);
    if (rows == 0) return;
    const int stride[3] = {1, a.nx, a.nx * a.ny};

    for (int pass = 0; pass < (normals ? 2 : 1); ++pass) {
        const StagedRun<float> rec(s_rec, pass == 0 ? points : normals, 3, base);
        const StagedRun<int> idx(s_idx, index, 1, base);
        int rank = first_rank;
        VoxelAt at = at0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e < n) {
                const int v = v0 + e;
#pragma unroll
                for (int axis = 0; axis < 3; ++axis) {
                    const int d = 1 << axis;
                    if (packed >> (8 * e + d - 1) & 1) {
                        const int nb = v + stride[axis];
                        const float r = value[e] / (value[e] - tsdf[nb]);   // (signs differ: the difference is not 0)
                        if (pass == 0) {
                            tsdf_surface_point(a, at.i, at.j, at.k, d, r, rec.at(rank));
                            if (index) *idx.at(rank) = 3 * v + axis;
                        } else {
                            tsdf_surface_normal(a, tsdf, weight, v, nb, at.i, at.j, at.k, d, r, rec.at(rank));
                        }
                        ++rank;
                    }
                }
                at.next(a.nx, a.ny);
            }
        }
        __syncthreads();
        rec.store(rows);
        if (pass == 0 && index) idx.store(rows);
        __syncthreads();   // (s_rec is written again by the normals)
    }
}

}  // namespace

size_t tsdf_integrate_workspace_bytes(long long pixels) {
    return 2 * round_up_256((size_t)pixels * sizeof(float));
}

int tsdf_integrate_groups(long long voxels, int shift) {
    const long long quads = (voxels + shift + 3) / 4;
    const long long groups = (quads + kTsdfQuadsPerGroup - 1) / kTsdfQuadsPerGroup;
    return (int)(groups < kTsdfIntegrateMaxGroups ? groups : kTsdfIntegrateMaxGroups);
}

int launch_tsdf_depth(const ReprojectArgs& r, const float* disparity, const unsigned char* valid,
                      const float* confidence, float* zbuf, float* wbuf, int h, int w, hipStream_t s) {
    return launch_probed("tsdf_depth", aligned16(disparity) ? tsdf_depth_kernel<true> : tsdf_depth_kernel<false>,
                         compaction_tiles(h * w), kTsdfThreads, s, r, disparity, valid, confidence, zbuf, wbuf, h * w, h,
                         w);
}

int launch_tsdf_integrate(const ReprojectArgs& r, const TsdfIntegrateArgs& args, const float* transforms,
                          int weight_by_confidence, const float* disparity, const unsigned char* valid, const float* confidence, float* tsdf,
                          float* weight, int nx, int ny, int nz, int batch, int h, int w, void* workspace,
                          hipStream_t s) {
    const int hw = h * w, total = nx * ny * nz;
    float* zbuf = static_cast<float*>(workspace);
    float* wbuf = weight_by_confidence ? zbuf + tsdf_integrate_workspace_bytes(hw) / (2 * sizeof(float)) : nullptr;
    // quads begin on a 16-byte boundary of both tensors where the two agree in their misalignment
    const bool vec = (((uintptr_t)tsdf ^ (uintptr_t)weight) & 15u) == 0;
    const int shift = vec ? (int)(((uintptr_t)tsdf & 15u) / sizeof(float)) : 0;
    const int quads = (int)(((long long)total + shift + 3) / 4);
    const int groups = tsdf_integrate_groups(total, shift);
    const auto integrate = vec ? (wbuf ? tsdf_integrate_kernel<true, true> : tsdf_integrate_kernel<true, false>)
                               : (wbuf ? tsdf_integrate_kernel<false, true> : tsdf_integrate_kernel<false, false>);
    for (int b = 0; b < batch; ++b) {
        const float* d = disparity + (size_t)b * hw;
        const unsigned char* ok = valid ? valid + (size_t)b * hw : nullptr;
        const float* c = confidence ? confidence + (size_t)b * hw : nullptr;
        TsdfIntegrateArgs a = args;
        for (int k = 0; k < 12; ++k) (k < 9 ? a.A[k] : a.b[k - 9]) = transforms[12 * (size_t)b + k];
        if (int rc = launch_tsdf_depth(r, d, ok, c, zbuf, wbuf, h, w, s)) return rc;
        if (int rc = launch_probed("tsdf_integrate", integrate, groups, kTsdfThreads, s, a, zbuf, wbuf, tsdf, weight, nx,
                                   ny, total, shift, quads, h, w))
            return rc;
    }
    return 0;
}

size_t tsdf_extract_workspace_bytes(long long voxels) { return point_cloud_workspace_bytes(voxels); }

static TsdfExtractArgs extract_args(const float* origin, float voxel_size, float min_weight, int nx, int ny, int nz) {
    TsdfExtractArgs a;
    for (int m = 0; m < 3; ++m) a.origin[m] = origin[m];
    a.voxel_size = voxel_size;
    a.min_weight = min_weight;
    a.nx = nx;
    a.ny = ny;
    a.nz = nz;
    a.total = nx * ny * nz;
    return a;
}

int launch_tsdf_extract(const float* tsdf, const float* weight, const float* origin, float voxel_size,
                        float min_weight, float* points, float* normals, int* index, int* offsets, long long capacity,
                        int nx, int ny, int nz, void* workspace, hipStream_t s) {
    const TsdfExtractArgs a = extract_args(origin, voxel_size, min_weight, nx, ny, nz);
    const int tiles = compaction_tiles(a.total);
    int* tile_words = static_cast<int*>(workspace);
    const bool vec = aligned16(tsdf) && aligned16(weight);

    if (int rc = launch_probed("tsdf_extract_count", vec ? tsdf_extract_count_kernel<true> : tsdf_extract_count_kernel<false>,
                               tiles, kPcThreads, s, a, tsdf, weight, tile_words))
        return rc;
    if (int rc = launch_compaction_scan("tsdf_extract_scan", tile_words, tiles, offsets, 1, s)) return rc;
    return launch_probed("tsdf_extract_scatter",
                         vec ? tsdf_extract_scatter_kernel<true> : tsdf_extract_scatter_kernel<false>, tiles,
                         kPcThreads, s, a, tsdf, weight, tile_words, points, normals, index, capacity);
}

int launch_tsdf_extract_leaving(const float* tsdf, const float* weight, const float* origin, float voxel_size,
                                float min_weight, const int* delta, float* points, float* normals, int* index,
                                int* offsets, long long capacity, int nx, int ny, int nz, void* workspace,
                                hipStream_t s) {
    TsdfLeavingArgs a;
    static_cast<TsdfExtractArgs&>(a) = extract_args(origin, voxel_size, min_weight, nx, ny, nz);
    a.lands = tsdf_shift_range(nx, ny, nz, delta, false);
    const int tiles = compaction_tiles(a.total);
    int* tile_words = static_cast<int*>(workspace);
    const bool vec = aligned16(tsdf) && aligned16(weight);

    if (int rc = launch_probed("tsdf_extract_leaving_count",
                               vec ? tsdf_extract_count_kernel<true, TsdfLeavingArgs>
                                   : tsdf_extract_count_kernel<false, TsdfLeavingArgs>,
                               tiles, kPcThreads, s, a, tsdf, weight, tile_words))
        return rc;
    if (int rc = launch_compaction_scan("tsdf_extract_leaving_scan", tile_words, tiles, offsets, 1, s)) return rc;
    return launch_probed("tsdf_extract_leaving_scatter",
                         vec ? tsdf_extract_scatter_kernel<true, TsdfLeavingArgs>
                             : tsdf_extract_scatter_kernel<false, TsdfLeavingArgs>,
                         tiles, kPcThreads, s, a, tsdf, weight, tile_words, points, normals, index, capacity);
}

}  // namespace pds
