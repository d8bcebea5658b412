// Triangle mesh from disparity (pds_triangle_mesh_fwd; not in the reference): the packed cloud of point_cloud.hip as the
// vertices, and up to two triangles per 2 x 2 cell of the pixel grid as the faces, cut wherever a depth edge runs through
// the cell.  include/pds_hip.h holds the table (corners a b / c e, the diagonal, the candidates, the winding).
//
// Every output is an integer or a bit-copy.  Two kept pixels are joined iff fabsf(D[p] - D[q]) <= max_difference: one
// fp32 subtraction of the input disparities, the rule of surface_normals.hip.  Faces are ordered by the flat index of
// their corner a, the first candidate of a cell before the second; integer arithmetic only in the ordering.
//
// Six launches on the caller's stream, two ordered compactions on the scaffold of compaction.hpp (its three rules --
// integer-only order, no workgroup waits on another, `capacity` -- are stated there):
//   vertices      launch_point_cloud_ranked: the three launches of point_cloud.hip; its scatter also writes the dense
//                 rank map (int32 per pixel: the packed row, or -1 where the pixel is not kept) into the workspace
//   face count    one workgroup of 256 threads per tile of kPointCloudTile = 1024 flat pixels, the pixel being corner a
//                 of its cell.  D and the rank map of [t0, t0 + 1025) and of the row below, [t0 + w, t0 + w + 1025), are
//                 staged in LDS once (coalesced 4-byte loads: t0 + w has any alignment, and so may the disparity
//                 pointer -- there is no vector form to choose), each corner is then read from LDS.  0, 1 or 2 faces per
//                 anchor, four anchors per thread: eight ballots and popcounts
//   scan          the scan kernel of point_cloud.hip over the face counts; it writes face_offsets[0] and
//                 face_offsets[batch], the TRUE total
//   face scatter  the predicate again; the rank of a face within its tile is mbcnt over the eight ballots + the wave
//                 prefix + the faces before it in the thread's own quad; the 12-byte records are staged at their rank
//                 and leave as one run per tile.  The thread that owns the first pixel of entry b writes face_offsets[b].
//
// Resources, from the compiler's own output for gfx950 (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   face count    20 VGPRs, 38 SGPRs, 16 464 bytes of LDS, 8 waves per SIMD, no scratch
//   face scatter  50 VGPRs, 48 SGPRs, 41 056 bytes of LDS (three workgroups per CU: 3 waves per SIMD), no scratch
//   the scatter of point_cloud.hip with the rank map: 28 to 38 VGPRs and 78 to 82 SGPRs over its six forms, at most 2
//   VGPRs more than the form without (30 -> 32 and 28 -> 30 in the two scalar-load forms), the same LDS (16 432, 28 736
//   and 19 520 bytes without, with float and with uint8 colours: 8, 5 and 8 waves per SIMD), no scratch
#include "compaction.hpp"

namespace pds {

namespace {

constexpr int kTmStage = kPointCloudTile + 4;   // pixels staged per row: the tile and the corner right of its last pixel

struct MeshArgs {
    float max_difference;
    int flip;
    int total, h, w;
};

struct CellRows {
    float d[2][kTmStage];   // [0]: the tile's pixels, [1]: the pixels one row below them
    int r[2][kTmStage];     // their packed rows, -1: not kept (or beyond the last pixel)
};

// D and the rank map of [t0, t0 + T] and [t0 + w, t0 + w + T] into LDS, by the whole workgroup
__device__ __forceinline__ void stage_rows(CellRows& s, const MeshArgs& a, const float* __restrict__ disparity,
                                           const int* __restrict__ rank_map, long long t0) {
    for (int i = threadIdx.x; i <= kPointCloudTile; i += kPcThreads) {
#pragma unroll
        for (int row = 0; row < 2; ++row) {
            const long long p = t0 + i + (row ? a.w : 0);
            int r = -1;
            float d = 0.f;
            if (p < a.total) {
                r = rank_map[p];
                d = disparity[p];
            }
            s.r[row][i] = r;
            s.d[row][i] = d;
        }
    }
}

__device__ __forceinline__ bool joined(float p, float q, float max_difference) { return fabsf(p - q) <= max_difference; }

// The faces of the cell whose corner a is staged at i (the caller knows that the cell exists): their number, and with
// EMIT their vertices (packed rows) in the order of the table
template <bool EMIT>
__device__ __forceinline__ int cell_faces(const CellRows& s, int i, const MeshArgs& m, int (&f)[2][3]) {
    const int ra = s.r[0][i], rb = s.r[0][i + 1], rc = s.r[1][i], re = s.r[1][i + 1];
    const bool ka = ra >= 0, kb = rb >= 0, kc = rc >= 0, ke = re >= 0;
    const int kept = (int)ka + (int)kb + (int)kc + (int)ke;
    if (kept < 3) return 0;
    const float da = s.d[0][i], db = s.d[0][i + 1], dc = s.d[1][i], de = s.d[1][i + 1];
    const float t = m.max_difference;
    // four corners: the diagonal with the smaller difference, b-c on a tie; three: the one that avoids the missing corner
    const bool diagonal_ae = kept == 4 ? fabsf(da - de) < fabsf(db - dc) : !(kb && kc);
    // the two candidates of that diagonal (every index into f is a constant: nothing is spilled)
    bool first, second;
    int v0, v1, v2, u0, u1, u2;
    if (diagonal_ae) {
        const bool diagonal = ka && ke && joined(da, de, t);
        first = diagonal && kc && joined(da, dc, t) && joined(dc, de, t);    // (a, c, e)
        second = diagonal && kb && joined(de, db, t) && joined(da, db, t);   // (a, e, b)
        v0 = ra, v1 = rc, v2 = re;
        u0 = ra, u1 = re, u2 = rb;
    } else {
        const bool diagonal = kb && kc && joined(db, dc, t);
        first = diagonal && ka && joined(da, dc, t) && joined(da, db, t);    // (a, c, b)
        second = diagonal && ke && joined(dc, de, t) && joined(db, de, t);   // (b, c, e)
        v0 = ra, v1 = rc, v2 = rb;
        u0 = rb, u1 = rc, u2 = re;
    }
    if (EMIT) {
        f[0][0] = first ? v0 : u0, f[0][1] = first ? v1 : u1, f[0][2] = first ? v2 : u2;
        f[1][0] = u0, f[1][1] = u1, f[1][2] = u2;
    }
    return (int)first + (int)second;
}

// The four anchors of this thread: faces per anchor (0 where the pixel does not exist or is in the last column or the
// last row of its entry), and with EMIT their vertices.  -> x, y of the first anchor (for the owner of an entry's start)
template <bool EMIT>
__device__ __forceinline__ void quad_faces(const CellRows& s, const MeshArgs& m, long long t0, int (&n)[4],
                                           int (&f)[4][2][3], int& x0, int& y0) {
    const int i0 = 4 * (int)threadIdx.x;
    const int p0 = (int)t0 + i0;   // (below total + T: it fits)
    int x = p0 % m.w, y = (p0 / m.w) % m.h;
    x0 = x;
    y0 = y;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        n[k] = 0;
        if (p0 + k < m.total && x < m.w - 1 && y < m.h - 1) n[k] = cell_faces<EMIT>(s, i0 + k, m, f[k]);
        if (++x == m.w) {
            x = 0;
            if (++y == m.h) y = 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------- face count
__global__ __launch_bounds__(kPcThreads) void triangle_mesh_face_count_kernel(MeshArgs m,
                                                                              const float* __restrict__ disparity,
                                                                              const int* __restrict__ rank_map,
                                                                              int* __restrict__ tile_count) {
    __shared__ CellRows s;
    __shared__ int wave_total[kPcWaves];
    const long long t0 = (long long)blockIdx.x * kPointCloudTile;
    stage_rows(s, m, disparity, rank_map, t0);
    __syncthreads();
    int n[4], f[4][2][3], x0, y0;
    quad_faces<false>(s, m, t0, n, f, x0, y0);
    int count = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) count += __popcll(__ballot(n[k] >= 1)) + __popcll(__ballot(n[k] == 2));
    store_tile_count(count, wave_total, &tile_count[blockIdx.x]);
}

// ---------------------------------------------------------------------------------------------- face scatter
__global__ __launch_bounds__(kPcThreads) void triangle_mesh_face_scatter_kernel(
    MeshArgs m, const float* __restrict__ disparity, const int* __restrict__ rank_map,
    const int* __restrict__ tile_offset, int* __restrict__ faces, int* __restrict__ face_offsets,
    long long face_capacity) {
    constexpr int T = kPointCloudTile;
    __shared__ CellRows s;
    __shared__ alignas(16) unsigned char s_faces[12 * 2 * T + 16];
    __shared__ int wave_total[kPcWaves];

    const int base = tile_offset[blockIdx.x];   // faces of the tiles before this one
    const StagedRun<int> run(s_faces, faces, 3, base);

    const long long t0 = (long long)blockIdx.x * T;
    stage_rows(s, m, disparity, rank_map, t0);
    __syncthreads();
    int n[4], f[4][2][3], x0, y0;
    quad_faces<true>(s, m, t0, n, f, x0, y0);
    int before = 0, wave_n = 0;   // faces of the lower lanes of this wave; of the whole wave
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long one = __ballot(n[k] >= 1), two = __ballot(n[k] == 2);
        before += lower_lanes(one) + lower_lanes(two);
        wave_n += __popcll(one) + __popcll(two);
    }
    int tile_n;
    int rank = tile_ranks(before, wave_n, wave_total, tile_n);

    const int p0 = (int)t0 + 4 * (int)threadIdx.x;
    int x = x0, y = y0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (p0 + k < m.total) {
            // entry b > 0 begins at this pixel: the faces anchored before it
            if (x == 0 && y == 0 && p0 + k > 0) face_offsets[(p0 + k) / (m.h * m.w)] = base + rank;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j < n[k]) {
                    int* face = run.at(rank);
                    face[0] = f[k][j][0];
                    face[1] = m.flip ? f[k][j][2] : f[k][j][1];
                    face[2] = m.flip ? f[k][j][1] : f[k][j][2];
                    ++rank;
                }
            }
        }
        if (++x == m.w) {
            x = 0;
            if (++y == m.h) y = 0;
        }
    }
    __syncthreads();

    run.store(rows_below(face_capacity, base, tile_n));
}

}  // namespace

// [tile words of the vertices][tile words of the faces][the rank map]
size_t triangle_mesh_workspace_bytes(long long total) {
    return 2 * point_cloud_workspace_bytes(total) + round_up_256((size_t)total * sizeof(int));
}

int launch_triangle_mesh(const ReprojectArgs& r, float min_depth, float max_depth, float max_difference, int flip,
                         const float* disparity, const unsigned char* valid, const float* confidence, const void* image,
                         int image_layout, float* points, void* colors, int* index, int* offsets, long long capacity,
                         int* faces, int* face_offsets, long long face_capacity, int batch, int h, int w,
                         void* workspace, hipStream_t s) {
    const int total = batch * h * w;
    const int tiles = compaction_tiles(total);
    const size_t words = point_cloud_workspace_bytes(total);
    unsigned char* bytes = static_cast<unsigned char*>(workspace);
    int* face_words = reinterpret_cast<int*>(bytes + words);
    int* rank_map = reinterpret_cast<int*>(bytes + 2 * words);

    if (int rc = launch_point_cloud_ranked(r, min_depth, max_depth, disparity, valid, confidence, image, image_layout,
                                           points, colors, index, offsets, capacity, batch, h, w, workspace, rank_map, s))
        return rc;

    MeshArgs m;
    m.max_difference = max_difference;
    m.flip = flip ? 1 : 0;
    m.total = total;
    m.h = h;
    m.w = w;
    if (int rc = launch_probed("triangle_mesh_face_count", triangle_mesh_face_count_kernel, tiles, kPcThreads, s, m,
                               disparity, rank_map, face_words))
        return rc;
    if (int rc = launch_compaction_scan("triangle_mesh_face_scan", face_words, tiles, face_offsets, batch, s)) return rc;
    return launch_probed("triangle_mesh_face_scatter", triangle_mesh_face_scatter_kernel, tiles, kPcThreads, s, m,
                         disparity, rank_map, face_words, faces, face_offsets, face_capacity);
}

}  // namespace pds
