// TSDF mesh (pds_tsdf_mesh_fwd; not in the reference): the surface of the volume of tsdf.hip as a closed triangle mesh, by
// marching tetrahedra on the Kuhn triangulation of each cell (six tetrahedra around the body diagonal).  Sixteen sign
// cases per tetrahedron; neighbouring cells agree on the diagonal of every shared face, so the mesh is closed wherever
// the volume is observed.  include/pds_hip.h holds the contract (edges, vertices, cells, cases, winding, order).
//
// Six launches on the caller's stream, two ordered compactions on the scaffold of compaction.hpp (the tile, the ranks, the
// staged runs and the three rules are stated there): tiles of kPointCloudTile = 1024 flat voxels, four consecutive voxels
// per thread, at most kTsdfMeshMaxGroups workgroups that stride over the tiles beyond (hence a barrier behind each tile).
//   tsdf_mesh_count         per voxel the mask of its seven edge directions d = 1 .. 7 that carry a vertex (both ends
//                           observed, signs differ: decided on the stored bits); vertices per tile
//   tsdf_mesh_scan          launch_compaction_scan: exclusive offsets of the tiles, offsets[1] = the TRUE count
//   tsdf_mesh_scatter       the masks again (quad_edges, tsdf_surface.hpp), ranked (scan within a wave).  Per voxel the record
//                           goes to the workspace: the row of its first vertex (one 16-byte store per thread) and its
//                           mask (one 4-byte store per thread), whatever the capacity.  The vertices are staged in LDS at
//                           their rank, kMeshChunk rows at a time, and stored as contiguous runs (store_run): points and
//                           index, then -- the same LDS again -- the normals, by the device functions of tsdf.hip's scatter
//                           (tsdf_surface.hpp).  Only rows below `capacity`.
//   tsdf_mesh_face_count    a voxel is corner 0 of its cell.  Per voxel of [t0, t0 + 1024] and of the three rows beside it
//                           (+y, +z, +y+z) two bits, observed and negative, are staged in LDS once; a cell reads its eight
//                           corners from there.  A tetrahedron with four observed corners has 0, 1 or 2 faces by the
//                           number of negative corners; faces per tile
//   tsdf_mesh_face_scan     the scan over the face counts, face_offsets[1] = the TRUE count
//   tsdf_mesh_face_scatter  the counts again, ranked; where a tile has faces, the records of the same four rows are staged
//                           beside the bits, and a vertex of edge (v, d) is row first[v] + popc(mask[v] & ((1 << (d - 1))
//                           - 1)).  The faces are staged at their rank, kMeshChunk rows at a time, and leave through
//                           store_run.  Nothing here compares floating-point numbers but `observed` and the sign.
// The case table (which edges, in which order), the corners of the tetrahedra and the winding bits are computed at compile
// time from the rule itself (tet_case, tet_corner, tet_flip: integer geometry on edge midpoints), not transcribed.
// Not measured: LDS bank conflicts of the quad reads (one 16-byte read and one 4-byte read per row and thread), occupancy.
#include "tsdf_surface.hpp"

#pragma clang fp contract(off)

namespace pds {

namespace {

constexpr int kMeshChunk = 2048;                      // rows of an output staged in LDS at a time
constexpr int kMeshStage = kPointCloudTile + 4;       // voxels staged per row: the tile and the corner beyond its last one
static_assert(kMeshStage % 4 == 0, "rows of 16-byte units");

// ---------------------------------------------------------------------------------------------- the tables
constexpr int kTetAxes[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

// corner (a mask of three offset bits) at position m = 0 .. 3 of tetrahedron t
constexpr int tet_corner(int t, int m) {
    return m == 0 ? 0 : m == 1 ? 1 << kTetAxes[t][0] : m == 2 ? (1 << kTetAxes[t][0]) | (1 << kTetAxes[t][1]) : 7;
}

// an edge between the positions p and q of a tetrahedron: four bits, the lower position first
constexpr unsigned tet_edge(int p, int q) { return p < q ? (unsigned)(p << 2 | q) : (unsigned)(q << 2 | p); }

// The faces of the sign pattern s (bit m: the corner at position m is negative): bits 0-1 their number, then four bits
// per vertex, three vertices per face
constexpr unsigned tet_case(int s) {
    int negative[4] = {}, positive[4] = {}, nn = 0, np = 0;
    for (int m = 0; m < 4; ++m) {
        if (s >> m & 1) negative[nn++] = m;
        else positive[np++] = m;
    }
    if (nn == 0 || np == 0) return 0;
    unsigned v[6] = {};
    int faces = 1;
    if (nn == 1 || np == 1) {
        const int A = nn == 1 ? negative[0] : positive[0];
        const int* rest = nn == 1 ? positive : negative;   // B < C < D
        for (int j = 0; j < 3; ++j) v[j] = tet_edge(A, rest[j]);
    } else {
        const int A = negative[0], B = negative[1], C = positive[0], D = positive[1];
        v[0] = tet_edge(A, C), v[1] = tet_edge(A, D), v[2] = tet_edge(B, D);
        v[3] = tet_edge(A, C), v[4] = tet_edge(B, D), v[5] = tet_edge(B, C);
        faces = 2;
    }
    unsigned code = (unsigned)faces;
    for (int j = 0; j < 6; ++j) code |= v[j] << (2 + 4 * j);
    return code;
}

// Whether the listed order of the faces of (t, s) has to be reversed: with every vertex at the midpoint of its edge, the
// normal (v1 - v0) x (v2 - v0) of the first face against the vector from the negative corners' centroid to the positive
// corners' (both faces of a two-against-two case lie in one plane and run the same way).  Integers: twice the midpoints.
constexpr bool tet_flip(int t, int s) {
    const unsigned code = tet_case(s);
    if ((code & 3) == 0) return false;
    int mid[3][3] = {};
    for (int j = 0; j < 3; ++j) {
        const int e = code >> (2 + 4 * j) & 15, p = tet_corner(t, e >> 2), q = tet_corner(t, e & 3);
        for (int m = 0; m < 3; ++m) mid[j][m] = (p >> m & 1) + (q >> m & 1);
    }
    int u[3] = {}, w[3] = {};
    for (int m = 0; m < 3; ++m) u[m] = mid[1][m] - mid[0][m], w[m] = mid[2][m] - mid[0][m];
    const int n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
    int nn = 0;
    for (int m = 0; m < 4; ++m) nn += s >> m & 1;
    const int np = 4 - nn;
    // (positive centroid - negative centroid) * nn * np
    int dot = 0;
    for (int m = 0; m < 4; ++m) {
        const int c = tet_corner(t, m), scale = (s >> m & 1) ? -np : nn;
        for (int x = 0; x < 3; ++x) dot += scale * (c >> x & 1) * n[x];
    }
    return dot < 0;
}

struct TetTables {
    unsigned cases[16];    // tet_case
    unsigned corners[6];   // three bits per position
    unsigned flips[6];     // bit s: tet_flip(t, s)
};

constexpr TetTables make_tet_tables() {
    TetTables tables = {};
    for (int s = 0; s < 16; ++s) tables.cases[s] = tet_case(s);
    for (int t = 0; t < 6; ++t) {
        for (int m = 0; m < 4; ++m) tables.corners[t] |= (unsigned)tet_corner(t, m) << (3 * m);
        for (int s = 0; s < 16; ++s) tables.flips[t] |= (unsigned)tet_flip(t, s) << s;
    }
    return tables;
}

constexpr TetTables kTetHost = make_tet_tables();
// All six tetrahedra meet in the body diagonal.  The complement of a pattern has the same faces the other way round: a
// lone corner keeps its listing, so the bit differs; two against two list each other's faces reversed, so the bit agrees.
constexpr bool tet_tables_ok() {
    for (int t = 0; t < 6; ++t) {
        if ((kTetHost.corners[t] & 7) != 0 || (kTetHost.corners[t] >> 9 & 7) != 7) return false;
        for (int s = 1; s < 15; ++s) {
            const bool pair = (kTetHost.cases[s] & 3) == 2;
            if ((tet_flip(t, s) == tet_flip(t, 15 - s)) != pair) return false;
        }
    }
    return true;
}
static_assert(tet_tables_ok(), "the winding table contradicts itself");

__constant__ TetTables kTet = make_tet_tables();

// ---------------------------------------------------------------------------------------------- vertices
// (tile_quad, the ranks and the staged runs: compaction.hpp; VoxelAt and quad_edges: tsdf_surface.hpp)
constexpr unsigned kAllDirs = 0x7f;   // the seven directions d = 1 .. 7 of quad_edges

template <bool VEC>
__global__ __launch_bounds__(kPcThreads) void tsdf_mesh_count_kernel(TsdfExtractArgs a, const float* __restrict__ tsdf,
                                                                     const float* __restrict__ weight,
                                                                     int* __restrict__ tile_count, int tiles) {
    __shared__ int wave_total[kPcWaves];
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        int v0;
        float own[4];   // (own and at: outputs of quad_edges that a count has no use for)
        VoxelAt at;
        const int n = tile_quad(a.total, tile, v0);
        const int mine = __popc(quad_edges<VEC, kAllDirs>(a, tsdf, weight, v0, n, own, at));
        store_tile_count(wave_count(mine), wave_total, &tile_count[tile]);
        __syncthreads();   // (wave_total is written again by the next tile)
    }
}

template <bool VEC>
__global__ __launch_bounds__(kPcThreads) void tsdf_mesh_scatter_kernel(
    TsdfExtractArgs a, const float* __restrict__ tsdf, const float* __restrict__ weight,
    const int* __restrict__ tile_offset, float* __restrict__ points, float* __restrict__ normals,
    int* __restrict__ index, long long capacity, int* __restrict__ first, unsigned char* __restrict__ edge_mask,
    int tiles) {
    __shared__ alignas(16) unsigned char s_rec[12 * kMeshChunk + 16];   // the points, then the normals
    __shared__ alignas(16) unsigned char s_idx[4 * kMeshChunk + 16];
    __shared__ int wave_total[kPcWaves];

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int base = tile_offset[tile];   // vertices in the tiles before this one
        int v0;
        float own[4];   // (not read: the loop over e below is not unrolled, and a dynamic index would spill the array)
        VoxelAt at0;
        const int n = tile_quad(a.total, tile, v0);
        const unsigned packed = quad_edges<VEC, kAllDirs>(a, tsdf, weight, v0, n, own, at0);
        const int mine = __popc(packed), before = wave_exclusive(mine);
        int tile_n;
        const int first_rank = tile_ranks(before, before + mine, wave_total, tile_n);

        // the record of every voxel, whatever the capacity (both arrays are 16-byte aligned and padded beyond `total`)
        if (n > 0) {
            int4 rows;
            rows.x = base + first_rank;
            rows.y = rows.x + __popc(packed & 0xffu);
            rows.z = rows.y + __popc(packed >> 8 & 0xffu);
            rows.w = rows.z + __popc(packed >> 16 & 0xffu);
            *reinterpret_cast<int4*>(first + v0) = rows;
            *reinterpret_cast<unsigned*>(edge_mask + v0) = packed;
        }

        // rows [base, base + tile_n) of the outputs, as far as they lie below capacity, kMeshChunk at a time
        const int rows = rows_below(capacity, base, tile_n);
        const int sy = a.nx, sz = a.nx * a.ny;
        for (int c0 = 0; c0 < rows; c0 += kMeshChunk) {
            const int cn = rows - c0 < kMeshChunk ? rows - c0 : kMeshChunk;
            for (int pass = 0; pass < (normals ? 2 : 1); ++pass) {
                const StagedRun<float> rec(s_rec, pass == 0 ? points : normals, 3, base + c0);
                const StagedRun<int> idx(s_idx, index, 1, base + c0);
                int rank = first_rank - c0;
                VoxelAt at = at0;
                for (int e = 0; e < n; ++e) {
                    unsigned m = packed >> (8 * e) & 0x7fu;
                    const int v = v0 + e;
                    if (m != 0 && rank < cn && rank + __popc(m) > 0) {
                        const float value = tsdf[v];
                        while (m != 0) {
                            const int d = __ffs((int)m);   // 1 .. 7
                            m &= m - 1;
                            if (rank >= 0 && rank < cn) {
                                const int nb = v + (d & 1) + ((d & 2) ? sy : 0) + ((d & 4) ? sz : 0);
                                const float r = value / (value - tsdf[nb]);   // (signs differ: the difference is not 0)
                                if (pass == 0) {
                                    tsdf_surface_point(a, at.i, at.j, at.k, d, r, rec.at(rank));
                                    if (index) *idx.at(rank) = 7 * v + d - 1;
                                } else {
                                    tsdf_surface_normal(a, tsdf, weight, v, nb, at.i, at.j, at.k, d, r, rec.at(rank));
                                }
                            }
                            ++rank;
                        }
                    } else {
                        rank += __popc(m);
                    }
                    at.next(a.nx, a.ny);
                }
                __syncthreads();
                rec.store(cn);
                if (pass == 0 && index) idx.store(cn);
                __syncthreads();   // (s_rec is written again by the normals or the next chunk)
            }
        }
        __syncthreads();   // (wave_total is written again by the next tile)
    }
}

// ---------------------------------------------------------------------------------------------- faces
// Per staged voxel a word: bit 0 observed, bit 1 negative; the scatter adds the edge mask in bits 8 .. 14.
// Row y + 2 z of the corner, column = the voxel within the tile + x of the corner.
struct MeshCells {
    alignas(16) int word[4][kMeshStage];
};

__device__ __forceinline__ void stage_states(MeshCells& s, const TsdfExtractArgs& a, const float* __restrict__ tsdf,
                                             const float* __restrict__ weight, int t0) {
    const int off[4] = {0, a.nx, a.nx * a.ny, a.nx * a.ny + a.nx};
    for (int i = threadIdx.x; i <= kPointCloudTile; i += kPcThreads) {
#pragma unroll
        for (int row = 0; row < 4; ++row) {
            const long long p = (long long)t0 + i + off[row];
            int w = 0;
            if (p < a.total) w = (weight[p] >= a.min_weight ? 1 : 0) | (tsdf[p] < 0.f ? 2 : 0);
            s.word[row][i] = w;
        }
    }
}

// (every word is completed by the thread that wrote it in stage_states)
__device__ __forceinline__ void stage_records(MeshCells& s, int (&s_first)[4][kMeshStage], const TsdfExtractArgs& a,
                                              const int* __restrict__ first,
                                              const unsigned char* __restrict__ edge_mask, int t0) {
    const int off[4] = {0, a.nx, a.nx * a.ny, a.nx * a.ny + a.nx};
    for (int i = threadIdx.x; i <= kPointCloudTile; i += kPcThreads) {
#pragma unroll
        for (int row = 0; row < 4; ++row) {
            const long long p = (long long)t0 + i + off[row];
            if (p < a.total) {
                s_first[row][i] = first[p];
                s.word[row][i] |= (int)edge_mask[p] << 8;
            }
        }
    }
}

// The four cells of this thread: bits 0 .. 7 observed, bits 8 .. 15 negative, per corner; 0 where the cell does not exist
__device__ __forceinline__ void quad_cells(const MeshCells& s, const TsdfExtractArgs& a, int t0, unsigned (&cell)[4]) {
    const int c0 = 4 * (int)threadIdx.x;
    const int p0 = t0 + c0;   // (below total + 1024: it fits)
    int w[4][5];
#pragma unroll
    for (int row = 0; row < 4; ++row) {
        const int4 q = *reinterpret_cast<const int4*>(&s.word[row][c0]);
        w[row][0] = q.x; w[row][1] = q.y; w[row][2] = q.z; w[row][3] = q.w;
        w[row][4] = s.word[row][c0 + 4];
    }
    // The walk is written out here, not VoxelAt: with VoxelAt::next the face scatter keeps one more SGPR in a VGPR lane and
    // measured 0.3 % slower in three series (docs/LAB_NOTES.md); this is the form it had before the scaffold.
    int i = p0 % a.nx;
    const int rest = p0 / a.nx;
    int j = rest % a.ny, k = rest / a.ny;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        cell[e] = 0;
        if (p0 + e < a.total && i + 1 < a.nx && j + 1 < a.ny && k + 1 < a.nz) {
            unsigned bits = 0;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int word = w[c >> 1][e + (c & 1)];
                bits |= (unsigned)(word & 1) << c | (unsigned)(word >> 1 & 1) << (8 + c);
            }
            cell[e] = bits;
        }
        if (++i == a.nx) {
            i = 0;
            if (++j == a.ny) {
                j = 0;
                ++k;
            }
        }
    }
}

// Faces of tetrahedron t of a cell, and its sign pattern
__device__ __forceinline__ int tet_faces(unsigned cell, int t, int& pattern) {
    const unsigned corners = kTet.corners[t];
    unsigned all = 1;
    pattern = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int c = corners >> (3 * m) & 7;
        all &= cell >> c;
        pattern |= (int)(cell >> (8 + c) & 1) << m;
    }
    if (!(all & 1)) return 0;
    const int negative = __popc(pattern);
    return negative == 2 ? 2 : (negative & 1);
}

__device__ __forceinline__ int quad_face_count(const unsigned (&cell)[4]) {
    int count = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (cell[e] & 0xffu) {
            for (int t = 0; t < 6; ++t) {
                int pattern;
                count += tet_faces(cell[e], t, pattern);
            }
        }
    }
    return count;
}

__global__ __launch_bounds__(kPcThreads) void tsdf_mesh_face_count_kernel(TsdfExtractArgs a,
                                                                          const float* __restrict__ tsdf,
                                                                          const float* __restrict__ weight,
                                                                          int* __restrict__ tile_count, int tiles) {
    __shared__ MeshCells s;
    __shared__ int wave_total[kPcWaves];
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int t0 = tile * kPointCloudTile;
        stage_states(s, a, tsdf, weight, t0);
        __syncthreads();
        unsigned cell[4];
        quad_cells(s, a, t0, cell);
        store_tile_count(wave_count(quad_face_count(cell)), wave_total, &tile_count[tile]);
        __syncthreads();   // (s and wave_total are written again by the next tile)
    }
}

__global__ __launch_bounds__(kPcThreads) void tsdf_mesh_face_scatter_kernel(
    TsdfExtractArgs a, const float* __restrict__ tsdf, const float* __restrict__ weight,
    const int* __restrict__ first, const unsigned char* __restrict__ edge_mask, const int* __restrict__ tile_offset,
    int* __restrict__ faces, long long face_capacity, int tiles) {
    __shared__ MeshCells s;
    __shared__ alignas(16) int s_first[4][kMeshStage];
    __shared__ alignas(16) unsigned char s_faces[12 * kMeshChunk + 16];
    __shared__ int wave_total[kPcWaves];

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int base = tile_offset[tile];   // faces of the tiles before this one
        const int t0 = tile * kPointCloudTile;
        stage_states(s, a, tsdf, weight, t0);
        __syncthreads();
        unsigned cell[4];
        quad_cells(s, a, t0, cell);
        const int mine = quad_face_count(cell), before = wave_exclusive(mine);
        int tile_n;
        const int first_rank = tile_ranks(before, before + mine, wave_total, tile_n);   // (a barrier: every cell is read)

        // rows [base, base + tile_n) of faces, as far as they lie below face_capacity, kMeshChunk at a time
        const int rows = rows_below(face_capacity, base, tile_n);
        if (rows > 0) {   // (the whole workgroup: most tiles of a volume hold no surface)
            stage_records(s, s_first, a, first, edge_mask, t0);
            __syncthreads();
        }
        for (int c0 = 0; c0 < rows; c0 += kMeshChunk) {
            const int cn = rows - c0 < kMeshChunk ? rows - c0 : kMeshChunk;
            const StagedRun<int> run(s_faces, faces, 3, base + c0);
            int rank = first_rank - c0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (!(cell[e] & 0xffu)) continue;
                const int column = 4 * (int)threadIdx.x + e;
                for (int t = 0; t < 6; ++t) {
                    int pattern;
                    const int count = tet_faces(cell[e], t, pattern);
                    if (count == 0) continue;
                    if (rank >= cn || rank + count <= 0) {
                        rank += count;
                        continue;
                    }
                    const unsigned code = kTet.cases[pattern], corners = kTet.corners[t];
                    const bool flip = kTet.flips[t] >> pattern & 1;
                    for (int f = 0; f < count; ++f) {
                        if (rank >= 0 && rank < cn) {
                            int row[3];
#pragma unroll
                            for (int j = 0; j < 3; ++j) {
                                const int edge = code >> (2 + 4 * (3 * f + j)) & 15;
                                const int pm = corners >> (3 * (edge >> 2)) & 7, pn = corners >> (3 * (edge & 3)) & 7;
                                const int d = pm ^ pn, at = column + (pm & 1);
                                row[j] = s_first[pm >> 1][at] +
                                         __popc((unsigned)(s.word[pm >> 1][at] >> 8) & ((1u << (d - 1)) - 1u));
                            }
                            int* face = run.at(rank);
                            face[0] = row[0];
                            face[1] = flip ? row[2] : row[1];
                            face[2] = flip ? row[1] : row[2];
                        }
                        ++rank;
                    }
                }
            }
            __syncthreads();
            run.store(cn);
            __syncthreads();   // (s_faces is written again by the next chunk)
        }
        __syncthreads();   // (s, s_first and wave_total are written again by the next tile)
    }
}

}  // namespace

// [tile words of the vertices][tile words of the faces][first: int32 per voxel][mask: one byte per voxel]
size_t tsdf_mesh_workspace_bytes(long long voxels) {
    return 2 * point_cloud_workspace_bytes(voxels) + round_up_256((size_t)voxels * sizeof(int)) + round_up_256((size_t)voxels);
}

int tsdf_mesh_groups(long long voxels) {
    const int tiles = compaction_tiles(voxels);
    return tiles < kTsdfMeshMaxGroups ? tiles : kTsdfMeshMaxGroups;
}

int launch_tsdf_mesh(const float* tsdf, const float* weight, const float* origin, float voxel_size, float min_weight,
                     float* points, float* normals, int* index, int* offsets, long long capacity, int* faces,
                     int* face_offsets, long long face_capacity, int nx, int ny, int nz, void* workspace, hipStream_t s) {
    TsdfExtractArgs a;
    for (int m = 0; m < 3; ++m) a.origin[m] = origin[m];
    a.voxel_size = voxel_size;
    a.min_weight = min_weight;
    a.nx = nx;
    a.ny = ny;
    a.nz = nz;
    a.total = nx * ny * nz;
    const int tiles = compaction_tiles(a.total);
    const int groups = tsdf_mesh_groups(a.total);
    const size_t words = point_cloud_workspace_bytes(a.total);
    unsigned char* bytes = static_cast<unsigned char*>(workspace);
    int* tile_words = reinterpret_cast<int*>(bytes);
    int* face_words = reinterpret_cast<int*>(bytes + words);
    int* first = reinterpret_cast<int*>(bytes + 2 * words);
    unsigned char* edge_mask = bytes + 2 * words + round_up_256((size_t)a.total * sizeof(int));
    const bool vec = aligned16(tsdf) && aligned16(weight);

    if (int rc = launch_probed("tsdf_mesh_count", vec ? tsdf_mesh_count_kernel<true> : tsdf_mesh_count_kernel<false>,
                               groups, kPcThreads, s, a, tsdf, weight, tile_words, tiles))
        return rc;
    if (int rc = launch_compaction_scan("tsdf_mesh_scan", tile_words, tiles, offsets, 1, s)) return rc;
    if (int rc = launch_probed("tsdf_mesh_scatter", vec ? tsdf_mesh_scatter_kernel<true> : tsdf_mesh_scatter_kernel<false>,
                               groups, kPcThreads, s, a, tsdf, weight, tile_words, points, normals, index, capacity,
                               first, edge_mask, tiles))
        return rc;
    if (int rc = launch_probed("tsdf_mesh_face_count", tsdf_mesh_face_count_kernel, groups, kPcThreads, s, a, tsdf,
                               weight, face_words, tiles))
        return rc;
    if (int rc = launch_compaction_scan("tsdf_mesh_face_scan", face_words, tiles, face_offsets, 1, s)) return rc;
    return launch_probed("tsdf_mesh_face_scatter", tsdf_mesh_face_scatter_kernel, groups, kPcThreads, s, a, tsdf,
                         weight, first, edge_mask, face_words, faces, face_capacity, tiles);
}

}  // namespace pds
