// The scaffold of the ordered compactions: what is an element, what is kept and what is its record stay in the clients,
// the mechanics are here.  The clients, five compactions in four files:
//   point_cloud.hip    the kept pixels of a disparity map (and the scan kernel that all five go through)
//   triangle_mesh.hip  the faces of the disparity mesh
//   tsdf.hip           the surface points of the volume (tsdf_extract_*; tsdf_depth only loads its quads from here)
//   tsdf_mesh.hip      the vertices and the faces of the volume's mesh
// Each is three launches over tiles of kPointCloudTile flat elements, four consecutive elements (a quad) per thread of a
// workgroup of kPcThreads: count per tile, ONE workgroup that scans the tile counts, and a scatter that evaluates the
// predicate again, ranks the kept records within the tile, stages them in LDS at their rank and stores them as
// contiguous runs.  Three rules hold in all of them:
//   order     integer arithmetic only: a record's row is the tile's offset + the wave totals before its wave + the
//             records of the lower lanes + those before it in its own thread, so every run gives the same rows.
//   no wait   no workgroup ever waits on another (no look-back, no flag, no spin: a compaction that spins hangs when
//             its predecessor is not resident, and the machine with it).  The launches are the only ordering.
//   capacity  only rows below `capacity` are written; the counts and the offsets are always the TRUE ones.
// The two LDS meetings below (store_tile_count, tile_ranks) contain a workgroup barrier, so every thread of the
// workgroup calls them; a kernel that walks several tiles also puts a __syncthreads() behind each tile, because the
// next tile writes the same LDS again.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace pds {

constexpr int kPcThreads = 256;
constexpr int kPcWaves = kPcThreads / 64;
static_assert(kPointCloudTile == 4 * kPcThreads, "one quad of elements per thread");

// ---------------------------------------------------------------------------------------------- the quad of a thread
// This thread's quad of `tile`: its first element and how many of its four elements exist (0: none, first = 0)
__device__ __forceinline__ int tile_quad(int total, int tile, int& first) {
    const long long at = (long long)tile * kPointCloudTile + 4 * (int)threadIdx.x;
    if (at >= total) {
        first = 0;
        return 0;
    }
    first = (int)at;
    return total - first < 4 ? total - first : 4;
}

// out[e] = ptr[first + e] for e < n, `fill` beyond.  VEC: ptr is 16-byte aligned and first a multiple of four, so a
// whole quad is one 16-byte load
template <bool VEC>
__device__ __forceinline__ void load_quad(const float* __restrict__ ptr, int first, int n, float fill,
                                          float (&out)[4]) {
    if (VEC && n == 4) {
        const float4 v = *reinterpret_cast<const float4*>(ptr + first);
        out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = e < n ? ptr[first + e] : fill;
    }
}

// ---------------------------------------------------------------------------------------------- count
// The sum of v over the wave, in every lane (not named wave_sum: common.hpp has wave_sum(double), and a float argument
// would be ambiguous between the two)
__device__ __forceinline__ int wave_count(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// *tile_count = the sum of the waves' wave_n (uniform within a wave).  A WORKGROUP BARRIER: wave_total[kPcWaves] is LDS
__device__ __forceinline__ void store_tile_count(int wave_n, int* wave_total, int* __restrict__ tile_count) {
    if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = wave_n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
#pragma unroll
        for (int k = 0; k < kPcWaves; ++k) sum += wave_total[k];
        *tile_count = sum;
    }
}

// ---------------------------------------------------------------------------------------------- rank
// The two in-wave prefixes.  Of a 0/1 flag: the set bits of the lower lanes of its ballot
__device__ __forceinline__ int lower_lanes(unsigned long long ballot) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

// Of a count per thread: the sum of `mine` over the lower lanes (so the last lane's result + its `mine` is the wave's sum)
__device__ __forceinline__ int wave_exclusive(int mine) {
    const int lane = threadIdx.x & 63;
    int inclusive = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int below = __shfl_up(inclusive, off, 64);
        if (lane >= off) inclusive += below;
    }
    return inclusive - mine;
}

// The cross-wave half: -> the rank within the tile of this thread's first record, tile_n = the records of the tile.
// before_in_wave: the records of the lower lanes of this wave; wave_n: those of the whole wave, read from the wave's
// LAST lane only (a ballot's popcount is the same in every lane; of a scan, before_in_wave + mine is right there).
// A WORKGROUP BARRIER: wave_total[kPcWaves] is LDS
__device__ __forceinline__ int tile_ranks(int before_in_wave, int wave_n, int* wave_total, int& tile_n) {
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) wave_total[wave] = wave_n;
    __syncthreads();
    int first_rank = before_in_wave;
    tile_n = 0;
#pragma unroll
    for (int k = 0; k < kPcWaves; ++k) {
        const int s = wave_total[k];
        first_rank += k < wave ? s : 0;
        tile_n += s;
    }
    return first_rank;
}

// ---------------------------------------------------------------------------------------------- store
// The rows of [base, base + tile_n) that lie below capacity
__device__ __forceinline__ int rows_below(long long capacity, int base, int tile_n) {
    const long long room = capacity - base;
    return room <= 0 ? 0 : (room < tile_n ? (int)room : tile_n);
}

// lds[shift + j] -> dst[j] for j < bytes, by the whole workgroup.  shift = dst & 15, so lds + lo and dst - shift + lo
// are 16-byte aligned together; E (4 or 1) is the element size, which divides shift and bytes.
template <int E>
__device__ __forceinline__ void store_run(const unsigned char* lds, unsigned char* dst, int shift, int bytes) {
    unsigned char* g = dst - shift;
    const int end = shift + bytes;
    for (int lo = 16 * (int)threadIdx.x; lo < end; lo += 16 * kPcThreads) {
        if (lo >= shift && lo + 16 <= end) {
            *reinterpret_cast<uint4*>(g + lo) = *reinterpret_cast<const uint4*>(lds + lo);
        } else {
            const int from = lo > shift ? lo : shift, to = lo + 16 < end ? lo + 16 : end;
            for (int j = from; j < to; j += E) {
                if constexpr (E == 4)
                    *reinterpret_cast<unsigned*>(g + j) = *reinterpret_cast<const unsigned*>(lds + j);
                else
                    g[j] = lds[j];
            }
        }
    }
}

// One staged output of a scatter: the run of records of `record` elements T (4 bytes, or 1) that begins at row `first_row`
// of the output `base`.  `staging` is a 16-byte aligned LDS buffer of the run's bytes + 16; the run is staged at the
// misalignment of its global address, so that a 16-byte store of store_run reads a 16-byte aligned LDS address.
// The staging pointer is kept in the LDS address space: as a generic pointer in a member it costs the point cloud's
// scatter 14 to 22 VGPRs (the ranks' addresses are then formed in 64 bits before the address space is inferred).
template <typename T>
struct StagedRun {
    using Lds = __attribute__((address_space(3))) unsigned char*;
    Lds staging;
    unsigned char* out;   // the global address of the run
    int shift, record;    // shift = out & 15
    __device__ __forceinline__ StagedRun(unsigned char* staging_, void* base, int record_, long long first_row)
        : staging((Lds)staging_), out(static_cast<unsigned char*>(base) + (long long)sizeof(T) * record_ * first_row),
          shift((int)((uintptr_t)out & 15)), record(record_) {}
    // where row `rank` of the run is staged
    __device__ __forceinline__ T* at(int rank) const {
        return (T*)(staging + shift + (int)sizeof(T) * record * rank);
    }
    // the first `rows` rows, by the whole workgroup; the caller puts a __syncthreads() before and, where the staging is
    // written again, behind
    __device__ __forceinline__ void store(int rows) const {
        store_run<(int)sizeof(T)>((const unsigned char*)staging, out, shift, (int)sizeof(T) * record * rows);
    }
};

// ---------------------------------------------------------------------------------------------- host
inline int compaction_tiles(long long total) { return (int)((total + kPointCloudTile - 1) / kPointCloudTile); }

// One launch between its probes: -> check_launch(name).  `groups` is also what the probe reports
template <typename... Params, typename... Args>
int launch_probed(const char* name, void (*kernel)(Params...), int groups, int threads, hipStream_t s, Args... args) {
    const int probe = probe_before(name, s);
    hipLaunchKernelGGL(kernel, dim3(groups), dim3(threads), 0, s, static_cast<Params>(args)...);
    probe_after(probe, groups, s);
    return check_launch(name);
}

}  // namespace pds
