// What the persistent-tile kernels of the full-resolution hourglass layers share: conv3d_t8.hip, conv3d_t8x.hip and
// deconv3d_cell.hip.  All three run 256 threads per workgroup, a grid of (records, batch) workgroups that each walk a static
// list of tiles, a double-buffered LDS halo tile, and ONE deterministic fp64 statistics record per (workgroup, channel).
// The tile walk, the buffer resources, the arguments and the plan of the two 8 -> 8 kernels, the records rule and the launch
// bracket live here; a kernel built on this header provides its LDS layout, its staging (prepare / fetch / stash), its A
// fragments, its MFMA loop and its epilogue.
// The short names below (f32x4 ..., buffer_rsrc, uniform) are meant to become the single definitions of namespace pds: a
// file that starts to include this header drops its own typedef or helper of the same name.
#pragma once
#include "common.hpp"

namespace pds {

constexpr int P3D_THREADS = 256;
constexpr int T8_C = 8;   // input and output channels of conv3d_t8 / conv3d_t8x
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// ---- device side ----------------------------------------------------------------------------------------------------
// The tiles of one workgroup.  gridDim.x (a multiple of 8) workgroups share the `tiles` of a batch element: XCD x (the
// hardware deals workgroups round-robin, so x = blockIdx.x & 7) gets the x-th contiguous eighth of the list, so the halo
// planes that neighbouring tiles share stay in one L2; its per_xcd workgroups visit tile, tile + per_xcd, ... < t_end.
// The coordinates advance by per_xcd in mixed radix: scalar adds with carry instead of divisions.
struct TileWalk {
    int tiles_x, tiles_y, per_xcd, t_end, tile;
    int tx, ty, tz;                // coordinates of `tile`
    int step_x, step_y, step_z;
    __device__ __forceinline__ TileWalk(int tiles_x_, int tiles_y_, int tiles) : tiles_x(tiles_x_), tiles_y(tiles_y_) {
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        per_xcd = gridDim.x >> 3;
        t_end = (int)(((long long)(xcd + 1) * tiles) >> 3);
        tile = (int)(((long long)xcd * tiles) >> 3) + slot;
        tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, tz = tile / (tiles_x * tiles_y);
        step_x = per_xcd % tiles_x, step_y = (per_xcd / tiles_x) % tiles_y, step_z = per_xcd / (tiles_x * tiles_y);
    }
    __device__ __forceinline__ void advance(int& ax, int& ay, int& az) const {
        ax += step_x;
        int carry = ax >= tiles_x ? 1 : 0;
        ax -= carry ? tiles_x : 0;
        ay += step_y + carry;
        carry = ay >= tiles_y ? 1 : 0;
        ay -= carry ? tiles_y : 0;
        az += step_z + carry;
    }
    // Moves (tx, ty, tz) on to the next tile of the list; (px, py, pz) is the tile to stage meanwhile: that next tile, or,
    // behind the last one, the current tile once more (into the idle buffer) instead of a branch around the riders -- the
    // MFMA loop stays one basic block, which is what lets the scheduler interleave it.  The caller steps `tile` itself.
    __device__ __forceinline__ void next(int& px, int& py, int& pz) {
        int nx = tx, ny = ty, nz = tz;
        advance(nx, ny, nz);
        const bool more = tile + per_xcd < t_end;
        px = more ? nx : tx, py = more ? ny : ty, pz = more ? nz : tz;
        tx = nx, ty = ny, tz = nz;
    }
};

// Buffer resource over `bytes` from `base` (wave-uniform base + 32-bit lane offset + scalar offset: no 64-bit vector
// address math).  Stride 0 and flag word 0x00020000 (a raw 32-bit-data buffer) make the hardware range-check offset
// against `bytes`: the kernels pass an offset of ~0u for "outside", which loads 0.0f and drops a store -- the zero padding.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* base, size_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}

__device__ __forceinline__ float uniform(float v) {   // v is the same in every lane: keep it in a scalar register
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

struct T8Args {   // conv3d_t8 and conv3d_t8x
    Src a, b;
    const float* __restrict__ w;     // [8][8][3][3][3]
    const float* __restrict__ bias;  // [8]
    float* __restrict__ out;
    double* __restrict__ partials;   // [(n, oc)][records][2]
    int D, H, W;
    int lrelu;
    int tiles_x, tiles_y, tiles;     // per batch element
    int records;                     // persistent workgroups per batch element (= gridDim.x)
};

// ---- host side ------------------------------------------------------------------------------------------------------
// Persistent workgroups (= statistics records) per batch element: `budget` (2 or 4 per CU) over the whole batch, no more
// than there are tiles, a multiple of 8 (the XCDs of the walk), at least 8.
inline int persistent_records(int tiles, int batch, int budget) {
    int per_n = budget / (batch > 0 ? batch : 1);
    if (per_n > tiles) per_n = tiles;
    per_n = (per_n + 7) / 8 * 8;
    return per_n < 8 ? 8 : per_n;
}

// Tiling and dispatch facts of an 8 -> 8 layer, computed once by launch_conv3d_t8 (conv3d_t8.hip) for both kernels.
struct T8Plan {
    int nb;                              // 16-column blocks per tile
    int tiles_x, tiles_y, tiles, records;
    int src;                             // 0 one plain source, 1 one with a deferred InstanceNorm, 2 two sources
    bool exact;                          // D, H, W are multiples of the tile (2, 4, 16 nb)
    bool certified;                      // every source carries a range certificate
};
inline T8Args t8_args(const ConvLayer& L, const T8Plan& p) {
    return T8Args{L.a,    L.b,    L.weight, L.bias,    L.out,     L.partials, L.in.d,
                  L.in.h, L.in.w, L.lrelu,  p.tiles_x, p.tiles_y, p.tiles,    p.records};
}
bool conv3d_t8x_enabled();   // conv3d_t8x.hip: the same layer on the 16-bit matrix pipe (split operands)
int launch_conv3d_t8x(const ConvLayer& L, const T8Plan& plan, hipStream_t s);

// Launch of KERNEL(A) on (records, batch) workgroups with lds_bytes of dynamic LDS (up to the 160 KB of a CU), bracketed
// by the launch probe; `what` names the kernel to check_launch.
template <auto KERNEL, typename Args>
int launch_persistent(const char* probe_name, const char* what, const Args& A, int records, int batch, size_t lds_bytes,
                      hipStream_t s) {
    static std::atomic<unsigned> attr_done{0};   // (per kernel instantiation) one bit per device
    if (DeviceOnce once{attr_done}) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(160 * 1024));
    }
    const int probe = probe_before(probe_name, s);
    hipLaunchKernelGGL(KERNEL, dim3(records, batch), dim3(P3D_THREADS), lds_bytes, s, A);
    probe_after(probe, records * batch, s);
    return check_launch(what);
}

}  // namespace pds
