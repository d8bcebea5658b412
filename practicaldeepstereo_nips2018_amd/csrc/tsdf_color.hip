// Colour in TSDF fusion (pds_tsdf_color_integrate_fwd, pds_tsdf_color_gather_fwd, pds_tsdf_color_render_fwd; not in the
// reference): the image of every frame is fused beside the distances, and the extracted surface and the raycast get their
// colours back (KinectFusion, Open3D TSDFVolume with colour).
//
// The volume: tsdf and weight as in tsdf.hip, float32 [nz, ny, nx]; color float32 [nz, ny, nx, 3], interleaved: voxel v
// owns color[3 v .. 3 v + 2].  The colour shares the weight.
//
// integrate, per batch entry the two launches of tsdf.hip:
//   tsdf_depth            tsdf.hip's kernel, unchanged (launch_tsdf_depth)
//   tsdf_color_integrate  tsdf_integrate with one step more.  The decisions per voxel are those of tsdf_sample and the
//                         running average that of tsdf_update (tsdf_surface.hpp: one device function each for the two
//                         kernels), so tsdf and weight receive the bits tsdf_integrate gives them.  Where the voxel is
//                         updated, per channel, with x the image value at the pixel the Z was read from and W_old the
//                         weight before the update:  color = fmaf(color, W_old, x * w) / (W_old + w).
//                         The same walk: the volume as ONE row cut into quads of four consecutive voxels that begin on a
//                         16-byte boundary of tsdf and weight (`shift`), one quad per thread and step, 256 threads, a
//                         grid-stride loop.  A quad's colour is 12 consecutive floats from color + 3 * first: three
//                         16-byte accesses where that address is 16-byte aligned (CVEC: color = 12 * shift mod 16), and
//                         voxel by voxel otherwise or where the quad is mixed.  A skipped voxel is neither read nor
//                         written in any of the three tensors.
// gather: tsdf_color_gather, one launch over the rows an extraction wrote (row -> index -> the edge (v, d) -> r -> colour).
// render: tsdf_color_render, one thread per pixel in the 16 x 16 tile of tsdf_raycast: the cell of g(depth) through the
//   device functions of tsdf_ray.hpp, so the colour is read where the normal was taken.
// No atomics, no LDS, no workgroup waits on another.  Every multiply-add is an explicit fmaf and contraction is off, so
// that every form of a kernel gives the same bits.
#include "tsdf_ray.hpp"
#include "tsdf_surface.hpp"

#pragma clang fp contract(off)

namespace pds {

namespace {

constexpr int kTsdfColorThreads = 256;
static_assert(kTsdfQuadsPerGroup == kTsdfColorThreads, "one quad per thread");
static_assert(kTsdfRaycastTile * kTsdfRaycastTile == kTsdfColorThreads, "8 x 8 pixels per wave");

// ---------------------------------------------------------------------------------------------- integrate
// The value of channel c of source pixel `pixel`; image: this entry's.  layout 0: float32 [3, hw], 1: uint8 [hw, 3]
__device__ __forceinline__ float image_value(const void* __restrict__ image, int layout, int hw, int pixel, int c) {
    if (layout == 1) return (float)static_cast<const unsigned char*>(image)[3 * (size_t)pixel + c];
    return static_cast<const float*>(image)[(size_t)c * hw + pixel];
}

// W_old: the weight before tsdf_update
__device__ __forceinline__ float color_update(float held, float W_old, float x, float wt) {
    return fmaf(held, W_old, x * wt) / (W_old + wt);
}

template <bool VEC, bool CVEC, bool CONF>
__global__ __launch_bounds__(kTsdfColorThreads) void tsdf_color_integrate_kernel(
    TsdfIntegrateArgs a, const float* __restrict__ zbuf, const float* __restrict__ wbuf,
    const void* __restrict__ image, int layout, float* __restrict__ tsdf, float* __restrict__ weight,
    float* __restrict__ color, int nx, int ny, int total, int shift, int quads, int h, int w) {
    const int hw = h * w;
    for (int q = blockIdx.x * kTsdfColorThreads + (int)threadIdx.x; q < quads; q += gridDim.x * kTsdfColorThreads) {
        const int first = 4 * q - shift;   // (3 * total < 2^31: no overflow, neither here nor in 3 * first below)
        const int lo = first < 0 ? 0 : first, hi = first + 4 < total ? first + 4 : total;
        // the walk of tsdf_integrate_kernel, from lo: the first quad may begin before the volume
        int i = lo % nx, rest = lo / nx;
        int j = rest % ny, k = rest / ny;
        float t[4], wt[4];
        int pixel[4];
        bool update[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            update[e] = false;
            if (first + e >= lo && first + e < hi) {
                update[e] = tsdf_sample<CONF>(a, zbuf, wbuf, i, j, k, h, w, t[e], wt[e], pixel[e]);
                if (++i == nx) {
                    i = 0;
                    if (++j == ny) {
                        j = 0;
                        ++k;
                    }
                }
            }
        }
        if ((VEC || CVEC) && update[0] && update[1] && update[2] && update[3]) {
            // (all four updated: the quad lies inside the volume, and first is a multiple of 4 behind `shift`)
            float value[4], held[4], old[4];
            if (VEC) {
                const float4 v4 = *reinterpret_cast<const float4*>(tsdf + first);
                const float4 w4 = *reinterpret_cast<const float4*>(weight + first);
                value[0] = v4.x; value[1] = v4.y; value[2] = v4.z; value[3] = v4.w;
                held[0] = w4.x; held[1] = w4.y; held[2] = w4.z; held[3] = w4.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    value[e] = tsdf[first + e];
                    held[e] = weight[first + e];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                old[e] = held[e];
                tsdf_update(a.max_weight, t[e], wt[e], value[e], held[e]);
            }
            if (VEC) {
                *reinterpret_cast<float4*>(tsdf + first) = make_float4(value[0], value[1], value[2], value[3]);
                *reinterpret_cast<float4*>(weight + first) = make_float4(held[0], held[1], held[2], held[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    tsdf[first + e] = value[e];
                    weight[first + e] = held[e];
                }
            }
            float* at = color + 3 * (size_t)first;
            float c[12];
            if (CVEC) {
                // (color + 3 * first is 16-byte aligned: 48 q - 12 shift bytes behind a base of 12 shift mod 16)
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    const float4 v = reinterpret_cast<const float4*>(at)[m];
                    c[4 * m] = v.x; c[4 * m + 1] = v.y; c[4 * m + 2] = v.z; c[4 * m + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int m = 0; m < 12; ++m) c[m] = at[m];
            }
#pragma unroll
            for (int m = 0; m < 12; ++m)
                c[m] = color_update(c[m], old[m / 3], image_value(image, layout, hw, pixel[m / 3], m % 3), wt[m / 3]);
            if (CVEC) {
#pragma unroll
                for (int m = 0; m < 3; ++m)
                    reinterpret_cast<float4*>(at)[m] = make_float4(c[4 * m], c[4 * m + 1], c[4 * m + 2], c[4 * m + 3]);
            } else {
#pragma unroll
                for (int m = 0; m < 12; ++m) at[m] = c[m];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (update[e]) {
                    float value = tsdf[first + e], held = weight[first + e];
                    const float old = held;
                    tsdf_update(a.max_weight, t[e], wt[e], value, held);
                    tsdf[first + e] = value;
                    weight[first + e] = held;
                    float* at = color + 3 * (size_t)(first + e);
#pragma unroll
                    for (int m = 0; m < 3; ++m)
                        at[m] = color_update(at[m], old, image_value(image, layout, hw, pixel[e], m), wt[e]);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- gather
// One lane per output FLOAT, not per row: element e = 3 row + c.  The store of a wave is then 256 contiguous bytes in one
// instruction, whatever the count, with no staging; a lane per row would store 12 bytes at a stride of 12, three
// instructions that each touch every line of the run.  The price is that the three lanes of a row each form r (one
// division) and read the same index and the same two tsdf values -- one address within the wave's request, so no more
// traffic -- while their reads of c_v and c_n fall on neighbouring floats.  The kernel is a gather: its time is the
// latency of those dependent reads (index -> tsdf, color), not the arithmetic.
// A row whose index names no edge of the volume (negative, or a neighbour beyond the last voxel: not what an extraction
// writes) gets NaN and reads nothing.
__global__ __launch_bounds__(kTsdfColorThreads) void tsdf_color_gather_kernel(
    const int* __restrict__ index, const int* __restrict__ offsets, int edges, const float* __restrict__ tsdf,
    const float* __restrict__ color, float* __restrict__ colors, long long capacity, int nx, int sz, int total) {
    const long long found = offsets[1];
    const long long elements = 3 * (found < capacity ? found : capacity);   // (found >= 0)
    const long long stride = (long long)gridDim.x * kTsdfColorThreads;
    for (long long e = (long long)blockIdx.x * kTsdfColorThreads + threadIdx.x; e < elements; e += stride) {
        const long long row = e / 3;
        const int c = (int)(e - 3 * row);
        const int id = index[row];
        float out = __builtin_nanf("");
        if (id >= 0) {
            const int v = id / edges, rest = id - v * edges;
            const int d = edges == 3 ? 1 << rest : rest + 1;
            const long long n = (long long)v + (d & 1) + ((d & 2) ? nx : 0) + ((d & 4) ? sz : 0);
            if (n < total) {   // (v < n)
                const float own = tsdf[v];
                const float r = own / (own - tsdf[n]);   // (the expression of the scatters)
                const float cv = color[3 * (size_t)v + c], cn = color[3 * (size_t)n + c];
                out = fmaf(r, cn - cv, cv);
            }
        }
        colors[e] = out;
    }
}

// ---------------------------------------------------------------------------------------------- render
__global__ __launch_bounds__(kTsdfColorThreads) void tsdf_color_render_kernel(TsdfRaycastArgs a,
                                                                              const float* __restrict__ weight,
                                                                              const float* __restrict__ color,
                                                                              const float* __restrict__ depth,
                                                                              float* __restrict__ colors) {
    // the pixel of tsdf_raycast_kernel: each wave an 8 x 8 block of the tile
    const int tiles = a.tiles_x * a.tiles_y;
    const int entry = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - entry * tiles;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int px = tx * kTsdfRaycastTile + (wave & 1) * 8 + (lane & 7);
    const int py = ty * kTsdfRaycastTile + (wave >> 1) * 8 + (lane >> 3);
    if (px >= a.w || py >= a.h) return;
    const int pixel = (entry * a.h + py) * a.w + px;   // (batch * h * w < 2^31)
    const float* pose = a.pose[entry];
    const float nan = __builtin_nanf("");
    float rgb[3] = {nan, nan, nan};
    const float s = depth[pixel];
    // (a volume without cells has no surface to a raycast; raycast_cell needs every n_a >= 2)
    if (s == s && a.nx >= 2 && a.ny >= 2 && a.nz >= 2) {
        float x, y, d[3], o[3];
        raycast_ray(a, pose, px, py, x, y, d, o);
        const float g[3] = {fmaf(s, d[0], o[0]), fmaf(s, d[1], o[1]), fmaf(s, d[2], o[2])};
        float f[3], held[8];
        const int sy = a.nx, sz = a.nx * a.ny;
        const int base = raycast_cell(a, g, f);
        raycast_corners(weight, base, sy, sz, held);
        if (raycast_observed(held, a.min_weight)) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    v[e] = color[3 * (size_t)(base + (e & 1) + (e >> 1 & 1) * sy + (e >> 2) * sz) + c];
                rgb[c] = raycast_value(v, f);
            }
        }
    }
    float* out = colors + 3 * (size_t)pixel;
    out[0] = rgb[0];
    out[1] = rgb[1];
    out[2] = rgb[2];
}

template <bool VEC, bool CVEC>
auto integrate_form(bool conf) {
    return conf ? tsdf_color_integrate_kernel<VEC, CVEC, true> : tsdf_color_integrate_kernel<VEC, CVEC, false>;
}

}  // namespace

int launch_tsdf_color_integrate(const ReprojectArgs& r, const TsdfIntegrateArgs& args, const float* transforms,
                                int weight_by_confidence, const float* disparity, const unsigned char* valid,
                                const float* confidence, const void* image, int image_layout, float* tsdf,
                                float* weight, float* color, int nx, int ny, int nz, int batch, int h, int w,
                                void* workspace, hipStream_t s) {
    const int hw = h * w, total = nx * ny * nz;
    float* zbuf = static_cast<float*>(workspace);
    float* wbuf = weight_by_confidence ? zbuf + tsdf_integrate_workspace_bytes(hw) / (2 * sizeof(float)) : nullptr;
    // the quads of launch_tsdf_integrate; the colour of a quad begins 12 * shift bytes before a multiple of 48 behind color
    const bool vec = (((uintptr_t)tsdf ^ (uintptr_t)weight) & 15u) == 0;
    const int shift = vec ? (int)(((uintptr_t)tsdf & 15u) / sizeof(float)) : 0;
    const bool cvec = (((uintptr_t)color - 12u * (unsigned)shift) & 15u) == 0;
    const int quads = (int)(((long long)total + shift + 3) / 4);
    const int groups = tsdf_integrate_groups(total, shift);
    const auto integrate = vec ? (cvec ? integrate_form<true, true>(wbuf) : integrate_form<true, false>(wbuf))
                               : (cvec ? integrate_form<false, true>(wbuf) : integrate_form<false, false>(wbuf));
    const size_t entry_bytes = image_layout == 1 ? 3 * (size_t)hw : 3 * (size_t)hw * sizeof(float);
    for (int b = 0; b < batch; ++b) {
        const float* d = disparity + (size_t)b * hw;
        const unsigned char* ok = valid ? valid + (size_t)b * hw : nullptr;
        const float* c = confidence ? confidence + (size_t)b * hw : nullptr;
        const void* picture = static_cast<const unsigned char*>(image) + b * entry_bytes;
        TsdfIntegrateArgs a = args;
        for (int k = 0; k < 12; ++k) (k < 9 ? a.A[k] : a.b[k - 9]) = transforms[12 * (size_t)b + k];
        if (int rc = launch_tsdf_depth(r, d, ok, c, zbuf, wbuf, h, w, s)) return rc;
        if (int rc = launch_probed("tsdf_color_integrate", integrate, groups, kTsdfColorThreads, s, a, zbuf, wbuf,
                                   picture, image_layout, tsdf, weight, color, nx, ny, total, shift, quads, h, w))
            return rc;
    }
    return 0;
}

int launch_tsdf_color_gather(const int* index, const int* offsets, int edges_per_voxel, const float* tsdf,
                             const float* color, float* colors, long long capacity, int nx, int ny, int nz,
                             hipStream_t s) {
    const long long total = (long long)nx * ny * nz;
    // the count lives on the device: the grid is sized by what the buffers can hold, and the lanes beyond the count leave
    const long long most = capacity < edges_per_voxel * total ? capacity : edges_per_voxel * total;
    if (most == 0) return 0;
    const long long wanted = (3 * most + kTsdfColorThreads - 1) / kTsdfColorThreads;
    const int groups = (int)(wanted < kTsdfColorGatherMaxGroups ? wanted : kTsdfColorGatherMaxGroups);
    return launch_probed("tsdf_color_gather", tsdf_color_gather_kernel, groups, kTsdfColorThreads, s, index, offsets,
                         edges_per_voxel, tsdf, color, colors, capacity, nx, nx * ny, (int)total);
}

int launch_tsdf_color_render(const TsdfRaycastArgs& args, const float* rays, const float* weight, const float* color,
                             const float* depth, float* colors, int batch, hipStream_t s) {
    for (int first = 0; first < batch; first += kTsdfRaycastPoses) {
        const int entries = batch - first < kTsdfRaycastPoses ? batch - first : kTsdfRaycastPoses;
        TsdfRaycastArgs a = args;
        for (int e = 0; e < entries; ++e)
            for (int k = 0; k < 12; ++k) a.pose[e][k] = rays[12 * (size_t)(first + e) + k];
        const size_t offset = (size_t)first * a.h * a.w;
        if (int rc = launch_probed("tsdf_color_render", tsdf_color_render_kernel, tsdf_raycast_groups(entries, a.h, a.w),
                                   kTsdfColorThreads, s, a, weight, color, depth + offset, colors + 3 * offset))
            return rc;
    }
    return 0;
}

}  // namespace pds
