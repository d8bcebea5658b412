// Point-to-plane ICP of a disparity frame against a rendered model (pds_icp_system_fwd; not in the reference): the
// linearised system of frame-to-model tracking, the consumer of tsdf_raycast.hip's model prediction.
//
// Per batch entry the host gives the transform [R | t] (frame camera -> model camera), rounded once to float32.  Per source
// pixel, in fp32, every multiply-add an explicit fmaf (contraction is off below the include; reproject_one is the shared
// device function, compiled as everywhere else):
//   1. P = reproject_one(...); no row where P is NaN
//   2. q_a = fmaf(R_a0, P_x, fmaf(R_a1, P_y, fmaf(R_a2, P_z, t_a))); no row unless q_z > 0 and q is finite
//   3. x = q_x / q_z, y = q_y / q_z, u = fmaf(fx, x, fmaf(skew, y, cx)), v = fmaf(fy, y, cy);
//      px = floorf(u + 0.5f), py = floorf(v + 0.5f); no row outside [0, wm) x [0, hm) (a NaN fails)
//   4. Z = depth[py, px], n = normals[py, px]; no row where any of the four is NaN
//      y_m = (py - cy) / fy, x_m = fmaf(-skew, y_m, px - cx) / fx, m = (Z x_m, Z y_m, Z)
//   5. e = m - q; no row unless fmaf(e_x, e_x, fmaf(e_y, e_y, e_z e_z)) <= max_distance * max_distance
//   6. with frame normals n_f: s_a = fmaf(R_a0, n_fx, fmaf(R_a1, n_fy, R_a2 n_fz)); no row where n_f holds a NaN or
//      not fmaf(s_x, n_x, fmaf(s_y, n_y, s_z n_z)) >= min_cosine
//   7. r = fmaf(n_x, e_x, fmaf(n_y, e_y, n_z e_z)); J = (q x n, n) with (q x n)_x = fmaf(q_y, n_z, -(q_z n_y)) and its
//      cyclic successors.  The row is (J_0 .. J_5, r).
//
// The system of an entry: 29 doubles -- the upper triangle of sum J J^T (21, row-major), sum J r (6), sum r^2, the row
// count.  Every product is fma((double)a, (double)b, sum): the product of two float32 is exact in fp64 (48 bits in 53), so
// this is the product added in fp64 and nothing else.  The order of the additions is fixed:
//   icp_rows    one workgroup of 256 threads per tile of kIcpTile = 1024 source pixels of one entry; thread t takes the
//               pixels tile * 1024 + k * 256 + t, k = 0 .. 3 in that order, into its own 28 doubles and a counter; each
//               wave folds its 64 lanes by lane + 32, + 16, ... + 1 (__shfl_down: lane 0 holds the sum); the four waves
//               meet in LDS and threads 0 .. 28 add wave 0, 1, 2, 3 in that order and store one partial of 29 doubles
//               per workgroup into the workspace
//   icp_reduce  one workgroup per entry: thread c < 29 adds component c of the entry's partials in ascending tile order
//               and stores it as two 32-bit words (the output need only be 4-byte aligned)
// No atomics, no workgroup waits on another, plain vector stores: the same bits on every run and on every stream.
// pds_icp_system_robust_fwd runs the same two kernels with Huber weights (icp_rows_kernel<true>, below).
// rows (optional) [B, H, W, 7]: the row of every pixel, seven NaNs where there is none.
#include "common.hpp"

#pragma clang fp contract(off)

#include "icp_row.hpp"   // icp_row: steps 1 - 7, shared with icp_color.hip

namespace pds {

namespace {

constexpr int kIcpThreads = 256;
constexpr int kIcpWaves = kIcpThreads / 64;
constexpr int kIcpPerThread = kIcpTile / kIcpThreads;
static_assert(kIcpPerThread * kIcpThreads == kIcpTile, "whole pixels per thread");

// ROBUST: the Huber weight of a row, w = |r| <= huber ? 1.f : huber / |r| (fp32), multiplies every term of the first 28
// sums: fma((double)w, (double)a * (double)b, sum) -- the inner product is exact in fp64, so the weight adds one rounding per
// term; slot 27 is sum w r^2, slot 28 stays the unweighted row count; the order of the additions is the same.  With w = 1
// (huber = inf) the term is the exact product and the sum has the bits of the unweighted kernel.  huber comes last so that
// the unweighted instantiation, which never reads it, keeps its argument offsets and its code.
template <bool ROBUST>
__global__ __launch_bounds__(kIcpThreads) void icp_rows_kernel(IcpArgs a, const float* __restrict__ disparity,
                                                               const unsigned char* __restrict__ valid,
                                                               const float* __restrict__ confidence,
                                                               const float* __restrict__ normals,
                                                               const float* __restrict__ model_depth,
                                                               const float* __restrict__ model_normals,
                                                               double* __restrict__ partials, float* __restrict__ rows,
                                                               float huber) {
    __shared__ double wave_part[kIcpWaves][kIcpSystem];
    const int local = (int)blockIdx.x / a.tiles, tile = (int)blockIdx.x - local * a.tiles;
    const int entry = a.first + local;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pixels = a.h * a.w;
    const float* T = a.transform[local];   // uniform over the workgroup

    double acc[kIcpSystem - 1];
#pragma unroll
    for (int c = 0; c < kIcpSystem - 1; ++c) acc[c] = 0.0;
    int count = 0;
    for (int k = 0; k < kIcpPerThread; ++k) {
        const long long at = (long long)tile * kIcpTile + k * kIcpThreads + tid;   // (may pass 2^31 in the last tile)
        if (at >= pixels) break;
        const int pixel = (int)at;
        float row[7];
        IcpProjection unused;   // (what a photometric row would read: dead here)
        const bool has = icp_row(a, T, disparity, valid, confidence, normals, model_depth, model_normals, entry, pixel, row,
                                 unused);
        if (rows) {
            float* out = rows + 7 * ((size_t)entry * pixels + pixel);
            const float nan = __builtin_nanf("");
#pragma unroll
            for (int c = 0; c < 7; ++c) out[c] = has ? row[c] : nan;
        }
        if (has) {
            double d[7];
#pragma unroll
            for (int c = 0; c < 7; ++c) d[c] = (double)row[c];
            int c = 0;
            if constexpr (ROBUST) {
                const float size = fabsf(row[6]);
                const double weight = (double)(size <= huber ? 1.f : huber / size);
#pragma unroll
                for (int i = 0; i < 6; ++i)
#pragma unroll
                    for (int j = i; j < 6; ++j, ++c) acc[c] = fma(weight, d[i] * d[j], acc[c]);
#pragma unroll
                for (int i = 0; i < 6; ++i) acc[21 + i] = fma(weight, d[i] * d[6], acc[21 + i]);
                acc[27] = fma(weight, d[6] * d[6], acc[27]);
            } else {
#pragma unroll
                for (int i = 0; i < 6; ++i)
#pragma unroll
                    for (int j = i; j < 6; ++j, ++c) acc[c] = fma(d[i], d[j], acc[c]);
#pragma unroll
                for (int i = 0; i < 6; ++i) acc[21 + i] = fma(d[i], d[6], acc[21 + i]);
                acc[27] = fma(d[6], d[6], acc[27]);
            }
            ++count;
        }
    }
    // the wave: lane + 32, + 16, ... + 1; lane 0 holds the sum of the 64 lanes
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int c = 0; c < kIcpSystem - 1; ++c) acc[c] += __shfl_down(acc[c], off, 64);
        count += __shfl_down(count, off, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < kIcpSystem - 1; ++c) wave_part[wave][c] = acc[c];
        wave_part[wave][kIcpSystem - 1] = (double)count;
    }
    __syncthreads();
    if (tid < kIcpSystem) {
        double sum = wave_part[0][tid];
#pragma unroll
        for (int k = 1; k < kIcpWaves; ++k) sum += wave_part[k][tid];
        partials[((size_t)entry * a.tiles + tile) * kIcpSystem + tid] = sum;
    }
}

__global__ __launch_bounds__(64) void icp_reduce_kernel(const double* __restrict__ partials, int tiles,
                                                        int* __restrict__ system) {
    const int entry = (int)blockIdx.x, c = (int)threadIdx.x;
    if (c >= kIcpSystem) return;
    const double* from = partials + (size_t)entry * tiles * kIcpSystem + c;
    double sum = 0.0;
#pragma unroll 8
    for (int t = 0; t < tiles; ++t) sum += from[(size_t)t * kIcpSystem];
    int* out = system + 2 * ((size_t)entry * kIcpSystem + c);
    out[0] = __double2loint(sum);
    out[1] = __double2hiint(sum);
}

}  // namespace

int icp_tiles(int h, int w) { return (int)(((long long)h * w + kIcpTile - 1) / kIcpTile); }

size_t icp_workspace_bytes(int batch, int h, int w) {
    return ((size_t)batch * icp_tiles(h, w) * kIcpSystem * sizeof(double) + 255) & ~(size_t)255;
}

int launch_icp_system(const IcpArgs& args, const float* transforms, const float* disparity, const unsigned char* valid,
                      const float* confidence, const float* normals, const float* model_depth,
                      const float* model_normals, void* system, float* rows, int batch, void* workspace,
                      hipStream_t s, bool robust, float huber) {
    double* partials = static_cast<double*>(workspace);
    for (int first = 0; first < batch; first += kIcpPoses) {
        const int entries = batch - first < kIcpPoses ? batch - first : kIcpPoses;
        IcpArgs a = args;
        a.first = first;
        for (int e = 0; e < entries; ++e)
            for (int k = 0; k < 12; ++k) a.transform[e][k] = transforms[12 * (size_t)(first + e) + k];
        const int groups = entries * a.tiles;
        const int probe = probe_before("icp_rows", s);
        if (robust)
            hipLaunchKernelGGL(icp_rows_kernel<true>, dim3(groups), dim3(kIcpThreads), 0, s, a, disparity, valid,
                               confidence, normals, model_depth, model_normals, partials, rows, huber);
        else
            hipLaunchKernelGGL(icp_rows_kernel<false>, dim3(groups), dim3(kIcpThreads), 0, s, a, disparity, valid,
                               confidence, normals, model_depth, model_normals, partials, rows, 0.f);
        probe_after(probe, groups, s);
        if (int rc = check_launch("icp_rows")) return rc;
    }
    const int probe = probe_before("icp_reduce", s);
    hipLaunchKernelGGL(icp_reduce_kernel, dim3(batch), dim3(64), 0, s, partials, args.tiles, static_cast<int*>(system));
    probe_after(probe, batch, s);
    return check_launch("icp_reduce");
}

}  // namespace pds
