// Point-to-plane plus photometric system of a disparity frame with its image against a rendered, coloured model
// (pds_icp_color_system_fwd; not in the reference): the two linearised systems of colour tracking in one pass.
//
// The geometric row of a pixel is icp_row (icp_row.hpp): steps 1 - 7 of icp.hip, the same device code and the same bits.
// The photometric row exists only where the geometric row exists, and only where all of this holds -- fp32, every
// multiply-add an explicit fmaf, contraction off:
//   1. I_f = intensity[p] is not NaN
//   2. u, v of step 3, not rounded: x0 = floorf(u), y0 = floorf(v), a = u - x0, b = v - y0; no row unless 0 <= x0,
//      x0 + 1 <= wm - 1, 0 <= y0, y0 + 1 <= hm - 1
//   3. the taps L00, L10 (x0 + 1), L01 (y0 + 1), L11 of model_intensity and the model depths Z00 .. Z11 there; no row where
//      one of the eight is NaN or unless |Z_tap - q_z| <= max_distance for all four (the same surface: no colour is mixed
//      across an occlusion edge)
//   4. the bilinear patch and its own derivative:
//        top = fmaf(a, L10 - L00, L00), bot = fmaf(a, L11 - L01, L01), I_m = fmaf(b, bot - top, top)
//        I_u = fmaf(b, (L11 - L01) - (L10 - L00), L10 - L00), I_v = bot - top
//   5. r_c = I_f - I_m; with x = q_x / q_z, y = q_y / q_z as in step 3 and iz = 1 / q_z:
//        g_x = (I_u fx) iz, g_y = fmaf(I_u, skew, I_v fy) iz, g_z = -fmaf(g_x, x, g_y y)
//      J_c = (q x g, g), the cross product formed as in step 7.  The row is (J_c0 .. J_c5, r_c), in intensity units.
// Sign: the frame point moves as q <- q + omega x q + v, its projection by (du, dv) = dpi/dq . dq, and the sampled model
// intensity by grad I . (du, dv) = g . dq with g = (dI/dq) as above (dpi/dq is [fx, skew, -(fx x + skew y); 0, fy, -fy y] / q_z).
// The residual after the step is I_f - I_m(q + dq) = r_c - g . (omega x q + v) = r_c - (q x g) . omega - g . v = r_c - J_c xi:
// min sum (r - J xi)^2 with xi = (omega, v), as for the geometric row (r - n . dq, J = (q x n, n)).
//
// Sums: two systems of 29 doubles per entry, in the layout and with the Huber weights of icp.hip (huber for the geometric
// rows, color_huber for the photometric ones; +inf: the weight is 1.f and the term the exact product, so the sums have the
// bits of the unweighted kernel).  The order of the additions is icp.hip's: thread t of a tile of 1024 pixels takes the
// pixels k * 256 + t, k = 0 .. 3; a wave folds lane + 32, + 16, ... + 1; waves 0 .. 3 meet in LDS; icp_reduce adds the tiles
// of an entry in ascending order.  The geometric partials live in the first icp_workspace_bytes of the workspace, the
// photometric ones in the second; one reduce launch of 2 * batch workgroups serves both.  No atomics.
// A thread holds 56 fp64 accumulators (112 VGPRs) beside the row arithmetic: the kernel-resource-usage remark of the
// compiler reports no scratch (DESIGN.md 3.20 records the figures).
// rows (optional) [B, H, W, 14]: the geometric row then the photometric row of every pixel, seven NaNs each where absent.
#include "common.hpp"

#pragma clang fp contract(off)

#include "icp_row.hpp"

namespace pds {

namespace {

constexpr int kIcpThreads = 256;
constexpr int kIcpWaves = kIcpThreads / 64;
constexpr int kIcpPerThread = kIcpTile / kIcpThreads;
constexpr int kSums = kIcpSystem - 1;   // the 28 weighted sums; the count travels as an int
static_assert(kIcpPerThread * kIcpThreads == kIcpTile, "whole pixels per thread");

// The photometric row of a pixel whose geometric row exists (g: what icp_row left of step 3); false: none
__device__ __forceinline__ bool icp_color_row(const IcpArgs& a, const IcpProjection& g, float frame_intensity,
                                              const float* __restrict__ model_depth,
                                              const float* __restrict__ model_intensity, int entry, float (&row)[7]) {
    // One decision at the end instead of a return per test: every nested branch of a wave costs a saved exec mask, and
    // the kernel has no scalar registers to spare.  The taps of a refused cell are read at the cell's
    // clamped origin, inside the model, and not used.
    // 1.
    bool ok = frame_intensity == frame_intensity;
    // 2. (u and v are finite: their roundings lie inside the model)
    const float fx0 = floorf(g.u), fy0 = floorf(g.v);
    ok = ok && fx0 >= 0.f && fx0 + 1.f <= (float)(a.wm - 1) && fy0 >= 0.f && fy0 + 1.f <= (float)(a.hm - 1);
    const float ta = g.u - fx0, tb = g.v - fy0;
    const int x0 = ok ? (int)fx0 : 0, y0 = ok ? (int)fy0 : 0;
    const int right = ok ? 1 : 0, below = ok ? a.wm : 0;
    // 3.
    const size_t at = (size_t)(a.model_batch == 1 ? 0 : entry) * ((size_t)a.hm * a.wm) + (size_t)y0 * a.wm + x0;
    const float L00 = model_intensity[at], L10 = model_intensity[at + right];
    const float L01 = model_intensity[at + below], L11 = model_intensity[at + below + right];
    const float Z00 = model_depth[at], Z10 = model_depth[at + right];
    const float Z01 = model_depth[at + below], Z11 = model_depth[at + below + right];
    ok = ok && L00 == L00 && L10 == L10 && L01 == L01 && L11 == L11;
    // (a NaN depth fails its comparison)
    ok = ok && fabsf(Z00 - g.q[2]) <= a.max_distance && fabsf(Z10 - g.q[2]) <= a.max_distance &&
         fabsf(Z01 - g.q[2]) <= a.max_distance && fabsf(Z11 - g.q[2]) <= a.max_distance;
    // 4.
    const float dx0 = L10 - L00, dx1 = L11 - L01;
    const float top = fmaf(ta, dx0, L00), bot = fmaf(ta, dx1, L01);
    const float Iv = bot - top;
    const float Im = fmaf(tb, Iv, top);
    const float Iu = fmaf(tb, dx1 - dx0, dx0);
    // 5.
    // x and y are formed here, by the divisions of step 3 and so with its bits, and do not travel in IcpProjection:
    // DESIGN.md 3.20 shows the generated code that read x from a register never written when they did
    const float x = g.q[0] / g.q[2], y = g.q[1] / g.q[2];
    const float iz = 1.f / g.q[2];
    const float gx = (Iu * a.camera[0]) * iz;
    const float gy = fmaf(Iu, a.camera[4], Iv * a.camera[1]) * iz;
    const float gz = -fmaf(gx, x, gy * y);
    row[0] = fmaf(g.q[1], gz, -(g.q[2] * gy));
    row[1] = fmaf(g.q[2], gx, -(g.q[0] * gz));
    row[2] = fmaf(g.q[0], gy, -(g.q[1] * gx));
    row[3] = gx;
    row[4] = gy;
    row[5] = gz;
    row[6] = frame_intensity - Im;
    return ok;
}

// One row into 28 sums: the terms of icp_rows_kernel, in its order
template <bool ROBUST>
__device__ __forceinline__ void accumulate(double (&acc)[kSums], const float (&row)[7], float huber) {
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
}

// ROBUST: one of the two thresholds is finite; the other, +inf, weights by 1.f and leaves the exact product
template <bool ROBUST>
__global__ __launch_bounds__(kIcpThreads) void icp_color_rows_kernel(
    IcpArgs a, const float* __restrict__ disparity, const float* __restrict__ intensity,
    const unsigned char* __restrict__ valid, const float* __restrict__ confidence, const float* __restrict__ normals,
    const float* __restrict__ model_depth, const float* __restrict__ model_normals,
    const float* __restrict__ model_intensity, double* __restrict__ partials, double* __restrict__ color_partials,
    float* __restrict__ rows, float huber, float color_huber) {
    __shared__ double wave_part[2][kIcpWaves][kIcpSystem];
    const int local = (int)blockIdx.x / a.tiles, tile = (int)blockIdx.x - local * a.tiles;
    const int entry = a.first + local;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pixels = a.h * a.w;
    // The entry's transform, uniform over the workgroup, is read from LDS and so lives in vector registers, of which the
    // kernel has many to spare; held in scalar registers, as icp.hip holds it, it is what made the compiler spill them
    __shared__ float T[12];
    if (tid < 12) T[tid] = a.transform[local][tid];
    __syncthreads();

    double acc[kSums], color_acc[kSums];
#pragma unroll
    for (int c = 0; c < kSums; ++c) acc[c] = color_acc[c] = 0.0;
    int count = 0, color_count = 0;
    for (int k = 0; k < kIcpPerThread; ++k) {
        const long long at = (long long)tile * kIcpTile + k * kIcpThreads + tid;   // (may pass 2^31 in the last tile)
        if (at >= pixels) break;
        const int pixel = (int)at;
        float row[7], color_row[7];
        IcpProjection g;
        const bool has = icp_row(a, T, disparity, valid, confidence, normals, model_depth, model_normals, entry, pixel, row, g);
        bool has_color = false;
        if (has)
            has_color = icp_color_row(a, g, intensity[(size_t)entry * pixels + pixel], model_depth, model_intensity, entry,
                                      color_row);
        if (rows) {
            float* out = rows + 14 * ((size_t)entry * pixels + pixel);
            const float nan = __builtin_nanf("");
#pragma unroll
            for (int c = 0; c < 7; ++c) out[c] = has ? row[c] : nan;
#pragma unroll
            for (int c = 0; c < 7; ++c) out[7 + c] = has_color ? color_row[c] : nan;
        }
        if (has) {
            accumulate<ROBUST>(acc, row, huber);
            ++count;
        }
        if (has_color) {
            accumulate<ROBUST>(color_acc, color_row, color_huber);
            ++color_count;
        }
    }
    // the wave: lane + 32, + 16, ... + 1; lane 0 holds the sum of the 64 lanes
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int c = 0; c < kSums; ++c) acc[c] += __shfl_down(acc[c], off, 64);
#pragma unroll
        for (int c = 0; c < kSums; ++c) color_acc[c] += __shfl_down(color_acc[c], off, 64);
        count += __shfl_down(count, off, 64);
        color_count += __shfl_down(color_count, off, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < kSums; ++c) {
            wave_part[0][wave][c] = acc[c];
            wave_part[1][wave][c] = color_acc[c];
        }
        wave_part[0][wave][kSums] = (double)count;
        wave_part[1][wave][kSums] = (double)color_count;
    }
    __syncthreads();
    if (tid < 2 * kIcpSystem) {
        const int which = tid >= kIcpSystem, c = tid - which * kIcpSystem;
        double sum = wave_part[which][0][c];
#pragma unroll
        for (int k = 1; k < kIcpWaves; ++k) sum += wave_part[which][k][c];
        (which ? color_partials : partials)[((size_t)entry * a.tiles + tile) * kIcpSystem + c] = sum;
    }
}

// workgroup e < batch: the geometric system of entry e; batch <= e < 2 batch: the photometric system of entry e - batch
__global__ __launch_bounds__(64) void icp_color_reduce_kernel(const double* __restrict__ partials,
                                                              const double* __restrict__ color_partials, int tiles,
                                                              int batch, int* __restrict__ system,
                                                              int* __restrict__ color_system) {
    const int c = (int)threadIdx.x;
    if (c >= kIcpSystem) return;
    const bool color = (int)blockIdx.x >= batch;
    const int entry = (int)blockIdx.x - (color ? batch : 0);
    const double* from = (color ? color_partials : partials) + (size_t)entry * tiles * kIcpSystem + c;
    double sum = 0.0;
#pragma unroll 8
    for (int t = 0; t < tiles; ++t) sum += from[(size_t)t * kIcpSystem];
    int* out = (color ? color_system : system) + 2 * ((size_t)entry * kIcpSystem + c);
    out[0] = __double2loint(sum);
    out[1] = __double2hiint(sum);
}

}  // namespace

size_t icp_color_workspace_bytes(int batch, int h, int w) { return 2 * icp_workspace_bytes(batch, h, w); }

int launch_icp_color_system(const IcpArgs& args, const float* transforms, const float* disparity, const float* intensity,
                            const unsigned char* valid, const float* confidence, const float* normals,
                            const float* model_depth, const float* model_normals, const float* model_intensity,
                            float huber, float color_huber, void* system, void* color_system, float* rows, int batch,
                            void* workspace, hipStream_t s) {
    double* partials = static_cast<double*>(workspace);
    double* color_partials = reinterpret_cast<double*>(static_cast<char*>(workspace) + icp_workspace_bytes(batch, args.h, args.w));
    const bool robust = huber < INFINITY || color_huber < INFINITY;
    for (int first = 0; first < batch; first += kIcpPoses) {
        const int entries = batch - first < kIcpPoses ? batch - first : kIcpPoses;
        IcpArgs a = args;
        a.first = first;
        for (int e = 0; e < entries; ++e)
            for (int k = 0; k < 12; ++k) a.transform[e][k] = transforms[12 * (size_t)(first + e) + k];
        const int groups = entries * a.tiles;
        const int probe = probe_before("icp_color_rows", s);
        if (robust)
            hipLaunchKernelGGL(icp_color_rows_kernel<true>, dim3(groups), dim3(kIcpThreads), 0, s, a, disparity, intensity,
                               valid, confidence, normals, model_depth, model_normals, model_intensity, partials,
                               color_partials, rows, huber, color_huber);
        else
            hipLaunchKernelGGL(icp_color_rows_kernel<false>, dim3(groups), dim3(kIcpThreads), 0, s, a, disparity, intensity,
                               valid, confidence, normals, model_depth, model_normals, model_intensity, partials,
                               color_partials, rows, huber, color_huber);
        probe_after(probe, groups, s);
        if (int rc = check_launch("icp_color_rows")) return rc;
    }
    const int probe = probe_before("icp_reduce", s);
    hipLaunchKernelGGL(icp_color_reduce_kernel, dim3(2 * batch), dim3(64), 0, s, partials, color_partials, args.tiles, batch,
                       static_cast<int*>(system), static_cast<int*>(color_system));
    probe_after(probe, 2 * batch, s);
    return check_launch("icp_reduce");
}

}  // namespace pds
