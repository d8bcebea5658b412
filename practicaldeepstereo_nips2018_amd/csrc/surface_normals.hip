// Surface normals from disparity by an edge-aware plane fit (pds_surface_normals_fwd; not in the reference).
//
// Per image and per pixel p = (x0, y0) with d0 = D[p]: W(p) = the eligible pixels q (D finite and > 0, valid,
// confidence >= min_confidence) of the k x k window around p, clipped at the border, with fabsf(D[q] - d0) <=
// max_difference; the least-squares plane delta = a i + b j + c0 through (i, j, delta(q) = D[q] - d0) over W(p); its
// image under the matrix is a 3-D plane, whose unit normal, turned towards the viewpoint, is the output
// (include/pds_hip.h has the formulas).  p is degenerate -- fill_value, valid_out = 0 -- when reproject_one (reproject.hpp,
// the function behind pds_reproject_fwd) does not keep it, |W(p)| < min_valid, the pixels of W(p) are collinear (det == 0,
// decided in integers), or the point or the normal does not exist.
//
// One launch, no atomics, no workspace, no traffic between workgroups.  A workgroup of 256 threads owns a tile of
// kNormalsTileW x kNormalsTileH = 64 x 16 pixels (median.hip's tile):
//   staging    the tile plus a halo of r = k / 2 pixels goes to LDS once, with eligibility folded in: a pixel that is not
//              eligible or lies outside the image becomes NaN, and NaN fails the test on delta by itself, so a tap is one
//              LDS value, one subtraction and one comparison.  The mask and confidence bytes are paid here, once per pixel.
//   fit        a thread produces four neighbouring pixels of one row.  Per window row it reads the k + 3 values its four
//              windows share as aligned 16-byte LDS reads (the row stride is a multiple of four floats) and, per pixel,
//              forms the row's sums of 1, i, i^2 (integers) and delta, i delta (fp32) with compile-time i; a row then
//              enters the window's sums with its compile-time j: Sj += j * n_row, Sij += j * Si_row, Sjd += j * Sd_row
//              ...  The loops are templated on k and fully unrolled.  n, Si .. Sjj and det are exact integers.
//   stores     the 12-byte records of a tile row are contiguous in memory: they are staged in LDS, shifted by the
//              misalignment of the row's first byte (point_cloud.hip's scheme), and leave as 16-byte stores wherever the
//              OUTPUT address is 16-byte aligned, element stores for the head and the tail of the row.  A pointer that is
//              only 4-byte aligned, or a width that is no multiple of four, changes the shift and nothing else.  The
//              valid bytes go out as uchar4 where w % 4 == 0 and the pointer is 4-byte aligned, one by one otherwise.
#include "common.hpp"

namespace pds {

namespace {

constexpr int kNormalsTileW = 64;
constexpr int kNormalsTileH = 16;
constexpr int kNormalsThreads = 256;
constexpr int kNormalsPerThread = 4;                          // neighbouring pixels of one row per thread
constexpr int kNormalsRowBytes = 12 * kNormalsTileW + 16;     // a staged output row and room for its shift
constexpr int kNormalsRowChunks = kNormalsRowBytes / 16;

static_assert(kNormalsTileW / kNormalsPerThread * kNormalsTileH == kNormalsThreads, "one thread per four pixels of the tile");
static_assert(kNormalsRowBytes % 16 == 0, "staged rows keep the 16-byte alignment");

struct PlaneSums {
    int n, si, sj, sii, sij, sjj;
    float sd, sid, sjd;
};

// The normal at pixel (x, y) with centre disparity d0 from the sums over its window; false: degenerate
__device__ __forceinline__ bool normal_of(const SurfaceNormalsArgs& a, const PlaneSums& s, bool kept, int x, int y,
                                          float d0, float (&N)[3]) {
    const int A = s.n * s.sii - s.si * s.si, Bm = s.n * s.sij - s.si * s.sj, C = s.n * s.sjj - s.sj * s.sj;
    const int det = A * C - Bm * Bm;
    if (!kept || s.n < a.min_valid || det == 0) return false;
    const float u = (float)s.n * s.sid - (float)s.si * s.sd, v = (float)s.n * s.sjd - (float)s.sj * s.sd;
    const float fdet = (float)det;
    const float pa = ((float)C * u - (float)Bm * v) / fdet, pb = ((float)A * v - (float)Bm * u) / fdet;
    const float c0 = (s.sd - pa * (float)s.si - pb * (float)s.sj) / (float)s.n;
    const float dh = d0 + c0, fx = (float)x, fy = (float)y;
    const float* M = a.r.matrix;
    const float Hw = M[12] * fx + M[13] * fy + M[14] * dh + M[15];
    if (!(Hw > 0.f) || !isfinite(Hw)) return false;
    float X[3], tx[3], ty[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        X[c] = (M[4 * c] * fx + M[4 * c + 1] * fy + M[4 * c + 2] * dh + M[4 * c + 3]) / Hw;
        const float along_d = M[4 * c + 2] - X[c] * M[14];
        tx[c] = (M[4 * c] - X[c] * M[12]) + pa * along_d;
        ty[c] = (M[4 * c + 1] - X[c] * M[13]) + pb * along_d;
    }
    N[0] = tx[1] * ty[2] - tx[2] * ty[1];
    N[1] = tx[2] * ty[0] - tx[0] * ty[2];
    N[2] = tx[0] * ty[1] - tx[1] * ty[0];
    const float norm2 = N[0] * N[0] + N[1] * N[1] + N[2] * N[2];
    if (!(norm2 > 0.f) || !isfinite(norm2)) return false;
    const float norm = sqrtf(norm2);
    const float facing = N[0] * (X[0] - a.viewpoint[0]) + N[1] * (X[1] - a.viewpoint[1]) + N[2] * (X[2] - a.viewpoint[2]);
    const float sign = facing > 0.f ? -1.f : 1.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) N[c] = sign * (N[c] / norm) + 0.f;   // (+ 0: a -0 leaves as +0)
    return true;
}

// grid: batch * tiles_y * tiles_x workgroups
template <int KS>
__global__ __launch_bounds__(kNormalsThreads) void surface_normals_kernel(
    SurfaceNormalsArgs a, const float* __restrict__ disparity, const unsigned char* __restrict__ valid,
    const float* __restrict__ confidence, float* __restrict__ normals, unsigned char* __restrict__ valid_out, int h, int w,
    int tiles_x, int tiles_y, int vec_valid) {
    constexpr int R = KS / 2, LW = (kNormalsTileW + 2 * R + 3) & ~3, LH = kNormalsTileH + 2 * R;
    constexpr int SPAN = KS + kNormalsPerThread - 1, QUADS = (SPAN + 3) / 4;   // values / 16-byte reads per window row
    static_assert((kNormalsTileW / kNormalsPerThread - 1) * kNormalsPerThread + 4 * QUADS <= LW, "the reads stay in the row");
    __shared__ alignas(16) float tile[LH * LW];
    __shared__ alignas(16) unsigned char staged[kNormalsTileH * kNormalsRowBytes];
    const int t = blockIdx.x % (tiles_x * tiles_y), b = blockIdx.x / (tiles_x * tiles_y);
    const int y0 = (t / tiles_x) * kNormalsTileH, x0 = (t % tiles_x) * kNormalsTileW;
    const size_t image = (size_t)b * h * w;

    for (int i = threadIdx.x; i < LH * LW; i += kNormalsThreads) {
        const int gy = y0 - R + i / LW, gx = x0 - R + i % LW;
        float v = __builtin_nanf("");
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
            const size_t p = image + (size_t)gy * w + gx;
            const float d = disparity[p];
            bool ok = isfinite(d) && d > 0.f;
            if (valid) ok = ok && valid[p] != 0;
            if (confidence) ok = ok && confidence[p] >= a.r.min_confidence;   // (a NaN confidence fails too)
            if (ok) v = d;
        }
        tile[i] = v;
    }
    __syncthreads();

    const int tx = threadIdx.x % (kNormalsTileW / kNormalsPerThread), ty = threadIdx.x / (kNormalsTileW / kNormalsPerThread);
    const int x = x0 + tx * kNormalsPerThread, y = y0 + ty;
    if (y < h && x < w) {
        const float* corner = tile + ty * LW + tx * kNormalsPerThread;   // the top left corner of the first window
        float row[4 * QUADS], d0[kNormalsPerThread];
        PlaneSums s[kNormalsPerThread];
#pragma unroll
        for (int v = 0; v < QUADS; ++v) {
            const float4 f = *reinterpret_cast<const float4*>(corner + R * LW + 4 * v);
            row[4 * v] = f.x; row[4 * v + 1] = f.y; row[4 * v + 2] = f.z; row[4 * v + 3] = f.w;
        }
#pragma unroll
        for (int q = 0; q < kNormalsPerThread; ++q) {
            d0[q] = row[q + R];
            s[q] = PlaneSums{0, 0, 0, 0, 0, 0, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int jj = 0; jj < KS; ++jj) {
            const int j = jj - R;
#pragma unroll
            for (int v = 0; v < QUADS; ++v) {
                const float4 f = *reinterpret_cast<const float4*>(corner + jj * LW + 4 * v);
                row[4 * v] = f.x; row[4 * v + 1] = f.y; row[4 * v + 2] = f.z; row[4 * v + 3] = f.w;
            }
#pragma unroll
            for (int q = 0; q < kNormalsPerThread; ++q) {
                int rn = 0, ri = 0, rii = 0;
                float rd = 0.f, rid = 0.f;
#pragma unroll
                for (int ii = 0; ii < KS; ++ii) {
                    const int i = ii - R;
                    const float delta = row[q + ii] - d0[q];
                    const bool in = fabsf(delta) <= a.max_difference;   // (false for NaN: not eligible, or outside)
                    const int one = in ? 1 : 0;
                    const float dm = in ? delta : 0.f;
                    rn += one;
                    ri += i * one;
                    rii += i * i * one;
                    rd += dm;
                    rid += (float)i * dm;
                }
                s[q].n += rn;
                s[q].si += ri;
                s[q].sii += rii;
                s[q].sj += j * rn;
                s[q].sij += j * ri;
                s[q].sjj += j * j * rn;
                s[q].sd += rd;
                s[q].sid += rid;
                s[q].sjd += (float)j * rd;
            }
        }

        // the row's first byte in memory decides the shift of its staged copy (the store loop below derives the same)
        const size_t row_pixel = image + (size_t)y * w + x0;
        const int shift = (int)(((uintptr_t)normals + 12 * row_pixel) & 15);
        float* out = reinterpret_cast<float*>(staged + ty * kNormalsRowBytes + shift) + 3 * tx * kNormalsPerThread;
        unsigned char good[kNormalsPerThread];
#pragma unroll
        for (int q = 0; q < kNormalsPerThread; ++q) {
            float N[3];
            bool ok = false;
            if (x + q < w) {
                const int p = (int)(row_pixel + tx * kNormalsPerThread + q);   // (batch * h * w fits int)
                const Point3 point = reproject_one(a.r, valid, confidence, p, d0[q], h, w);
                ok = normal_of(a, s[q], point.x == point.x, x + q, y, d0[q], N);
            }
            good[q] = ok ? 1 : 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) out[3 * q + c] = ok ? N[c] : a.fill_value;
        }
        if (valid_out) {
            unsigned char* flags = valid_out + image + (size_t)y * w + x;
            if (vec_valid) {
                // (w % 4 == 0 and x % 4 == 0: the four pixels are inside the row together)
                *reinterpret_cast<uchar4*>(flags) = make_uchar4(good[0], good[1], good[2], good[3]);
            } else {
#pragma unroll
                for (int q = 0; q < kNormalsPerThread; ++q)
                    if (x + q < w) flags[q] = good[q];
            }
        }
    }
    __syncthreads();

    // staged[row][shift + j] -> the row's bytes [0, 12 * columns) in memory; shift = their address & 15, so a staged
    // chunk and the memory it goes to are 16-byte aligned together
    const int columns = w - x0 < kNormalsTileW ? w - x0 : kNormalsTileW;
    for (int c = threadIdx.x; c < kNormalsTileH * kNormalsRowChunks; c += kNormalsThreads) {
        const int r = c / kNormalsRowChunks, lo = 16 * (c % kNormalsRowChunks);
        if (y0 + r >= h) break;
        unsigned char* dst = reinterpret_cast<unsigned char*>(normals) + 12 * (image + (size_t)(y0 + r) * w + x0);
        const int shift = (int)((uintptr_t)dst & 15), end = shift + 12 * columns;
        if (lo >= end) continue;
        const unsigned char* lds = staged + r * kNormalsRowBytes;
        unsigned char* g = dst - shift;
        if (lo >= shift && lo + 16 <= end) {
            *reinterpret_cast<uint4*>(g + lo) = *reinterpret_cast<const uint4*>(lds + lo);
        } else {
            const int from = lo > shift ? lo : shift, to = lo + 16 < end ? lo + 16 : end;
            for (int j = from; j < to; j += 4)
                *reinterpret_cast<unsigned*>(g + j) = *reinterpret_cast<const unsigned*>(lds + j);
        }
    }
}

}  // namespace

// batch * h * w fits int (checked by the entry point), so the number of tiles does
int launch_surface_normals(const SurfaceNormalsArgs& a, const float* disparity, const unsigned char* valid,
                           const float* confidence, float* normals, unsigned char* valid_out, int batch, int h, int w,
                           int kernel_size, hipStream_t s) {
    const int tiles_x = (w + kNormalsTileW - 1) / kNormalsTileW, tiles_y = (h + kNormalsTileH - 1) / kNormalsTileH;
    const long long grid = (long long)batch * tiles_x * tiles_y;
    if (grid > 0x7fffffffLL) return set_error(-1, "surface_normals: %lld tiles do not fit one launch", grid);
    const int vec_valid = w % 4 == 0 && ((uintptr_t)valid_out & 3) == 0;
    const int probe = probe_before("surface_normals", s);
#define PDS_NORMALS(K)                                                                                                  \
    hipLaunchKernelGGL((surface_normals_kernel<K>), dim3((int)grid), dim3(kNormalsThreads), 0, s, a, disparity, valid, \
                       confidence, normals, valid_out, h, w, tiles_x, tiles_y, vec_valid)
    if (kernel_size == 3) PDS_NORMALS(3);
    else if (kernel_size == 5) PDS_NORMALS(5);
    else PDS_NORMALS(7);
#undef PDS_NORMALS
    probe_after(probe, (int)grid, s);
    return check_launch("surface_normals");
}

}  // namespace pds
