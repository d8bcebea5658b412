// The rolling volume's shift (pds_tsdf_shift_fwd; Kintinuous; not in the reference): the dense volume follows the rig by
// whole voxels.  Out of place, for tsdf and weight [nz, ny, nx] and, where given, color [nz, ny, nx, 3]:
//   out voxel (i, j, k) = in voxel (i + dx, j + dy, k + dz)   where that lies inside the volume  (the voxel STAYS)
//                       = tsdf 1.0f, weight 0.0f, colour 0.0f   elsewhere                          (the voxel ENTERS)
// A voxel that stays has its source at the constant flat offset off = (dz * ny + dy) * nx + dx (3 * off for the colour),
// so the kernel is a streaming copy under a mask: three ranges [lo_a, hi_a) of the output's (i, j, k), found on the host
// (tsdf_shift_range; a |d_a| >= n_a empties them, and then off is not used and passed as 0).  The words are moved as
// 32-bit integers: NaN payloads and -0.0 survive.
//
// ONE launch, tsdf_shift, for the two or three tensors; no workspace, no atomics, no workgroup waits on another, each
// output voxel belongs to one thread.  The work is that of tsdf_integrate (tsdf.hip): the volume as one row of voxels cut
// into quads of four consecutive OUTPUT voxels that begin on a 16-byte boundary of the outputs (misalignment `mis` in
// elements: quad q = voxels [4 q - mis, 4 q - mis + 4), the first and the last may be partial), one quad per thread and
// step, 256 threads, a grid-stride loop over at most kTsdfShiftMaxGroups workgroups.  A whole quad whose four voxels all
// stay, or all enter, is one 16-byte store per tensor and three for the colour; a mixed or partial quad goes voxel by
// voxel.  Three forms, chosen once per launch on the host:
//   FORM 2  16-byte loads.  The source of a quad sits at (in + first + off), whose misalignment against 16 bytes,
//           (in's - mis + off) mod 4 elements, is the same for every quad of the launch: this form where it is 0 for tsdf
//           and weight (and (in's + mis - off) mod 4 = 0 for the colour, whose quad is 12 floats at 3 (first + off)).
//   FORM 1  dword loads, 16-byte stores: any other source misalignment, tsdf and weight each with its own.  The four
//           (twelve) loads of a lane are consecutive words and the lanes of a wave read consecutive quads, so every cache
//           line is still fetched once; two aligned 16-byte loads and a select would touch the 16 bytes before or behind
//           the source of the first or last quad that stays, which the bound below forbids.
//   FORM 0  voxel by voxel: the outputs disagree in their misalignment (tsdf against weight, or the colour's quads do not
//           begin on a 16-byte boundary where those of tsdf do, (color_out's + mis) mod 4 != 0), so no quad fits them all.
//
// THE BOUND: no byte outside [in, in + 4 total) of tsdf or weight, or [color, color + 12 total) of the colour, is read.
//   * A voxel is read only where it stays.  (i, j, k) stays iff (i + dx, j + dy, k + dz) lies inside the volume, and
//     then v + off is that voxel's flat index, in [0, total): a dword load at in + v + off, and the three of the colour at
//     color + 3 (v + off) + {0, 1, 2}, lie inside.  Voxels that enter are never read.
//   * A 16-byte load happens only in FORM 2 and only for a whole quad whose FOUR voxels stay: its 16 bytes are exactly
//     the four words at v + off .. v + 3 + off, each inside by the line above (the 48 bytes of the colour likewise), and
//     FORM 2 is chosen only where that address is 16-byte aligned.  No load is widened, rounded down to a boundary or
//     issued for a partial quad, so a state tensor may be a view at any 4-byte offset into an exactly-sized allocation.
//   * Stores: a 16-byte store is issued only for a whole quad, first >= 0 and first + 4 <= total, at out + first.
#include "tsdf_surface.hpp"

namespace pds {

namespace {

constexpr int kShiftThreads = 256;
constexpr unsigned kEmptyTsdf = 0x3f800000u;   // 1.0f; weight and colour: 0

template <int FORM>
__device__ __forceinline__ uint4 load_words(const unsigned* __restrict__ p) {
    if constexpr (FORM == 2) return *reinterpret_cast<const uint4*>(p);
    return make_uint4(p[0], p[1], p[2], p[3]);
}

template <int FORM, bool COLOR>
__global__ __launch_bounds__(kShiftThreads) void tsdf_shift_kernel(
    TsdfShiftRange r, const unsigned* __restrict__ tsdf_in, const unsigned* __restrict__ weight_in,
    const unsigned* __restrict__ color_in, unsigned* __restrict__ tsdf_out, unsigned* __restrict__ weight_out,
    unsigned* __restrict__ color_out, int nx, int ny, int total, int off, int mis, int quads) {
    for (int q = blockIdx.x * kShiftThreads + (int)threadIdx.x; q < quads; q += gridDim.x * kShiftThreads) {
        const int first = 4 * q - mis;   // (3 * total < 2^31: no overflow)
        const int lo = first < 0 ? 0 : first, hi = first + 4 < total ? first + 4 : total;
        VoxelAt at = VoxelAt::from_flat(lo, nx, ny);
        unsigned stays = 0;   // bit e: voxel first + e exists and stays
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (first + e >= lo && first + e < hi) {
                if (at.i >= r.lo[0] && at.i < r.hi[0] && at.j >= r.lo[1] && at.j < r.hi[1] && at.k >= r.lo[2] &&
                    at.k < r.hi[2])
                    stays |= 1u << e;
                at.next(nx, ny);
            }
        }
        const bool whole = hi - lo == 4;
        if (FORM > 0 && whole && stays == 0xfu) {
            // (the four sources are the words first + off .. first + off + 3, all inside: see THE BOUND)
            const int from = first + off;
            const uint4 t = load_words<FORM>(tsdf_in + from), w = load_words<FORM>(weight_in + from);
            *reinterpret_cast<uint4*>(tsdf_out + first) = t;
            *reinterpret_cast<uint4*>(weight_out + first) = w;
            if constexpr (COLOR) {
                const unsigned* c = color_in + 3 * from;
                const uint4 c0 = load_words<FORM>(c), c1 = load_words<FORM>(c + 4), c2 = load_words<FORM>(c + 8);
                uint4* o = reinterpret_cast<uint4*>(color_out + 3 * first);
                o[0] = c0;
                o[1] = c1;
                o[2] = c2;
            }
        } else if (FORM > 0 && whole && stays == 0u) {
            *reinterpret_cast<uint4*>(tsdf_out + first) = make_uint4(kEmptyTsdf, kEmptyTsdf, kEmptyTsdf, kEmptyTsdf);
            *reinterpret_cast<uint4*>(weight_out + first) = make_uint4(0u, 0u, 0u, 0u);
            if constexpr (COLOR) {
                uint4* o = reinterpret_cast<uint4*>(color_out + 3 * first);
                o[0] = o[1] = o[2] = make_uint4(0u, 0u, 0u, 0u);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int v = first + e;
                if (v >= lo && v < hi) {
                    unsigned t = kEmptyTsdf, w = 0u, c[3] = {0u, 0u, 0u};
                    if (stays >> e & 1u) {   // (the only loads of this branch: a voxel that enters is not read)
                        t = tsdf_in[v + off];
                        w = weight_in[v + off];
                        if constexpr (COLOR) {
#pragma unroll
                            for (int m = 0; m < 3; ++m) c[m] = color_in[3 * (v + off) + m];
                        }
                    }
                    tsdf_out[v] = t;
                    weight_out[v] = w;
                    if constexpr (COLOR) {
#pragma unroll
                        for (int m = 0; m < 3; ++m) color_out[3 * v + m] = c[m];
                    }
                }
            }
        }
    }
}

inline int words_off_16(const void* p) { return (int)(((uintptr_t)p & 15u) / sizeof(float)); }
inline int mod4(long long x) { return (int)(((x % 4) + 4) % 4); }

}  // namespace

TsdfShiftRange tsdf_shift_range(int nx, int ny, int nz, const int* delta, bool output) {
    const int n[3] = {nx, ny, nz};
    TsdfShiftRange r;
    bool empty = false;
    for (int a = 0; a < 3; ++a) {
        const long long d = output ? (long long)delta[a] : -(long long)delta[a];   // the voxels i with 0 <= i + d < n
        const long long lo = d < 0 ? -d : 0, hi = d > 0 ? n[a] - d : n[a];
        r.lo[a] = (int)(lo < n[a] ? lo : n[a]);
        r.hi[a] = (int)(hi > 0 ? hi : 0);
        empty = empty || r.lo[a] >= r.hi[a];
    }
    if (empty)
        for (int a = 0; a < 3; ++a) r.lo[a] = r.hi[a] = 0;
    return r;
}

int tsdf_shift_groups(long long voxels, int misalignment) {
    const long long quads = (voxels + misalignment + 3) / 4;
    const long long groups = (quads + kShiftThreads - 1) / kShiftThreads;
    return (int)(groups < kTsdfShiftMaxGroups ? groups : kTsdfShiftMaxGroups);
}

int launch_tsdf_shift(const float* tsdf_in, const float* weight_in, const float* color_in, float* tsdf_out,
                      float* weight_out, float* color_out, int nx, int ny, int nz, const int* delta, hipStream_t s) {
    const int total = nx * ny * nz;
    const TsdfShiftRange r = tsdf_shift_range(nx, ny, nz, delta, true);
    // (something stays: |d_a| < n_a on every axis, so |off| < total)
    const long long off = r.hi[0] > r.lo[0] ? ((long long)delta[2] * ny + delta[1]) * nx + delta[0] : 0;
    const bool color = color_in != nullptr;
    // FORM 0 unless one grid of quads fits every output
    bool quads_fit = words_off_16(tsdf_out) == words_off_16(weight_out);
    const int mis = quads_fit ? words_off_16(tsdf_out) : 0;
    if (color) quads_fit = quads_fit && mod4(words_off_16(color_out) + mis) == 0;
    // FORM 2 where every source quad begins on a 16-byte boundary
    bool aligned = mod4(words_off_16(tsdf_in) - mis + off) == 0 && mod4(words_off_16(weight_in) - mis + off) == 0;
    if (color) aligned = aligned && mod4(words_off_16(color_in) + mis - off) == 0;
    const int form = !quads_fit ? 0 : (aligned ? 2 : 1);
    const int quads = (int)(((long long)total + mis + 3) / 4);
    const auto kernel = color ? (form == 2   ? tsdf_shift_kernel<2, true>
                                 : form == 1 ? tsdf_shift_kernel<1, true>
                                             : tsdf_shift_kernel<0, true>)
                              : (form == 2   ? tsdf_shift_kernel<2, false>
                                 : form == 1 ? tsdf_shift_kernel<1, false>
                                             : tsdf_shift_kernel<0, false>);
    return launch_probed("tsdf_shift", kernel, tsdf_shift_groups(total, mis), kShiftThreads, s, r,
                         reinterpret_cast<const unsigned*>(tsdf_in), reinterpret_cast<const unsigned*>(weight_in),
                         reinterpret_cast<const unsigned*>(color_in), reinterpret_cast<unsigned*>(tsdf_out),
                         reinterpret_cast<unsigned*>(weight_out), reinterpret_cast<unsigned*>(color_out), nx, ny, total,
                         (int)off, mis, quads);
}

}  // namespace pds
