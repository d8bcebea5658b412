// What the ordered compactions share (point_cloud.hip: the kept pixels; triangle_mesh.hip: the faces): the workgroup
// shape of a tile of kPointCloudTile flat pixels and the store of one tile's records as a contiguous run.
#pragma once
#include "common.hpp"

namespace pds {

constexpr int kPcThreads = 256;
constexpr int kPcWaves = kPcThreads / 64;
static_assert(kPointCloudTile == 4 * kPcThreads, "one quad of pixels per thread");

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

}  // namespace pds
