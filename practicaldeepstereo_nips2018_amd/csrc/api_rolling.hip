// C ABI of the rolling volume (include/pds_hip_rolling.h): validation without touching the GPU, then the launchers of
// tsdf_shift.hip and, for the leaving surface, tsdf.hip.
#include <cmath>

#include "api_internal.hpp"

namespace {

bool overlap(const void* x, size_t xbytes, const void* y, size_t ybytes) {
    const uintptr_t p = (uintptr_t)x, q = (uintptr_t)y;
    return x && y && xbytes && ybytes && p < q + ybytes && q < p + xbytes;
}

// (the limits of a volume, as every pds_tsdf_* entry point states them)
bool volume_ok(int nx, int ny, int nz) {
    if (!(nx > 0 && ny > 0 && nz > 0)) {
        pds::set_error(-1, "tsdf: bad volume (%d, %d, %d)", nx, ny, nz);
        return false;
    }
    if (nx > (1 << 24) || ny > (1 << 24) || nz > (1 << 24)) {
        pds::set_error(-1, "tsdf: a dimension above 2^24 (%d, %d, %d)", nx, ny, nz);
        return false;
    }
    if ((size_t)nx * ny > 0x7fffffffu || (size_t)nx * ny * nz > 0x7fffffffu / 3) {
        pds::set_error(-1, "tsdf: 3 * nx * ny * nz does not fit 32-bit indices (%d, %d, %d)", nx, ny, nz);
        return false;
    }
    return true;
}

}  // namespace

extern "C" {

using namespace pds;

int pds_tsdf_shift_fwd(const float* tsdf, const float* weight, const float* color, float* tsdf_out, float* weight_out,
                       float* color_out, int dx, int dy, int dz, int nx, int ny, int nz, pds_stream_t stream) {
    PDS_REQUIRE(tsdf && weight && tsdf_out && weight_out, "tsdf_shift: null pointer");
    PDS_REQUIRE((color != nullptr) == (color_out != nullptr), "tsdf_shift: color and color_out go together");
    if (!volume_ok(nx, ny, nz)) return -1;
    PDS_REQUIRE(((uintptr_t)tsdf & 3u) == 0 && ((uintptr_t)weight & 3u) == 0 && ((uintptr_t)color & 3u) == 0 &&
                    ((uintptr_t)tsdf_out & 3u) == 0 && ((uintptr_t)weight_out & 3u) == 0 &&
                    ((uintptr_t)color_out & 3u) == 0,
                "tsdf_shift: a 32-bit buffer is not 4-byte aligned");
    // out of place: a voxel's source may be written by another thread before it is read
    const size_t voxels = (size_t)nx * ny * nz;
    const struct { const void* p; size_t bytes; } in[] = {{tsdf, voxels * 4}, {weight, voxels * 4}, {color, voxels * 12}},
                                                  out[] = {{tsdf_out, voxels * 4}, {weight_out, voxels * 4},
                                                           {color_out, voxels * 12}};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, in[j].p, in[j].bytes), "tsdf_shift: an output aliases an input");
        for (int j = i + 1; j < 3; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes),
                        "tsdf_shift: an output aliases another output");
    }
    const int delta[3] = {dx, dy, dz};
    return launch_tsdf_shift(tsdf, weight, color, tsdf_out, weight_out, color_out, nx, ny, nz, delta, (hipStream_t)stream);
}

int pds_tsdf_extract_leaving_fwd(const float* tsdf, const float* weight, const float* origin, float voxel_size,
                                 float min_weight, float* points, float* normals, int* index, int* offsets,
                                 long long capacity, int nx, int ny, int nz, int dx, int dy, int dz, void* workspace,
                                 size_t workspace_bytes, pds_stream_t stream) {
    PDS_REQUIRE(tsdf && weight && origin && points && offsets && workspace, "tsdf_extract_leaving: null pointer");
    if (!volume_ok(nx, ny, nz)) return -1;
    const size_t need = tsdf_extract_workspace_bytes((long long)nx * ny * nz);
    PDS_REQUIRE(capacity >= 0, "tsdf_extract_leaving: capacity must be >= 0 (got %lld)", capacity);
    PDS_REQUIRE(workspace_bytes >= need, "tsdf_extract_leaving: workspace too small (%zu < %zu)", workspace_bytes, need);
    PDS_REQUIRE(voxel_size > 0.f && std::isfinite(voxel_size),
                "tsdf_extract_leaving: voxel_size must be positive and finite (got %g)", (double)voxel_size);
    PDS_REQUIRE(!std::isnan(min_weight), "tsdf_extract_leaving: min_weight is NaN");
    PDS_REQUIRE(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]),
                "tsdf_extract_leaving: non-finite origin");
    PDS_REQUIRE(((uintptr_t)tsdf & 3u) == 0 && ((uintptr_t)weight & 3u) == 0 && ((uintptr_t)points & 3u) == 0 &&
                    ((uintptr_t)normals & 3u) == 0 && ((uintptr_t)index & 3u) == 0 && ((uintptr_t)offsets & 3u) == 0 &&
                    ((uintptr_t)workspace & 3u) == 0,
                "tsdf_extract_leaving: a 32-bit buffer is not 4-byte aligned");
    // the scatter pass reads the volume again after rows have been written
    const size_t voxels = (size_t)nx * ny * nz, rows = (size_t)capacity;
    const struct { const void* p; size_t bytes; } in[] = {{tsdf, voxels * 4}, {weight, voxels * 4}},
                                                  out[] = {{points, rows * 12},
                                                           {normals, rows * 12},
                                                           {index, rows * 4},
                                                           {offsets, 8},
                                                           {workspace, need}};
    for (int i = 0; i < 5; ++i) {
        for (int j = 0; j < 2; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, in[j].p, in[j].bytes),
                        "tsdf_extract_leaving: an output aliases an input");
        for (int j = i + 1; j < 5; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes),
                        "tsdf_extract_leaving: an output aliases another output");
    }
    const int delta[3] = {dx, dy, dz};
    return launch_tsdf_extract_leaving(tsdf, weight, origin, voxel_size, min_weight, delta, points, normals, index,
                                       offsets, capacity, nx, ny, nz, workspace, (hipStream_t)stream);
}

}  // extern "C"
