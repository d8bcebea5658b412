// C ABI of photometric tracking (include/pds_hip_photometric.h): validation without touching the GPU, then the launchers
// of intensity.hip and icp_color.hip.
#include <cmath>

#include "api_internal.hpp"

namespace {

bool overlap(const void* x, size_t xbytes, const void* y, size_t ybytes) {
    const uintptr_t p = (uintptr_t)x, q = (uintptr_t)y;
    return x && y && p < q + ybytes && q < p + xbytes;
}

// (shared by the query and the entry point; 0: refused, the message is set)
size_t icp_color_checked_bytes(int batch, int h, int w) {
    if (!(batch > 0 && h > 0 && w > 0)) {
        pds::set_error(-1, "icp_color: bad shape (%d, %d, %d)", batch, h, w);
        return 0;
    }
    if ((size_t)batch * h * w > 0x7fffffffu) {
        pds::set_error(-1, "icp_color: batch * h * w = %zu does not fit 32-bit indices", (size_t)batch * h * w);
        return 0;
    }
    return pds::icp_color_workspace_bytes(batch, h, w);
}

}  // namespace

extern "C" {

using namespace pds;

int pds_intensity_pyramid_fwd(const void* image, int image_layout, float* const* out, int levels, int batch, int h, int w,
                              pds_stream_t stream) {
    PDS_REQUIRE(image && out, "intensity_pyramid: null pointer");
    PDS_REQUIRE(batch > 0 && h > 0 && w > 0, "intensity_pyramid: bad shape (%d, %d, %d)", batch, h, w);
    PDS_REQUIRE((size_t)batch * h * w <= 0x7fffffffu, "intensity_pyramid: batch * h * w = %zu does not fit 32-bit indices",
                (size_t)batch * h * w);
    PDS_REQUIRE(image_layout >= 0 && image_layout <= 2, "intensity_pyramid: image_layout must be 0, 1 or 2 (got %d)",
                image_layout);
    PDS_REQUIRE(levels >= 1 && levels <= kIntensityLevels, "intensity_pyramid: levels must be in 1 .. %d (got %d)",
                kIntensityLevels, levels);
    PDS_REQUIRE((h >> (levels - 1)) >= 1 && (w >> (levels - 1)) >= 1, "intensity_pyramid: level %d of %d x %d is empty",
                levels - 1, w, h);
    PDS_REQUIRE(image_layout == 1 || ((uintptr_t)image & 3u) == 0, "intensity_pyramid: a 32-bit buffer is not 4-byte aligned");
    PDS_REQUIRE(intensity_groups(batch, h, w) > 0, "intensity_pyramid: the blocks do not fit one launch");
    // a workgroup reads its block of the image and writes its pixels of every level
    const size_t image_bytes = (size_t)batch * h * w * 3 * (image_layout == 1 ? 1 : 4);
    size_t bytes[kIntensityLevels];
    for (int k = 0; k < levels; ++k) {
        PDS_REQUIRE(out[k], "intensity_pyramid: null pointer");
        PDS_REQUIRE(((uintptr_t)out[k] & 3u) == 0, "intensity_pyramid: a 32-bit buffer is not 4-byte aligned");
        bytes[k] = (size_t)batch * (h >> k) * (w >> k) * 4;
        PDS_REQUIRE(!overlap(out[k], bytes[k], image, image_bytes), "intensity_pyramid: an output aliases the image");
        for (int j = 0; j < k; ++j)
            PDS_REQUIRE(!overlap(out[k], bytes[k], out[j], bytes[j]), "intensity_pyramid: an output aliases another output");
    }
    return launch_intensity_pyramid(image, image_layout, out, levels, batch, h, w, (hipStream_t)stream);
}

size_t pds_icp_color_workspace_bytes(int batch, int h, int w) { return icp_color_checked_bytes(batch, h, w); }

int pds_icp_color_system_fwd(const float* disparity, const float* intensity, const unsigned char* valid,
                             const float* confidence, float min_confidence, const float* matrix, const float* normals,
                             const float* model_depth, const float* model_normals, const float* model_intensity,
                             int model_batch, int hm, int wm, const float* camera, const float* transforms,
                             float max_distance, float min_cosine, float huber, float color_huber, double* system,
                             double* color_system, float* rows, int batch, int h, int w, void* workspace,
                             size_t workspace_bytes, pds_stream_t stream) {
    PDS_REQUIRE(disparity && intensity && matrix && model_depth && model_normals && model_intensity && camera &&
                    transforms && system && color_system && workspace,
                "icp_color: null pointer");
    PDS_REQUIRE(huber > 0.f, "icp_color: huber must be positive (got %g)", (double)huber);   // (a NaN fails)
    PDS_REQUIRE(color_huber > 0.f, "icp_color: color_huber must be positive (got %g)", (double)color_huber);
    const size_t need = icp_color_checked_bytes(batch, h, w);
    if (need == 0) return -1;
    PDS_REQUIRE(batch <= 0x3fffffff, "icp_color: 2 * batch = 2 * %d does not fit one reduce launch", batch);
    PDS_REQUIRE(model_batch == 1 || model_batch == batch, "icp_color: model_batch must be 1 or batch = %d (got %d)", batch,
                model_batch);
    PDS_REQUIRE(hm > 0 && wm > 0 && hm < (1 << 24) && wm < (1 << 24), "icp_color: bad model shape (%d, %d)", hm, wm);
    PDS_REQUIRE((size_t)model_batch * hm * wm <= 0x7fffffffu,
                "icp_color: model_batch * hm * wm = %zu does not fit 32-bit indices", (size_t)model_batch * hm * wm);
    PDS_REQUIRE(workspace_bytes >= need, "icp_color: workspace too small (%zu < %zu)", workspace_bytes, need);
    PDS_REQUIRE(!std::isnan(min_confidence), "icp_color: min_confidence is NaN");
    PDS_REQUIRE(max_distance > 0.f && std::isfinite(max_distance),
                "icp_color: max_distance must be positive and finite (got %g)", (double)max_distance);
    PDS_REQUIRE(!std::isnan(min_cosine), "icp_color: min_cosine is NaN");
    PDS_REQUIRE(((uintptr_t)disparity & 3u) == 0 && ((uintptr_t)intensity & 3u) == 0 && ((uintptr_t)confidence & 3u) == 0 &&
                    ((uintptr_t)normals & 3u) == 0 && ((uintptr_t)model_depth & 3u) == 0 &&
                    ((uintptr_t)model_normals & 3u) == 0 && ((uintptr_t)model_intensity & 3u) == 0 &&
                    ((uintptr_t)system & 3u) == 0 && ((uintptr_t)color_system & 3u) == 0 && ((uintptr_t)rows & 3u) == 0,
                "icp_color: a 32-bit buffer is not 4-byte aligned");
    PDS_REQUIRE(((uintptr_t)workspace & 7u) == 0, "icp_color: workspace is not 8-byte aligned");
    // the frame and the model are read while the partials, the systems and the rows are written
    const size_t count = (size_t)batch * h * w, model = (size_t)model_batch * hm * wm;
    const struct { const void* p; size_t bytes; } in[] = {{disparity, count * 4}, {intensity, count * 4}, {valid, count},
                                                          {confidence, count * 4}, {normals, count * 12},
                                                          {model_depth, model * 4}, {model_normals, model * 12},
                                                          {model_intensity, model * 4}},
                                                  out[] = {{system, (size_t)batch * kIcpSystem * 8},
                                                           {color_system, (size_t)batch * kIcpSystem * 8},
                                                           {rows, count * 56}, {workspace, need}};
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 8; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, in[j].p, in[j].bytes), "icp_color: an output aliases an input");
        for (int j = i + 1; j < 4; ++j)
            PDS_REQUIRE(!overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes),
                        "icp_color: an output aliases another output");
    }
    IcpArgs a = {};
    for (int k = 0; k < 16; ++k) {
        a.r.matrix[k] = matrix[k];
        PDS_REQUIRE(std::isfinite(a.r.matrix[k]), "icp_color: non-finite matrix");
    }
    a.r.min_confidence = min_confidence;
    a.r.first = 0;
    for (int k = 0; k < 5; ++k) {
        a.camera[k] = camera[k];
        PDS_REQUIRE(std::isfinite(a.camera[k]), "icp_color: non-finite camera");
    }
    PDS_REQUIRE(a.camera[0] > 0.f && a.camera[1] > 0.f, "icp_color: focal lengths must be positive (got %g, %g)",
                (double)a.camera[0], (double)a.camera[1]);
    for (size_t k = 0; k < 12 * (size_t)batch; ++k)
        PDS_REQUIRE(std::isfinite(transforms[k]), "icp_color: non-finite transform");
    a.max_distance = max_distance;
    a.min_cosine = min_cosine;
    a.h = h;
    a.w = w;
    a.hm = hm;
    a.wm = wm;
    a.model_batch = model_batch;
    a.tiles = icp_tiles(h, w);
    return launch_icp_color_system(a, transforms, disparity, intensity, valid, confidence, normals, model_depth,
                                   model_normals, model_intensity, huber, color_huber, system, color_system, rows, batch,
                                   workspace, (hipStream_t)stream);
}

}  // extern "C"
