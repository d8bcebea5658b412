/* Photometric tracking: the entry points of colour ICP on the coloured raycast (not in the reference).
 * An extension of pds_hip.h under the same ABI version: pds_hip.h, pds_hip_tracking.h and the tables of their symbols stay
 * as they were, and a caller that does not track with colour needs neither this file nor its symbols. */
#ifndef PDS_HIP_PHOTOMETRIC_H
#define PDS_HIP_PHOTOMETRIC_H

#include "pds_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * Intensity pyramid: luma and up to three halvings in one launch                    not in the reference
 * Additive: ABI version unchanged.  The frame and model images of photometric tracking.
 * image: image_layout 0: float32 [batch, 3, h, w]; 1: uint8 [batch, h, w, 3]; 2: float32 [batch, h, w, 3] (the layout
 * of the colours of pds_tsdf_color_render_fwd).  Values are taken as they are, not rescaled.  out: host array of `levels`
 * device pointers, 1 <= levels <= 4, h >> (levels - 1) >= 1 and w >> (levels - 1) >= 1; out[k] receives level k,
 * [batch, h >> k, w >> k] fp32.  Everything is fp32 without contraction:
 *   level 0      L = fmaf(0.299f, c0, fmaf(0.587f, c1, 0.114f * c2)) of the three channels; a NaN channel gives NaN
 *   level l + 1  ((a00 + a01) + (a10 + a11)) * 0.25f over the four children (row, column) of level l; NaN propagates
 * Sizes floor, a last odd row or column is dropped.  Pixel centres are integers, so the pixel (x', y') of level l + 1 sits
 * at (2 x' + 0.5, 2 y' + 0.5) of level l: the convention of pds_disparity_pyramid_fwd.  batch * h * w <= 2^31 - 1 and at
 * most 2^24 blocks of 32 x 32, batch * ceil(h / 32) * ceil(w / 32) (a launch holds at most 2^32 threads); float
 * buffers 4-byte aligned (16-byte accesses are used where w % 4 == 0 and the pointers allow).  No output may overlap the
 * image or another output.  One launch on `stream`, a workgroup per 32 x 32 block, no workspace, no atomics, no host
 * synchronisation: the same bits on every run and stream.
 * ---------------------------------------------------------------------------------- */
int pds_intensity_pyramid_fwd(const void* image, int image_layout,
                              float* const* out /* host, [levels] device pointers */, int levels, int batch, int h, int w,
                              pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Point-to-plane plus photometric system                                            not in the reference
 * Additive: ABI version unchanged.
 * pds_icp_color_system_fwd: the arguments of pds_icp_system_robust_fwd (pds_hip_tracking.h) plus the frame's
 * `intensity` [batch, h, w] fp32, the model's `model_intensity` [model_batch, hm, wm] fp32 (level 0 of
 * pds_intensity_pyramid_fwd on the colours of the raycast), `color_huber` and `color_system`.  huber and color_huber are
 * > 0; +inf means exact products (the unweighted sums).
 *
 * The geometric row of a pixel is that of pds_icp_system_fwd, steps 1 - 7, by the same device code; `system` [batch, 29]
 * has the bits pds_icp_system_robust_fwd gives on the same arguments (those of pds_icp_system_fwd with huber = +inf).
 *
 * The photometric row exists only where the geometric row exists, and only where all of this holds (fp32, every
 * multiply-add an explicit fmaf, no contraction); q, x = q_x / q_z, y = q_y / q_z, u and v are those of step 3:
 *   1. I_f = intensity[p] is not NaN
 *   2. x0 = floorf(u), y0 = floorf(v), a = u - x0, b = v - y0; no row unless 0 <= x0, x0 + 1 <= wm - 1, 0 <= y0,
 *      y0 + 1 <= hm - 1
 *   3. the taps L00, L10 (x0 + 1), L01 (y0 + 1), L11 of model_intensity and the model depths Z00 .. Z11 at the same taps;
 *      no row where any of the eight is NaN, or unless |Z_tap - q_z| <= max_distance for all four (the same surface)
 *   4. top = fmaf(a, L10 - L00, L00), bot = fmaf(a, L11 - L01, L01), I_m = fmaf(b, bot - top, top),
 *      I_u = fmaf(b, (L11 - L01) - (L10 - L00), L10 - L00), I_v = bot - top: the bilinear patch and its own derivative
 *   5. r_c = I_f - I_m; iz = 1 / q_z, g_x = (I_u fx) iz, g_y = fmaf(I_u, skew, I_v fy) iz, g_z = -fmaf(g_x, x, g_y y);
 *      J_c = (q x g, g) with (q x g)_x = fmaf(q_y, g_z, -(q_z g_y)) and its cyclic successors.
 *      The row is (J_c0 .. J_c5, r_c), unscaled, in intensity units.
 * Sign: with q <- q + omega x q + v the residual becomes r_c - J_c (omega, v) to first order, so both systems minimise
 * sum (r - J xi)^2 over the same xi and may be added after scaling the photometric one by the square of a weight in
 * metres per intensity level.
 *
 * color_system [batch, 29]: the 29 sums of pds_icp_system_robust_fwd over the photometric rows, weighted by
 * w = |r_c| <= color_huber ? 1.f : color_huber / |r_c|; slot 28 is the unweighted photometric row count.  The order of
 * the additions is that of pds_icp_system_fwd (thread, wave fold, waves, tiles); no atomics: the same bits on every run
 * and stream.  rows (or NULL) [batch, h, w, 14]: the geometric row then the photometric row of every pixel, seven NaNs
 * each where absent.  workspace: pds_icp_color_workspace_bytes(batch, h, w) = 2 * pds_icp_workspace_bytes(batch, h, w)
 * bytes, 8-byte aligned (0: refused, see pds_last_error).  One launch of the rows kernel per 16 entries and one reduce
 * launch on `stream`; no host synchronisation.  Nothing written may overlap anything read or written.
 * ---------------------------------------------------------------------------------- */
size_t pds_icp_color_workspace_bytes(int batch, int h, int w);
int pds_icp_color_system_fwd(const float* disparity, const float* intensity, const unsigned char* valid /* or NULL */,
                             const float* confidence /* or NULL */, float min_confidence,
                             const float* matrix /* host, [16] */, const float* normals /* or NULL */,
                             const float* model_depth, const float* model_normals, const float* model_intensity,
                             int model_batch, int hm, int wm, const float* camera /* host, [5] */,
                             const float* transforms /* host, [batch][12] */, float max_distance, float min_cosine,
                             float huber, float color_huber, double* system, double* color_system,
                             float* rows /* or NULL */, int batch, int h, int w, void* workspace, size_t workspace_bytes,
                             pds_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PDS_HIP_PHOTOMETRIC_H */
