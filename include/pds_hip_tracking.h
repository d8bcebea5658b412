/* Coarse-to-fine, robust tracking: the entry points added beside pds_icp_system_fwd (not in the reference).
 * An extension of pds_hip.h under the same ABI version: pds_hip.h and the table of its symbols stay as they were, and a
 * caller that does not track on a pyramid or with weights needs neither this file nor its symbols. */
#ifndef PDS_HIP_TRACKING_H
#define PDS_HIP_TRACKING_H

#include "pds_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * Huber-weighted point-to-plane system                                              not in the reference
 * Additive: ABI version unchanged.
 * pds_icp_system_robust_fwd: the arguments of pds_icp_system_fwd (pds_hip.h) plus `huber` (> 0; +inf allowed), the same
 * two kernels.  Steps 1 - 7 and the row are unchanged.  The weight of a row is w = |r| <= huber ? 1.f : huber / |r| in fp32, and every term of the first
 * 28 sums becomes fma((double)w, (double)a * (double)b, sum): the inner product is exact in fp64, so the weight adds one
 * rounding per term.  Slot 27 is sum w r^2; slot 28 stays the unweighted row count; the order of the additions is
 * unchanged.  With huber = +inf the system has the bits pds_icp_system_fwd gives.  A x = g with these sums is one step of
 * iteratively reweighted least squares.
 * ---------------------------------------------------------------------------------- */
int pds_icp_system_robust_fwd(const float* disparity, const unsigned char* valid /* or NULL */,
                              const float* confidence /* or NULL */, float min_confidence,
                              const float* matrix /* host, [16] */, const float* normals /* or NULL */,
                              const float* model_depth, const float* model_normals, int model_batch, int hm, int wm,
                              const float* camera /* host, [5] */, const float* transforms /* host, [batch][12] */,
                              float max_distance, float min_cosine, float huber, double* system,
                              float* rows /* or NULL */, int batch, int h, int w, void* workspace,
                              size_t workspace_bytes, pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Disparity pyramid: up to three edge- and hole-aware halvings in one launch        not in the reference
 * Additive: ABI version unchanged.  The frame side of coarse-to-fine tracking.  disparity [batch, h, w] fp32 is level
 * `source_level` of a pyramid; out[k] (host array of `levels` device pointers, 1 <= levels <= 3) receives level
 * source_level + k + 1, [batch, h >> (k + 1), w >> (k + 1)] fp32: sizes floor, a last odd row or column is dropped, and
 * h >> levels, w >> levels must be >= 1.  A pixel is formed from its four children one level below, taken in the order
 * (0,0), (0,1), (1,0), (1,1) (row, column), in fp32 without contraction:
 *   eligible   source_level == 0, the children of out[0]: isfinite(d) && d > 0 && (valid == NULL || valid[p] != 0) &&
 *              (confidence == NULL || confidence[p] >= min_confidence) (a NaN confidence fails): the mask of
 *              pds_reproject_fwd less its matrix test.  Every other child: it is not NaN (valid and confidence are
 *              not read when source_level > 0)
 *   m          the largest eligible child: the foreground wins, a block astride a depth edge is not averaged across
 *   members    the eligible children with m - c <= max_difference (one fp32 subtraction)
 *   value      the sum of the members in child order divided by their count; NaN without a member
 * Values stay in the units of the source.  Pixel centres are integers, so the pixel (x', y') of out[k] sits at
 * 2^(k+1) x' + (2^(k+1) - 1) / 2 of the source.  max_difference finite and >= 0, min_confidence not NaN, batch * h * w
 * <= 2^31 - 1, 4-byte alignment (16-byte loads are used where w % 4 == 0 and the pointers allow).  No output may overlap an
 * input or another output.  One launch on `stream`, a workgroup per 32 x 32 block of the source, no workspace, no atomics,
 * no host synchronisation: the same bits on every run and stream.  A deeper pyramid repeats the call on its last output
 * with source_level raised.
 * ---------------------------------------------------------------------------------- */
int pds_disparity_pyramid_fwd(const float* disparity, const unsigned char* valid /* or NULL */,
                              const float* confidence /* or NULL */, float min_confidence, float max_difference,
                              float* const* out /* host, [levels] device pointers */, int levels, int source_level,
                              int batch, int h, int w, pds_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PDS_HIP_TRACKING_H */
