/* The rolling volume: the entry points that let a dense TSDF volume follow the rig (Kintinuous; not in the reference).
 * An extension of pds_hip.h under the same ABI version: pds_hip.h, pds_hip_tracking.h, pds_hip_photometric.h and the
 * tables of their symbols stay as they were, and a caller whose volume never moves needs neither this file nor its
 * symbols. */
#ifndef PDS_HIP_ROLLING_H
#define PDS_HIP_ROLLING_H

#include "pds_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * Shift of the volume by whole voxels                                               not in the reference
 * Additive: ABI version unchanged.
 * tsdf, weight: float32 [nz, ny, nx], x fastest; color (or NULL): float32 [nz, ny, nx, 3]; the limits of the volume are
 * those of pds_tsdf_integrate_fwd.  tsdf_out, weight_out, color_out (NULL iff color is): the same shapes.  With
 * (dx, dy, dz) whole voxels:
 *   out voxel (i, j, k) = in voxel (i + dx, j + dy, k + dz)   where that lies inside the volume
 *                       = tsdf 1.0f, weight 0.0f, colour 0.0f   elsewhere (the state of a fresh volume)
 * so the volume whose origin was o now has its origin at o + voxel_size * (dx, dy, dz).  The copies are bit copies: NaN
 * payloads and -0.0 survive.  Any int is a legal d; with |d_a| >= n_a on some axis the whole output is the empty state.
 * Out of place: no output may overlap an input or another output, which is refused from the pointers and the sizes.
 * Buffers are 4-byte aligned and may sit at any 4-byte offset of an allocation: no byte outside [in, in + 4 nx ny nz)
 * of tsdf or weight or [color, color + 12 nx ny nz) is read, whatever the alignment (16-byte accesses are used only for
 * four consecutive voxels that all exist, and for loads only where their source is 16-byte aligned).  Voxels that enter
 * are not read.  ONE launch (tsdf_shift) on `stream` for the two or three tensors; no workspace, no atomics, no host
 * synchronisation: the same bits on every run and stream.
 * ---------------------------------------------------------------------------------- */
int pds_tsdf_shift_fwd(const float* tsdf, const float* weight, const float* color /* or NULL */, float* tsdf_out,
                       float* weight_out, float* color_out /* NULL iff color is */, int dx, int dy, int dz, int nx, int ny,
                       int nz, pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The surface that a shift is about to lose                                          not in the reference
 * Additive: ABI version unchanged.
 * The arguments of pds_tsdf_extract_fwd and (dx, dy, dz) of pds_tsdf_shift_fwd; to be called on the volume BEFORE it is
 * shifted.  Voxel (i, j, k) lands inside the shifted volume iff 0 <= i - dx < nx, 0 <= j - dy < ny and 0 <= k - dz < nz.
 * The edge from voxel v to its neighbour n along +x, +y or +z survives iff both v and n land inside; otherwise it leaves.
 * Written are exactly those rows of pds_tsdf_extract_fwd, on the same arguments, whose edge leaves: the same bits in
 * points, normals and index = 3 v + a (the numbering of the volume as it is, before the shift), in ascending index.
 * The rows of pds_tsdf_extract_fwd on the shifted volume, their index moved by 3 ((dz ny + dy) nx + dx), are the others
 * (for min_weight > 0: the voxels that enter have weight 0).  offsets [2] = {0, the TRUE count of leaving rows}; only rows
 * below `capacity` are written.  workspace: pds_tsdf_extract_workspace_bytes(nx, ny, nz) bytes, 4-byte aligned.  Any int is
 * a legal d: (0, 0, 0) gives no row, |d_a| >= n_a the whole surface.  Three launches on `stream`
 * (tsdf_extract_leaving_count, tsdf_extract_leaving_scan, tsdf_extract_leaving_scatter), the kernels of
 * pds_tsdf_extract_fwd with the mask; no atomics, no host synchronisation: the same bits on every run and stream.  No
 * output may overlap an input or another output.  Colours: pds_tsdf_color_gather_fwd on these rows, before the shift.
 * ---------------------------------------------------------------------------------- */
int pds_tsdf_extract_leaving_fwd(const float* tsdf, const float* weight, const float* origin /* host, [3] */,
                                 float voxel_size, float min_weight, float* points, float* normals /* or NULL */,
                                 int* index /* or NULL */, int* offsets, long long capacity, int nx, int ny, int nz,
                                 int dx, int dy, int dz, void* workspace, size_t workspace_bytes, pds_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PDS_HIP_ROLLING_H */
