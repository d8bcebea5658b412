"""CPU: TSDF fusion (pds_tsdf_integrate_workspace_bytes, pds_tsdf_integrate_fwd, pds_tsdf_extract_workspace_bytes,
pds_tsdf_extract_fwd; TsdfVolume, StereoRig.tsdf_volume, StereoRig.integrate).  The entry points are declared, exported and
bound and validate their arguments without a GPU, and the Python surface refuses what it cannot run.

The numpy fp64 oracles of tests/test_gpu_tsdf.py live here and are themselves held to hand-written answers, so that a
wrong oracle cannot pass a wrong kernel.  oracle_integrate sees A, b, the camera and the matrix as the entry point gets
them (rounded once to float32).  It does not decide what fp32 cannot: a voxel whose u + 0.5 or v + 0.5 lies within TAU of
an integer may read the pixel on either side, one whose sdf lies within EPS (Z + z_c) of -truncation, or whose z_c lies
within 1e-6 of 0, may be skipped or updated; every admissible outcome of such an AMBIGUOUS voxel is listed, and
check_integration accepts any of them there (and nowhere else).  oracle_extract is exact in its decisions."""
import collections
import ctypes
import inspect

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib, tsdf as tsdf_module
from tests.test_register_depth_host import EPS, TAU, simple_rig

NAN, INF = float('nan'), float('inf')
TILE = 1024          # csrc/common.hpp: kPointCloudTile, kTsdfDepthTile
MAX_GROUPS = 2048    # csrc/common.hpp: kTsdfIntegrateMaxGroups
IDENTITY = np.hstack([np.eye(3), np.zeros((3, 1))])

# tsdf, weight [nz, ny, nx] fp64: the outcome where the voxel is not ambiguous (the first candidate otherwise); updated
# bool; ambiguous bool; bound fp64: the admissible error of tsdf; outcomes: a list of (applies bool, tsdf, weight, bound,
# skipped bool), every admissible outcome of every voxel (a non-ambiguous voxel has exactly one distinct outcome)
Integration = collections.namedtuple('Integration', ['tsdf', 'weight', 'updated', 'ambiguous', 'bound', 'outcomes',
                                                     'projects'])
Surface = collections.namedtuple('Surface', ['index', 'points', 'normals', 'gradient_norm'])


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def q_of(height, width, focal, baseline):
    return np.array([[1.0, 0.0, 0.0, -0.5 * (width - 1)], [0.0, 1.0, 0.0, -0.5 * (height - 1)], [0.0, 0.0, 0.0, focal],
                     [0.0, 0.0, 1.0 / baseline, 0.0]])


def camera_of(Q):
    """The rectified left camera itself, from Q."""
    return (Q[2, 3], Q[2, 3], -Q[0, 3], -Q[1, 3], 0.0)


def as_the_kernel_sees(origin, voxel_size, pose, camera, matrix):
    """-> (A (3, 3), b (3,), camera (5,), matrix (4, 4)) in fp64, each first rounded to float32 as the entry point gets
    them; A = voxel_size R, b = R (origin + voxel_size / 2) + t, composed in fp64."""
    pose = np.asarray(IDENTITY if pose is None else pose, dtype=np.float64)
    R, t = pose[:, :3], pose[:, 3]
    return (f32(voxel_size * R), f32(R @ (np.asarray(origin, dtype=np.float64) + 0.5 * voxel_size) + t), f32(camera),
            f32(matrix))


# ------------------------------------------------------------------------------------------------ the oracles
def oracle_depth(disparity, matrix, valid=None, confidence=None, min_confidence=0.0):
    """Launch 1 in fp64: Z [H, W] of `reproject` for a float32 matrix, NaN where dropped or not finite and positive."""
    d = np.asarray(disparity, dtype=np.float32).astype(np.float64)
    height, width = d.shape
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    M = matrix
    with np.errstate(all='ignore'):
        Z, W = (M[r, 0] * xx + M[r, 1] * yy + M[r, 2] * d + M[r, 3] for r in (2, 3))
        kept = np.isfinite(d) & (d > 0) & (W > 0)
        if valid is not None:
            kept &= np.asarray(valid, dtype=bool)
        if confidence is not None:
            kept &= np.asarray(confidence, dtype=np.float32) >= np.float32(min_confidence)   # (a NaN fails)
        Z = Z / W
        kept &= np.isfinite(Z) & (Z > 0)
    return np.where(kept, Z, NAN)


def oracle_integrate(tsdf, weight, disparity, matrix, origin, voxel_size, truncation, max_weight=64.0, pose=None,
                     camera=None, valid=None, confidence=None, min_confidence=0.0, weight_by_confidence=False, tau=TAU,
                     eps=EPS):
    """One frame (disparity [H, W]) into the state (tsdf, weight: [nz, ny, nx], any float type) -> Integration."""
    tsdf, weight = np.asarray(tsdf, dtype=np.float64), np.asarray(weight, dtype=np.float64)
    nz, ny, nx = tsdf.shape
    A, b, (fx, fy, cx, cy, skew), M = as_the_kernel_sees(origin, voxel_size, pose,
                                                          camera_of(matrix) if camera is None else camera, matrix)
    truncation, max_weight = float(f32(truncation)), float(f32(max_weight))
    Z = oracle_depth(disparity, M, valid, confidence, min_confidence)
    height, width = Z.shape
    per_pixel = np.asarray(confidence, dtype=np.float32).astype(np.float64) if weight_by_confidence else np.ones(Z.shape)
    kk, jj, ii = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float64)
    xc, yc, zc = (A[r, 0] * ii + A[r, 1] * jj + A[r, 2] * kk + b[r] for r in range(3))
    with np.errstate(all='ignore'):
        front = zc > 0
        u = fx * (xc / zc) + skew * (yc / zc) + cx
        v = fy * (yc / zc) + cy
        finite = front & np.isfinite(u) & np.isfinite(v)
        u, v = np.where(finite, np.clip(u, -4.0, width + 4.0), -4.0), np.where(finite, np.clip(v, -4.0, height + 4.0), -4.0)
    near_zero = np.abs(zc) <= 1e-6
    outcomes = []
    for du in (-tau, tau):
        for dv in (-tau, tau):
            px, py = np.floor(u + 0.5 + du).astype(np.int64), np.floor(v + 0.5 + dv).astype(np.int64)
            inside = finite & (px >= 0) & (px < width) & (py >= 0) & (py < height)
            pxc, pyc = np.clip(px, 0, width - 1), np.clip(py, 0, height - 1)
            z, w = Z[pyc, pxc], per_pixel[pyc, pxc]
            with np.errstate(all='ignore'):
                sdf = z - zc
                hit = inside & ~np.isnan(z) & (w > 0)
                margin = eps * (z + zc)
                update = hit & (sdf >= -truncation)
                either = (hit & (np.abs(sdf + truncation) <= margin)) | near_zero
                t = np.minimum(1.0, sdf / truncation)
                new_tsdf = (tsdf * weight + t * w) / (weight + w)
                new_weight = np.minimum(weight + w, max_weight)
                bound = margin / truncation
            updated = (update | (either & hit))
            outcomes.append((updated, np.where(updated, new_tsdf, tsdf), np.where(updated, new_weight, weight),
                             np.where(updated, bound, 0.0), np.zeros_like(updated)))
            skipped = ~update | either
            outcomes.append((skipped, tsdf, weight, np.zeros_like(tsdf), np.ones_like(updated)))
    # a voxel is ambiguous unless the four pixel choices agree and none of them may go either way
    first = outcomes[0][0]
    ambiguous = near_zero.copy()
    px0, py0 = np.floor(u + 0.5 - tau), np.floor(v + 0.5 - tau)
    ambiguous |= finite & ((px0 != np.floor(u + 0.5 + tau)) | (py0 != np.floor(v + 0.5 + tau)))
    for k in range(0, 8, 2):
        ambiguous |= outcomes[k][0] & outcomes[k + 1][0]
    projects = finite & (px0 >= 0) & (px0 < width) & (py0 >= 0) & (py0 < height)
    return Integration(np.where(first, outcomes[0][1], tsdf), np.where(first, outcomes[0][2], weight), first & ~ambiguous,
                       ambiguous, outcomes[0][3], outcomes, projects)


def check_integration(got_tsdf, got_weight, old_tsdf, old_weight, oracle, extra=0.0, weight_rtol=0.0, case=''):
    """got_* / old_*: float32 [nz, ny, nx] after and before the frame.  A non-ambiguous voxel: the weight exact (or within
    weight_rtol), the tsdf within its bound + extra, and where it is not updated the bits of before.  An ambiguous voxel:
    one of its admissible outcomes, to the same bounds.  -> the number of updated voxels."""
    assert got_tsdf.dtype == got_weight.dtype == np.float32 and got_tsdf.shape == oracle.tsdf.shape, case
    same_bits = (got_tsdf.view(np.int32) == old_tsdf.view(np.int32)) & (got_weight.view(np.int32) == old_weight.view(np.int32))
    matched = np.zeros(got_tsdf.shape, dtype=bool)
    for applies, value, held, bound, skipped in oracle.outcomes:
        with np.errstate(invalid='ignore'):
            close = (np.abs(got_tsdf - value) <= bound + extra) & (np.abs(got_weight - held) <= weight_rtol * np.abs(held))
        matched |= applies & np.where(skipped, same_bits, close)
    assert matched.all(), (case, int((~matched).sum()), np.argwhere(~matched)[:5].tolist())
    sure = ~oracle.ambiguous
    assert (same_bits | oracle.updated)[sure].all(), case
    return int(oracle.updated.sum())


def oracle_extract(tsdf, weight, origin, voxel_size, min_weight=1.0):
    """tsdf, weight float32 [nz, ny, nx] -> Surface(index int64 ascending, points fp64 [N, 3], normals fp64 [N, 3] with NaN
    rows, gradient_norm fp64 [N]: |g| before the normalisation, NaN where the stencil fails).  The decisions are made on
    the float32 values as they are."""
    tsdf, weight = np.asarray(tsdf), np.asarray(weight)
    assert tsdf.dtype == weight.dtype == np.float32 and tsdf.shape == weight.shape and tsdf.ndim == 3
    nz, ny, nx = tsdf.shape
    observed = weight >= np.float32(min_weight)
    negative = tsdf < 0
    value = tsdf.astype(np.float64)
    origin, voxel_size = f32(origin), float(f32(voxel_size))
    # g(c) and whether its six voxels are inside and observed
    gradient = np.full((nz, ny, nx, 3), NAN)
    whole = np.ones((nz, ny, nx), dtype=bool)
    for m, axis in enumerate((2, 1, 0)):
        plus, minus = np.roll(value, -1, axis), np.roll(value, 1, axis)
        ok = np.roll(observed, -1, axis) & np.roll(observed, 1, axis)
        position = np.arange(tsdf.shape[axis]).reshape([-1 if a == axis else 1 for a in range(3)])
        ok = ok & (position >= 1) & (position + 1 < tsdf.shape[axis])
        gradient[..., m] = plus - minus
        whole &= ok
    index, points, normals, norms = [], [], [], []
    kk, jj, ii = np.mgrid[0:nz, 0:ny, 0:nx]
    flat = (kk * ny + jj) * nx + ii
    for a, axis in enumerate((2, 1, 0)):
        inside = np.arange(tsdf.shape[axis]).reshape([-1 if d == axis else 1 for d in range(3)]) + 1 < tsdf.shape[axis]
        crossing = inside & observed & np.roll(observed, -1, axis) & (negative != np.roll(negative, -1, axis))
        where = np.nonzero(crossing)
        neighbour = tuple(w + (1 if d == axis else 0) for d, w in enumerate(where))
        tv, tn = value[where], value[neighbour]
        r = tv / (tv - tn)
        at = np.stack([ii[where], jj[where], kk[where]], axis=1) + 0.5
        at[:, a] += r
        g = (1.0 - r)[:, None] * gradient[where] + r[:, None] * gradient[neighbour]
        length = np.sqrt((g * g).sum(axis=1))
        good = whole[where] & whole[neighbour] & (length > 0)
        with np.errstate(invalid='ignore', divide='ignore'):
            unit = np.where(good[:, None], g / length[:, None], NAN)
        index.append(3 * flat[where] + a)
        points.append(origin + voxel_size * at)
        normals.append(unit)
        norms.append(np.where(whole[where] & whole[neighbour], length, NAN))
    index = np.concatenate(index).astype(np.int64)
    order = np.argsort(index, kind='stable')
    return Surface(index[order], np.concatenate(points)[order], np.concatenate(normals)[order],
                   np.concatenate(norms)[order])


def surface_gap(points, index, tsdf, disparity, matrix, origin, voxel_size, pose=None, camera=None, tau=TAU):
    """How far every extracted point lies, along the camera's z, from the surface its own edge was measured against.
    `index = 3 v + a` names the edge from voxel v to its neighbour n along axis a; the one of the two with the negative
    tsdf was updated with sdf = Z - z_c in [-truncation, 0) against the Z of the pixel ITS centre projects to, and the
    point lies on the edge, at most voxel_size along axis a from that centre, which moves its depth by at most
    voxel_size |R[2, a]|.  So |z_point - Z| <= truncation + voxel_size |R[2, a]| (+ the oracle's margin) for every point,
    at a silhouette as anywhere else, and a misplaced point fails.  -> (gap [N], Z [N], reach [N]): the smallest
    |z_point - Z| over the pixels that voxel may have read (the roundings within tau; inf where it read none), that Z, and
    voxel_size |R[2, a]|."""
    tsdf = np.asarray(tsdf)
    nz, ny, nx = tsdf.shape
    index = np.asarray(index, dtype=np.int64)
    v, a = index // 3, index % 3
    n = v + np.array([1, nx, nx * ny])[a]
    negative = np.where(tsdf.reshape(-1)[v] < 0, v, n)
    assert ((tsdf.reshape(-1)[v] < 0) != (tsdf.reshape(-1)[n] < 0)).all()
    ijk = np.stack([negative % nx, negative // nx % ny, negative // (nx * ny)], axis=1).astype(np.float64)
    A, b, (fx, fy, cx, cy, skew), M = as_the_kernel_sees(origin, voxel_size, pose,
                                                          camera_of(matrix) if camera is None else camera, matrix)
    centre = ijk @ A.T + b
    u = fx * centre[:, 0] / centre[:, 2] + skew * centre[:, 1] / centre[:, 2] + cx
    w = fy * centre[:, 1] / centre[:, 2] + cy
    Z = oracle_depth(disparity, M)
    height, width = Z.shape
    pose = np.asarray(IDENTITY if pose is None else pose, dtype=np.float64)
    z_point = np.asarray(points, dtype=np.float64) @ pose[2, :3] + pose[2, 3]
    gap, read = np.full(len(index), np.inf), np.full(len(index), NAN)
    for du in (-tau, tau):
        for dv in (-tau, tau):
            px, py = np.floor(u + 0.5 + du).astype(np.int64), np.floor(w + 0.5 + dv).astype(np.int64)
            inside = (px >= 0) & (px < width) & (py >= 0) & (py < height)
            sample = np.where(inside, Z[np.clip(py, 0, height - 1), np.clip(px, 0, width - 1)], NAN)
            with np.errstate(invalid='ignore'):
                nearer = np.abs(z_point - sample) < gap
            gap, read = np.where(nearer, np.abs(z_point - sample), gap), np.where(nearer, sample, read)
    return gap, read, voxel_size * np.abs(pose[2, :3])[a]


# ------------------------------------------------------------------------------------------------ the wall, by hand
# Every number is a dyadic fraction, so float32 holds it exactly: focal 74 px, baseline 1/8 m, a wall of disparity 8:
# Z = 74 / (8 * 8) = 1.15625 m.  Voxels of 1/8 m whose layers lie at z = 1, 1.125, 1.25, 1.375, 1.5; truncation 1/8:
# sdf = 0.15625, 0.03125, -0.09375, -0.21875, -0.34375  ->  t = 1, 0.25, -0.75, skipped, skipped.
# The zero crossing lies a quarter of the way from layer 1 to layer 2: 0.25 / (0.25 + 0.75), at z = 1.15625.
WALL = dict(height=48, width=64, focal=74.0, baseline=0.125, disparity=8.0, depth=1.15625, voxel_size=0.125,
            z0=0.9375, truncation=0.125, layers=(1.0, 0.25, -0.75))


def wall_volume(dims):
    """-> (origin, matrix): the volume's x and y extent centred on the optical axis, 1 / 64 m off, so that few voxel
    centres project onto a pixel border."""
    nx, ny, _ = dims
    vs = WALL['voxel_size']
    origin = np.array([-0.5 * nx * vs + 0.015625, -0.5 * ny * vs + 0.015625, WALL['z0']])
    return origin, q_of(WALL['height'], WALL['width'], WALL['focal'], WALL['baseline'])


def wall_layers(nz):
    """-> (tsdf, weight) per layer after one frame, by hand: 1.0 / 0.0 where the layer is skipped."""
    t = np.ones(nz)
    w = np.zeros(nz)
    for k, value in enumerate(WALL['layers'][:nz]):
        t[k], w[k] = value, 1.0
    return t, w


def test_oracle_integrate_wall_by_hand():
    dims = (3, 2, 5)
    origin, Q = wall_volume(dims)
    d = np.full((WALL['height'], WALL['width']), WALL['disparity'], dtype=np.float32)
    assert np.array_equal(oracle_depth(d, f32(Q)), np.full(d.shape, WALL['depth']))
    fresh = (np.ones((5, 2, 3)), np.zeros((5, 2, 3)))
    o = oracle_integrate(*fresh, d, Q, origin, WALL['voxel_size'], WALL['truncation'])
    assert not o.ambiguous.any() and o.projects.all()
    for k, (t, w) in enumerate(zip([1.0, 0.25, -0.75, 1.0, 1.0], [1.0, 1.0, 1.0, 0.0, 0.0])):
        assert (o.tsdf[k] == t).all() and (o.weight[k] == w).all(), k
        assert o.updated[k].all() == (k < 3) and o.updated[k].any() == (k < 3), k
    assert wall_layers(5)[0].tolist() == [1.0, 0.25, -0.75, 1.0, 1.0] and wall_layers(5)[1].tolist() == [1, 1, 1, 0, 0]
    # three identical frames: the same tsdf, weight 3; with max_weight 2 the weight stops at 2
    for cap, final in ((64.0, 3.0), (2.0, 2.0)):
        state = fresh
        for _ in range(3):
            o = oracle_integrate(*state, d, Q, origin, WALL['voxel_size'], WALL['truncation'], max_weight=cap)
            state = (o.tsdf, o.weight)
        assert np.allclose(o.tsdf[:3, 0, 0], [1.0, 0.25, -0.75], rtol=0, atol=1e-15)
        assert o.weight[:, 0, 0].tolist() == [final, final, final, 0.0, 0.0] and (o.tsdf[3:] == 1.0).all()
    # the checker takes the answer and refuses a wrong value, a wrong weight and a touched voxel
    old = (np.ones((5, 2, 3), dtype=np.float32), np.zeros((5, 2, 3), dtype=np.float32))
    o = oracle_integrate(*fresh, d, Q, origin, WALL['voxel_size'], WALL['truncation'])
    good = (o.tsdf.astype(np.float32), o.weight.astype(np.float32))
    assert check_integration(*good, *old, o) == 18
    for k, (dt, dw) in ((1, (1e-3, 0.0)), (1, (0.0, 1.0)), (4, (0.0, 1.0)), (4, (-0.5, 0.0))):
        bad = (good[0].copy(), good[1].copy())
        bad[0][k, 1, 2] += dt
        bad[1][k, 1, 2] += dw
        with pytest.raises(AssertionError):
            check_integration(*bad, *old, o)
    # valid, confidence and the confidence as the weight: pixel (24, 32) is where voxel (1, 1, *) of layer 0 projects
    o0 = oracle_integrate(*fresh, d, Q, origin, WALL['voxel_size'], WALL['truncation'], valid=np.zeros(d.shape, dtype=bool))
    assert not o0.updated.any() and (o0.tsdf == 1.0).all() and (o0.weight == 0.0).all()
    confidence = np.full(d.shape, 0.5, dtype=np.float32)
    o1 = oracle_integrate(*fresh, d, Q, origin, WALL['voxel_size'], WALL['truncation'], confidence=confidence,
                          min_confidence=0.75)
    assert not o1.updated.any()
    o2 = oracle_integrate(*fresh, d, Q, origin, WALL['voxel_size'], WALL['truncation'], confidence=confidence,
                          weight_by_confidence=True)
    assert (o2.weight[:3] == 0.5).all() and (o2.tsdf[1] == 0.25).all() and (o2.weight[3:] == 0.0).all()
    o3 = oracle_integrate(o2.tsdf, o2.weight, 2 * d, Q, origin, WALL['voxel_size'], WALL['truncation'])
    # the wall at half the depth, 0.578 m, lies in front of every layer: sdf = -0.42 .. : all skipped
    assert not o3.updated.any() and (o3.weight == o2.weight).all()
    # a pose that moves the world 1/8 m away along z shifts the layers by one: t = 0.25, -0.75, skipped ...
    away = np.hstack([np.eye(3), [[0.0], [0.0], [0.125]]])
    o4 = oracle_integrate(*fresh, d, Q, origin, WALL['voxel_size'], WALL['truncation'], pose=away)
    assert o4.tsdf[:, 0, 0].tolist() == [0.25, -0.75, 1.0, 1.0, 1.0] and o4.weight[:, 0, 0].tolist() == [1, 1, 0, 0, 0]


def test_oracle_integrate_marks_what_fp32_cannot_decide():
    # one voxel whose centre projects exactly onto the border between two pixels of different depth: either is admissible
    Q = q_of(4, 4, 64.0, 0.125)
    d = np.array([[8.0, 8.0, 4.0, 4.0]] * 4, dtype=np.float32)   # Z = 1 | 2
    # the voxel centre at x = 0 m projects to u = cx = 1.5: floor(2.0) -- a border
    o = oracle_integrate(np.ones((1, 1, 1)), np.zeros((1, 1, 1)), d, Q, (-0.0625, -0.0625, 0.9375), 0.125, 0.25)
    assert o.ambiguous.all() and not o.updated.any()
    got = {(float(v[0, 0, 0]), float(w[0, 0, 0])) for applies, v, w, _, _ in o.outcomes if applies[0, 0, 0]}
    assert got == {(0.0, 1.0), (1.0, 1.0)}   # z_c = 1: Z = 1 gives sdf 0, Z = 2 gives 1 (truncated)
    old = (np.ones((1, 1, 1), dtype=np.float32), np.zeros((1, 1, 1), dtype=np.float32))
    for value in (0.0, 1.0):
        check_integration(np.full((1, 1, 1), value, dtype=np.float32), np.ones((1, 1, 1), dtype=np.float32), *old, o)
    with pytest.raises(AssertionError):
        check_integration(np.full((1, 1, 1), 0.5, dtype=np.float32), np.ones((1, 1, 1), dtype=np.float32), *old, o)
    with pytest.raises(AssertionError):   # (skipping is not admissible here)
        check_integration(*old, *old, o)
    # sdf == -truncation: updated (t = -1) or skipped
    o = oracle_integrate(np.ones((1, 1, 1)), np.zeros((1, 1, 1)), np.full((4, 4), 8.0, dtype=np.float32), Q,
                         (-0.04, -0.04, 1.1875), 0.125, 0.25)   # z_c = 1.25, Z = 1
    assert o.ambiguous.all()
    got = {(float(v[0, 0, 0]), float(w[0, 0, 0])) for applies, v, w, _, _ in o.outcomes if applies[0, 0, 0]}
    assert got == {(-1.0, 1.0), (1.0, 0.0)}
    # behind the camera, and outside the image: skipped, not ambiguous
    for origin in ((-0.04, -0.04, -2.0), (5.0, -0.04, 0.9375)):
        o = oracle_integrate(np.ones((1, 1, 1)), np.zeros((1, 1, 1)), np.full((4, 4), 8.0, dtype=np.float32), Q, origin,
                             0.125, 0.25)
        assert not o.ambiguous.any() and not o.updated.any() and not o.projects.any()


# ------------------------------------------------------------------------------------------------ extraction, by hand
def hand_volume():
    """4 x 4 x 4, voxels of 1/2 m from the origin (1, 2, 3).  tsdf = 0.25 for i <= 1 and -0.75 for i >= 2: a plane a
    quarter of the way from i = 1 to i = 2.  Then: (i, j, k) = (0, 2, 0) and (0, 3, 0) are set to -0.25; the weight of
    (0, 1, 1) and of (2, 3, 3) is 0."""
    tsdf = np.full((4, 4, 4), 0.25, dtype=np.float32)
    tsdf[:, :, 2:] = -0.75
    tsdf[0, 2, 0] = tsdf[0, 3, 0] = -0.25
    weight = np.ones((4, 4, 4), dtype=np.float32)
    weight[1, 1, 0] = weight[3, 3, 2] = 0.0
    return tsdf, weight


def test_oracle_extract_4x4x4_by_hand():
    tsdf, weight = hand_volume()
    s = oracle_extract(tsdf, weight, (1.0, 2.0, 3.0), 0.5)
    v = (lambda i, j, k: (k * 4 + j) * 4 + i)
    # the plane: axis 0 at i = 1 for every (j, k) but (3, 3), whose neighbour is unobserved
    plane = {3 * v(1, j, k) for k in range(4) for j in range(4)} - {3 * v(1, 3, 3)}
    # the two voxels at (0, 2, 0), (0, 3, 0): towards +x (axis 0) and +z (axis 2) of each, and along +y from (0, 1, 0)
    extra = {3 * v(0, 2, 0), 3 * v(0, 3, 0), 3 * v(0, 2, 0) + 2, 3 * v(0, 3, 0) + 2, 3 * v(0, 1, 0) + 1}
    assert s.index.tolist() == sorted(plane | extra) and len(s.index) == 20
    assert s.index.tolist()[:8] == [3, 13, 15, 24, 26, 27, 36, 38]
    rows = {int(index): row for row, index in enumerate(s.index)}
    # positions: origin + 0.5 * ((i, j, k) + 0.5 + r e_a)
    assert s.points[rows[3 * v(1, 0, 0)]].tolist() == [1.0 + 0.5 * 1.75, 2.0 + 0.25, 3.0 + 0.25]
    assert s.points[rows[3 * v(1, 2, 3)]].tolist() == [1.875, 2.0 + 0.5 * 2.5, 3.0 + 0.5 * 3.5]
    assert s.points[rows[3 * v(0, 1, 0) + 1]].tolist() == [1.25, 2.0 + 0.5 * 2.0, 3.25]           # r = 0.5 along y
    assert s.points[rows[3 * v(0, 3, 0) + 2]].tolist() == [1.25, 2.0 + 0.5 * 3.5, 3.0 + 0.5 * 1.0]   # r = 0.5 along z
    assert s.points[rows[3 * v(0, 2, 0)]].tolist() == [1.0 + 0.5 * 1.0, 2.0 + 0.5 * 2.5, 3.25]   # -0.25 / (-0.25 - 0.25)
    # normals need j, k in {1, 2} (and i - 1 >= 0: i = 1 has it): of the plane's four such points, (1, 1, 1) has the
    # unobserved (0, 1, 1) in its stencil.  One by hand: at (1, 2, 2), g(v) = (t[2] - t[0], 0, 0) = (-1, 0, 0) = g(n)
    has_normal = sorted(int(index) for index, n in zip(s.index, s.normals) if not np.isnan(n).any())
    assert has_normal == [3 * v(1, 2, 1), 3 * v(1, 1, 2), 3 * v(1, 2, 2)]
    assert s.normals[rows[3 * v(1, 2, 2)]].tolist() == [-1.0, 0.0, 0.0] and s.gradient_norm[rows[3 * v(1, 2, 2)]] == 1.0
    assert np.isnan(s.normals[rows[3 * v(1, 1, 1)]]).all() and np.isnan(s.gradient_norm[rows[3 * v(1, 1, 1)]])
    # min_weight above every weight: nothing; -0.0 is not negative; a volume of one voxel has no neighbour
    assert len(oracle_extract(tsdf, weight, (0, 0, 0), 1.0, min_weight=1.5).index) == 0
    zeros = np.array([[[-0.0, 0.0, 1.0, -1.0]]], dtype=np.float32)
    assert oracle_extract(zeros, np.ones_like(zeros), (0, 0, 0), 1.0).index.tolist() == [3 * 2]
    assert len(oracle_extract(zeros[:, :, :1], np.ones((1, 1, 1), dtype=np.float32), (0, 0, 0), 1.0).index) == 0
    # a zero gradient: the point stays, the normal is NaN
    flat = np.zeros((3, 3, 4), dtype=np.float32)
    flat[:, :, 0], flat[:, :, 1], flat[:, :, 2], flat[:, :, 3] = 0.5, -0.5, 0.5, -0.5
    s = oracle_extract(flat, np.ones_like(flat), (0, 0, 0), 1.0)
    row = s.index.tolist().index(3 * ((1 * 3 + 1) * 4 + 1))   # (1, 1, 1) -> (2, 1, 1): g(v) = (0, 0, 0) = g(n)
    assert np.isnan(s.normals[row]).all() and s.gradient_norm[row] == 0.0 and s.points[row].tolist() == [2.0, 1.5, 1.5]


# ------------------------------------------------------------------------------------------------ the general case
GENERAL = dict(height=48, width=64, focal=60.0, baseline=0.12, dims=(40, 36, 28), voxel_size=0.02,
               origin=(-0.40, -0.36, 0.35), truncation=0.06)


def general_disparity(seed=0):
    height, width = GENERAL['height'], GENERAL['width']
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    d = 10.0 + 0.05 * xx - 0.03 * yy
    d[10:30, 20:40] = 16.0
    d[np.random.RandomState(seed).rand(height, width) < 0.05] = NAN
    return d.astype(np.float32)


def general_pose(k=0):
    """Three poses a few degrees and centimetres apart; never the identity, whose voxel centres project onto pixel
    borders."""
    rotations = ((0.05, -0.08, 0.03), (-0.04, 0.06, 0.02), (0.02, 0.03, -0.05))
    translations = ((0.01, -0.02, 0.03), (-0.02, 0.01, 0.02), (0.015, 0.02, 0.01))
    return np.hstack([pds.rectification.rodrigues(np.array(rotations[k])), np.array(translations[k])[:, None]])


def general_case(k=0):
    """-> the keyword arguments of oracle_integrate for frame k (state aside)."""
    return dict(disparity=general_disparity(k), matrix=q_of(GENERAL['height'], GENERAL['width'], GENERAL['focal'],
                                                             GENERAL['baseline']),
                origin=GENERAL['origin'], voxel_size=GENERAL['voxel_size'], truncation=GENERAL['truncation'],
                pose=general_pose(k))


def fresh_state(dims, dtype=np.float64):
    nx, ny, nz = dims
    return np.ones((nz, ny, nx), dtype=dtype), np.zeros((nz, ny, nx), dtype=dtype)


def test_the_general_case_is_neither_swallowed_by_its_bands_nor_empty():
    o = oracle_integrate(*fresh_state(GENERAL['dims']), **general_case())
    voxels = o.tsdf.size
    assert voxels == 40320 and voxels % TILE != 0
    projecting, updated = int(o.projects.sum()), int(o.updated.sum())
    ambiguous = int((o.ambiguous & o.projects).sum()) / projecting
    crossings = len(oracle_extract(o.tsdf.astype(np.float32), o.weight.astype(np.float32), GENERAL['origin'],
                                   GENERAL['voxel_size']).index)
    print('%.1f %% project into the image, %.1f %% are updated, %.1f %% negative, %.2f %% of the projecting voxels '
          'ambiguous, %d crossings' % (100 * projecting / voxels, 100 * updated / voxels,
                                       100 * float((o.tsdf < 0).mean()), 100 * ambiguous, crossings))
    assert ambiguous <= 0.05 and updated / voxels >= 0.20 and crossings >= 1000
    # and the fp64 answer itself passes the check it is the yardstick of
    old = fresh_state(GENERAL['dims'], np.float32)
    assert check_integration(o.tsdf.astype(np.float32), o.weight.astype(np.float32), *old, o, extra=1e-7) == updated
    # the surface of that volume: every point within truncation + its edge's reach in depth of the Z its negative voxel
    # was measured against -- and of the points moved by five voxels along the optical axis, either way, nine in ten are not
    case = general_case()
    state = (o.tsdf.astype(np.float32), o.weight.astype(np.float32))
    s = oracle_extract(*state, GENERAL['origin'], GENERAL['voxel_size'])
    geometry = dict(disparity=case['disparity'], matrix=case['matrix'], origin=GENERAL['origin'],
                    voxel_size=GENERAL['voxel_size'], pose=case['pose'])
    gap, read, reach = surface_gap(s.points, s.index, state[0], **geometry)
    allowed = GENERAL['truncation'] + reach + EPS * 2.0 * read
    print('the surface: %d points, at most %.4f m from the depth their edge was measured against, %.4f m more than '
          'allowed' % (len(gap), gap.max(), (gap - allowed).max()))
    assert np.isfinite(gap).all() and (gap <= allowed).all()
    for direction in (1.0, -1.0):
        moved = s.points + direction * 5 * GENERAL['voxel_size'] * case['pose'][2, :3]
        assert (surface_gap(moved, s.index, state[0], **geometry)[0] > allowed).mean() > 0.9, direction
    assert (surface_gap(-s.points, s.index, state[0], **geometry)[0] > allowed).all()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_tsdf_symbols_declared_exported_and_bound(hip_library):
    header = open(_lib.HEADER_PATH).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('pds_tsdf_integrate_workspace_bytes', 'pds_tsdf_integrate_fwd', 'pds_tsdf_extract_workspace_bytes',
                 'pds_tsdf_extract_fwd'):
        assert name + '(' in header and hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert hip_library.pds_abi_version() == 7 and '#define PDS_ABI_VERSION 7' in header
    for name in ('TsdfVolume', 'SurfacePoints'):
        assert name in pds.__all__, name
    assert pds.SurfacePoints._fields == ('cloud', 'normals') and pds.TsdfVolume is tsdf_module.TsdfVolume
    csrc = _lib.HEADER_PATH.replace('include/pds_hip.h', 'practicaldeepstereo_nips2018_amd/csrc/')
    common = open(csrc + 'common.hpp').read()
    assert 'constexpr int kTsdfDepthTile = %d;' % TILE in common
    assert 'constexpr int kTsdfIntegrateMaxGroups = %d;' % MAX_GROUPS in common
    # integrate: Z and the weights of one entry, 4 bytes per pixel each, each rounded up to 256
    sizes = hip_library.pds_tsdf_integrate_workspace_bytes
    assert sizes(1, 1) == 512 and sizes(8, 8) == 512 and sizes(5, 13) == 1024 and sizes(540, 960) == 2 * 540 * 960 * 4
    assert sizes(3, 43) == 2 * 768
    # extract: one int per tile of 1024 voxels rounded up to 256, plus 256 (the compaction of point_cloud)
    sizes = hip_library.pds_tsdf_extract_workspace_bytes
    assert sizes(1, 1, 1) == 512 and sizes(40, 36, 28) == 512 and sizes(256, 256, 1) == 512
    assert sizes(256, 256, 2) == 768 and sizes(256, 256, 128) == 8192 * 4 + 256


def test_tsdf_validation_needs_no_gpu(hip_library):
    lib = hip_library
    big = 1 << 24
    d, v, c, t, w, ws, pts, nrm, idx, off = [ctypes.c_void_p(big * n) for n in range(1, 11)]   # never dereferenced
    floats = (lambda values: (ctypes.c_float * len(values))(*values))
    identity = floats(np.eye(4, dtype=np.float32).reshape(-1).tolist())
    rows = floats([0.1, 0, 0, 0, 0.1, 0, 0, 0, 0.1, 0, 0, 1.0])
    camera = floats([4.0, 4.0, 1.0, 0.5, 0.0])
    error = lib.pds_last_error

    def integrate(disparity=d, valid=v, confidence=c, min_confidence=0.0, by_confidence=0, matrix=identity,
                  transforms=rows, camera=camera, truncation=0.1, max_weight=64.0, tsdf=t, weight=w, dims=(4, 3, 2),
                  shape=(1, 2, 3), workspace=ws, workspace_bytes=512):
        return lib.pds_tsdf_integrate_fwd(disparity, valid, confidence, min_confidence, by_confidence, matrix,
                                          transforms, camera, truncation, max_weight, tsdf, weight, *dims, *shape,
                                          workspace, workspace_bytes, None)

    for name in ('disparity', 'matrix', 'transforms', 'camera', 'tsdf', 'weight', 'workspace'):
        assert integrate(**{name: None}) != 0 and error() == b'tsdf_integrate: null pointer', name
    for shape in [(0, 2, 3), (-1, 2, 3)]:
        assert integrate(shape=shape) != 0 and b'tsdf_integrate: bad batch' in error(), shape
    for shape in [(1, 0, 3), (1, 2, 0), (1, -2, 3), (1, 2, -3)]:
        assert integrate(shape=shape) != 0 and b'tsdf_integrate: bad shape' in error(), shape
        assert lib.pds_tsdf_integrate_workspace_bytes(*shape[1:]) == 0 and b'bad shape' in error(), shape
    assert integrate(shape=(1, 1 << 16, 1 << 15)) != 0 and b'h * w' in error() and b'32-bit indices' in error()
    assert lib.pds_tsdf_integrate_workspace_bytes(1 << 16, 1 << 15) == 0 and b'32-bit indices' in error()
    assert integrate(shape=(1 << 12, 1 << 10, 1 << 10), workspace_bytes=1 << 40) != 0 and b'batch * h * w' in error()
    for dims in [(0, 3, 2), (4, 0, 2), (4, 3, 0), (-4, 3, 2)]:
        assert integrate(dims=dims) != 0 and b'tsdf: bad volume' in error(), dims
        assert lib.pds_tsdf_extract_workspace_bytes(*dims) == 0 and b'tsdf: bad volume' in error(), dims
    # 3 * nx * ny * nz must fit: 895^3 * 3 = 2 150 776 125 does not, 894^3 * 3 = 2 143 574 952 does
    # a voxel index must be an exact float: no dimension above 2^24
    for dims in [((1 << 24) + 1, 1, 1), (1, 1 << 25, 1), (2, 2, (1 << 24) + 8)]:
        assert integrate(dims=dims) != 0 and b'tsdf: a dimension above 2^24' in error(), dims
        assert lib.pds_tsdf_extract_workspace_bytes(*dims) == 0 and b'above 2^24' in error(), dims
    assert lib.pds_tsdf_extract_workspace_bytes(1 << 24, 1, 1) == (1 << 14) * 4 + 256
    for dims in [(895, 895, 895), (1 << 16, 1 << 16, 1), (1 << 11, 1 << 11, 1 << 11)]:
        assert integrate(dims=dims) != 0 and b'3 * nx * ny * nz does not fit' in error(), dims
        assert lib.pds_tsdf_extract_workspace_bytes(*dims) == 0 and b'does not fit' in error(), dims
    assert lib.pds_tsdf_extract_workspace_bytes(894, 894, 894) == ((894 ** 3 + 1023) // 1024 * 4 + 255) // 256 * 256 + 256
    assert integrate(workspace_bytes=511) != 0 and b'workspace too small (511 < 512)' in error()
    assert integrate(by_confidence=1, confidence=None) != 0 and b'weight_by_confidence without a confidence' in error()
    for bad in (NAN, INF, -INF):
        assert integrate(min_confidence=bad) != 0 and b'min_confidence must be finite' in error(), bad
    for bad in (0.0, -0.1, NAN, INF):
        assert integrate(truncation=bad) != 0 and b'truncation must be positive and finite' in error(), bad
    for bad in (0.0, -1.0, NAN):
        assert integrate(max_weight=bad) != 0 and b'max_weight must be positive' in error(), bad
    assert integrate(tsdf=ctypes.c_void_p(t.value + 2)) != 0 and b'not 4-byte aligned' in error()
    assert integrate(weight=ctypes.c_void_p(w.value + 1)) != 0 and b'not 4-byte aligned' in error()
    assert integrate(workspace=ctypes.c_void_p(ws.value + 4)) != 0 and b'workspace is not 16-byte aligned' in error()
    # nothing written may overlap anything (4 x 3 x 2 voxels: 96 bytes; 2 x 3 pixels: 24 / 6 bytes)
    assert integrate(tsdf=d) != 0 and b'aliases an input' in error()
    assert integrate(weight=ctypes.c_void_p(c.value + 20)) != 0 and b'aliases an input' in error()
    assert integrate(workspace=ctypes.c_void_p(v.value - 496)) != 0 and b'aliases an input' in error()
    assert integrate(weight=t) != 0 and b'alias one another' in error()
    assert integrate(weight=ctypes.c_void_p(t.value + 92)) != 0 and b'alias one another' in error()
    assert integrate(workspace=ctypes.c_void_p(w.value + 80)) != 0 and b'alias one another' in error()
    for k, name, base in ((0, 'matrix', np.eye(4).reshape(-1).tolist()), (11, 'transforms', list(rows)),
                          (4, 'camera', list(camera))):
        for bad in (NAN, INF):
            values = list(base)
            values[k] = bad
            assert integrate(**{name: floats(values)}) != 0, (name, bad)
            assert b'non-finite ' + name.rstrip('s').encode() in error(), (name, bad, error())

    origin = floats([0.0, 0.0, 0.0])

    def extract(tsdf=t, weight=w, origin=origin, voxel_size=0.1, min_weight=1.0, points=pts, normals=nrm, index=idx,
                offsets=off, capacity=10, dims=(4, 3, 2), workspace=ws, workspace_bytes=512):
        return lib.pds_tsdf_extract_fwd(tsdf, weight, origin, voxel_size, min_weight, points, normals, index, offsets,
                                        capacity, *dims, workspace, workspace_bytes, None)

    for name in ('tsdf', 'weight', 'origin', 'points', 'offsets', 'workspace'):
        assert extract(**{name: None}) != 0 and error() == b'tsdf_extract: null pointer', name
    assert extract(dims=(4, 0, 2)) != 0 and b'tsdf: bad volume' in error()
    assert extract(dims=(895, 895, 895)) != 0 and b'does not fit' in error()
    assert extract(capacity=-1) != 0 and b'capacity must be >= 0 (got -1)' in error()
    assert extract(workspace_bytes=511) != 0 and b'workspace too small (511 < 512)' in error()
    for bad in (0.0, -1.0, NAN, INF):
        assert extract(voxel_size=bad) != 0 and b'voxel_size must be positive and finite' in error(), bad
    assert extract(min_weight=NAN) != 0 and b'min_weight is NaN' in error()
    assert extract(origin=floats([0.0, NAN, 0.0])) != 0 and b'non-finite origin' in error()
    assert extract(points=ctypes.c_void_p(pts.value + 2)) != 0 and b'not 4-byte aligned' in error()
    assert extract(normals=ctypes.c_void_p(nrm.value + 1)) != 0 and b'not 4-byte aligned' in error()
    assert extract(points=t) != 0 and b'an output aliases an input' in error()
    assert extract(index=ctypes.c_void_p(w.value + 92)) != 0 and b'an output aliases an input' in error()
    assert extract(normals=ctypes.c_void_p(pts.value + 116)) != 0 and b'an output aliases another output' in error()
    assert extract(offsets=ctypes.c_void_p(idx.value + 36)) != 0 and b'an output aliases another output' in error()
    assert extract(workspace=ctypes.c_void_p(off.value + 4)) != 0 and b'an output aliases another output' in error()
    # capacity 0 holds no row, so nothing can overlap there
    assert extract(capacity=0, normals=pts, workspace_bytes=511) != 0 and b'workspace too small' in error()


# ------------------------------------------------------------------------------------------------ Python
def test_tsdf_volume_python_errors():
    def make(origin=(0.0, 0.0, 0.0), voxel_size=0.1, dims=(4, 3, 2), truncation=0.3, **kw):
        return pds.TsdfVolume(origin, voxel_size, dims, truncation, **kw)

    for bad in ((0.0, NAN, 0.0), (INF, 0.0, 0.0), (0.0, 0.0), (0.0,) * 4):
        with pytest.raises(ValueError, match='origin must hold 3 finite values'):
            make(origin=bad, device='cpu')
    for name in ('voxel_size', 'truncation', 'max_weight'):
        for bad in (0.0, -1.0, NAN):
            with pytest.raises(ValueError, match='%s must be positive' % name):
                make(device='cpu', **{name: bad})
        with pytest.raises(TypeError, match='%s must be a number' % name):
            make(device='cpu', **{name: 'thick'})
    with pytest.raises(ValueError, match='must be finite'):
        make(voxel_size=INF, device='cpu')
    for bad in ((4, 3), (4, 3, 2, 1), 7, (4.5, 3, 2), None):
        with pytest.raises(ValueError, match=r'dims must be three integers'):
            make(dims=bad, device='cpu')
    for bad in ((0, 3, 2), (4, -3, 2), (4, 3, 0)):
        with pytest.raises(ValueError, match=r'dims must be at least \(1, 1, 1\)'):
            make(dims=bad, device='cpu')
    for bad in (((1 << 24) + 1, 1, 1), (1, 1, 1 << 25)):
        with pytest.raises(ValueError, match=r'dims must be at most 2\^24 each'):
            make(dims=bad, device='cpu')
    for bad in ((895, 895, 895), (1 << 16, 1 << 16, 1)):
        with pytest.raises(ValueError, match='does not fit 32-bit indices'):
            make(dims=bad, device='cpu')
    # all of that comes before the device: what is left is that there is no CPU fallback
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        make(device='cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        simple_rig(64, 48).tsdf_volume((0.0, 0.0, 0.0), 0.1, (4, 3, 2), 0.3, device='cpu')
    parameters = inspect.signature(pds.TsdfVolume.__init__).parameters
    assert [(n, p.default) for n, p in parameters.items()][5:] == [('max_weight', 64.0), ('device', 'cuda')]
    parameters = inspect.signature(pds.TsdfVolume.integrate).parameters
    assert list(parameters)[1:3] == ['disparity', 'matrix']
    assert [(n, p.default) for n, p in parameters.items()][3:] == [
        ('pose', None), ('camera', None), ('valid', None), ('confidence', None), ('min_confidence', 0.0),
        ('weight_by_confidence', False)]
    parameters = inspect.signature(pds.TsdfVolume.extract_points).parameters
    assert [(n, p.default) for n, p in parameters.items()][1:] == [('min_weight', 1.0), ('with_normals', True),
                                                                   ('capacity', None), ('trim', True)]
    parameters = inspect.signature(pds.StereoRig.integrate).parameters
    assert [(n, p.default) for n, p in parameters.items()][3:] == [
        ('pose', None), ('valid', None), ('confidence', None), ('min_confidence', 0.0), ('weight_by_confidence', False)]
    for phrase in ('marching-cubes faces', 'raycasting', 'colour', 'depth-dependent truncation or weights',
                   'hashed or sparse volumes', 'pose estimation', 'no CPU fallback'):
        assert phrase in tsdf_module.__doc__, phrase


class HostVolume(pds.TsdfVolume):
    """A volume whose state stays on the host: the argument checks of integrate / extract_points run up to the point where
    they ask where the tensors live."""

    def __init__(self, *args, **kw):
        try:
            super(HostVolume, self).__init__(*args, device='cpu', **kw)
        except RuntimeError as e:
            assert 'no CPU fallback' in str(e)
        self._tsdf, self._weight = torch.ones(self.shape), torch.zeros(self.shape)


def test_integrate_and_extract_python_errors():
    volume = HostVolume((0.0, 0.0, 0.0), 0.1, (4, 3, 2), 0.3)
    assert volume.shape == (2, 3, 4) and volume.dims == (4, 3, 2) and volume.tsdf.shape == (2, 3, 4)
    ok, Q = torch.zeros(1, 4, 5), q_of(4, 5, 4.0, 0.5)

    def run(disparity=ok, matrix=Q, **kw):
        return volume.integrate(disparity, matrix, **kw)

    with pytest.raises(TypeError, match='disparity must be a torch.Tensor'):
        run(np.zeros((1, 4, 5), dtype=np.float32))
    for bad in (ok.double(), ok.half()):
        with pytest.raises(TypeError, match='disparity must be float32'):
            run(bad)
    for bad in (torch.zeros(4, 5), torch.zeros(1, 1, 4, 5)):
        with pytest.raises(ValueError, match='disparity must have 3 dimensions'):
            run(bad)
    with pytest.raises(ValueError, match='empty input'):
        run(torch.zeros(0, 4, 5))
    for bad in (np.eye(3), np.full((4, 4), NAN)):
        with pytest.raises(ValueError, match='matrix must be a finite 4x4'):
            run(matrix=bad)
    for bad in (np.eye(3), np.eye(4), np.full((3, 4), NAN), np.zeros((2, 3, 4)), np.zeros((1, 4, 3))):
        with pytest.raises(ValueError, match=r'pose must be a finite 3x4 \[R \| t\] or \[1, 3, 4\]'):
            run(pose=bad)
    # camera=None reads the pinhole off a canonical matrix and refuses any other
    assert tsdf_module.camera_of_matrix(Q) == camera_of(Q) == (4.0, 4.0, 2.0, 1.5, 0.0)
    skewed = Q.copy()
    skewed[0, 1] = 0.01
    rotated = np.diag([1.0, -1.0, -1.0, 1.0]) @ Q
    for bad in (skewed, rotated, simple_rig(64, 48).reprojection_matrix('camera') @ np.diag([2.0, 1.0, 1.0, 1.0])):
        with pytest.raises(ValueError, match='camera=None needs a matrix of the canonical rectified form'):
            run(matrix=bad)
    for bad in ((4.0, 4.0, 2.0, 1.5), (4.0,) * 6):
        with pytest.raises(ValueError, match='camera must hold 5 values'):
            run(camera=bad)
    with pytest.raises(ValueError, match='camera has non-finite entries'):
        run(camera=(4.0, NAN, 2.0, 1.5, 0.0))
    with pytest.raises(ValueError, match='camera must have positive focal lengths'):
        run(camera=(0.0, 4.0, 2.0, 1.5, 0.0))
    for bad in (NAN, INF):
        with pytest.raises(ValueError, match='min_confidence must be finite'):
            run(min_confidence=bad)
    for valid in (torch.ones(1, 4, 5), torch.ones(1, 4, 6, dtype=torch.bool)):
        with pytest.raises(ValueError, match='valid must be torch.bool'):
            run(valid=valid)
    with pytest.raises(TypeError, match='valid must be a torch.Tensor'):
        run(valid=np.ones((1, 4, 5), dtype=bool))
    with pytest.raises(TypeError, match='confidence must be float32'):
        run(confidence=ok.double())
    with pytest.raises(ValueError, match='confidence .* differ in shape'):
        run(confidence=torch.zeros(1, 5, 4))
    with pytest.raises(ValueError, match='weight_by_confidence needs a confidence'):
        run(weight_by_confidence=True)
    # every argument in order, and still no CPU fallback
    for kwargs in ({}, {'pose': np.zeros((1, 3, 4)), 'camera': (4.0, 4.0, 2.0, 1.5, 0.1), 'matrix': skewed,
                        'valid': torch.ones(1, 4, 5, dtype=torch.bool), 'confidence': ok, 'min_confidence': 0.5,
                        'weight_by_confidence': True}):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            run(**kwargs)
    rig = simple_rig(64, 48)
    with pytest.raises(TypeError, match='volume must be a TsdfVolume'):
        rig.integrate(None, torch.zeros(1, 48, 64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rig.integrate(volume, torch.zeros(1, 48, 64), pose=IDENTITY)
    # the state: settable with the same shape, dtype and device only
    volume.tsdf = torch.full((2, 3, 4), 0.5)
    assert float(volume.tsdf[0, 0, 0]) == 0.5
    with pytest.raises(TypeError, match='tsdf must be a torch.Tensor'):
        volume.tsdf = np.ones((2, 3, 4), dtype=np.float32)
    for bad in (torch.ones(4, 3, 2), torch.ones(2, 3, 4, dtype=torch.float64)):
        with pytest.raises(ValueError, match=r'weight must be float32 \(2, 3, 4\)'):
            volume.weight = bad
    with pytest.raises(ValueError, match='tsdf must be contiguous'):
        volume.tsdf = torch.ones(2, 3, 8)[:, :, ::2]
    # extract_points
    with pytest.raises(ValueError, match='min_weight is NaN'):
        volume.extract_points(min_weight=NAN)
    with pytest.raises(ValueError, match='capacity must be >= 0'):
        volume.extract_points(capacity=-1)
    with pytest.raises(TypeError, match='capacity must be an integer or None'):
        volume.extract_points(capacity=1.5)
    # the transforms the host folds the pose into: A = voxel_size R, b = R (origin + voxel_size / 2) + t
    other = HostVolume((1.0, 2.0, 3.0), 0.5, (2, 2, 2), 1.0)
    turn = np.array([[0.0, -1.0, 0.0, 10.0], [1.0, 0.0, 0.0, 20.0], [0.0, 0.0, 1.0, 30.0]])
    rows = other.transforms(np.stack([IDENTITY, turn]), 2)
    assert rows[0].tolist() == [0.5, 0, 0, 0, 0.5, 0, 0, 0, 0.5, 1.25, 2.25, 3.25]
    assert rows[1].tolist() == [0, -0.5, 0, 0.5, 0, 0, 0, 0, 0.5, -2.25 + 10, 1.25 + 20, 3.25 + 30]
    assert other.transforms(None, 3).tolist() == [rows[0].tolist()] * 3
