"""CPU: frame-to-model tracking (pds_icp_workspace_bytes, pds_icp_system_fwd; icp_system, icp_solve, se3_exp,
TsdfVolume.track, StereoRig.track).  The entry points are declared, exported and bound and validate without a GPU; the
Python surface refuses what it cannot run.

oracle_rows is the numpy fp64 oracle of tests/test_gpu_icp.py: steps 1 - 7 of tracking.py on the matrix, the transform,
the camera, max_distance and min_cosine as the entry point gets them (rounded once to float32).  It is held to hand-written
answers below.  It does not decide what fp32 cannot.  With EPS of tests/test_register_depth_host.py (relative: about twenty
fp32 roundings; the longest chain here, disparity -> P -> q -> x -> u, has fourteen) and c = (x, y, d, 1):

    P_m = (M_m . c) / W   E_P = EPS (sum_k |M_mk c_k| / |W| + |P_m| (1 + sum_k |M_3k c_k| / |W|)): the numerator's sum,
                          the denominator's, the division.  W > 0 is undecided where |W| <= EPS sum_k |M_3k c_k|
    q_a = R_a . P + t_a   E_q = sum_m |R_am| E_P_m + EPS (sum_m |R_am P_m| + |t_a|); q_z > 0 is undecided where |q_z| <= E_qz
    x = q_x / q_z         E_x = (E_qx + |x| E_qz) / q_z + EPS |x|, and y likewise
    u = fx x + skew y + cx  E_u = fx E_x + |skew| E_y + EPS (|fx x| + |skew y| + |cx| + |u| + 0.5);
    v = fy y + cy           E_v = fy E_y + EPS (|fy y| + |cy| + |v| + 0.5)
                          px = floor(u + 0.5) is undecided where u + 0.5 lies within E_u of an integer, py likewise
    m = Z (x_m, y_m, 1)   Z and (px, py) are exact: E_m = EPS |m_a|
    e = m - q             E_e = E_m + E_q + EPS |e_a|; with s = sum_a e_a^2: E_s = sum_a 2 |e_a| E_e_a + EPS s.  The test
                          s <= max_distance^2 (the square rounded in fp32: EPS max_distance^2) is undecided within the two
    cos = (R n_f) . n     E_c = EPS sum_a sum_m |R_am n_fm n_a|; cos >= min_cosine is undecided within E_c

An undecided pixel may hold a row or NaNs.  Everything else is compared: a decided pixel has a row exactly where the
oracle has one, and every component lies within its bound.  The bound follows the rule of tests/test_surface_normals_host.py:
the same formulas restated in float32 numpy (every operation rounded to float32, no fused multiply-add) are compared with
the fp64 oracle, component by component, relative to the component's SCALE -- the sum of the absolute values of the terms
it is made of, down to P: with Q_a = sum_m |R_am P_m| + |t_a| (q_a itself may have cancelled), Q_y |n_z| + Q_z |n_y| for
J_0, sum_a |n_a| (|m_a| + Q_a) for r, and 0 for J_3 .. J_5, which are copies of the model's normal.  REL32 is the largest such ratio over the scenes of the GPU file (measured here, on the CPU, never
against the kernel: test_the_restatement_stays_within_its_measured_error prints it), and the kernel is held to
4 * REL32 * scale per pixel and component; the factor covers the fused multiply-adds and the compiler's contraction inside
the shared reproject_one.

The tracking scene: three mutually non-parallel planes (a floor, a back wall, a side wall) meet in a corner; the disparity
of a frame is the ray-plane intersection in fp64.  Frame 0 is fused with oracle_integrate into a 40 x 32 x 32 volume of 3 cm
voxels, rendered with oracle_raycast at the pose of frame 0, and frame 1 -- 0.021 rad and 4.4 cm (1.5 voxels) away -- is
tracked against it by oracle_track, the fp64 loop of TsdfVolume.track.  The conditions of the GPU test are asserted here on
the oracle alone: the undecided share stays below 2 % of the rows at every iteration, at least 20 % of the pixels give rows,
and the pose error falls by at least 10 x in ten iterations."""
import collections
import ctypes
import functools
import inspect
import math

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib, tracking
from tests.test_register_depth_host import EPS, simple_rig
from tests.test_tsdf_host import HostVolume, camera_of, f32, fresh_state, oracle_integrate, q_of
from tests.test_tsdf_raycast_host import oracle_raycast

NAN, INF = float('nan'), float('inf')
TILE = 1024     # csrc/common.hpp: kIcpTile
SYSTEM = 29     # csrc/common.hpp: kIcpSystem
IDENTITY = np.hstack([np.eye(3), np.zeros((3, 1))])
# measured by test_the_restatement_stays_within_its_measured_error: the largest error of the float32 restatement against
# the fp64 oracle relative to the component's scale, over the scenes of tests/test_gpu_icp.py; the GPU is held to 4 x
REL32 = 2.4e-7   # (measured 2.351e-07, on the aligned corner scene)

# rows [H, W, 7] fp64 (NaN where none); mask, undecided [H, W] bool; bound [H, W, 7] fp64; scale [H, W, 7];
# rows32 [H, W, 7]: the float32 restatement (NaN where IT has none)
Rows = collections.namedtuple('Rows', ['rows', 'mask', 'undecided', 'bound', 'scale', 'rows32'])


# ------------------------------------------------------------------------------------------------ the oracle
def _steps(ft, d, M, T, camera, depth, normals_m, frame_normals, valid, confidence, min_confidence, max_distance,
           min_cosine, margins):
    """Steps 1 - 7 in the float type ft on float32 inputs -> (rows [H, W, 7], mask, undecided, scale)."""
    height, width = d.shape
    hm, wm = depth.shape
    c = (lambda a: np.asarray(a, dtype=ft))
    yy, xx = np.mgrid[0:height, 0:width]
    xx, yy, dd = c(xx), c(yy), c(d)
    M, T = c(M), c(T)
    fx, fy, cx, cy, skew = (ft(v) for v in camera)
    half = ft(0.5)
    with np.errstate(all='ignore'):
        X, Y, Z, W = (M[r, 0] * xx + M[r, 1] * yy + M[r, 2] * dd + M[r, 3] for r in range(4))
        kept = np.isfinite(d) & (d > 0) & (W > 0)
        if valid is not None:
            kept &= np.asarray(valid, dtype=bool)
        if confidence is not None:
            kept &= np.asarray(confidence, dtype=np.float32) >= np.float32(min_confidence)
        P = [X / W, Y / W, Z / W]
        q = [T[a, 0] * P[0] + T[a, 1] * P[1] + T[a, 2] * P[2] + T[a, 3] for a in range(3)]
        front = kept & (q[2] > 0) & np.isfinite(q[0]) & np.isfinite(q[1]) & np.isfinite(q[2])
        x, y = q[0] / q[2], q[1] / q[2]
        u, v = fx * x + skew * y + cx, fy * y + cy
        fu, fv = np.floor(u + half), np.floor(v + half)
        inside = front & (fu >= 0) & (fu < wm) & (fv >= 0) & (fv < hm)
        px = np.where(inside, fu, 0).astype(np.int64)
        py = np.where(inside, fv, 0).astype(np.int64)
        Zm, n = c(depth)[py, px], c(normals_m)[py, px]
        seen = inside & ~np.isnan(Zm) & ~np.isnan(n).any(axis=-1)
        ym = (c(py) - cy) / fy
        xm = (c(px) - cx - skew * ym) / fx
        m = [Zm * xm, Zm * ym, Zm]
        e = [m[a] - q[a] for a in range(3)]
        s = e[0] * e[0] + e[1] * e[1] + e[2] * e[2]
        limit = ft(np.float32(max_distance)) * ft(np.float32(max_distance))
        mask = seen & (s <= limit)
        if frame_normals is not None:
            nf = c(frame_normals)
            turned = [T[a, 0] * nf[..., 0] + T[a, 1] * nf[..., 1] + T[a, 2] * nf[..., 2] for a in range(3)]
            cosine = turned[0] * n[..., 0] + turned[1] * n[..., 1] + turned[2] * n[..., 2]
            mask &= ~np.isnan(nf).any(axis=-1) & (cosine >= ft(np.float32(min_cosine)))
        r = n[..., 0] * e[0] + n[..., 1] * e[1] + n[..., 2] * e[2]
        J = [q[1] * n[..., 2] - q[2] * n[..., 1], q[2] * n[..., 0] - q[0] * n[..., 2], q[0] * n[..., 1] - q[1] * n[..., 0]]
        rows = np.stack(J + [n[..., 0], n[..., 1], n[..., 2], r], axis=-1).astype(np.float64)
        rows = np.where(mask[..., None], rows, NAN)
        if not margins:
            return rows, mask, None, None
        # ---- what fp32 cannot decide (the derivation is in the module text)
        eps = EPS
        cc = [np.abs(xx), np.abs(yy), np.abs(dd), np.ones_like(dd)]
        mass = [sum(abs(M[r, k]) * cc[k] for k in range(4)) for r in range(4)]
        undecided = kept & (np.abs(W) <= eps * mass[3])
        E_P = [eps * (mass[a] / np.abs(W) + np.abs(P[a]) * (1 + mass[3] / np.abs(W))) for a in range(3)]
        E_q = [sum(abs(T[a, k]) * E_P[k] for k in range(3)) +
               eps * (sum(np.abs(T[a, k] * P[k]) for k in range(3)) + abs(T[a, 3])) for a in range(3)]
        undecided |= kept & (np.abs(q[2]) <= E_q[2])
        E_x = (E_q[0] + np.abs(x) * E_q[2]) / q[2] + eps * np.abs(x)
        E_y = (E_q[1] + np.abs(y) * E_q[2]) / q[2] + eps * np.abs(y)
        E_u = fx * E_x + abs(skew) * E_y + eps * (np.abs(fx * x) + np.abs(skew * y) + abs(cx) + np.abs(u) + 0.5)
        E_v = fy * E_y + eps * (np.abs(fy * y) + abs(cy) + np.abs(v) + 0.5)
        for coordinate, error, size in ((u, E_u, wm), (v, E_v, hm)):
            t = coordinate + 0.5
            near = np.abs(t - np.round(t)) <= error
            undecided |= front & near & (t > -1) & (t < size + 1)
        E_e = [eps * np.abs(m[a]) + E_q[a] + eps * np.abs(e[a]) for a in range(3)]
        E_s = sum(2 * np.abs(e[a]) * E_e[a] for a in range(3)) + eps * s
        undecided |= seen & (np.abs(s - limit) <= E_s + eps * limit)
        if frame_normals is not None:
            E_c = eps * sum(np.abs(T[a, k] * nf[..., k] * n[..., a]) for a in range(3) for k in range(3))
            undecided |= seen & (np.abs(cosine - ft(np.float32(min_cosine))) <= E_c)
        Q_ = [sum(np.abs(T[a, k] * P[k]) for k in range(3)) + abs(T[a, 3]) for a in range(3)]   # the terms of q_a
        na = [np.abs(n[..., a]) for a in range(3)]
        scale = np.stack([Q_[1] * na[2] + Q_[2] * na[1], Q_[2] * na[0] + Q_[0] * na[2], Q_[0] * na[1] + Q_[1] * na[0],
                          np.zeros_like(r), np.zeros_like(r), np.zeros_like(r),
                          sum(na[a] * (np.abs(m[a]) + Q_[a]) for a in range(3))], axis=-1)
    return rows, mask, undecided, np.where(mask[..., None], scale, 0.0)


def oracle_rows(disparity, matrix, depth, normals, camera, transform=None, frame_normals=None, valid=None,
                confidence=None, min_confidence=0.0, max_distance=0.1, min_cosine=0.0):
    """One entry: disparity [H, W], the model's depth [Hm, Wm] and normals [Hm, Wm, 3] (float32 values), transform 3x4
    or None -> Rows."""
    d = np.asarray(disparity, dtype=np.float32)
    depth, normals = np.asarray(depth, dtype=np.float32), np.asarray(normals, dtype=np.float32)
    assert d.ndim == 2 and depth.ndim == 2 and normals.shape == depth.shape + (3,)
    M, T = f32(matrix), f32(IDENTITY if transform is None else transform)
    cam = f32(camera)
    if frame_normals is not None:
        frame_normals = np.asarray(frame_normals, dtype=np.float32)
    args = (depth, normals, frame_normals, valid, confidence, min_confidence, max_distance, min_cosine)
    rows, mask, undecided, scale = _steps(np.float64, d, M, T, cam, *args, margins=True)
    rows32 = _steps(np.float32, d, M.astype(np.float32), T.astype(np.float32), cam.astype(np.float32), *args,
                    margins=False)[0]
    return Rows(rows, mask, undecided, 4.0 * REL32 * scale, scale, rows32)


def restatement_error(o):
    """The largest |rows32 - rows| / scale over the decided rows both have (0 without any)."""
    both = o.mask & ~o.undecided & ~np.isnan(o.rows32[..., 6])
    with np.errstate(all='ignore'):
        ratio = np.abs(o.rows32 - o.rows) / o.scale
    ratio = np.where(both[..., None] & (o.scale > 0), ratio, 0.0)
    assert (o.rows32[..., 3:6][both] == o.rows[..., 3:6][both]).all()   # copies of the model's normal
    return float(ratio.max(initial=0.0))


def check_rows(got, o, case=''):
    """got float32 [H, W, 7] against Rows -> (decided rows compared, the largest share of the bound)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == o.rows.shape, case
    has = ~np.isnan(got[..., 6])
    assert (np.isnan(got).all(axis=-1) == ~has).all() and (np.isnan(got).any(axis=-1) == ~has).all(), case
    decided = ~o.undecided
    wrong = decided & (has != o.mask)
    assert not wrong.any(), (case, 'rows where the oracle has none or none where it has: %d' % int(wrong.sum()))
    compared = decided & o.mask
    error = np.abs(got.astype(np.float64) - o.rows)[compared]
    bound = o.bound[compared]
    assert (error <= bound).all(), (case, float((error - bound).max()))
    with np.errstate(all='ignore'):
        share = float(np.where(bound > 0, error / bound, 0.0).max(initial=0.0))
    return int(compared.sum()), share


_TRIANGLE = np.triu_indices(6)


def oracle_system(rows):
    """rows [..., 7] (NaN rows: none) -> the 29 fp64 values of one entry."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 7)
    rows = rows[~np.isnan(rows[:, 6])]
    J, r = rows[:, :6], rows[:, 6]
    A = J.T @ J
    return np.concatenate([A[_TRIANGLE], J.T @ r, [r @ r], [float(len(rows))]])


def system_terms(rows):
    """-> (the 29 sums of |term|, the count): the yardstick of a summation in any order."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 7)
    rows = np.abs(rows[~np.isnan(rows[:, 6])])
    J, r = rows[:, :6], rows[:, 6]
    return np.concatenate([(J.T @ J)[_TRIANGLE], J.T @ r, [r @ r], [0.0]]), len(rows)


def exact_system(rows):
    """float32 rows [..., 7] -> (the 29 sums, each the EXACT sum of its fp64 products rounded once (math.fsum; a product
    of two float32 is exact in fp64), the 29 sums of |term|, the count).  A summation of n such terms in fp64 in any
    order lies within (n - 1) 2^-53 sum |term| of the exact sum, and this reference within 2^-53 |sum| of it: a kernel's
    sum lies within n 2^-53 sum |term| of this one, whatever its order."""
    rows = np.asarray(rows)
    assert rows.dtype == np.float32
    rows = rows.reshape(-1, 7).astype(np.float64)
    rows = rows[~np.isnan(rows[:, 6])]
    pairs = [(i, j) for i in range(6) for j in range(i, 6)] + [(i, 6) for i in range(6)] + [(6, 6)]
    sums = [math.fsum((rows[:, i] * rows[:, j]).tolist()) for i, j in pairs] + [float(len(rows))]
    terms = [math.fsum(np.abs(rows[:, i] * rows[:, j]).tolist()) for i, j in pairs] + [0.0]
    return np.array(sums), np.array(terms), len(rows)


def pose_error(pose, truth):
    """-> (rotation angle, translation norm) of pose o truth^-1."""
    E = tracking.compose(np.asarray(pose), tracking.invert(np.asarray(truth)))
    return float(np.linalg.norm(pds.rectification.rodrigues_inverse(E[:, :3]))), float(np.linalg.norm(E[:, 3]))


# ------------------------------------------------------------------------------------------------ the wall, by hand
WALL = dict(height=21, width=37, focal=64.0, baseline=0.125, disparity=4.0, depth=2.0, model_depth=1.9375, delta=0.0625)


def wall_case(height=None, width=None, slope=0.0):
    """-> (disparity [H, W], Q, model depth [H, W], model normals [H, W, 3], camera): a frontal wall frame at depth 2 and a
    wall model at 1.9375 (+ slope per column) with normals (0, 0, -1), through the same camera."""
    height, width = height or WALL['height'], width or WALL['width']
    Q = q_of(height, width, WALL['focal'], WALL['baseline'])
    d = np.full((height, width), WALL['disparity'], dtype=np.float32)
    depth = (WALL['model_depth'] + slope * np.arange(width)[None, :] * np.ones((height, 1))).astype(np.float32)
    normals = np.zeros((height, width, 3), dtype=np.float32)
    normals[..., 2] = -1.0
    return d, Q, depth, normals, camera_of(Q)


def test_oracle_wall_by_hand():
    d, Q, depth, normals, camera = wall_case()
    o = oracle_rows(d, Q, depth, normals, camera, max_distance=0.1)
    assert o.mask.all() and not o.undecided.any()
    yy, xx = np.mgrid[0:21, 0:37].astype(np.float64)
    X, Y = (xx - 18.0) * 2.0 / 64.0, (yy - 10.0) * 2.0 / 64.0
    # q = (X, Y, 2), n = (0, 0, -1): q x n = (-Y, X, 0); e = (.., .., -0.0625): r = 0.0625
    hand = np.stack([-Y, X, np.zeros_like(X), np.zeros_like(X), np.zeros_like(X), -np.ones_like(X),
                     np.full_like(X, WALL['delta'])], axis=-1)
    assert np.abs(o.rows - hand).max() <= 1e-12
    assert restatement_error(o) <= REL32
    # too far: no row anywhere; the distance test is undecided when the limit is the distance itself
    assert not oracle_rows(d, Q, depth, normals, camera, max_distance=0.0624).mask.any()
    # (e = -delta (x, y, 1) along the pixel's ray: exactly delta long at the principal point (18, 10), longer elsewhere)
    limit = oracle_rows(d, Q, depth, normals, camera, max_distance=0.0625)
    assert limit.undecided[10, 18] and not limit.undecided[0, 0] and int((limit.mask & ~limit.undecided).sum()) == 0
    assert limit.undecided.sum() < 0.1 * limit.undecided.size
    # the system of this wall by hand: sum J J^T over the pixel grid
    s = oracle_system(o.rows)
    A, g, rr, count = tracking.unpack_system(s)
    assert count[0] == 21 * 37 and abs(rr[0] - 21 * 37 * WALL['delta'] ** 2) <= 1e-12
    assert abs(A[0, 0, 0] - (Y * Y).sum()) <= 1e-9 and abs(A[0, 1, 1] - (X * X).sum()) <= 1e-9
    assert abs(A[0, 0, 1] + (X * Y).sum()) <= 1e-9 and abs(A[0, 5, 5] - 21 * 37) <= 1e-12
    assert abs(g[0, 5] + 21 * 37 * WALL['delta']) <= 1e-12 and (A[0, 2] == 0).all() and (A[0] == A[0].T).all()
    # a masked pixel, a NaN disparity, a NaN model pixel and a frame normal that looks away give no row
    valid = np.ones((21, 37), dtype=bool)
    valid[3, 4] = False
    holes = d.copy()
    holes[5, 6] = NAN
    model = depth.copy()
    model[7, 8] = NAN
    facing = np.zeros((21, 37, 3), dtype=np.float32)
    facing[..., 2] = -1.0
    facing[9, 10] = (0.0, 0.0, 1.0)
    facing[11, 12] = NAN
    o = oracle_rows(holes, Q, model, normals, camera, frame_normals=facing, valid=valid, min_cosine=0.5)
    gone = [(3, 4), (5, 6), (7, 8), (9, 10), (11, 12)]
    assert int(o.mask.sum()) == 21 * 37 - 5 and not any(o.mask[p] for p in gone) and not o.undecided.any()


def test_oracle_half_a_pixel_moves_the_association():
    d, Q, depth, normals, camera = wall_case(slope=0.001)
    pixel = 2.0 / 64.0   # the width of a pixel at depth 2
    shifted = IDENTITY.copy()
    shifted[0, 3] = 0.75 * pixel
    o = oracle_rows(d, Q, depth, normals, camera, transform=shifted, max_distance=0.1)
    # u = x + 0.75: px = x + 1; the last column leaves the image
    assert o.mask[:, :-1].all() and not o.mask[:, -1].any() and not o.undecided.any()
    xx = np.arange(36, dtype=np.float64)
    model_z = f32(WALL['model_depth'] + 0.001 * (xx + 1))
    assert np.abs(o.rows[4, :-1, 6] - (2.0 - model_z)).max() <= 1e-12   # r = -(Z_m - q_z)
    # exactly half a pixel: fp32 cannot say
    shifted[0, 3] = 0.5 * pixel
    assert oracle_rows(d, Q, depth, normals, camera, transform=shifted, max_distance=0.1).undecided.all()
    shifted[0, 3] = 0.25 * pixel
    o = oracle_rows(d, Q, depth, normals, camera, transform=shifted, max_distance=0.1)
    assert o.mask.all() and not o.undecided.any()
    assert np.abs(o.rows[4, :, 6] - (2.0 - f32(WALL['model_depth'] + 0.001 * np.arange(37.0)))).max() <= 1e-12


def test_oracle_system_against_a_hand_sum():
    rows = np.array([[1.0, 2.0, 0.0, 0.0, 0.0, 1.0, 0.5], [NAN] * 7, [0.0, 1.0, 3.0, 1.0, 0.0, 0.0, -2.0]])
    s = oracle_system(rows)
    assert len(s) == SYSTEM and s[28] == 2 and s[27] == 0.25 + 4.0
    A, g, rr, count = tracking.unpack_system(s)
    assert A[0, 0, 0] == 1 and A[0, 0, 1] == 2 and A[0, 1, 1] == 5 and A[0, 1, 2] == 3 and A[0, 2, 2] == 9
    assert A[0, 0, 5] == 1 and A[0, 1, 5] == 2 and A[0, 2, 3] == 3 and A[0, 3, 3] == 1 and A[0, 5, 5] == 1
    assert g[0].tolist() == [0.5, 1.0 - 2.0, -6.0, -2.0, 0.0, 0.5]
    terms, count = system_terms(rows)
    assert count == 2 and terms[21:27].tolist() == [0.5, 3.0, 6.0, 2.0, 0.0, 0.5] and terms[28] == 0
    assert oracle_system(np.full((4, 7), NAN)).tolist() == [0.0] * SYSTEM
    sums, exact_terms, exact_count = exact_system(rows.astype(np.float32))
    assert (sums == s).all() and (exact_terms == terms).all() and exact_count == 2


# ------------------------------------------------------------------------------------------------ solve, exp
def test_icp_solve_refuses_the_wall_and_recovers_a_twist():
    d, Q, depth, normals, camera = wall_case()
    wall = oracle_system(oracle_rows(d, Q, depth, normals, camera).rows)
    s = pds.icp_solve(wall[None], min_count=100, min_eigenvalue=1e-4)
    assert s.status.tolist() == [tracking.DEGENERATE] and (s.xi == 0).all() and s.count.tolist() == [21 * 37]
    assert abs(s.rmse[0] - WALL['delta']) <= 1e-12
    assert pds.icp_solve(wall[None], min_count=1000).status.tolist() == [tracking.TOO_FEW_ROWS]
    empty = pds.icp_solve(np.zeros((1, SYSTEM)))
    assert empty.status.tolist() == [tracking.TOO_FEW_ROWS] and np.isnan(empty.rmse[0])
    rng = np.random.RandomState(3)
    J = rng.randn(500, 6)
    truth = np.array([0.01, -0.02, 0.015, 0.03, -0.01, 0.02])
    rows = np.concatenate([J, (J @ truth)[:, None]], axis=1)
    both = np.stack([oracle_system(rows), wall])
    s = pds.icp_solve(both)
    assert s.status.tolist() == [tracking.TRACKED, tracking.DEGENERATE]
    assert np.abs(s.xi[0] - truth).max() <= 1e-12 and s.count.tolist() == [500, 21 * 37]
    assert abs(s.rmse[0] - math.sqrt(((J @ truth) ** 2).mean())) <= 1e-12
    assert np.abs(pds.icp_solve(torch.from_numpy(both)).xi[0] - truth).max() <= 1e-12
    with pytest.raises(ValueError, match=r'system must be \[B, 29\]'):
        pds.icp_solve(np.zeros((2, 28)))


def test_se3_exp_against_rodrigues_and_the_closed_form():
    assert (pds.se3_exp(np.zeros(6)) == IDENTITY).all()
    assert (pds.se3_exp([0, 0, 0, 1.0, -2.0, 3.0]) == np.hstack([np.eye(3), [[1.0], [-2.0], [3.0]]])).all()
    for omega in ((0.3, -0.2, 0.5), (1e-3, 2e-3, -1e-3), (3e-5, 0.0, 4e-5), (1e-9, 0, 0), (0.0, 2.0, 0.0)):
        w, v = np.array(omega), np.array([0.1, -0.4, 0.25])
        T = pds.se3_exp(np.concatenate([w, v]))
        assert np.abs(T[:, :3] - pds.rectification.rodrigues(w)).max() == 0
        # the matrix exponential of the 4x4 twist, by its series
        X = np.zeros((4, 4))
        X[:3, :3] = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
        X[:3, 3] = v
        term, total = np.eye(4), np.eye(4)
        for k in range(1, 40):
            term = term @ X / k
            total = total + term
        assert np.abs(T - total[:3]).max() <= 1e-14, omega
    # a pure rotation about z by a quarter turn with v along x: the screw's closed form
    T = pds.se3_exp([0, 0, math.pi / 2, 1.0, 0, 0])
    assert np.abs(T[:, 3] - np.array([2 / math.pi, 2 / math.pi, 0.0])).max() <= 1e-15
    with pytest.raises(ValueError, match='xi must hold 6 finite values'):
        pds.se3_exp(np.zeros(5))
    with pytest.raises(ValueError, match='xi must hold 6 finite values'):
        pds.se3_exp([0, 0, NAN, 0, 0, 0])


# ------------------------------------------------------------------------------------------------ the corner scene
CORNER = dict(height=48, width=64, focal=60.0, baseline=0.12, dims=(40, 32, 32), voxel_size=0.03,
              origin=(-0.6, -0.5, 0.75), truncation=0.09,
              planes=(((0.0, 1.0, 0.0), 0.3), ((0.3, 0.0, 1.0), 1.45), ((1.0, 0.0, 0.2), 0.75)))
POSE0 = np.hstack([pds.rectification.rodrigues(np.array([0.01, -0.02, 0.005])), [[0.004], [-0.003], [0.002]]])
MOTION = np.hstack([pds.rectification.rodrigues(np.array([0.012, -0.015, 0.008])), [[0.03], [-0.02], [0.025]]])
POSE1 = tracking.compose(MOTION, POSE0)   # world -> frame 1: 0.021 rad and 4.4 cm from frame 0
TRACK = dict(iterations=10, min_count=100, min_eigenvalue=1e-4, tolerance=1e-6)


def corner_matrix():
    return q_of(CORNER['height'], CORNER['width'], CORNER['focal'], CORNER['baseline'])


def corner_disparity(pose, size=None):
    """The disparity [H, W] float32 of the corner seen from `pose` (world -> camera): the nearest ray-plane intersection."""
    height, width = size or (CORNER['height'], CORNER['width'])
    Q = q_of(height, width, CORNER['focal'] * width / CORNER['width'], CORNER['baseline'])
    fx, fy, cx, cy, _ = camera_of(Q)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    rays = np.stack([(xx - cx) / fx, (yy - cy) / fy, np.ones_like(xx)], axis=-1) @ pose[:, :3]   # R^T dir, per pixel
    centre = -pose[:, :3].T @ pose[:, 3]
    best = np.full((height, width), INF)
    for normal, offset in CORNER['planes']:
        normal = np.array(normal)
        with np.errstate(all='ignore'):
            t = (offset - normal @ centre) / (rays @ normal)
        best = np.where((t > 0) & (t < best), t, best)
    return (Q[2, 3] / (best * Q[3, 2])).astype(np.float32)   # Z = f / (a d)


@functools.lru_cache(maxsize=None)
def corner_state():
    """-> (tsdf, weight) float32 after frame 0, by oracle_integrate."""
    o = oracle_integrate(*fresh_state(CORNER['dims']), disparity=corner_disparity(POSE0), matrix=corner_matrix(),
                         origin=CORNER['origin'], voxel_size=CORNER['voxel_size'], truncation=CORNER['truncation'],
                         pose=POSE0)
    return o.tsdf.astype(np.float32), o.weight.astype(np.float32)


@functools.lru_cache(maxsize=None)
def corner_model(pose_key=0):
    """-> (depth [H, W], normals [H, W, 3]) float32: the oracle's raycast of corner_state at POSE0."""
    tsdf, weight = corner_state()
    rays = oracle_raycast(tsdf, weight, CORNER['origin'], CORNER['voxel_size'], camera_of(corner_matrix()),
                          (CORNER['width'], CORNER['height']), pose=POSE0, truncation=CORNER['truncation'])
    return rays.depth.astype(np.float32), rays.normals.astype(np.float32)


def oracle_track(disparity, matrix, depth, normals, camera, predicted, iterations=10, max_distance=0.1, min_count=100,
                 min_eigenvalue=1e-4, tolerance=1e-6, truth=None, **kw):
    """The loop of TsdfVolume.track in fp64 on the oracle's rows -> (pose 3x4, [per iteration (rows, undecided rows,
    rotation error, translation error before the step)], status)."""
    T = IDENTITY.copy()
    history, status = [], tracking.TRACKED
    for _ in range(iterations):
        o = oracle_rows(disparity, matrix, depth, normals, camera, transform=T, max_distance=max_distance, **kw)
        error = pose_error(tracking.compose(tracking.invert(T), predicted), truth) if truth is not None else (NAN, NAN)
        history.append((int(o.mask.sum()), int((o.undecided & o.mask).sum())) + error)
        s = pds.icp_solve(oracle_system(o.rows)[None], min_count, min_eigenvalue)
        status = int(s.status[0])
        if status != tracking.TRACKED:
            return predicted.copy(), history, status
        T = tracking.compose(pds.se3_exp(s.xi[0]), T)
        if np.linalg.norm(s.xi[0]) < tolerance:
            break
    return tracking.compose(tracking.invert(T), predicted), history, status


@functools.lru_cache(maxsize=None)
def corner_tracked():
    depth, normals = corner_model()
    return oracle_track(corner_disparity(POSE1), corner_matrix(), depth, normals, camera_of(corner_matrix()), POSE0,
                        max_distance=2 * CORNER['truncation'], truth=POSE1, **TRACK)


def test_the_corner_scene_meets_its_conditions_on_the_oracle():
    pose, history, status = corner_tracked()
    pixels = CORNER['height'] * CORNER['width']
    start, end = pose_error(POSE0, POSE1), pose_error(pose, POSE1)
    for k, (rows, undecided, angle, distance) in enumerate(history):
        print('iteration %d: %d rows (%.1f %% of the pixels), %d undecided, error %.3e rad %.3e m' %
              (k, rows, 100.0 * rows / pixels, undecided, angle, distance))
        assert undecided < 0.02 * rows and rows >= 0.20 * pixels, k
    print('start %.3e rad %.3e m -> end %.3e rad %.3e m' % (start + end))
    assert status == tracking.TRACKED
    assert abs(start[0] - 0.0206) < 1e-3 and 0.03 < start[1] < 0.06   # one to two voxels
    assert end[0] <= start[0] / 10 and end[1] <= start[1] / 10


def gpu_scenes():
    """name -> the keyword arguments of oracle_rows for every scene tests/test_gpu_icp.py holds against the oracle."""
    scenes = {}
    for height, width in ((1, 1), (21, 37), (25, 41), (48, 64)):
        d, Q, depth, normals, camera = wall_case(height, width, slope=0.0005)
        # (a single pixel keeps its row only under a transform that leaves it inside the model's one pixel)
        tilted = np.hstack([pds.rectification.rodrigues(np.array([0.01, -0.02, 0.015])),
                            [[0.011], [-0.007], [0.004]]]) if height > 1 else np.hstack([np.eye(3), [[0.003], [0.002], [0.01]]])
        scenes['wall %dx%d' % (width, height)] = dict(disparity=d, matrix=Q, depth=depth, normals=normals, camera=camera,
                                                      transform=tilted, max_distance=0.1)
    depth, normals = corner_model()
    scenes['corner'] = dict(disparity=corner_disparity(POSE1), matrix=corner_matrix(), depth=depth, normals=normals,
                            camera=camera_of(corner_matrix()), transform=IDENTITY,
                            max_distance=2 * CORNER['truncation'])
    near = tracking.compose(POSE0, tracking.invert(POSE1))   # the true transform: frame 1 -> the model's camera
    scenes['corner aligned'] = dict(scenes['corner'], transform=near)
    frame_normals = corner_frame_normals()
    scenes['corner with normals'] = dict(scenes['corner aligned'], frame_normals=frame_normals, min_cosine=0.9)
    return scenes


def corner_frame_normals():
    """The normals of frame 1 by hand: the plane each pixel's ray meets first, facing the camera, in the frame's frame."""
    d = corner_disparity(POSE1).astype(np.float64)
    Q = corner_matrix()
    fx, fy, cx, cy, _ = camera_of(Q)
    yy, xx = np.mgrid[0:CORNER['height'], 0:CORNER['width']].astype(np.float64)
    Z = Q[2, 3] / (d * Q[3, 2])
    points = np.stack([(xx - cx) / fx * Z, (yy - cy) / fy * Z, Z], axis=-1)
    world = (points - POSE1[:, 3]) @ POSE1[:, :3]
    out = np.full(points.shape, NAN)
    gap = np.full(Z.shape, INF)
    for normal, offset in CORNER['planes']:
        normal = np.array(normal)
        distance = np.abs(world @ normal - offset) / np.linalg.norm(normal)
        turned = POSE1[:, :3] @ (normal / np.linalg.norm(normal))
        facing = np.where(((points @ turned) > 0)[..., None], -turned, turned)
        out = np.where((distance < gap)[..., None], facing, out)
        gap = np.minimum(gap, distance)
    out[5, 7] = NAN
    return out.astype(np.float32)


def test_the_restatement_stays_within_its_measured_error():
    worst = 0.0
    for name, kw in gpu_scenes().items():
        o = oracle_rows(**kw)
        error = restatement_error(o)
        decided = ~o.undecided
        # the restatement's own decisions agree with the oracle's wherever the oracle decides
        assert ((~np.isnan(o.rows32[..., 6])) == o.mask)[decided].all(), name
        rows = int(o.mask.sum())
        print('%s: %d rows, %d undecided, float32 restatement vs fp64: %.3e of the scale' %
              (name, rows, int((o.undecided & o.mask).sum()), error))
        assert (o.undecided & o.mask).sum() <= 0.02 * max(rows, 1) or name.startswith('wall 1x1'), name
        worst = max(worst, error)
    print('REL32: measured %.3e, held %.3e' % (worst, REL32))
    assert 0.25 * REL32 <= worst <= REL32
    # the corner scenes give rows on at least 20 % of the pixels, and the normals take some away but not most
    scenes = gpu_scenes()
    plain, with_normals = oracle_rows(**scenes['corner aligned']), oracle_rows(**scenes['corner with normals'])
    assert plain.mask.mean() >= 0.2 and 0.5 * plain.mask.sum() <= with_normals.mask.sum() < plain.mask.sum()
    # check_rows takes the oracle's own answer, rounded, and refuses a moved component, a missing and a spare row
    got = plain.rows.astype(np.float32)
    count, share = check_rows(got, plain)
    assert count == int((plain.mask & ~plain.undecided).sum()) and share <= 0.25
    py, px = np.argwhere(plain.mask & ~plain.undecided)[0]
    for edit in ('moved', 'missing', 'spare'):
        bad = got.copy()
        if edit == 'moved':
            bad[py, px, 6] += 1e-4
        elif edit == 'missing':
            bad[py, px] = NAN
        else:
            qy, qx = np.argwhere(~plain.mask & ~plain.undecided)[0]
            bad[qy, qx] = 1.0
        with pytest.raises(AssertionError):
            check_rows(bad, plain)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_icp_symbols_declared_exported_and_bound(hip_library):
    header = open(_lib.HEADER_PATH).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('pds_icp_workspace_bytes', 'pds_icp_system_fwd'):
        assert name + '(' in header and hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert hip_library.pds_abi_version() == 7 and '#define PDS_ABI_VERSION 7' in header
    for name in ('icp_system', 'icp_solve', 'se3_exp', 'IcpSystem', 'IcpSolution', 'Tracking'):
        assert name in pds.__all__ and getattr(pds, name) is getattr(tracking, name), name
    assert pds.IcpSystem._fields == ('system', 'rows')
    assert pds.IcpSolution._fields == ('xi', 'rmse', 'count', 'status')
    assert pds.Tracking._fields == ('pose', 'rmse', 'inliers', 'iterations', 'status')
    assert (tracking.TRACKED, tracking.TOO_FEW_ROWS, tracking.DEGENERATE) == (0, 1, 2) and tracking.SYSTEM == SYSTEM
    csrc = _lib.HEADER_PATH.replace('include/pds_hip.h', 'practicaldeepstereo_nips2018_amd/csrc/')
    common = open(csrc + 'common.hpp').read()
    assert 'constexpr int kIcpTile = %d;' % TILE in common and 'constexpr int kIcpSystem = %d;' % SYSTEM in common
    assert 'icp.hip' in [name.rsplit('/', 1)[-1] for name in _lib.sources()]
    # one partial of 29 doubles per tile of 1024 pixels and entry, rounded up to 256
    sizes = hip_library.pds_icp_workspace_bytes
    assert sizes(1, 1, 1) == 256 and sizes(1, 32, 32) == 256 and sizes(1, 25, 41) == 512 and sizes(3, 48, 64) == 2304
    assert sizes(1, 540, 960) == (507 * 232 + 255) // 256 * 256 and sizes(19, 1, 1) == (19 * 232 + 255) // 256 * 256


def test_icp_validation_needs_no_gpu(hip_library):
    lib = hip_library
    big = 1 << 24
    d, v, c, n, md, mn, sy, rw, ws = [ctypes.c_void_p(big * k) for k in range(1, 10)]   # never dereferenced
    floats = (lambda values: (ctypes.c_float * len(values))(*values))
    identity = floats(np.eye(4, dtype=np.float32).reshape(-1).tolist())
    transforms = floats([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0])
    camera = floats([4.0, 4.0, 1.0, 0.5, 0.0])
    error = lib.pds_last_error

    def call(disparity=d, valid=v, confidence=c, min_confidence=0.0, matrix=identity, normals=n, model_depth=md,
             model_normals=mn, model=(1, 2, 3), camera=camera, transforms=transforms, max_distance=0.1, min_cosine=0.0,
             system=sy, rows=rw, shape=(1, 2, 3), workspace=ws, workspace_bytes=256):
        return lib.pds_icp_system_fwd(disparity, valid, confidence, min_confidence, matrix, normals, model_depth,
                                      model_normals, *model, camera, transforms, max_distance, min_cosine, system, rows,
                                      *shape, workspace, workspace_bytes, None)

    for name in ('disparity', 'matrix', 'model_depth', 'model_normals', 'camera', 'transforms', 'system', 'workspace'):
        assert call(**{name: None}) != 0 and error() == b'icp: null pointer', name
    for shape in [(0, 2, 3), (1, 0, 3), (1, 2, 0), (-1, 2, 3), (1, -2, 3)]:
        assert call(shape=shape) != 0 and b'icp: bad shape' in error(), shape
        assert lib.pds_icp_workspace_bytes(*shape) == 0 and b'icp: bad shape' in error(), shape
    assert call(shape=(1 << 12, 1 << 10, 1 << 10), workspace_bytes=1 << 40) != 0 and b'32-bit indices' in error()
    assert lib.pds_icp_workspace_bytes(1 << 12, 1 << 10, 1 << 10) == 0 and b'32-bit indices' in error()
    assert call(model=(2, 2, 3)) != 0 and b'model_batch must be 1 or batch = 1 (got 2)' in error()
    for model in [(1, 0, 3), (1, 2, -3), (1, 1 << 24, 1)]:
        assert call(model=model) != 0 and b'icp: bad model shape' in error(), model
    assert call(model=(1, 1 << 16, 1 << 16)) != 0 and b'model_batch * hm * wm' in error()
    assert call(workspace_bytes=255) != 0 and b'workspace too small (255 < 256)' in error()
    assert call(min_confidence=NAN) != 0 and b'min_confidence is NaN' in error()
    for bad in (0.0, -0.1, NAN, INF):
        assert call(max_distance=bad) != 0 and b'max_distance must be positive and finite' in error(), bad
    assert call(min_cosine=NAN) != 0 and b'min_cosine is NaN' in error()
    for name, pointer in (('disparity', d), ('normals', n), ('model_depth', md), ('system', sy), ('rows', rw)):
        assert call(**{name: ctypes.c_void_p(pointer.value + 2)}) != 0 and b'not 4-byte aligned' in error(), name
    assert call(workspace=ctypes.c_void_p(ws.value + 4)) != 0 and b'workspace is not 8-byte aligned' in error()
    # nothing written may overlap anything read or written (2 x 3 pixels: 24 / 6 / 72 bytes; system 232, rows 168)
    assert call(system=d) != 0 and b'an output aliases an input' in error()
    assert call(rows=ctypes.c_void_p(mn.value + 68)) != 0 and b'an output aliases an input' in error()
    assert call(workspace=ctypes.c_void_p(md.value + 16)) != 0 and b'an output aliases an input' in error()
    assert call(rows=ctypes.c_void_p(sy.value + 228)) != 0 and b'an output aliases another output' in error()
    assert call(workspace=ctypes.c_void_p(rw.value + 160)) != 0 and b'an output aliases another output' in error()
    for k, name, base in ((0, 'matrix', np.eye(4).reshape(-1).tolist()), (11, 'transform', list(transforms)),
                          (4, 'camera', list(camera))):
        for bad in (NAN, INF):
            values = list(base)
            values[k] = bad
            key = 'transforms' if name == 'transform' else name
            assert call(**{key: floats(values)}) != 0 and b'non-finite ' + name.encode() in error(), (name, bad)
    for focal in (0, 1):
        values = list(camera)
        values[focal] = 0.0
        assert call(camera=floats(values)) != 0 and b'focal lengths must be positive' in error()


# ------------------------------------------------------------------------------------------------ Python
def test_icp_python_errors_and_signatures():
    ok, Q = torch.zeros(2, 4, 5), q_of(4, 5, 4.0, 0.5)
    model = pds.Raycast(torch.zeros(2, 4, 5), torch.zeros(2, 4, 5, 3))
    camera = camera_of(Q)

    def run(disparity=ok, matrix=Q, model=model, camera=camera, **kw):
        return pds.icp_system(disparity, matrix, model, camera, **kw)

    with pytest.raises(TypeError, match='disparity must be a torch.Tensor'):
        run(np.zeros((2, 4, 5), dtype=np.float32))
    with pytest.raises(TypeError, match='disparity must be float32'):
        run(ok.double())
    with pytest.raises(ValueError, match='disparity must have 3 dimensions'):
        run(torch.zeros(4, 5))
    with pytest.raises(ValueError, match='empty input'):
        run(torch.zeros(0, 4, 5))
    with pytest.raises(ValueError, match='matrix must be a finite 4x4'):
        run(matrix=np.eye(3))
    with pytest.raises(TypeError, match='model must be a Raycast'):
        run(model=None)
    with pytest.raises(ValueError, match='model has no normals'):
        run(model=pds.Raycast(torch.zeros(2, 4, 5), None))
    with pytest.raises(ValueError, match=r'model.depth must be \[2, Hm, Wm\] or \[1, Hm, Wm\]'):
        run(model=pds.Raycast(torch.zeros(3, 4, 5), torch.zeros(3, 4, 5, 3)))
    with pytest.raises(ValueError, match='model.normals must be'):
        run(model=pds.Raycast(torch.zeros(1, 4, 5), torch.zeros(1, 4, 5, 2)))
    with pytest.raises(TypeError, match='model.depth must be float32'):
        run(model=pds.Raycast(torch.zeros(1, 4, 5).double(), torch.zeros(1, 4, 5, 3)))
    with pytest.raises(ValueError, match='camera must hold 5 values'):
        run(camera=(1.0, 1.0, 0.0))
    with pytest.raises(ValueError, match='positive focal lengths'):
        run(camera=(0.0, 1.0, 0.0, 0.0, 0.0))
    for bad in (np.eye(3), np.zeros((3, 3, 4)), np.full((3, 4), NAN)):
        with pytest.raises(ValueError, match=r'transform must be a finite 3x4 \[R \| t\] or \[2, 3, 4\]'):
            run(transform=bad)
    with pytest.raises(ValueError, match='normals must be'):
        run(normals=torch.zeros(2, 4, 5, 2))
    with pytest.raises(ValueError, match='valid must be torch.bool'):
        run(valid=torch.zeros(2, 4, 5))
    with pytest.raises(ValueError, match='differ in shape'):
        run(confidence=torch.zeros(2, 4, 4))
    with pytest.raises(ValueError, match='min_confidence is NaN'):
        run(min_confidence=NAN)
    for bad in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError, match='max_distance must be positive and finite'):
            run(max_distance=bad)
    with pytest.raises(TypeError, match='max_distance must be a number'):
        run(max_distance='far')
    with pytest.raises(ValueError, match='min_cosine is NaN'):
        run(min_cosine=NAN)
    # all of that comes before the device: what is left is that there is no CPU fallback
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        run()
    parameters = inspect.signature(pds.icp_system).parameters
    assert list(parameters)[:4] == ['disparity', 'matrix', 'model', 'camera']
    assert [(k, p.default) for k, p in parameters.items()][4:] == [
        ('transform', None), ('normals', None), ('valid', None), ('confidence', None), ('min_confidence', 0.0),
        ('max_distance', 0.1), ('min_cosine', 0.0), ('with_rows', False)]
    assert list(inspect.signature(pds.icp_solve).parameters) == ['system', 'min_count', 'min_eigenvalue']
    parameters = inspect.signature(pds.TsdfVolume.track).parameters
    assert list(parameters)[1:4] == ['disparity', 'matrix', 'pose']
    assert [(k, p.default) for k, p in parameters.items()][4:] == [
        ('camera', None), ('size', None), ('iterations', 10), ('max_distance', None), ('min_cosine', 0.5),
        ('normals', None), ('valid', None), ('confidence', None), ('min_confidence', 0.0), ('min_weight', 1.0),
        ('min_count', 100), ('min_eigenvalue', 1e-4), ('tolerance', 1e-6)]
    parameters = inspect.signature(pds.StereoRig.track).parameters
    assert [(k, p.default) for k, p in list(parameters.items())[1:5]] == [
        ('volume', inspect.Parameter.empty), ('disparity', inspect.Parameter.empty), ('pose', inspect.Parameter.empty),
        ('valid', None)]
    assert list(parameters.values())[5].kind is inspect.Parameter.VAR_KEYWORD
    # track: what it can judge comes before the raycast asks where the volume lives
    volume = HostVolume((0.0, 0.0, 0.0), 0.1, (4, 3, 2), 0.3)
    frame = torch.zeros(1, 4, 5)
    with pytest.raises(ValueError, match='track needs the predicted pose'):
        volume.track(frame, Q, None)
    with pytest.raises(ValueError, match=r'pose must be a finite 3x4'):
        volume.track(frame, Q, np.eye(4))
    with pytest.raises(ValueError, match='iterations must be at least 1'):
        volume.track(frame, Q, IDENTITY, iterations=0)
    with pytest.raises(ValueError, match='canonical rectified form'):
        volume.track(frame, np.eye(4) * 2.0, IDENTITY)
    with pytest.raises(ValueError, match='tolerance must be >= 0'):
        volume.track(frame, Q, IDENTITY, tolerance=-1.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        volume.track(frame, Q, IDENTITY)
    with pytest.raises(TypeError, match='volume must be a TsdfVolume'):
        simple_rig(64, 48).track(None, frame, IDENTITY)
    for phrase in ('image pyramids', 'robust kernels or reweighting', 'colour terms', 'frame-to-frame tracking',
                   'loop closure', 'no CPU fallback'):
        assert phrase in tracking.__doc__, phrase
    for module in (pds.tsdf, pds.tsdf_raycast):
        assert 'tracking.py' in module.__doc__
        assert 'pose estimation' not in module.__doc__.split('Out of scope')[1]
