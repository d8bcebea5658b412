"""CPU: colour tracking (pds_intensity_pyramid_fwd, pds_icp_color_workspace_bytes, pds_icp_color_system_fwd;
intensity_pyramid, icp_color_system, ColorTsdfVolume.track_color, StereoRig.track_color).  The entry points are declared,
exported and bound and validate without a GPU; the Python surface refuses what it cannot run.

oracle_intensity_pyramid is float32 numpy, operation by operation what the kernel does: the luma's fused multiply-adds
are formed in fp64 and rounded once (a product of two float32 is exact in fp64, and the sum of it and a float32 rounds to
float32 as the fused operation does -- double rounding needs a 53-bit tie, which a 48-bit product plus a 24-bit addend
cannot reach here), the halvings are float32 additions and an exact multiplication by 0.25.  It is bit-exact by construction.

oracle_color_rows is the numpy fp64 oracle of tests/test_gpu_icp_color.py, built on oracle_rows of tests/test_icp_host.py
(the geometric half and its undecided set) and on the same steps 1 - 3 for q, u, v and their errors E_q, E_u, E_v, whose
derivation stands at the top of that file.  The photometric half follows its rule: the formulas restated in float32 numpy
are compared with the fp64 oracle, component by component, relative to the component's SCALE (the sum of the absolute
values of the terms it is made of), and the kernel is held to 4 * REL32C * scale.  Position error moves the sample, which
no rounding bound of the formulas covers, so each component also gets its first-order term: with D = (L11 - L01) -
(L10 - L00), the mixed difference of the cell,

    r_c       |I_u| E_u + |I_v| E_v
    I_u, I_v  |D| E_v, |D| E_u                       (e_Iu, e_Iv)
    g_x       fx iz e_Iu + |g_x| E_qz / q_z          (e_gx; iz = 1 / q_z)
    g_y       iz (|skew| e_Iu + fy e_Iv) + |g_y| E_qz / q_z
    g_z       |x| e_gx + |y| e_gy + |g_x| E_x + |g_y| E_y
    J_c0      |q_y| e_gz + |g_z| E_qy + |q_z| e_gy + |g_y| E_qz, and cyclic

A pixel is UNDECIDED, beside the geometric undecided set, where u or v lies within E_u / E_v of an integer (the cell, and
with it I_u and I_v, may flip) or where a tap's depth gate |Z - q_z| <= max_distance lies within E_qz + EPS (|Z| + |q_z| +
max_distance) of its limit.  REL32C is the largest error of the restatement relative to the scale over the scenes of the GPU
file (measured here, never against the kernel: test_the_colour_restatement_stays_within_its_measured_error prints it).  The
restatement's own sample position differs from the oracle's, so the measured figure holds some of the position effect
already; the first-order term is added all the same, since the kernel's fused multiply-adds place its sample elsewhere
again.

The textured wall: the WALL volume of tests/test_tsdf_host.py, 14 x 12 x 3 voxels of 1/8 m, with a colour set analytically
from the voxel position (two non-parallel sinusoids), seen by the 64 x 48 camera.  The frame is rendered by oracle_raycast
and oracle_render at a truth pose shifted in the wall's plane from the predicted one, and oracle_track_color, the fp64
loop of track_color, runs on it; what the GPU test relies on is asserted here on the oracle alone."""
import collections
import ctypes
import functools
import inspect
import re

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib, pyramid, tracking
from tests.test_icp_host import (CORNER, IDENTITY, POSE0, POSE1, TRACK, camera_of, corner_disparity, corner_matrix,
                                 corner_state, oracle_rows, oracle_system, pose_error, wall_case)
from tests.test_register_depth_host import EPS, simple_rig
from tests.test_tsdf_color_host import oracle_render
from tests.test_tsdf_host import WALL as TSDF_WALL, HostVolume, f32, q_of, wall_layers, wall_volume
from tests.test_tsdf_raycast_host import oracle_raycast

NAN, INF = float('nan'), float('inf')
F = np.float32
# measured by test_the_colour_restatement_stays_within_its_measured_error: the largest error of the float32 restatement
# of the photometric row beyond its first-order position term, relative to the component's scale; the GPU is held to 4 x
REL32C = 2.5e-7   # (measured 2.396e-07, on the corner scene)

# rows [H, W, 7] fp64 (NaN where none); mask, undecided [H, W]; bound, scale [H, W, 7]; rows32: the float32 restatement;
# geometric: the Rows of oracle_rows
ColorRows = collections.namedtuple('ColorRows', ['rows', 'mask', 'undecided', 'bound', 'scale', 'rows32', 'first_order',
                                                 'geometric'])


# ------------------------------------------------------------------------------------------------ the intensity oracle
def fmaf32(a, b, c):
    """fmaf on float32 arrays: the exact product and sum in fp64, rounded once."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)


def oracle_intensity_pyramid(image, levels=1, layout='nchw'):
    """image: uint8 [B, H, W, 3], float32 [B, 3, H, W] ('nchw') or float32 [B, H, W, 3] ('nhwc') -> a list of float32."""
    image = np.asarray(image)
    if image.dtype == np.uint8 or layout == 'nhwc':
        c = [image[..., k].astype(F) for k in range(3)]
    else:
        c = [image[:, k].astype(F) for k in range(3)]
    with np.errstate(all='ignore'):
        level = fmaf32(F(0.299), c[0], fmaf32(F(0.587), c[1], F(0.114) * c[2]))
        out = [level]
        for _ in range(levels - 1):
            h, w = level.shape[1] // 2, level.shape[2] // 2
            a = level[:, :2 * h, :2 * w]
            level = ((a[:, 0::2, 0::2] + a[:, 0::2, 1::2]) + (a[:, 1::2, 0::2] + a[:, 1::2, 1::2])) * F(0.25)
            out.append(level)
    return out


def test_luma_and_one_halving_by_hand():
    image = np.zeros((1, 3, 2, 2), dtype=F)
    image[0, :, 0, 0] = (1.0, 2.0, 4.0)
    image[0, :, 0, 1] = (8.0, 0.0, 0.0)
    image[0, :, 1, 0] = (0.0, 16.0, 0.0)
    image[0, :, 1, 1] = (0.0, 0.0, 32.0)
    l0, l1 = oracle_intensity_pyramid(image, 2)
    hand = np.array([[0.299 + 2 * 0.587 + 4 * 0.114, 8 * 0.299], [16 * 0.587, 32 * 0.114]])
    assert l0.dtype == F and l0.shape == (1, 2, 2) and np.abs(l0[0] - hand).max() <= 4e-7 * 16
    assert l1.shape == (1, 1, 1) and l1[0, 0, 0] == ((l0[0, 0, 0] + l0[0, 0, 1]) + (l0[0, 1, 0] + l0[0, 1, 1])) * F(0.25)
    # the three layouts of the same picture agree bit for bit (uint8 converts exactly)
    rng = np.random.RandomState(0)
    bytes_ = rng.randint(0, 256, size=(2, 3, 5, 3)).astype(np.uint8)
    as_uint8 = oracle_intensity_pyramid(bytes_, 2)
    as_nhwc = oracle_intensity_pyramid(bytes_.astype(F), 2, layout='nhwc')
    as_nchw = oracle_intensity_pyramid(bytes_.astype(F).transpose(0, 3, 1, 2), 2)
    for x, y, z in zip(as_uint8, as_nhwc, as_nchw):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    # 3 x 5 floors to 1 x 2: the last row and the last column are dropped; a NaN channel spreads to its parent only
    assert as_uint8[0].shape == (2, 3, 5) and as_uint8[1].shape == (2, 1, 2)
    holed = bytes_.astype(F)
    holed[0, 1, 2, 1] = NAN    # pixel (1, 2): parent (0, 1)
    holed[1, 2, 4, 0] = NAN    # the dropped row and column: no parent
    l0, l1 = oracle_intensity_pyramid(holed, 2, layout='nhwc')
    assert np.isnan(l0[0, 1, 2]) and np.isnan(l0[1, 2, 4]) and int(np.isnan(l0).sum()) == 2
    assert np.isnan(l1[0, 0, 1]) and int(np.isnan(l1).sum()) == 1
    assert (l1[1] == as_uint8[1][1]).all()
    # a constant image keeps its value on every level, up to the rounding of the three weights
    flat = oracle_intensity_pyramid(np.full((1, 8, 8, 3), 200, dtype=np.uint8), 4)
    assert [t.shape for t in flat] == [(1, 8, 8), (1, 4, 4), (1, 2, 2), (1, 1, 1)]
    assert all((t == flat[0][0, 0, 0]).all() for t in flat) and abs(float(flat[0][0, 0, 0]) - 200.0) <= 200 * 2e-7


# ------------------------------------------------------------------------------------------------ the rows oracle
def _projection(ft, d, M, T, camera, margins):
    """Steps 1 - 3 of tests/test_icp_host.py in the float type ft -> q [3], x, y, u, v (and, with margins, E_q, E_x, E_y,
    E_u, E_v as derived there)."""
    height, width = d.shape
    c = (lambda a: np.asarray(a, dtype=ft))
    yy, xx = np.mgrid[0:height, 0:width]
    xx, yy, dd = c(xx), c(yy), c(d)
    M, T = c(M), c(T)
    fx, fy, cx, cy, skew = (ft(v) for v in camera)
    with np.errstate(all='ignore'):
        X, Y, Z, W = (M[r, 0] * xx + M[r, 1] * yy + M[r, 2] * dd + M[r, 3] for r in range(4))
        P = [X / W, Y / W, Z / W]
        q = [T[a, 0] * P[0] + T[a, 1] * P[1] + T[a, 2] * P[2] + T[a, 3] for a in range(3)]
        x, y = q[0] / q[2], q[1] / q[2]
        u, v = fx * x + skew * y + cx, fy * y + cy
        if not margins:
            return q, x, y, u, v
        eps = EPS
        cc = [np.abs(xx), np.abs(yy), np.abs(dd), np.ones_like(dd)]
        mass = [sum(abs(M[r, k]) * cc[k] for k in range(4)) for r in range(4)]
        E_P = [eps * (mass[a] / np.abs(W) + np.abs(P[a]) * (1 + mass[3] / np.abs(W))) for a in range(3)]
        E_q = [sum(abs(T[a, k]) * E_P[k] for k in range(3)) +
               eps * (sum(np.abs(T[a, k] * P[k]) for k in range(3)) + abs(T[a, 3])) for a in range(3)]
        E_x = (E_q[0] + np.abs(x) * E_q[2]) / q[2] + eps * np.abs(x)
        E_y = (E_q[1] + np.abs(y) * E_q[2]) / q[2] + eps * np.abs(y)
        E_u = fx * E_x + abs(skew) * E_y + eps * (np.abs(fx * x) + np.abs(skew * y) + abs(cx) + np.abs(u) + 0.5)
        E_v = fy * E_y + eps * (np.abs(fy * y) + abs(cy) + np.abs(v) + 0.5)
        Q_ = [sum(np.abs(T[a, k] * P[k]) for k in range(3)) + abs(T[a, 3]) for a in range(3)]
    return q, x, y, u, v, E_q, E_x, E_y, E_u, E_v, Q_


def _photometric(ft, has, q, x, y, u, v, intensity, depth, model_intensity, camera, max_distance):
    """Steps 1 - 5 of the photometric row in ft, where `has` (the geometric row exists) -> (rows [H, W, 7], mask, parts)."""
    hm, wm = depth.shape
    c = (lambda a: np.asarray(a, dtype=ft))
    fx, fy, cx, cy, skew = (ft(s) for s in camera)
    with np.errstate(all='ignore'):
        If = c(intensity)
        fx0, fy0 = np.floor(u), np.floor(v)
        inside = has & ~np.isnan(If) & (fx0 >= 0) & (fx0 + 1 <= wm - 1) & (fy0 >= 0) & (fy0 + 1 <= hm - 1)
        x0 = np.where(inside, fx0, 0).astype(np.int64)
        y0 = np.where(inside, fy0, 0).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, wm - 1), np.minimum(y0 + 1, hm - 1)
        a, b = u - fx0, v - fy0
        L, Zm = c(model_intensity), c(depth)
        L00, L10, L01, L11 = L[y0, x0], L[y0, x1], L[y1, x0], L[y1, x1]
        taps = [Zm[y0, x0], Zm[y0, x1], Zm[y1, x0], Zm[y1, x1]]
        limit = ft(F(max_distance))
        gates = [np.abs(t - q[2]) for t in taps]
        seen = inside & ~np.isnan(L00) & ~np.isnan(L10) & ~np.isnan(L01) & ~np.isnan(L11)
        seen &= ~np.isnan(taps[0]) & ~np.isnan(taps[1]) & ~np.isnan(taps[2]) & ~np.isnan(taps[3])
        mask = seen & (gates[0] <= limit) & (gates[1] <= limit) & (gates[2] <= limit) & (gates[3] <= limit)
        dx0, dx1 = L10 - L00, L11 - L01
        top, bot = a * dx0 + L00, a * dx1 + L01
        Iv = bot - top
        Im = b * Iv + top
        Iu = b * (dx1 - dx0) + dx0
        iz = ft(1.0) / q[2]
        gx = (Iu * fx) * iz
        gy = (Iu * skew + Iv * fy) * iz
        gz = -(gx * x + gy * y)
        J = [q[1] * gz - q[2] * gy, q[2] * gx - q[0] * gz, q[0] * gy - q[1] * gx]
        rows = np.stack(J + [gx, gy, gz, If - Im], axis=-1).astype(np.float64)
        rows = np.where(mask[..., None], rows, NAN)
    parts = dict(inside=inside, seen=seen, gates=gates, taps=taps, limit=limit, L=(L00, L10, L01, L11), a=a, b=b, Iu=Iu,
                 Iv=Iv, If=If, iz=iz, g=(gx, gy, gz), D=dx1 - dx0)
    return rows, mask, parts


def oracle_color_rows(disparity, intensity, matrix, depth, normals, model_intensity, camera, transform=None,
                      frame_normals=None, valid=None, confidence=None, min_confidence=0.0, max_distance=0.1, min_cosine=0.0):
    """One entry -> ColorRows: the photometric rows of the pixels whose geometric row oracle_rows gives."""
    geometric = oracle_rows(disparity, matrix, depth, normals, camera, transform=transform, frame_normals=frame_normals,
                            valid=valid, confidence=confidence, min_confidence=min_confidence, max_distance=max_distance,
                            min_cosine=min_cosine)
    d = np.asarray(disparity, dtype=F)
    depth, L = np.asarray(depth, dtype=F), np.asarray(model_intensity, dtype=F)
    intensity = np.asarray(intensity, dtype=F)
    assert L.shape == depth.shape and intensity.shape == d.shape
    M, T, cam = f32(matrix), f32(IDENTITY if transform is None else transform), f32(camera)
    q, x, y, u, v, E_q, E_x, E_y, E_u, E_v, Q_ = _projection(np.float64, d, M, T, cam, True)
    rows, mask, p = _photometric(np.float64, geometric.mask, q, x, y, u, v, intensity, depth, L, cam, max_distance)
    q32, x32, y32, u32, v32 = _projection(F, d, M.astype(F), T.astype(F), cam.astype(F), False)
    has32 = ~np.isnan(geometric.rows32[..., 6])
    rows32 = _photometric(F, has32, q32, x32, y32, u32, v32, intensity, depth, L, cam.astype(F), max_distance)[0]
    fx, fy, cx, cy, skew = cam
    with np.errstate(all='ignore'):
        undecided = geometric.undecided.copy()
        near_u, near_v = np.abs(u - np.round(u)) <= E_u, np.abs(v - np.round(v)) <= E_v
        undecided |= geometric.mask & ~np.isnan(p['If']) & (near_u | near_v)
        for gate, tap in zip(p['gates'], p['taps']):
            slack = E_q[2] + EPS * (np.abs(tap) + np.abs(q[2]) + p['limit'])
            undecided |= p['seen'] & (np.abs(gate - p['limit']) <= slack)
        # ---- the scales: the sums of the absolute values of the terms of each component
        L00, L10, L01, L11 = (np.abs(t) for t in p['L'])
        s_r = np.abs(p['If']) + L00 + L10 + L01 + L11
        s_Iu, s_Iv = L00 + L10 + L01 + L11, L00 + L10 + L01 + L11
        iz = np.abs(p['iz'])
        s_gx = s_Iu * fx * iz
        s_gy = (s_Iu * abs(skew) + s_Iv * fy) * iz
        s_gz = s_gx * np.abs(x) + s_gy * np.abs(y)
        s_g = (s_gx, s_gy, s_gz)
        scale = np.stack([Q_[1] * s_g[2] + Q_[2] * s_g[1], Q_[2] * s_g[0] + Q_[0] * s_g[2], Q_[0] * s_g[1] + Q_[1] * s_g[0],
                          s_gx, s_gy, s_gz, s_r], axis=-1)
        # ---- the first-order terms of the position error
        gx, gy, gz = (np.abs(t) for t in p['g'])
        D = np.abs(p['D'])
        e_Iu, e_Iv = D * E_v, D * E_u
        e_gx = fx * iz * e_Iu + gx * E_q[2] / q[2]
        e_gy = iz * (abs(skew) * e_Iu + fy * e_Iv) + gy * E_q[2] / q[2]
        e_gz = np.abs(x) * e_gx + np.abs(y) * e_gy + gx * E_x + gy * E_y
        e_g, g = (e_gx, e_gy, e_gz), (gx, gy, gz)
        aq = [np.abs(t) for t in q]
        first = np.stack([aq[1] * e_g[2] + g[2] * E_q[1] + aq[2] * e_g[1] + g[1] * E_q[2],
                          aq[2] * e_g[0] + g[0] * E_q[2] + aq[0] * e_g[2] + g[2] * E_q[0],
                          aq[0] * e_g[1] + g[1] * E_q[0] + aq[1] * e_g[0] + g[0] * E_q[1],
                          e_gx, e_gy, e_gz, np.abs(p['Iu']) * E_u + np.abs(p['Iv']) * E_v], axis=-1)
    scale = np.where(mask[..., None], scale, 0.0)
    first = np.where(mask[..., None], first, 0.0)
    return ColorRows(rows, mask, undecided, 4.0 * REL32C * scale + first, scale, rows32, first, geometric)


def colour_restatement_error(o):
    """The largest |rows32 - rows| / scale over the decided rows both have (0 without any)."""
    both = o.mask & ~o.undecided & ~np.isnan(o.rows32[..., 6])
    with np.errstate(all='ignore'):
        ratio = np.abs(o.rows32 - o.rows) / o.scale
    ratio = np.where(both[..., None] & (o.scale > 0), ratio, 0.0)
    return float(ratio.max(initial=0.0))


# ------------------------------------------------------------------------------------------------ the ramp wall, by hand
def ramp(height, width, alpha, beta, offset=10.0):
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    return (offset + alpha * xx + beta * yy).astype(F)


def test_oracle_ramp_wall_by_hand():
    d, Q, depth, normals, camera = wall_case()
    depth = np.full_like(depth, 2.0)   # the model wall where the frame's is: the taps pass any gate
    alpha, beta = 0.5, -0.25
    L = ramp(21, 37, alpha, beta)
    frame = np.full((21, 37), 12.0, dtype=F)
    shifted = IDENTITY.copy()
    shifted[0, 3], shifted[1, 3] = 0.25 * 2.0 / 64.0, 0.25 * 2.0 / 64.0    # u = x + 0.25, v = y + 0.25
    o = oracle_color_rows(d, frame, Q, depth, normals, L, camera, transform=shifted, max_distance=0.1)
    inner = np.zeros((21, 37), dtype=bool)
    inner[:-1, :-1] = True    # the last row and column have no cell to the right / below
    decided = ~o.undecided
    assert (o.mask == inner)[decided].all() and decided[:, :-1].mean() > 0.9 and o.geometric.mask.all()
    yy, xx = np.mgrid[0:21, 0:37].astype(np.float64)
    X, Y, Z = (xx - 18.0 + 0.25) / 32.0, (yy - 10.0 + 0.25) / 32.0, 2.0
    I_m = 10.0 + alpha * (xx + 0.25) + beta * (yy + 0.25)
    gx, gy = alpha * 64.0 / Z, beta * 64.0 / Z
    gz = -(gx * X / Z + gy * Y / Z)
    hand = np.stack([Y * gz - Z * gy, Z * gx - X * gz, X * gy - Y * gx, np.full_like(X, gx), np.full_like(X, gy), gz,
                     12.0 - I_m], axis=-1)
    assert np.abs(o.rows - hand)[o.mask & decided].max() <= 1e-9
    assert colour_restatement_error(o) <= REL32C
    # half a pixel of u moves the cell (x0 changes) but not I_m: the ramp is linear
    for shift, cell in ((0.25, 0), (0.75, 0), (1.25, 1)):
        shifted[0, 3] = shift * 2.0 / 64.0
        moved = oracle_color_rows(d, frame, Q, depth, normals, L, camera, transform=shifted, max_distance=0.1)
        want = 12.0 - (10.0 + alpha * (5 + shift) + beta * (4 + 0.25))
        assert abs(moved.rows[4, 5, 6] - want) <= 1e-9 and abs(moved.rows[4, 5, 3] - gx) <= 1e-12, shift
    shifted[0, 3] = 0.25 * 2.0 / 64.0
    # a tap with NaN depth or intensity, or beyond the depth gate, removes only the photometric row -- of the four
    # cells that read it; a NaN frame intensity removes its own
    for edit in ('depth', 'intensity', 'gate', 'frame'):
        Z_, L_, f_ = depth.copy(), L.copy(), frame.copy()
        if edit == 'depth':
            Z_[7, 8] = NAN
        elif edit == 'intensity':
            L_[7, 8] = NAN
        elif edit == 'gate':
            Z_[7, 8] = 2.2
        else:
            f_[7, 8] = NAN
        e = oracle_color_rows(d, f_, Q, Z_, normals, L_, camera, transform=shifted, max_distance=0.1)
        gone = (o.mask & ~e.mask)
        cells = [(7, 8)] if edit == 'frame' else [(6, 7), (6, 8), (7, 7), (7, 8)]
        assert sorted(map(tuple, np.argwhere(gone))) == sorted(cells), edit
        if edit in ('intensity', 'frame'):
            assert e.geometric.mask.all(), edit


# ------------------------------------------------------------------------------------------------ the sign convention
def textured(height, width):
    """Two non-parallel sinusoids of period >= 16 px."""
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    return (128.0 + 40.0 * np.sin(2 * np.pi * (xx + 0.3 * yy) / 16.0) + 30.0 * np.sin(2 * np.pi * (yy - 0.2 * xx) / 20.0))


def test_the_sign_convention_recovers_a_twist_on_the_wall():
    height, width = 48, 64
    d, Q, depth, normals, camera = wall_case(height, width)
    depth = np.full_like(depth, 2.0)
    L = textured(height, width).astype(F)
    xi = np.array([0.0, 0.0, 0.004, 0.006, -0.004, 0.0])   # in-plane: what the wall leaves free
    # the frame sees the model moved by exp(xi)^-1: its pixel p, moved by xi, lands on the model sample it shows
    step = pds.se3_exp(xi)
    q, x, y, u, v = _projection(np.float64, d, f32(Q), step, f32(camera), False)
    frame = (128.0 + 40.0 * np.sin(2 * np.pi * (u + 0.3 * v) / 16.0) + 30.0 * np.sin(2 * np.pi * (v - 0.2 * u) / 20.0)).astype(F)
    o = oracle_color_rows(d, frame, Q, depth, normals, L, camera, max_distance=0.1)
    assert o.mask.mean() > 0.9
    geometric = oracle_system(o.geometric.rows)
    assert pds.icp_solve(geometric[None]).status.tolist() == [tracking.DEGENERATE]
    weight = 1e-3
    S = geometric.copy()
    S[:28] += weight ** 2 * oracle_system(o.rows)[:28]
    s = pds.icp_solve(S[None])
    assert s.status.tolist() == [tracking.TRACKED]
    # the tolerance is the linearisation error, from the second-order term: the image moves by m = |du, dv| <= 0.25 px
    # and the sinusoids have second derivatives A k^2; the residual's neglected term is A k^2 m^2 / 2 against a gradient
    # A k, a relative error k m / 2 of the step per sinusoid (k = 2 pi |(1, 0.3)| / 16 and 2 pi |(-0.2, 1)| / 20), to
    # which the bilinear model of the sinusoid adds its own curvature over one pixel, k / 8 in the same units
    moved = float(np.hypot(u - np.mgrid[0:height, 0:width][1], v - np.mgrid[0:height, 0:width][0]).max())
    k = max(2 * np.pi * np.hypot(1, 0.3) / 16.0, 2 * np.pi * np.hypot(0.2, 1) / 20.0)
    relative = k * moved / 2 + k / 8
    print('moved %.3f px, k %.3f / px, relative linearisation error %.3f; recovered %s' % (moved, k, relative, s.xi[0]))
    assert moved < 0.5
    assert np.abs(s.xi[0] - xi).max() <= relative * np.abs(xi).max()
    # the opposite sign would double the error instead
    assert np.abs(s.xi[0] + xi).max() > np.abs(xi).max()


# ------------------------------------------------------------------------------------------------ the GPU file's scenes
def corner_color():
    """The colour [nz, ny, nx, 3] of the corner volume, analytic in the voxel position."""
    nx, ny, nz = CORNER['dims']
    kk, jj, ii = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float64)
    one = 128.0 + 60.0 * np.sin(2 * np.pi * (ii + 0.4 * jj) / 9.0) + 30.0 * np.sin(2 * np.pi * (kk + 0.3 * ii) / 7.0)
    two = 120.0 + 50.0 * np.sin(2 * np.pi * (jj - 0.3 * kk) / 8.0)
    three = 100.0 + 40.0 * np.cos(2 * np.pi * (ii - jj + kk) / 11.0)
    return np.stack([one, two, three], axis=-1).astype(F)


def luma64(colors):
    return oracle_intensity_pyramid(np.asarray(colors, dtype=F)[None], 1, layout='nhwc')[0][0]


@functools.lru_cache(maxsize=None)
def corner_colour_scene(size=(72, 96)):
    """-> the keyword arguments of oracle_color_rows for the corner scene at `size` (height, width): frame 1 against the
    oracle's coloured raycast of the fused volume at POSE0, under the true transform."""
    height, width = size
    Q = q_of(height, width, CORNER['focal'] * width / CORNER['width'], CORNER['baseline'])
    camera = camera_of(Q)
    tsdf, weight = corner_state()
    rays = oracle_raycast(tsdf, weight, CORNER['origin'], CORNER['voxel_size'], camera, (width, height), pose=POSE0,
                          truncation=CORNER['truncation'])
    depth = rays.depth.astype(F)
    rendered = oracle_render(corner_color(), weight, CORNER['origin'], CORNER['voxel_size'], camera, (width, height), depth,
                             pose=POSE0)
    model_intensity = luma64(rendered.colors.reshape(height, width, 3))
    # the frame's image: the same texture seen from POSE1 (rendered through the same volume at the frame's pose)
    rays1 = oracle_raycast(tsdf, weight, CORNER['origin'], CORNER['voxel_size'], camera, (width, height), pose=POSE1,
                           truncation=CORNER['truncation'])
    rendered1 = oracle_render(corner_color(), weight, CORNER['origin'], CORNER['voxel_size'], camera, (width, height),
                              rays1.depth.astype(F), pose=POSE1)
    intensity = luma64(rendered1.colors.reshape(height, width, 3))
    near = tracking.compose(POSE0, tracking.invert(POSE1))
    return dict(disparity=corner_disparity(POSE1, size=size), intensity=intensity, matrix=Q, depth=depth,
                normals=rays.normals.astype(F), model_intensity=model_intensity, camera=camera, transform=near,
                max_distance=2 * CORNER['truncation'])


def colour_scenes():
    """name -> the keyword arguments of oracle_color_rows for every scene tests/test_gpu_icp_color.py holds against it."""
    scenes = {}
    for height, width in ((21, 37), (25, 41), (48, 64)):
        d, Q, depth, normals, camera = wall_case(height, width, slope=0.0005)
        rng = np.random.RandomState(height)
        tilted = np.hstack([pds.rectification.rodrigues(np.array([0.01, -0.02, 0.015])), [[0.011], [-0.007], [0.004]]])
        L = textured(height, width).astype(F)
        frame = (textured(height, width) + 3.0 * rng.randn(height, width)).astype(F)
        L[rng.rand(height, width) < 0.02] = NAN
        frame[rng.rand(height, width) < 0.02] = NAN
        scenes['wall %dx%d' % (width, height)] = dict(disparity=d, intensity=frame, matrix=Q, depth=depth, normals=normals,
                                                      model_intensity=L, camera=camera, transform=tilted, max_distance=0.1)
    # frame normals that look at the wall, look away or are NaN: step 6 runs (the photometric rows of such frames once
    # differed from run to run: csrc/icp_color.hip)
    rng = np.random.RandomState(11)
    facing = np.zeros((25, 41, 3), dtype=F)
    facing[..., 2] = np.where(rng.rand(25, 41) < 0.1, 1.0, -1.0)
    facing[rng.rand(25, 41) < 0.05] = NAN
    scenes['wall 41x25 with normals'] = dict(scenes['wall 41x25'], frame_normals=facing, min_cosine=0.5)
    corner = corner_colour_scene()
    scenes['corner'] = dict(corner)
    # (under the identity every pixel projects onto an integer u, v, the border of four cells: all undecided; see
    # textured_camera)
    rng = np.random.RandomState(5)
    scenes['corner masked'] = dict(corner, valid=rng.rand(72, 96) < 0.9, confidence=rng.rand(72, 96).astype(F),
                                   min_confidence=0.2)
    return scenes


def test_the_colour_restatement_stays_within_its_measured_error():
    worst = 0.0
    for name, kw in colour_scenes().items():
        o = oracle_color_rows(**kw)
        error = colour_restatement_error(o)
        decided = ~o.undecided
        assert ((~np.isnan(o.rows32[..., 6])) == o.mask)[decided].all(), name
        rows, undecided = int(o.mask.sum()), int((o.undecided & o.mask).sum())
        print('%s: %d photometric rows of %d geometric, %d undecided, float32 restatement vs fp64: %.3e of the scale' %
              (name, rows, int(o.geometric.mask.sum()), undecided, error))
        # (most rows must be compared; the 2 % of the tracking scenes is asked of the loops below, here 3 % do)
        assert rows >= 0.2 * o.mask.size and undecided <= 0.03 * rows, name
        worst = max(worst, error)
    print('REL32C: measured %.3e, held %.3e' % (worst, REL32C))
    assert 0.25 * REL32C <= worst <= REL32C


# ------------------------------------------------------------------------------------------------ the textured wall
TEXTURED = dict(dims=(14, 12, 3), color_weight=1e-3, iterations=10,
                shifts={1: (0.009, -0.006), 3: (0.045, -0.03)})   # metres in the wall's plane; a pixel is 15.6 mm at Z


def textured_camera():
    """The model's camera: the frame's, its principal point moved by a fraction of a pixel.  Seen through the frame's own
    camera every pixel of the first iteration (T = identity) projects onto an integer u, v -- the border of four bilinear
    cells, where one fp32 rounding picks the cell and with it I_u, I_v: every row would be undecided."""
    fx, fy, cx, cy, skew = camera_of(wall_volume(TEXTURED['dims'])[1])
    return (fx, fy, cx + 0.37, cy + 0.29, skew)


def textured_wall_state():
    """-> (tsdf, weight, color) float32 of the WALL volume after one frame, the colour analytic in the voxel position."""
    nx, ny, nz = TEXTURED['dims']
    t, w = wall_layers(nz)
    tsdf = np.broadcast_to(t[:, None, None], (nz, ny, nx)).astype(F).copy()
    weight = np.broadcast_to(w[:, None, None], (nz, ny, nx)).astype(F).copy()
    kk, jj, ii = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float64)
    one = 128.0 + 60.0 * np.sin(2 * np.pi * (ii + 0.35 * jj) / 5.0)
    two = 128.0 + 60.0 * np.sin(2 * np.pi * (jj - 0.25 * ii) / 4.0)
    three = 128.0 + 0.0 * kk
    return tsdf, weight, np.stack([one, two, three], axis=-1).astype(F)


def textured_truth(levels):
    sx, sy = TEXTURED['shifts'][levels]
    return np.hstack([np.eye(3), [[sx], [sy], [0.0]]])


@functools.lru_cache(maxsize=None)
def textured_wall_frame(levels, flat=False):
    """-> (disparity [48, 64], image float32 [3, 48, 64]) rendered at the truth pose of `levels` by the oracles."""
    tsdf, weight, color = textured_wall_state()
    if flat:
        color = np.full_like(color, 128.0)
    origin, Q = wall_volume(TEXTURED['dims'])
    camera, size = camera_of(Q), (TSDF_WALL['width'], TSDF_WALL['height'])
    pose = textured_truth(levels)
    rays = oracle_raycast(tsdf, weight, origin, TSDF_WALL['voxel_size'], camera, size, pose=pose,
                          truncation=TSDF_WALL['truncation'])
    depth = rays.depth.astype(F)
    rendered = oracle_render(color, weight, origin, TSDF_WALL['voxel_size'], camera, size, depth, pose=pose)
    with np.errstate(all='ignore'):
        disparity = (Q[2, 3] / (depth.astype(np.float64) * Q[3, 2])).astype(F)
    image = rendered.colors.reshape(size[1], size[0], 3).astype(F).transpose(2, 0, 1)
    return disparity, np.ascontiguousarray(image)


def oracle_pyramids(disparity, image, levels):
    """The frame side of track_color on the host: the disparity pyramid of a hole-free wall is the plain mean where all
    four children exist and NaN-aware otherwise (tests/test_pyramid_host.py holds the kernel to its own oracle; the wall
    has no depth edge, so max_difference never excludes a child)."""
    frames = [np.asarray(disparity, dtype=F)]
    for _ in range(levels - 1):
        a = frames[-1]
        h, w = a.shape[0] // 2, a.shape[1] // 2
        kids = np.stack([a[0:2 * h:2, 0:2 * w:2], a[0:2 * h:2, 1:2 * w:2], a[1:2 * h:2, 0:2 * w:2], a[1:2 * h:2, 1:2 * w:2]])
        ok = np.isfinite(kids) & (kids > 0)
        total = np.zeros((h, w), dtype=F)
        for k in range(4):
            total = np.where(ok[k], total + np.where(ok[k], kids[k], 0).astype(F), total).astype(F)
        n = ok.sum(axis=0)
        with np.errstate(all='ignore'):
            frames.append(np.where(n > 0, total / n.astype(F), NAN).astype(F))
    return frames, [t[0] for t in oracle_intensity_pyramid(image[None], levels)]


def oracle_track_color(levels, color_weight, flat=False, truth=None):
    """The loop of track_color in fp64 on the oracles' rows -> (pose, history, status); history: per iteration (level,
    geometric rows, photometric rows, undecided photometric rows, translation error before the step)."""
    tsdf, weight, color = textured_wall_state()
    if flat:
        color = np.full_like(color, 128.0)
    origin, Q = wall_volume(TEXTURED['dims'])
    camera, size = textured_camera(), (TSDF_WALL['width'], TSDF_WALL['height'])
    disparity, image = textured_wall_frame(levels, flat)
    frames, intensities = oracle_pyramids(disparity, image, levels)
    predicted = IDENTITY.copy()
    truth = textured_truth(levels)
    T, history, status = IDENTITY.copy(), [], tracking.TRACKED
    for l in range(levels - 1, -1, -1):
        camera_l = pds.pyramid_camera(camera, l)
        size_l = (size[0] >> l, size[1] >> l)
        rays = oracle_raycast(tsdf, weight, origin, TSDF_WALL['voxel_size'], camera_l, size_l, pose=predicted,
                              truncation=TSDF_WALL['truncation'])
        depth = rays.depth.astype(F)
        rendered = oracle_render(color, weight, origin, TSDF_WALL['voxel_size'], camera_l, size_l, depth, pose=predicted)
        L = luma64(rendered.colors.reshape(size_l[1], size_l[0], 3))
        for _ in range(TEXTURED['iterations']):
            o = oracle_color_rows(frames[l], intensities[l], pds.pyramid_matrix(Q, l), depth, rays.normals.astype(F), L,
                                  camera_l, transform=T, max_distance=2 * TSDF_WALL['truncation'], min_cosine=0.5)
            error = pose_error(tracking.compose(tracking.invert(T), predicted), truth)[1]
            history.append((l, int(o.geometric.mask.sum()), int(o.mask.sum()), int((o.undecided & o.mask).sum()), error))
            S = oracle_system(o.geometric.rows)
            S[:28] += color_weight ** 2 * oracle_system(o.rows)[:28]
            s = pds.icp_solve(S[None], 100, 1e-4)
            if l == 0:
                status = int(s.status[0])
            if s.status[0] != tracking.TRACKED:
                break
            T = tracking.compose(pds.se3_exp(s.xi[0]), T)
            if np.linalg.norm(s.xi[0]) < 1e-6:
                break
    if status != tracking.TRACKED:
        return predicted, history, status
    return tracking.compose(tracking.invert(T), predicted), history, status


# the end errors of oracle_track_color (metres from the truth pose), recorded by the test below: what the GPU is compared with
ORACLE_END = {1: 3.0e-4, 3: 1.1e-4}   # (measured 2.909e-04 and 1.082e-04)


@pytest.mark.parametrize('levels', (1, 3))
def test_the_textured_wall_meets_its_conditions_on_the_oracle(levels):
    truth = textured_truth(levels)
    pixel = TSDF_WALL['depth'] / TSDF_WALL['focal']
    shift = float(np.linalg.norm(truth[:, 3]))
    assert shift < pixel if levels == 1 else pixel < shift < 8 * pixel
    # geometry alone is refused
    pose, history, status = oracle_track_color(levels, 0.0)
    assert status == tracking.DEGENERATE and (pose == IDENTITY).all()
    # colour converges
    pose, history, status = oracle_track_color(levels, TEXTURED['color_weight'])
    pixels = TSDF_WALL['height'] * TSDF_WALL['width']
    for k, (l, rows, color_rows, undecided, error) in enumerate(history):
        print('iteration %d, level %d: %d rows, %d photometric (%.1f %% of the pixels), %d undecided, error %.3e m' %
              (k, l, rows, color_rows, 100.0 * color_rows / (pixels >> (2 * l)), undecided, error))
        assert undecided < 0.02 * color_rows and color_rows >= 0.20 * (pixels >> (2 * l)), k
    end = pose_error(pose, truth)
    print('levels %d: start %.3e m -> end %.3e rad %.3e m (recorded %.3e)' % ((levels, shift) + end + (ORACLE_END[levels],)))
    assert status == tracking.TRACKED and end[1] <= shift / 5
    assert 0.5 * ORACLE_END[levels] <= end[1] <= ORACLE_END[levels]
    # an untextured wall stays degenerate
    assert oracle_track_color(levels, TEXTURED['color_weight'], flat=True)[2] == tracking.DEGENERATE


# ------------------------------------------------------------------------------------------------ the corner, with colour
def corner_camera():
    """The model's camera of the coloured corner: the frame's, moved off the cell borders as textured_camera is."""
    fx, fy, cx, cy, skew = camera_of(corner_matrix())
    return (fx, fy, cx + 0.37, cy + 0.29, skew)


@functools.lru_cache(maxsize=None)
def corner_colour_frame():
    """-> the image float32 [3, 48, 64] of frame 1: the coloured volume rendered by the oracles at POSE1 (NaN where the
    volume shows no surface)."""
    tsdf, weight = corner_state()
    size = (CORNER['width'], CORNER['height'])
    camera = camera_of(corner_matrix())
    rays = oracle_raycast(tsdf, weight, CORNER['origin'], CORNER['voxel_size'], camera, size, pose=POSE1,
                          truncation=CORNER['truncation'])
    rendered = oracle_render(corner_color(), weight, CORNER['origin'], CORNER['voxel_size'], camera, size,
                             rays.depth.astype(F), pose=POSE1)
    return np.ascontiguousarray(rendered.colors.reshape(size[1], size[0], 3).astype(F).transpose(2, 0, 1))


@functools.lru_cache(maxsize=None)
def oracle_corner_loop(color_weight):
    """The single-level loop of track_color in fp64 on the coloured corner, frame 1 against the model at POSE0 with the
    keywords TRACK -> (pose, status); color_weight = 0 is the loop of track_pyramid(levels=1)."""
    tsdf, weight = corner_state()
    size, camera = (CORNER['width'], CORNER['height']), corner_camera()
    rays = oracle_raycast(tsdf, weight, CORNER['origin'], CORNER['voxel_size'], camera, size, pose=POSE0,
                          truncation=CORNER['truncation'])
    depth = rays.depth.astype(F)
    rendered = oracle_render(corner_color(), weight, CORNER['origin'], CORNER['voxel_size'], camera, size, depth, pose=POSE0)
    L = luma64(rendered.colors.reshape(size[1], size[0], 3))
    intensity = oracle_intensity_pyramid(corner_colour_frame()[None], 1)[0][0]
    T, status = IDENTITY.copy(), tracking.TRACKED
    for _ in range(TRACK['iterations']):
        o = oracle_color_rows(corner_disparity(POSE1), intensity, corner_matrix(), depth, rays.normals.astype(F), L, camera,
                              transform=T, max_distance=2 * CORNER['truncation'], min_cosine=0.5)
        S = oracle_system(o.geometric.rows)
        S[:28] += color_weight ** 2 * oracle_system(o.rows)[:28]
        s = pds.icp_solve(S[None], TRACK['min_count'], TRACK['min_eigenvalue'])
        status = int(s.status[0])
        if status != tracking.TRACKED:
            return POSE0.copy(), status
        T = tracking.compose(pds.se3_exp(s.xi[0]), T)
        if np.linalg.norm(s.xi[0]) < TRACK['tolerance']:
            break
    return tracking.compose(tracking.invert(T), POSE0), status


# what the two fp64 loops end at, (rad, m) from POSE1, recorded by the test below: the GPU's two loops may differ by as much
ORACLE_CORNER = {'geometric': (1.583e-3, 2.577e-3), 'colour': (1.184e-3, 2.469e-3)}


def test_the_coloured_corner_on_the_oracle():
    plain, status_plain = oracle_corner_loop(0.0)
    colour, status_colour = oracle_corner_loop(1e-3)
    assert status_plain == status_colour == tracking.TRACKED
    start, a, b = pose_error(POSE0, POSE1), pose_error(plain, POSE1), pose_error(colour, POSE1)
    print('start %.3e rad %.3e m; geometric %.3e rad %.3e m; with colour %.3e rad %.3e m' % (start + a + b))
    assert a[0] <= start[0] / 5 and a[1] <= start[1] / 5 and b[0] <= start[0] / 5 and b[1] <= start[1] / 5
    for got, name in ((a, 'geometric'), (b, 'colour')):
        for k in range(2):
            assert abs(got[k] - ORACLE_CORNER[name][k]) <= 0.01 * ORACLE_CORNER[name][k], (name, got)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_photometric_symbols_declared_exported_and_bound(hip_library):
    header = open(_lib.PHOTOMETRIC_HEADER_PATH).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = ('pds_intensity_pyramid_fwd', 'pds_icp_color_workspace_bytes', 'pds_icp_color_system_fwd')
    for name in names:
        assert name + '(' in header and hasattr(raw, name) and name in _lib.PHOTOMETRIC_SIGNATURES, name
        assert getattr(hip_library, name).argtypes == _lib.PHOTOMETRIC_SIGNATURES[name][1], name
        assert getattr(hip_library, name).restype == _lib.PHOTOMETRIC_SIGNATURES[name][0], name
    declared = sorted(set(re.findall(r'\b(pds_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S))))
    assert declared == sorted(names) == sorted(_lib.PHOTOMETRIC_SIGNATURES) and '#include "pds_hip.h"' in header
    assert header.count('Additive: ABI version unchanged') == 2
    assert not set(_lib.PHOTOMETRIC_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.TRACKING_SIGNATURES))
    assert hip_library.pds_abi_version() == 7 and _lib.ABI_VERSION == 7
    for phrase in ('fmaf(0.299f, c0, fmaf(0.587f, c1, 0.114f * c2))', '((a00 + a01) + (a10 + a11)) * 0.25f',
                   'I_u = fmaf(b, (L11 - L01) - (L10 - L00), L10 - L00)', 'g_z = -fmaf(g_x, x, g_y y)',
                   '2 * pds_icp_workspace_bytes', 'not in the reference'):
        assert phrase in header, phrase
    csrc = _lib.HEADER_PATH.replace('include/pds_hip.h', 'practicaldeepstereo_nips2018_amd/csrc/')
    assert 'pds_hip_photometric.h' in open(csrc + 'common.hpp').read()
    sources = [name.rsplit('/', 1)[-1] for name in _lib.sources()]
    assert 'intensity.hip' in sources and 'icp_color.hip' in sources
    # icp_row lives in the header both kernels include
    assert 'bool icp_row(' in open(csrc + 'icp_row.hpp').read()
    for user in ('icp.hip', 'icp_color.hip'):
        text = open(csrc + user).read()
        assert '#include "icp_row.hpp"' in text and 'bool icp_row(' not in text, user
    assert 'constexpr int kIntensityLevels = %d;' % pyramid.INTENSITY_LEVELS in open(csrc + 'common.hpp').read()
    sizes, plain = hip_library.pds_icp_color_workspace_bytes, hip_library.pds_icp_workspace_bytes
    for shape in ((1, 1, 1), (1, 25, 41), (3, 48, 64), (1, 540, 960), (19, 1, 1)):
        assert sizes(*shape) == 2 * plain(*shape) > 0, shape
    for name in ('intensity_pyramid', 'icp_color_system', 'IcpColorSystem', 'ColorTracking'):
        assert name in pds.__all__ and hasattr(pds, name), name
    assert pds.IcpColorSystem._fields == ('system', 'color_system', 'rows')
    assert pds.ColorTracking._fields == ('pose', 'rmse', 'inliers', 'iterations', 'status', 'color_rmse', 'color_inliers')


# sha256 of the two older headers at the commit this feature was built on: they are byte-identical to it
PARENT_HEADER_DIGESTS = {'pds_hip.h': '8e2b7e364d026901b87480c5a673fd40efc678234ad3e7c64ff51ed1e902f683',
                         'pds_hip_tracking.h': '3480237ec98835ecfaf92b7fa5bf0b5517b84b4a9cb8ab07fb7a2f7fbc9def9b'}


def test_the_older_headers_are_those_of_the_parent_commit():
    import hashlib
    for name, path in (('pds_hip.h', _lib.HEADER_PATH), ('pds_hip_tracking.h', _lib.TRACKING_HEADER_PATH)):
        assert hashlib.sha256(open(path, 'rb').read()).hexdigest() == PARENT_HEADER_DIGESTS[name], name


def test_photometric_validation_needs_no_gpu(hip_library):
    # (every call below is refused by the validation: the pointers are made up, and none may reach a launch)
    lib = hip_library
    big = 1 << 24
    error = lib.pds_last_error
    image, o0, o1, o2, o3 = [big * k for k in range(1, 6)]   # never dereferenced

    def pyramid_call(image=image, layout=0, out=(o0, o1, o2, o3), levels=4, shape=(1, 16, 24)):
        pointers = (ctypes.c_void_p * max(len(out), 1))(*out) if out is not None else None
        return lib.pds_intensity_pyramid_fwd(image, layout, pointers, levels, *shape, None)

    assert pyramid_call(image=None) != 0 and error() == b'intensity_pyramid: null pointer'
    assert pyramid_call(out=None) != 0 and error() == b'intensity_pyramid: null pointer'
    assert pyramid_call(out=(o0, None, o2, o3)) != 0 and error() == b'intensity_pyramid: null pointer'
    for shape in [(0, 16, 24), (1, 0, 24), (1, 16, -1)]:
        assert pyramid_call(shape=shape) != 0 and b'intensity_pyramid: bad shape' in error(), shape
    assert pyramid_call(shape=(1 << 12, 1 << 10, 1 << 10)) != 0 and b'32-bit indices' in error()
    assert pyramid_call(levels=1, out=(o0,), shape=((1 << 24) + 1, 1, 1)) != 0 and b'do not fit one launch' in error()
    assert pyramid_call(levels=1, out=(o0,), shape=(1 << 24, 1, 1)) != 0 and b'aliases' in error()   # (past that check)
    for levels in (0, 5, -1):
        assert pyramid_call(levels=levels) != 0 and b'levels must be in 1 .. 4' in error(), levels
    assert pyramid_call(shape=(1, 7, 24)) != 0 and b'level 3 of 24 x 7 is empty' in error()
    for layout in (-1, 3):
        assert pyramid_call(layout=layout) != 0 and b'image_layout must be 0, 1 or 2' in error(), layout
    assert pyramid_call(image=image + 2) != 0 and b'not 4-byte aligned' in error()
    assert pyramid_call(out=(o0 + 2, o1, o2, o3)) != 0 and b'not 4-byte aligned' in error()
    assert pyramid_call(out=(image + 64, o1, o2, o3)) != 0 and b'an output aliases the image' in error()
    assert pyramid_call(out=(o0, o0 + 64, o2, o3)) != 0 and b'an output aliases another output' in error()

    d, it, v, c, n, md, mn, mi, sy, cs, rw, ws = [ctypes.c_void_p(big * k) for k in range(1, 13)]
    floats = (lambda values: (ctypes.c_float * len(values))(*values))
    identity = floats(np.eye(4, dtype=F).reshape(-1).tolist())
    transforms = floats([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0])
    camera = floats([4.0, 4.0, 1.0, 0.5, 0.0])

    def call(disparity=d, intensity=it, valid=v, confidence=c, min_confidence=0.0, matrix=identity, normals=n,
             model_depth=md, model_normals=mn, model_intensity=mi, model=(1, 2, 3), camera=camera, transforms=transforms,
             max_distance=0.1, min_cosine=0.0, huber=INF, color_huber=INF, system=sy, color_system=cs, rows=rw,
             shape=(1, 2, 3), workspace=ws, workspace_bytes=512):
        return lib.pds_icp_color_system_fwd(disparity, intensity, valid, confidence, min_confidence, matrix, normals,
                                            model_depth, model_normals, model_intensity, *model, camera, transforms,
                                            max_distance, min_cosine, huber, color_huber, system, color_system, rows,
                                            *shape, workspace, workspace_bytes, None)

    for name in ('disparity', 'intensity', 'matrix', 'model_depth', 'model_normals', 'model_intensity', 'camera',
                 'transforms', 'system', 'color_system', 'workspace'):
        assert call(**{name: None}) != 0 and error() == b'icp_color: null pointer', name
    for shape in [(0, 2, 3), (1, 0, 3), (1, 2, 0), (-1, 2, 3)]:
        assert call(shape=shape) != 0 and b'icp_color: bad shape' in error(), shape
        assert lib.pds_icp_color_workspace_bytes(*shape) == 0 and b'icp_color: bad shape' in error(), shape
    assert call(shape=(1 << 12, 1 << 10, 1 << 10), workspace_bytes=1 << 40) != 0 and b'32-bit indices' in error()
    assert lib.pds_icp_color_workspace_bytes(1 << 12, 1 << 10, 1 << 10) == 0 and b'32-bit indices' in error()
    assert call(model=(2, 2, 3)) != 0 and b'model_batch must be 1 or batch = 1 (got 2)' in error()
    for model in [(1, 0, 3), (1, 2, -3), (1, 1 << 24, 1)]:
        assert call(model=model) != 0 and b'icp_color: bad model shape' in error(), model
    assert call(workspace_bytes=511) != 0 and b'workspace too small (511 < 512)' in error()
    for name in ('huber', 'color_huber'):
        for bad in (0.0, -1.0, NAN):
            assert call(**{name: bad}) != 0 and name.encode() + b' must be positive' in error(), (name, bad)
    assert call(min_confidence=NAN) != 0 and b'min_confidence is NaN' in error()
    for bad in (0.0, -0.1, NAN, INF):
        assert call(max_distance=bad) != 0 and b'max_distance must be positive and finite' in error(), bad
    assert call(min_cosine=NAN) != 0 and b'min_cosine is NaN' in error()
    for name, pointer in (('intensity', it), ('model_intensity', mi), ('color_system', cs), ('rows', rw)):
        assert call(**{name: ctypes.c_void_p(pointer.value + 2)}) != 0 and b'not 4-byte aligned' in error(), name
    assert call(workspace=ctypes.c_void_p(ws.value + 4)) != 0 and b'workspace is not 8-byte aligned' in error()
    assert call(color_system=it) != 0 and b'an output aliases an input' in error()
    assert call(color_system=ctypes.c_void_p(sy.value + 8)) != 0 and b'an output aliases another output' in error()
    assert call(rows=ctypes.c_void_p(mi.value + 20)) != 0 and b'an output aliases an input' in error()


# ------------------------------------------------------------------------------------------------ Python
def test_colour_python_errors_and_signatures():
    with pytest.raises(TypeError, match='image must be a torch.Tensor'):
        pds.intensity_pyramid(np.zeros((1, 3, 4, 5), dtype=F))
    with pytest.raises(TypeError, match='image must be uint8'):
        pds.intensity_pyramid(torch.zeros(1, 3, 4, 5).double())
    with pytest.raises(ValueError, match='a uint8 image must be'):
        pds.intensity_pyramid(torch.zeros(1, 3, 4, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match='a float32 image must be'):
        pds.intensity_pyramid(torch.zeros(1, 4, 5, 6))
    with pytest.raises(ValueError, match='a float32 image must be'):
        pds.intensity_pyramid(torch.zeros(1, 3, 5, 6), layout='nhwc')
    with pytest.raises(ValueError, match='layout must be'):
        pds.intensity_pyramid(torch.zeros(1, 3, 5, 6), layout='chw')
    with pytest.raises(ValueError, match='empty input'):
        pds.intensity_pyramid(torch.zeros(0, 3, 5, 6))
    with pytest.raises(ValueError, match='leaves no pixel'):
        pds.intensity_pyramid(torch.zeros(1, 3, 4, 32), levels=4)
    with pytest.raises(ValueError, match='levels must be in 1 .. 4'):
        pds.intensity_pyramid(torch.zeros(1, 3, 64, 64), levels=5)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pds.intensity_pyramid(torch.zeros(1, 3, 8, 8), levels=2)
    assert pyramid.intensity_layout(torch.zeros(2, 3, 4, 5))[0] == 0 and pyramid.intensity_layout(torch.zeros(2, 4, 5, 3))[0] == 2
    assert pyramid.intensity_layout(torch.zeros(2, 3, 4, 3))[0] == 0 and pyramid.intensity_layout(torch.zeros(2, 3, 4, 3), 'nhwc') == (2, (2, 3, 4))
    assert pyramid.intensity_layout(torch.zeros(2, 4, 5, 3, dtype=torch.uint8)) == (1, (2, 4, 5))
    assert list(inspect.signature(pds.intensity_pyramid).parameters) == ['image', 'levels', 'layout']

    ok, Q = torch.zeros(2, 4, 5), q_of(4, 5, 4.0, 0.5)
    model = pds.Raycast(torch.zeros(2, 4, 5), torch.zeros(2, 4, 5, 3))
    camera = camera_of(Q)

    def run(disparity=ok, intensity=ok, matrix=Q, model=model, model_intensity=ok, camera=camera, **kw):
        return pds.icp_color_system(disparity, intensity, matrix, model, model_intensity, camera, **kw)

    with pytest.raises(TypeError, match='intensity must be a torch.Tensor'):
        run(intensity=None)
    with pytest.raises(TypeError, match='model_intensity must be float32'):
        run(model_intensity=ok.double())
    with pytest.raises(ValueError, match='intensity .* and disparity .* differ in shape'):
        run(intensity=torch.zeros(2, 4, 4))
    with pytest.raises(ValueError, match='model_intensity must be'):
        run(model_intensity=torch.zeros(1, 4, 5))
    for name in ('huber', 'color_huber'):
        for bad in (0.0, -1.0, NAN):
            with pytest.raises(ValueError, match='%s must be positive' % name):
                run(**{name: bad})
    with pytest.raises(ValueError, match='max_distance must be positive and finite'):
        run(max_distance=NAN)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        run()
    parameters = inspect.signature(pds.icp_color_system).parameters
    assert list(parameters)[:6] == ['disparity', 'intensity', 'matrix', 'model', 'model_intensity', 'camera']
    assert [(k, p.default) for k, p in parameters.items()][6:] == [
        ('transform', None), ('normals', None), ('valid', None), ('confidence', None), ('min_confidence', 0.0),
        ('max_distance', 0.1), ('min_cosine', 0.0), ('huber', None), ('color_huber', None), ('with_rows', False)]
    parameters = inspect.signature(pds.ColorTsdfVolume.track_color).parameters
    assert [(k, p.default) for k, p in parameters.items()][1:9] == [
        ('disparity', inspect.Parameter.empty), ('image', inspect.Parameter.empty), ('matrix', inspect.Parameter.empty),
        ('pose', inspect.Parameter.empty), ('levels', 1), ('huber', None), ('color_huber', None), ('color_weight', 1e-3)]
    assert list(parameters.values())[9].kind is inspect.Parameter.VAR_KEYWORD
    track, color = inspect.signature(tracking.track).parameters, inspect.signature(tracking.track_color).parameters
    assert set(track) <= set(color) and all(color[k].default == track[k].default for k in track if k != 'levels')
    parameters = inspect.signature(pds.StereoRig.track_color).parameters
    assert list(parameters)[1:6] == ['volume', 'disparity', 'image', 'pose', 'valid']
    # a volume without colour has no model image; the colour keywords are judged before any device is asked
    plain = HostVolume((0.0, 0.0, 0.0), 0.1, (4, 3, 2), 0.3)
    frame, image = torch.zeros(1, 4, 5), torch.zeros(1, 3, 4, 5)
    with pytest.raises(TypeError, match='track_color needs a ColorTsdfVolume'):
        tracking.track_color(plain, frame, image, Q, IDENTITY)
    with pytest.raises(TypeError, match='volume must be a ColorTsdfVolume'):
        simple_rig(64, 48).track_color(plain, frame, image, IDENTITY)
    plain.color = None   # (enough of a colour volume for the argument checks)
    with pytest.raises(ValueError, match='color_weight must be finite and >= 0'):
        tracking.track_color(plain, frame, image, Q, IDENTITY, color_weight=-1.0)
    with pytest.raises(ValueError, match='color_huber must be positive'):
        tracking.track_color(plain, frame, image, Q, IDENTITY, color_huber=0.0)
    with pytest.raises(ValueError, match='does not match disparity'):
        tracking.track_color(plain, frame, torch.zeros(1, 3, 4, 4), Q, IDENTITY)
    with pytest.raises(ValueError, match='track needs the predicted pose'):
        tracking.track_color(plain, frame, image, Q, None)
    for phrase in ('track_color', 'metres per intensity level', '0.255', 'r_c - J_c xi', 'colour terms'):
        assert phrase in tracking.__doc__, phrase
    assert 'colour terms' not in tracking.__doc__.split('Out of scope for the module:')[1]
