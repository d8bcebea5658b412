"""CPU: the disparity pyramid (pds_disparity_pyramid_fwd; disparity_pyramid, pyramid_matrix, pyramid_camera), the
Huber-weighted ICP system (pds_icp_system_robust_fwd; icp_system_robust) and coarse-to-fine tracking
(TsdfVolume.track_pyramid(..., levels=, huber=, max_difference=)).

oracle_halve is the float32 numpy oracle of ONE halving, as practicaldeepstereo_nips2018_amd/pyramid.py states it: every
operation rounded to float32, the children in the order (0,0), (0,1), (1,0), (1,1).  It is held to hand-written 2 x 2 blocks
below and is what tests/test_gpu_pyramid.py compares the kernel with.  oracle_system_robust is the fp64 weighted system with
the weight computed in float32.

The tracking scene is the corner of tests/test_icp_host.py at 96 x 72, where three levels exist (24 x 18 at level 2).
oracle_track_pyramid is the fp64 loop of TsdfVolume.track_pyramid(levels=L) on oracle_rows.  The frame is moved k times the
POSE0 -> POSE1 motion away from the model (rotation vector and translation scaled by k), and both loops are scanned over k on
the oracle alone, never against the kernel (test_the_scan_over_start_offsets prints the scan).  An offset SEPARATES the
loops where the single-level loop is refused or ends farther from the truth than a tenth of its start while the three-level
loop cuts both error components by at least 10 x.  On this scene none does: three smooth planes under a gate of
2 * truncation = 18 cm let the single-level loop converge from 13 cm and 0.06 rad away (offset 3), and beyond offset 3.5 the
frame has left the volume for both.  The scan asserts exactly that, so that a change of the scene or the loop that makes an
offset separate is noticed, and the GPU test keeps the condition that holds: at POSE1 (offset 1) the three-level loop ends
no farther from the truth than the single-level loop, with the undecided share under 2 % of the rows at every iteration of
every level.  The Huber scene overwrites a rectangle of about 10 % of the frame with a disparity offset that still
passes max_distance; the Huber loop must end closer to the truth than the plain loop."""
import ctypes
import functools
import inspect
import math
import re

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib, pyramid, tracking
from tests.test_icp_host import (CORNER, IDENTITY, POSE0, TRACK, corner_disparity, oracle_rows, oracle_system, pose_error)
from tests.test_register_depth_host import EPS
from tests.test_tsdf_host import HostVolume, camera_of, fresh_state, oracle_integrate, q_of
from tests.test_tsdf_raycast_host import oracle_raycast

NAN, INF = float('nan'), float('inf')
F = np.float32


# ------------------------------------------------------------------------------------------------ one halving
def oracle_halve(d, max_difference, first=False, valid=None, confidence=None, min_confidence=0.0):
    """d float32 [..., H, W] -> (the next level float32 [..., H >> 1, W >> 1], the member count of every pixel).
    first: d is level 0 (its eligibility, with valid / confidence); otherwise a child is eligible if it is not NaN."""
    d = np.asarray(d)
    assert d.dtype == np.float32
    with np.errstate(all='ignore'):
        if first:
            ok = np.isfinite(d) & (d > 0)
            if valid is not None:
                ok &= np.asarray(valid) != 0
            if confidence is not None:
                ok &= np.asarray(confidence, dtype=F) >= F(min_confidence)
            d = np.where(ok, d, F(NAN))
        h, w = d.shape[-2] >> 1, d.shape[-1] >> 1
        children = [d[..., i:2 * h:2, j:2 * w:2] for i in (0, 1) for j in (0, 1)]
        m = np.full(children[0].shape, NAN, dtype=F)
        for c in children:
            m = np.where(~np.isnan(c) & ~(m >= c), c, m)
        total, count = np.zeros(m.shape, dtype=F), np.zeros(m.shape, dtype=np.int64)
        for c in children:
            member = ~np.isnan(c) & ((m - c).astype(F) <= F(max_difference))
            total = np.where(member, (total + c).astype(F), total)
            count += member
        out = np.where(count > 0, (total / np.maximum(count, 1).astype(F)).astype(F), F(NAN))
    return out.astype(F), count


def oracle_pyramid(d, levels, max_difference, **kw):
    out = [np.asarray(d, dtype=F)]
    for level in range(1, levels):
        out.append(oracle_halve(out[-1], max_difference, first=level == 1, **(kw if level == 1 else {}))[0])
    return out


def one(block, max_difference=1.0, **kw):
    return oracle_halve(np.array(block, dtype=F).reshape(2, 2), max_difference, **kw)[0].reshape(()).item()


def test_oracle_every_eligibility_pattern():
    values = [F(3.0), F(3.25), F(3.5), F(2.75)]
    for pattern in range(16):
        block = [values[i] if pattern >> i & 1 else F(NAN) for i in range(4)]
        kept = [values[i] for i in range(4) if pattern >> i & 1]
        for first in (True, False):
            got = one(block, 1.0, first=first)
            if not kept:
                assert math.isnan(got), pattern
                continue
            total = F(0.0)
            for v in kept:
                total = F(total + v)
            assert got == F(total / F(len(kept))), (pattern, first)
    # by hand: all four 12.5 / 4; three 9.75 / 3 = 3.25; the first two 6.25 / 2
    assert one(values) == 3.125 and one(values[:3] + [NAN]) == 3.25 and one(values[:2] + [NAN, NAN]) == 3.125
    # the same through valid and confidence at level 0: the pattern is the mask
    d = np.array(values, dtype=F).reshape(2, 2)
    for pattern in range(16):
        mask = np.array([pattern >> i & 1 for i in range(4)]).reshape(2, 2)
        by_nan = one([values[i] if pattern >> i & 1 else NAN for i in range(4)], first=True)
        by_valid = oracle_halve(d, 1.0, first=True, valid=mask)[0].item()
        by_confidence = oracle_halve(d, 1.0, first=True, confidence=np.where(mask, 0.5, 0.25), min_confidence=0.5)[0].item()
        assert (by_valid == by_nan or (math.isnan(by_valid) and math.isnan(by_nan))), pattern
        assert (by_confidence == by_nan or (math.isnan(by_confidence) and math.isnan(by_nan))), pattern


def test_oracle_the_foreground_wins_and_the_limit_is_a_member():
    # a block astride a depth edge: the largest disparity is the reference, the background is left out
    assert one([10.0, 10.5, 4.0, 4.25], 1.0) == 10.25 and one([4.0, 4.25, 10.0, NAN], 1.0) == 10.0
    assert one([10.0, 10.5, 4.0, 4.25], 7.0) == F(28.75) / F(4)
    # exactly m - c == max_difference: a member; the next float beyond it: not
    below = np.nextafter(F(7.0), F(-INF))
    assert F(8.0) - below > F(1.0) and F(8.0) - F(7.0) == F(1.0)
    assert one([8.0, 7.0, NAN, NAN], 1.0) == 7.5 and one([8.0, below, NAN, NAN], 1.0) == 8.0
    assert one([7.0, NAN, NAN, 8.0], 1.0) == 7.5 and one([below, NAN, NAN, 8.0], 1.0) == 8.0
    # max_difference 0: only the children equal to the largest
    assert one([5.0, 5.0, 4.999, 5.0], 0.0) == 5.0 and oracle_halve(np.array([[5, 5], [4.999, 5]], dtype=F), 0.0)[1].item() == 3


def test_oracle_what_level_zero_refuses():
    for bad in (0.0, -1.0, -0.0, INF, -INF, NAN):
        assert one([bad, 6.0, 6.5, 7.0], 5.0, first=True) == 6.5, bad
        assert math.isnan(one([bad] * 4, 5.0, first=True)), bad
    # above level 0 a child is eligible if it is not NaN: zero and negative values are values
    assert one([0.0, 1.0, NAN, NAN], 5.0) == 0.5 and one([-1.0, -2.0, NAN, NAN], 5.0) == -1.5
    # a NaN confidence fails, one below the threshold fails, one at it passes
    d = np.full((2, 2), 6.0, dtype=F)
    d[0, 0] = 8.0
    confidence = np.array([[NAN, 0.5], [0.49, 0.75]], dtype=F)
    out, count = oracle_halve(d, 5.0, first=True, confidence=confidence, min_confidence=0.5)
    assert out.item() == 6.0 and count.item() == 2
    assert oracle_halve(d, 5.0, first=False)[0].item() == 6.5


def test_oracle_odd_sizes_floor():
    d = np.arange(1, 36, dtype=F).reshape(5, 7)
    out, count = oracle_halve(d, 100.0, first=True)
    assert out.shape == (2, 3) and (count == 4).all()
    assert out[0, 0] == (1 + 2 + 8 + 9) / 4 and out[1, 2] == (19 + 20 + 26 + 27) / 4   # row 4 and column 6 are dropped
    levels = oracle_pyramid(np.ones((3, 21, 37), dtype=F), 5, 1.0)
    assert [a.shape for a in levels] == [(3, 21, 37), (3, 10, 18), (3, 5, 9), (3, 2, 4), (3, 1, 2)]
    assert all((a == 1).all() for a in levels)


def pattern_image(height, width, seed=0):
    """The adversarial image of the GPU test: smooth slopes, depth edges, every kind of hole, members at the limit."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    d = (20.0 + 0.05 * xx - 0.03 * yy + 0.2 * rng.rand(height, width)).astype(F)
    d[(xx // 5 + yy // 3) % 4 == 0] += F(6.0)                       # foreground tiles: edges everywhere
    d[::2, 1::2] = (d[::2, ::2][:, :d[::2, 1::2].shape[1]] - F(1.0))  # pairs exactly max_difference = 1 apart ...
    d[1::2, 1::4] = np.nextafter(d[1::2, 1::4], F(-INF))            # ... and neighbours a float further
    holes = rng.rand(height, width)
    for k, bad in enumerate((NAN, 0.0, -3.0, INF, -INF)):
        d[(holes >= 0.06 * k) & (holes < 0.06 * (k + 1))] = bad
    d[rng.rand(height, width) < 0.1] = NAN
    if height >= 8 and width >= 8:
        d[:8, :8] = NAN                                                # a whole level-3 pixel without a child
    valid = rng.rand(height, width) > 0.1
    confidence = rng.rand(height, width).astype(F)
    confidence[rng.rand(height, width) < 0.05] = NAN
    return d, valid, confidence


def test_the_pattern_image_exercises_every_member_count():
    d, valid, confidence = pattern_image(66, 70)
    out, count = oracle_halve(d, 1.0, first=True, valid=valid, confidence=confidence, min_confidence=0.2)
    assert set(np.unique(count).tolist()) == {0, 1, 2, 3, 4} and np.isnan(out).sum() == (count == 0).sum()
    plain = oracle_pyramid(d, 5, 1.0)
    assert all(np.isnan(a).any() and (~np.isnan(a)).any() for a in plain[:4])


# ------------------------------------------------------------------------------------------------ matrices, cameras
def test_pyramid_matrix_and_camera_closed_forms():
    Q = q_of(96, 128, 120.0, 0.12)
    S = np.array([[2, 0, 0, .5], [0, 2, 0, .5], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    assert (pyramid.STEP == S).all()
    assert (pds.pyramid_matrix(Q, 0) == Q).all()
    for level in (1, 2, 3, 5):
        power = np.linalg.matrix_power(S, level)
        assert np.abs(pds.pyramid_matrix(Q, level) - Q @ power).max() == 0 and pds.pyramid_matrix(Q, level).dtype == np.float64
        assert power[0, 3] == (2 ** level - 1) / 2
    camera = (120.0, 118.0, 63.5, 47.5, 0.25)
    assert pds.pyramid_camera(camera, 0) == camera
    assert pds.pyramid_camera(camera, 1) == (60.0, 59.0, 31.5, 23.5, 0.125)
    assert pds.pyramid_camera(camera, 2) == (30.0, 29.5, 15.5, 11.5, 0.0625)
    # the camera of a level sees the ray of the level's pixel centre: u_l = (u_0 - (2^l - 1) / 2) / 2^l
    for level in (1, 2, 3):
        fx, fy, cx, cy, skew = pds.pyramid_camera(camera, level)
        x, y = 0.3, -0.2
        u0, v0 = camera[0] * x + camera[4] * y + camera[2], camera[1] * y + camera[3]
        assert abs(fx * x + skew * y + cx - (u0 - (2 ** level - 1) / 2) / 2 ** level) <= 1e-12
        assert abs(fy * y + cy - (v0 - (2 ** level - 1) / 2) / 2 ** level) <= 1e-12
    # and it is the camera of the level's matrix
    # (the level's matrix is not in camera_of's canonical form: the ray of its pixel (x', y') is ((x' - cx) / fx, ..))
    fx, fy, cx, cy, _ = pds.pyramid_camera(camera_of(Q), 2)
    P = plane_points(pds.pyramid_matrix(Q, 2), 24, 32, 5.0)
    yy, xx = np.mgrid[0:24, 0:32].astype(np.float64)
    assert np.abs(P[..., 0] / P[..., 2] - (xx - cx) / fx).max() <= 1e-14 and np.abs(P[..., 1] / P[..., 2] - (yy - cy) / fy).max() <= 1e-14
    with pytest.raises(ValueError, match='level must be at least 0'):
        pds.pyramid_matrix(Q, -1)
    with pytest.raises(TypeError, match='level must be an integer'):
        pds.pyramid_camera(camera, 1.0)
    with pytest.raises(ValueError, match='matrix must be a finite 4x4'):
        pds.pyramid_matrix(np.eye(3), 1)
    with pytest.raises(ValueError, match='camera must hold 5 values'):
        pds.pyramid_camera((1.0, 2.0), 1)


def plane_points(matrix, height, width, d):
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    c = np.stack([xx, yy, np.full_like(xx, d), np.ones_like(xx)], axis=-1) @ np.asarray(matrix).T
    return c[..., :3] / c[..., 3:]


def test_a_constant_plane_reprojects_to_the_mean_of_its_children():
    Q = q_of(21, 37, 64.0, 0.125)
    fine = plane_points(Q, 21, 37, 4.0)
    for level in (1, 2):
        coarse = plane_points(pds.pyramid_matrix(Q, level), 21 >> level, 37 >> level, 4.0)
        step = 2 ** level
        h, w = 21 >> level, 37 >> level
        mean = fine[:h * step, :w * step].reshape(h, step, w, step, 3).mean(axis=(1, 3))
        assert np.abs(coarse - mean).max() <= 1e-14 * np.abs(fine).max(), level
    # the level-1 map of the constant plane is the plane
    assert (oracle_halve(np.full((21, 37), 4.0, dtype=F), 1.0, first=True)[0] == 4.0).all()


# ------------------------------------------------------------------------------------------------ the weighted system
_TRIANGLE = np.triu_indices(6)


def huber_weights(r, huber):
    """The weight of float32 residuals, computed in float32 as the kernel does."""
    r = np.abs(np.asarray(r, dtype=F))
    with np.errstate(all='ignore'):
        return np.where(r <= F(huber), F(1.0), (F(huber) / r).astype(F)).astype(F)


def oracle_system_robust(rows, huber):
    """rows [..., 7] (NaN rows: none) -> the 29 fp64 values with Huber weights (the weight in float32)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 7)
    rows = rows[~np.isnan(rows[:, 6])]
    J, r = rows[:, :6], rows[:, 6]
    w = huber_weights(r.astype(F), huber).astype(np.float64)
    A = J.T @ (J * w[:, None])
    return np.concatenate([A[_TRIANGLE], J.T @ (w * r), [(w * r) @ r], [float(len(rows))]])


def test_oracle_system_robust_against_a_hand_sum():
    rows = np.array([[1.0, 2.0, 0.0, 0.0, 0.0, 1.0, 0.5], [NAN] * 7, [0.0, 1.0, 3.0, 1.0, 0.0, 0.0, -2.0]])
    # huber 1: the first row weighs 1, the second 1 / 2
    s = oracle_system_robust(rows, 1.0)
    A, g, rr, count = tracking.unpack_system(s)
    assert count[0] == 2 and rr[0] == 0.25 + 0.5 * 4.0
    assert A[0, 0, 0] == 1 and A[0, 0, 1] == 2 and A[0, 1, 1] == 4 + 0.5 and A[0, 1, 2] == 1.5 and A[0, 2, 2] == 4.5
    assert A[0, 2, 3] == 1.5 and A[0, 3, 3] == 0.5 and A[0, 5, 5] == 1
    assert g[0].tolist() == [0.5, 1.0 - 1.0, -3.0, -1.0, 0.0, 0.5]
    # |r| == huber weighs 1, and huber = inf is the unweighted system exactly
    assert huber_weights([0.5, -2.0, 2.0, 0.0], 2.0).tolist() == [1.0, 1.0, 1.0, 1.0]
    assert huber_weights([4.0, -8.0], 2.0).tolist() == [0.5, 0.25] and huber_weights([3.0], 1.0)[0] == F(1.0) / F(3.0)
    rng = np.random.RandomState(5)
    many = rng.randn(300, 7).astype(F)
    many[::7] = NAN
    assert (oracle_system_robust(many, INF) == oracle_system(many)).all()
    assert (oracle_system_robust(many, 0.5)[:28] != oracle_system(many)[:28]).all()
    assert oracle_system_robust(many, 0.5)[28] == oracle_system(many)[28]


# ------------------------------------------------------------------------------------------------ the C ABI, Python
def test_pyramid_symbols_declared_exported_and_bound(hip_library):
    # the extension header of the tracking entry points and its own table
    header = open(_lib.TRACKING_HEADER_PATH).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('pds_disparity_pyramid_fwd', 'pds_icp_system_robust_fwd'):
        assert name + '(' in header and hasattr(raw, name) and name in _lib.TRACKING_SIGNATURES, name
        assert getattr(hip_library, name).argtypes == _lib.TRACKING_SIGNATURES[name][1], name
    declared = sorted(set(re.findall(r'\b(pds_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S))))
    assert declared == sorted(_lib.TRACKING_SIGNATURES) and '#include "pds_hip.h"' in header
    assert header.count('Additive: ABI version unchanged') == 2
    assert hip_library.pds_abi_version() == 7 and '#define PDS_ABI_VERSION 7' in open(_lib.HEADER_PATH).read()
    for name in ('disparity_pyramid', 'pyramid_matrix', 'pyramid_camera'):
        assert name in pds.__all__ and getattr(pds, name) is getattr(pyramid, name), name
    assert 'icp_system_robust' in pds.__all__ and pds.icp_system_robust is tracking.icp_system_robust
    assert 'pyramid.hip' in [name.rsplit('/', 1)[-1] for name in _lib.sources()]
    csrc = _lib.HEADER_PATH.replace('include/pds_hip.h', 'practicaldeepstereo_nips2018_amd/csrc/')
    assert 'constexpr int kPyramidLevels = %d;' % pyramid.LEVELS_PER_LAUNCH in open(csrc + 'common.hpp').read()
    assert 'constexpr int kPyramidBlock = %d;' % pyramid.BLOCK in open(csrc + 'pyramid.hip').read()
    assert [pyramid.launches(n) for n in (1, 2, 4, 5, 7, 8)] == [0, 1, 1, 2, 2, 3]
    assert list(inspect.signature(pds.disparity_pyramid).parameters) == ['disparity', 'levels', 'max_difference', 'valid',
                                                                        'confidence', 'min_confidence']
    # icp_system_robust: the arguments of icp_system with huber after the camera
    robust, plain = inspect.signature(pds.icp_system_robust).parameters, inspect.signature(pds.icp_system).parameters
    assert [k for k in robust if k != 'huber'] == [k for k in plain if k != 'huber'] and list(robust)[4] == 'huber'
    assert robust['huber'].default is inspect.Parameter.empty
    assert all(robust[k].default == plain[k].default for k in list(plain)[4:] if k != 'huber')
    parameters = inspect.signature(pds.TsdfVolume.track_pyramid).parameters
    assert [(k, p.default) for k, p in parameters.items()][1:7] == [
        ('disparity', inspect.Parameter.empty), ('matrix', inspect.Parameter.empty), ('pose', inspect.Parameter.empty),
        ('levels', 3), ('huber', None), ('max_difference', None)]
    assert list(parameters.values())[7].kind is inspect.Parameter.VAR_KEYWORD
    parameters = inspect.signature(tracking.track).parameters
    assert [(k, parameters[k].default) for k in ('levels', 'huber', 'max_difference')] == [
        ('levels', 1), ('huber', None), ('max_difference', None)]
    assert 'Out of scope: colour terms, frame-to-frame tracking, loop closure.' in tracking.__doc__
    assert tracking.DEFAULT_MAX_DIFFERENCE == 1.0


def test_pyramid_c_validation_needs_no_gpu(hip_library):
    lib = hip_library
    big = 1 << 24
    d, v, c, o1, o2, o3 = [big * k for k in range(1, 7)]   # never dereferenced
    error = lib.pds_last_error

    def call(disparity=d, valid=v, confidence=c, min_confidence=0.0, max_difference=1.0, out=(o1, o2, o3), levels=3,
             source_level=0, shape=(1, 16, 24)):
        pointers = (ctypes.c_void_p * max(len(out), 1))(*out) if out is not None else None
        return lib.pds_disparity_pyramid_fwd(disparity, valid, confidence, min_confidence, max_difference, pointers, levels,
                                             source_level, *shape, None)

    assert call(disparity=None) != 0 and error() == b'disparity_pyramid: null pointer'
    assert call(out=None) != 0 and error() == b'disparity_pyramid: null pointer'
    assert call(out=(o1, None, o3)) != 0 and error() == b'disparity_pyramid: null pointer'
    for shape in [(0, 16, 24), (1, 0, 24), (1, 16, -1)]:
        assert call(shape=shape) != 0 and b'disparity_pyramid: bad shape' in error(), shape
    assert call(shape=(1 << 12, 1 << 10, 1 << 10)) != 0 and b'32-bit indices' in error()
    for levels in (0, 4, -1):
        assert call(levels=levels) != 0 and b'levels must be in 1 .. 3' in error(), levels
    assert call(source_level=-1) != 0 and b'source_level must be >= 0' in error()
    assert call(shape=(1, 7, 24)) != 0 and b'level 3 of 24 x 7 is empty' in error()
    assert call(min_confidence=NAN) != 0 and b'min_confidence is NaN' in error()
    for bad in (-0.5, NAN, INF):
        assert call(max_difference=bad) != 0 and b'max_difference must be finite and >= 0' in error(), bad
    assert call(disparity=d + 2) != 0 and b'not 4-byte aligned' in error()
    assert call(out=(o1 + 1, o2, o3)) != 0 and b'not 4-byte aligned' in error()
    # 16 x 24: 1536 bytes of source; the levels hold 384, 96 and 24 bytes
    assert call(out=(d + 1532, o2, o3)) != 0 and b'an output aliases an input' in error()
    assert call(out=(o1, v + 380, o3)) != 0 and b'an output aliases an input' in error()
    assert call(out=(o1, o2, c)) != 0 and b'an output aliases an input' in error()
    assert call(out=(o1, o1 + 380, o3)) != 0 and b'an output aliases another output' in error()
    assert call(out=(o1, o2, o2 + 92)) != 0 and b'an output aliases another output' in error()
    # above level 0 valid and confidence are not read: an output may lie there
    assert call(out=(o1, o2, d), source_level=3) != 0 and b'an output aliases an input' in error()


def test_robust_c_validation_needs_no_gpu(hip_library):
    lib = hip_library
    big = 1 << 24
    d, md, mn, sy, ws = [ctypes.c_void_p(big * k) for k in range(1, 6)]
    floats = (lambda values: (ctypes.c_float * len(values))(*values))
    identity = floats(np.eye(4, dtype=F).reshape(-1).tolist())
    transforms = floats([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0])
    camera = floats([4.0, 4.0, 1.0, 0.5, 0.0])

    def call(huber=0.1, disparity=d, max_distance=0.1):
        return lib.pds_icp_system_robust_fwd(disparity, None, None, 0.0, identity, None, md, mn, 1, 2, 3, camera, transforms,
                                             max_distance, 0.0, huber, sy, None, 1, 2, 3, ws, 256, None)

    for bad in (0.0, -1.0, NAN):
        assert call(huber=bad) != 0 and b'icp: huber must be positive' in lib.pds_last_error(), bad
    assert call(disparity=None) != 0 and lib.pds_last_error() == b'icp: null pointer'
    assert call(max_distance=0.0) != 0 and b'max_distance must be positive and finite' in lib.pds_last_error()


def test_python_errors_come_before_the_device():
    ok = torch.zeros(2, 8, 12)
    with pytest.raises(TypeError, match='disparity must be a torch.Tensor'):
        pds.disparity_pyramid(np.zeros((2, 8, 12), dtype=F), 2, 1.0)
    with pytest.raises(TypeError, match='disparity must be float32'):
        pds.disparity_pyramid(ok.double(), 2, 1.0)
    with pytest.raises(ValueError, match='disparity must have 3 dimensions'):
        pds.disparity_pyramid(torch.zeros(8, 12), 2, 1.0)
    with pytest.raises(ValueError, match='empty input'):
        pds.disparity_pyramid(torch.zeros(0, 8, 12), 2, 1.0)
    for bad in (0, -1):
        with pytest.raises(ValueError, match='levels must be at least 1'):
            pds.disparity_pyramid(ok, bad, 1.0)
    for bad in (2.0, True, None):
        with pytest.raises(TypeError, match='levels must be an integer'):
            pds.disparity_pyramid(ok, bad, 1.0)
    with pytest.raises(ValueError, match='levels = 5 leaves no pixel of a 12 x 8 frame at level 4'):
        pds.disparity_pyramid(ok, 5, 1.0)
    for bad in (-1.0, NAN, INF):
        with pytest.raises(ValueError, match='max_difference must be finite and >= 0'):
            pds.disparity_pyramid(ok, 2, bad)
    with pytest.raises(TypeError, match='max_difference must be a number'):
        pds.disparity_pyramid(ok, 2, None)
    with pytest.raises(ValueError, match='valid must be torch.bool or torch.uint8'):
        pds.disparity_pyramid(ok, 2, 1.0, valid=torch.zeros(2, 8, 12))
    with pytest.raises(ValueError, match='differ in shape'):
        pds.disparity_pyramid(ok, 2, 1.0, confidence=torch.zeros(2, 8, 11))
    with pytest.raises(ValueError, match='min_confidence is NaN'):
        pds.disparity_pyramid(ok, 2, 1.0, min_confidence=NAN)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pds.disparity_pyramid(ok, 4, 1.0)
    # icp_system and track
    Q = q_of(8, 12, 4.0, 0.5)
    model = pds.Raycast(torch.zeros(2, 8, 12), torch.zeros(2, 8, 12, 3))
    for bad in (0.0, -0.1, NAN):
        with pytest.raises(ValueError, match='huber must be positive'):
            pds.icp_system_robust(ok, Q, model, camera_of(Q), bad)
    with pytest.raises(TypeError, match='huber must be a number'):
        pds.icp_system_robust(ok, Q, model, camera_of(Q), 'soft')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pds.icp_system_robust(ok, Q, model, camera_of(Q), INF)
    volume = HostVolume((0.0, 0.0, 0.0), 0.1, (4, 3, 2), 0.3)
    frame = torch.zeros(1, 8, 12)
    with pytest.raises(ValueError, match='levels must be at least 1'):
        volume.track_pyramid(frame, Q, IDENTITY, levels=0)
    with pytest.raises(ValueError, match='levels = 5 leaves no pixel'):
        volume.track_pyramid(frame, Q, IDENTITY, levels=5)
    with pytest.raises(ValueError, match=r'iterations must be a single value or hold one per level \(3\), got 2'):
        volume.track_pyramid(frame, Q, IDENTITY, levels=3, iterations=(4, 4))
    with pytest.raises(ValueError, match='iterations must be at least 1'):
        volume.track_pyramid(frame, Q, IDENTITY, levels=3, iterations=(4, 0, 4))
    with pytest.raises(ValueError, match=r'max_distance must be a single value or hold one per level \(2\), got 3'):
        volume.track_pyramid(frame, Q, IDENTITY, levels=2, max_distance=(0.1, 0.2, 0.3))
    with pytest.raises(ValueError, match='max_distance must be positive and finite'):
        volume.track_pyramid(frame, Q, IDENTITY, levels=2, max_distance=(0.1, 0.0))
    with pytest.raises(ValueError, match='huber must be positive'):
        volume.track_pyramid(frame, Q, IDENTITY, levels=1, huber=0.0)
    with pytest.raises(ValueError, match='max_difference must be finite and >= 0'):
        volume.track_pyramid(frame, Q, IDENTITY, levels=2, max_difference=-1.0)
    with pytest.raises(ValueError, match='levels = 3 leaves no pixel of a 3 x 8 model'):
        volume.track_pyramid(frame, Q, IDENTITY, levels=3, size=(3, 8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        volume.track_pyramid(frame, Q, IDENTITY, levels=3)


# ------------------------------------------------------------------------------------------------ the tracking scene
SIZE = (72, 96)                  # (height, width): 24 x 18 pixels at level 2, where more than min_count rows remain
LEVELS = 3
ROTATION, TRANSLATION = np.array([0.012, -0.015, 0.008]), np.array([0.03, -0.02, 0.025])   # MOTION of test_icp_host
OFFSETS = (1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0)
PYRAMID_OFFSET = 1.0             # POSE1: no offset of the scan separates the two loops (test_the_scan_over_start_offsets)
MAX_DISTANCE = 2 * CORNER['truncation']
HUBER = dict(offset=1.0, rectangle=(slice(22, 48), slice(30, 56)), shift=0.45, huber=0.01)


def scene_matrix():
    return q_of(SIZE[0], SIZE[1], CORNER['focal'] * SIZE[1] / CORNER['width'], CORNER['baseline'])


def offset_pose(k):
    """world -> the frame k times the POSE0 -> POSE1 motion away from frame 0."""
    motion = np.hstack([pds.rectification.rodrigues(k * ROTATION), (k * TRANSLATION)[:, None]])
    return tracking.compose(motion, POSE0)


@functools.lru_cache(maxsize=None)
def scene_state():
    o = oracle_integrate(*fresh_state(CORNER['dims']), disparity=corner_disparity(POSE0, SIZE), matrix=scene_matrix(),
                         origin=CORNER['origin'], voxel_size=CORNER['voxel_size'], truncation=CORNER['truncation'],
                         pose=POSE0)
    return o.tsdf.astype(F), o.weight.astype(F)


@functools.lru_cache(maxsize=None)
def scene_models():
    """-> per level (depth, normals) float32: the oracle's raycasts of scene_state at POSE0."""
    tsdf, weight = scene_state()
    models = []
    for level in range(LEVELS):
        rays = oracle_raycast(tsdf, weight, CORNER['origin'], CORNER['voxel_size'],
                              pds.pyramid_camera(camera_of(scene_matrix()), level), (SIZE[1] >> level, SIZE[0] >> level),
                              pose=POSE0, truncation=CORNER['truncation'])
        models.append((rays.depth.astype(F), rays.normals.astype(F)))
    return models


def oracle_track_pyramid(disparity, matrix, models, camera, predicted, truth, max_difference=tracking.DEFAULT_MAX_DIFFERENCE,
                         iterations=10, max_distance=0.1, min_count=100, min_eigenvalue=1e-4, tolerance=1e-6, huber=None):
    """The loop of TsdfVolume.track_pyramid(levels=len(models)) in fp64 on the oracle's rows -> (pose, [per system (level, rows,
    undecided rows, rotation error, translation error before the step)], status)."""
    levels = len(models)
    frames = oracle_pyramid(disparity, levels, max_difference)
    T, history, status = IDENTITY.copy(), [], tracking.TRACKED
    for level in range(levels - 1, -1, -1):
        for _ in range(iterations):
            o = oracle_rows(frames[level], pds.pyramid_matrix(matrix, level), models[level][0], models[level][1],
                            pds.pyramid_camera(camera, level), transform=T, max_distance=max_distance)
            error = pose_error(tracking.compose(tracking.invert(T), predicted), truth)
            history.append((level, int(o.mask.sum()), int((o.undecided & o.mask).sum())) + error)
            system = oracle_system(o.rows) if huber is None else oracle_system_robust(o.rows, huber)
            s = pds.icp_solve(system[None], min_count, min_eigenvalue)
            if s.status[0] != tracking.TRACKED:
                if level == 0:
                    return predicted.copy(), history, int(s.status[0])
                break
            T = tracking.compose(pds.se3_exp(s.xi[0]), T)
            if np.linalg.norm(s.xi[0]) < tolerance:
                break
    return tracking.compose(tracking.invert(T), predicted), history, status


@functools.lru_cache(maxsize=None)
def scanned(k, levels):
    truth = offset_pose(k)
    return oracle_track_pyramid(corner_disparity(truth, SIZE), scene_matrix(), scene_models()[:levels],
                                camera_of(scene_matrix()), POSE0, truth, max_distance=MAX_DISTANCE, **TRACK)


def test_the_scan_over_start_offsets():
    chosen, separates = None, []
    for k in OFFSETS:
        truth = offset_pose(k)
        start = pose_error(POSE0, truth)
        single, history1, status1 = scanned(k, 1)
        coarse, history3, status3 = scanned(k, LEVELS)
        end1, end3 = pose_error(single, truth), pose_error(coarse, truth)
        worst = max(undecided / max(rows, 1) for _, rows, undecided, _, _ in history1 + history3)
        fails = status1 != tracking.TRACKED or end1[0] > start[0] / 10 or end1[1] > start[1] / 10
        wins = status3 == tracking.TRACKED and end3[0] <= start[0] / 10 and end3[1] <= start[1] / 10
        print('offset %.1f: start %.3e rad %.3e m | one level: status %d, %2d systems, end %.3e rad %.3e m | %d levels: '
              'status %d, %2d systems, end %.3e rad %.3e m | undecided at most %.2f %% | %s' %
              (k, start[0], start[1], status1, len(history1), end1[0], end1[1], LEVELS, status3, len(history3), end3[0],
               end3[1], 100 * worst, 'separates' if fails and wins else '-'))
        separates.append(fails and wins)
        if k == PYRAMID_OFFSET:
            chosen = (status1, status3, start, end1, end3, history1 + history3)
    # no offset of this scene separates the loops (the module text): the condition of the GPU test is the one at POSE1
    assert not any(separates)
    status1, status3, start, end1, end3, history = chosen
    assert status1 == status3 == tracking.TRACKED
    assert end1[0] <= start[0] / 5 and end1[1] <= start[1] / 10   # both loops converge there ...
    # ... and the three-level loop ends no farther from the truth (to the last bits of two fp64 paths to one fixed point)
    assert end3[0] <= end1[0] * (1 + 1e-6) and end3[1] <= end1[1] * (1 + 1e-6)
    for level, rows, undecided, _, _ in history:
        assert undecided < 0.02 * rows and rows >= 100, (level, rows, undecided)
    assert {level for level, _, _, _, _ in history} == {0, 1, 2}


def huber_frame():
    """-> (the frame HUBER['offset'] motions away with a rectangle of about 10 % of its pixels shifted in disparity, its
    true pose)."""
    truth = offset_pose(HUBER['offset'])
    d = corner_disparity(truth, SIZE).copy()
    d[HUBER['rectangle']] += F(HUBER['shift'])
    return d, truth


@functools.lru_cache(maxsize=None)
def huber_tracked(huber):
    d, truth = huber_frame()
    return oracle_track_pyramid(d, scene_matrix(), scene_models()[:1], camera_of(scene_matrix()), POSE0, truth,
                                max_distance=MAX_DISTANCE, huber=huber, **TRACK)


def test_huber_ends_closer_than_the_plain_loop_on_the_oracle():
    d, truth = huber_frame()
    rectangle = np.zeros(SIZE, dtype=bool)
    rectangle[HUBER['rectangle']] = True
    assert 0.08 <= rectangle.mean() <= 0.12
    # the blob still passes max_distance: at the true pose its pixels give rows
    depth, normals = scene_models()[0]
    aligned = oracle_rows(d, scene_matrix(), depth, normals, camera_of(scene_matrix()),
                          transform=tracking.compose(POSE0, tracking.invert(truth)), max_distance=MAX_DISTANCE)
    assert (aligned.mask & rectangle).sum() >= 0.8 * (aligned.mask.sum() * rectangle.mean())
    assert np.nanmedian(np.abs(aligned.rows[..., 6][rectangle])) > 3 * HUBER['huber']
    plain, _, status_plain = huber_tracked(None)
    robust, history, status_robust = huber_tracked(HUBER['huber'])
    assert status_plain == status_robust == tracking.TRACKED
    e_plain, e_robust = pose_error(plain, truth), pose_error(robust, truth)
    print('the blob frame: plain %.3e rad %.3e m; huber %.3g m: %.3e rad %.3e m; ratio %.2f (rotation) %.2f (translation)' %
          (e_plain + (HUBER['huber'],) + e_robust + (e_plain[0] / e_robust[0], e_plain[1] / e_robust[1])))
    assert e_robust[0] < e_plain[0] and e_robust[1] < e_plain[1]
    for _, rows, undecided, _, _ in history:
        assert undecided < 0.02 * rows
