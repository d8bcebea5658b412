"""CPU: depth registration (pds_register_depth_workspace_bytes, pds_register_depth_fwd; register_depth,
StereoRig.register_depth).  The entry points are declared, exported and bound and validate their arguments without a GPU,
the Python surface refuses what it cannot run, and the rig builds the poses its doc string promises.

The numpy fp64 oracle of tests/test_gpu_register_depth.py lives here and is itself held to hand-written answers, so that
a wrong oracle cannot pass a wrong kernel.  Semantics (include/pds_hip.h): every kept pixel of `reproject` under M' =
[[R, t], [0, 0, 0, 1]] matrix is projected into the target camera through the Brown-Conrady model, lands on the footprint
of `splat`, and the nearest wins -- among equal depths the smaller source index.  The oracle does not decide winners near
a pixel border: a source whose u or v lies within tau of a border of its footprint is an AMBIGUOUS candidate of the
pixels on either side, and check_registration accepts either outcome there (and nowhere else)."""
import collections
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib, registration

NAN, INF = float('nan'), float('inf')
EPS = 1e-5          # relative, on depths: about twenty fp32 roundings of 6e-8 without cancellation
TAU = 2.0 ** -8     # px: coordinates below 2048 have an ulp of at most 2^-13; such a chain stays well below 32 ulp
TILE = 1024         # csrc/common.hpp: kRegisterDepthTile

# kept [B, H, W] bool; z, u, v [B, H, W] fp64 (NaN where dropped); sure / maybe: per batch entry, {target pixel
# ty * Wt + tx: [source pixels p, ascending]}
Registration = collections.namedtuple('Registration', ['kept', 'z', 'u', 'v', 'sure', 'maybe', 'size'])


# ------------------------------------------------------------------------------------------------ the oracle
def as_the_kernel_sees(matrix, pose, camera, distortion):
    """-> (M' (4, 4), camera (5,), distortion (5,)) in fp64, each first rounded to float32 as the entry point gets them."""
    composed = registration.compose(pose, matrix).astype(np.float32).astype(np.float64)
    camera = np.asarray(camera, dtype=np.float64).astype(np.float32).astype(np.float64)
    distortion = np.asarray([] if distortion is None else distortion, dtype=np.float64).reshape(-1)
    distortion = np.concatenate([distortion, np.zeros(5 - distortion.size)]).astype(np.float32).astype(np.float64)
    return composed, camera, distortion


def span(coordinate, splat, tau):
    """Per source: (first sure, last sure, first possible, last possible) target column (or row) of its footprint when
    the coordinate may be off by tau.  An empty sure range has first > last."""
    if splat == 1:
        lo, hi = np.floor(coordinate - tau + 0.5), np.floor(coordinate + tau + 0.5)
        return np.where(lo == hi, lo, 1), np.where(lo == hi, hi, 0), lo, hi
    lo, hi = np.floor(coordinate - tau), np.floor(coordinate + tau)
    return hi, lo + 1, lo, hi + 1   # {lo, lo + 1} and {hi, hi + 1} share hi .. lo + 1


def oracle_registration(disparity, matrix, pose, camera, distortion, size, valid=None, confidence=None,
                        min_confidence=0.0, splat=1, tau=0.0):
    disparity = np.asarray(disparity, dtype=np.float32)
    assert disparity.ndim == 3 and splat in (1, 2)
    batch, height, width = disparity.shape
    target_width, target_height = size
    M, (fx, fy, cx, cy, skew), (k1, k2, p1, p2, k3) = as_the_kernel_sees(matrix, pose, camera, distortion)
    d = disparity.astype(np.float64)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    with np.errstate(all='ignore'):
        X, Y, Z, W = (M[r, 0] * xx + M[r, 1] * yy + M[r, 2] * d + M[r, 3] for r in range(4))
        kept = np.isfinite(d) & (d > 0) & (W > 0)
        if valid is not None:
            kept &= np.asarray(valid, dtype=bool)
        if confidence is not None:
            kept &= np.asarray(confidence, dtype=np.float32) >= np.float32(min_confidence)   # (a NaN fails)
        X, Y, Z = X / W, Y / W, Z / W
        kept &= np.isfinite(Z) & (Z > 0)
        x, y = X / Z, Y / Z
        r2 = x * x + y * y
        kept &= 1.0 + 3.0 * k1 * r2 + 5.0 * k2 * r2 ** 2 + 7.0 * k3 * r2 ** 3 > 0
        kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = x * kr + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        yd = y * kr + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        u = fx * xd + skew * yd + cx
        v = fy * yd + cy
        kept &= np.isfinite(u) & np.isfinite(v)
    z, u, v = (np.where(kept, a, NAN) for a in (Z, u, v))
    sure, maybe = [], []
    for b in range(batch):
        sure_b, maybe_b = collections.defaultdict(list), collections.defaultdict(list)
        sources = np.flatnonzero(kept[b].reshape(-1))
        ub, vb = u[b].reshape(-1)[sources], v[b].reshape(-1)[sources]
        xs = [a.astype(np.int64) for a in span(np.clip(ub, -4.0, target_width + 4.0), splat, tau)]
        ys = [a.astype(np.int64) for a in span(np.clip(vb, -4.0, target_height + 4.0), splat, tau)]
        for i, p in enumerate(sources.tolist()):
            for ty in range(max(int(ys[2][i]), 0), min(int(ys[3][i]), target_height - 1) + 1):
                for tx in range(max(int(xs[2][i]), 0), min(int(xs[3][i]), target_width - 1) + 1):
                    certain = xs[0][i] <= tx <= xs[1][i] and ys[0][i] <= ty <= ys[1][i]
                    (sure_b if certain else maybe_b)[ty * target_width + tx].append(p)
        sure.append(dict(sure_b))
        maybe.append(dict(maybe_b))
    return Registration(kept, z, u, v, sure, maybe, (target_width, target_height))


def winners(oracle):
    """-> (depth fp64 [B, Ht, Wt] with NaN, index int32 with -1, valid) where nothing is ambiguous: the nearest sure
    candidate, among equal depths the smaller index."""
    target_width, target_height = oracle.size
    batch = len(oracle.sure)
    depth = np.full((batch, target_height * target_width), NAN)
    index = np.full((batch, target_height * target_width), -1, dtype=np.int32)
    for b in range(batch):
        assert not oracle.maybe[b], 'winners() needs tau = 0'
        z = oracle.z[b].reshape(-1)
        for t, sources in oracle.sure[b].items():
            index[b, t] = min(sources, key=lambda p: (z[p], p))
            depth[b, t] = z[index[b, t]]
    shape = (batch, target_height, target_width)
    return depth.reshape(shape), index.reshape(shape), (index >= 0).reshape(shape)


def statistics(oracle):
    """-> (share of (source, target) pairs that are ambiguous, share of the target pixels with a sure candidate that have
    two or more)."""
    sure_pairs = sum(len(s) for entry in oracle.sure for s in entry.values())
    maybe_pairs = sum(len(s) for entry in oracle.maybe for s in entry.values())
    hit = sum(len(entry) for entry in oracle.sure)
    contested = sum(len(s) >= 2 for entry in oracle.sure for s in entry.values())
    return maybe_pairs / max(sure_pairs + maybe_pairs, 1), contested / max(hit, 1)


def check_registration(depth, index, valid, oracle, eps=EPS, case=''):
    """The three conditions on a result (numpy: depth float32, index int32, valid bool, [B, Ht, Wt]), with C(t) the sure
    and P(t) the ambiguous candidates of target pixel t:
        C u P empty  =>  invalid
        C not empty  =>  valid and min Z(C u P) (1 - eps) <= depth <= min Z(C) (1 + eps)
        valid        =>  index in C u P and that source's Z within eps (relative) of depth
    and, on every invalid pixel, index == -1.  No pixel is excluded.  -> the number of valid pixels."""
    target_width, target_height = oracle.size
    batch = len(oracle.sure)
    assert depth.shape == index.shape == valid.shape == (batch, target_height, target_width), case
    assert depth.dtype == np.float32 and index.dtype == np.int32 and valid.dtype == np.bool_, case
    for b in range(batch):
        z = oracle.z[b].reshape(-1)
        got_depth, got_index, got_valid = (a[b].reshape(-1) for a in (depth, index, valid))
        sure, maybe = oracle.sure[b], oracle.maybe[b]
        for t in range(target_height * target_width):
            C, P = sure.get(t, []), maybe.get(t, [])
            where = (case, b, divmod(t, target_width))
            if not C and not P:
                assert not got_valid[t], where
            if C:
                assert got_valid[t], where
                low, high = min(z[p] for p in C + P) * (1.0 - eps), min(z[p] for p in C) * (1.0 + eps)
                assert low <= got_depth[t] <= high, where + (low, float(got_depth[t]), high)
            if got_valid[t]:
                assert got_index[t] in C or got_index[t] in P, where + (int(got_index[t]),)
                assert abs(z[got_index[t]] - got_depth[t]) <= eps * z[got_index[t]], where
            else:
                assert got_index[t] == -1, where
    return int(valid.sum())


# ------------------------------------------------------------------------------------------------ hand-made cameras
F, B = 4.0, 0.5


def q_of(height, width):
    """The Q of a rectified rig with focal length F px and baseline B: the point of (x, y, d) is B (x - cx, y - cy, F) / d,
    its depth B F / d."""
    return np.array([[1.0, 0.0, 0.0, -0.5 * (width - 1)], [0.0, 1.0, 0.0, -0.5 * (height - 1)], [0.0, 0.0, 0.0, F],
                     [0.0, 0.0, 1.0 / B, 0.0]])


def same_camera(height, width, scale=1.0, shift=0.0):
    return (F * scale, F * scale, 0.5 * (width - 1) * scale + shift, 0.5 * (height - 1) * scale, 0.0)


IDENTITY = np.hstack([np.eye(3), np.zeros((3, 1))])
TO_THE_RIGHT = np.hstack([np.eye(3), [[-B], [0.0], [0.0]]])   # the rectified right camera: u = x - d


def test_oracle_2x3_by_hand():
    # the right view: column x - d.  Row 0: x = 1 (d = 1) and x = 2 (d = 2) both land on column 0, d = 2 is nearer.
    # Row 1: x = 0 leaves the image, x = 1 -> 0, x = 2 -> 1.
    d = np.array([[[NAN, 1.0, 2.0], [1.0, 1.0, 1.0]]], dtype=np.float32)
    o = oracle_registration(d, q_of(2, 3), TO_THE_RIGHT, same_camera(2, 3), None, (3, 2))
    assert o.kept.tolist() == [[[False, True, True], [True, True, True]]]
    assert np.allclose(o.u[0], [[NAN, 0.0, 0.0], [-1.0, 0.0, 1.0]], equal_nan=True, atol=1e-12)
    assert np.allclose(o.v[0], [[NAN, 0.0, 0.0], [1.0, 1.0, 1.0]], equal_nan=True, atol=1e-12)
    assert np.allclose(o.z[0], [[NAN, 2.0, 1.0], [2.0, 2.0, 2.0]], equal_nan=True, atol=1e-12)   # B F / d
    assert o.sure == [{0: [1, 2], 3: [4], 4: [5]}] and o.maybe == [{}]
    depth, index, valid = winners(o)
    assert index.tolist() == [[[2, -1, -1], [4, 5, -1]]] and index.dtype == np.int32
    assert np.allclose(depth, [[[1.0, NAN, NAN], [2.0, 2.0, NAN]]], equal_nan=True)
    assert valid.tolist() == [[[True, False, False], [True, True, False]]]
    # valid and confidence take the nearer one away: the farther one is seen
    o = oracle_registration(d, q_of(2, 3), TO_THE_RIGHT, same_camera(2, 3), None, (3, 2),
                            valid=np.array([[[True, True, False], [True, True, True]]]))
    assert winners(o)[1].tolist() == [[[1, -1, -1], [4, 5, -1]]]
    confidence = np.array([[[0.9, 0.5, 0.4999], [NAN, 0.5, 0.6]]], dtype=np.float32)
    o = oracle_registration(d, q_of(2, 3), TO_THE_RIGHT, same_camera(2, 3), None, (3, 2), confidence=confidence,
                            min_confidence=0.5)
    assert winners(o)[1].tolist() == [[[1, -1, -1], [4, 5, -1]]] and not o.kept[0, 1, 0]
    # d <= 0 and non-finite d are dropped; behind the camera (a pose that turns round) everything is
    o = oracle_registration(np.array([[[0.0, -1.0, INF]]], dtype=np.float32), q_of(1, 3), IDENTITY, same_camera(1, 3),
                            None, (3, 1))
    assert not o.kept.any() and o.sure == [{}]
    about_face = np.hstack([np.diag([-1.0, 1.0, -1.0]), np.zeros((3, 1))])
    o = oracle_registration(np.ones((1, 2, 3), dtype=np.float32), q_of(2, 3), about_face, same_camera(2, 3), None, (3, 2))
    assert not o.kept.any() and np.isnan(o.z).all()


def test_oracle_an_equal_depth_tie_goes_to_the_smaller_index():
    # a target of half the resolution whose principal point puts x = 0, 1 at u = -0.25, 0.25: both round to column 0
    d = np.full((1, 1, 4), 2.0, dtype=np.float32)
    camera = (0.5 * F, 0.5 * F, 0.5, 0.0, 0.0)   # u = (x - 1.5) / 2 + 0.5
    o = oracle_registration(d, q_of(1, 4), IDENTITY, camera, None, (2, 1))
    assert np.allclose(o.u[0, 0], [-0.25, 0.25, 0.75, 1.25]) and np.all(o.z == 1.0)
    assert o.sure == [{0: [0, 1], 1: [2, 3]}]
    depth, index, valid = winners(o)
    assert index.tolist() == [[[0, 2]]] and depth.tolist() == [[[1.0, 1.0]]] and valid.all()
    # the checker refuses the larger index of a tie, a depth that is off and a hole
    good = (depth.astype(np.float32), index, valid)
    assert check_registration(*good, o) == 2
    for bad in ((np.array([[[1.0, 1.0001]]], dtype=np.float32), index, valid),
                (good[0], np.array([[[0, 1]]], dtype=np.int32), valid),
                (good[0], np.array([[[0, -1]]], dtype=np.int32), valid),
                (np.array([[[1.0, NAN]]], dtype=np.float32), np.array([[[0, -1]]], dtype=np.int32),
                 np.array([[[True, False]]]))):
        with pytest.raises(AssertionError):
            check_registration(*bad, o)
    # (the bands cannot tell index 1 from index 0 at equal Z: the known-answer GPU tests compare the index exactly)
    assert check_registration(good[0], np.array([[[1, 2]]], dtype=np.int32), valid, o) == 2


def test_oracle_fold_back_is_rejected():
    # k1 = -0.5: d(r kr)/dr = 1 - 1.5 r2 <= 0 from r2 = 2/3 on.  The point at x = 1 (r2 = 1) would land at u = F / 2 + cx,
    # inside the image, where the point at x = 0.5 (r2 = 0.25, kept) lands at u = 0.4375 F + cx
    width = 9
    d = np.full((1, 1, width), 1.0, dtype=np.float32)   # depth B F, x_n = (x - 4) / F: -1 .. 1
    o = oracle_registration(d, q_of(1, width), IDENTITY, same_camera(1, width), (-0.5, 0.0, 0.0, 0.0), (width, 1))
    r2 = ((np.arange(width) - 4.0) / F) ** 2
    assert o.kept[0, 0].tolist() == (r2 < 2.0 / 3.0).tolist() == [False] + [True] * 7 + [False]
    assert np.allclose(o.u[0, 0, 1:8], F * ((np.arange(1, 8) - 4.0) / F) * (1 - 0.5 * r2[1:8]) + 4.0)
    without = oracle_registration(d, q_of(1, width), IDENTITY, same_camera(1, width), None, (width, 1))
    assert without.kept.all()
    # without the guard the folded point WOULD be inside: u = 0.5 F + 4 = 6
    assert 0 <= F * 1.0 * (1 - 0.5) + 4.0 < width
    # k2 and k3 count too: 1 + 5 k2 r2^2 <= 0 and 1 + 7 k3 r2^3 <= 0 at r2 = 1
    for distortion in ((0.0, -0.2, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0, -1.0 / 7.0)):
        o = oracle_registration(d, q_of(1, width), IDENTITY, same_camera(1, width), distortion, (width, 1))
        assert not o.kept[0, 0, 0] and not o.kept[0, 0, 8] and o.kept[0, 0, 1:8].all(), distortion


def test_oracle_splat_2_footprints_at_the_corners():
    # u = x - 0.5, v = y - 0.5: the source (0, 0) covers {-1, 0}^2, of which (0, 0) is inside; the last source covers
    # {Wt - 1, Wt} x {Ht - 1, Ht}, of which one pixel is inside
    d = np.full((1, 2, 3), 1.0, dtype=np.float32)
    o = oracle_registration(d, q_of(2, 3), IDENTITY, same_camera(2, 3, shift=-0.5)[:3] + (0.0, 0.0), None, (3, 2), splat=2)
    assert np.allclose(o.u[0], [[-0.5, 0.5, 1.5]] * 2) and np.allclose(o.v[0], [[-0.5] * 3, [0.5] * 3])
    assert o.sure == [{0: [0, 1, 3, 4], 1: [1, 2, 4, 5], 2: [2, 5], 3: [3, 4], 4: [4, 5], 5: [5]}]
    assert winners(o)[1].tolist() == [[[0, 1, 2], [3, 4, 5]]]   # equal depths: the smallest index
    # splat 1 rounds half up: u = -0.5 -> column 0, v = -0.5 -> row 0
    o1 = oracle_registration(d, q_of(2, 3), IDENTITY, same_camera(2, 3, shift=-0.5)[:3] + (0.0, 0.0), None, (3, 2))
    assert o1.sure == [{0: [0], 1: [1], 2: [2], 3: [3], 4: [4], 5: [5]}]
    # a coordinate within tau of a border is ambiguous on both sides, sure on neither
    o = oracle_registration(d[:, :1, :1], q_of(1, 1), IDENTITY, (F, F, 1.499, 1.0, 0.0), None, (4, 3), tau=0.01)
    assert o.sure == [{}] and o.maybe == [{5: [0], 6: [0]}]   # row 1, column 1 or 2
    # splat 2 at u = 1.001, v = 1.5: column 1 is in {0, 1} and in {1, 2}, columns 0 and 2 in one of them; rows 1 and 2
    o = oracle_registration(d[:, :1, :1], q_of(1, 1), IDENTITY, (F, F, 1.001, 1.5, 0.0), None, (4, 3), splat=2, tau=0.01)
    assert o.sure == [{5: [0], 9: [0]}] and o.maybe == [{4: [0], 6: [0], 8: [0], 10: [0]}]
    assert statistics(o) == (4 / 6, 0.0)


# ------------------------------------------------------------------------------------------------ the general case
def rotated_rig(width, height):
    """A rig with two degrees between the cameras, so that R1 and R2 are no identities."""
    K = np.array([[0.7 * width, 0.0, 0.5 * width - 0.5], [0.0, 0.7 * width, 0.5 * height - 0.5], [0.0, 0.0, 1.0]])
    R = pds.rectification.rodrigues(np.array([0.3, -0.8, 0.5]) / np.linalg.norm([0.3, -0.8, 0.5]) * np.radians(2.0))
    return pds.StereoRig(K, np.array([-0.05, 0.01, 1e-3, -5e-4]), K, np.array([-0.04, 0.02, -4e-4, 6e-4]), R,
                         np.array([-0.12, 0.004, -0.002]), (width, height))


def depth_scene(shape, seed, focal_times_baseline):
    """Disparities of a slanted wall 20 .. 50 m away with boxes 1 .. 8 m away in front of it, 2 % outliers anywhere in
    1 .. 50 m and a few NaN / inf / negative holes: float32 [B, H, W]."""
    batch, height, width = shape
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    out = []
    for b in range(batch):
        depth = 20.0 + 30.0 * (0.7 * xx / max(width - 1, 1) + 0.3 * yy / max(height - 1, 1))
        for _ in range(3 + b):
            y, x = rng.randint(0, height), rng.randint(0, width)
            depth[y:y + rng.randint(height // 6 + 1, height // 2 + 2),
                  x:x + rng.randint(width // 8 + 1, width // 3 + 2)] = 1.0 + 7.0 * rng.rand()
        outliers = rng.rand(height, width) < 0.02
        depth[outliers] = 1.0 + 49.0 * rng.rand(int(outliers.sum()))
        d = focal_times_baseline / depth
        holes = rng.rand(height, width)
        d[holes < 0.01] = NAN
        d[(holes >= 0.01) & (holes < 0.013)] = INF
        d[(holes >= 0.013) & (holes < 0.016)] = -1.0
        out.append(d)
    return np.stack(out).astype(np.float32)


DISTORTION = (-0.28, 0.07, 1e-3, -5e-4, 0.0)
# (Wt, Ht), focal length in px: the source is 129 x 65 with 0.7 * 129 = 90.3 px.  The smaller target has the same field
# of view on fewer pixels; the larger one has more pixels and a wider field of view, so that the source fills its middle
# (a target that samples the surface more densely than the source has no collisions to speak of: the contested share
# asked for below cannot be met there).
TARGETS = {'smaller': ((97, 61), 0.7 * 97), 'larger': ((161, 81), 0.36 * 161)}
GENERAL_SHAPE = (2, 65, 129)


def general_case(target, seed=0):
    """-> the keyword arguments of register_depth / oracle_registration (numpy) for the rotated rig and a distorted
    third camera rotated by three degrees and moved by a few centimetres against the rectified left frame."""
    batch, height, width = GENERAL_SHAPE
    rig = rotated_rig(width, height)
    (target_width, target_height), focal = TARGETS[target]
    rotation = pds.rectification.rodrigues(np.array([0.5, 0.7, -0.5]) / np.linalg.norm([0.5, 0.7, -0.5]) * np.radians(3.0))
    pose = np.hstack([rotation @ rig.R1.T, [[0.05], [-0.02], [0.01]]])
    rng = np.random.RandomState(100 + seed)
    return dict(disparity=depth_scene(GENERAL_SHAPE, seed, -rig.P2[0, 3]),   # (P2[0, 3] = Tx f)
                matrix=rig.reprojection_matrix('rectified'), pose=pose,
                camera=(focal, 1.01 * focal, 0.5 * target_width - 0.3, 0.5 * target_height + 0.2, 0.05),
                distortion=DISTORTION, size=(target_width, target_height), valid=rng.rand(*GENERAL_SHAPE) > 0.1,
                confidence=rng.rand(*GENERAL_SHAPE).astype(np.float32), min_confidence=0.05)


@pytest.mark.parametrize('splat', [1, 2])
@pytest.mark.parametrize('target', sorted(TARGETS))
def test_the_general_case_is_neither_swallowed_by_its_bands_nor_free_of_occlusion(target, splat):
    case = general_case(target)
    depths = registration.compose(np.hstack([np.eye(3), np.zeros((3, 1))]), case['matrix'])
    d = case['disparity'][np.isfinite(case['disparity']) & (case['disparity'] > 0)]
    z = depths[2, 3] / (depths[3, 2] * d)
    assert 0.99 <= z.min() and z.max() <= 50.01   # the depth range 1 .. 50 m
    oracle = oracle_registration(splat=splat, tau=TAU, **case)
    ambiguous, contested = statistics(oracle)
    print('%s, splat %d: %.2f %% of the pairs ambiguous, %.1f %% of the hit pixels contested, %d kept sources' %
          (target, splat, 100 * ambiguous, 100 * contested, int(oracle.kept.sum())))
    assert ambiguous <= 0.05 and contested >= 0.30
    # and the fp64 winners themselves pass the check they are the yardstick of
    exact = oracle_registration(splat=splat, **case)
    depth, index, valid = winners(exact)
    assert check_registration(depth.astype(np.float32), index, valid, oracle) == int(valid.sum()) > 1000


# ------------------------------------------------------------------------------------------------ the C ABI
def test_register_depth_symbols_declared_exported_and_bound(hip_library):
    header = open(_lib.HEADER_PATH).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('pds_register_depth_workspace_bytes', 'pds_register_depth_fwd'):
        assert name + '(' in header and hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert hip_library.pds_abi_version() == 7
    for name in ('register_depth', 'RegisteredDepth'):
        assert name in pds.__all__, name
    assert pds.RegisteredDepth._fields == ('depth', 'index', 'valid')
    assert pds.register_depth is registration.register_depth
    common = open(_lib.HEADER_PATH.replace('include/pds_hip.h', 'practicaldeepstereo_nips2018_amd/csrc/common.hpp')).read()
    assert 'constexpr int kRegisterDepthTile = %d;' % TILE in common
    # the key buffer: 8 bytes per target pixel, rounded up to 256
    assert hip_library.pds_register_depth_workspace_bytes(1, 1, 1) == 256
    assert hip_library.pds_register_depth_workspace_bytes(1, 4, 8) == 256
    assert hip_library.pds_register_depth_workspace_bytes(1, 3, 11) == 512
    assert hip_library.pds_register_depth_workspace_bytes(4, 720, 1280) == 4 * 720 * 1280 * 8
    # one device function for the point, one for the polynomial: called, not restated
    csrc = _lib.HEADER_PATH.replace('include/pds_hip.h', 'practicaldeepstereo_nips2018_amd/csrc/')
    kernel = open(csrc + 'register_depth.hip').read()
    assert 'reproject_one(a.r, valid, confidence, p, d, h, w)' in kernel and 'distort_point<float>(' in kernel
    assert 'distort_point<double>(' in open(csrc + 'rectification.hip').read()


def test_register_depth_validation_needs_no_gpu(hip_library):
    lib = hip_library
    big = 1 << 24
    d, v, c, dep, idx, hit, ws = [ctypes.c_void_p(big * n) for n in range(1, 8)]   # never dereferenced
    floats = (lambda values: (ctypes.c_float * len(values))(*values))
    identity = floats(np.eye(4, dtype=np.float32).reshape(-1).tolist())
    camera, distortion = floats([4.0, 4.0, 1.0, 0.5, 0.0]), floats([-0.1, 0.01, 0.0, 0.0, 0.0])
    error = lib.pds_last_error

    def call(disparity=d, valid=v, confidence=c, min_confidence=0.0, matrix=identity, camera=camera,
             distortion=distortion, splat=1, fill_value=NAN, depth=dep, index=idx, valid_out=hit, shape=(1, 2, 3),
             target=(3, 5), workspace=ws, workspace_bytes=256):
        return lib.pds_register_depth_fwd(disparity, valid, confidence, min_confidence, matrix, camera, distortion,
                                          splat, fill_value, depth, index, valid_out, *shape, *target, workspace,
                                          workspace_bytes, None)

    for name in ('disparity', 'matrix', 'camera', 'distortion', 'depth', 'workspace'):
        assert call(**{name: None}) != 0 and error() == b'register_depth: null pointer', name
    for shape in [(0, 2, 3), (1, 0, 3), (1, 2, 0), (-1, 2, 3), (1, -2, 3), (1, 2, -3)]:
        assert call(shape=shape) != 0 and b'register_depth: bad shape' in error(), shape
    for target in [(0, 5), (3, 0), (-3, 5), (3, -5)]:
        assert call(target=target) != 0 and b'register_depth: bad target shape' in error(), target
        assert lib.pds_register_depth_workspace_bytes(1, *target) == 0 and b'bad target shape' in error(), target
    assert lib.pds_register_depth_workspace_bytes(0, 3, 5) == 0 and b'bad target shape' in error()
    # h * w, ht * wt and batch * ht * wt >= 2^31 (and batch * h * w: the flat source index is an int as well)
    for shape in [(1, 1 << 16, 1 << 15), (1, 1 << 16, 1 << 16), (4, 1 << 15, 1 << 14)]:
        assert call(shape=shape) != 0 and b'batch * h * w' in error() and b'32-bit indices' in error(), shape
    for batch, target in [(1, (1 << 16, 1 << 15)), (1, (1 << 16, 1 << 16)), (4, (1 << 15, 1 << 14))]:
        assert call(shape=(batch, 2, 3), target=target, workspace_bytes=1 << 40) != 0, target
        assert b'batch * ht * wt' in error() and b'32-bit indices' in error(), target
        assert lib.pds_register_depth_workspace_bytes(batch, *target) == 0 and b'32-bit indices' in error(), target
    assert lib.pds_register_depth_workspace_bytes(1, (1 << 15) - 1, 1 << 16) == ((1 << 31) - (1 << 16)) * 8
    for splat in (0, 3, -1, 4):
        assert call(splat=splat) != 0 and b'splat must be 1 or 2 (got %d)' % splat in error(), splat
    assert call(workspace_bytes=255) != 0 and b'workspace too small (255 < 256)' in error()
    assert call(workspace_bytes=0) != 0 and b'workspace too small' in error()
    assert call(target=(720, 1280), workspace_bytes=7372799) != 0 and b'(7372799 < 7372800)' in error()
    for bad in (NAN, INF, -INF):
        assert call(min_confidence=bad) != 0 and b'min_confidence must be finite' in error(), bad
    assert call(depth=ctypes.c_void_p(dep.value + 2)) != 0 and b'not 4-byte aligned' in error()
    assert call(index=ctypes.c_void_p(idx.value + 1)) != 0 and b'not 4-byte aligned' in error()
    assert call(workspace=ctypes.c_void_p(ws.value + 4)) != 0 and b'workspace is not 8-byte aligned' in error()
    # nothing written may overlap anything read or written (3 x 5 targets: 60 / 60 / 15 / 256 bytes)
    assert call(depth=d) != 0 and b'an output aliases an input' in error()
    assert call(depth=ctypes.c_void_p(d.value + 20)) != 0 and b'an output aliases an input' in error()
    assert call(index=c) != 0 and b'an output aliases an input' in error()
    assert call(valid_out=v) != 0 and b'an output aliases an input' in error()
    assert call(valid_out=ctypes.c_void_p(v.value + 5)) != 0 and b'an output aliases an input' in error()
    assert call(workspace=ctypes.c_void_p(c.value - 248)) != 0 and b'an output aliases an input' in error()
    assert call(index=ctypes.c_void_p(dep.value + 56)) != 0 and b'an output aliases another output' in error()
    assert call(valid_out=ctypes.c_void_p(idx.value + 59)) != 0 and b'an output aliases another output' in error()
    assert call(workspace=ctypes.c_void_p(hit.value + 8)) != 0 and b'an output aliases another output' in error()
    assert call(workspace=ctypes.c_void_p(dep.value - 248)) != 0 and b'an output aliases another output' in error()
    for k in (0, 15):
        for bad in (NAN, INF):
            values = np.eye(4, dtype=np.float32).reshape(-1).tolist()
            values[k] = bad
            assert call(matrix=floats(values)) != 0 and b'non-finite matrix' in error(), (k, bad)
    for k in range(5):
        for bad in (NAN, -INF):
            values = [4.0, 4.0, 1.0, 0.5, 0.0]
            values[k] = bad
            assert call(camera=floats(values)) != 0 and b'non-finite camera or distortion' in error(), (k, bad)
            values = [0.0] * 5
            values[k] = bad
            assert call(distortion=floats(values)) != 0 and b'non-finite camera or distortion' in error(), (k, bad)


# ------------------------------------------------------------------------------------------------ Python
def test_register_depth_python_errors():
    ok, Q = torch.zeros(1, 4, 5), np.eye(4)
    pose, camera, size = IDENTITY, (4.0, 4.0, 2.0, 1.5, 0.0), (5, 4)

    def run(disparity=ok, matrix=Q, pose=pose, camera=camera, distortion=None, size=size, **kw):
        return pds.register_depth(disparity, matrix, pose, camera, distortion, size, **kw)

    with pytest.raises(TypeError, match='disparity must be a torch.Tensor'):
        run(np.zeros((1, 4, 5), dtype=np.float32))
    for bad in (ok.double(), ok.half(), ok.to(torch.int32)):
        with pytest.raises(TypeError, match='disparity must be float32'):
            run(bad)
    for bad in (torch.zeros(4, 5), torch.zeros(1, 1, 4, 5)):
        with pytest.raises(ValueError, match='disparity must have 3 dimensions'):
            run(bad)
    for bad in (np.eye(3), np.zeros((4, 3)), np.full((4, 4), NAN), np.diag([1.0, 1.0, 1.0, INF])):
        with pytest.raises(ValueError, match='matrix must be a finite 4x4'):   # reproject's message
            run(matrix=bad)
    for bad in (np.eye(3), np.eye(4), np.full((3, 4), NAN), np.zeros((4, 3))):
        with pytest.raises(ValueError, match=r'pose must be a finite 3x4 \[R \| t\]'):
            run(pose=bad)
    for bad in ((4.0, 4.0, 2.0, 1.5), (4.0,) * 6, ()):
        with pytest.raises(ValueError, match='camera must hold 5 values'):
            run(camera=bad)
    with pytest.raises(ValueError, match='camera has non-finite entries'):
        run(camera=(4.0, NAN, 2.0, 1.5, 0.0))
    for bad in ((0.0, 4.0, 2.0, 1.5, 0.0), (4.0, -4.0, 2.0, 1.5, 0.0)):
        with pytest.raises(ValueError, match='camera must have positive focal lengths'):
            run(camera=bad)
    for bad in ((0.1, 0.2, 0.3), (0.1,) * 8):
        with pytest.raises(ValueError, match='distortion must hold 4 or 5 values'):
            run(distortion=bad)
    with pytest.raises(ValueError, match='distortion has non-finite entries'):
        run(distortion=(0.1, INF, 0.0, 0.0))
    for bad in (5, (5,), (5, 4, 3), 'ab', None):
        with pytest.raises(ValueError, match=r'size must be \(width, height\)'):
            run(size=bad)
    for bad in ((0, 4), (5, -1)):
        with pytest.raises(ValueError, match=r'size must be at least \(1, 1\)'):
            run(size=bad)
    for bad in (NAN, INF):
        with pytest.raises(ValueError, match='min_confidence must be finite'):
            run(min_confidence=bad)
    for bad in (0, 3, 1.5, True, '2', None):
        with pytest.raises(ValueError, match='splat must be 1 or 2'):
            run(splat=bad)
    for valid in (torch.ones(1, 4, 5), torch.ones(1, 4, 5, dtype=torch.uint8), torch.ones(1, 4, 6, dtype=torch.bool)):
        with pytest.raises(ValueError, match='valid must be torch.bool'):    # reproject's message
            run(valid=valid)
    with pytest.raises(TypeError, match='valid must be a torch.Tensor'):
        run(valid=np.ones((1, 4, 5), dtype=bool))
    with pytest.raises(TypeError, match='confidence must be float32'):
        run(confidence=ok.double())
    with pytest.raises(ValueError, match='confidence .* differ in shape'):
        run(confidence=torch.zeros(1, 5, 4))
    # every argument in order, and still no CPU fallback
    for kwargs in ({}, {'distortion': (-0.1, 0.01, 0.0, 0.0), 'valid': torch.ones(1, 4, 5, dtype=torch.bool),
                        'confidence': ok, 'min_confidence': 0.5, 'splat': 2, 'fill_value': 0.0, 'with_index': False}):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            run(**kwargs)
    parameters = inspect.signature(pds.register_depth).parameters
    assert list(parameters)[:6] == ['disparity', 'matrix', 'pose', 'camera', 'distortion', 'size']
    defaults = [(n, p.default) for n, p in parameters.items()][6:]
    assert defaults[:4] == [('valid', None), ('confidence', None), ('min_confidence', 0.0), ('splat', 1)]
    assert defaults[4][0] == 'fill_value' and math.isnan(defaults[4][1]) and defaults[5] == ('with_index', True)
    for phrase in ('OpenCV\'s\n       projectPoints has no such guard', 'smaller source index', 'fill_holes=True',
                   'no CPU fallback'):
        assert phrase in registration.__doc__, phrase


# ------------------------------------------------------------------------------------------------ the rig's poses
def simple_rig(width, height, distortion=True):
    K = np.array([[0.7 * width, 0.0, 0.5 * width - 0.5], [0.0, 0.7 * width, 0.5 * height - 0.5], [0.0, 0.0, 1.0]])
    D1, D2 = (np.array([-0.05, 0.01, 1e-3, -5e-4]), np.array([-0.04, 0.02, -4e-4, 6e-4])) if distortion else (None, None)
    return pds.StereoRig(K, np.zeros(4) if D1 is None else D1, K, np.zeros(4) if D2 is None else D2, np.eye(3),
                         np.array([-0.12, 0.0, 0.0]), (width, height))


def test_the_rig_builds_the_three_poses():
    parameters = inspect.signature(pds.StereoRig.register_depth).parameters
    assert [(n, p.default) for n, p in parameters.items()][2:] == [
        ('view', 'left'), ('valid', None), ('confidence', None), ('min_confidence', 0.0), ('splat', 1), ('camera', None)]
    assert 'rig.register_depth(r.disparity, \'left\', r.valid)' in pds.StereoRig.register_depth.__doc__

    # simple_rig: no rotation anywhere, so every number can be written down.  f = P1[0, 0], Tx = -0.12
    rig = simple_rig(256, 128)
    f, cx, cy = rig.P1[0, 0], rig.P1[0, 2], rig.P1[1, 2]
    assert np.allclose(rig.R1, np.eye(3), atol=1e-15) and np.isclose(rig.P2[0, 3] / f, -0.12)
    pose, camera, distortion, size = rig.registration_target('left')
    assert np.allclose(pose, IDENTITY, atol=1e-15) and size == (256, 128)
    assert camera.tolist() == [0.7 * 256, 0.7 * 256, 127.5, 63.5, 0.0] and distortion.tolist() == [-0.05, 0.01, 1e-3, -5e-4, 0.0]
    pose, camera, distortion, size = rig.registration_target('right')
    assert np.allclose(pose, np.hstack([np.eye(3), [[-0.12], [0.0], [0.0]]]), atol=1e-15) and size == (256, 128)
    assert distortion.tolist() == [-0.04, 0.02, -4e-4, 6e-4, 0.0]
    # M' of the right view by hand: the rows of Q, the first one moved by Tx * (row 3 of Q): X' = x - cx - 0.12 d / 0.12
    composed = registration.compose(pose, rig.reprojection_matrix('rectified'))
    by_hand = np.array([[1.0, 0.0, -1.0, -cx], [0.0, 1.0, 0.0, -cy], [0.0, 0.0, 0.0, f], [0.0, 0.0, 1.0 / 0.12, 0.0]])
    assert np.allclose(composed, by_hand, rtol=1e-13, atol=1e-13)
    # so a pixel (x, y, d) lands at column x - d of the RECTIFIED right view: (X', Y', Z') / Z' * f + c
    point = composed @ np.array([100.0, 40.0, 7.0, 1.0])
    assert np.allclose(point[:2] / point[2] * f + [cx, cy], [93.0, 40.0])
    # a third camera 5 cm above the left one, turned by 10 degrees about y, with its own lens and size
    K3 = np.array([[300.0, 0.5, 319.5], [0.0, 310.0, 239.5], [0.0, 0.0, 1.0]])
    R3, T3 = pds.rectification.rodrigues([0.0, np.radians(10.0), 0.0]), np.array([0.01, -0.05, 0.002])
    pose, camera, distortion, size = rig.registration_target(camera=(K3, [-0.2, 0.05, 0.0, 0.0, 0.01], R3, T3, (640, 480)))
    c, s = math.cos(np.radians(10.0)), math.sin(np.radians(10.0))
    assert np.allclose(pose, [[c, 0.0, s, 0.01], [0.0, 1.0, 0.0, -0.05], [-s, 0.0, c, 0.002]], atol=1e-15)
    assert camera.tolist() == [300.0, 310.0, 319.5, 239.5, 0.5] and distortion.tolist() == [-0.2, 0.05, 0.0, 0.0, 0.01]
    assert size == (640, 480)

    # the rotated rig: R1, R2 are no identities.  A point of the raw left frame, carried through the rectification and
    # each pose, must come out where the calibration itself puts it
    K = np.array([[90.3, 0.0, 64.0], [0.0, 90.3, 32.0], [0.0, 0.0, 1.0]])
    R = pds.rectification.rodrigues(np.array([0.3, -0.8, 0.5]) / np.linalg.norm([0.3, -0.8, 0.5]) * np.radians(2.0))
    T = np.array([-0.12, 0.004, -0.002])
    rig = pds.StereoRig(K, np.zeros(4), K, np.zeros(4), R, T, (129, 65))
    assert np.abs(rig.R1 - np.eye(3)).max() > 1e-3
    X_left = np.array([0.3, -0.2, 4.0])
    X_rectified = rig.R1 @ X_left
    Q, f = rig.reprojection_matrix('rectified'), rig.P1[0, 0]
    pixel = rig.P1[:, :3] @ X_rectified
    pixel = pixel[:2] / pixel[2]
    disparity = -rig.P2[0, 3] / X_rectified[2]
    source = np.array([pixel[0], pixel[1], disparity, 1.0])
    back = Q @ source
    assert np.allclose(back[:3] / back[3], X_rectified, rtol=1e-12)
    for view, expected in (('left', X_left), ('right', R @ X_left + T)):
        pose, camera, _, size = rig.registration_target(view)
        point = registration.compose(pose, Q) @ source
        assert np.allclose(point[:3] / point[3], expected, rtol=1e-11, atol=1e-13), view
        assert camera.tolist() == [90.3, 90.3, 64.0, 32.0, 0.0] and size == (129, 65)
    assert np.allclose(rig.registration_target('left')[0], np.hstack([rig.R1.T, np.zeros((3, 1))]), atol=0)
    shift = np.array([rig.P2[0, 3] / rig.P2[0, 0], 0.0, 0.0])
    assert np.allclose(rig.registration_target('right')[0], np.hstack([rig.R2.T, (rig.R2.T @ shift)[:, None]]), atol=0)
    pose = rig.registration_target(camera=(K3, None if False else np.zeros(4), R3, T3, (640, 480)))[0]
    point = registration.compose(pose, Q) @ source
    assert np.allclose(point[:3] / point[3], R3 @ X_left + T3, rtol=1e-11, atol=1e-13)
    assert np.allclose(pose, np.hstack([R3 @ rig.R1.T, T3[:, None]]), atol=0)

    # what the rig refuses; and it has no CPU fallback either
    with pytest.raises(ValueError, match="view must be 'left' or 'right'"):
        rig.register_depth(torch.zeros(1, 65, 129), view='up')
    with pytest.raises(ValueError, match="leave view='left'"):
        rig.register_depth(torch.zeros(1, 65, 129), view='right', camera=(K3, np.zeros(4), R3, T3, (640, 480)))
    with pytest.raises(ValueError, match=r'camera must be \(K, D, R, T, size\)'):
        rig.register_depth(torch.zeros(1, 65, 129), camera=(K3, np.zeros(4), R3))
    with pytest.raises(ValueError, match='camera R is not a rotation'):
        rig.register_depth(torch.zeros(1, 65, 129), camera=(K3, np.zeros(4), 2 * R3, T3, (640, 480)))
    with pytest.raises(ValueError, match='camera T must hold 3 finite values'):
        rig.register_depth(torch.zeros(1, 65, 129), camera=(K3, np.zeros(4), R3, [0.0, NAN, 0.0], (640, 480)))
    with pytest.raises(ValueError, match=r'camera size must be'):
        rig.register_depth(torch.zeros(1, 65, 129), camera=(K3, np.zeros(4), R3, T3, (640, 0)))
    with pytest.raises(ValueError, match='splat must be 1 or 2'):
        rig.register_depth(torch.zeros(1, 65, 129), splat=3)
    for kwargs in ({}, {'view': 'right', 'splat': 2}, {'camera': (K3, np.zeros(4), R3, T3, (640, 480))}):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            rig.register_depth(torch.zeros(1, 65, 129), **kwargs)
    # reconstruct and its result are what they were
    assert pds.rectification.Reconstruction._fields == ('left_image', 'right_image', 'disparity', 'valid', 'points')
