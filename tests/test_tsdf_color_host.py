"""CPU: colour in TSDF fusion (pds_tsdf_color_integrate_fwd, pds_tsdf_color_gather_fwd, pds_tsdf_color_render_fwd;
ColorTsdfVolume, ColorRaycast, StereoRig.color_tsdf_volume, StereoRig.integrate_color).  The entry points are declared,
exported and bound and refuse without a GPU what they cannot run, and so does the Python surface.

The numpy fp64 oracles of tests/test_gpu_tsdf_color.py live here, each with a bound per voxel, row or pixel whose derivation
is in its docstring (U = 2^-24, the unit roundoff of float32; none of the constants was tuned on kernel output), and each is
held to answers worked out by hand on a 4 x 4 x 4 volume.  The geometry is that of tests/test_tsdf_host.py and
tests/test_tsdf_raycast_host.py, whose oracles are imported, not copied."""
import collections
import ctypes
import inspect
import itertools

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib, tsdf_color as color_module, tsdf as tsdf_module
from practicaldeepstereo_nips2018_amd import tsdf_raycast as raycast_module
from tests.test_register_depth_host import EPS, TAU, simple_rig
from tests.test_tsdf_host import (GENERAL, IDENTITY, WALL, HostVolume, as_the_kernel_sees, camera_of, f32, fresh_state,
                                  general_case, hand_volume, oracle_extract, oracle_integrate, q_of, wall_volume)
from tests.test_tsdf_raycast_host import (GENERAL_SIZE, RANDOM, RANDOM_DIMS, as_the_kernel_sees as rays_as_the_kernel_sees,
                                          corners_of, fourth_pose, general_camera, general_pose, oracle_raycast,
                                          raycast_random_volume, trilinear)

NAN, INF = float('nan'), float('inf')
U = 2.0 ** -24               # the unit roundoff of float32
SECOND_ORDER = 1.0 + 2.0 ** -20   # (1 + U)^k - 1 <= k U (1 + 2^-20) for the k <= 8 roundings of the chains below

# color [nz, ny, nx, 3] fp64: the state after the frame; bound: its admissible error; pixel [nz, ny, nx] int64: py * W + px
# of the voxel (-1: none); updated, ambiguous, projects: those of the Integration the colours belong to
ColorIntegration = collections.namedtuple('ColorIntegration', ['color', 'bound', 'pixel', 'updated', 'ambiguous', 'projects',
                                                               'geometry'])
Rendered = collections.namedtuple('Rendered', ['colors', 'bound', 'absent', 'undecided', 'position_bound'])


def image_hwc(image):
    """uint8 [H, W, 3] or float32 [3, H, W] (one entry, the two layouts of the entry point) -> fp64 [H, W, 3]."""
    image = np.asarray(image)
    if image.dtype == np.uint8:
        assert image.ndim == 3 and image.shape[2] == 3
        return image.astype(np.float64)
    assert image.dtype == np.float32 and image.ndim == 3 and image.shape[0] == 3
    return image.transpose(1, 2, 0).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the oracles
def oracle_color_integrate(color, tsdf, weight, image, tau=TAU, **case):
    """One frame into the state (color [nz, ny, nx, 3], tsdf, weight: float32 as the GPU held them, or any float) ->
    ColorIntegration.  `case`: the keyword arguments of oracle_integrate, which decides what is updated; where it is,

        color' = (color W_old + x w) / (W_old + w)

    with x the image at the pixel the voxel projects to (the rounding of the oracle's first candidate, du = dv = -tau) and
    w = 1 or the pixel's confidence.  oracle_integrate marks a voxel AMBIGUOUS when the four roundings of (u, v) within tau
    do not agree on the pixel, so its mask covers the choice of the pixel as well: nothing is added to it here.

    The bound, for an input state that is exact in float32 (the test feeds the GPU's own state of before the frame), per
    channel, with m = max(|color|, |x|): the kernel computes fl(fmaf(color, W_old, fl(x w)) / fl(W_old + w)).
        p = x w (1 + e1);  s = (color W_old + p)(1 + e2);  S = (W_old + w)(1 + e3);  q = s / S (1 + e4),  |e| <= U.
    With W_old >= 0 and w > 0, |color W_old + x w| <= m (W_old + w) and |x w| <= m (W_old + w), so the four roundings move
    the quotient by at most U m each: 4 U m to first order -- the issue's starting point, confirmed -- times SECOND_ORDER."""
    color = np.asarray(color, dtype=np.float64)
    o = oracle_integrate(tsdf, weight, **case)
    W_old = np.asarray(weight, dtype=np.float64)
    nz, ny, nx = W_old.shape
    matrix = case['matrix']
    A, b, (fx, fy, cx, cy, skew), _ = as_the_kernel_sees(case['origin'], case['voxel_size'], case.get('pose'),
                                                         camera_of(matrix) if case.get('camera') is None else case['camera'],
                                                         matrix)
    picture = image_hwc(image)
    height, width = picture.shape[:2]
    kk, jj, ii = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float64)
    xc, yc, zc = (A[r, 0] * ii + A[r, 1] * jj + A[r, 2] * kk + b[r] for r in range(3))
    with np.errstate(all='ignore'):
        u = fx * (xc / zc) + skew * (yc / zc) + cx
        v = fy * (yc / zc) + cy
        ok = (zc > 0) & np.isfinite(u) & np.isfinite(v)
        px = np.floor(np.where(ok, np.clip(u, -4.0, width + 4.0), -4.0) + 0.5 - tau).astype(np.int64)
        py = np.floor(np.where(ok, np.clip(v, -4.0, height + 4.0), -4.0) + 0.5 - tau).astype(np.int64)
    inside = ok & (px >= 0) & (px < width) & (py >= 0) & (py < height)
    pixel = np.where(inside, py * width + px, -1)
    assert (pixel[o.updated] >= 0).all()
    x = picture.reshape(-1, 3)[np.clip(pixel, 0, None)]
    w = np.ones(pixel.shape)
    if case.get('weight_by_confidence'):
        w = np.asarray(case['confidence'], dtype=np.float32).astype(np.float64).reshape(-1)[np.clip(pixel, 0, None)]
    with np.errstate(all='ignore'):
        fused = (color * W_old[..., None] + x * w[..., None]) / (W_old + w)[..., None]
    updated = o.updated[..., None]
    bound = np.where(updated, 4.0 * U * SECOND_ORDER * np.maximum(np.abs(color), np.abs(x)), 0.0)
    return ColorIntegration(np.where(updated, fused, color), bound, pixel, o.updated, o.ambiguous, o.projects, o)


def edge_ends(index, edges_per_voxel, dims):
    """index [N] of an extraction -> (v, n): the two voxels of each row's edge, flat."""
    nx, ny, _ = dims
    index = np.asarray(index, dtype=np.int64)
    v, rest = index // edges_per_voxel, index % edges_per_voxel
    d = np.where(edges_per_voxel == 3, 1 << rest, rest + 1)
    return v, v + (d & 1) + ((d >> 1) & 1) * nx + ((d >> 2) & 1) * nx * ny


def oracle_gather(index, edges_per_voxel, tsdf, color):
    """The colours of the rows `index` (3 v + a, or 7 v + (d - 1)) of an extraction from float32 tsdf [nz, ny, nx] and color
    [nz, ny, nx, 3] -> (colors fp64 [N, 3], bound [N, 3]).  colors = c_v + r (c_n - c_v), r = tsdf[v] / (tsdf[v] - tsdf[n]).

    The bound: the kernel computes fmaf(r', fl(c_n - c_v), c_v) with r' = fl(tsdf[v] / fl(tsdf[v] - tsdf[n])) = r (1 + 2 e)
    (a subtraction of two float32 values and a division, one rounding each), fl(c_n - c_v) = (c_n - c_v)(1 + e) and one
    rounding of the result c.  The ends of an extracted edge differ in sign, so 0 <= r <= 1 and the first three move the
    product by at most 3 U |c_n - c_v|; the last by U |c|.  That is U (|c| + 3 |c_n - c_v|): the derivation gives 3 where the
    issue's starting point has 4, and the derived constant is used, times SECOND_ORDER."""
    tsdf, color = np.asarray(tsdf), np.asarray(color)
    assert tsdf.dtype == color.dtype == np.float32 and color.shape == tsdf.shape + (3,)
    nz, ny, nx = tsdf.shape
    v, n = edge_ends(index, edges_per_voxel, (nx, ny, nz))
    value = tsdf.reshape(-1).astype(np.float64)
    flat = color.reshape(-1, 3).astype(np.float64)
    r = value[v] / (value[v] - value[n])
    assert ((r >= 0) & (r <= 1)).all()
    colors = flat[v] + r[:, None] * (flat[n] - flat[v])
    return colors, U * SECOND_ORDER * (np.abs(colors) + 3.0 * np.abs(flat[n] - flat[v]))


def oracle_render(color, weight, origin, voxel_size, camera, size, depth, pose=None, min_weight=1.0, eps=EPS, tau=TAU):
    """The colour of one raycast entry -> Rendered.  color float32 [nz, ny, nx, 3], weight float32 [nz, ny, nx], depth
    float32 [H, W] AS GIVEN to the entry point (the GPU's own raycast in the GPU test), size = (width, height).

    g = o + depth d per pixel, with M, o and the camera rounded once to float32 and the ray of oracle_raycast; the cell
    c_a = clip(floor(g_a), 0, n_a - 2); colors = the trilinear interpolant over its corners; absent (NaN expected) where the
    depth is NaN, a corner of the cell has weight < min_weight, or a dimension is below 2.

    The position bound is that of oracle_raycast for a sample whose parameter is exact (the depth is an input here):
    E_g = |depth| EPS D_a + EPS (|o_a| + |depth d_a|), D_a = sum_m |M_am dir_m|.  A pixel is UNDECIDED when a cell within
    max(E_g, TAU) of g differs from the cell of g in being observed.  The bound of a colour, per channel: the interpolant
    changes along an axis by at most the spread (max - min) of the corners per unit, over every cell within that margin, so
    the position costs spread sum_a E_g_a; the seven lerps fmaf(t, fl(b - a), a), three levels deep, each cost at most
    U (|b - a| + |result|) <= U (spread + max|c|) and pass the errors of the level before on undiminished at most
    (0 <= t <= 1), so the roundings cost 3 U (spread + max|c|), times SECOND_ORDER."""
    color, weight, depth = np.asarray(color), np.asarray(weight), np.asarray(depth)
    assert color.dtype == weight.dtype == depth.dtype == np.float32 and color.shape == weight.shape + (3,)
    nz, ny, nx = weight.shape
    width, height = size
    assert depth.shape == (height, width)
    M, o, _ = rays_as_the_kernel_sees(origin, voxel_size, pose)
    fx, fy, cx, cy, skew = f32(camera)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    y = ((yy - cy) / fy).reshape(-1)
    x = (xx.reshape(-1) - cx - skew * y) / fx
    direction = np.stack([x, y, np.ones_like(x)], axis=1)
    pixels = len(x)
    colors, bound = np.full((pixels, 3), NAN), np.full((pixels, 3), NAN)
    position = np.full((pixels, 3), NAN)
    absent, undecided = np.ones(pixels, dtype=bool), np.zeros(pixels, dtype=bool)
    shape = (height, width)
    dims = np.array([nx, ny, nz])
    s = depth.reshape(-1).astype(np.float64)
    idx = np.nonzero(~np.isnan(s))[0]
    if dims.min() >= 2 and len(idx):
        top = (dims - 1).astype(np.float64)
        d = direction[idx] @ M.T
        eps_d = eps * (np.abs(direction[idx]) @ np.abs(M).T)
        z = s[idx]
        g = o[None, :] + z[:, None] * d
        E_g = np.abs(z)[:, None] * eps_d + eps * (np.abs(o)[None, :] + np.abs(z[:, None] * d))
        margin = np.maximum(E_g, tau)
        observed_voxel = weight >= np.float32(min_weight)
        value = color.astype(np.float64)
        shifts = [(slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
                  for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
        cell_observed = np.logical_and.reduce([observed_voxel[t] for t in shifts])
        cell_max = np.maximum.reduce([value[t] for t in shifts])
        cell_min = np.minimum.reduce([value[t] for t in shifts])
        cell = np.clip(np.floor(g), 0, top - 1).astype(np.int64)
        low = np.clip(np.floor(g - margin), 0, top - 1).astype(np.int64)
        high = np.clip(np.floor(g + margin), 0, top - 1).astype(np.int64)
        seen = cell_observed[cell[:, 2], cell[:, 1], cell[:, 0]]
        spread = (cell_max - cell_min)[cell[:, 2], cell[:, 1], cell[:, 0]]
        largest = np.maximum(np.abs(cell_max), np.abs(cell_min))[cell[:, 2], cell[:, 1], cell[:, 0]]
        differs = np.zeros(len(idx), dtype=bool)
        for pick in itertools.product((0, 1), repeat=3):
            i, j, k = ((high if p else low)[:, a] for a, p in enumerate(pick))
            differs |= cell_observed[k, j, i] != seen
            spread = np.maximum(spread, (cell_max - cell_min)[k, j, i])
            largest = np.maximum(largest, np.maximum(np.abs(cell_max), np.abs(cell_min))[k, j, i])
        f = g - cell
        for c in range(3):
            colors[idx, c] = trilinear(corners_of(value[..., c], cell), f)
        colors[idx[~seen]] = NAN
        bound[idx] = spread * E_g.sum(axis=1)[:, None] + 3.0 * U * SECOND_ORDER * (spread + largest)
        absent[idx] = ~seen
        undecided[idx] = differs
        position[idx] = E_g
    return Rendered(colors.reshape(shape + (3,)), bound.reshape(shape + (3,)), absent.reshape(shape),
                    undecided.reshape(shape), position.reshape(shape + (3,)))


def check_render(got, oracle, case=''):
    """got float32 [H, W, 3] against Rendered -> (pixels compared, the largest share of the bound).  A row is NaN as a whole;
    at decided pixels it is NaN exactly where the oracle's is, and the others lie within their bound."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == oracle.colors.shape, case
    missing = np.isnan(got).any(axis=2)
    assert np.array_equal(np.isnan(got).all(axis=2), missing), case
    sure = ~oracle.undecided
    assert np.array_equal(missing[sure], oracle.absent[sure]), (case, np.argwhere(sure & (missing != oracle.absent))[:5].tolist())
    compared = sure & ~oracle.absent
    error = np.abs(got.astype(np.float64) - oracle.colors)[compared]
    share = error / oracle.bound[compared]
    assert (error <= oracle.bound[compared]).all(), (case, float(share.max()))
    return int(compared.sum()), float(share.max(initial=0.0))


# ------------------------------------------------------------------------------------------------ by hand, 4 x 4 x 4
def test_oracle_color_integrate_4x4x4_by_hand():
    # the wall of tests/test_tsdf_host.py: layers 0, 1, 2 are updated (t = 1, 0.25, -0.75), layer 3 is skipped
    dims = (4, 4, 4)
    origin, Q = wall_volume(dims)
    d = np.full((WALL['height'], WALL['width']), WALL['disparity'], dtype=np.float32)
    case = dict(disparity=d, matrix=Q, origin=origin, voxel_size=WALL['voxel_size'], truncation=WALL['truncation'])
    picture = np.zeros((WALL['height'], WALL['width'], 3), dtype=np.uint8)
    picture[...] = (100, 20, 255)
    tsdf, weight = fresh_state(dims)
    first = oracle_color_integrate(np.zeros((4, 4, 4, 3)), tsdf, weight, picture, **case)
    assert not first.ambiguous.any() and first.updated[:3].all() and not first.updated[3].any()
    assert (first.color[:3] == (100.0, 20.0, 255.0)).all() and (first.color[3] == 0.0).all()
    assert (first.bound[3] == 0.0).all() and np.allclose(first.bound[0, 0, 0], 4 * U * np.array([100.0, 20.0, 255.0]), rtol=1e-5)
    # a second frame of another colour on weight 1: the mean; in the other layout
    other = np.stack([np.full(d.shape, v, dtype=np.float32) for v in (50.0, 40.0, 5.0)])
    state = (first.geometry.tsdf, first.geometry.weight)
    second = oracle_color_integrate(first.color, *state, other, **case)
    assert (second.color[:3] == (75.0, 30.0, 130.0)).all() and (second.color[3] == 0.0).all()
    # the confidence as the weight: W_old = 1, w = 1/2: (100 + 40 / 2) / 1.5 = 80
    half = dict(case, confidence=np.full(d.shape, 0.5, dtype=np.float32), weight_by_confidence=True)
    third = oracle_color_integrate(first.color, *state, np.stack([np.full(d.shape, 40.0, dtype=np.float32)] * 3), **half)
    assert np.allclose(third.color[:3, :, :, 0], 80.0, rtol=0, atol=1e-12) and (third.geometry.weight[:3] == 1.5).all()
    # an image that names its pixel: voxel (i, j) of every layer k reads the pixel its centre projects to, by hand
    # u = 74 x / z + 31.5 with x = origin_x + (i + 1/2) / 8: layer 0 (z = 1), voxel i = 3: x = 0.203125 -> u = 46.53 -> 47
    yy, xx = np.mgrid[0:WALL['height'], 0:WALL['width']]
    named = np.stack([3.0 * xx + yy, xx, yy]).astype(np.float32)
    fourth = oracle_color_integrate(np.zeros((4, 4, 4, 3)), tsdf, weight, named, **case)
    assert fourth.pixel[0, 0, 3] % WALL['width'] == 47 and fourth.color[0, 0, 3, 1] == 47.0
    px, py = fourth.pixel[:3] % WALL['width'], fourth.pixel[:3] // WALL['width']
    assert np.array_equal(fourth.color[:3, :, :, 0], 3.0 * px + py) and (fourth.pixel[3] >= 0).all()


def colour_of_position(dims):
    """color[k, j, i] = (i, 10 j, 100 k): linear, so every interpolant of it is exact and known."""
    nx, ny, nz = dims
    kk, jj, ii = np.mgrid[0:nz, 0:ny, 0:nx]
    return np.stack([ii, 10 * jj, 100 * kk], axis=3).astype(np.float32)


def test_oracle_gather_4x4x4_by_hand():
    tsdf, weight = hand_volume()   # 0.25 for i <= 1, -0.75 for i >= 2; (0, 2, 0) and (0, 3, 0) are -0.25
    color = colour_of_position((4, 4, 4))
    v = (lambda i, j, k: (k * 4 + j) * 4 + i)
    surface = oracle_extract(tsdf, weight, (1.0, 2.0, 3.0), 0.5)
    colors, bound = oracle_gather(surface.index, 3, tsdf, color)
    rows = {int(index): row for row, index in enumerate(surface.index)}
    # the plane a quarter of the way from i = 1 to i = 2
    assert colors[rows[3 * v(1, 2, 3)]].tolist() == [1.25, 20.0, 300.0]
    # along +y from (0, 1, 0) to (0, 2, 0), r = 0.5; along +z from (0, 3, 0), r = -0.25 / (-0.25 - 0.25) = 0.5
    assert colors[rows[3 * v(0, 1, 0) + 1]].tolist() == [0.0, 15.0, 0.0]
    assert colors[rows[3 * v(0, 3, 0) + 2]].tolist() == [0.0, 30.0, 50.0]
    assert bound[rows[3 * v(1, 2, 3)]].tolist() == [U * SECOND_ORDER * (1.25 + 3.0), U * SECOND_ORDER * 20.0,
                                                    U * SECOND_ORDER * 300.0]
    # stride 7: the face diagonal d = 3 from (1, 0, 0) to (2, 1, 0), r = 0.25, and the axis edge d = 1 of the same voxel
    colors, _ = oracle_gather(np.array([7 * v(1, 0, 0) + 2, 7 * v(1, 0, 0)]), 7, tsdf, color)
    assert colors.tolist() == [[1.25, 2.5, 0.0], [1.25, 0.0, 0.0]]
    ends = edge_ends(np.array([7 * v(1, 0, 0) + 6, 3 * v(1, 0, 0) + 2]), np.array([7, 3]), (4, 4, 4))
    assert ends[1].tolist() == [v(2, 1, 1), v(1, 0, 1)]


def test_oracle_render_4x4x4_by_hand():
    # voxels of 1/2 m from (-1, -1, 0.75): o = -origin / 0.5 - 0.5 = (1.5, 1.5, -2), M = 2 I.  fx = fy = 4, cx = cy = 0
    color, weight = colour_of_position((4, 4, 4)), np.ones((4, 4, 4), dtype=np.float32)
    geometry = dict(origin=(-1.0, -1.0, 0.75), voxel_size=0.5, camera=(4.0, 4.0, 0.0, 0.0, 0.0), size=(2, 2))
    depth = np.array([[1.75, 1.75], [NAN, 1.5]], dtype=np.float32)
    r = oracle_render(color, weight, depth=depth, **geometry)
    # pixel (0, 0): dir = (0, 0, 1), g = (1.5, 1.5, -2 + 3.5);  pixel (1, 0): dir = (1/4, 0, 1), g_x = 1.5 + 2 * 1.75 / 4
    assert r.colors[0, 0].tolist() == [1.5, 15.0, 150.0] and r.colors[0, 1].tolist() == [2.375, 15.0, 150.0]
    # pixel (1, 1) at depth 1.5: g = (2.25, 2.25, 1);  a NaN depth has no colour
    assert r.colors[1, 1].tolist() == [2.25, 22.5, 100.0] and np.isnan(r.colors[1, 0]).all()
    assert r.absent.tolist() == [[False, False], [True, False]] and not r.undecided.any()
    # the bound: spread (1, 10, 100) times sum E_g, plus 3 U (spread + the largest corner)
    E_g = r.position_bound[0, 0]
    assert np.allclose(E_g, EPS * (np.array([1.5, 1.5, 2.0]) + np.array([0.0, 0.0, 3.5]) + 1.75 * np.array([0.0, 0.0, 2.0])))
    assert np.allclose(r.bound[0, 0], np.array([1.0, 10.0, 100.0]) * E_g.sum() +
                       3 * U * (np.array([1.0, 10.0, 100.0]) + np.array([2.0, 20.0, 200.0])), rtol=1e-5)
    # an unobserved corner (i, j, k) = (1, 1, 2) of the cell (1, 1, 1) .. (2, 2, 2): no colour at pixel (0, 0); pixel (1, 0)
    # sits in cell (2, 1, 1) and (1, 1) in cell (2, 2, 1), on the face k = 1 whose lower cell (2, 2, 0) is observed too
    holed = weight.copy()
    holed[2, 1, 1] = 0.5
    r = oracle_render(color, holed, depth=depth, **geometry)
    assert r.absent.tolist() == [[True, False], [True, False]] and not np.isnan(r.colors[1, 1]).any()
    assert r.undecided.tolist() == [[False, False], [False, False]]
    # min_weight below it brings the colour back; a hole next to the face the position lies on makes the pixel undecided
    assert not oracle_render(color, holed, depth=depth, min_weight=0.5, **geometry).absent[0, 0]
    holed = weight.copy()
    holed[0, 2, 2] = 0.0
    assert oracle_render(color, holed, depth=depth, **geometry).undecided.tolist() == [[False, False], [False, True]]
    # check_render takes the answer and refuses a wrong colour, a missing one and one too many
    good = oracle_render(color, weight, depth=depth, **geometry)
    answer = good.colors.astype(np.float32)
    assert check_render(answer, good)[0] == 3
    for at, value in (((0, 0, 1), 15.01), ((0, 0, 1), NAN), ((1, 0, 0), 1.0)):
        bad = answer.copy()
        bad[at] = value
        if np.isnan(value):
            bad[at[:2]] = NAN
        with pytest.raises(AssertionError):
            check_render(bad, good)
    # a volume without cells has no colour
    flat = oracle_render(color[:1], weight[:1], depth=depth, **geometry)
    assert flat.absent.all() and np.isnan(flat.colors).all()


# ------------------------------------------------------------------------------------------------ the scenes of the GPU file
def random_image(seed, layout):
    rng = np.random.RandomState(seed)
    picture = rng.randint(0, 256, (GENERAL['height'], GENERAL['width'], 3)).astype(np.uint8)
    return picture if layout == 1 else np.ascontiguousarray(picture.transpose(2, 0, 1)).astype(np.float32)


def random_colors(dims, seed):
    nx, ny, nz = dims
    return np.random.RandomState(seed).uniform(0.0, 255.0, (nz, ny, nx, 3)).astype(np.float32)


RENDER_CASES = ((1.0, 1.0), (0.375, 0.97))   # (min_weight, observed): a fully observed volume and a partly observed one


def render_scene(min_weight, observed):
    tsdf, weight = raycast_random_volume(RANDOM_DIMS, sum(RANDOM_DIMS), min_weight, observed)
    return tsdf, weight, random_colors(RANDOM_DIMS, 17)


def holed_weight():
    return raycast_random_volume(RANDOM_DIMS, sum(RANDOM_DIMS) + 1, 1.0, 0.6)[1]


def render_oracle(color, weight, depth, pose, min_weight):
    return oracle_render(color, weight, RANDOM['origin'], RANDOM['voxel_size'], general_camera(), GENERAL_SIZE, depth,
                         pose=pose, min_weight=min_weight)


def test_the_scenes_keep_within_the_cap_on_the_oracle_alone():
    # integration: the voxels left out (the ambiguous ones of oracle_integrate, which cover the choice of the pixel) are at
    # most 5 % of the projecting voxels, and more than 8000 are kept
    state = fresh_state(GENERAL['dims'], np.float32)
    o = oracle_color_integrate(np.zeros(state[0].shape + (3,), dtype=np.float32), *state, random_image(0, 1), **general_case())
    left_out = float((o.ambiguous & o.projects).sum()) / float(o.projects.sum())
    print('integration: %.2f %% of the projecting voxels left out, %d kept' % (100 * left_out, int(o.updated.sum())))
    assert left_out <= 0.05 and int(o.updated.sum()) > 8000
    # the render: on the oracle's own depth the undecided pixels are at most 5 % of those with a depth
    for min_weight, observed in RENDER_CASES:
        tsdf, weight, color = render_scene(min_weight, observed)
        for pose in (fourth_pose(), general_pose(0)):
            rays = oracle_raycast(tsdf, weight, RANDOM['origin'], RANDOM['voxel_size'], general_camera(), GENERAL_SIZE,
                                  pose=pose, min_weight=min_weight, truncation=RANDOM['truncation'])
            depth = rays.depth.astype(np.float32)
            r = render_oracle(color, weight, depth, pose, min_weight)
            has = ~np.isnan(depth)
            share = float(r.undecided[has].mean())
            print('render %g: %d pixels with a depth, %.2f %% undecided, %d with a colour' %
                  (observed, int(has.sum()), 100 * share, int((has & ~r.absent).sum())))
            assert has.sum() > 500 and share <= 0.05 and (has & ~r.absent & ~r.undecided).sum() > 400
            assert check_render(r.colors.astype(np.float32), r)[1] <= 1.0   # (the fp64 answer, rounded once, passes)
            if observed == 1.0:
                assert not r.absent[has].any() and not r.undecided.any()
                # A hit lies between two observed samples, so its cell is nearly always observed and the rule that
                # withholds a colour would go untested: the depth of the fully observed volume is also rendered against
                # the weights of a volume observed in 60 % of its blocks of 4 x 4 x 4 (HOLED), as the entry point allows
                holed = render_oracle(color, holed_weight(), depth, pose, 1.0)
                share = float(holed.undecided[has].mean())
                print('render, holed: %.2f %% undecided, %d without a colour, %d with one' %
                      (100 * share, int((has & holed.absent).sum()), int((has & ~holed.absent).sum())))
                assert share <= 0.05 and (has & holed.absent & ~holed.undecided).sum() > 400
                assert (has & ~holed.absent & ~holed.undecided).sum() > 200


# ------------------------------------------------------------------------------------------------ the C ABI
NAMES = ('pds_tsdf_color_integrate_fwd', 'pds_tsdf_color_gather_fwd', 'pds_tsdf_color_render_fwd')


def test_color_symbols_declared_exported_and_bound(hip_library):
    header = open(_lib.HEADER_PATH).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name + '(' in header and hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert hip_library.pds_abi_version() == 7 and '#define PDS_ABI_VERSION 7' in header and _lib.ABI_VERSION == 7
    assert 'TSDF colour' in header and header.count('Additive: ABI version unchanged') >= 12
    assert len(_lib.SIGNATURES) == 83
    assert 'tsdf_color.hip' in [s.rsplit('/', 1)[-1] for s in _lib.sources()]
    VP, I, F, LL, SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong, ctypes.c_size_t
    assert _lib.SIGNATURES[NAMES[0]] == (I, [VP, VP, VP, F, I, VP, I, VP, VP, VP, F, F, VP, VP, VP, I, I, I, I, I, I, VP, SZ, VP])
    assert _lib.SIGNATURES[NAMES[1]] == (I, [VP, VP, I, VP, VP, VP, LL, I, I, I, VP])
    assert _lib.SIGNATURES[NAMES[2]] == (I, [VP, VP, I, I, I, VP, VP, F, VP, VP, I, I, I, VP])
    for name in ('ColorTsdfVolume', 'ColorRaycast'):
        assert name in pds.__all__ and getattr(pds, name) is getattr(color_module, name), name
    assert pds.ColorRaycast._fields == ('depth', 'normals', 'colors') and issubclass(pds.ColorTsdfVolume, pds.TsdfVolume)
    # the parent's products keep their fields
    assert pds.Raycast._fields == ('depth', 'normals') and pds.SurfacePoints._fields == ('cloud', 'normals')
    csrc = _lib.HEADER_PATH.replace('include/pds_hip.h', 'practicaldeepstereo_nips2018_amd/csrc/')
    source = open(csrc + 'tsdf_color.hip').read()
    for probe in ('"tsdf_color_integrate"', '"tsdf_color_gather"', '"tsdf_color_render"'):
        assert 'launch_probed(' + probe in source, probe
    # the shared device functions live in headers and are called from both sides
    for name, header_name, users in (('tsdf_sample', 'tsdf_surface.hpp', ('tsdf.hip', 'tsdf_color.hip')),
                                     ('raycast_cell', 'tsdf_ray.hpp', ('tsdf_raycast.hip', 'tsdf_color.hip'))):
        shared = open(csrc + header_name).read()
        assert shared.count('bool %s(' % name) + shared.count('int %s(' % name) == 1, name
        for user in users:
            text = open(csrc + user).read()
            assert name + '(' in text or name + '<' in text, (name, user)
            assert '__forceinline__ bool %s(' % name not in text and '__forceinline__ int %s(' % name not in text, (name, user)


def test_color_validation_needs_no_gpu(hip_library):
    lib = hip_library
    big = 1 << 24
    d, v, c, t, w, ws, col, img, idx, off, out, dep = [ctypes.c_void_p(big * n) for n in range(1, 13)]   # never dereferenced
    floats = (lambda values: (ctypes.c_float * len(values))(*values))
    identity = floats(np.eye(4, dtype=np.float32).reshape(-1).tolist())
    rows = floats([0.1, 0, 0, 0, 0.1, 0, 0, 0, 0.1, 0, 0, 1.0])
    camera = floats([4.0, 4.0, 1.0, 0.5, 0.0])
    error = lib.pds_last_error

    def integrate(disparity=d, valid=v, confidence=c, min_confidence=0.0, by_confidence=0, image=img, layout=1,
                  matrix=identity, transforms=rows, camera=camera, truncation=0.1, max_weight=64.0, tsdf=t, weight=w,
                  color=col, dims=(4, 3, 2), shape=(1, 2, 3), workspace=ws, workspace_bytes=512):
        return lib.pds_tsdf_color_integrate_fwd(disparity, valid, confidence, min_confidence, by_confidence, image, layout,
                                                matrix, transforms, camera, truncation, max_weight, tsdf, weight, color,
                                                *dims, *shape, workspace, workspace_bytes, None)

    for name in ('disparity', 'image', 'matrix', 'transforms', 'camera', 'tsdf', 'weight', 'color', 'workspace'):
        assert integrate(**{name: None}) != 0 and error() == b'tsdf_color_integrate: null pointer', name
    for shape in [(0, 2, 3), (-1, 2, 3)]:
        assert integrate(shape=shape) != 0 and b'tsdf_color_integrate: bad batch' in error(), shape
    for shape in [(1, 0, 3), (1, 2, 0), (1, -2, 3)]:
        assert integrate(shape=shape) != 0 and b'tsdf_color_integrate: bad shape' in error(), shape
    assert integrate(shape=(1, 1 << 16, 1 << 15)) != 0 and b'h * w' in error() and b'32-bit indices' in error()
    assert integrate(shape=(1 << 12, 1 << 10, 1 << 10), workspace_bytes=1 << 40) != 0 and b'batch * h * w' in error()
    for dims in [(0, 3, 2), (4, 3, -1)]:
        assert integrate(dims=dims) != 0 and b'tsdf: bad volume' in error(), dims
    assert integrate(dims=((1 << 24) + 1, 1, 1)) != 0 and b'tsdf: a dimension above 2^24' in error()
    assert integrate(dims=(895, 895, 895)) != 0 and b'3 * nx * ny * nz does not fit' in error()
    for layout in (-1, 2, 7):
        assert integrate(layout=layout) != 0 and b'image_layout must be 0' in error(), layout
    assert integrate(workspace_bytes=511) != 0 and b'workspace too small (511 < 512)' in error()
    assert integrate(by_confidence=1, confidence=None) != 0 and b'weight_by_confidence without a confidence' in error()
    for bad in (NAN, INF, -INF):
        assert integrate(min_confidence=bad) != 0 and b'min_confidence must be finite' in error(), bad
    for bad in (0.0, -0.1, NAN, INF):
        assert integrate(truncation=bad) != 0 and b'truncation must be positive and finite' in error(), bad
    for bad in (0.0, -1.0, NAN):
        assert integrate(max_weight=bad) != 0 and b'max_weight must be positive' in error(), bad
    assert integrate(color=ctypes.c_void_p(col.value + 2)) != 0 and b'not 4-byte aligned' in error()
    assert integrate(layout=0, image=ctypes.c_void_p(img.value + 1)) != 0 and b'not 4-byte aligned' in error()
    assert integrate(layout=1, image=ctypes.c_void_p(img.value + 1)) != 0 and b'aligned' not in error()   # (bytes)
    assert integrate(workspace=ctypes.c_void_p(ws.value + 4)) != 0 and b'workspace is not 16-byte aligned' in error()
    # nothing written may overlap anything (4 x 3 x 2 voxels: 96 bytes, colour 288; 2 x 3 pixels: image 18 or 72 bytes)
    assert integrate(color=d) != 0 and b'aliases an input' in error()
    assert integrate(color=ctypes.c_void_p(img.value + 17)) != 0 and b'not 4-byte aligned' in error()
    assert integrate(color=ctypes.c_void_p(img.value + 16)) != 0 and b'aliases an input' in error()
    assert integrate(layout=0, color=ctypes.c_void_p(img.value + 68)) != 0 and b'aliases an input' in error()
    assert integrate(tsdf=img) != 0 and b'aliases an input' in error()
    assert integrate(color=t) != 0 and b'alias one another' in error()
    assert integrate(weight=ctypes.c_void_p(col.value + 284)) != 0 and b'alias one another' in error()
    assert integrate(workspace=ctypes.c_void_p(col.value + 272)) != 0 and b'alias one another' in error()
    for k, name, base in ((0, 'matrix', np.eye(4).reshape(-1).tolist()), (11, 'transforms', list(rows)),
                          (4, 'camera', list(camera))):
        for bad in (NAN, INF):
            values = list(base)
            values[k] = bad
            assert integrate(**{name: floats(values)}) != 0, (name, bad)
            assert b'tsdf_color_integrate: non-finite ' + name.rstrip('s').encode() in error(), (name, bad, error())

    def gather(index=idx, offsets=off, edges=3, tsdf=t, color=col, colors=out, capacity=10, dims=(4, 3, 2)):
        return lib.pds_tsdf_color_gather_fwd(index, offsets, edges, tsdf, color, colors, capacity, *dims, None)

    for name in ('index', 'offsets', 'tsdf', 'color', 'colors'):
        assert gather(**{name: None}) != 0 and error() == b'tsdf_color_gather: null pointer', name
    assert gather(dims=(4, 0, 2)) != 0 and b'tsdf: bad volume' in error()
    for edges in (0, 1, 4, 6, 8, -3):
        assert gather(edges=edges) != 0 and b'edges_per_voxel must be 3 (extract) or 7 (mesh)' in error(), edges
    # 7 * nx * ny * nz must fit: 674^3 * 7 = 2 143 288 168 does, 675^3 * 7 does not (3 * 675^3 does)
    assert gather(edges=7, dims=(675, 675, 675)) != 0 and b'7 * nx * ny * nz does not fit' in error()
    assert gather(dims=(895, 895, 895)) != 0 and b'does not fit' in error()
    assert gather(capacity=-1) != 0 and b'capacity must be >= 0 (got -1)' in error()
    assert gather(colors=ctypes.c_void_p(out.value + 2)) != 0 and b'not 4-byte aligned' in error()
    assert gather(index=ctypes.c_void_p(idx.value + 1)) != 0 and b'not 4-byte aligned' in error()
    assert gather(colors=t) != 0 and b'the output aliases an input' in error()
    assert gather(colors=ctypes.c_void_p(col.value + 284)) != 0 and b'the output aliases an input' in error()
    assert gather(colors=ctypes.c_void_p(idx.value + 36)) != 0 and b'the output aliases an input' in error()
    assert gather(colors=ctypes.c_void_p(off.value + 4)) != 0 and b'the output aliases an input' in error()

    ray = floats([10.0, 0, 0, 0, 10.0, 0, 0, 0, 10.0, 1.0, 1.0, -5.0])

    def render(weight=w, color=col, dims=(4, 3, 2), rays=ray, camera=camera, min_weight=1.0, depth=dep, colors=out,
               shape=(1, 2, 3)):
        return lib.pds_tsdf_color_render_fwd(weight, color, *dims, rays, camera, min_weight, depth, colors, *shape, None)

    for name in ('weight', 'color', 'rays', 'camera', 'depth', 'colors'):
        assert render(**{name: None}) != 0 and error() == b'tsdf_color_render: null pointer', name
    assert render(dims=(4, 3, 0)) != 0 and b'tsdf: bad volume' in error()
    assert render(dims=(895, 895, 895)) != 0 and b'does not fit' in error()
    for shape in [(0, 2, 3), (-1, 2, 3)]:
        assert render(shape=shape) != 0 and b'tsdf_color_render: bad batch' in error(), shape
    for shape in [(1, 0, 3), (1, 2, -3)]:
        assert render(shape=shape) != 0 and b'tsdf_color_render: bad shape' in error(), shape
    assert render(shape=(1 << 12, 1 << 10, 1 << 10)) != 0 and b'batch * h * w' in error()
    assert render(min_weight=NAN) != 0 and b'min_weight is NaN' in error()
    for k, bad in ((0, NAN), (4, INF)):
        values = list(camera)
        values[k] = bad
        assert render(camera=floats(values)) != 0 and b'non-finite camera' in error(), (k, bad)
    for k in (0, 1):
        values = list(camera)
        values[k] = 0.0
        assert render(camera=floats(values)) != 0 and b'focal lengths must be positive' in error(), k
    values = list(ray)
    values[9] = NAN
    assert render(rays=floats(values)) != 0 and b'non-finite ray' in error()
    assert render(colors=ctypes.c_void_p(out.value + 2)) != 0 and b'not 4-byte aligned' in error()
    assert render(depth=ctypes.c_void_p(dep.value + 3)) != 0 and b'not 4-byte aligned' in error()
    assert render(colors=w) != 0 and b'the output aliases an input' in error()
    assert render(colors=ctypes.c_void_p(col.value + 284)) != 0 and b'the output aliases an input' in error()
    assert render(colors=ctypes.c_void_p(dep.value + 20)) != 0 and b'the output aliases an input' in error()


# ------------------------------------------------------------------------------------------------ Python
class HostColorVolume(pds.ColorTsdfVolume):
    """The HostVolume of tests/test_tsdf_host.py with a colour: the argument checks run up to the point where they ask
    where the tensors live."""

    def __init__(self, *args, **kw):
        try:
            super(HostColorVolume, self).__init__(*args, device='cpu', **kw)
        except RuntimeError as e:
            assert 'no CPU fallback' in str(e)
        self._tsdf, self._weight = torch.ones(self.shape), torch.zeros(self.shape)
        self._color = torch.zeros(self.shape + (3,))


def test_color_volume_python_errors_and_signatures():
    defaults = (lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()])
    assert defaults(pds.ColorTsdfVolume.__init__) == defaults(pds.TsdfVolume.__init__)
    assert defaults(pds.ColorTsdfVolume.integrate) == defaults(pds.TsdfVolume.integrate) + [('image', None)]
    assert defaults(pds.ColorTsdfVolume.extract_points) == defaults(pds.TsdfVolume.extract_points) + [('with_colors', True)]
    assert defaults(pds.ColorTsdfVolume.extract_mesh) == defaults(pds.TsdfVolume.extract_mesh) + [('with_colors', True)]
    assert defaults(pds.ColorTsdfVolume.raycast) == defaults(pds.TsdfVolume.raycast) + [('with_colors', True)]
    assert defaults(pds.StereoRig.color_tsdf_volume) == defaults(pds.StereoRig.tsdf_volume)
    assert [n for n, _ in defaults(pds.StereoRig.integrate_color)][:4] == ['self', 'volume', 'disparity', 'image']
    assert defaults(pds.StereoRig.integrate_color)[4:] == defaults(pds.StereoRig.integrate)[3:]
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pds.ColorTsdfVolume((0.0, 0.0, 0.0), 0.1, (4, 3, 2), 0.3, device='cpu')
    with pytest.raises(ValueError, match='dims must be at least'):
        pds.ColorTsdfVolume((0.0, 0.0, 0.0), 0.1, (4, 0, 2), 0.3, device='cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        simple_rig(64, 48).color_tsdf_volume((0.0, 0.0, 0.0), 0.1, (4, 3, 2), 0.3, device='cpu')
    volume = HostColorVolume((0.0, 0.0, 0.0), 0.1, (4, 3, 2), 0.3)
    assert volume.color.shape == (2, 3, 4, 3) and volume.color.dtype == torch.float32 and float(volume.color.abs().max()) == 0
    ok, Q = torch.zeros(1, 4, 5), q_of(4, 5, 4.0, 0.5)
    bytes_image, float_image = torch.zeros(1, 4, 5, 3, dtype=torch.uint8), torch.zeros(1, 3, 4, 5)
    # every frame carries its image
    with pytest.raises(ValueError, match='needs the image of every frame'):
        volume.integrate(ok, Q)
    with pytest.raises(TypeError, match='image must be a torch.Tensor'):
        volume.integrate(ok, Q, image=np.zeros((1, 4, 5, 3), dtype=np.uint8))
    with pytest.raises(TypeError, match=r'image must be uint8 \[B, H, W, 3\] or float32 \[B, 3, H, W\]'):
        volume.integrate(ok, Q, image=float_image.double())
    for bad in (torch.zeros(1, 3, 4, 5, dtype=torch.uint8), torch.zeros(4, 5, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r'a uint8 image must be \[B, H, W, 3\]'):
            volume.integrate(ok, Q, image=bad)
    for bad in (torch.zeros(1, 4, 5, 3), torch.zeros(3, 4, 5)):
        with pytest.raises(ValueError, match=r'a float32 image must be \[B, 3, H, W\]'):
            volume.integrate(ok, Q, image=bad)
    for bad in (torch.zeros(2, 4, 5, 3, dtype=torch.uint8), torch.zeros(1, 3, 5, 4)):
        with pytest.raises(ValueError, match='does not match disparity'):
            volume.integrate(ok, Q, image=bad)
    # the parent's checks hold, and come first
    with pytest.raises(TypeError, match='disparity must be float32'):
        volume.integrate(ok.double(), Q, image=bytes_image)
    with pytest.raises(ValueError, match='weight_by_confidence needs a confidence'):
        volume.integrate(ok, Q, image=torch.zeros(9), weight_by_confidence=True)
    for image in (bytes_image, float_image):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            volume.integrate(ok, Q, image=image)
    rig = simple_rig(64, 48)
    with pytest.raises(TypeError, match='volume must be a ColorTsdfVolume'):
        rig.integrate_color(HostVolume((0.0, 0.0, 0.0), 0.1, (4, 3, 2), 0.3), torch.zeros(1, 48, 64),
                            torch.zeros(1, 48, 64, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match='needs the image of every frame'):
        rig.integrate_color(volume, torch.zeros(1, 48, 64), None)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rig.integrate_color(volume, torch.zeros(1, 48, 64), torch.zeros(1, 48, 64, 3, dtype=torch.uint8), pose=IDENTITY)
    with pytest.raises(ValueError, match='needs the image of every frame'):   # (the plain method of the rig has no image)
        rig.integrate(volume, torch.zeros(1, 48, 64))
    # the state: settable with the same shape, dtype and device only
    volume.color = torch.full((2, 3, 4, 3), 7.0)
    assert float(volume.color[1, 2, 3, 2]) == 7.0
    with pytest.raises(TypeError, match='color must be a torch.Tensor'):
        volume.color = np.zeros((2, 3, 4, 3), dtype=np.float32)
    for bad in (torch.zeros(2, 3, 4), torch.zeros(3, 2, 3, 4), torch.zeros(2, 3, 4, 3, dtype=torch.float64)):
        with pytest.raises(ValueError, match=r'color must be float32 \(2, 3, 4, 3\)'):
            volume.color = bad
    with pytest.raises(ValueError, match='color must be contiguous'):
        volume.color = torch.zeros(2, 3, 4, 6)[..., ::2]
    # extraction and raycast: the parent's refusals, then no CPU fallback
    with pytest.raises(ValueError, match='min_weight is NaN'):
        volume.extract_points(min_weight=NAN)
    with pytest.raises(ValueError, match='capacity must be >= 0'):
        volume.extract_mesh(capacity=-1)
    with pytest.raises(ValueError, match='camera must hold 5 values'):
        volume.raycast((4.0, 4.0), (5, 4))
    for run in (volume.extract_points, volume.extract_mesh, lambda: volume.raycast((4.0, 4.0, 2.0, 1.5, 0.0), (5, 4))):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            run()
    # the module texts point here, and colour is no longer out of scope of the package
    assert 'tsdf_color.py' in tsdf_module.__doc__ and 'tsdf_color.py' in raycast_module.__doc__
    for phrase in ('pds_tsdf_color_integrate_fwd', 'pds_tsdf_color_gather_fwd', 'pds_tsdf_color_render_fwd',
                   'fmaf(color, W_old, x * w) / (W_old + w)', 'no CPU fallback'):
        assert phrase in color_module.__doc__, phrase
