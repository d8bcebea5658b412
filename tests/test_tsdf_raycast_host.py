"""CPU: TSDF raycast (pds_tsdf_raycast_fwd; TsdfVolume.raycast, TsdfVolume.rays, StereoRig.raycast, depth_to_disparity).
The entry point is declared, exported and bound and validates without a GPU; the Python surface refuses what it cannot run.

oracle_raycast is the numpy fp64 oracle of tests/test_gpu_tsdf_raycast.py: the contract of tsdf_raycast.py, on M, o, R, the
camera, step, near, far and min_weight as the entry point gets them (rounded once to float32).  It is held to hand-written
answers below.  It does not decide what fp32 cannot.  With EPS (relative: about twenty fp32 roundings) and TAU (absolute,
on a coordinate below 2048) of tests/test_register_depth_host.py, dir = (x, y, 1) and D_a = sum_m |M_am dir_m|:

    d_a              absolute error EPS D_a (a sum of three products; d_a itself may have cancelled)
    a slab value t   (bound - o_a) / d_a: relative error EPS + EPS D_a / |d_a|.  s0 is a max and s1 a min of such values
                     and of near / far, so each lies between the max (min) of the values minus and plus their errors:
                     E_s0, E_s1.  Where |d_a| <= EPS D_a and not both are exactly 0 the kernel may or may not see a
                     zero: undecided.
    a sample s_m     E_s = E_s0 + EPS |s_m|
    g_a(s_m)         E_g = |d_a| E_s + |s_m| EPS D_a + EPS (|o_a| + |s_m d_a|)
    a value          the interpolant changes along an axis by at most the spread of the cell's corners per unit, so
                     E_v = spread * sum_a E_g + EPS max|tsdf|, spread = max - min over the corners of every cell within
                     max(E_g, TAU) of g
    the depth        r = v_prev / (v_prev - v_cur) moves by at most max(E_v) / (v_prev - v_cur) per value, so
                     |depth - oracle| <= E_s + 2 step max(E_v_prev, E_v_cur) / (v_prev - v_cur) + EPS depth
    the normal       within a cell the gradient's components change by at most 2 spread per unit of the other coordinates:
                     angle <= 2.28e-5 rad (tests/test_gpu_surface_normals.py: a float32 unit vector) +
                     sqrt(3) (2 spread sum_a dg_a + EPS max|tsdf|) / |gradient|, dg = |d_a| depth bound + E_g(depth);
                     compared where |gradient| >= 1e-4, as tests/test_gpu_tsdf.py does

A pixel is UNDECIDED when, at any sample up to the oracle's last: an observed value lies within E_v of 0; a grid
coordinate lies within max(E_g, TAU) of an integer whose cells differ in being observed; s_m lies within E_s + E_s1 of
s1; s0 lies within E_s0 + E_s1 of s1; a direction component may or may not be zero; or the depth bound exceeds step.  An
undecided pixel may hold NaN or any depth in [s0, s1]; everything else is compared.  The gradient of a trilinear
interpolant jumps at a cell face, so the NORMAL of a decided hit is compared only where g(depth) is farther than
max(dg, TAU) from every integer, and where the dot product that turns it towards the camera lies farther from 0 than the
gradient's error above times |dir| plus EPS sum_a |(R gradient)_a dir_a| (`normal_decided`); its depth is compared all the
same.  None of this was tuned on kernel
output.

The cap is the project's own 5 % of tests/test_tsdf_host.py: on every scene the GPU file holds against the oracle, the
undecided pixels are at most 5 % of the pixels whose ray meets the box, the decided hits at least 20 % of all pixels, and
at least 90 % of the decided hits have a decided normal (six cell faces at max(dg, TAU) = 0.004 .. 0.01 of a voxel each take
2 .. 6 %) -- asserted here, on the oracle alone.  The wall scenes keep the 5 % but not the 20 %: their images are sized
around the kernel's tile and their volumes around its edge cases, and a 2 x 2 x 2 volume fills one pixel of 33 x 19.

The random volume: weights drawn per voxel at observed = 0.6 leave 0.6^8 = 1.7 % of the cells observed and no ray a hit,
so `raycast_random_volume` draws the weights of random_volume per block of 4 x 4 x 4 voxels, and its tsdf is a slanted
plane under noise with the special values of random_volume (-0.0, 0.0, 1.0) among it."""
import collections
import ctypes
import functools
import inspect
import itertools
import math

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib, tsdf_raycast as raycast_module
from tests.test_register_depth_host import EPS, TAU, simple_rig
from tests.test_tsdf_host import (GENERAL, IDENTITY, HostVolume, camera_of, f32, fresh_state, general_case, general_pose,
                                  oracle_depth, oracle_integrate, q_of)

NAN, INF = float('nan'), float('inf')
ANGLE = 2.28e-5   # rad: tests/test_gpu_surface_normals.py, 4 eps32
TILE = 16         # csrc/common.hpp: kTsdfRaycastTile
POSES = 16        # csrc/common.hpp: kTsdfRaycastPoses

# depth [H, W] fp64 (NaN: a miss); normals [H, W, 3] fp64 (NaN rows); hit, enters, undecided, normal_decided [H, W] bool;
# depth_bound, angle_bound, gradient_norm, s0, s1, slack [H, W] fp64 (slack: E_s0 + E_s1)
Rays = collections.namedtuple('Rays', ['depth', 'normals', 'hit', 'enters', 'undecided', 'normal_decided', 'depth_bound',
                                       'angle_bound', 'gradient_norm', 's0', 's1', 'slack', 'direction'])


def as_the_kernel_sees(origin, voxel_size, pose):
    """-> (M (3, 3), o (3,), R (3, 3)) in fp64, each first rounded to float32; composed in fp64."""
    pose = np.asarray(IDENTITY if pose is None else pose, dtype=np.float64)
    R, t = pose[:, :3], pose[:, 3]
    return f32(R.T / voxel_size), f32((-R.T @ t - np.asarray(origin, dtype=np.float64)) / voxel_size - 0.5), f32(R)


def corners_of(volume, cell):
    """volume [nz, ny, nx], cell int [P, 3] = (i, j, k) -> [P, 8], corner e: bit 0 = +x, bit 1 = +y, bit 2 = +z."""
    i, j, k = cell[:, 0], cell[:, 1], cell[:, 2]
    return np.stack([volume[k + dz, j + dy, i + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)], axis=1)


def trilinear(v, f):
    c00, c10 = v[:, 0] + f[:, 0] * (v[:, 1] - v[:, 0]), v[:, 2] + f[:, 0] * (v[:, 3] - v[:, 2])
    c01, c11 = v[:, 4] + f[:, 0] * (v[:, 5] - v[:, 4]), v[:, 6] + f[:, 0] * (v[:, 7] - v[:, 6])
    c0, c1 = c00 + f[:, 1] * (c10 - c00), c01 + f[:, 1] * (c11 - c01)
    return c0 + f[:, 2] * (c1 - c0)


def trilinear_gradient(v, f):
    lerp = (lambda t, a, b: a + t * (b - a))
    gx = lerp(f[:, 2], lerp(f[:, 1], v[:, 1] - v[:, 0], v[:, 3] - v[:, 2]), lerp(f[:, 1], v[:, 5] - v[:, 4], v[:, 7] - v[:, 6]))
    c00, c10 = lerp(f[:, 0], v[:, 0], v[:, 1]), lerp(f[:, 0], v[:, 2], v[:, 3])
    c01, c11 = lerp(f[:, 0], v[:, 4], v[:, 5]), lerp(f[:, 0], v[:, 6], v[:, 7])
    gy = lerp(f[:, 2], c10 - c00, c11 - c01)
    gz = lerp(f[:, 1], c01, c11) - lerp(f[:, 1], c00, c10)
    return np.stack([gx, gy, gz], axis=1)


def oracle_raycast(tsdf, weight, origin, voxel_size, camera, size, pose=None, min_weight=1.0, step=None, truncation=None,
                   near=0.0, far=INF, eps=EPS, tau=TAU):
    """One pose (3x4 or None) -> Rays.  tsdf, weight float32 [nz, ny, nx]; size = (width, height)."""
    tsdf, weight = np.asarray(tsdf), np.asarray(weight)
    assert tsdf.dtype == weight.dtype == np.float32 and tsdf.shape == weight.shape and tsdf.ndim == 3
    nz, ny, nx = tsdf.shape
    width, height = size
    M, o, R = as_the_kernel_sees(origin, voxel_size, pose)
    fx, fy, cx, cy, skew = f32(camera)
    step = float(f32(0.5 * truncation if step is None else step))
    near, far, min_weight = float(f32(near)), float(f32(far)), np.float32(min_weight)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    y = ((yy - cy) / fy).reshape(-1)
    x = ((xx.reshape(-1) - cx - skew * y) / fx)
    direction = np.stack([x, y, np.ones_like(x)], axis=1)
    pixels = len(x)
    d = direction @ M.T
    eps_d = eps * (np.abs(direction) @ np.abs(M).T)
    dims = np.array([nx, ny, nz])
    top = (dims - 1).astype(np.float64)
    undecided = np.zeros(pixels, dtype=bool)
    blank = np.full(pixels, NAN)
    if dims.min() < 2:
        none = np.zeros(pixels, dtype=bool).reshape(height, width)
        plane = blank.reshape(height, width)
        return Rays(plane, np.full((height, width, 3), NAN), none, none, none, none, plane, plane, plane, plane, plane, plane,
                    direction.reshape(height, width, 3))

    # 2. the slabs, each value with its error
    inside = np.ones(pixels, dtype=bool)
    s0, s0_up, s0_dn = (np.full(pixels, near) for _ in range(3))
    s1, s1_up, s1_dn = (np.full(pixels, far) for _ in range(3))
    with np.errstate(all='ignore'):
        for a in range(3):
            da = d[:, a]
            exact_zero = (da == 0) & (eps_d[:, a] == 0)
            maybe_zero = (np.abs(da) <= eps_d[:, a]) & ~exact_zero
            undecided |= maybe_zero
            inside &= np.where(exact_zero, (o[a] >= 0) & (o[a] <= top[a]), True)
            free = exact_zero | maybe_zero
            t0, t1 = (0.0 - o[a]) / da, (top[a] - o[a]) / da
            relative = eps + eps_d[:, a] / np.abs(da)
            e0, e1 = np.abs(t0) * relative, np.abs(t1) * relative
            first = t0 <= t1
            lo, hi = np.where(free, -INF, np.minimum(t0, t1)), np.where(free, INF, np.maximum(t0, t1))
            e_lo, e_hi = np.where(free, 0.0, np.where(first, e0, e1)), np.where(free, 0.0, np.where(first, e1, e0))
            s0, s0_up, s0_dn = np.maximum(s0, lo), np.maximum(s0_up, lo + e_lo), np.maximum(s0_dn, lo - e_lo)
            s1, s1_up, s1_dn = np.minimum(s1, hi), np.minimum(s1_up, hi + e_hi), np.minimum(s1_dn, hi - e_hi)
        E_s0 = np.maximum(s0_up - s0, s0 - s0_dn)
        E_s1 = np.where(np.isfinite(s1), np.maximum(s1_up - s1, s1 - s1_dn), 0.0)
        enters = inside & (s0 <= s1) & np.isfinite(s0) & np.isfinite(s1)
        undecided |= inside & np.isfinite(s0) & np.isfinite(s1) & (np.abs(s1 - s0) <= E_s0 + E_s1)

    observed_voxel = weight >= min_weight
    value = tsdf.astype(np.float64)
    largest = float(np.abs(value).max())
    shifts = [(slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
              for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    cell_observed = np.logical_and.reduce([observed_voxel[s] for s in shifts])
    cell_spread = np.maximum.reduce([value[s] for s in shifts]) - np.minimum.reduce([value[s] for s in shifts])

    def cells(g, margin):
        """-> (cell [P, 3], f [P, 3], observed [P], differs [P], spread [P]) for the positions g under `margin`."""
        cell = np.clip(np.floor(g), 0, top - 1).astype(np.int64)
        low = np.clip(np.floor(g - margin), 0, top - 1).astype(np.int64)
        high = np.clip(np.floor(g + margin), 0, top - 1).astype(np.int64)
        seen = cell_observed[cell[:, 2], cell[:, 1], cell[:, 0]]
        spread = cell_spread[cell[:, 2], cell[:, 1], cell[:, 0]]
        differs = np.zeros(len(g), dtype=bool)
        for pick in itertools.product((0, 1), repeat=3):
            i, j, k = ((high if p else low)[:, a] for a, p in enumerate(pick))
            differs |= cell_observed[k, j, i] != seen
            spread = np.maximum(spread, cell_spread[k, j, i])
        return cell, g - cell, seen, differs, spread

    def position_error(s, E_s):
        return np.abs(d) * E_s[:, None] + np.abs(s)[:, None] * eps_d + eps * (np.abs(o)[None, :] + np.abs(s[:, None] * d))

    # 3., 4., 5. the march, all pixels at once
    depth, depth_bound = blank.copy(), blank.copy()
    hit = np.zeros(pixels, dtype=bool)
    done = ~enters
    prev_ok = np.zeros(pixels, dtype=bool)
    s_prev, v_prev, e_prev = np.zeros(pixels), np.zeros(pixels), np.zeros(pixels)
    with np.errstate(all='ignore'):
        most = int(np.ceil(np.where(enters, (s1 - s0) / step, 0.0).max())) + 3
    assert most <= 65538
    for m in range(most):
        alive = ~done
        if not alive.any():
            break
        idx = np.nonzero(alive)[0]
        s = s0[idx] + m * step
        E_s = E_s0[idx] + eps * np.abs(s)
        undecided[idx] |= np.abs(s - s1[idx]) <= E_s + E_s1[idx]
        exists = s <= s1[idx]
        done[idx[~exists]] = True   # past s1: a miss
        idx, s, E_s = idx[exists], s[exists], E_s[exists]
        g = o[None, :] + s[:, None] * d[idx]
        E_g = position_error(s, E_s) if len(idx) == pixels else (
            np.abs(d[idx]) * E_s[:, None] + np.abs(s)[:, None] * eps_d[idx] +
            eps * (np.abs(o)[None, :] + np.abs(s[:, None] * d[idx])))
        margin = np.maximum(E_g, tau)
        assert margin.max(initial=0.0) < 0.5, 'the rounding margin of a grid coordinate exceeds half a voxel'
        cell, f, seen, differs, spread = cells(g, margin)
        undecided[idx] |= differs
        v = trilinear(corners_of(value, cell), f)
        E_v = spread * E_g.sum(axis=1) + eps * largest
        undecided[idx] |= seen & (np.abs(v) <= E_v)
        negative = seen & (v < 0)
        now = negative & prev_ok[idx]
        delta = v_prev[idx] - v
        with np.errstate(all='ignore'):
            z = s_prev[idx] + step * v_prev[idx] / delta
            bound = E_s + 2.0 * step * np.maximum(E_v, e_prev[idx]) / delta + eps * np.abs(z)
        depth[idx[now]], depth_bound[idx[now]] = z[now], bound[now]
        hit[idx[now]] = True
        undecided[idx[now]] |= ~(bound[now] <= step)
        done[idx[negative]] = True
        prev_ok[idx], s_prev[idx], v_prev[idx], e_prev[idx] = seen & ~negative, s, np.where(seen, v, 0.0), E_v
    assert done.all()

    # 6. the normals of the hits
    normals = np.full((pixels, 3), NAN)
    angle_bound, gradient_norm = blank.copy(), blank.copy()
    normal_decided = np.zeros(pixels, dtype=bool)
    idx = np.nonzero(hit)[0]
    if len(idx):
        z = depth[idx]
        g = o[None, :] + z[:, None] * d[idx]
        E_g = (np.abs(d[idx]) * (E_s0[idx] + eps * z)[:, None] + z[:, None] * eps_d[idx] +
               eps * (np.abs(o)[None, :] + np.abs(z[:, None] * d[idx])))
        dg = np.abs(d[idx]) * depth_bound[idx][:, None] + E_g
        margin = np.maximum(dg, tau)
        cell, f, seen, _, _ = cells(g, margin)
        spread = cell_spread[cell[:, 2], cell[:, 1], cell[:, 0]]
        with np.errstate(invalid='ignore'):
            one_cell = (np.floor(g - margin) == np.floor(g + margin)).all(axis=1)
        normal_decided[idx] = one_cell & ~undecided[idx]
        gradient = trilinear_gradient(corners_of(value, cell), f)
        turned = gradient @ R.T
        # towards the camera; which way is for the rounding to say where the dot product lies within its error
        along = (turned * direction[idx]).sum(axis=1)
        slack = (math.sqrt(3.0) * (2.0 * spread * dg.sum(axis=1) + eps * largest) * np.linalg.norm(direction[idx], axis=1) +
                 eps * (np.abs(turned) * np.abs(direction[idx])).sum(axis=1))
        normal_decided[idx] &= np.abs(along) > slack
        turned = np.where((along > 0)[:, None], -turned, turned)
        length = np.sqrt((turned * turned).sum(axis=1))
        good = seen & (length > 0) & np.isfinite(length)
        with np.errstate(all='ignore'):
            normals[idx] = np.where(good[:, None], turned / length[:, None], NAN)
            grid_length = np.sqrt((gradient * gradient).sum(axis=1))
            gradient_norm[idx] = np.where(seen, grid_length, NAN)
            angle_bound[idx] = ANGLE + math.sqrt(3.0) * (2.0 * spread * dg.sum(axis=1) + eps * largest) / grid_length
    shape = (height, width)
    return Rays(depth.reshape(shape), normals.reshape(shape + (3,)), hit.reshape(shape), enters.reshape(shape),
                undecided.reshape(shape), normal_decided.reshape(shape), depth_bound.reshape(shape),
                angle_bound.reshape(shape), gradient_norm.reshape(shape), s0.reshape(shape), s1.reshape(shape),
                (E_s0 + E_s1).reshape(shape), direction.reshape(shape + (3,)))


def check_raycast(depth, normals, oracle, case=''):
    """depth float32 [H, W], normals float32 [H, W, 3] or None against Rays -> (decided hits, normals compared).  Decided
    pixels: hit or miss exactly, the depth within its bound; undecided ones: NaN or a depth in [s0, s1].  Normals: NaN
    wherever the depth is; on decided hits with a decided normal NaN exactly where the oracle's is, the others unit and
    within the angle bound (where |gradient| >= 1e-4)."""
    depth = np.asarray(depth)
    assert depth.dtype == np.float32 and depth.shape == oracle.depth.shape, case
    got = depth.astype(np.float64)
    sure = ~oracle.undecided
    assert np.array_equal(np.isnan(got)[sure], ~oracle.hit[sure]), (
        case, 'hit or miss', np.argwhere(sure & (np.isnan(got) == oracle.hit))[:5].tolist())
    both = sure & oracle.hit
    with np.errstate(invalid='ignore'):
        off = np.abs(got - oracle.depth) - oracle.depth_bound
        assert (off[both] <= 0).all(), (case, 'depth', float(off[both].max()), np.argwhere(both & (off > 0))[:5].tolist())
        loose = oracle.undecided & ~np.isnan(got)
        assert ((got >= oracle.s0 - oracle.slack) & (got <= oracle.s1 + oracle.slack))[loose].all(), (case, 'undecided')
    if normals is None:
        return int(both.sum()), 0
    normals = np.asarray(normals)
    assert normals.dtype == np.float32 and normals.shape == oracle.normals.shape, case
    n = normals.astype(np.float64)
    missing = np.isnan(n).any(axis=2)
    assert np.array_equal(np.isnan(n).all(axis=2), missing), case            # (a row is NaN as a whole)
    assert missing[np.isnan(got)].all(), (case, 'a normal without a depth')
    assert np.abs(np.linalg.norm(n[~missing], axis=1) - 1.0).max(initial=0.0) <= 1e-6, case
    compared = both & oracle.normal_decided
    absent = np.isnan(oracle.normals).any(axis=2)
    assert np.array_equal(missing[compared], absent[compared]), (case, 'NaN normals')
    with np.errstate(invalid='ignore'):
        checked = compared & ~absent & (oracle.gradient_norm >= 1e-4)
    cross = np.linalg.norm(np.cross(n[checked], oracle.normals[checked]), axis=1)
    angle = np.arctan2(cross, (n[checked] * oracle.normals[checked]).sum(axis=1))
    over = angle - oracle.angle_bound[checked]
    assert (over <= 0).all(), (case, 'angle', float(over.max()))
    return int(both.sum()), int(checked.sum())


def shares(oracle):
    """-> (the undecided among the pixels whose ray meets the box, the decided hits among all pixels, those with a decided
    normal among the decided hits)."""
    meets = oracle.enters | oracle.undecided
    hits = oracle.hit & ~oracle.undecided
    return (float(oracle.undecided[meets].mean()) if meets.any() else 0.0, float(hits.mean()),
            float(oracle.normal_decided[hits].mean()) if hits.any() else 1.0)


# ------------------------------------------------------------------------------------------------ the wall, by hand
# Dyadic throughout.  Voxels of 1/8 m, truncation 1/4 m, step = truncation / 4 = 1/16 m.  The wall is the plane
# z = z0 = origin_z + (layer + 1/2) / 8 + 3/32 of the world: 3/4 of the way from the centres of layer `layer` to those of the
# next.  tsdf = clip((z0 - z) / truncation): 0.375 on that layer, -0.125 on the next, +0.5 per layer towards the camera.
# A trilinear interpolant of a linear function is exact, and with step = truncation / 4 both samples around the crossing
# and every voxel they read lie within step + 1/8 = 3/16 < truncation of the wall: in the unclipped, linear part.
# A volume of two layers is two steps deep, so a march from its front face would put its third sample exactly on the back
# face, which no oracle can promise: the scenes of the GPU file start at near = 1.0625 + 3/64 instead, and their samples lie
# 3/64 and 7/64 m into the box, around the wall at 6/64.
RAYWALL = dict(voxel_size=0.125, truncation=0.25, step=0.0625, origin_z=1.0, focal=16.0, near=1.109375)


def raywall_volume(dims, layer=0):
    """-> (origin, z0, tsdf, weight): x and y centred on the optical axis, every weight 1."""
    nx, ny, nz = dims
    vs = RAYWALL['voxel_size']
    origin = np.array([-0.5 * nx * vs, -0.5 * ny * vs, RAYWALL['origin_z']])
    z0 = RAYWALL['origin_z'] + (layer + 0.5) * vs + 0.09375
    z = RAYWALL['origin_z'] + (np.arange(nz) + 0.5) * vs
    tsdf = np.broadcast_to(np.clip((z0 - z) / RAYWALL['truncation'], -1.0, 1.0)[:, None, None], (nz, ny, nx))
    return origin, z0, np.ascontiguousarray(tsdf, dtype=np.float32), np.ones((nz, ny, nx), dtype=np.float32)


def raywall_camera(size, focal=None):
    width, height = size
    focal = RAYWALL['focal'] if focal is None else focal
    return (focal, focal, 0.5 * (width - 1), 0.5 * (height - 1), 0.0)


def raywall_oracle(dims, size, layer=0, pose=None, weight=None, focal=None, **kw):
    origin, z0, tsdf, ones = raywall_volume(dims, layer)
    return oracle_raycast(tsdf, ones if weight is None else weight, origin, RAYWALL['voxel_size'],
                          raywall_camera(size, focal), size, pose=pose, step=RAYWALL['step'], **kw), z0


def test_oracle_wall_by_hand():
    dims, size = (8, 6, 8), (33, 25)
    o, z0 = raywall_oracle(dims, size, layer=4, focal=32.0)
    assert z0 == 1.0 + 4.5 / 8 + 3 / 32 and not o.undecided[12, 16]
    # (dyadic numbers make ties: a ray along y = -1/4 leaves the box exactly on its third sample.  Those are undecided)
    assert 0 < o.undecided.sum() <= 0.1 * o.enters.sum() and o.undecided[4, 5] and o.s1[4, 5] == o.s0[4, 5] + 3 / 16
    # the centre ray by hand: it enters at z = 1.0625 (the centres of layer 0), and 1.0625 + 9 / 16 = 1.625 is the last
    # sample in front of the wall at 1.65625 with v = 0.125; the next has v = -0.125: depth = 1.625 + (1 / 16) / 2
    assert o.s0[12, 16] == 1.0625 and o.s1[12, 16] == 1.0625 + 7 / 8 and o.depth[12, 16] == z0 == 1.65625
    assert o.normals[12, 16].tolist() == [0.0, 0.0, -1.0] and o.gradient_norm[12, 16] == 0.5
    # every hit lies on the wall and faces the camera
    assert o.hit.sum() > 50 and np.abs(o.depth[o.hit] - z0).max() <= 1e-12
    assert np.abs(o.normals[o.hit] - [0.0, 0.0, -1.0]).max() <= 1e-12 and o.normal_decided[o.hit].any()
    # which rays: the wall point (x z0, y z0, z0) and the ray one step behind it inside the box -> a hit; a ray that has
    # left the box through a side before the wall -> a miss, though it entered
    vs = RAYWALL['voxel_size']
    half = 0.5 * (np.array(dims[:2]) - 1) * vs
    reach = lambda z: (np.abs(o.direction[..., 0] * z) <= half[0]) & (np.abs(o.direction[..., 1] * z) <= half[1])
    assert o.hit[reach(z0) & reach(z0 + RAYWALL['step']) & reach(1.0625)].all()
    left_early = o.enters & (o.s1 < z0 - 1e-9)
    assert left_early.sum() > 20 and not o.hit[left_early].any() and not o.hit[~o.enters].any()
    assert (~o.enters).sum() > 100   # (and the image is wider than the volume)
    # the camera behind the wall, looking back at it: negative values first, all rays miss
    behind = np.hstack([np.diag([-1.0, 1.0, -1.0]), [[0.0], [0.0], [3.0]]])
    b, _ = raywall_oracle(dims, size, layer=4, pose=behind, focal=32.0)
    assert b.enters.sum() > 50 and not b.hit.any() and np.isnan(b.depth).all() and np.isnan(b.normals).all()
    # a slab of zero weight in free space in front of the wall: still a hit, the same depth
    weight = np.ones((8, 6, 8), dtype=np.float32)
    weight[1] = 0.0
    w, _ = raywall_oracle(dims, size, layer=4, weight=weight, focal=32.0)
    assert np.array_equal(w.hit, o.hit) and np.array_equal(w.depth, o.depth, equal_nan=True)
    # zero weight at the surface: a miss (the first observed negative sample has no observed predecessor)
    weight = np.ones((8, 6, 8), dtype=np.float32)
    weight[4] = 0.0
    w, _ = raywall_oracle(dims, size, layer=4, weight=weight, focal=32.0)
    assert w.enters.sum() > 50 and not w.hit.any()
    # min_weight: the same slab at weight 0.5 is observed at min_weight 0.5 and not at 1
    weight[4] = 0.5
    assert raywall_oracle(dims, size, layer=4, weight=weight, focal=32.0, min_weight=0.5)[0].hit.sum() == o.hit.sum()
    assert not raywall_oracle(dims, size, layer=4, weight=weight, focal=32.0)[0].hit.any()
    # near beyond the wall: the march starts behind it; far in front of it: it ends before it
    assert not raywall_oracle(dims, size, layer=4, focal=32.0, near=1.7)[0].hit.any()
    assert not raywall_oracle(dims, size, layer=4, focal=32.0, far=1.6)[0].hit.any()
    # a volume with a dimension of 1 has no cell
    flat, _ = raywall_oracle((8, 1, 8), size, layer=4)
    assert not flat.hit.any() and not flat.enters.any() and np.isnan(flat.depth).all()


def test_oracle_tilted_pose_against_the_ray_plane_intersection():
    dims, size = (16, 12, 8), (33, 25)
    origin, z0, tsdf, weight = raywall_volume(dims, layer=3)
    pose = np.hstack([pds.rectification.rodrigues(np.array([0.12, -0.2, 0.05])), [[0.05], [-0.03], [0.1]]])
    o = oracle_raycast(tsdf, weight, origin, RAYWALL['voxel_size'], raywall_camera(size, 40.0), size, pose=pose,
                       step=RAYWALL['step'])
    # as the kernel sees the pose: R, and the camera centre from o = (C - origin) / voxel_size - 0.5
    M, offset, R = as_the_kernel_sees(origin, RAYWALL['voxel_size'], pose)
    centre_z = (offset[2] + 0.5) * RAYWALL['voxel_size'] + origin[2]
    along = (o.direction @ (M * RAYWALL['voxel_size']).T)[..., 2]   # the world z a ray gains per unit of s
    expected = (z0 - centre_z) / along
    assert o.hit.sum() > 200 and np.abs(o.depth - expected)[o.hit].max() <= 1e-9
    assert np.abs(o.normals[o.hit] - R @ [0.0, 0.0, -1.0]).max() <= 1e-7   # (R rounded to float32 is not quite a rotation)
    assert ((o.normals[o.hit] * o.direction[o.hit]).sum(axis=1) < 0).all()
    assert o.undecided.mean() <= 0.05 and (o.depth_bound[o.hit & ~o.undecided] < 1e-3).all()


def test_check_raycast_takes_the_answer_and_refuses_others():
    o, z0 = raywall_oracle((8, 6, 8), (33, 25), layer=4, focal=32.0)
    depth, normals = o.depth.astype(np.float32), o.normals.astype(np.float32)
    hits, compared = check_raycast(depth, normals, o)
    assert hits == o.hit.sum() > 50 and compared > 10 and check_raycast(depth, None, o) == (hits, 0)
    row, col = np.argwhere(o.hit & o.normal_decided)[0]
    miss = tuple(np.argwhere(o.enters & ~o.hit)[0])
    for change in ('shifted', 'hit where it misses', 'miss where it hits', 'flipped', 'normal on a miss', 'not unit'):
        bad_depth, bad_normals = depth.copy(), normals.copy()
        if change == 'shifted':
            bad_depth[row, col] += 1e-3
        elif change == 'hit where it misses':
            bad_depth[miss] = z0
        elif change == 'miss where it hits':
            bad_depth[row, col] = NAN
            bad_normals[row, col] = NAN
        elif change == 'flipped':
            bad_normals[row, col] *= -1.0
        elif change == 'normal on a miss':
            bad_normals[miss] = (0.0, 0.0, -1.0)
        else:
            bad_normals[row, col] *= 1.001
        with pytest.raises(AssertionError):
            check_raycast(bad_depth, bad_normals, o, change)
    # an undecided pixel may hold NaN or any depth in [s0, s1], and nothing else
    loose = o._replace(undecided=o.undecided | o.hit)
    bad_depth, bad_normals = depth.copy(), normals.copy()
    bad_depth[row, col] = o.s0[row, col]
    check_raycast(bad_depth, bad_normals, loose)
    bad_depth[row, col], bad_normals[row, col] = NAN, NAN
    check_raycast(bad_depth, bad_normals, loose)
    bad_depth[row, col] = o.s1[row, col] + 0.01
    with pytest.raises(AssertionError):
        check_raycast(bad_depth, normals, loose)


def test_oracle_marks_what_fp32_cannot_decide():
    # a sample exactly on the wall has the value 0: < 0 or not is for the rounding to say
    dims, size = (4, 4, 8), (1, 1)
    origin, z0, tsdf, weight = raywall_volume(dims, layer=4)
    o = oracle_raycast(tsdf, weight, origin, 0.125, raywall_camera(size), size, step=0.0625)
    assert not o.undecided.any() and o.hit.all() and o.depth[0, 0] == z0 == 1.65625
    tsdf = tsdf + np.float32(0.125)    # the wall moves 1/32 m back, onto a sample: 1.6875 = 1.0625 + 10 / 16
    o = oracle_raycast(tsdf, weight, origin, 0.125, raywall_camera(size), size, step=0.0625)
    assert o.undecided.all()
    # a sample on a cell face between an observed and an unobserved cell
    weight = np.ones((8, 4, 4), dtype=np.float32)
    weight[0] = 0.0
    o = oracle_raycast(tsdf, weight, origin, 0.125, raywall_camera(size), size, step=0.0625)
    assert o.undecided.all()   # (sample 2 sits on the face between cell layers 0 and 1)
    # the last sample exactly on s1
    o = oracle_raycast(tsdf + np.float32(1.0), np.ones_like(tsdf), origin, 0.125, raywall_camera(size), size, step=0.0625)
    assert o.undecided.all() and not o.hit.any()   # (no surface: the march runs to s1 = s0 + 14 steps exactly)


# ------------------------------------------------------------------------------------------------ the scenes of the GPU file
WALL_SIZES = ((1, 1), (5, 3), (17, 9), (33, 19))
WALL_DIMS = ((2, 2, 2), (5, 3, 2), (33, 7, 9))
GENERAL_SIZE = (GENERAL['width'], GENERAL['height'])
RANDOM_DIMS = (40, 36, 28)
RANDOM_CASES = ((1.0, 0.6), (0.375, 0.97))   # (min_weight, observed)


def fourth_pose():
    return np.hstack([pds.rectification.rodrigues(np.array([-0.03, 0.05, 0.04])), [[-0.01], [0.015], [0.02]]])


def general_camera():
    return camera_of(general_case()['matrix'])


@functools.lru_cache(maxsize=None)
def general_state():
    """The general case of tests/test_tsdf_host.py fused from its three poses by the fp64 oracle -> float32 (tsdf, weight)."""
    state = fresh_state(GENERAL['dims'])
    for k in range(3):
        step = oracle_integrate(*state, **general_case(k))
        state = (step.tsdf, step.weight)
    return state[0].astype(np.float32), state[1].astype(np.float32)


def general_oracle(tsdf, weight, pose, **kw):
    return oracle_raycast(tsdf, weight, GENERAL['origin'], GENERAL['voxel_size'], general_camera(), GENERAL_SIZE, pose=pose,
                          truncation=GENERAL['truncation'], **kw)


def raycast_random_volume(dims, seed, min_weight=1.0, observed=0.6):
    """In the manner of random_volume (tests/test_gpu_tsdf.py), see the module text: float32 tsdf = a slanted plane through
    the middle of the volume, in units of 6 voxels, clipped, plus noise of +-0.05, with -0.0, 0.0 and 1.0 sprinkled in;
    weights around min_weight drawn per block of 4 x 4 x 4 voxels, of which the share `observed` reaches it."""
    nx, ny, nz = dims
    rng = np.random.RandomState(seed)
    kk, jj, ii = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float64)
    plane = (0.55 * nz + 0.15 * (ii - 0.5 * nx) - 0.1 * (jj - 0.5 * ny) - kk) / 6.0
    tsdf = (np.clip(plane, -1.0, 1.0) + rng.uniform(-0.05, 0.05, plane.shape)).astype(np.float32)
    special = rng.rand(nz, ny, nx)
    tsdf[special < 0.01] = -0.0
    tsdf[(special >= 0.01) & (special < 0.02)] = 0.0
    tsdf[(special >= 0.02) & (special < 0.03)] = 1.0
    blocks = tuple((n + 3) // 4 for n in (nz, ny, nx))
    spread = (lambda a: np.repeat(np.repeat(np.repeat(a, 4, 0), 4, 1), 4, 2)[:nz, :ny, :nx])
    above = spread(rng.choice(np.array([min_weight, min_weight, 2.0 * min_weight, 64.0], dtype=np.float32), blocks))
    below = spread(rng.choice(np.array([0.0, 0.5 * min_weight, np.nextafter(np.float32(min_weight), np.float32(0.0))],
                                       dtype=np.float32), blocks))
    weight = np.where(spread(rng.rand(*blocks) < observed), above, below).astype(np.float32)
    return tsdf, weight


RANDOM = dict(origin=(-0.41, -0.37, 0.5), voxel_size=0.02, truncation=0.06)


def random_oracle(tsdf, weight, min_weight, pose):
    return oracle_raycast(tsdf, weight, RANDOM['origin'], RANDOM['voxel_size'], general_camera(), GENERAL_SIZE, pose=pose,
                          min_weight=min_weight, truncation=RANDOM['truncation'])


def test_the_scenes_are_decided_and_not_empty():
    scenes = {}
    state = general_state()
    scenes['general, fourth pose'] = general_oracle(*state, fourth_pose())
    for k in range(3):
        scenes['general, pose %d' % k] = general_oracle(*state, general_pose(k))
    for min_weight, observed in RANDOM_CASES:
        volume = raycast_random_volume(RANDOM_DIMS, sum(RANDOM_DIMS), min_weight, observed)
        scenes['random %g' % observed] = random_oracle(*volume, min_weight, fourth_pose())
    for name, oracle in scenes.items():
        loose, hits, with_normal = shares(oracle)
        print('%s: %.2f %% of the rays that meet the box undecided, %.1f %% of the pixels decided hits, %.1f %% of those '
              'with a decided normal, largest depth bound %.3g m' %
              (name, 100 * loose, 100 * hits, 100 * with_normal,
               np.nanmax(oracle.depth_bound[oracle.hit & ~oracle.undecided])))
        assert loose <= 0.05 and hits >= 0.20 and with_normal >= 0.90, name
        # and the fp64 answer passes the check it is the yardstick of
        check_raycast(oracle.depth.astype(np.float32), oracle.normals.astype(np.float32), oracle, name)
        # every normal faces the camera, n . dir < 0
        has = ~np.isnan(oracle.normals).any(axis=2)
        assert ((oracle.normals[has] * oracle.direction[has]).sum(axis=1) < 0).all(), name
    for dims in WALL_DIMS:
        for size in WALL_SIZES:
            oracle, z0 = raywall_oracle(dims, size, near=RAYWALL['near'])
            assert shares(oracle)[0] <= 0.05 and oracle.hit.any(), (dims, size)
            assert np.abs(oracle.depth[oracle.hit] - z0).max() <= 1e-12, (dims, size)


def test_end_to_end_bound_on_the_oracle():
    """Raycasting at an integration pose with the integrating camera against oracle_depth of that frame.  A hit lies
    between a sample with tsdf >= 0 and one with tsdf < 0, both interpolated from voxels within one voxel of the sample on
    every axis; a voxel of one frame holds (Z - z_c) / truncation of the pixel its centre projects to, so the zero of the
    interpolant lies within one voxel's reach in depth, voxel_size (|R[2, 0]| + |R[2, 1]| + |R[2, 2]|), of a depth that
    pixel or a neighbour of it saw, and where the surface is cut (a depth edge within the neighbourhood) within
    truncation of one: truncation + one voxel's reach + EPS Z, against the nearest Z in the 5 x 5 pixels around, as
    surface_gap derives its own.  The largest gap of the fp64 oracle is printed beside what the bound allows."""
    gap, allowed, count = end_to_end_gap(*end_to_end_state(), None)
    print('end to end: %d hits, at most %.4f m from the depth their pixels were measured at, %.4f m more than allowed' %
          (count, gap.max(), (gap - allowed).max()))
    assert count > 0.2 * 48 * 64 and (gap <= allowed).all()


@functools.lru_cache(maxsize=None)
def end_to_end_state():
    step = oracle_integrate(*fresh_state(GENERAL['dims']), **general_case())
    return step.tsdf.astype(np.float32), step.weight.astype(np.float32)


def end_to_end_gap(tsdf, weight, depth):
    """depth [H, W] (None: the oracle's own) -> (gap [N], allowed [N], N) over the hits."""
    case = general_case()
    if depth is None:
        depth = general_oracle(tsdf, weight, case['pose']).depth
    depth = np.asarray(depth, dtype=np.float64)
    Z = oracle_depth(case['disparity'], f32(case['matrix']))
    height, width = Z.shape
    padded = np.pad(Z, 2, constant_values=NAN)
    around = np.stack([padded[dy:dy + height, dx:dx + width] for dy in range(5) for dx in range(5)])
    with np.errstate(invalid='ignore'):
        apart = np.abs(around - depth[None])
    nearest = np.where(np.isnan(apart), INF, apart).min(axis=0)
    hits = ~np.isnan(depth)
    reach = GENERAL['voxel_size'] * np.abs(case['pose'][2, :3]).sum()
    allowed = GENERAL['truncation'] + reach + EPS * depth[hits]
    return nearest[hits], allowed, int(hits.sum())


# ------------------------------------------------------------------------------------------------ the C ABI
def test_raycast_symbol_declared_exported_and_bound(hip_library):
    header = open(_lib.HEADER_PATH).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    name = 'pds_tsdf_raycast_fwd'
    assert name + '(' in header and hasattr(raw, name) and name in _lib.SIGNATURES
    assert hip_library.pds_abi_version() == 7 and '#define PDS_ABI_VERSION 7' in header
    assert len(_lib.SIGNATURES[name][1]) == 19
    for exported in ('Raycast', 'depth_to_disparity'):
        assert exported in pds.__all__ and hasattr(pds, exported), exported
    assert pds.Raycast._fields == ('depth', 'normals') and pds.Raycast is raycast_module.Raycast
    csrc = _lib.HEADER_PATH.replace('include/pds_hip.h', 'practicaldeepstereo_nips2018_amd/csrc/')
    common = open(csrc + 'common.hpp').read()
    assert 'constexpr int kTsdfRaycastTile = %d;' % TILE in common
    assert 'constexpr int kTsdfRaycastPoses = %d;' % POSES in common
    assert 'tsdf_raycast.hip' in [s.rsplit('/', 1)[-1] for s in _lib.sources()]


def test_raycast_validation_needs_no_gpu(hip_library):
    lib = hip_library
    big = 1 << 24
    t, w, dp, nm = [ctypes.c_void_p(big * n) for n in range(1, 5)]   # never dereferenced
    floats = (lambda values: (ctypes.c_float * len(values))(*values))
    rays = floats([10.0, 0, 0, 0, 10.0, 0, 0, 0, 10.0, 1.5, 1.0, -5.0])
    turn = floats(np.eye(3).reshape(-1).tolist())
    camera = floats([4.0, 4.0, 1.0, 0.5, 0.0])
    error = lib.pds_last_error

    def run(tsdf=t, weight=w, dims=(4, 3, 2), voxel_size=0.1, rays=rays, rotations=turn, camera=camera, step=0.05,
            near=0.0, far=INF, min_weight=1.0, depth=dp, normals=nm, shape=(1, 2, 3)):
        return lib.pds_tsdf_raycast_fwd(tsdf, weight, *dims, voxel_size, rays, rotations, camera, step, near, far,
                                        min_weight, depth, normals, *shape, None)

    for name in ('tsdf', 'weight', 'rays', 'rotations', 'camera', 'depth'):
        assert run(**{name: None}) != 0 and error() == b'tsdf_raycast: null pointer', name
    for dims in [(0, 3, 2), (4, 3, -2)]:
        assert run(dims=dims) != 0 and b'tsdf: bad volume' in error(), dims
    assert run(dims=((1 << 24) + 1, 1, 1)) != 0 and b'above 2^24' in error()
    assert run(dims=(895, 895, 895)) != 0 and b'does not fit 32-bit indices' in error()
    for shape in [(0, 2, 3), (-1, 2, 3)]:
        assert run(shape=shape) != 0 and b'tsdf_raycast: bad batch' in error(), shape
    for shape in [(1, 0, 3), (1, 2, 0), (1, -2, 3)]:
        assert run(shape=shape) != 0 and b'tsdf_raycast: bad shape' in error(), shape
    assert run(shape=(1 << 12, 1 << 10, 1 << 10)) != 0 and b'batch * h * w' in error() and b'32-bit indices' in error()
    for bad in (0.0, -1.0, NAN, INF):
        assert run(voxel_size=bad) != 0 and b'voxel_size must be positive and finite' in error(), bad
        assert run(step=bad) != 0 and b'step must be positive and finite' in error(), bad
    for bad in (-0.5, NAN, INF):
        assert run(near=bad) != 0 and b'near must be >= 0 and finite' in error(), bad
    for near, far in ((1.0, 1.0), (1.0, 0.5), (0.0, NAN), (0.0, 0.0)):
        assert run(near=near, far=far) != 0 and b'far must be above near' in error(), (near, far)
    assert run(min_weight=NAN) != 0 and b'min_weight is NaN' in error()
    # a march that could be long: 4 x 3 x 2 voxels of 0.1 m have a diagonal of 0.1 sqrt(9 + 4 + 1) = 0.374 m
    assert run(step=5e-6) != 0 and b'samples of step' in error() and b'at most 65536' in error()
    assert run(dims=(1 << 20, 2, 2), step=1.0 / 1024) != 0 and b'at most 65536' in error()
    for k, bad in itertools.product((0, 4), (NAN, INF)):
        values = list(camera)
        values[k] = bad
        assert run(camera=floats(values)) != 0 and b'non-finite camera' in error(), (k, bad)
    for k, bad in ((0, 0.0), (1, -4.0)):
        values = list(camera)
        values[k] = bad
        assert run(camera=floats(values)) != 0 and b'focal lengths must be positive' in error(), (k, bad)
    for bad in (NAN, INF):
        values = list(rays)
        values[11] = bad
        assert run(rays=floats(values)) != 0 and b'non-finite ray' in error(), bad
        values = list(turn)
        values[8] = bad
        assert run(rotations=floats(values)) != 0 and b'non-finite rotation' in error(), bad
    for name, p in (('tsdf', t), ('weight', w), ('depth', dp), ('normals', nm)):
        for off in (1, 2):
            assert run(**{name: ctypes.c_void_p(p.value + off)}) != 0 and b'not 4-byte aligned' in error(), (name, off)
    # 4 x 3 x 2 voxels: 96 bytes; 2 x 3 pixels: 24 bytes of depth, 72 of normals
    assert run(depth=t) != 0 and b'an output aliases the volume' in error()
    assert run(depth=ctypes.c_void_p(w.value + 92)) != 0 and b'an output aliases the volume' in error()
    assert run(normals=ctypes.c_void_p(t.value - 68)) != 0 and b'an output aliases the volume' in error()
    assert run(normals=dp) != 0 and b'an output aliases another output' in error()
    assert run(normals=ctypes.c_void_p(dp.value + 20)) != 0 and b'an output aliases another output' in error()
    assert run(depth=ctypes.c_void_p(nm.value + 68)) != 0 and b'an output aliases another output' in error()


# ------------------------------------------------------------------------------------------------ Python
def test_raycast_python_errors_and_signatures():
    volume = HostVolume((0.0, 0.0, 0.0), 0.1, (4, 3, 2), 0.3)
    camera = (4.0, 4.0, 2.0, 1.5, 0.0)

    def run(camera=camera, size=(5, 4), **kw):
        return volume.raycast(camera, size, **kw)

    for bad in ((4.0, 4.0, 2.0, 1.5), (4.0,) * 6):
        with pytest.raises(ValueError, match='camera must hold 5 values'):
            run(camera=bad)
    with pytest.raises(TypeError, match='camera must be a sequence of numbers'):
        run(camera='wide')
    with pytest.raises(ValueError, match='camera has non-finite entries'):
        run(camera=(4.0, NAN, 2.0, 1.5, 0.0))
    with pytest.raises(ValueError, match='camera must have positive focal lengths'):
        run(camera=(4.0, 0.0, 2.0, 1.5, 0.0))
    for bad in ((5,), (5, 4, 3), 5, (5.5, 4), None):
        with pytest.raises(ValueError, match='size must be two integers'):
            run(size=bad)
    for bad in ((0, 4), (5, -1)):
        with pytest.raises(ValueError, match=r'size must be at least \(1, 1\)'):
            run(size=bad)
    for bad in (np.eye(3), np.eye(4), np.full((3, 4), NAN), np.zeros((1, 4, 3))):
        with pytest.raises(ValueError, match=r'pose must be a finite 3x4 \[R \| t\] or \[1, 3, 4\]'):
            run(pose=bad)
    with pytest.raises(ValueError, match=r'pose must be a finite 3x4 \[R \| t\] or \[2, 3, 4\]'):
        run(pose=np.full((2, 3, 4), INF))
    with pytest.raises(ValueError, match='at least one entry'):
        run(pose=np.zeros((0, 3, 4)))
    with pytest.raises(ValueError, match='does not fit 32-bit indices'):
        run(size=(1 << 16, 1 << 15))
    with pytest.raises(ValueError, match='min_weight is NaN'):
        run(min_weight=NAN)
    for bad in (0.0, -0.1, NAN, INF):
        with pytest.raises(ValueError, match='step must be positive and finite'):
            run(step=bad)
    with pytest.raises(TypeError, match='step must be a number'):
        run(step='fine')
    for bad in (-1.0, NAN, INF):
        with pytest.raises(ValueError, match='near must be >= 0 and finite'):
            run(near=bad)
    for near, far in ((1.0, 1.0), (2.0, 1.0), (0.0, NAN)):
        with pytest.raises(ValueError, match='far must be above near'):
            run(near=near, far=far)
    with pytest.raises(ValueError, match='step 1e-06 is too small'):
        run(step=1e-6)
    # every argument in order, and still no CPU fallback
    for kwargs in ({}, dict(pose=np.stack([IDENTITY] * 3), min_weight=0.5, step=0.01, near=0.1, far=5.0,
                            with_normals=False)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            run(**kwargs)
    rig = simple_rig(64, 48)
    with pytest.raises(TypeError, match='volume must be a TsdfVolume'):
        rig.raycast(None)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rig.raycast(volume, IDENTITY, step=0.01)
    parameters = inspect.signature(pds.TsdfVolume.raycast).parameters
    assert [(n, p.default) for n, p in parameters.items()][1:] == [
        ('camera', inspect.Parameter.empty), ('size', inspect.Parameter.empty), ('pose', None), ('min_weight', 1.0),
        ('step', None), ('near', 0.0), ('far', INF), ('with_normals', True)]
    assert list(inspect.signature(pds.TsdfVolume.rays).parameters) == ['self', 'pose', 'batch']
    parameters = inspect.signature(pds.StereoRig.raycast).parameters
    assert [(n, p.default) for n, p in list(parameters.items())[1:3]] == [('volume', inspect.Parameter.empty),
                                                                          ('pose', None)]
    assert list(parameters.values())[3].kind is inspect.Parameter.VAR_KEYWORD
    for phrase in ('empty-space skipping', 'refinement beyond the one linear step', 'colour', 'a\nsparse volume',
                   'pose estimation', 'no CPU fallback', 'truncation / 2'):
        assert phrase in raycast_module.__doc__, phrase
    assert 'tsdf_raycast.py' in pds.tsdf.__doc__ and 'raycasting' in pds.tsdf.__doc__


def test_rays_on_a_hand_pose():
    volume = HostVolume((1.0, 2.0, 3.0), 0.5, (2, 2, 2), 1.0)
    turn = np.array([[0.0, -1.0, 0.0, 10.0], [1.0, 0.0, 0.0, 20.0], [0.0, 0.0, 1.0, 30.0]])
    rows = volume.rays(np.stack([IDENTITY, turn]), 2)
    assert rows.shape == (2, 21) and rows.dtype == np.float64
    # the identity: M = 1 / voxel_size, o = -origin / voxel_size - 0.5
    assert rows[0].tolist() == [2.0, 0, 0, 0, 2.0, 0, 0, 0, 2.0, -2.5, -4.5, -6.5] + np.eye(3).reshape(-1).tolist()
    # the turn: R^T = [[0, 1, 0], [-1, 0, 0], [0, 0, 1]]; the camera centre -R^T t = (-20, 10, -30)
    assert rows[1, :9].tolist() == [0, 2.0, 0, -2.0, 0, 0, 0, 0, 2.0]
    assert rows[1, 9:12].tolist() == [(-20.0 - 1.0) / 0.5 - 0.5, (10.0 - 2.0) / 0.5 - 0.5, (-30.0 - 3.0) / 0.5 - 0.5]
    assert rows[1, 12:].tolist() == turn[:, :3].reshape(-1).tolist()
    assert volume.rays(None, 3).tolist() == [rows[0].tolist()] * 3
    # they agree with integrate's transforms: the centre of voxel (i, j, k), sent to the camera and back, is (i, j, k)
    forward = volume.transforms(turn, 1)[0]
    p = forward[:9].reshape(3, 3) @ [1.0, 0.0, 1.0] + forward[9:]
    assert np.allclose(rows[1, :9].reshape(3, 3) @ p + rows[1, 9:12], [1.0, 0.0, 1.0], rtol=0, atol=1e-12)
    # and the test's own mirror
    M, o, R = as_the_kernel_sees((1.0, 2.0, 3.0), 0.5, turn)
    assert np.array_equal(np.concatenate([M.reshape(-1), o, R.reshape(-1)]), rows[1])


def test_depth_to_disparity_round_trip_on_the_cpu():
    Q = q_of(4, 5, 64.0, 0.125)
    d = torch.tensor([[8.0, 4.0, NAN, 16.0, 0.5]])
    depth = 64.0 * 0.125 / d
    back = pds.depth_to_disparity(depth, Q)
    assert back.dtype == torch.float32 and torch.equal(torch.isnan(back), torch.isnan(d))
    assert torch.equal(back[~torch.isnan(back)], d[~torch.isnan(d)])   # (dyadic: exact)
    # through the oracle of reproject's depth
    image = pds.depth_to_disparity(torch.full((4, 5), 1.15625), Q).numpy()
    assert np.abs(oracle_depth(image, f32(Q)) - 1.15625).max() <= 1e-6
    # a depth that is not positive becomes NaN; a matrix with an offset b: Z = f / (a d + b)
    assert torch.isnan(pds.depth_to_disparity(torch.tensor([0.0, -1.0, INF]), Q)[:2]).all()
    shifted = Q.copy()
    shifted[3, 3] = 0.5
    assert pds.depth_to_disparity(torch.tensor([2.0], dtype=torch.float64), shifted).tolist() == [(64.0 / 2.0 - 0.5) / 8.0]
    assert pds.depth_to_disparity(torch.tensor([200.0]), shifted).isnan().all()   # (its disparity would be negative)
    with pytest.raises(ValueError, match='canonical rectified form'):
        pds.depth_to_disparity(depth, np.eye(4))
    flat = Q.copy()
    flat[3, 2] = 0.0
    with pytest.raises(ValueError, match='the same depth'):
        pds.depth_to_disparity(depth, flat)
    with pytest.raises(TypeError, match='depth must be a torch.Tensor'):
        pds.depth_to_disparity(depth.numpy(), Q)
    with pytest.raises(TypeError, match='floating-point'):
        pds.depth_to_disparity(torch.ones(2, dtype=torch.int32), Q)
