"""Cost of TSDF fusion (pds_tsdf_integrate_fwd: tsdf_depth, tsdf_integrate; pds_tsdf_extract_fwd: count, scan, scatter)
against the compositions a user had before it.

960x540 into 256^3 voxels of 5 mm with a truncation of 20 mm: a slanted wall 1.1 .. 1.7 m away that runs through the
volume, so that about a quarter of the voxels lie in the band or in the free space in front of it and are updated.
integrate: the same integration composed in torch (voxel grid, projection, gather, `where` on the whole volume).
extract_points: the crossings along the three axes from comparisons, `nonzero` and gathers (points and index, no
normals).  Same inputs for both paths, in the same run: after a warm-up, `calls` calls in one region between two device
events, the paths taking turns region by region; the median of the regions, per call.  The kernels of the new path alone
come from the library's launch probe (HIP events around each launch).  The shader clock is read before the timed loops.

    python tools/bench_tsdf.py [regions] [calls]
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import practicaldeepstereo_nips2018_amd as pds  # noqa: E402
from practicaldeepstereo_nips2018_amd import _lib  # noqa: E402

HBM_BYTES_PER_SECOND = 6.3e12   # achievable, MI355X


def integrate_bytes(pixels, updated):
    """tsdf_depth: 4 B of disparity read and 4 B of Z written per pixel; tsdf_integrate: Z gathered (the map is read once
    from memory) and, per UPDATED voxel, 8 B read and 8 B written.  A skipped voxel costs arithmetic only."""
    return pixels * 8 + pixels * 4 + updated * 16


def extract_bytes(voxels, points):
    """count and scatter each read tsdf and weight once from memory (the neighbours come from the caches); per point 12 B
    of position, 12 B of normal and 4 B of index."""
    return 2 * voxels * 8 + points * 28


def composed_integrate(tsdf, weight, d, matrix, rows, camera, truncation, max_weight):
    """The integration of one frame in torch, on the whole volume."""
    nz, ny, nx = tsdf.shape
    dev = tsdf.device
    depth = pds.reproject(d, matrix, depth_only=True)[0]
    height, width = depth.shape
    A, b = rows[:9].view(3, 3), rows[9:]
    k, j, i = torch.meshgrid(torch.arange(nz, device=dev, dtype=torch.float32),
                             torch.arange(ny, device=dev, dtype=torch.float32),
                             torch.arange(nx, device=dev, dtype=torch.float32), indexing='ij')
    xc = A[0, 0] * i + A[0, 1] * j + A[0, 2] * k + b[0]
    yc = A[1, 0] * i + A[1, 1] * j + A[1, 2] * k + b[1]
    zc = A[2, 0] * i + A[2, 1] * j + A[2, 2] * k + b[2]
    fx, fy, cx, cy, skew = camera
    x, y = xc / zc, yc / zc
    px = torch.floor(fx * x + skew * y + cx + 0.5)
    py = torch.floor(fy * y + cy + 0.5)
    inside = (zc > 0) & (px >= 0) & (px < width) & (py >= 0) & (py < height)
    flat = (py.clamp(0, height - 1).long() * width + px.clamp(0, width - 1).long())
    Z = depth.reshape(-1)[flat.reshape(-1)].view(nz, ny, nx)
    sdf = Z - zc
    update = inside & ~torch.isnan(Z) & (sdf >= -truncation)
    t = torch.clamp(sdf / truncation, max=1.0)
    new_tsdf = torch.where(update, (tsdf * weight + t) / (weight + 1.0), tsdf)
    new_weight = torch.where(update, torch.clamp(weight + 1.0, max=max_weight), weight)
    return new_tsdf, new_weight


def composed_extract(tsdf, weight, origin, voxel_size, min_weight):
    """Points and index (no normals) from comparisons, nonzero and gathers."""
    nz, ny, nx = tsdf.shape
    observed, negative = weight >= min_weight, tsdf < 0
    points, index = [], []
    for a, axis in enumerate((2, 1, 0)):
        length = tsdf.shape[axis]
        here, there = [slice(None)] * 3, [slice(None)] * 3
        here[axis], there[axis] = slice(0, length - 1), slice(1, length)
        here, there = tuple(here), tuple(there)
        crossing = observed[here] & observed[there] & (negative[here] != negative[there])
        where = crossing.nonzero()
        tv, tn = tsdf[here][crossing], tsdf[there][crossing]
        r = tv / (tv - tn)
        at = where.flip(1).to(torch.float32) + 0.5
        at[:, a] += r
        points.append(origin + voxel_size * at)
        index.append(3 * ((where[:, 0] * ny + where[:, 1]) * nx + where[:, 2]) + a)
    index = torch.cat(index)
    order = torch.argsort(index)
    return torch.cat(points)[order], index[order]


def kernel_times(name, fn, expected):
    """Microseconds of the launches of one call whose names contain `name` (the launch probe)."""
    lib = _lib.load()
    _lib.check(lib.pds_probe_begin(name, 8), 'pds_probe_begin')
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        ms = (ctypes.c_float * 8)()
        count = lib.pds_probe_end(ms, None, 8)
    assert count == expected, (name, count)
    return [t * 1e3 for t in ms[:count]]


def region(fn, calls):
    """Microseconds per call of `calls` calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def main():
    regions = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device('cuda:0')
    try:
        print('device: %s, shader clock now %s MHz' % (torch.cuda.get_device_name(dev), torch.cuda.clock_rate(dev)))
    except Exception as e:   # (the clock query needs amdsmi)
        print('device: %s (clock query unavailable: %s)' % (torch.cuda.get_device_name(dev), type(e).__name__))
    width, height, n = 960, 540, 256
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    depth = 1.12 + 0.5 * xx / width + 0.1 * yy / height
    focal, baseline = 700.0, 0.12
    d = focal * baseline / depth
    d[np.random.RandomState(0).rand(height, width) < 0.02] = np.nan
    d = torch.from_numpy(d.astype(np.float32)[None]).to(dev)
    Q = np.array([[1.0, 0.0, 0.0, -0.5 * (width - 1)], [0.0, 1.0, 0.0, -0.5 * (height - 1)], [0.0, 0.0, 0.0, focal],
                  [0.0, 0.0, 1.0 / baseline, 0.0]])
    camera = (focal, focal, 0.5 * (width - 1), 0.5 * (height - 1), 0.0)
    pose = np.hstack([pds.rectification.rodrigues(np.array([0.02, -0.03, 0.01])), [[0.01], [-0.02], [0.02]]])
    geometry = dict(origin=(-0.64, -0.64, 1.0), voxel_size=0.005, dims=(n, n, n), truncation=0.02)
    volume = pds.TsdfVolume(device=dev, **geometry)
    rows = torch.from_numpy(volume.transforms(pose, 1)[0].astype(np.float32)).to(dev)
    origin = torch.tensor(geometry['origin'], device=dev)

    # ---- integrate
    volume.integrate(d, Q, pose=pose)
    ours = (volume.tsdf.clone(), volume.weight.clone())
    fresh = (torch.ones_like(ours[0]), torch.zeros_like(ours[1]))
    theirs = composed_integrate(*fresh, d, Q, rows, camera, geometry['truncation'], 64.0)
    torch.cuda.synchronize()
    updated = int((ours[1] > 0).sum())
    differ = int((ours[1] != theirs[1]).sum())
    worst = float((ours[0] - theirs[0])[ours[1] == theirs[1]].abs().max())
    voxels = n ** 3
    print('integrate 960x540 into %d^3: %.1f %% of the voxels updated; against the composition %d voxels differ in the '
          'weight (fp32 rounding at pixel borders and at the band\'s rim), the others by at most %.2g in the tsdf (a '
          'neighbouring pixel read where u + 0.5 rounds the other way)' %
          (n, 100.0 * updated / voxels, differ, worst))
    paths = {'integrate': lambda: volume.integrate(d, Q, pose=pose),
             'composition': lambda: composed_integrate(volume.tsdf, volume.weight, d, Q, rows, camera,
                                                       geometry['truncation'], 64.0)}
    for fn in paths.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    kernels = []
    for _ in range(regions):
        for name, fn in paths.items():
            times[name].append(region(fn, calls))
        kernels.append(kernel_times(b'tsdf_', paths['integrate'], 2))
    nbytes = integrate_bytes(height * width, updated)
    print('  %-12s %9.1f us per call (min %9.1f)   kernels: tsdf_depth %.1f us, tsdf_integrate %.1f us; touched %.1f MB '
          '(HBM floor %.1f us)' % ('integrate', median(times['integrate']), min(times['integrate']),
                                   median([k[0] for k in kernels]), median([k[1] for k in kernels]), nbytes / 1e6,
                                   nbytes / HBM_BYTES_PER_SECOND * 1e6))
    print('  %-12s %9.1f us per call (min %9.1f)' % ('composition', median(times['composition']),
                                                     min(times['composition'])))
    print('  composition / integrate: %.1f x' % (median(times['composition']) / median(times['integrate'])))

    # ---- extract_points (on the volume after the integrations above)
    capacity = 1 << 21
    surface = volume.extract_points(capacity=capacity)
    points, index = composed_extract(volume.tsdf, volume.weight, origin, geometry['voxel_size'], 1.0)
    torch.cuda.synchronize()
    count = surface.cloud.points.shape[0]
    same = count == index.shape[0] and bool((surface.cloud.index.long() == index).all())
    print('extract_points from %d^3: %d points; the composition finds the same index: %s' % (n, count, same))
    paths = {'extract_points': lambda: volume.extract_points(capacity=capacity),
             'extract_points, trim=False': lambda: volume.extract_points(capacity=capacity, trim=False),
             'extract_points, no normals': lambda: volume.extract_points(capacity=capacity, with_normals=False),
             'composition (no normals)': lambda: composed_extract(volume.tsdf, volume.weight, origin,
                                                                  geometry['voxel_size'], 1.0)}
    for fn in paths.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    kernels = []
    for _ in range(regions):
        for name, fn in paths.items():
            times[name].append(region(fn, calls))
        kernels.append(kernel_times(b'tsdf_extract', paths['extract_points, trim=False'], 3))
    nbytes = extract_bytes(voxels, count)
    for name in paths:
        line = '  %-28s %9.1f us per call (min %9.1f)' % (name, median(times[name]), min(times[name]))
        if name == 'extract_points, trim=False':
            line += '   kernels: count %.1f us, scan %.1f us, scatter %.1f us; model %.1f MB (HBM floor %.1f us)' % (
                median([k[0] for k in kernels]), median([k[1] for k in kernels]), median([k[2] for k in kernels]),
                nbytes / 1e6, nbytes / HBM_BYTES_PER_SECOND * 1e6)
        print(line)
    print('  composition / extract_points, no normals: %.1f x' %
          (median(times['composition (no normals)']) / median(times['extract_points, no normals'])))


if __name__ == '__main__':
    main()
