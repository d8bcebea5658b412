"""Cost of the triangle mesh (pds_triangle_mesh_fwd: the cloud's three launches, face count, scan, face scatter) against
the composition a user had before it: point_cloud(with_index=True), a dense rank map scattered from `index`, six shifted
comparisons, a diagonal choice and two masks, two nonzero, two gathers of the corners, a cat, and an argsort that restores
the order.

960x540, batch 1, on a plane scene with 2 % outliers and NaN / inf holes (tools/bench_speckle.py) and on a smooth map in
which every pixel is kept.  The composition must give the kernel's faces as a set (and, after its argsort, in the kernel's
order) before anything is timed.  Same inputs and the same timing for both paths, interleaved, median of the repeats
after a warm-up:
  * device  device events around the call (the GPU's view: launches, gaps and hidden synchronisations included)
  * host    time.perf_counter around the call and a device synchronise behind it (what a caller waits for)
  * kernels the six launches of the new path alone, from the library's launch probe (HIP events around each launch)
Inputs are seeded.

    python tools/bench_triangle_mesh.py [reps]
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import practicaldeepstereo_nips2018_amd as pds  # noqa: E402
from practicaldeepstereo_nips2018_amd import _lib  # noqa: E402
from tools.bench_point_cloud import HBM_BYTES_PER_SECOND, host_timed, median  # noqa: E402
from tools.bench_rectify import rig_for, timed  # noqa: E402
from tools.bench_speckle import plane_scene  # noqa: E402

MAX_DIFFERENCE = 1.0


def algorithmic_bytes(pixels, kept, faces):
    """The new path without colours: the cloud's count and scatter read the disparity (4 B each) and the scatter writes
    xyz and the index per kept point (16 B) and the rank map (4 B per pixel); the face count and the face scatter each
    read the disparity and the rank map of their tile and of the row below it (16 B per pixel each; the row below is the
    top row of another tile, so at best half of that comes from HBM: 8 B); 12 B per face are written; 4 B per tile of
    1024 pixels are written, read, written and read again, twice."""
    return pixels * (8 + 4 + 2 * 8) + kept * 16 + faces * 12 + (pixels + 1023) // 1024 * 32


def composition(d, matrix):
    """-> (faces [F, 3] int64 in the kernel's order, the cloud), in torch on the packed cloud."""
    cloud = pds.point_cloud(d, matrix, with_index=True)
    batch, height, width = d.shape
    pixels = height * width
    rows = torch.arange(cloud.index.shape[0], device=d.device)
    entry = torch.bucketize(rows, cloud.offsets[1:].to(torch.int64), right=True)
    rank = torch.full((batch * pixels,), -1, dtype=torch.int64, device=d.device)
    rank[entry * pixels + cloud.index.to(torch.int64)] = rows
    rank = rank.view(batch, height, width)
    corner = (lambda m: (m[:, :-1, :-1], m[:, :-1, 1:], m[:, 1:, :-1], m[:, 1:, 1:]))   # a, b, c, e
    (da, db, dc, de), (ra, rb, rc, re) = corner(d), corner(rank)
    ka, kb, kc, ke = ra >= 0, rb >= 0, rc >= 0, re >= 0
    joined = (lambda kp, kq, p, q: kp & kq & ((p - q).abs() <= MAX_DIFFERENCE))
    ab, ac, ae = joined(ka, kb, da, db), joined(ka, kc, da, dc), joined(ka, ke, da, de)
    bc, be, ce = joined(kb, kc, db, dc), joined(kb, ke, db, de), joined(kc, ke, dc, de)
    diagonal_ae = torch.where(ka & kb & kc & ke, (da - de).abs() < (db - dc).abs(), ~(kb & kc))
    first = torch.where(diagonal_ae, ae & ac & ce, bc & ac & ab)
    second = torch.where(diagonal_ae, ae & be & ab, bc & ce & be)
    i1, i2 = first.reshape(-1).nonzero()[:, 0], second.reshape(-1).nonzero()[:, 0]
    flat = (lambda m, i: m.reshape(-1)[i])
    pick1, pick2 = flat(diagonal_ae, i1), flat(diagonal_ae, i2)
    f1 = torch.stack([flat(ra, i1), flat(rc, i1), torch.where(pick1, flat(re, i1), flat(rb, i1))], dim=1)
    f2 = torch.stack([torch.where(pick2, flat(ra, i2), flat(rb, i2)), torch.where(pick2, flat(re, i2), flat(rc, i2)),
                      torch.where(pick2, flat(rb, i2), flat(re, i2))], dim=1)
    order = torch.argsort(torch.cat([2 * i1, 2 * i2 + 1]))   # (cells in raster order, entries in batch order)
    return torch.cat([f1, f2])[order], cloud


def cases_of(dev):
    width, height = 960, 540
    matrix = rig_for(width, height).Q
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float32)
    smooth = (40.0 + 10.0 * np.sin(xx / 90.0) * np.cos(yy / 70.0)).astype(np.float32)
    maps = {'plane scene': torch.from_numpy(plane_scene(height, width, 0)[None]).to(dev),
            'all kept': torch.from_numpy(smooth[None]).to(dev)}
    cases = {}
    for name, d in maps.items():
        mesh = pds.triangle_mesh(d, matrix, with_index=True, max_difference=MAX_DIFFERENCE)
        faces, cloud = composition(d, matrix)
        got, want = mesh.faces.to(torch.int64), faces
        assert torch.equal(mesh.points.view(torch.int32), cloud.points.view(torch.int32))
        assert got.shape == want.shape, (name, got.shape, want.shape)
        key = (lambda f: torch.sort(f[:, 0] * (1 << 42) + f[:, 1] * (1 << 21) + f[:, 2])[0])
        assert torch.equal(key(got), key(want)), '%s: the composition and the kernel disagree as sets' % name
        assert torch.equal(got, want), '%s: the composition and the kernel disagree in order' % name
        cases[name] = {
            'triangle_mesh trim=False': lambda d=d: pds.triangle_mesh(d, matrix, with_index=True, trim=False,
                                                                      max_difference=MAX_DIFFERENCE),
            'triangle_mesh trim=True': lambda d=d: pds.triangle_mesh(d, matrix, with_index=True,
                                                                     max_difference=MAX_DIFFERENCE),
            'point_cloud trim=False': lambda d=d: pds.point_cloud(d, matrix, with_index=True, trim=False),
            'composition': lambda d=d: composition(d, matrix),
            'pixels': d.numel(), 'kept': mesh.size(), 'faces': mesh.face_count(),
        }
    return cases


def kernel_times(fn):
    """Microseconds of the six launches of one call (the launch probe): the cloud's three, then the faces' three."""
    lib = _lib.load()
    times = []
    for name in (b'point_cloud', b'triangle_mesh'):
        _lib.check(lib.pds_probe_begin(name, 8), 'pds_probe_begin')
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            ms = (ctypes.c_float * 8)()
            count = lib.pds_probe_end(ms, None, 8)
        assert count == 3, count
        times += [t * 1e3 for t in ms[:3]]
    return times


def main():
    dev = torch.device('cuda:0')
    cases = cases_of(dev)
    paths = ('triangle_mesh trim=False', 'triangle_mesh trim=True', 'point_cloud trim=False', 'composition')
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    try:
        print('device: %s, shader clock now %s MHz' % (torch.cuda.get_device_name(dev), torch.cuda.clock_rate(dev)))
    except Exception as e:   # (the clock query needs amdsmi)
        print('device: %s (clock query unavailable: %s)' % (torch.cuda.get_device_name(dev), type(e).__name__))
    for name, case in cases.items():
        for path in paths:
            for _ in range(10):
                case[path]()
        torch.cuda.synchronize()
        device = {path: [] for path in paths}
        host = {path: [] for path in paths}
        kernels = []
        for _ in range(reps):
            for path in paths:
                device[path].append(timed(case[path]))
            for path in paths:
                host[path].append(host_timed(case[path]))
            kernels.append(kernel_times(case['triangle_mesh trim=False']))
        model = algorithmic_bytes(case['pixels'], case['kept'], case['faces'])
        print('%s: %d of %d pixels kept, %d faces; model %.2f MB (%.1f B/pixel, HBM floor %.2f us)' %
              (name, case['kept'], case['pixels'], case['faces'], model / 1e6, model / case['pixels'],
               model / HBM_BYTES_PER_SECOND * 1e6))
        for path in paths:
            print('  %-26s device %8.1f us (min %8.1f)   host %8.1f us (min %8.1f)' %
                  (path, median(device[path]), min(device[path]), median(host[path]), min(host[path])))
        k = [median([t[i] for t in kernels]) for i in range(6)]
        print('  kernels (event pairs): count %.1f us, scan %.1f us, scatter + rank map %.1f us, face count %.1f us, '
              'face scan %.1f us, face scatter %.1f us, sum %.1f us' % (tuple(k) + (sum(k),)))
        for path in paths[:2]:
            print('  composition / %s: device %.2f x, host %.2f x' %
                  (path, median(device['composition']) / median(device[path]),
                   median(host['composition']) / median(host[path])))


if __name__ == '__main__':
    main()
