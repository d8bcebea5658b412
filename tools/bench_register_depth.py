"""Cost of depth registration (pds_register_depth_fwd: clear, scatter, resolve) against the composition a user had
before it: reproject with the composed matrix, the projection through the distortion model in torch, and
scatter_reduce_(..., 'amin') into the target -- which yields the depth only, not the source pixel that won.

960x540 on a plane scene with 2 % outliers and NaN / inf holes (tools/bench_speckle.py), registered into the raw left
camera of a distorting rig (tools/bench_rectify.py: 960x540 -> 960x540), batch 1 and 4, splat 1 and 2 (the composition
has splat 1 only), and batch 4 into a 1280x720 third camera.  Same inputs for both paths, in the same run: after a
warm-up, `calls` calls in one region between two device events, the paths taking turns region by region; the median of
the regions, per call.  The kernels of the new path alone come from the library's launch probe (HIP events around each
launch).  Inputs are seeded.

    python tools/bench_register_depth.py [regions] [calls]
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import practicaldeepstereo_nips2018_amd as pds  # noqa: E402
from practicaldeepstereo_nips2018_amd import _lib, registration  # noqa: E402
from tools.bench_rectify import rig_for  # noqa: E402
from tools.bench_speckle import plane_scene  # noqa: E402

HBM_BYTES_PER_SECOND = 6.3e12


def algorithmic_bytes(sources, kept, targets, splat):
    """4 B of disparity per source pixel, 8 B per atomic (splat^2 per kept source), and per target pixel 8 B cleared,
    8 B read and 9 B written (depth, index, valid) by the resolve."""
    return sources * 4 + kept * 8 * splat * splat + targets * (8 + 8 + 9)


def composition(d, composed, camera, distortion, size):
    """Depth only, splat 1: the nearest of the points that round to a target pixel."""
    fx, fy, cx, cy, skew = camera
    k1, k2, p1, p2, k3 = distortion
    width, height = size
    points = pds.reproject(d, composed)
    X, Y, Z = points[..., 0], points[..., 1], points[..., 2]
    x, y = X / Z, Y / Z
    r2 = x * x + y * y
    kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * kr + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * kr + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    u = torch.floor(fx * xd + skew * yd + cx + 0.5)
    v = torch.floor(fy * yd + cy + 0.5)
    keep = (Z > 0) & (1.0 + 3.0 * k1 * r2 + 5.0 * k2 * r2 * r2 + 7.0 * k3 * r2 * r2 * r2 > 0) & \
           (u >= 0) & (u < width) & (v >= 0) & (v < height)
    batch = d.shape[0]
    entry = torch.arange(batch, device=d.device).view(batch, 1, 1) * (width * height)
    flat = (entry + v.long() * width + u.long())[keep]
    out = torch.full((batch * height * width,), float('inf'), device=d.device)
    out.scatter_reduce_(0, flat, Z[keep], 'amin')
    return torch.where(torch.isinf(out), torch.full_like(out, float('nan')), out).view(batch, height, width)


def kernel_times(fn):
    """Microseconds of the scatter and resolve launches of one call (the launch probe)."""
    lib = _lib.load()
    _lib.check(lib.pds_probe_begin(b'register_depth', 8), 'pds_probe_begin')
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        ms = (ctypes.c_float * 8)()
        count = lib.pds_probe_end(ms, None, 8)
    assert count == 2, count
    return [t * 1e3 for t in ms[:2]]


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
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    dev = torch.device('cuda:0')
    try:
        print('device: %s, shader clock now %s MHz' % (torch.cuda.get_device_name(dev), torch.cuda.clock_rate(dev)))
    except Exception as e:   # (the clock query needs amdsmi)
        print('device: %s (clock query unavailable: %s)' % (torch.cuda.get_device_name(dev), type(e).__name__))
    width, height = 960, 540
    rig = rig_for(width, height)
    matrix = rig.reprojection_matrix('rectified')
    K3 = np.array([[930.0, 0.0, 639.5], [0.0, 930.0, 359.5], [0.0, 0.0, 1.0]])
    third = (K3, rig.D1, pds.rectification.rodrigues([0.01, -0.02, 0.005]), np.array([0.03, -0.05, 0.01]), (1280, 720))
    for batch, target_name, target in ((1, 'raw left 960x540', rig.registration_target('left')),
                                       (4, 'raw left 960x540', rig.registration_target('left')),
                                       (4, 'third camera 1280x720', rig.registration_target(camera=third))):
        pose, camera, distortion, size = target
        d = torch.from_numpy(np.stack([plane_scene(height, width, b) for b in range(batch)])).to(dev)
        composed = registration.compose(pose, matrix)
        paths = {'register_depth splat 1': lambda: pds.register_depth(d, matrix, pose, camera, distortion, size),
                 'register_depth splat 2': lambda: pds.register_depth(d, matrix, pose, camera, distortion, size, splat=2),
                 'composition (depth only)': lambda: composition(d, composed, camera.tolist(), distortion.tolist(), size)}
        ours = paths['register_depth splat 1']()
        theirs = paths['composition (depth only)']()
        torch.cuda.synchronize()
        differ = int(((ours.depth != theirs) & ~(torch.isnan(ours.depth) & torch.isnan(theirs))).sum())
        kept = int((~torch.isnan(pds.reproject(d, composed, depth_only=True))).sum())
        for fn in paths.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in paths}
        kernels = {name: [] for name in list(paths)[:2]}
        for _ in range(regions):
            for name, fn in paths.items():
                times[name].append(region(fn, calls))
            for name in kernels:
                kernels[name].append(kernel_times(paths[name]))
        targets = batch * size[0] * size[1]
        print('batch %d -> %s: %d of %d source pixels kept, %.1f %% of the target hit; %d target pixels differ from the '
              'composition (fp32 rounding at pixel borders)' %
              (batch, target_name, kept, d.numel(), 100.0 * float(ours.valid.float().mean()), differ))
        for name in paths:
            line = '  %-26s %8.1f us per call (min %8.1f)' % (name, median(times[name]), min(times[name]))
            if name in kernels:
                scatter, resolve = (median([k[i] for k in kernels[name]]) for i in range(2))
                nbytes = algorithmic_bytes(d.numel(), kept, targets, 1 if name.endswith('1') else 2)
                line += '   kernels: scatter %.1f us, resolve %.1f us; model %.1f MB (HBM floor %.1f us)' % (
                    scatter, resolve, nbytes / 1e6, nbytes / HBM_BYTES_PER_SECOND * 1e6)
            print(line)
        for name in list(paths)[:2]:
            print('  composition / %s: %.2f x' % (name, median(times['composition (depth only)']) / median(times[name])))


if __name__ == '__main__':
    main()
