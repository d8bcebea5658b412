"""Cost of the disparity pyramid (pds_disparity_pyramid_fwd), of the Huber-weighted ICP system
(pds_icp_system_robust_fwd) beside the unweighted one, and of one coarse-to-fine `TsdfVolume.track_pyramid` beside the single-level
loop on the same frame.

The scene of tools/bench_icp.py: a 960x540 frame against 256 x 256 x 128 voxels of 5 mm, integrated once, the frame a few
milliradians and millimetres away.  After a warm-up, `calls` calls in one region between two device events, the paths taking
turns region by region; the median of the regions, per call.  `track` is timed one call per region with `tolerance=0`, so
that every level runs all its iterations: one iteration is host-bound (a launch pair, one read of 29 doubles, a 6 x 6 solve),
so a coarse iteration is not expected to be much cheaper than a fine one; the figures say what it is.  The kernel alone
comes from the library's launch probe.  The shader clock is read before the
timed loops.  No hardware counter is collected.

    python tools/bench_tracking_pyramid.py [regions] [calls]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import practicaldeepstereo_nips2018_amd as pds  # noqa: E402
from practicaldeepstereo_nips2018_amd import tracking  # noqa: E402
from tools.bench_tsdf import kernel_times, median, region  # noqa: E402


def main():
    regions = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device('cuda:0')
    try:
        print('device: %s, shader clock now %s MHz' % (torch.cuda.get_device_name(dev), torch.cuda.clock_rate(dev)))
    except Exception as e:   # (the clock query needs amdsmi)
        print('device: %s (clock query unavailable: %s)' % (torch.cuda.get_device_name(dev), type(e).__name__))
    width, height = 960, 540
    focal, baseline = 700.0, 0.12
    Q = np.array([[1.0, 0.0, 0.0, -0.5 * (width - 1)], [0.0, 1.0, 0.0, -0.5 * (height - 1)], [0.0, 0.0, 0.0, focal],
                  [0.0, 0.0, 1.0 / baseline, 0.0]])
    camera = (focal, focal, 0.5 * (width - 1), 0.5 * (height - 1), 0.0)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    depth = 1.12 + 0.5 * xx / width + 0.1 * yy / height + 0.03 * np.sin(xx / 40.0) * np.cos(yy / 30.0)
    d = focal * baseline / depth
    d[np.random.RandomState(0).rand(height, width) < 0.02] = np.nan
    d = torch.from_numpy(d.astype(np.float32)[None]).to(dev)
    pose = np.hstack([pds.rectification.rodrigues(np.array([0.02, -0.03, 0.01])), [[0.01], [-0.02], [0.02]]])
    geometry = dict(origin=(-0.64, -0.64, 1.0), voxel_size=0.005, dims=(256, 256, 128), truncation=0.02)
    volume = pds.TsdfVolume(device=dev, **geometry).integrate(d, Q, pose=pose)
    model = volume.raycast(camera, (width, height), pose=pose)
    transform = np.hstack([pds.rectification.rodrigues(np.array([0.002, -0.003, 0.001])), [[0.002], [-0.001], [0.003]]])
    moved = tracking.compose(tracking.invert(transform), pose)
    max_distance = 2 * geometry['truncation']
    huber = 0.25 * geometry['truncation']

    paths = {'disparity_pyramid, 3 levels': lambda: pds.disparity_pyramid(d, 3, tracking.DEFAULT_MAX_DIFFERENCE),
             'disparity_pyramid, 4 levels': lambda: pds.disparity_pyramid(d, 4, tracking.DEFAULT_MAX_DIFFERENCE),
             'icp_system': lambda: pds.icp_system(d, Q, model, camera, transform=transform, max_distance=max_distance),
             'icp_system_robust': lambda: pds.icp_system_robust(d, Q, model, camera, huber, transform=transform,
                                                                max_distance=max_distance),
             'track, 1 level, 10 iterations': lambda: volume.track(d, Q, moved, iterations=10, tolerance=0.0),
             'track, 3 levels, 10 iterations each': lambda: volume.track_pyramid(d, Q, moved, iterations=10, tolerance=0.0, levels=3),
             'track, 3 levels, iterations (10, 5, 4)': lambda: volume.track_pyramid(d, Q, moved, iterations=(10, 5, 4),
                                                                             tolerance=0.0, levels=3)}
    for name, fn in paths.items():
        if name.startswith('track'):
            t = fn()
            print('%s: status %s, %d systems, %d inliers, rmse %.2g m' % (name, t.status.tolist(), t.iterations, t.inliers[0],
                                                                         t.rmse[0]))
        else:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    kernels = {name: [] for name in paths if not name.startswith('track')}
    for _ in range(regions):
        for name, fn in paths.items():
            times[name].append(region(fn, 1 if name.startswith('track') else calls))
        for name in kernels:
            kernels[name].append(kernel_times(b'disparity_pyramid' if name.startswith('disparity') else b'icp_', paths[name],
                                              1 if name.startswith('disparity') else 2))
    for name in paths:
        line = '  %-40s %9.1f us per call (min %9.1f)' % (name, median(times[name]), min(times[name]))
        if name in kernels:
            line += '   kernels: %s us' % ', '.join('%.1f' % median([k[i] for k in kernels[name]])
                                                    for i in range(len(kernels[name][0])))
        print(line)


if __name__ == '__main__':
    main()
