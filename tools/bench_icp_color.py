"""Cost of the geometric plus photometric ICP system (pds_icp_color_system_fwd) beside the Huber-weighted geometric one
(pds_icp_system_robust_fwd) and the unweighted one (pds_icp_system_fwd), of the intensity pyramid
(pds_intensity_pyramid_fwd) for 1 and 3 levels, and of one `ColorTsdfVolume.track_color` beside one `track_pyramid` on the
same frame.

The scene of tools/bench_tracking_pyramid.py with a textured image: a 960x540 frame against 256 x 256 x 128 voxels of 5 mm,
integrated once with its image, the frame a few milliradians and millimetres away.  After a warm-up, `calls` calls in one
region between two device events, the paths taking turns region by region; the median of the regions, per call.  The
tracking loops are timed one call per region with `tolerance=0`, so that every iteration runs.  The kernel alone comes from
the library's launch probe.  The shader clock is read before the timed loops.  No hardware counter is collected.

`icp_system` and `icp_system_robust` are here to be read beside tools/bench_tracking_pyramid.py of the commit before, run in
the same session: icp.hip's kernels are the same code, and the figures should say so.

    python tools/bench_icp_color.py [regions] [calls]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import practicaldeepstereo_nips2018_amd as pds  # noqa: E402
from practicaldeepstereo_nips2018_amd import _lib, tracking  # noqa: E402
from tools.bench_tsdf import kernel_times, median, region  # noqa: E402


def main():
    regions = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device('cuda:0')
    try:
        print('device: %s, shader clock now %s MHz' % (torch.cuda.get_device_name(dev), torch.cuda.clock_rate(dev)))
    except Exception as e:   # (the clock query needs amdsmi)
        print('device: %s (clock query unavailable: %s)' % (torch.cuda.get_device_name(dev), type(e).__name__))
    print('library: %s' % _lib.LIB_PATH)
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
    texture = 128.0 + 50.0 * np.sin((xx + 0.3 * yy) / 9.0) + 40.0 * np.sin((yy - 0.2 * xx) / 7.0)
    picture = torch.from_numpy(np.clip(np.stack([texture, texture + 10.0, texture - 10.0], axis=-1), 0, 255)
                               .astype(np.uint8)[None]).to(dev)
    pose = np.hstack([pds.rectification.rodrigues(np.array([0.02, -0.03, 0.01])), [[0.01], [-0.02], [0.02]]])
    geometry = dict(origin=(-0.64, -0.64, 1.0), voxel_size=0.005, dims=(256, 256, 128), truncation=0.02)
    transform = np.hstack([pds.rectification.rodrigues(np.array([0.002, -0.003, 0.001])), [[0.002], [-0.001], [0.003]]])
    moved = tracking.compose(tracking.invert(transform), pose)
    max_distance = 2 * geometry['truncation']
    huber = 0.25 * geometry['truncation']
    volume = pds.ColorTsdfVolume(device=dev, **geometry).integrate(d, Q, pose=pose, image=picture)
    model = volume.raycast(camera, (width, height), pose=pose)

    paths = {'icp_system': lambda: pds.icp_system(d, Q, model, camera, transform=transform, max_distance=max_distance),
             'icp_system_robust': lambda: pds.icp_system_robust(d, Q, model, camera, huber, transform=transform,
                                                                max_distance=max_distance),
             'track_pyramid, 1 level, 10 iterations': lambda: volume.track_pyramid(d, Q, moved, levels=1, iterations=10,
                                                                                   tolerance=0.0)}
    intensity = pds.intensity_pyramid(picture, 1)[0]
    model_intensity = pds.intensity_pyramid(model.colors, 1, layout='nhwc')[0]
    paths.update({
        'intensity_pyramid, 1 level': lambda: pds.intensity_pyramid(picture, 1),
        'intensity_pyramid, 3 levels': lambda: pds.intensity_pyramid(picture, 3),
        'icp_color_system': lambda: pds.icp_color_system(d, intensity, Q, model, model_intensity, camera,
                                                         transform=transform, max_distance=max_distance),
        'icp_color_system, both Huber': lambda: pds.icp_color_system(d, intensity, Q, model, model_intensity, camera,
                                                                     transform=transform, max_distance=max_distance,
                                                                     huber=huber, color_huber=10.0),
        'track_color, 1 level, 10 iterations': lambda: volume.track_color(d, picture, Q, moved, levels=1, iterations=10,
                                                                          tolerance=0.0)})
    for name, fn in paths.items():
        if name.startswith('track'):
            t = fn()
            print('%s: status %s, %d systems, %d inliers, rmse %.2g' % (name, t.status.tolist(), t.iterations, t.inliers[0],
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
            kernels[name].append(kernel_times(b'intensity_pyramid' if name.startswith('intensity') else b'icp_', paths[name],
                                              1 if name.startswith('intensity') else 2))
    for name in paths:
        line = '  %-40s %9.1f us per call (min %9.1f)' % (name, median(times[name]), min(times[name]))
        if name in kernels:
            line += '   kernels: %s us' % ', '.join('%.1f' % median([k[i] for k in kernels[name]])
                                                    for i in range(len(kernels[name][0])))
        print(line)


if __name__ == '__main__':
    main()
