"""Cost of the TSDF raycast (pds_tsdf_raycast_fwd: tsdf_raycast) against the composition a user had before it.

960x540 rendered from 256 x 256 x 128 voxels of 5 mm with a truncation of 20 mm, the scene of tools/bench_tsdf.py (a
slanted wall 1.1 .. 1.7 m away, integrated once), from the integration pose, step = truncation / 2.  The composition is the
same march in torch: the slab clip per pixel, then per step one `grid_sample` of the tsdf and one of the observed mask
(trilinear, align_corners) and `where` on the whole image, for as many steps as the longest ray has; depth only.  Same
inputs for both paths, in the same run: after a warm-up, `calls` calls in one region between two device events, the paths
taking turns region by region; the median of the regions, per call.  The kernel alone comes from the library's launch
probe (HIP events around the launch).  The shader clock is read before the timed loops.

    python tools/bench_raycast.py [regions] [calls]
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import practicaldeepstereo_nips2018_amd as pds  # noqa: E402
from tools.bench_tsdf import kernel_times, median, region  # noqa: E402


def composed_raycast(tsdf, weight, rows, camera, size, step, min_weight, steps):
    """Depth [H, W] of the same march in torch; rows: M (9), o (3) on the device."""
    nz, ny, nx = tsdf.shape
    dev = tsdf.device
    width, height = size
    fx, fy, cx, cy, skew = camera
    py, px = torch.meshgrid(torch.arange(height, device=dev, dtype=torch.float32),
                            torch.arange(width, device=dev, dtype=torch.float32), indexing='ij')
    y = (py - cy) / fy
    x = (px - cx - skew * y) / fx
    direction = torch.stack([x, y, torch.ones_like(x)], dim=-1)
    M, o = rows[:9].view(3, 3), rows[9:12]
    d = direction @ M.T
    top = torch.tensor([nx - 1.0, ny - 1.0, nz - 1.0], device=dev)
    t0, t1 = (0.0 - o) / d, (top - o) / d
    s0 = torch.minimum(t0, t1).amax(dim=-1).clamp(min=0.0)
    s1 = torch.maximum(t0, t1).amin(dim=-1)
    volume = tsdf[None, None]
    observed = (weight >= min_weight).to(torch.float32)[None, None]
    scale = 2.0 / top
    nan = torch.full_like(s0, float('nan'))
    depth, done = nan.clone(), ~(s0 <= s1)
    prev_ok, s_prev, v_prev = torch.zeros_like(done), torch.zeros_like(s0), torch.zeros_like(s0)
    for m in range(steps):
        s = s0 + m * step
        done = done | ~(s <= s1)
        grid = ((o + s[..., None] * d) * scale - 1.0)[None, None]
        v = torch.nn.functional.grid_sample(volume, grid, mode='bilinear', align_corners=True)[0, 0, 0]
        seen = torch.nn.functional.grid_sample(observed, grid, mode='bilinear', align_corners=True)[0, 0, 0] > 0.9999
        negative = seen & (v < 0) & ~done
        depth = torch.where(negative & prev_ok, s_prev + step * v_prev / (v_prev - v), depth)
        done = done | negative
        prev_ok, s_prev, v_prev = seen & ~negative, s, v
    return depth


def main():
    regions = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dev = torch.device('cuda:0')
    try:
        print('device: %s, shader clock now %s MHz' % (torch.cuda.get_device_name(dev), torch.cuda.clock_rate(dev)))
    except Exception as e:   # (the clock query needs amdsmi)
        print('device: %s (clock query unavailable: %s)' % (torch.cuda.get_device_name(dev), type(e).__name__))
    width, height = 960, 540
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
    geometry = dict(origin=(-0.64, -0.64, 1.0), voxel_size=0.005, dims=(256, 256, 128), truncation=0.02)
    volume = pds.TsdfVolume(device=dev, **geometry).integrate(d, Q, pose=pose)
    step = 0.5 * geometry['truncation']
    rows = torch.from_numpy(volume.rays(pose, 1)[0].astype(np.float32)).to(dev)
    diagonal = geometry['voxel_size'] * math.sqrt(255.0 ** 2 + 255.0 ** 2 + 127.0 ** 2)
    steps = int(diagonal / step) + 2

    ours = volume.raycast(camera, (width, height), pose=pose)
    theirs = composed_raycast(volume.tsdf, volume.weight, rows, camera, (width, height), step, 1.0, steps)
    torch.cuda.synchronize()
    hit, also = ~ours.depth[0].isnan(), ~theirs.isnan()
    both = hit & also
    print('raycast 960x540 from 256 x 256 x 128: %.1f %% of the pixels hit; the composition disagrees on %d pixels (hit '
          'or miss) and by at most %.2g m on the others; against the integrated depth the median error is %.2g m' %
          (100.0 * float(hit.float().mean()), int((hit != also).sum()),
           float((ours.depth[0] - theirs)[both].abs().max()),
           float((ours.depth[0] - pds.reproject(d, Q, depth_only=True)[0]).abs()[hit].nanmedian())))
    paths = {'raycast': lambda: volume.raycast(camera, (width, height), pose=pose),
             'raycast, no normals': lambda: volume.raycast(camera, (width, height), pose=pose, with_normals=False),
             'composition (no normals)': lambda: composed_raycast(volume.tsdf, volume.weight, rows, camera,
                                                                  (width, height), step, 1.0, steps)}
    for fn in paths.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    kernels = []
    for _ in range(regions):
        for name, fn in paths.items():
            times[name].append(region(fn, 1 if name.startswith('composition') else calls))
        kernels.append(kernel_times(b'tsdf_raycast', paths['raycast'], 1))
    for name in paths:
        line = '  %-26s %9.1f us per call (min %9.1f)' % (name, median(times[name]), min(times[name]))
        if name == 'raycast':
            line += '   kernel: tsdf_raycast %.1f us' % median([k[0] for k in kernels])
        print(line)
    print('  composition / raycast, no normals: %.1f x (%d steps of the composition)' %
          (median(times['composition (no normals)']) / median(times['raycast, no normals']), steps))


if __name__ == '__main__':
    main()
