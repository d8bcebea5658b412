"""Cost of the point-to-plane ICP system (pds_icp_system_fwd: icp_rows, icp_reduce) against the composition a user had
before it, and of one whole `TsdfVolume.track`.

A 960x540 frame against a 960x540 model: the scene of tools/bench_raycast.py (a slanted wall 1.1 .. 1.7 m away in 256 x
256 x 128 voxels of 5 mm, integrated once), raycast from the integration pose; the frame is that of a camera a few
milliradians and millimetres away.  The composition is the same system in torch: `reproject`, the transform, the
projection, a gather of the model's depth and normals, the masks, and `einsum` for the 6 x 6 and 6 x 1 sums in fp64.  Same
inputs for both paths, in the same run: after a warm-up, `calls` calls in one region between two device events, the paths
taking turns region by region; the median of the regions, per call.  The kernels alone come from the library's launch
probe (HIP events around each launch).  The shader clock is read before the timed loops.  No hardware counter is
collected: which unit bounds icp_rows is not measured here.

    python tools/bench_icp.py [regions] [calls]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import practicaldeepstereo_nips2018_amd as pds  # noqa: E402
from practicaldeepstereo_nips2018_amd import tracking  # noqa: E402
from tools.bench_tsdf import kernel_times, median, region  # noqa: E402


def composed_system(d, Q, model, camera, transform, max_distance):
    """[29] fp64 of entry 0: the same system in torch."""
    dev = d.device
    fx, fy, cx, cy, skew = camera
    P = pds.reproject(d, Q)[0]
    T = torch.from_numpy(transform.astype(np.float32)).to(dev)
    q = P @ T[:, :3].T + T[:, 3]
    u = fx * q[..., 0] / q[..., 2] + skew * q[..., 1] / q[..., 2] + cx
    v = fy * q[..., 1] / q[..., 2] + cy
    px, py = torch.floor(u + 0.5), torch.floor(v + 0.5)
    height, width = model.depth.shape[1:]
    ok = (q[..., 2] > 0) & (px >= 0) & (px < width) & (py >= 0) & (py < height)
    at = torch.where(ok, py * width + px, torch.zeros_like(px)).long()
    Z = model.depth[0].reshape(-1)[at]
    n = model.normals[0].reshape(-1, 3)[at]
    ym = (py - cy) / fy
    xm = (px - cx - skew * ym) / fx
    m = torch.stack([Z * xm, Z * ym, Z], dim=-1)
    e = m - q
    ok = ok & ~Z.isnan() & ~n[..., 0].isnan() & ((e * e).sum(dim=-1) <= max_distance * max_distance)
    J = torch.cat([torch.cross(q, n, dim=-1), n], dim=-1)
    r = (n * e).sum(dim=-1)
    J = torch.where(ok[..., None], J, torch.zeros_like(J)).double().reshape(-1, 6)
    r = torch.where(ok, r, torch.zeros_like(r)).double().reshape(-1)
    A = torch.einsum('pi,pj->ij', J, J)
    g = torch.einsum('pi,p->i', J, r)
    upper = torch.triu_indices(6, 6, device=dev)
    return torch.cat([A[upper[0], upper[1]], g, (r * r).sum()[None], ok.sum()[None].double()])


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

    def frame(shift):
        depth = 1.12 + shift + 0.5 * xx / width + 0.1 * yy / height + 0.03 * np.sin(xx / 40.0) * np.cos(yy / 30.0)
        d = focal * baseline / depth
        d[np.random.RandomState(0).rand(height, width) < 0.02] = np.nan
        return torch.from_numpy(d.astype(np.float32)[None]).to(dev)

    pose = np.hstack([pds.rectification.rodrigues(np.array([0.02, -0.03, 0.01])), [[0.01], [-0.02], [0.02]]])
    geometry = dict(origin=(-0.64, -0.64, 1.0), voxel_size=0.005, dims=(256, 256, 128), truncation=0.02)
    d = frame(0.0)
    volume = pds.TsdfVolume(device=dev, **geometry).integrate(d, Q, pose=pose)
    model = volume.raycast(camera, (width, height), pose=pose)
    transform = np.hstack([pds.rectification.rodrigues(np.array([0.002, -0.003, 0.001])), [[0.002], [-0.001], [0.003]]])
    moved = tracking.compose(tracking.invert(transform), pose)   # the pose of the frame `transform` away from the model
    max_distance = 2 * geometry['truncation']

    ours = pds.icp_system(d, Q, model, camera, transform=transform, max_distance=max_distance).system[0]
    theirs = composed_system(d, Q, model, camera, transform, max_distance)
    torch.cuda.synchronize()
    scale = ours.abs().clamp(min=1.0)
    print('icp_system 960x540 against 960x540: %d rows (%.1f %% of the pixels); the composition has %d and differs by at '
          'most %.2g of a component' % (int(ours[28]), 100.0 * float(ours[28]) / (width * height), int(theirs[28]),
                                        float(((ours - theirs).abs() / scale)[:28].max())))
    paths = {'icp_system': lambda: pds.icp_system(d, Q, model, camera, transform=transform, max_distance=max_distance),
             'icp_system, with rows': lambda: pds.icp_system(d, Q, model, camera, transform=transform,
                                                             max_distance=max_distance, with_rows=True),
             'composition': lambda: composed_system(d, Q, model, camera, transform, max_distance),
             'track, 10 iterations': lambda: volume.track(d, Q, moved, iterations=10, tolerance=0.0)}
    t = paths['track, 10 iterations']()
    print('track: status %s, %d iterations, %d inliers, rmse %.2g m' % (t.status.tolist(), t.iterations, t.inliers[0],
                                                                       t.rmse[0]))
    for fn in paths.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    kernels = []
    for _ in range(regions):
        for name, fn in paths.items():
            times[name].append(region(fn, 1 if name.startswith('track') else calls))
        kernels.append(kernel_times(b'icp_', paths['icp_system'], 2))
    for name in paths:
        line = '  %-24s %9.1f us per call (min %9.1f)' % (name, median(times[name]), min(times[name]))
        if name == 'icp_system':
            line += '   kernels: icp_rows %.1f us, icp_reduce %.1f us' % (median([k[0] for k in kernels]),
                                                                         median([k[1] for k in kernels]))
        print(line)
    print('  composition / icp_system: %.1f x' % (median(times['composition']) / median(times['icp_system'])))


if __name__ == '__main__':
    main()
