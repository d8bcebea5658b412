"""Cost of the TSDF mesh (pds_tsdf_mesh_fwd: tsdf_mesh_count, _scan, _scatter, _face_count, _face_scan, _face_scatter)
beside extract_points and integrate on the same volume, in the same run.

The 256^3 volume and the 960x540 frame of tools/bench_tsdf.py: a slanted wall 1.1 .. 1.7 m away that runs through the
volume.  After a warm-up, `calls` calls in one region between two device events, the paths taking turns region by region;
the median of the regions, per call.  The kernels alone come from the library's launch probe (HIP events around each
launch).  The shader clock is read before the timed loops.  Not here: the same faces composed in torch (joining faces to
vertices needs a sort or a dense map of 7 ints per voxel there; it was not written).

    python tools/bench_tsdf_mesh.py [regions] [calls]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import practicaldeepstereo_nips2018_amd as pds  # noqa: E402
from tools.bench_tsdf import HBM_BYTES_PER_SECOND, extract_bytes, kernel_times, median, region  # noqa: E402


def mesh_bytes(voxels, vertices, faces):
    """count and scatter each read tsdf and weight once from memory (the neighbours come from the caches) and the scatter
    writes 5 B of record per voxel; the face passes each read tsdf and weight once more and the face scatter reads the
    records of the tiles that hold faces (at most all: 5 B per voxel); per vertex 28 B, per face 12 B."""
    return 4 * voxels * 8 + 2 * voxels * 5 + vertices * 28 + faces * 12


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
    pose = np.hstack([pds.rectification.rodrigues(np.array([0.02, -0.03, 0.01])), [[0.01], [-0.02], [0.02]]])
    geometry = dict(origin=(-0.64, -0.64, 1.0), voxel_size=0.005, dims=(n, n, n), truncation=0.02)
    volume = pds.TsdfVolume(device=dev, **geometry)
    for _ in range(4):
        volume.integrate(d, Q, pose=pose)
    voxels = n ** 3
    capacity, face_capacity = 1 << 22, 1 << 23
    surface = volume.extract_mesh(capacity=capacity, face_capacity=face_capacity)
    cloud = volume.extract_points(capacity=1 << 21)
    vertices, faces, points = surface.mesh.points.shape[0], surface.mesh.faces.shape[0], cloud.cloud.points.shape[0]
    print('extract_mesh from %d^3: %d vertices, %d faces (%.2f per vertex); extract_points finds %d points' %
          (n, vertices, faces, faces / max(vertices, 1), points))
    paths = {'integrate': lambda: volume.integrate(d, Q, pose=pose),
             'extract_points, trim=False': lambda: volume.extract_points(capacity=1 << 21, trim=False),
             'extract_mesh': lambda: volume.extract_mesh(capacity=capacity, face_capacity=face_capacity),
             'extract_mesh, trim=False': lambda: volume.extract_mesh(capacity=capacity, face_capacity=face_capacity,
                                                                     trim=False),
             'extract_mesh, no normals': lambda: volume.extract_mesh(capacity=capacity, face_capacity=face_capacity,
                                                                     with_normals=False, trim=False)}
    for fn in paths.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    kernels, yardstick, fusion = [], [], []
    for _ in range(regions):
        for name, fn in paths.items():
            times[name].append(region(fn, calls))
        kernels.append(kernel_times(b'tsdf_mesh', paths['extract_mesh, trim=False'], 6))
        yardstick.append(kernel_times(b'tsdf_extract', paths['extract_points, trim=False'], 3))
        fusion.append(kernel_times(b'tsdf_', paths['integrate'], 2))
    names = ('count', 'scan', 'scatter', 'face_count', 'face_scan', 'face_scatter')
    for name in paths:
        print('  %-28s %9.1f us per call (min %9.1f)' % (name, median(times[name]), min(times[name])))
    print('  kernels of extract_mesh:   ' + ', '.join('%s %.1f us' % (names[k], median([r[k] for r in kernels]))
                                                      for k in range(6)))
    print('  kernels of extract_points: ' + ', '.join('%s %.1f us' % (names[k], median([r[k] for r in yardstick]))
                                                      for k in range(3)))
    print('  kernels of integrate:      tsdf_depth %.1f us, tsdf_integrate %.1f us' %
          (median([r[0] for r in fusion]), median([r[1] for r in fusion])))
    nbytes, base = mesh_bytes(voxels, vertices, faces), extract_bytes(voxels, points)
    print('  model: extract_mesh touches %.1f MB (HBM floor %.1f us), extract_points %.1f MB (HBM floor %.1f us)' %
          (nbytes / 1e6, nbytes / HBM_BYTES_PER_SECOND * 1e6, base / 1e6, base / HBM_BYTES_PER_SECOND * 1e6))


if __name__ == '__main__':
    main()
