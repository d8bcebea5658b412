"""Cost of colour in TSDF fusion (pds_tsdf_color_integrate_fwd, pds_tsdf_color_gather_fwd, pds_tsdf_color_render_fwd) beside
the plain kernels, in the manner of tools/bench_tsdf.py and on its scene: 960x540 into 256^3 voxels of 5 mm.

  (a) ColorTsdfVolume.integrate beside TsdfVolume.integrate, taking turns region by region in one session
  (b) the gather after extract_points and after extract_mesh
  (c) the render after raycast
  (d) the same coloured integration composed in torch

After a warm-up, `calls` calls in one region between two device events, the paths taking turns; the median of the regions,
per call.  The kernels alone come from the library's launch probe.  The shader clock is read before the timed loops.
Whether the plain kernels moved against the parent commit is measured with tools/bench_tsdf.py, which both commits have,
on the two checkouts in the same session.

    python tools/bench_tsdf_color.py [regions] [calls]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import practicaldeepstereo_nips2018_amd as pds  # noqa: E402
from bench_tsdf import HBM_BYTES_PER_SECOND, composed_integrate, integrate_bytes, kernel_times, median, region  # noqa: E402


def color_integrate_bytes(pixels, updated):
    """integrate_bytes, and per UPDATED voxel 12 B of colour read and 12 B written (40 B where the plain kernel moves 16),
    and the image gathered (3 B per pixel, read once from memory)."""
    return integrate_bytes(pixels, updated) + updated * 24 + pixels * 3


def gather_bytes(rows):
    """per row 4 B of index read and 12 B of colour written; two tsdf values and two colours (32 B) gathered"""
    return rows * (4 + 12 + 32)


def render_bytes(pixels, hits):
    """per pixel 4 B of depth read and 12 B written; per hit eight weights and eight colours (128 B) gathered"""
    return pixels * 16 + hits * 128


def composed_color(color, weight, update, flat, image):
    """The colour step of one frame in torch, on the whole volume: `update` and `flat` as composed_integrate forms them."""
    x = image.reshape(-1, 3)[flat.reshape(-1)].view(color.shape).to(torch.float32)
    w = weight[..., None]
    return torch.where(update[..., None], (color * w + x) / (w + 1.0), color)


def measure(paths, regions, calls):
    for fn in paths.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    for _ in range(regions):
        for name, fn in paths.items():
            times[name].append(region(fn, calls))
    return times


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
    image = torch.from_numpy(np.random.RandomState(1).randint(0, 256, (1, height, width, 3)).astype(np.uint8)).to(dev)
    Q = np.array([[1.0, 0.0, 0.0, -0.5 * (width - 1)], [0.0, 1.0, 0.0, -0.5 * (height - 1)], [0.0, 0.0, 0.0, focal],
                  [0.0, 0.0, 1.0 / baseline, 0.0]])
    camera = (focal, focal, 0.5 * (width - 1), 0.5 * (height - 1), 0.0)
    pose = np.hstack([pds.rectification.rodrigues(np.array([0.02, -0.03, 0.01])), [[0.01], [-0.02], [0.02]]])
    geometry = dict(origin=(-0.64, -0.64, 1.0), voxel_size=0.005, dims=(n, n, n), truncation=0.02)
    plain = pds.TsdfVolume(device=dev, **geometry)
    plain_paths = {'TsdfVolume.integrate': lambda: plain.integrate(d, Q, pose=pose)}
    volume = pds.ColorTsdfVolume(device=dev, **geometry)

    # ---- (a) integrate
    paths = dict(plain_paths)
    paths['ColorTsdfVolume.integrate'] = lambda: volume.integrate(d, Q, pose=pose, image=image)
    times = measure(paths, regions, calls)
    updated = int((plain.weight > 0).sum())
    same = torch.equal(plain.tsdf, volume.tsdf) and torch.equal(plain.weight, volume.weight)
    print('integrate 960x540 into %d^3: %.1f %% of the voxels updated; tsdf and weight of the two volumes equal: %s' %
          (n, 100.0 * updated / n ** 3, same))
    for name, probe, model in (('TsdfVolume.integrate', b'tsdf_integrate', integrate_bytes),
                               ('ColorTsdfVolume.integrate', b'tsdf_color_integrate', color_integrate_bytes)):
        kernels = [kernel_times(probe, paths[name], 1)[0] for _ in range(regions)]
        nbytes = model(height * width, updated)
        print('  %-28s %9.1f us per call (min %9.1f, max %9.1f)   %s %.1f us (min %.1f, max %.1f); model %.1f MB '
              '(HBM floor %.1f us)' % (name, median(times[name]), min(times[name]), max(times[name]), probe.decode(),
                                       median(kernels), min(kernels), max(kernels), nbytes / 1e6,
                                       nbytes / HBM_BYTES_PER_SECOND * 1e6))
    print('  coloured / plain: %.2f x' % (median(times['ColorTsdfVolume.integrate']) / median(times['TsdfVolume.integrate'])))

    # ---- (d) the same integration composed in torch
    rows = torch.from_numpy(volume.transforms(pose, 1)[0].astype(np.float32)).to(dev)

    # (composed_integrate keeps its pixel indices to itself: the colour gather is paid for with indices as coherent as the
    # real ones, consecutive voxels reading consecutive pixels)
    flat = (torch.arange(n ** 3, device=dev) % (height * width)).view(volume.shape)

    def composition():
        tsdf, weight = composed_integrate(volume.tsdf, volume.weight, d, Q, rows, camera, geometry['truncation'], 64.0)
        update = weight != volume.weight
        return tsdf, weight, composed_color(volume.color, volume.weight, update, flat, image[0])

    composed = measure({'composition': composition}, max(regions // 3, 1), max(calls // 4, 1))['composition']
    print('  %-28s %9.1f us per call (min %9.1f)   composition / coloured: %.1f x' %
          ('composition in torch', median(composed), min(composed),
           median(composed) / median(times['ColorTsdfVolume.integrate'])))

    # ---- (b) the gather
    capacity, face_capacity = 1 << 21, 1 << 22
    for name, edges, extract in (('extract_points', 3, lambda **kw: volume.extract_points(capacity=capacity, trim=False, **kw)),
                                 ('extract_mesh', 7, lambda **kw: volume.extract_mesh(capacity=4 * capacity, trim=False,
                                                                                      face_capacity=face_capacity, **kw))):
        found = extract()
        rows_found = int((found.cloud if edges == 3 else found.mesh).offsets[1])
        paths = {'with colours': extract, 'without': lambda: extract(with_colors=False)}
        times = measure(paths, regions, calls)
        kernels = [kernel_times(b'tsdf_color_gather', extract, 1)[0] for _ in range(regions)]
        nbytes = gather_bytes(rows_found)
        print('%s, trim=False: %d rows' % (name, rows_found))
        print('  with colours %9.1f us per call, without %9.1f us   tsdf_color_gather %.1f us (min %.1f, max %.1f); model '
              '%.1f MB (HBM floor %.1f us)' % (median(times['with colours']), median(times['without']), median(kernels),
                                               min(kernels), max(kernels), nbytes / 1e6,
                                               nbytes / HBM_BYTES_PER_SECOND * 1e6))

    # ---- (c) the render
    cast = (lambda **kw: volume.raycast(camera, (width, height), pose=pose, **kw))
    hits = int((~cast().depth.isnan()).sum())
    times = measure({'with colours': cast, 'without': lambda: cast(with_colors=False)}, regions, calls)
    kernels = [kernel_times(b'tsdf_color_render', cast, 1)[0] for _ in range(regions)]
    marches = [kernel_times(b'tsdf_raycast', cast, 1)[0] for _ in range(regions)]
    nbytes = render_bytes(height * width, hits)
    print('raycast 960x540: %d hits' % hits)
    print('  with colours %9.1f us per call, without %9.1f us   tsdf_color_render %.1f us (min %.1f, max %.1f), tsdf_raycast '
          '%.1f us; model %.1f MB (HBM floor %.1f us)' % (median(times['with colours']), median(times['without']),
                                                          median(kernels), min(kernels), max(kernels), median(marches),
                                                          nbytes / 1e6, nbytes / HBM_BYTES_PER_SECOND * 1e6))


if __name__ == '__main__':
    main()
