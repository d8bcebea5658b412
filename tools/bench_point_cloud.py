"""Cost of the packed point cloud (pds_point_cloud_fwd: count, scan, scatter) against the composition a user had before
it:  reproject, then ~isnan, then boolean indexing of the points and of the permuted image, then nonzero.

960x540, batch 1, on a plane scene with 2 % outliers and NaN / inf holes (tools/bench_speckle.py) and on a map in which
every pixel is kept; colours from a uint8 [B, H, W, 3] image and from a float32 [B, 3, H, W] one (what
StereoRig.reconstruct hands on).  Same inputs and the same timing for both paths, interleaved, median of the repeats
after a warm-up:
  * device  device events around the call (the GPU's view: launches, gaps and hidden synchronisations included)
  * host    time.perf_counter around the call and a device synchronise behind it (what a caller waits for)
  * kernels the three launches of the new path alone, from the library's launch probe (HIP events around each launch)
Inputs are seeded.

    python tools/bench_point_cloud.py [reps]
    python tools/bench_point_cloud.py launches    # every case ten times and nothing else: run this form under
                                                   # rocprofv3 --kernel-trace --stats for the kernel times
"""
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import practicaldeepstereo_nips2018_amd as pds  # noqa: E402
from practicaldeepstereo_nips2018_amd import _lib  # noqa: E402
from tools.bench_rectify import rig_for, timed  # noqa: E402
from tools.bench_speckle import plane_scene  # noqa: E402

HBM_BYTES_PER_SECOND = 6.3e12


def algorithmic_bytes(pixels, kept, colour_bytes):
    """The new path: the disparity is read twice (count, scatter), 4 B each; per kept point the colour is gathered
    (3 * colour_bytes) and xyz (12 B), rgb (3 * colour_bytes) and the index (4 B) are written; 4 B per tile of 1024
    pixels are written, read, written and read again."""
    return pixels * 8 + kept * (12 + 6 * colour_bytes + 4) + (pixels + 1023) // 1024 * 16


def composition_bytes(pixels, kept, colour_bytes):
    """The least the torch composition moves: reproject reads 4 B and writes 12 B per pixel; ~isnan reads the x of every
    point (whole lines: 12 B) and writes 1 B; each of the two boolean indexings and nonzero reads the mask (1 B) and
    writes int64 indices (8 B per kept point and dimension: 3 for the mask's nonzero), the indexings then gather
    (12 B / 3 * colour_bytes read, the same written)."""
    return pixels * (4 + 12 + 12 + 1 + 3) + kept * (3 * 24 + 24 + 6 * colour_bytes)


def composition(d, matrix, image_nhwc):
    points = pds.reproject(d, matrix)
    keep = ~torch.isnan(points[..., 0])
    return points[keep], image_nhwc[keep], keep.nonzero()


def cases_of(dev):
    width, height = 960, 540
    matrix = rig_for(width, height).Q
    g = torch.Generator().manual_seed(1)
    bytes_ = torch.randint(0, 256, (1, height, width, 3), generator=g, dtype=torch.uint8).to(dev)
    floats = (torch.rand(1, 3, height, width, generator=g) * 255).to(dev)
    maps = {'plane scene': torch.from_numpy(plane_scene(height, width, 0)[None]).to(dev),
            'all kept': (torch.rand(1, height, width, generator=g) * 100 + 5).to(dev)}
    cases = {}
    for scene, d in maps.items():
        for colour, image in (('u8', bytes_), ('f32', floats)):
            nhwc = image if image.dtype == torch.uint8 else image.permute(0, 2, 3, 1)
            name = '%-11s %s' % (scene, colour)
            cases[name] = {
                'point_cloud trim=False': lambda d=d, image=image: pds.point_cloud(d, matrix, image=image,
                                                                                   with_index=True, trim=False),
                'point_cloud trim=True': lambda d=d, image=image: pds.point_cloud(d, matrix, image=image,
                                                                                  with_index=True),
                'composition': lambda d=d, nhwc=nhwc: composition(d, matrix, nhwc),
                'pixels': d.numel(), 'colour_bytes': image.element_size(),
                'kept': int(pds.point_cloud(d, matrix).offsets[-1]),
            }
    return cases


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def kernel_times(fn):
    """Microseconds of the count, scan and scatter launches of one call (the launch probe)."""
    lib = _lib.load()
    _lib.check(lib.pds_probe_begin(b'point_cloud', 8), 'pds_probe_begin')
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        ms = (ctypes.c_float * 8)()
        count = lib.pds_probe_end(ms, None, 8)
    assert count == 3, count
    return [t * 1e3 for t in ms[:3]]


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def main():
    dev = torch.device('cuda:0')
    cases = cases_of(dev)
    paths = ('point_cloud trim=False', 'point_cloud trim=True', 'composition')
    if len(sys.argv) > 1 and sys.argv[1] == 'launches':
        for case in cases.values():
            for path in paths:
                for _ in range(10):
                    case[path]()
        torch.cuda.synchronize()
        return
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
            kernels.append(kernel_times(case['point_cloud trim=False']))
        new_bytes = algorithmic_bytes(case['pixels'], case['kept'], case['colour_bytes'])
        old_bytes = composition_bytes(case['pixels'], case['kept'], case['colour_bytes'])
        print('%s: %d of %d pixels kept; model %.2f MB (%.1f B/pixel, HBM floor %.2f us) against %.2f MB (%.1f B/pixel) of '
              'the composition' % (name, case['kept'], case['pixels'], new_bytes / 1e6, new_bytes / case['pixels'],
                                   new_bytes / HBM_BYTES_PER_SECOND * 1e6, old_bytes / 1e6, old_bytes / case['pixels']))
        for path in paths:
            print('  %-24s device %8.1f us (min %8.1f)   host %8.1f us (min %8.1f)' %
                  (path, median(device[path]), min(device[path]), median(host[path]), min(host[path])))
        count, scan, scatter = (median([k[i] for k in kernels]) for i in range(3))
        print('  kernels (event pairs): count %.1f us, scan %.1f us, scatter %.1f us, sum %.1f us' %
              (count, scan, scatter, count + scan + scatter))
        for path in paths[:2]:
            print('  composition / %s: device %.2f x, host %.2f x' %
                  (path, median(device['composition']) / median(device[path]),
                   median(host['composition']) / median(host[path])))


if __name__ == '__main__':
    main()
