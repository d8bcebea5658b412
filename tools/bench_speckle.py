"""Cost of the speckle filter, timed with device events (interleaved, median of reps):
  * speckle_filter and region_sizes (pds_speckle_filter_fwd) at 960x540 and 1242x375, batch 1 and 4, on a plane scene
    with 2 % speckles (the realistic case) and on a serpentine, a checkerboard and white noise (the worst cases for the
    find loops and for the number of roots);
  * StereoRig.reconstruct with and without speckle_size against PdsNetwork.forward_left_right at 960x540, D = 192;
  * the same filter on the host: the numpy union-find of tests/test_speckle_host.py on this machine's CPU (a Python
    restatement, not an optimised CPU filter), copies not included.
Inputs are seeded.  Event times include the launch overhead of four short kernels.

    python tools/bench_speckle.py [reps]
    python tools/bench_speckle.py launches      # every filter case ten times and nothing else: run this form under
                                                # rocprofv3 --kernel-trace --stats for the per-pass kernel times
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import practicaldeepstereo_nips2018_amd as pds  # noqa: E402
from tools.bench_rectify import rig_for, timed  # noqa: E402


def plane_scene(height, width, seed):
    """A slanted plane with a step edge, 2 % single-pixel outliers, small blobs and non-finite holes."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float32)
    d = (20.0 + 0.05 * xx + 0.02 * yy).astype(np.float32)
    d[:, width // 2:] += 30.0
    outliers = rng.rand(height, width) < 0.02
    d[outliers] += (rng.rand(int(outliers.sum())) * 60 + 5).astype(np.float32)
    for _ in range(height * width // 4000):
        y, x = rng.randint(0, height), rng.randint(0, width)
        d[y:y + rng.randint(1, 5), x:x + rng.randint(1, 7)] = 150.0 + rng.rand() * 50
    for _ in range(height * width // 20000):
        y, x = rng.randint(0, height), rng.randint(0, width)
        d[y:y + rng.randint(1, 20), x:x + rng.randint(1, 30)] = np.nan
    return d


def serpentine(height, width, seed):
    d = np.full((height, width), 100.0, dtype=np.float32)
    d[0::2] = 5.0 + seed
    d[1::4, -1] = 5.0 + seed
    d[3::4, 0] = 5.0 + seed
    return d


def checkerboard(height, width, seed):
    yy, xx = np.mgrid[0:height, 0:width]
    return np.where((yy + xx + seed) % 2 == 0, 0.0, 50.0).astype(np.float32)


def noise(height, width, seed):
    return (np.random.RandomState(100 + seed).rand(height, width) * 16).astype(np.float32)


SCENES = (('plane', plane_scene, 1.0), ('serpentine', serpentine, 1.0), ('checkerboard', checkerboard, 1.0),
          ('noise md 8', noise, 8.0))


def filter_cases(dev):
    cases, host = {}, {}
    for width, height in ((960, 540), (1242, 375)):
        for batch in (1, 4):
            for name, make, md in SCENES:
                images = np.stack([make(height, width, k) for k in range(batch)])
                d = torch.from_numpy(images).to(dev)
                key = '%-12s %4dx%-3d b%d' % (name, width, height, batch)
                cases['filter ' + key] = (lambda d=d, md=md: pds.speckle_filter(d, 100, md))
                if batch == 1:
                    cases['sizes  ' + key] = (lambda d=d, md=md: pds.region_sizes(d, md))
                    host[key] = (images[0], md)
    return cases, host


def main():
    dev = torch.device('cuda:0')
    cases, host = filter_cases(dev)
    if len(sys.argv) > 1 and sys.argv[1] == 'launches':
        for fn in cases.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        return
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50

    torch.manual_seed(0)
    net = pds.PdsNetwork.default(191).eval().to(dev).freeze_weights()
    rig = rig_for(960, 540)
    g = torch.Generator().manual_seed(1)
    raw_l = torch.randint(0, 256, (1, 540, 960, 3), generator=g, dtype=torch.uint8).to(dev)
    raw_r = torch.randint(0, 256, (1, 540, 960, 3), generator=g, dtype=torch.uint8).to(dev)
    with torch.no_grad():
        left, right = rig.rectify(raw_l, raw_r)
    cases['forward_left_right 960x540 D192'] = lambda: net.forward_left_right(left, right, max_difference=1.0)
    cases['reconstruct, check'] = lambda: rig.reconstruct(net, raw_l, raw_r, max_difference=1.0)
    cases['reconstruct, check + speckle'] = lambda: rig.reconstruct(net, raw_l, raw_r, max_difference=1.0,
                                                                    speckle_size=100)

    times = {k: [] for k in cases}
    with torch.no_grad():
        for fn in cases.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            for name, fn in cases.items():
                times[name].append(timed(fn))
    med = {}
    for name, ts in times.items():
        ts.sort()
        med[name] = ts[len(ts) // 2]
        print('%-40s min %9.1f us  median %9.1f us  max %9.1f us' % (name, ts[0], med[name], ts[-1]))
    base = med['forward_left_right 960x540 D192']
    print('reconstruct / forward_left_right (median): with the check %.4f, with the check and the speckle filter %.4f' %
          (med['reconstruct, check'] / base, med['reconstruct, check + speckle'] / base))
    plane = [v for k, v in med.items() if k.startswith('filter plane')]
    worst = max((v, k) for k, v in med.items() if k.startswith('filter'))
    print('filter: plane scenes %.1f - %.1f us, slowest case %.1f us (%s)' % (min(plane), max(plane), worst[0], worst[1]))

    from tests.test_speckle_host import oracle_sizes
    for key, (image, md) in host.items():
        t0 = time.perf_counter()
        oracle_sizes(image, None, md)
        print('host numpy union-find  %s  %9.1f ms' % (key, (time.perf_counter() - t0) * 1e3))


if __name__ == '__main__':
    main()
