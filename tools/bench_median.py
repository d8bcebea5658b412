"""Cost of the median filter (pds_median_filter_fwd: one launch):
  * median_filter at 960x540 and 1242x375, batch 1 and 4, kernel_size 3 / 5 / 7, with and without a mask, on a plane
    scene with 2 % outliers and NaN holes (tools/bench_speckle.py), timed with device events (interleaved, median of
    reps); the event time of one short kernel is mostly launch overhead, the kernel times come from the trace;
  * StereoRig.reconstruct(..., speckle_size=100) with and without median_size=5 at 960x540, D = 192, as a ratio.
Inputs are seeded.

    python tools/bench_median.py [reps]
    python tools/bench_median.py launches      # every filter case ten times and nothing else: run this form under
                                                # rocprofv3 --kernel-trace --stats for the kernel times
    python tools/bench_median.py events [reps] # the filter cases alone, without the network
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import practicaldeepstereo_nips2018_amd as pds  # noqa: E402
from tools.bench_rectify import rig_for, timed  # noqa: E402
from tools.bench_speckle import plane_scene  # noqa: E402

HBM_BYTES_PER_SECOND = 6.3e12


def algorithmic_bytes(batch, height, width, masked):
    """Read 4 B (+ 1 B of mask), write 4 B + 1 B per pixel."""
    return batch * height * width * (4 + (1 if masked else 0) + 4 + 1)


def filter_cases(dev):
    cases = {}
    for width, height in ((960, 540), (1242, 375)):
        for batch in (1, 4):
            d = torch.from_numpy(np.stack([plane_scene(height, width, k) for k in range(batch)])).to(dev)
            mask = torch.from_numpy(np.random.RandomState(7).rand(batch, height, width) > 0.1).to(dev)
            for k in (3, 5, 7):
                for masked in (False, True):
                    name = 'median k%d %-7s %4dx%-3d b%d' % (k, 'mask' if masked else 'no mask', width, height, batch)
                    cases[name] = (lambda d=d, k=k, v=(mask if masked else None):
                                   pds.median_filter(d, k, valid=v, fill_holes=True),
                                   algorithmic_bytes(batch, height, width, masked))
    return cases


def report(times, extra=None):
    med = {}
    for name, ts in times.items():
        ts.sort()
        med[name] = ts[len(ts) // 2]
        print('%-40s min %9.1f us  median %9.1f us  max %9.1f us%s' %
              (name, ts[0], med[name], ts[-1], '' if not extra or name not in extra else extra[name]))
    return med


def main():
    dev = torch.device('cuda:0')
    cases = filter_cases(dev)
    mode = sys.argv[1] if len(sys.argv) > 1 else ''
    if mode == 'launches':
        for fn, _ in cases.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        return
    numbers = [a for a in sys.argv[1:] if a.isdigit()]
    reps = int(numbers[0]) if numbers else 30

    run = {name: fn for name, (fn, _) in cases.items()}
    floors = {name: '   (%.2f MB, HBM floor %.2f us)' % (nbytes / 1e6, nbytes / HBM_BYTES_PER_SECOND * 1e6)
              for name, (_, nbytes) in cases.items()}
    if mode != 'events':
        torch.manual_seed(0)
        net = pds.PdsNetwork.default(191).eval().to(dev).freeze_weights()
        rig = rig_for(960, 540)
        g = torch.Generator().manual_seed(1)
        raw_l = torch.randint(0, 256, (1, 540, 960, 3), generator=g, dtype=torch.uint8).to(dev)
        raw_r = torch.randint(0, 256, (1, 540, 960, 3), generator=g, dtype=torch.uint8).to(dev)
        run = {}   # (the network alone takes the window: the filter cases are the `events` form)
        run['reconstruct, check + speckle'] = lambda: rig.reconstruct(net, raw_l, raw_r, max_difference=1.0,
                                                                      speckle_size=100)
        run['reconstruct, check + speckle + median 5'] = lambda: rig.reconstruct(
            net, raw_l, raw_r, max_difference=1.0, speckle_size=100, median_size=5, median_fill_holes=True)

    times = {k: [] for k in run}
    with torch.no_grad():
        for fn in run.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            for name, fn in run.items():
                times[name].append(timed(fn))
    med = report(times, floors)
    if mode != 'events':
        print('reconstruct with median_size=5 / without (median of %d interleaved repeats): %.4f' %
              (reps, med['reconstruct, check + speckle + median 5'] / med['reconstruct, check + speckle']))


if __name__ == '__main__':
    main()
