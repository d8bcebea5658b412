"""Cost of the confidence map: four cases timed with CUDA events (interleaved, median of reps):
  * stand-alone SubpixelMap on a [1, 96, 576, 960] volume, plain and with_confidence;
  * the eval tail Regularization + SubpixelMap (fused) at config 2 (960x540, D = 192), plain and with_confidence.
The tail times include the hourglass trunk; the difference of the two is the fused kernel's.  Per-kernel times: run it
under rocprofv3 --kernel-trace --stats.

    python tools/bench_confidence.py [reps]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import practicaldeepstereo_nips2018_amd as pds  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    vol = torch.randn(1, 96, 576, 960, device=dev)
    est = pds.SubpixelMap()
    net = pds.PdsNetwork.default(191).eval().to(dev)
    g = torch.Generator().manual_seed(1)
    ms = torch.randn(1, 8, 48, 144, 240, generator=g).to(dev)
    sc = torch.randn(1, 8, 144, 240, generator=g).to(dev)
    reg = net._regularization
    cases = {
        'estimator': lambda: est(vol),
        'estimator+confidence': lambda: est.with_confidence(vol),
        'fused tail': lambda: reg.forward_with_estimator(ms, sc, est),
        'fused tail+confidence': lambda: reg.forward_with_estimator(ms, sc, est, with_confidence=True),
    }
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
        print('%-22s min %8.1f us  median %8.1f us' % (name, ts[0], med[name]))
    print('confidence / plain (median): estimator %.3fx, fused tail +%.1f us' %
          (med['estimator+confidence'] / med['estimator'], med['fused tail+confidence'] - med['fused tail']))


if __name__ == '__main__':
    main()
