"""Cost of the right view and the left-right consistency check, timed with CUDA events (interleaved, median of reps):
  * PdsNetwork.forward against forward_right at config 2 (960x540, D = 192);
  * forward_left_right against two forward calls one after the other (the right view runs on a second stream);
  * the check kernel alone (pds_left_right_check_fwd) at config 2 and config 4 (1242x375), with and without the fill.
Per-kernel times: run it under rocprofv3 --kernel-trace --stats.

    python tools/bench_left_right.py [reps]
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
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = pds.PdsNetwork.default(191).eval().to(dev).freeze_weights()
    g = torch.Generator().manual_seed(1)
    left = (torch.rand(1, 3, 540, 960, generator=g) * 255).to(dev)
    right = (torch.rand(1, 3, 540, 960, generator=g) * 255).to(dev)
    with torch.no_grad():
        dl2 = net(left, right)
        dr2 = net.forward_right(left, right)
    dl4 = torch.rand(1, 375, 1242, generator=g).to(dev) * 100
    dr4 = dl4 + torch.randn(1, 375, 1242, generator=g).to(dev)
    cases = {
        'forward': lambda: net(left, right),
        'forward_right': lambda: net.forward_right(left, right),
        '2 x forward': lambda: (net(left, right), net(right, left)),
        'forward_left_right': lambda: net.forward_left_right(left, right),
        'forward_left_right fill': lambda: net.forward_left_right(left, right, fill=True),
        'check config 2': lambda: pds.left_right_check(dl2, dr2),
        'check+fill config 2': lambda: pds.left_right_check(dl2, dr2, fill=True),
        'check config 4': lambda: pds.left_right_check(dl4, dr4),
        'check+fill config 4': lambda: pds.left_right_check(dl4, dr4, fill=True),
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
        print('%-24s min %9.1f us  median %9.1f us' % (name, ts[0], med[name]))
    print('forward_right / forward (median) %.4f; forward_left_right / (2 x forward) %.4f' %
          (med['forward_right'] / med['forward'], med['forward_left_right'] / med['2 x forward']))


if __name__ == '__main__':
    main()
