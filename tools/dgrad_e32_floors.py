"""The fp32 floors quoted in tests/test_gpu_dgrad_layers.py: for every case of its table, the distance of the CPU's fp32
autograd from the fp64 autograd of the same block, inputs and upstream gradient (e32), per gradient tensor (dx, dx2, dbias,
dgamma, dbeta) -- relative to the tensor's largest entry, and for dx the mean error relative to the mean magnitude -- and
the floors F / F_MEAN that follow per group of cases (2-D layers, 3-D layers): the largest value of the column over the
group, rounded up to one significant digit.
Needs no GPU:  python tools/dgrad_e32_floors.py [-v]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import test_gpu_dgrad_layers as layers   # noqa: E402
from tools.wgrad_e32_floors import round_up         # noqa: E402


def main(verbose):
    worst, worst_mean, total = {}, {}, 0.0
    for c in layers.CASES:
        t0 = time.time()
        _, want, theirs = layers.reference(c)
        rows = {name: layers.distance(theirs[name], want[name]) for name in want}
        e32 = [v[0] for v in rows.values()]
        e32_mean = [v[1] for name, v in rows.items() if name.startswith('dx')]
        dt = time.time() - t0
        total += dt
        worst[c['group']] = max(worst.get(c['group'], 0.0), max(e32))
        worst_mean[c['group']] = max(worst_mean.get(c['group'], 0.0), max(e32_mean))
        print('  %-32s %d tensors  e32 %.1e .. %.1e | dx mean %.1e   %5.1f s'
              % (c['id'], len(rows), min(e32), max(e32), max(e32_mean), dt))
        if verbose:
            for name, (a, b, _) in rows.items():
                print('        %-8s %.2e  %.2e' % (name, a, b))
    for group in worst:
        print('    %-11s largest e32 %.2e -> F = %.0e;  largest dx mean %.2e -> F_MEAN = %.0e'
              % (group + ':', worst[group], round_up(worst[group]), worst_mean[group], round_up(worst_mean[group])))
    print('CPU references of the whole table: %.1f s' % total)
    for group in worst:
        assert layers.F_FLOOR[group] == round_up(worst[group]) and layers.F_MEAN[group] == round_up(worst_mean[group]), group


if __name__ == '__main__':
    main('-v' in sys.argv[1:])
