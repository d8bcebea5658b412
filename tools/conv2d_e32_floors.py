"""The fp32 floors quoted in tests/test_gpu_conv2d_layers.py: for every case of its table, the max-abs and mean-abs
distance of the CPU's fp32 F.conv2d (+ LeakyReLU) from the fp64 reference of the same inputs (e32), the gates that
follow from them, and the wall time of the two CPU convolutions.  Needs no GPU:  python tools/conv2d_e32_floors.py"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import test_gpu_conv2d_layers as layers   # noqa: E402


def main():
    by_cin, total = {}, 0.0
    for index, case in enumerate(layers.CASES):
        t0 = time.time()
        x, x_scale, x_shift, xhat, weight, bias, gamma, beta = layers.make_case(case, index)
        want_raw = layers.reference(xhat, weight, bias, gamma, beta, case[9], case[10])[0]
        e32, e32_mean = layers.fp32_floor(xhat, weight, bias, case[10], want_raw)
        dt = time.time() - t0
        total += dt
        by_cin.setdefault(case[3], []).append((e32, e32_mean))
        print('%-64s K %4d  |raw| max %5.2f  e32 %.2e  mean %.2e  gate %.2e  mean gate %.2e  %5.2f s'
              % (layers.case_id(case), 9 * case[3], float(want_raw.abs().max()), e32, e32_mean,
                 max(layers.TOL, 3 * e32), max(layers.TOL_MEAN, 3 * e32_mean), dt))
    for cin in sorted(by_cin):
        maxima, means = [v[0] for v in by_cin[cin]], [v[1] for v in by_cin[cin]]
        print('    Cin = %3d (K = %4d): %.1e .. %.1e | %.1e .. %.1e      3 * e32 <= %.1e | %.1e'
              % (cin, 9 * cin, min(maxima), max(maxima), min(means), max(means), 3 * max(maxima), 3 * max(means)))
    print('CPU references of the whole table: %.1f s' % total)


if __name__ == '__main__':
    main()
