"""The fp32 floors quoted in tests/test_gpu_conv3d_layers.py: for every case of its table, the max-abs distance of the
CPU's fp32 F.conv3d (+ LeakyReLU) from the fp64 reference of the same inputs (e32), and the wall time of the two CPU
convolutions.  Needs no GPU:  python tools/conv3d_e32_floors.py"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import test_gpu_conv3d_layers as layers   # noqa: E402


def main():
    by_cin, total = {}, 0.0
    for index, case in enumerate(layers.CASES):
        t0 = time.time()
        x, x_scale, x_shift, xhat, weight, bias, gamma, beta = layers.make_case(case, index)
        want_raw = layers.reference(xhat, weight, bias, gamma, beta, case[7])[0]
        e32 = layers.fp32_floor(xhat, weight, bias, case[7], want_raw)
        dt = time.time() - t0
        total += dt
        by_cin.setdefault(case[2], []).append(e32)
        print('%-44s K %4d  |raw| max %5.2f  e32 %.2e  3 x e32 %.2e  gate %.2e  %5.2f s'
              % (layers.case_id(case), 27 * case[2], float(want_raw.abs().max()), e32, 3 * e32,
                 max(layers.TOL, 3 * e32), dt))
    for cin in sorted(by_cin):
        print('Cin = %3d (K = %4d): e32 %.1e .. %.1e' % (cin, 27 * cin, min(by_cin[cin]), max(by_cin[cin])))
    print('CPU references of the whole table: %.1f s' % total)


if __name__ == '__main__':
    main()
