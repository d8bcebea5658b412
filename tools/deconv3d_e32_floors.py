"""The fp32 floors quoted in tests/test_gpu_deconv3d_layers.py: for every case of its table, the max-abs distance of the
CPU's fp32 F.conv_transpose3d (+ LeakyReLU when normed) from the fp64 reference of the same inputs (e32), and the wall
time of the two CPU transposed convolutions.  Needs no GPU:  python tools/deconv3d_e32_floors.py"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import test_gpu_deconv3d_layers as layers   # noqa: E402


def main():
    by_cin, total = {}, 0.0
    for index, case in enumerate(layers.CASES):
        t0 = time.time()
        x, x_scale, x_shift, xhat, weight, bias, gamma, beta = layers.make_case(case, index)
        kd, normed = case[4], case[9]
        want_raw = layers.reference(xhat, weight, bias, gamma, beta, kd, normed)[0]
        e32 = layers.fp32_floor(xhat, weight, bias, kd, normed, want_raw)
        dt = time.time() - t0
        total += dt
        by_cin.setdefault(case[2], []).append(e32)
        print('%-56s |raw| max %5.2f  e32 %.2e  3 x e32 %.2e  gate %.2e  %5.2f s'
              % (layers.case_id(case), float(want_raw.abs().max()), e32, 3 * e32, max(layers.TOL, 3 * e32), dt))
    for cin in sorted(by_cin):
        print('Cin = %3d: e32 %.1e .. %.1e' % (cin, min(by_cin[cin]), max(by_cin[cin])))
    print('CPU references of the whole table: %.1f s' % total)


if __name__ == '__main__':
    main()
