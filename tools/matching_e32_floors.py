"""The fp32 floors quoted in tests/test_gpu_matching_routes.py: for every case of its table, the max-relative and
mean-relative distance (to max(1, max|ref|)) of the CPU fp32 oracle of Matching from the fp64 oracle of the same inputs
(e32), the gates that follow, and the wall time of the two oracles.  Needs no GPU:  python tools/matching_e32_floors.py"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import test_gpu_matching_routes as routes   # noqa: E402


def main():
    total, largest, largest_mean = 0.0, 0.0, 0.0
    for case in routes.CASES:
        t0 = time.time()
        _, _, _, want, (e32, e32_mean) = routes.reference(case)
        dt = time.time() - t0
        total += dt
        largest, largest_mean = max(largest, e32), max(largest_mean, e32_mean)
        print('  %-36s e32 %.1e | %.1e   |ref| max %5.2f   gates %.1e | %.1e   %4.1f s'
              % (routes.case_id(case), e32, e32_mean, float(want.abs().max()), max(routes.REL_TOL, 3 * e32),
                 max(routes.REL_TOL_MEAN, 3 * e32_mean), dt))
    print('    largest e32 %.2e | %.2e: 3 * e32 %s the flat %.0e | %.0e of the Matching chain; both oracles of the whole '
          'table: %.1f s' % (largest, largest_mean,
                             'stays below' if 3 * largest <= routes.REL_TOL and 3 * largest_mean <= routes.REL_TOL_MEAN
                             else 'exceeds', routes.REL_TOL, routes.REL_TOL_MEAN, total))


if __name__ == '__main__':
    main()
