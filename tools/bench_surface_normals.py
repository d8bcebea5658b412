"""Cost of the surface normals (pds_surface_normals_fwd: one launch) at 960x540, kernel_size 3 / 5 / 7, on a plane scene
with 2 % outliers and NaN holes (tools/bench_speckle.py), against the composition a user writes in torch today:
``reproject``, central differences of the dense points along x and y, ``cross``, normalise, turn towards the camera.
Both run in the same process, interleaved, timed with device events (median of reps).  The event time of one short kernel
is mostly launch overhead: the kernel times come from the trace.

    python tools/bench_surface_normals.py [reps]
    python tools/bench_surface_normals.py launches   # every case ten times and nothing else: run this form under
                                                     # rocprofv3 --kernel-trace --stats for the kernel times
Inputs are seeded.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import practicaldeepstereo_nips2018_amd as pds  # noqa: E402
from tools.bench_median import report  # noqa: E402
from tools.bench_rectify import rig_for, timed  # noqa: E402
from tools.bench_speckle import plane_scene  # noqa: E402

HBM_BYTES_PER_SECOND = 6.3e12
WIDTH, HEIGHT = 960, 540


def algorithmic_bytes(batch, height, width, masked):
    """Read 4 B (+ 1 B of mask), write 12 B + 1 B per pixel."""
    return batch * height * width * (4 + (1 if masked else 0) + 12 + 1)


def torch_composition(disparity, matrix, valid=None):
    """What a user writes without the entry point: five passes over the 6 MB of dense points and a dozen launches."""
    points = pds.reproject(disparity, matrix, valid=valid)
    tx = torch.full_like(points, float('nan'))
    ty = torch.full_like(points, float('nan'))
    tx[:, :, 1:-1] = points[:, :, 2:] - points[:, :, :-2]
    ty[:, 1:-1] = points[:, 2:] - points[:, :-2]
    normal = torch.cross(tx, ty, dim=-1)
    normal = normal / normal.norm(dim=-1, keepdim=True)
    return torch.where(((normal * points).sum(-1, keepdim=True) > 0), -normal, normal)


def cases(dev):
    rig = rig_for(WIDTH, HEIGHT)
    matrix = rig.reprojection_matrix('rectified')
    d = torch.from_numpy(plane_scene(HEIGHT, WIDTH, 0)[None]).to(dev)
    mask = torch.from_numpy(np.random.RandomState(7).rand(1, HEIGHT, WIDTH) > 0.1).to(dev)
    out = {}
    for k in (3, 5, 7):
        for masked in (False, True):
            name = 'surface_normals k%d %-7s %dx%d' % (k, 'mask' if masked else 'no mask', WIDTH, HEIGHT)
            out[name] = (lambda k=k, v=(mask if masked else None): pds.surface_normals(d, matrix, kernel_size=k, valid=v),
                         algorithmic_bytes(1, HEIGHT, WIDTH, masked))
    out['torch composition no mask %dx%d' % (WIDTH, HEIGHT)] = (lambda: torch_composition(d, matrix), None)
    out['torch composition mask    %dx%d' % (WIDTH, HEIGHT)] = (lambda: torch_composition(d, matrix, mask), None)
    return out


def main():
    dev = torch.device('cuda:0')
    run = cases(dev)
    if len(sys.argv) > 1 and sys.argv[1] == 'launches':
        for fn, _ in run.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        return
    numbers = [a for a in sys.argv[1:] if a.isdigit()]
    reps = int(numbers[0]) if numbers else 50
    floors = {name: '   (%.2f MB, HBM floor %.2f us)' % (nbytes / 1e6, nbytes / HBM_BYTES_PER_SECOND * 1e6)
              for name, (_, nbytes) in run.items() if nbytes}
    times = {name: [] for name in run}
    with torch.no_grad():
        for fn, _ in run.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            for name, (fn, _) in run.items():
                times[name].append(timed(fn))
    med = report(times, floors)
    for masked in ('no mask', 'mask   '):
        baseline = med['torch composition %s %dx%d' % (masked, WIDTH, HEIGHT)]
        for k in (3, 5, 7):
            call = med['surface_normals k%d %-7s %dx%d' % (k, masked.strip(), WIDTH, HEIGHT)]
            print('k = %d, %s: call %.1f us, torch composition %.1f us, ratio %.2f (median of %d interleaved repeats)' %
                  (k, masked.strip(), call, baseline, baseline / call, reps))


if __name__ == '__main__':
    main()
