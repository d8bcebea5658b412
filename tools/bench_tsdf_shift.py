"""Cost of the rolling volume's shift (pds_tsdf_shift_fwd) beside the composition in torch a user would otherwise write,
``torch.full`` plus one sliced copy per tensor, and of the leaving extraction beside the full ``extract_points``; in the
manner of tools/bench_tsdf.py: 256^3 voxels, plain and coloured, deltas (8, 0, 0), (0, 0, 8) and (3, -2, 1).

After a warm-up, `calls` calls in one region between two device events, the two paths taking turns region by region in
one process; the median of the regions, per call.  Both paths allocate their outputs afresh, as ``shift`` does.  The
kernel alone comes from the library's launch probe.  Bytes: 4 B per float, written for every voxel and read for those
that stay.

    python tools/bench_tsdf_shift.py [regions] [calls]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import practicaldeepstereo_nips2018_amd as pds  # noqa: E402
from bench_tsdf import kernel_times, median, region  # noqa: E402

COPY_BYTES_PER_SECOND = 6.29e12   # the copy rate an MI355X reaches: a ceiling for context, not a target of this kernel


def staying(n, d):
    lo, hi = max(0, -d), min(n, n - d)
    return (lo, hi) if lo < hi else (0, 0)


def composed_shift(tensors, empties, delta):
    """out = full(empty); out[stays] = in[stays + delta], per tensor: two writes of the output in two launches each."""
    dx, dy, dz = delta
    out = []
    for t, empty in zip(tensors, empties):
        nz, ny, nx = t.shape[:3]
        (x0, x1), (y0, y1), (z0, z1) = staying(nx, dx), staying(ny, dy), staying(nz, dz)
        moved = torch.full_like(t, empty)
        moved[z0:z1, y0:y1, x0:x1] = t[z0 + dz:z1 + dz, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        out.append(moved)
    return out


def main():
    regions = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device('cuda:0')
    print('device: %s' % torch.cuda.get_device_name(dev))
    n = 256
    geometry = dict(origin=(-0.64, -0.64, 1.0), voxel_size=0.005, dims=(n, n, n), truncation=0.02)
    rng = np.random.RandomState(0)
    # a surface to extract: a slanted plane through the volume, observed everywhere
    kk, jj, ii = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing='ij')
    tsdf = np.clip((0.3 * ii + 0.2 * jj + kk - 0.75 * n) / 4.0, -1.0, 1.0).astype(np.float32)
    tsdf += (1e-3 * rng.standard_normal(tsdf.shape)).astype(np.float32)
    state = [torch.from_numpy(tsdf).to(dev), torch.ones((n, n, n), device=dev),
             torch.from_numpy(rng.uniform(0, 255, (n, n, n, 3)).astype(np.float32)).to(dev)]
    for color in (False, True):
        volume = (pds.ColorTsdfVolume if color else pds.TsdfVolume)(device=dev, **geometry)
        tensors = state if color else state[:2]
        floats = n ** 3 * (5 if color else 2)

        def restore():
            volume.tsdf, volume.weight = state[0], state[1]
            if color:
                volume.color = state[2]

        for delta in ((8, 0, 0), (0, 0, 8), (3, -2, 1)):
            def shift():
                restore()
                volume.shift(delta)

            paths = {'tsdf_shift': shift, 'torch': lambda: composed_shift(tensors, (1.0, 0.0, 0.0), delta)}
            for fn in paths.values():
                for _ in range(3):
                    fn()
            got = [volume.tsdf, volume.weight] + ([volume.color] if color else [])
            same = all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                       for a, b in zip(got, composed_shift(tensors, (1.0, 0.0, 0.0), delta)))
            torch.cuda.synchronize()
            times = {name: [] for name in paths}
            for _ in range(regions):
                for name, fn in paths.items():
                    times[name].append(region(fn, calls))
            kernels = [kernel_times(b'tsdf_shift', shift, 1)[0] for _ in range(regions)]
            share = np.prod([staying(n, d)[1] - staying(n, d)[0] for d in delta]) / n ** 3
            nbytes = 4.0 * floats * (1.0 + share)
            print('%s 256^3, delta %-11s equal bits: %s   shift %8.1f us per call (min %8.1f)   torch %8.1f us (min %8.1f)   '
                  'torch / shift %.2f x   kernel %8.1f us: %.2f TB/s of %.1f MB (%.0f %% of the copy rate)' %
                  ('coloured' if color else 'plain   ', delta, same, median(times['tsdf_shift']), min(times['tsdf_shift']),
                   median(times['torch']), min(times['torch']), median(times['torch']) / median(times['tsdf_shift']),
                   median(kernels), nbytes / median(kernels) / 1e6, nbytes / 1e6,
                   100.0 * nbytes / median(kernels) / 1e6 / (COPY_BYTES_PER_SECOND / 1e12)))

        # the leaving extraction beside the full one, on the same state
        restore()
        capacity = 1 << 21
        full = (lambda: volume.extract_points(capacity=capacity, trim=False))
        count = int(full().cloud.offsets[1])
        for delta in ((8, 0, 0), (0, 0, 8)):
            def leaving():
                restore()
                return volume.shift(delta, leaving=True, capacity=capacity, trim=False)

            def plain_shift():
                restore()
                volume.shift(delta)

            paths = {'extract_points': full, 'shift(leaving=True)': leaving, 'shift': plain_shift}
            for fn in paths.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name in paths}
            for _ in range(regions):
                for name, fn in paths.items():
                    times[name].append(region(fn, calls))
            kernels = [sum(kernel_times(b'tsdf_extract_leaving', leaving, 3)) for _ in range(regions)]
            whole = [sum(kernel_times(b'tsdf_extract', full, 3)) for _ in range(regions)]
            print('%s 256^3, delta %-11s %d of %d rows leave   extract_points %8.1f us (kernels %8.1f)   shift with leaving '
                  '%8.1f us (leaving kernels %8.1f)   shift alone %8.1f us' %
                  ('coloured' if color else 'plain   ', delta, int(leaving().cloud.offsets[1]), count,
                   median(times['extract_points']), median(whole), median(times['shift(leaving=True)']), median(kernels),
                   median(times['shift'])))


if __name__ == '__main__':
    main()
