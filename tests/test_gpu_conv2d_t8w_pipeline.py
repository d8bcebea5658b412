"""GPU (-m gpu): the balanced form of conv2d_t8w (csrc/conv2d_t8.hip, FORM 1 of the 6-row full-width kernel) alone.

The bare certified 64 -> 8 layer behind a deferred InstanceNorm through pds_conv_block_chained_fwd -- the entry point and
the helpers of tests/test_gpu_conv2d_layers.py -- against an fp64 convolution on the CPU, with that file's gate for the
layer (max-abs max(2e-5, 3 x e32), mean-abs max(6e-7, 3 x e32 mean); e32 = the CPU's own fp32 run, the floors written by
tools/conv2d_e32_floors.py).  The launch probe says that conv2d_t8w ran, once, and over how many tiles.

The form before it stays selectable (PDS_DEBUG_SWITCHES=1 PDS_CONV2D_T8W_BALANCED=0).  Both sum the same products in the
same order per output, so every case must be BIT-identical between the two.  Library switches are read once per process:
one child process (this file run as a script) computes every case under the switch and saves the outputs.

Shapes.  The form serves rows of 64 .. 256 columns (W % 4 == 0) and planes of at least 8 rows in tiles of 6 rows x the
whole row, so a plane of exactly one tile does not exist for it: the smallest plane (8 rows) is one whole tile + a
2-row partial one.  Blocks are 16 columns; the (row pair, block) jobs of a tile are dealt over eight waves, six each.
    8 x 64      the smallest: 12 jobs, six waves idle, second tile partial
    12 x 64     exactly two tiles
    13 x 68     one row and one 4-column quad over: a one-row third tile, a 4-column fifth block (right-edge mapping)
    13 x 100    a width that is no multiple of the block: 21 jobs, job lists of a wave straddle row pairs
    20 x 256    the widest row: 48 jobs = all eight waves full, no surplus staging thread
    36 x 64 x 48 planes   288 tiles on 256 workgroups: four workgroups per XCD take a second tile, six planes on (another
                plane's InstanceNorm coefficients mid-stream); the probe's tile count says 288
    batch 2
The two-source configuration (the residual sum formed while staging; the instance the hot path runs) cannot be built
through a single-layer entry point: both pass no second source.  It runs through the fused Matching operation
(pds.Matching(31, MatchingOperation) on descriptors of 54 x 68: 32 planes x 9 tiles = 288 tiles, more than a launch has
workgroups, rows of 68 columns = four blocks + a quad) and is compared with the SAME module evaluated in fp64 on the CPU
(oracle.matching_with_operation on fp64 parameters and inputs) at the project's gate for the signatures,
TOL_SIGNATURES = 2e-5 of tests/test_gpu_parity.py -- the whole chain, since the layer's inputs exist only inside it --
and bit for bit with the form before.

Which form ran: the launch probe counts FORM 1 under "conv2d_t8w<balanced>" and both forms under "conv2d_t8w"; the child
process must show one launch of the latter and none of the former.

Workgroups crossing planes: a launch has one workgroup per CU (rounded down to a multiple of 8), XCD x walks the x-th
eighth of the tile list with a stride of workgroups / 8; `workgroup_tiles` restates that (csrc/conv2d_t8.hip, "this
workgroup's tiles") from the device's CU count, and the 288-tile cases must give some workgroup tiles of two planes.

Determinism: the same inputs 20 times, alternately on one stream and dealt over three streams with a matrix product
running beside them on a fourth; all 20 outputs bit-equal -- for a one-source launch and for the two-source Matching run.
"""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from practicaldeepstereo_nips2018_amd import _lib
from oracle import pds_oracle as oracle
from tests import helpers
from tests.test_gpu_conv2d_layers import (BOUND, T8W, TOL, TOL_MEAN, fp32_floor, make_case, reference, run_layer)
from tests.test_gpu_parity import TOL_SIGNATURES

pytestmark = pytest.mark.gpu

# kernel, entry, n, cin, cout, d, h, w, x_per_plane, per_plane, affine, note  (the tuple of tests/test_gpu_conv2d_layers.py)
CASES = [
    (T8W, BOUND, 1, 64, 8, 1, 8, 64, 1, 1, False, 'the smallest plane: one tile + a 2-row partial one'),
    (T8W, BOUND, 1, 64, 8, 2, 12, 64, 1, 1, False, 'exactly two tiles'),
    (T8W, BOUND, 1, 64, 8, 2, 13, 68, 1, 1, False, 'one row and one quad of columns over'),
    (T8W, BOUND, 1, 64, 8, 3, 13, 100, 0, 1, False, 'width no multiple of the block, per-volume input'),
    (T8W, BOUND, 1, 64, 8, 1, 20, 256, 1, 1, False, 'the widest row'),
    (T8W, BOUND, 1, 64, 8, 48, 36, 64, 1, 1, False, '288 tiles: workgroups cross planes'),
    (T8W, BOUND, 2, 64, 8, 3, 14, 80, 1, 1, False, 'batch 2'),
]
SEED0 = 7000
MATCHING_SHAPE, MATCHING_MAXD = (1, 64, 54, 68), 31
MATCHING_TILES = (MATCHING_MAXD + 1) * ((MATCHING_SHAPE[2] + 5) // 6)
BALANCED = T8W + '<balanced>'


def case_id(c):
    return 'n%d_d%d_%dx%d_xpp%d' % (c[2], c[5], c[6], c[7], c[8])


def tiles_of(case):
    return case[2] * case[5] * ((case[6] + 5) // 6)


def probed(lib, run):
    """-> (result, [tiles of every conv2d_t8w launch in run], launches of the balanced form in a second run)."""
    import ctypes

    def once(name):
        _lib.check(lib.pds_probe_begin(name.encode(), 16), 'pds_probe_begin')
        try:
            result = run()
            torch.cuda.synchronize()
        finally:
            wgs = (ctypes.c_int * 16)()
            count = lib.pds_probe_end(None, wgs, 16)
        assert count >= 0, lib.pds_last_error()
        return result, [wgs[i] for i in range(count)]

    result, tiles = once(T8W)
    return result, tiles, len(once(BALANCED)[1])


def workgroup_tiles(tiles, cus):
    """Tile lists of the workgroups of a conv2d_t8w launch over `tiles` tiles on a device of `cus` CUs."""
    wgs = min(cus // 8 * 8, (tiles + 7) // 8 * 8)
    per_xcd = wgs // 8
    lists = []
    for block in range(wgs):
        xcd, slot = block & 7, block >> 3
        lists.append(list(range(xcd * tiles // 8 + slot, (xcd + 1) * tiles // 8, per_xcd)))
    return lists


def layer_runner(dev, index):
    case = CASES[index]
    x, x_scale, x_shift, xhat, weight, bias, gamma, beta = make_case(case, SEED0 + index)
    return run_layer(dev, case, x, x_scale, x_shift, xhat, xhat.abs().max(), weight, bias, gamma, beta), (xhat, weight, bias)


def matching_inputs():
    import practicaldeepstereo_nips2018_amd as pds
    op = helpers.seeded(pds.MatchingOperation, seed=7)
    g = torch.Generator().manual_seed(17)
    return op, torch.randn(*MATCHING_SHAPE, generator=g), torch.randn(*MATCHING_SHAPE, generator=g)


def matching_runner(dev):
    import practicaldeepstereo_nips2018_amd as pds
    op, left, right = matching_inputs()
    module = pds.Matching(MATCHING_MAXD, op).to(dev).eval()
    left, right = left.to(dev), right.to(dev)

    def run():
        with torch.no_grad():
            return module(left, right)

    return run


def all_outputs(dev):
    """Raw outputs of every case and the signatures of the two-source run, with the probe's tile counts."""
    lib = _lib.load()
    out = {}
    for index in range(len(CASES)):
        run, _ = layer_runner(dev, index)
        (raw, _, _, _), tiles, balanced = probed(lib, run)
        out[index] = (raw.cpu(), tiles, balanced)
    signatures, tiles, balanced = probed(lib, matching_runner(dev))
    out['matching'] = (signatures.cpu(), tiles, balanced)
    return out


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def new_form(dev):
    return all_outputs(dev)


@pytest.fixture(scope='module')
def old_form(hip_library):
    """The same cases in a child process under PDS_CONV2D_T8W_BALANCED=0."""
    env = dict(os.environ, PDS_DEBUG_SWITCHES='1', PDS_CONV2D_T8W_BALANCED='0')
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'old_form.pt')
        done = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True)
        assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
        return torch.load(path)


@pytest.mark.parametrize('index', range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_layer_against_fp64(new_form, index):
    case = CASES[index]
    _, _, _, xhat, weight, bias, gamma, beta = make_case(case, SEED0 + index)
    raw, tiles, _ = new_form[index]
    want, _, _, _ = reference(xhat, weight, bias, gamma, beta, 1, False)
    e32, e32_mean = fp32_floor(xhat, weight, bias, False, want)
    tol, tol_mean = max(TOL, 3.0 * e32), max(TOL_MEAN, 3.0 * e32_mean)
    assert not torch.isnan(raw).any(), 'output positions left unwritten'
    assert bool(torch.isfinite(raw).all())
    err = float((raw.double() - want).abs().max())
    err_mean = float((raw.double() - want).abs().mean())
    print('conv2d_t8w pipeline %s (%s): tiles %s  e32 %.2e (mean %.2e)  gate %.2e (mean %.2e)  err %.3g (mean %.3g)'
          % (case_id(case), case[-1], tiles, e32, e32_mean, tol, tol_mean, err, err_mean))
    assert tiles == [tiles_of(case)], (tiles, tiles_of(case))   # conv2d_t8w ran, once, over this many 6-row tiles
    assert err <= tol, (err, tol)
    assert err_mean <= tol_mean, (err_mean, tol_mean)


def test_two_sources_against_fp64(new_form):
    """The two-source launch inside Matching against the module in fp64 on the CPU."""
    op, left, right = matching_inputs()
    p = {k: v.double() for k, v in helpers.prefixed(op.state_dict(), '_m._operation').items()}
    want = oracle.matching_with_operation(p, '_m', left.double(), right.double(), MATCHING_MAXD)
    got, tiles, balanced = new_form['matching']
    assert got.shape == want.shape and want.dtype == torch.float64
    assert bool(torch.isfinite(got).all())
    err = float((got.double() - want).abs().max())
    print('conv2d_t8w pipeline, two sources through Matching %s, %d planes: tiles %s  err %.3g (mean %.3g)  gate %.1e'
          % (MATCHING_SHAPE, MATCHING_MAXD + 1, tiles, err, float((got.double() - want).abs().mean()), TOL_SIGNATURES))
    assert tiles == [MATCHING_TILES] and balanced == 1, (tiles, balanced)
    assert err <= TOL_SIGNATURES, (err, TOL_SIGNATURES)


@pytest.mark.parametrize('which', ['one_source_48_planes', 'two_sources_matching'])
def test_workgroups_cross_planes(dev, new_form, which):
    """More tiles than the launch has workgroups: some workgroup's tile list spans two planes (another plane's
    InstanceNorm coefficients mid-stream).  The grid follows from the CU count of the device."""
    tiles, tiles_y = (tiles_of(CASES[5]), 6) if which.startswith('one') else (MATCHING_TILES, 9)
    assert new_form[5 if which.startswith('one') else 'matching'][1] == [tiles]
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    lists = workgroup_tiles(tiles, cus)
    assert sorted(t for l in lists for t in l) == list(range(tiles))
    crossing = [l for l in lists if len(set(t // tiles_y for t in l)) > 1]
    print('conv2d_t8w pipeline %s: %d tiles on %d workgroups (%d CUs), %d workgroups cross planes'
          % (which, tiles, len(lists), cus, len(crossing)))
    assert len(lists) < tiles and crossing


@pytest.mark.parametrize('key', list(range(len(CASES))) + ['matching'],
                         ids=[case_id(c) for c in CASES] + ['two_sources_matching'])
def test_bit_identical_to_the_form_before(new_form, old_form, key):
    new, new_tiles, new_balanced = new_form[key]
    old, old_tiles, old_balanced = old_form[key]
    # the switch was honoured: one conv2d_t8w launch on each side, the balanced form here and not in the child
    assert (new_balanced, old_balanced) == (1, 0), (new_balanced, old_balanced)
    assert len(new_tiles) == 1 and new_tiles == old_tiles, (new_tiles, old_tiles)
    assert bool(torch.isfinite(new).all())
    assert torch.equal(new, old), 'max difference %.3g' % float((new - old).abs().max())


@pytest.mark.parametrize('which', ['one_source', 'two_sources_matching'])
def test_deterministic_across_schedules(dev, which):
    """20 runs of one launch (3 planes of 13 x 100) or of the two-source Matching run (288 tiles), alternately on the
    current stream and dealt over three streams while a matrix product runs on a fourth: bit-equal."""
    if which == 'one_source':
        run = layer_runner(dev, 3)[0]
    else:
        matching = matching_runner(dev)
        run = lambda: (matching(),)
    streams = [torch.cuda.Stream(dev) for _ in range(3)]
    side = torch.cuda.Stream(dev)
    a = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize()
    results = []
    keep = []
    for i in range(20):
        if i % 2 == 0:
            out = run()
        else:
            with torch.cuda.stream(side):
                keep.append(a @ a)
            with torch.cuda.stream(streams[(i // 2) % 3]):
                out = run()
        results.append(out[0])
        keep.append(out)
    torch.cuda.synchronize()
    first = results[0].cpu()
    assert bool(torch.isfinite(first).all())
    for i, r in enumerate(results[1:], 1):
        assert torch.equal(first, r.cpu()), 'run %d differs' % i


if __name__ == '__main__':
    _lib.build_library()
    torch.save(all_outputs(torch.device('cuda:0')), sys.argv[1])
