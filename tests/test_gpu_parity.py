"""GPU (-m gpu): the HIP path, called through the C ABI, against the oracle and the golden vectors.

Stated fp32 tolerances: Matching out max-abs <= 2e-5; cost volume max-abs <= 1e-4 and
mean-abs <= 1e-5; estimator on identical cost max-abs <= 1e-3 px / MAE <= 1e-4; end-to-end disparity
MAE <= 1e-3 with the flip fraction (|delta| > 0.5 px) reported.
"""
import numpy as np
import pytest
import torch

from oracle import pds_oracle as oracle
from tests import helpers
import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib

pytestmark = pytest.mark.gpu

TOL_SIGNATURES = 2e-5
TOL_COST_MAX = 1e-4
TOL_COST_MEAN = 1e-5
TOL_EST_MAX = 1e-3
TOL_EST_MAE = 1e-4
TOL_DISPARITY_MAE = 1e-3


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def mock_operation(x):
    return torch.max(x, dim=1, keepdim=True)[0]


# ------------------------------------------------------------------------------- estimator (a8)
def test_subpixel_map_reference_known_answers(dev):
    sim = torch.tensor([0.1, 0.4, 0.3, 0.2, 0.3], device=dev).view(1, 5, 1, 1)
    assert abs(pds.SubpixelMap(2, 1)(sim).item() - 1.52) < 1e-4      # test_estimator.py:14-21
    assert abs(pds.SubpixelMap(2, 2)(sim).item() - 2.124) < 1e-4     # test_estimator.py:23-27


def test_subpixel_map_golden_cases(dev):
    g = helpers.golden('g5_subpixel_map')
    for name in sorted(k[:-3] for k in g if k.endswith('_in')):
        hw, step = [int(v) for v in g[name + '_cfg']]
        out = pds.SubpixelMap(hw, step)(g[name + '_in'].to(dev))
        assert out.shape == g[name + '_out'].shape, name
        assert helpers.maxdiff(out, g[name + "_out"]) <= 1e-4, name   # 1e-4 px: a few ulp at ~60 px


@pytest.mark.parametrize('shape,hw,step', [((2, 32, 17, 23), 4, 2), ((1, 96, 64, 128), 4, 2),
                                           ((3, 7, 5, 4), 2, 1), ((1, 64, 33, 31), 8, 2),
                                           ((1, 48, 16, 20), 12, 2)])
def test_subpixel_map_random_vs_oracle(dev, shape, hw, step):
    sim = torch.randn(*shape, generator=torch.Generator().manual_seed(3))
    out = pds.SubpixelMap(hw, step)(sim.to(dev))
    ref = oracle.subpixel_map(sim, hw, step)
    assert helpers.maxdiff(out, ref) <= TOL_EST_MAX
    assert helpers.meandiff(out, ref) <= TOL_EST_MAE


def test_subpixel_map_ties_take_first_plane(dev):
    sim = torch.zeros(1, 12, 4, 8)
    sim[:, 3] = 1.0
    sim[:, 9] = 1.0
    out = pds.SubpixelMap()(sim.to(dev))
    assert helpers.maxdiff(out, oracle.subpixel_map(sim)) <= 1e-5


def test_subpixel_map_full_size_properties(dev):
    """Config 2 size [1, 96, 576, 960]: range, one-hot recovery, agreement with the oracle."""
    g = torch.Generator().manual_seed(4)
    sim = torch.randn(1, 96, 576, 960, generator=g) * 0.58
    out = pds.SubpixelMap()(sim.to(dev))
    assert out.shape == (1, 576, 960)
    assert float(out.min()) >= 0.0 and float(out.max()) <= 2 * 95 + 1e-4
    ref = oracle.subpixel_map(sim)
    assert helpers.maxdiff(out, ref) <= TOL_EST_MAX
    assert helpers.meandiff(out, ref) <= TOL_EST_MAE
    hot = torch.full((1, 96, 64, 64), -50.0)
    idx = torch.randint(0, 96, (1, 1, 64, 64), generator=g)
    hot.scatter_(1, idx, 50.0)
    got = pds.SubpixelMap()(hot.to(dev)).cpu()
    assert torch.allclose(got, 2.0 * idx[:, 0].float(), atol=1e-4)


# ------------------------------------------------------------------------------- matching (a1-a3)
def test_matching_generic_operation_known_answer(dev):
    # reference test/test_matching.py:17-32
    net = pds.Matching(maximum_disparity=2, operation=mock_operation)
    left = torch.tensor([0., 2., 1., 2.], device=dev).view(1, 1, 1, 4)
    right = torch.tensor([3., 4., 2., 4.], device=dev).view(1, 1, 1, 4)
    out = net(left, right)
    assert np.array_equal(out.cpu().numpy().reshape(3, 4), [[3, 4, 2, 4], [0, 3, 4, 2], [0, 2, 3, 4]])
    net.set_maximum_disparity(maximum_disparity=1)
    out = net(left, right)
    assert np.array_equal(out.cpu().numpy().reshape(2, 4), [[3, 4, 2, 4], [0, 3, 4, 2]])
    g = helpers.golden('g1_matching_mock')
    out = pds.Matching(5, mock_operation)(g['left2'].to(dev), g['right2'].to(dev))
    assert torch.equal(out.cpu(), g['out2_max5'])


def test_matching_operation_output_size_and_values(dev):
    # reference test/test_matching.py:35-40 (shape) + golden values
    g = helpers.golden('g2_matching')
    op = helpers.seeded(pds.MatchingOperation).to(dev)
    with torch.no_grad():
        out = op(g['concatenated'].to(dev))
    assert out.size() == (2, 8, 25, 25)
    assert helpers.maxdiff(out, g['operation_out']) <= TOL_SIGNATURES


def test_fused_matching_golden(dev):
    g = helpers.golden('g2_matching')
    op = helpers.seeded(pds.MatchingOperation)
    net = pds.Matching(15, op).to(dev)
    with torch.no_grad():
        out = net(g['left'].to(dev), g['right'].to(dev))
    assert out.shape == (1, 8, 16, 16, 32)
    assert helpers.maxdiff(out, g['signatures']) <= TOL_SIGNATURES
    # the fused path and the generic per-plane path (same HIP MatchingOperation) agree
    generic = pds.Matching(15, lambda x: op(x))
    with torch.no_grad():
        out2 = generic(g['left'].to(dev), g['right'].to(dev))
    assert helpers.maxdiff(out, out2) <= TOL_SIGNATURES


@pytest.mark.parametrize('batch,h,w,maxd', [(2, 9, 21, 6), (1, 32, 64, 15), (1, 8, 16, 20), (1, 5, 7, 0),
                                            (2, 6, 4, 5), (1, 4, 2, 3), (2, 20, 36, 11)])
def test_fused_matching_shapes_vs_oracle(dev, batch, h, w, maxd):
    """Ragged sizes, batch > 1, disparity range wider than the image, single plane."""
    op = helpers.seeded(pds.MatchingOperation, seed=7)
    p = helpers.prefixed(op.state_dict(), '_m._operation')
    g = torch.Generator().manual_seed(8)
    left = torch.randn(batch, 64, h, w, generator=g)
    right = torch.randn(batch, 64, h, w, generator=g)
    ref = oracle.matching_with_operation(p, '_m', left, right, maxd)
    net = pds.Matching(maxd, op).to(dev)
    with torch.no_grad():
        out = net(left.to(dev), right.to(dev))
    assert out.shape == ref.shape
    assert helpers.maxdiff(out, ref) <= TOL_SIGNATURES


def test_disparity_sharding_is_bit_identical(dev):
    """planes are independent, so N sequential shards concatenated == unsharded."""
    op = helpers.seeded(pds.MatchingOperation)
    g = torch.Generator().manual_seed(9)
    left = torch.randn(1, 64, 16, 32, generator=g).to(dev)
    right = torch.randn(1, 64, 16, 32, generator=g).to(dev)
    net = pds.Matching(15, op).to(dev)
    with torch.no_grad():
        whole = net(left, right)
        for shards in (2, 4, 8):
            per = 16 // shards
            parts = []
            for r in range(shards):
                net.set_disparity_shard((r * per, per))
                parts.append(net(left, right))
            net.set_disparity_shard(None)
            assert torch.equal(torch.cat(parts, dim=2), whole), shards


# ------------------------------------------------------------------------------- regularization (a4-a7)
def test_contraction_and_expansion_blocks_golden(dev):
    # shapes of reference test/test_regularization.py:11-26, values from the golden vectors
    g = helpers.golden('g4_blocks')
    con = helpers.seeded(lambda: (torch.rand(2, 6, 10, 14, 16), pds.ContractionBlock3d(6))[1]).to(dev)
    with torch.no_grad():
        down, smooth = con(g['contraction_in'].to(dev))
    assert down.size() == (2, 12, 5, 7, 8) and smooth.size() == (2, 12, 5, 7, 8)
    assert helpers.maxdiff(down, g['contraction_down']) <= TOL_COST_MAX
    assert helpers.maxdiff(smooth, g['contraction_smooth']) <= TOL_COST_MAX

    def make_expansion():
        torch.rand(2, 6, 10, 14, 16)
        torch.rand(2, 3, 20, 28, 32)
        return pds.ExpansionBlock3d(6)
    exp = helpers.seeded(make_expansion).to(dev)
    with torch.no_grad():
        out = exp(g['expansion_in'].to(dev), g['expansion_shortcut'].to(dev))
    assert out.size() == (2, 3, 20, 28, 32)
    assert helpers.maxdiff(out, g['expansion_out']) <= TOL_COST_MAX


def test_regularization_output_size(dev):
    # reference test/test_regularization.py:29-36
    reg = helpers.seeded(pds.Regularization).to(dev)
    with torch.no_grad():
        cost = reg(torch.rand(2, 8, 32, 32, 32, device=dev), torch.rand(2, 8, 32, 32, device=dev))
    assert cost.size() == (2, 64, 128, 128)


def test_regularization_golden(dev):
    g = helpers.golden('g3_regularization')
    reg = helpers.seeded(pds.Regularization).to(dev)
    with torch.no_grad():
        cost = reg(g['signatures'].to(dev), g['shortcut'].to(dev))
    assert cost.shape == (1, 32, 64, 128)
    assert helpers.maxdiff(cost, g['cost']) <= TOL_COST_MAX
    assert helpers.meandiff(cost, g['cost']) <= TOL_COST_MEAN


def test_regularization_batch2_vs_oracle(dev):
    reg = helpers.seeded(pds.Regularization, seed=5)
    p = helpers.prefixed(reg.state_dict(), '_r')
    g = torch.Generator().manual_seed(6)
    ms = torch.randn(2, 8, 16, 32, 48, generator=g)
    shortcut = torch.randn(2, 8, 32, 48, generator=g)
    ref = oracle.regularization(p, '_r', ms, shortcut)
    reg = reg.to(dev)
    with torch.no_grad():
        cost = reg(ms.to(dev), shortcut.to(dev))
    assert helpers.maxdiff(cost, ref) <= TOL_COST_MAX
    assert helpers.meandiff(cost, ref) <= TOL_COST_MEAN


THRESHOLD_SHAPES = [
    # signature shape, conv3d_nx launches, conv3d_mfma launches (the 8 -> 16 stride-2 layer always runs there), note
    ((1, 8, 16, 48, 80), 0, 1, 'w = 80: the guarded (non-EXACT) form of conv3d_t8 / conv3d_t8x inside the hourglass'),
    ((1, 8, 32, 64, 128), 0, 3, '262 144 voxels: both 16 -> 16 layers between the conv3d_ks and conv3d_nx volumes'),
    ((2, 8, 32, 160, 160), 2, 1, '819 200 voxels: both 16 -> 16 layers on conv3d_nx, with a batch axis'),
    ((1, 8, 16, 16, 32), 0, 1, 'the smallest legal size: 1 x 1 x 2 voxels at the deepest level'),
]


@pytest.mark.parametrize('shape,nx_launches,mfma_launches,note', THRESHOLD_SHAPES,
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else None)
def test_regularization_threshold_shapes(dev, shape, nx_launches, mfma_launches, note):
    """Signature shapes that walk the volume thresholds of the 3-D dispatch (csrc/api.hip conv_block): seed-0 default
    parameters against the oracle, the kernel that took the 16-channel level named by the launch probe, and the fused
    estimator against the stand-alone one on the unfused cost (the gate of test_fused_estimator_support_windows).

    Measured on an MI355X (max / mean distance of the cost volume from the fp64 oracle; the fp32 CPU oracle's own distance):
        (1, 8, 16, 48, 80)     8.1e-6 / 7.6e-7     CPU fp32 1.0e-5 / 7.9e-7
        (1, 8, 32, 64, 128)    1.0e-5 / 8.2e-7     CPU fp32 8.8e-6 / 7.0e-7
        (2, 8, 32, 160, 160)   8.7e-6 / 7.5e-7     CPU fp32 1.4e-5 / 1.0e-6
        (1, 8, 16, 16, 32)     5.7e-5 / 5.3e-6     CPU fp32 5.4e-5 / 4.8e-6
    The smallest shape found a defect: with the statistics of conv3d_ks kept in fp32 before the fp64 fold it was
    1.55e-4 / 1.57e-5 from fp64 and missed the gate -- two voxels per channel, close to each other and far from zero,
    cancel a one-pass variance built from fp32 squares (docs/LAB_NOTES.md).  That kernel now sums in fp64 from the first
    square on.  The shape stays the least well-conditioned of the suite: the fp32 CPU oracle itself moves between 2e-5
    and 1.5e-4 when only the order of its input channels is changed."""
    lib = _lib.load()
    reg = helpers.seeded(pds.Regularization)
    p = helpers.prefixed(reg.state_dict(), '_r')
    g = torch.Generator().manual_seed(60 + shape[4])
    ms = torch.randn(*shape, generator=g)
    shortcut = torch.randn(shape[0], shape[1], shape[3], shape[4], generator=g)
    with torch.no_grad():
        # the oracle in fp64 on the same fp32 parameters and inputs (its fp32 run is printed beside it)
        ref = oracle.regularization(oracle.cast_params(p, torch.float64), '_r', ms.double(), shortcut.double())
        ref32 = oracle.regularization(p, '_r', ms, shortcut)
    reg = reg.to(dev)
    msg, sg = ms.to(dev), shortcut.to(dev)
    launches = {}
    for name in ('conv3d_nx', 'conv3d_mfma', 'conv3d_ks', 'conv3d_t8<guarded>', 'conv3d_t8x<guarded>'):
        _lib.check(lib.pds_probe_begin(name.encode(), 64), 'pds_probe_begin')
        with torch.no_grad():
            cost = reg(msg, sg)
        torch.cuda.synchronize()
        launches[name] = lib.pds_probe_end(None, None, 64)
    err_max, err_mean = helpers.maxdiff(cost, ref), helpers.meandiff(cost, ref)
    print('regularization %s (%s): launches %s  cost vs fp64 max %.3g mean %.3g  (fp32 CPU oracle vs fp64 %.3g / %.3g; HIP vs '
          'fp32 CPU oracle %.3g / %.3g)' % (shape, note, launches, err_max, err_mean, helpers.maxdiff(ref32, ref),
                                             helpers.meandiff(ref32, ref), helpers.maxdiff(cost, ref32),
                                             helpers.meandiff(cost, ref32)))
    assert launches['conv3d_nx'] == nx_launches and launches['conv3d_mfma'] == mfma_launches, launches
    assert launches['conv3d_ks'] > 0, launches
    if shape[4] % 32 != 0 and shape[4] % 48 != 0:
        # the un-certified first layer on the exact-fp32 kernel, the certified last one on the split kernel
        assert launches['conv3d_t8<guarded>'] == 1 and launches['conv3d_t8x<guarded>'] == 1, launches
    assert err_max <= TOL_COST_MAX, err_max
    assert err_mean <= TOL_COST_MEAN, err_mean
    est = pds.SubpixelMap()
    with torch.no_grad():
        unfused = est(cost)
        fused = reg.forward_with_estimator(msg, sg, est)
    rep = helpers.disparity_report(fused, unfused)
    print('regularization %s: fused vs unfused estimator %s' % (shape, rep))
    assert rep['mae_noflip'] <= 1e-4 and round(rep['flips'] * fused.numel()) <= 2, rep


def test_regularization_rejects_illegal_sizes(dev):
    reg = pds.Regularization().to(dev)
    with pytest.raises(ValueError):
        reg(torch.rand(1, 8, 12, 16, 32, device=dev), torch.rand(1, 8, 16, 32, device=dev))
    with pytest.raises(ValueError):  # a single voxel at 1/16 scale (torch >= 2 InstanceNorm guard)
        reg(torch.rand(1, 8, 16, 16, 16, device=dev), torch.rand(1, 8, 16, 16, device=dev))


def test_fused_regularization_estimator_matches_unfused(dev):
    g = helpers.golden('g3_regularization')
    reg = helpers.seeded(pds.Regularization).to(dev)
    est = pds.SubpixelMap()
    with torch.no_grad():
        unfused = est(reg(g['signatures'].to(dev), g['shortcut'].to(dev)))
        fused = reg.forward_with_estimator(g['signatures'].to(dev), g['shortcut'].to(dev), est)
    ref = oracle.subpixel_map(g['cost'])
    assert helpers.disparity_report(fused, ref)['mae'] <= TOL_DISPARITY_MAE
    assert helpers.disparity_report(fused, unfused)['mae'] <= TOL_DISPARITY_MAE


@pytest.mark.parametrize('half_support_window,step', [(2, 2), (4, 2), (6, 2), (8, 2)])
def test_fused_estimator_support_windows(dev, half_support_window, step):
    """The fused upsample + sub-pixel MAP kernel has one instantiation per window half-width T = window // step in
    {1, 2, 4} (different register rings and unroll factors; T = 3 runs on the T = 4 build): every one against the
    stand-alone estimator on the cost volume of the same sweep, and against the oracle (estimator.py:45-91)."""
    g = helpers.golden('g3_regularization')
    reg = helpers.seeded(pds.Regularization).to(dev)
    est = pds.SubpixelMap(half_support_window, step)
    gen = torch.Generator().manual_seed(77)
    signatures = torch.randn(2, 8, 16, 32, 48, generator=gen).to(dev)
    shortcut = torch.randn(2, 8, 32, 48, generator=gen).to(dev)
    with torch.no_grad():
        cost = reg(signatures, shortcut)
        unfused = est(cost)
        fused = reg.forward_with_estimator(signatures, shortcut, est)
    assert fused.shape == unfused.shape == (2, 128, 192)
    rep = helpers.disparity_report(fused, unfused)
    assert rep['mae_noflip'] <= 1e-4 and round(rep['flips'] * fused.numel()) <= 2, rep
    ref = oracle.subpixel_map(cost.cpu(), half_support_window, step)
    rep = helpers.disparity_report(fused, ref)
    assert rep['mae_noflip'] <= 1e-4 and round(rep['flips'] * fused.numel()) <= 2, rep


# ------------------------------------------------------------------------------- whole hot path
def hot_path_inputs(maximum_disparity, batch, height, width):
    """SURVEY.md 8c recipe: seed-0 default network, seed-1 images, descriptors computed once on CPU."""
    net = helpers.seeded(lambda: pds.PdsNetwork.default(maximum_disparity)).eval()
    left, right = helpers.images(batch, height, width)
    net._size_adapter.measure(left)   # records the padding for a later unpad, as SizeAdapter.pad would
    ld, shortcut = helpers.host_descriptors(net, left)
    rd = helpers.host_descriptors(net, right)[0]
    return net, ld, rd, shortcut


def run_hot_path(net, dev, ld, rd, shortcut, fuse):
    net = net.to(dev)
    with torch.no_grad():
        ms = net._matching(ld.to(dev), rd.to(dev))
        if fuse:
            return ms, None, net._regularization.forward_with_estimator(ms, shortcut.to(dev), net._estimator)
        cost = net._regularization(ms, shortcut.to(dev))
        return ms, cost, net._estimator(cost)


def test_config1_hot_path_vs_golden(dev):
    """BASELINE configs[0] shape (128x256, D=64) through the HIP hot path."""
    g = helpers.golden('g6_config1')
    net, ld, rd, shortcut = hot_path_inputs(63, 1, 128, 256)
    assert abs(helpers.checksum(net.state_dict()) - g['weight_checksum'].item()) < 1e-9
    ms, cost, disparity = run_hot_path(net, dev, ld, rd, shortcut, fuse=False)
    assert ms.shape == (1, 8, 16, 32, 64) and cost.shape == (1, 32, 128, 256)
    assert helpers.maxdiff(ms[:, :, ::2, ::4, ::4], g['signatures_sub']) <= TOL_SIGNATURES
    assert helpers.maxdiff(cost[:, ::4, ::8, ::8], g['cost_sub']) <= TOL_COST_MAX
    # End-to-end disparity: on 32 768 pixels ONE flipped arg-max (a near-tie of the random-weight cost volume
    # resolved the other way, ~30 px) is already 9e-4 of MAE, so the raw MAE is printed and loosely bounded while
    # the gates are the smooth error, the number of flips, and the fp64 arbiter (as for config 2 below).
    rep = helpers.disparity_report(disparity, g['disparity'])
    print('config1 disparity', rep)
    flipped = round(rep['flips'] * disparity.numel())
    assert rep['mae_noflip'] <= 1e-4, rep
    # allowance from the same-run fp64 arbiter (helpers.flip_allowance), not a constant
    allowed, _, ref_flips = helpers.flip_allowance({k: v.cpu() for k, v in net.state_dict().items()}, ld, rd, shortcut, 63,
                                                   g['disparity'], slack=2)
    print('config1: reference fp32 flips vs fp64 %d -> allowance %d, seen %d' % (ref_flips, allowed, flipped))
    assert flipped <= allowed, rep
    # raw MAE: 1e-3 (north_star) with no flip; every flipped arg-max may add its own jump (at most 63 px / 32 768 px)
    assert rep['mae'] <= TOL_DISPARITY_MAE + flipped * 63.0 / disparity.numel(), rep
    p32 = {k: v.cpu() for k, v in net.state_dict().items()}
    with torch.no_grad():
        disp64 = oracle.hot_path(oracle.cast_params(p32, torch.float64), ld.double(), rd.double(),
                                 shortcut.double(), 63)
    cpu64 = helpers.disparity_report(g['disparity'], disp64)
    gpu64 = helpers.disparity_report(disparity, disp64)
    print('config1 arbiter: reference fp32 vs fp64', cpu64, ' gpu vs fp64', gpu64)
    assert gpu64['mae_noflip'] <= 1e-4 and gpu64['flips'] <= cpu64['flips'] + 1e-4, (gpu64, cpu64)
    # estimator alone on the identical (GPU) cost volume
    est = oracle.subpixel_map(cost.cpu())
    assert helpers.maxdiff(disparity, est) <= TOL_EST_MAX


def test_config1_full_network_on_gpu(dev):
    """The drop-in: PdsNetwork.default end to end on the library (virtual padding, HIP descriptor network, hot path)."""
    g = helpers.golden('g6_config1')
    net = helpers.seeded(lambda: pds.PdsNetwork.default(63)).eval().to(dev)
    left, right = helpers.images(1, 128, 256)
    with torch.no_grad():
        out = net(left.to(dev), right.to(dev))
    assert out.shape == (1, 128, 256)
    rep = helpers.disparity_report(out, g['disparity'])
    print('config1 full network (GPU embedding)', rep)
    # the GPU descriptors differ from the golden (CPU) ones by ~1e-5: a few arg-max flips; the raw MAE is 1e-3
    # (north_star) plus what every counted flip may add (at most 63 px / 32 768 px), as in the hot-path test above
    flipped = round(rep['flips'] * out.numel())
    assert flipped <= 6, rep
    assert rep['mae'] <= TOL_DISPARITY_MAE + flipped * 63.0 / out.numel(), rep
    assert rep['mae_noflip'] <= 1e-4, rep
    net.train()
    with torch.no_grad():
        cost = net(left.to(dev), right.to(dev))
    assert cost.shape == (1, 32, 128, 256)   # training mode returns the cost volume (network.py:50-52)


def test_config2_full_size_vs_oracle_and_golden(dev):
    """BASELINE configs[1]: 960x540, D=192.  Stage-wise parity against the oracle run on the host
    and against the committed statistics of the reference."""
    g = helpers.golden('g7_config2_stats')
    net, ld, rd, shortcut = hot_path_inputs(191, 1, 540, 960)
    assert abs(helpers.checksum(net.state_dict()) - g['weight_checksum'].item()) < 1e-9
    ms, cost, disparity = run_hot_path(net, dev, ld, rd, shortcut, fuse=False)
    assert ms.shape == (1, 8, 48, 144, 240) and cost.shape == (1, 96, 576, 960)
    assert helpers.maxdiff(ms[:, :, ::4, ::16, ::16], g['signatures_sub']) <= TOL_SIGNATURES
    assert helpers.maxdiff(cost[:, ::8, ::32, ::32], g['cost_sub']) <= TOL_COST_MAX
    p = {k: v.cpu() for k, v in net.state_dict().items()}
    ms_o, cost_o, disp_o = oracle.hot_path(p, ld, rd, shortcut, 191, return_stages=True)
    assert helpers.maxdiff(ms, ms_o) <= TOL_SIGNATURES
    assert helpers.maxdiff(cost, cost_o) <= TOL_COST_MAX
    assert helpers.meandiff(cost, cost_o) <= TOL_COST_MEAN
    # End-to-end disparity.  With random-init weights the cost volume has near-ties, and ANY fp32
    # re-association flips a handful of arg-maxes by ~100 px each: the reference's own fp32 output
    # differs from its fp64 output by MAE 5.4e-4 / 4 flips at this size (re-measured with
    # tools/noise_floor.py), so GPU-vs-CPU MAE is (GPU flips + CPU flips) * ~1.5e-4.  Gates:
    #   smooth error (pixels that did not flip)  <= 1e-4 px
    #   flipped arg-maxes                        <= 8 pixels of 552 960 (the reference's fp32-vs-fp64 count is 4)
    #   raw MAE                                  <= 1e-3 (north_star), also against the fp64 arbiter in
    #                                               test_config2_fp64_arbiter
    rep = helpers.disparity_report(disparity, disp_o)
    print('config2 disparity vs oracle', rep)
    # allowance from the same-run fp64 arbiter (helpers.flip_allowance): 2 x the reference's own fp32-vs-fp64 flips + 2
    allowed, _, ref_flips = helpers.flip_allowance(p, ld, rd, shortcut, 191, disp_o)
    print('config2: reference fp32 flips vs fp64 %d -> allowance %d, seen %d' %
          (ref_flips, allowed, round(rep['flips'] * disparity.numel())))
    assert round(rep['flips'] * disparity.numel()) <= allowed, rep
    assert rep['mae_noflip'] <= 1e-4, rep
    assert rep['mae'] <= TOL_DISPARITY_MAE, rep
    # the committed sub-sample of the reference's own output (2 160 pixels: one ~100 px flip alone is 0.046 of MAE):
    # at most one flipped sample, the others within the smooth tolerance
    sub = helpers.disparity_report(disparity[:, ::16, ::16], g['disparity_sub'])
    sub_flipped = round(sub['flips'] * g['disparity_sub'].numel())
    assert sub_flipped <= 1 and sub['mae_noflip'] <= 1e-4, sub
    assert sub['mae'] <= TOL_DISPARITY_MAE + sub_flipped * 191.0 / g['disparity_sub'].numel(), sub
    # fused eval path at full size
    _, _, fused = run_hot_path(net, dev, ld, rd, shortcut, fuse=True)
    rep_f = helpers.disparity_report(fused, disp_o)
    print('config2 fused disparity vs oracle', rep_f)
    assert round(rep_f['flips'] * fused.numel()) <= allowed and rep_f['mae_noflip'] <= 1e-4, rep_f
    assert rep_f['mae'] <= TOL_DISPARITY_MAE, rep_f
    # BASELINE configs[2] at full size: the 48 planes as 2 / 4 / 8 shards of 24 / 12 / 6 planes (what the ranks of
    # distributed.ShardedMatching compute, here one after the other on this GPU); the gathered signatures must equal
    # the unsharded ones bit for bit, hence everything downstream too
    matching = net._matching
    with torch.no_grad():
        for shards in (2, 4, 8):
            per = 48 // shards
            parts = []
            for r in range(shards):
                matching.set_disparity_shard((r * per, per))
                parts.append(matching(ld.to(dev), rd.to(dev)))
            matching.set_disparity_shard(None)
            gathered = torch.cat(parts, dim=2)
            assert torch.equal(gathered, ms), shards
            del parts
        assert torch.equal(net._regularization.forward_with_estimator(gathered, shortcut.to(dev), net._estimator), fused)


def test_config2_fp64_arbiter(dev):
    """the GPU must not be further from the truth than the reference is.  The truth is the
    oracle in fp64; 1e-3 MAE is the stated bar for the distance to it."""
    net, ld, rd, shortcut = hot_path_inputs(191, 1, 540, 960)
    p32 = {k: v.cpu() for k, v in net.state_dict().items()}
    p64 = oracle.cast_params(p32, torch.float64)
    with torch.no_grad():
        disp32 = oracle.hot_path(p32, ld, rd, shortcut, 191)
        disp64 = oracle.hot_path(p64, ld.double(), rd.double(), shortcut.double(), 191)
    _, _, disparity = run_hot_path(net, dev, ld, rd, shortcut, fuse=True)
    cpu = helpers.disparity_report(disp32, disp64)
    gpu = helpers.disparity_report(disparity, disp64)
    n = disparity.numel()
    cpu_flips, gpu_flips = round(cpu['flips'] * n), round(gpu['flips'] * n)
    print('config2 arbiter: cpu fp32 vs fp64', cpu, ' gpu vs fp64', gpu, ' flips cpu %d gpu %d' % (cpu_flips, gpu_flips))
    # Gates.  An arg-max flip moves one pixel by ~100 px = 1.8e-4 of MAE at this size, so MAE is a
    # flip counter in disguise: the GPU may flip at most two pixels more than the reference's own fp32 run does against
    # fp64, its smooth error (non-flipped pixels) must be within 1e-4 px and no worse than 2x the reference's smooth error
    # + 1e-5, and the raw MAE stays under north_star's 1e-3.
    assert gpu_flips <= cpu_flips + 2, (gpu, cpu)
    assert gpu['mae_noflip'] <= 1e-4, gpu
    assert gpu['mae_noflip'] <= 2.0 * cpu['mae_noflip'] + 1e-5, (gpu, cpu)
    assert gpu['mae'] <= TOL_DISPARITY_MAE, gpu


def test_config4_kitti_shape_batch(dev):
    """BASELINE configs[3]: 375x1242 (pads top 9 / left 38), D=256 -> run at batch 2 to bound the
    oracle's host time; checks unpad offsets and batch handling."""
    net, ld, rd, shortcut = hot_path_inputs(255, 2, 375, 1242)
    assert ld.shape == (2, 64, 96, 320)
    ms, cost, unfused = run_hot_path(net, dev, ld, rd, shortcut, fuse=False)
    p = {k: v.cpu() for k, v in net.state_dict().items()}
    ms_o, cost_o, disp_o = oracle.hot_path(p, ld, rd, shortcut, 255, return_stages=True)
    # stage-wise first: flips cannot hide a regression here
    assert helpers.maxdiff(ms, ms_o) <= TOL_SIGNATURES
    assert helpers.maxdiff(cost, cost_o) <= TOL_COST_MAX
    assert helpers.meandiff(cost, cost_o) <= TOL_COST_MEAN
    del cost
    _, _, disparity = run_hot_path(net, dev, ld, rd, shortcut, fuse=True)
    rep = helpers.disparity_report(disparity, disp_o)
    print('config4 disparity vs oracle', rep)
    allowed, _, ref_flips = helpers.flip_allowance(p, ld, rd, shortcut, 255, disp_o)   # (983 040 pixels)
    print('config4: reference fp32 flips vs fp64 %d -> allowance %d' % (ref_flips, allowed))
    assert round(rep['flips'] * disparity.numel()) <= allowed and rep['mae_noflip'] <= 1e-4, rep
    assert rep['mae'] <= TOL_DISPARITY_MAE, rep
    out = net._size_adapter.unpad(disparity)
    assert out.shape == (2, 375, 1242)


# ------------------------------------------------------------------------------- ABI properties
def test_hot_path_is_graph_capturable(dev):
    """include/pds_hip.h promises no allocation / synchronisation inside the library: the whole hot path
    must record into a HIP graph and replay bit-identically."""
    net, ld, rd, shortcut = hot_path_inputs(63, 1, 128, 256)
    net = net.to(dev)
    ld, rd, sc = ld.to(dev), rd.to(dev), shortcut.to(dev)
    with torch.no_grad():
        def run():
            ms = net._matching(ld, rd)
            return net._regularization.forward_with_estimator(ms, sc, net._estimator)
        eager = run().clone()          # also warms up workspaces and kernel attributes
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            run()                      # warm-up on the capture stream
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                captured = run()
        for _ in range(3):
            captured.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(captured, eager)


def test_config4_full_batch_values(dev):
    """BASELINE configs[3] at its full batch of 4 (375x1242 -> 96x320 descriptors, D=256): shapes, ranges, and VALUES:
    the oracle evaluates the batch entries one at a time on the host (InstanceNorm statistics are per batch entry, so
    entry b of the batched HIP result must equal the oracle on entry b alone); signatures, cost (strided sub-sample)
    and disparity are checked for the first and the last entry."""
    torch.manual_seed(0)
    net = pds.PdsNetwork.default(255).eval()
    params = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.to(dev)
    g = torch.Generator().manual_seed(12)
    ld = torch.randn(4, 64, 96, 320, generator=g)
    rd = torch.randn(4, 64, 96, 320, generator=g)
    sc = torch.randn(4, 8, 96, 320, generator=g)
    with torch.no_grad():
        ms = net._matching(ld.to(dev), rd.to(dev))
        cost = net._regularization(ms, sc.to(dev))
        cost_sub = cost[:, ::8, ::16, ::16].cpu()
        del cost
        disparity = net._regularization.forward_with_estimator(ms, sc.to(dev), net._estimator)
    assert ms.shape == (4, 8, 64, 96, 320) and disparity.shape == (4, 384, 1280)
    assert bool(torch.isfinite(disparity).all())
    assert float(disparity.min()) >= 0.0 and float(disparity.max()) <= 254.0 + 1e-3
    for b in (0, 3):
        with torch.no_grad():
            ms_o, cost_o, disp_o = oracle.hot_path(params, ld[b:b + 1], rd[b:b + 1], sc[b:b + 1], 255,
                                                   return_stages=True)
        assert helpers.maxdiff(ms[b:b + 1], ms_o) <= TOL_SIGNATURES, b
        assert helpers.maxdiff(cost_sub[b:b + 1], cost_o[:, ::8, ::16, ::16]) <= TOL_COST_MAX, b
        rep = helpers.disparity_report(disparity[b:b + 1], disp_o)
        print('config4 batch entry', b, rep)
        allowed, _, ref_flips = helpers.flip_allowance(params, ld[b:b + 1], rd[b:b + 1], sc[b:b + 1], 255, disp_o)
        print('config4 batch entry', b, 'reference fp32 flips vs fp64 %d -> allowance %d' % (ref_flips, allowed))
        assert round(rep['flips'] * disp_o.numel()) <= allowed and rep['mae_noflip'] <= 1e-4, rep
        assert rep['mae'] <= TOL_DISPARITY_MAE, rep


def test_stream_pipelines_are_bit_identical(dev):
    """bench.py's default N = 1 schedule (distributed.PairStreams: whole pairs round-robin over three streams, every
    module with one workspace per stream) and the tail-only overlap of distributed.ShardedHotPath without a process
    group: every result must equal the sequential one."""
    from practicaldeepstereo_nips2018_amd.distributed import PairStreams, ShardedHotPath
    net, ld, rd, shortcut = hot_path_inputs(63, 1, 128, 256)
    net = net.to(dev)
    reg, est = net._regularization, net._estimator

    def tail(signatures, sc):
        return reg.forward_with_estimator(signatures, sc, est)

    def whole(a, b, c):
        return tail(net._matching(a, b), c)

    pairs = []
    g = torch.Generator().manual_seed(77)
    for _ in range(7):
        noise = torch.randn(ld.shape, generator=g) * 0.05
        pairs.append(((ld + noise).to(dev), (rd - noise).to(dev), shortcut.to(dev)))
    with torch.no_grad():
        sequential = [whole(a, b, c).clone() for a, b, c in pairs]
        streams = PairStreams(whole, streams=3)
        dealt = [streams.submit(a, b, c) for a, b, c in pairs]
        streams.drain()
        hot_path = ShardedHotPath(net._matching, tail, max_pending=2)
        overlapped = [hot_path.submit(a, b, c) for a, b, c in pairs]
        hot_path.drain()
    for want, got, got2 in zip(sequential, dealt, overlapped):
        assert torch.equal(got, want) and torch.equal(got2, want)


# ----------------------------------------------------------------- weights kept in the workspace between calls
def _resident_case(dev):
    g = torch.Generator().manual_seed(5)
    left = torch.randn(1, 64, 32, 64, generator=g).to(dev)
    right = torch.randn(1, 64, 32, 64, generator=g).to(dev)
    shortcut = torch.randn(1, 8, 32, 64, generator=g).to(dev)

    def run(n):
        ms = n._matching(left, right)
        return ms, n._regularization.forward_with_estimator(ms, shortcut, n._estimator)

    def expected_of(n):
        fresh = pds.PdsNetwork.default(63).eval().to(dev)   # a module that has never packed anything
        fresh.load_state_dict(n.state_dict())
        return run(fresh)
    return run, expected_of


def test_resident_weights_follow_parameter_updates(dev):
    """A frozen network's workspaces keep the re-laid-out weights and skip the packing launches while the parameter
    values are unchanged (weights_resident of include/pds_hip.h); in-place updates through the parameters (optimizer
    step, load_state_dict) are noticed through their version counters, edits through ``.data`` after
    ``invalidate_weights()``."""
    torch.manual_seed(0)
    net = pds.PdsNetwork.default(63).eval().to(dev).freeze_weights()
    run, expected_of = _resident_case(dev)
    with torch.no_grad():
        first = run(net)
        again = run(net)            # second call: packing skipped
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
        for p in net.parameters():  # in-place update bumps p._version
            p.mul_(1.01)
        updated = run(net)
        expected = expected_of(net)
        assert not torch.equal(updated[0], first[0])
        assert torch.equal(updated[0], expected[0]) and torch.equal(updated[1], expected[1])
        # an edit behind autograd's back (EMA swap, old-style init): no version bump, so the frozen module must be told
        for p in net.parameters():
            p.data.copy_(p.data * 0.97)
        net.invalidate_weights()
        swapped = run(net)
        expected = expected_of(net)
        assert not torch.equal(swapped[0], updated[0])
        assert torch.equal(swapped[0], expected[0]) and torch.equal(swapped[1], expected[1])
        # load_state_dict and .to() invalidate on their own
        state = {k: v * 1.02 for k, v in net.state_dict().items()}
        net.load_state_dict(state)
        loaded = run(net)
        expected = expected_of(net)
        assert torch.equal(loaded[0], expected[0]) and torch.equal(loaded[1], expected[1])


def test_unfrozen_modules_always_repack(dev):
    """Default (not frozen): the weights are re-laid out on every call, so ``p.data.copy_()`` -- which no version
    counter sees -- takes effect immediately; and train() thaws a frozen network."""
    torch.manual_seed(0)
    net = pds.PdsNetwork.default(63).eval().to(dev)
    run, expected_of = _resident_case(dev)
    with torch.no_grad():
        first = run(net)
        for p in net.parameters():
            p.data.copy_(p.data * 1.03)
        edited = run(net)
        expected = expected_of(net)
        assert not torch.equal(edited[0], first[0])
        assert torch.equal(edited[0], expected[0]) and torch.equal(edited[1], expected[1])
        net.freeze_weights()
        run(net)
        net.train()
        assert not net._matching._weights_frozen and not net._regularization._weights_frozen
        net.eval()
        for p in net.parameters():
            p.data.copy_(p.data * 0.99)
        thawed = run(net)
        expected = expected_of(net)
        assert torch.equal(thawed[0], expected[0]) and torch.equal(thawed[1], expected[1])


def test_failed_call_leaves_no_resident_key(dev):
    """The residency key is committed only after the native call succeeded: a call that raised in between (here: a
    left/right shape the entry point refuses) must not make the next call skip its weight re-layout."""
    torch.manual_seed(0)
    net = pds.PdsNetwork.default(63).eval().to(dev).freeze_weights()
    run, expected_of = _resident_case(dev)
    matching = net._matching
    with torch.no_grad():
        good = run(net)
        slot_keys = dict(matching._workspace._keys)
        assert slot_keys, 'a frozen module records its key after a successful call'
        original = _lib.check

        def failing(rc, what):
            raise RuntimeError('injected failure in %s' % what)
        _lib.check = failing
        try:
            with pytest.raises(RuntimeError):
                run(net)
        finally:
            _lib.check = original
        assert not matching._workspace._keys, 'the failed call must leave no key behind'
        again = run(net)
    assert torch.equal(again[0], good[0]) and torch.equal(again[1], good[1])


def test_unpad_is_folded_into_the_estimator_store(dev):
    """SURVEY.md 8 f3, second half (size_adapter.py:45-52): the whole-network eval output is the contiguous cropped
    image written by the fused kernel, bit-identical to cropping the padded result; odd crops (KITTI: 9 rows, 38
    columns) take the unaligned store path."""
    for height, width in ((100, 154), (128, 192), (375 // 3, 1242 // 6)):
        net = helpers.seeded(lambda: pds.PdsNetwork.default(63)).eval().to(dev)
        left, right = helpers.images(1, height, width)
        with torch.no_grad():
            out = net(left.to(dev), right.to(dev))
            top, lft = net._size_adapter.padding()
            signatures, shortcut = net._signatures_from_unpadded(left.to(dev), right.to(dev))
            padded = net._regularization.forward_with_estimator(signatures, shortcut, net._estimator)
        assert out.shape == (1, height, width) and out.is_contiguous()
        assert torch.equal(out, padded[..., top:, lft:]), (height, width)


@pytest.mark.parametrize('scale', [0.03, 30.0])
def test_fused_matching_descriptor_scale(dev, scale):
    """The 64-channel layers split their fp32 operands into two fp16 parts (conv2d_x3.hip).  Behind an InstanceNorm the
    inputs are O(1) by construction; the first residual sum x1 = norm(t2) + x0 is a PLAIN tensor that carries the scale of
    the descriptors (x0 is linear in them), taken as it is (|x| < 65 504).  Descriptors 30x larger / smaller than a
    normalised tensor must still match the oracle to the signature tolerance, relative to the signatures' own scale."""
    op = helpers.seeded(pds.MatchingOperation, seed=11)
    p = helpers.prefixed(op.state_dict(), '_m._operation')
    g = torch.Generator().manual_seed(12)
    left = torch.randn(1, 64, 24, 40, generator=g) * scale
    right = torch.randn(1, 64, 24, 40, generator=g) * scale
    ref = oracle.matching_with_operation(p, '_m', left, right, 7)
    net = pds.Matching(7, op).to(dev)
    with torch.no_grad():
        out = net(left.to(dev), right.to(dev))
    assert torch.isfinite(out).all()
    assert helpers.maxdiff(out, ref) <= TOL_SIGNATURES * max(1.0, float(ref.abs().max()) / 4.0)


def test_frozen_network_alternating_shapes_is_repeatable(dev):
    """A frozen network re-uses its workspaces: the tile-queue counters of conv2d_x3 live behind the packed weights and
    are re-zeroed by the last workgroup of every launch (no memset per layer).  Alternating between two input shapes
    (different arena layouts over the same buffers) and repeating each several times must reproduce the first result of
    that shape bit for bit -- a counter left dirty would skip or repeat tiles."""
    torch.manual_seed(0)
    net = pds.PdsNetwork.default(63).eval().to(dev).freeze_weights()
    g = torch.Generator().manual_seed(5)
    shapes = [(1, 128, 256), (1, 192, 320), (2, 128, 256)]
    inputs = [(torch.rand(b, 3, h, w, generator=g).to(dev) * 255, torch.rand(b, 3, h, w, generator=g).to(dev) * 255)
              for b, h, w in shapes]
    with torch.no_grad():
        first = [net(left, right).clone() for left, right in inputs]
        for _ in range(3):
            for i in (2, 0, 1, 1, 0, 2):
                again = net(*inputs[i])
                assert torch.equal(again, first[i]), 'shape %s changed on re-use' % (shapes[i],)
    for out in first:
        assert torch.isfinite(out).all()
