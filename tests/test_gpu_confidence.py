"""GPU (-m gpu): the confidence map of the sub-pixel MAP estimator (SubpixelMap.with_confidence,
Regularization.forward_with_estimator(..., with_confidence=True), PdsNetwork.forward_with_confidence).

Contract: k* = first arg-max over the planes, W = the valid taps {k* + j : -T <= j <= T, 0 <= k* + j < P} the disparity
uses (T = half_support_window / disparity_step), c = sum_{k in W} exp(s_k) / sum_k exp(s_k), float32 in (0, 1].
The fp64 restatement below is the arbiter; the disparity of every confidence call must equal the plain call's bit for
bit.
"""
import math

import pytest
import torch

from tests import helpers
import practicaldeepstereo_nips2018_amd as pds

pytestmark = pytest.mark.gpu

# non-flip gates of the fused tail (fp32 sums over <= 256 planes, the streaming rescale and the two parts' merge).
# Measured on MI355X: max 1.2e-6 (config 4, batch entry 0; <= 1.8e-7 everywhere else), mean <= 3.7e-8.
TOL_FUSED_MAX = 5e-6
TOL_FUSED_MEAN = 2e-7
# stand-alone estimator against fp64 (same arg-max at every pixel): measured max 1.9e-7
TOL_STANDALONE_MAX = 1e-6
# the fused and the unfused cost volumes differ by rounding (<= 1e-4, TOL_COST_MAX of test_gpu_parity.py): only a pixel
# whose two largest planes are closer than this can take another arg-max, and those are the flips counted
NEAR_TIE = 2e-4
FLIPS_ALLOWED = 2   # as the disparity test of the fused estimator (test_fused_estimator_support_windows)


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def confidence64(sim, hw, step):
    """fp64 restatement: log_softmax over the planes, the window gathered around the first arg-max, logsumexp, exp.
    Runs on the tensor's own device (PyTorch, float64)."""
    s = sim.detach().double()
    planes, t = s.shape[1], hw // step
    lsm = torch.log_softmax(s, dim=1)
    k = s.argmax(dim=1, keepdim=True)   # first occurrence
    idx = k + torch.arange(-t, t + 1, device=s.device).view(1, -1, 1, 1)
    valid = (idx >= 0) & (idx < planes)
    window = lsm.gather(1, idx.clamp(0, planes - 1)).masked_fill(~valid, -math.inf)
    return torch.logsumexp(window, dim=1).exp()


def near_ties(sim):
    """Pixels whose two largest planes are within NEAR_TIE: the only ones where another rounding can move the arg-max."""
    top = sim.detach().topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) < NEAR_TIE


def check_gates(conf, ref, ties, what):
    """Non-flip max / mean gates; at near-tie pixels a differing confidence is counted as a flip."""
    delta = (conf.double() - ref.double().to(conf.device)).abs()
    calm = ~ties.to(conf.device)
    assert bool(calm.any()), what
    worst, mean = float(delta[calm].max()), float(delta[calm].mean())
    flips = int(((delta > TOL_FUSED_MAX) & ~calm).sum())
    print('%s: non-flip max %.3e mean %.3e, near ties %d, flips %d' % (what, worst, mean, int((~calm).sum()), flips))
    assert worst <= TOL_FUSED_MAX and mean <= TOL_FUSED_MEAN and flips <= FLIPS_ALLOWED, (what, worst, mean, flips)


def check_range(conf):
    assert bool(torch.isfinite(conf).all())
    assert float(conf.min()) > 0.0 and float(conf.max()) <= 1.0


# ------------------------------------------------------------------------------- known answers
def both_vec_paths(values):
    """[P] -> [1, P, 1, 1] (one pixel per lane) and [1, P, 1, 2] (two pixels per lane) on the GPU."""
    v = torch.tensor(values, dtype=torch.float32).view(1, -1, 1, 1)
    return [v, torch.cat([v, v], dim=3)]


@pytest.mark.parametrize('hw,step,expected', [(2, 1, 0.792906599), (2, 2, 0.605520741)])
def test_reference_vector_known_answers(dev, hw, step, expected):
    # the reference's own vector (test_estimator.py:14-27)
    for sim in both_vec_paths([0.1, 0.4, 0.3, 0.2, 0.3]):
        disparity, conf = pds.SubpixelMap(hw, step).with_confidence(sim.to(dev))
        assert torch.equal(disparity, pds.SubpixelMap(hw, step)(sim.to(dev)))
        assert abs(conf.cpu() - expected).max().item() <= 1e-6, conf


@pytest.mark.parametrize('planes,hw,step', [(7, 4, 2), (12, 4, 2), (9, 2, 2), (30, 8, 2), (40, 12, 2)])
def test_all_equal_planes(dev, planes, hw, step):
    # first arg-max: plane 0, so |W| = T + 1
    for sim in both_vec_paths([0.25] * planes):
        conf = pds.SubpixelMap(hw, step).with_confidence(sim.to(dev))[1].cpu()
        expected = min(hw // step + 1, planes) / planes
        assert abs(conf - expected).max().item() <= 1e-6, (conf, expected)


def test_single_plane_is_exactly_one(dev):
    sim = torch.randn(2, 1, 5, 6, generator=torch.Generator().manual_seed(5))
    for hw, step in [(4, 2), (2, 1), (12, 2)]:
        conf = pds.SubpixelMap(hw, step).with_confidence(sim.to(dev))[1]
        assert torch.equal(conf.cpu(), torch.ones(2, 5, 6))


@pytest.mark.parametrize('hw,step', [(4, 2), (8, 2), (12, 2)])
def test_window_covering_every_plane(dev, hw, step):
    t = hw // step
    planes = t + 1
    sim = torch.randn(1, planes, 8, 9, generator=torch.Generator().manual_seed(6))
    sim[:, 0] = sim.max(dim=1).values + 0.5   # the arg-max at plane 0: W covers every plane
    conf = pds.SubpixelMap(hw, step).with_confidence(sim.to(dev))[1]
    assert float(conf.max()) <= 1.0
    assert float(conf.min()) >= 1.0 - planes * 2.0 ** -23


@pytest.mark.parametrize('hw,step', [(4, 2), (2, 1), (12, 2)])
def test_negative_infinity_planes(dev, hw, step):
    g = torch.Generator().manual_seed(7)
    sim = torch.randn(2, 24, 6, 7, generator=g)
    sim[torch.rand(sim.shape, generator=g) < 0.4] = -math.inf
    sim[:, :3] = -math.inf        # leading -inf planes: the running maximum starts at -inf
    sim[:, 11] = torch.randn(2, 6, 7, generator=g)   # every pixel keeps a finite plane
    disparity, conf = pds.SubpixelMap(hw, step).with_confidence(sim.to(dev))
    assert not bool(torch.isnan(conf).any())
    check_range(conf)
    assert torch.equal(disparity, pds.SubpixelMap(hw, step)(sim.to(dev)))
    err = helpers.maxdiff(conf, confidence64(sim, hw, step))
    print('-inf planes hw %d step %d vs fp64: max %.3e' % (hw, step, err))
    assert err <= TOL_STANDALONE_MAX


# ------------------------------------------------------------------------------- standalone estimator vs fp64
def test_standalone_golden_inputs(dev):
    g = helpers.golden('g5_subpixel_map')
    for name in sorted(k[:-3] for k in g if k.endswith('_in')):
        hw, step = [int(v) for v in g[name + '_cfg']]
        sim = g[name + '_in'].to(dev)
        disparity, conf = pds.SubpixelMap(hw, step).with_confidence(sim)
        assert torch.equal(disparity, pds.SubpixelMap(hw, step)(sim)), name
        check_range(conf)
        err = helpers.maxdiff(conf, confidence64(sim, hw, step))
        print('golden %s vs fp64: max %.3e' % (name, err))
        assert err <= TOL_STANDALONE_MAX, name


@pytest.mark.parametrize('shape,hw,step', [((2, 32, 17, 23), 4, 2), ((1, 96, 64, 128), 4, 2),
                                           ((3, 7, 5, 4), 2, 1), ((1, 64, 33, 31), 8, 2),
                                           ((1, 48, 16, 20), 12, 2), ((1, 96, 9, 11), 2, 2)])
def test_standalone_random_vs_fp64(dev, shape, hw, step):
    # the shapes of test_subpixel_map_random_vs_oracle: odd pixel counts (one pixel per lane), the wide-window fallback
    sim = torch.randn(*shape, generator=torch.Generator().manual_seed(3)).to(dev)
    disparity, conf = pds.SubpixelMap(hw, step).with_confidence(sim)
    assert torch.equal(disparity, pds.SubpixelMap(hw, step)(sim))
    assert conf.shape == disparity.shape and conf.is_contiguous()
    check_range(conf)
    # the arg-max is that of the same fp32 values, so every pixel agrees with fp64
    err = helpers.maxdiff(conf, confidence64(sim, hw, step))
    print('standalone %s hw %d step %d vs fp64: max %.3e' % (shape, hw, step, err))
    assert err <= TOL_STANDALONE_MAX


# ------------------------------------------------------------------------------- fused tail
@pytest.mark.parametrize('half_support_window,step', [(2, 2), (4, 2), (6, 2), (8, 2)])
def test_fused_confidence_support_windows(dev, half_support_window, step):
    """T = 1, 2, 3 (on the T = 4 build), 4: the fused sweep's confidence against the standalone one and fp64 on the
    cost volume of the same sweep (the inputs of test_fused_estimator_support_windows)."""
    reg = helpers.seeded(pds.Regularization).to(dev)
    est = pds.SubpixelMap(half_support_window, step)
    gen = torch.Generator().manual_seed(77)
    signatures = torch.randn(2, 8, 16, 32, 48, generator=gen).to(dev)
    shortcut = torch.randn(2, 8, 32, 48, generator=gen).to(dev)
    with torch.no_grad():
        cost = reg(signatures, shortcut)
        standalone = est.with_confidence(cost)[1]
        plain = reg.forward_with_estimator(signatures, shortcut, est, with_confidence=False)
        disparity, conf = reg.forward_with_estimator(signatures, shortcut, est, with_confidence=True)
    assert conf.shape == disparity.shape == (2, 128, 192) and conf.is_contiguous()
    assert torch.equal(disparity, plain)
    check_range(conf)
    ties = near_ties(cost)
    check_gates(conf, standalone, ties, 'T=%d vs standalone' % (half_support_window // step))
    check_gates(conf, confidence64(cost, half_support_window, step), ties,
                'T=%d vs fp64' % (half_support_window // step))


def test_fused_confidence_refuses_backward(dev):
    reg = helpers.seeded(pds.Regularization).to(dev)
    gen = torch.Generator().manual_seed(78)
    signatures = torch.randn(1, 8, 16, 32, 48, generator=gen).to(dev).requires_grad_()
    shortcut = torch.randn(1, 8, 32, 48, generator=gen).to(dev)
    disparity, conf = reg.forward_with_estimator(signatures, shortcut, pds.SubpixelMap(), with_confidence=True)
    with pytest.raises(NotImplementedError, match='backward'):
        (disparity.sum() + conf.sum()).backward()


# ------------------------------------------------------------------------------- whole network
def unfused_cost(net, left, right):
    """The GPU's own unfused cost volume of the padded pair (same signatures as the fused call)."""
    with torch.no_grad():
        signatures, shortcut = net._signatures_from_unpadded(left, right)
        return net._regularization(signatures, shortcut)


def test_config2_full_size(dev):
    """Config 2 (960x540, D = 192): seed-0 network, seed-1 images."""
    net = helpers.seeded(lambda: pds.PdsNetwork.default(191)).eval().to(dev)
    left, right = [x.to(dev) for x in helpers.images(1, 540, 960)]
    with torch.no_grad():
        disparity, conf = net.forward_with_confidence(left, right)
        plain = net(left, right)
    assert conf.shape == disparity.shape == (1, 540, 960) and conf.is_contiguous()
    assert torch.equal(disparity, plain)
    check_range(conf)
    cost = unfused_cost(net, left, right)
    ref = net._size_adapter.unpad(confidence64(cost, 4, 2))
    ties = net._size_adapter.unpad(near_ties(cost))
    del cost
    check_gates(conf, ref, ties, 'config 2 vs fp64')


@pytest.mark.parametrize('height,width', [(100, 154), (128, 192), (125, 207)])
def test_crop_folding(dev, height, width):
    net = helpers.seeded(lambda: pds.PdsNetwork.default(63)).eval().to(dev)
    left, right = [x.to(dev) for x in helpers.images(1, height, width)]
    with torch.no_grad():
        disparity, conf = net.forward_with_confidence(left, right)
        plain = net(left, right)
        signatures, shortcut = net._signatures_from_unpadded(left, right)
        padded = net._regularization.forward_with_estimator(signatures, shortcut, net._estimator,
                                                            with_confidence=True)[1]
    assert conf.shape == (1, height, width) and conf.is_contiguous()
    assert torch.equal(disparity, plain)
    assert torch.equal(conf, net._size_adapter.unpad(padded))


def test_unfused_fallback_matches_fused(dev):
    """fuse_estimator = False: Regularization + SubpixelMap.with_confidence + unpad of both maps."""
    net = helpers.seeded(lambda: pds.PdsNetwork.default(63)).eval().to(dev)
    left, right = [x.to(dev) for x in helpers.images(1, 100, 154)]
    with torch.no_grad():
        fused = net.forward_with_confidence(left, right)
        net.fuse_estimator = False
        unfused = net.forward_with_confidence(left, right)
        cost = unfused_cost(net, left, right)
    assert unfused[1].shape == (1, 100, 154)
    unpad = net._size_adapter.unpad
    assert torch.equal(unfused[0], unpad(pds.SubpixelMap()(cost)))
    assert torch.equal(unfused[1], unpad(pds.SubpixelMap().with_confidence(cost)[1]))
    check_gates(fused[1], unfused[1], net._size_adapter.unpad(near_ties(cost)), 'fused vs unfused network')


def test_config4_batch2(dev):
    """Config-4 shape (375x1242, D = 256) at batch 2: every entry against fp64 on its own unfused cost volume (batch 2
    is not assumed to equal batch 1 bit for bit)."""
    net = helpers.seeded(lambda: pds.PdsNetwork.default(255)).eval().to(dev)
    left, right = [x.to(dev) for x in helpers.images(2, 375, 1242)]
    with torch.no_grad():
        disparity, conf = net.forward_with_confidence(left, right)
        plain = net(left, right)
        signatures, shortcut = net._signatures_from_unpadded(left, right)
    assert conf.shape == disparity.shape == (2, 375, 1242) and conf.is_contiguous()
    assert torch.equal(disparity, plain)
    check_range(conf)
    for b in range(2):
        with torch.no_grad():
            cost = net._regularization(signatures[b:b + 1], shortcut[b:b + 1])
        ref = net._size_adapter.unpad(confidence64(cost, 4, 2))
        ties = net._size_adapter.unpad(near_ties(cost))
        del cost
        check_gates(conf[b:b + 1], ref, ties, 'config 4 entry %d vs fp64' % b)
