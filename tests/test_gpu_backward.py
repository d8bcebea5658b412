"""GPU (-m gpu): backward of the HIP modules against torch autograd through the oracle in fp64.

Reference behaviour: pds_trainer.py:40-46 calls loss.backward() through network.py:38-52 in training mode,
i.e. through Matching, MatchingOperation and Regularization (the estimator is inference-only, estimator.py:19).
Tolerance: every gradient tensor within 2e-3 of the fp64 gradient, relative to that tensor's largest entry
(fp32 accumulation over up to ~1e6 terms on both sides of an InstanceNorm)."""
import os

import numpy as np
import pytest
import torch

from oracle import pds_oracle as oracle
from tests import helpers
import practicaldeepstereo_nips2018_amd as pds

pytestmark = pytest.mark.gpu
REL_TOL = 2e-3


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def relative_error(got, want):
    want = want.double().cpu()
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-12))


def oracle_grads(function, tensors, params, weight, dtype=torch.float64):
    """CPU autograd of sum(function(...) * weight) in ``dtype`` (fp64 = the reference gradient)."""
    tensors64 = [t.detach().to(dtype).cpu().requires_grad_(True) for t in tensors]
    params64 = {k: v.detach().to(dtype).cpu().requires_grad_(True) for k, v in params.items()}
    out = function(params64, *tensors64)
    (out * weight.to(dtype).cpu()).sum().backward()
    return out.detach(), [t.grad for t in tensors64], {k: v.grad for k, v in params64.items()}


def check_param_grads(module, prefix, want, noise_floor=None):
    """Every parameter gradient within REL_TOL of the fp64 gradient -- or, where the fp32 CPU oracle itself is
    further than that from fp64 (sums of millions of sign-cancelling terms amplify the fp32 noise of the
    forward pass), within 3x the fp32 CPU oracle's own distance."""
    errors, allowed = {}, {}
    for name, p in module.named_parameters():
        assert p.grad is not None, name
        errors[name] = relative_error(p.grad.detach(), want[prefix + '.' + name])
        floor = relative_error(noise_floor[prefix + '.' + name], want[prefix + '.' + name]) if noise_floor else 0.0
        allowed[name] = max(REL_TOL, 3.0 * floor)
    worst = sorted(errors.items(), key=lambda kv: -kv[1] / allowed[kv[0]])[:4]
    print('largest parameter-gradient errors (error, allowed):', [(n, e, allowed[n]) for n, e in worst])
    for name, err in errors.items():
        assert err <= allowed[name], (name, err, allowed[name])
    return worst[0][1]


def test_shift_concat_backward(dev):
    g = torch.Generator().manual_seed(1)
    left = torch.randn(2, 3, 4, 9, generator=g).to(dev).requires_grad_(True)
    right = torch.randn(2, 3, 4, 9, generator=g).to(dev).requires_grad_(True)
    w = torch.randn(2, 1, 6, 4, 9, generator=g)

    def op(x):  # differentiable mock operation
        return (x * x).sum(1, keepdim=True) + x[:, :1]
    out = pds.Matching(5, op)(left, right)
    (out * w.to(dev)).sum().backward()
    l64 = left.detach().double().cpu().requires_grad_(True)
    r64 = right.detach().double().cpu().requires_grad_(True)
    ref = oracle.matching(l64, r64, 5, op)
    (ref * w.double()).sum().backward()
    assert relative_error(out, ref.detach()) <= 1e-5
    assert relative_error(left.grad, l64.grad) <= 1e-5
    assert relative_error(right.grad, r64.grad) <= 1e-5


@pytest.mark.parametrize('n,h,w', [(2, 9, 11), (3, 16, 24)])
def test_matching_operation_backward(dev, n, h, w):
    op = helpers.seeded(pds.MatchingOperation, seed=3).to(dev)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(n, 128, h, w, generator=g).to(dev).requires_grad_(True)
    weight = torch.randn(n, 8, h, w, generator=g)
    out = op(x)
    (out * weight.to(dev)).sum().backward()
    params = helpers.prefixed(op.state_dict(), '_m')
    ref, (gx,), gp = oracle_grads(lambda p, t: oracle.matching_operation(p, '_m', t), [x], params, weight)
    assert relative_error(out, ref) <= 1e-4
    assert relative_error(x.grad, gx) <= REL_TOL
    print('matching operation worst parameter-gradient error', check_param_grads(op, '_m', gp))


@pytest.mark.parametrize('features,width,shard,blocks', [
    (64, 12, None, 2),        # the default operation: native route (pds_matching_train_fwd / pds_matching_bwd)
    (64, 13, (2, 4), 1),      # a disparity shard (d_begin > 0: partial sums in l0_combine_bwd) on an odd width
    (64, 12, (5, 3), 0),      # no residual block between the two bare convolutions
    (16, 9, None, 1),         # narrow features: still the native route
    (32, 12, None, 2),        # a width the native backward does not take: shift / concat route
    (48, 10, (1, 5), 1),
])
def test_matching_training_route_backward(dev, features, width, shard, blocks):
    """Matching(MatchingOperation) with gradients (matching.py:34-63 under pds_trainer.py:40-46): the native route keeps
    the factorised first layer and differentiates through it; widths it does not take fall back to shift / concat + the
    operation's own backward.  Shards: the gradient of a shard's planes only."""
    op = helpers.seeded(lambda: pds.MatchingOperation(2 * features, features, 8, blocks), seed=5).to(dev)
    net = pds.Matching(7, op)
    assert op.supports_native_training() == (features in (64, 16))
    net.set_disparity_shard(shard)
    begin, count = shard if shard else (0, 8)
    g = torch.Generator().manual_seed(6)
    left = torch.randn(2, features, 8, width, generator=g).to(dev).requires_grad_(True)
    right = torch.randn(2, features, 8, width, generator=g).to(dev).requires_grad_(True)
    weight = torch.randn(2, 8, count, 8, width, generator=g)
    out = net(left, right)
    assert out.shape == (2, 8, count, 8, width)
    with torch.no_grad():
        fused = net(left, right)          # inference route (factorised first layer, MFMA)
    assert helpers.maxdiff(out, fused) <= 2e-5
    (out * weight.to(dev)).sum().backward()
    params = helpers.prefixed(op.state_dict(), '_m._operation')

    def reference(p, a, b):
        full = oracle.matching(a, b, 7, lambda x: oracle.matching_operation(p, '_m._operation', x, blocks))
        return full[:, :, begin:begin + count]
    ref, (gl, gr), gp = oracle_grads(reference, [left, right], params, weight)
    assert relative_error(out, ref) <= 1e-4
    assert relative_error(left.grad, gl) <= REL_TOL
    assert relative_error(right.grad, gr) <= REL_TOL
    check_param_grads(op, '_m._operation', gp)


def test_regularization_backward(dev):
    reg = helpers.seeded(pds.Regularization, seed=7).to(dev)
    g = torch.Generator().manual_seed(8)
    ms = torch.randn(1, 8, 16, 32, 48, generator=g).to(dev).requires_grad_(True)
    shortcut = torch.randn(1, 8, 32, 48, generator=g).to(dev).requires_grad_(True)
    weight = torch.randn(1, 32, 128, 192, generator=g)
    cost = reg(ms, shortcut)
    (cost * weight.to(dev)).sum().backward()
    params = helpers.prefixed(reg.state_dict(), '_r')
    fn = lambda p, a, b: oracle.regularization(p, '_r', a, b)  # noqa: E731
    ref, (gms, gsc), gp = oracle_grads(fn, [ms, shortcut], params, weight)
    _, _, gp32 = oracle_grads(fn, [ms, shortcut], params, weight, dtype=torch.float32)
    assert relative_error(cost, ref) <= 1e-4
    assert relative_error(ms.grad, gms) <= REL_TOL
    assert relative_error(shortcut.grad, gsc) <= REL_TOL
    print('regularization worst parameter-gradient error', check_param_grads(reg, '_r', gp, gp32))


def test_network_training_step(dev):
    """config 5 in miniature: train-mode PdsNetwork -> cost volume -> a loss -> backward -> every parameter has a
    finite gradient, and an SGD step changes the loss."""
    net = helpers.seeded(lambda: pds.PdsNetwork.default(63)).to(dev).train()
    left, right = helpers.images(1, 128, 192)
    left, right = left.to(dev), right.to(dev)
    target = torch.randint(0, 32, (1, 128, 192), generator=torch.Generator().manual_seed(2)).to(dev)
    cost = net(left, right)
    assert cost.shape == (1, 32, 128, 192)
    loss = torch.nn.functional.cross_entropy(cost, target)
    loss.backward()
    for name, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    with torch.no_grad():
        for p in net.parameters():
            p -= 1e-3 * p.grad
    loss2 = torch.nn.functional.cross_entropy(net(left, right), target)
    assert float(loss2.detach()) < float(loss.detach())


def test_subpixel_cross_entropy_known_answer(dev):
    """reference test/test_loss.py:12-37: value 1.3654 and the gradient table, atol 1e-3."""
    g = helpers.golden('g8_loss')
    sim = g['ref_sim'].to(dev).requires_grad_(True)
    criterion = pds.SubpixelCrossEntropy(diversity=2.0, disparity_step=1)
    value = criterion(sim, g['ref_gt'].to(dev), g['ref_weights'].to(dev))
    value.backward()
    assert abs(value.item() - 1.3654) < 1e-3
    assert abs(value.item() - g['ref_value'].item()) < 1e-5
    assert helpers.maxdiff(sim.grad, g['ref_grad']) <= 1e-6


@pytest.mark.parametrize('weighted', [False, True])
def test_subpixel_cross_entropy_random(dev, weighted):
    g = helpers.golden('g8_loss')
    name = 'weighted' if weighted else 'plain'
    sim = g['random_sim'].to(dev).requires_grad_(True)
    w = g['random_weights'].to(dev) if weighted else None
    value = pds.SubpixelCrossEntropy()(sim, g['random_gt'].to(dev), w)
    (3.0 * value).backward()
    assert abs(value.item() - g['random_%s_value' % name].item()) < 1e-5
    assert helpers.maxdiff(sim.grad, 3.0 * g['random_%s_grad' % name]) <= 1e-6


def test_training_step_with_subpixel_cross_entropy(dev):
    """config 5 in miniature with the reference's criterion: PdsNetwork (train) -> SubpixelCrossEntropy -> backward,
    compared with the fp64 oracle for the loss value and the gradient reaching the cost volume."""
    net = helpers.seeded(lambda: pds.PdsNetwork.default(63)).to(dev).train()
    left, right = helpers.images(1, 128, 192)
    gt = torch.rand(1, 128, 192, generator=torch.Generator().manual_seed(5)) * 60
    gt[:, :8] = float('inf')
    cost = net(left.to(dev), right.to(dev))
    cost.retain_grad()
    loss = pds.SubpixelCrossEntropy()(cost, gt.to(dev))
    loss.backward()
    c64 = cost.detach().double().cpu().requires_grad_(True)
    ref = oracle.subpixel_cross_entropy(c64, gt.double())
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-4 * abs(ref.item())
    assert relative_error(cost.grad, c64.grad) <= 1e-4
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())


def test_network_image_gradients(dev):
    """network.py:38-52 under autograd down to the IMAGES (the reference's autograd reaches them through the first
    InstanceNorm2d, embedding.py:32): PdsNetwork (train) -> SubpixelCrossEntropy -> backward with both images requiring
    a gradient, against the fp64 oracle of the whole network.
    Tolerance (stated): the image gradient is a tiny, sign-cancelling quantity (largest entry ~1e-5) behind ~50 normalised
    layers.  The descriptor network alone, driven by identical upstream gradients, reproduces the fp64 image gradient to
    8e-7 of its largest entry (tools/diag_image_grad.py; tests/test_gpu_embedding.py holds it to 2e-3 with random upstream
    gradients and against the reference's own run, G12); end to end, the gradients ARRIVING at the descriptors differ
    from fp64 by ~1.5e-3 mean-relative (fp32 CPU oracle: 1.0e-3) and the image gradient by 1.2e-2 (left) / 2.0e-2
    (right) of the largest entry, mean error 1.7e-3 / 2.4e-3 of the mean magnitude.  Gates: 5e-2 / 1e-2, plus the
    finite-difference gates below, which are the tight ones."""
    net = helpers.seeded(lambda: pds.PdsNetwork.default(63)).to(dev).train()
    left, right = helpers.images(1, 100, 150)       # padded by 28 rows / 42 columns inside the network
    gt = torch.rand(1, 100, 150, generator=torch.Generator().manual_seed(6)) * 60
    gt[:, :8] = float('inf')
    left_dev, right_dev = left.to(dev).requires_grad_(True), right.to(dev).requires_grad_(True)
    loss = pds.SubpixelCrossEntropy()(net(left_dev, right_dev), gt.to(dev))
    loss.backward()
    params = {k: v.detach().cpu() for k, v in net.state_dict().items()}

    def run(dtype):
        l, r = left.clone().to(dtype).requires_grad_(True), right.clone().to(dtype).requires_grad_(True)
        cost = oracle.network_training_output(oracle.cast_params(params, dtype), l, r, 63)
        value = oracle.subpixel_cross_entropy(cost, gt.to(dtype))
        value.backward()
        return value.item(), l.grad, r.grad

    v64, gl64, gr64 = run(torch.float64)
    _, gl32, gr32 = run(torch.float32)
    assert abs(loss.item() - v64) <= 1e-4 * abs(v64)
    for name, got, want, theirs in (('left', left_dev.grad, gl64, gl32), ('right', right_dev.grad, gr64, gr32)):
        assert got is not None and got.shape == want.shape, name
        err, floor = relative_error(got, want), relative_error(theirs, want)
        mean_err = float((got.double().cpu() - want).abs().mean() / want.abs().mean())
        print('%s image gradient: error %.3g of the largest entry (fp32 CPU oracle %.3g), mean error %.3g of the mean '
              'magnitude' % (name, err, floor, mean_err))
        assert err <= 5e-2 and mean_err <= 1e-2, (name, err, mean_err, floor)
    # The gradient is the gradient of the HIP path's OWN loss: a central difference of that loss along the gradient
    # direction reproduces |g|^2 as far as the function is linear.  It hardly is: on the exact fp64 oracle the slope
    # is 0.965 |g|^2 when the largest pixel moves by +-0.02 grey levels and 0.36 |g|^2 at +-2 (random weights, ~50
    # normalised layers).  That curvature -- 3.5 % of the gradient per 0.02 grey levels -- is also what turns the
    # 1e-5 difference between two fp32 forward passes into the ~2e-3 mean gradient difference gated above.
    # Gates: the HIP slope equals the fp64 oracle's slope at the same steps, and approaches |g|^2 at the small one.
    gl, gr = left_dev.grad, right_dev.grad
    squared = float((gl.double() ** 2).sum() + (gr.double() ** 2).sum())
    peak = float(max(gl.abs().max(), gr.abs().max()))
    criterion = pds.SubpixelCrossEntropy()
    p64 = oracle.cast_params(params, torch.float64)

    def oracle_loss(l, r):
        return oracle.subpixel_cross_entropy(oracle.network_training_output(p64, l, r, 63), gt.double()).item()

    for move, slack in ((2.0, 0.01), (0.02, 0.05)):
        t = move / peak
        with torch.no_grad():
            up = criterion(net(left_dev + t * gl, right_dev + t * gr), gt.to(dev)).item()
            down = criterion(net(left_dev - t * gl, right_dev - t * gr), gt.to(dev)).item()
            dl, dr = (t * gl).double().cpu(), (t * gr).double().cpu()
            up64 = oracle_loss(left.double() + dl, right.double() + dr)
            down64 = oracle_loss(left.double() - dl, right.double() - dr)
        slope, slope64 = (up - down) / (2.0 * t), (up64 - down64) / (2.0 * t)
        print('largest pixel +-%.2f: finite-difference slope %.5g (fp64 oracle %.5g), |g|^2 %.5g'
              % (move, slope, slope64, squared))
        assert abs(slope - slope64) <= slack * squared, (move, slope, slope64, squared)
    assert 0.9 * squared <= slope <= 1.03 * squared, (slope, squared)


def test_standalone_blocks_backward(dev):
    """ContractionBlock3d / ExpansionBlock3d (regularization.py:11-57) with gradients, odd sizes and 6 features: channel
    counts that fill no 16-wide MFMA block.  The weight gradients still run on the matrix-pipe kernels -- none of the
    wgrad3d predicates looks at channel counts -- and the launch probe shows wgrad3d_s2_mfma<conv|deconv>,
    wgrad3d_mfma<tap> (12 -> 12) and wgrad3d_mfma<pair,2src> (3 -> 3) here (tests/test_gpu_wgrad_layers.py)."""
    g = torch.Generator().manual_seed(11)
    con = helpers.seeded(lambda: pds.ContractionBlock3d(6), seed=12).to(dev)
    x = torch.randn(2, 6, 10, 14, 16, generator=g).to(dev).requires_grad_(True)
    wd, wsm = torch.randn(2, 12, 5, 7, 8, generator=g), torch.randn(2, 12, 5, 7, 8, generator=g)
    down, smooth = con(x)
    ((down * wd.to(dev)).sum() + (smooth * wsm.to(dev)).sum()).backward()
    params = helpers.prefixed(con.state_dict(), '_c')
    x64 = x.detach().double().cpu().requires_grad_(True)
    p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
    d64, s64 = oracle.contraction_block_3d(p64, '_c', x64)
    ((d64 * wd.double()).sum() + (s64 * wsm.double()).sum()).backward()
    assert relative_error(x.grad, x64.grad) <= REL_TOL
    check_param_grads(con, '_c', {k: v.grad for k, v in p64.items()})

    exp = helpers.seeded(lambda: pds.ExpansionBlock3d(6), seed=13).to(dev)
    xi = torch.randn(2, 6, 5, 7, 8, generator=g).to(dev).requires_grad_(True)
    sc = torch.randn(2, 3, 10, 14, 16, generator=g).to(dev).requires_grad_(True)
    wo = torch.randn(2, 3, 10, 14, 16, generator=g)
    out = exp(xi, sc)
    (out * wo.to(dev)).sum().backward()
    params = helpers.prefixed(exp.state_dict(), '_e')
    ref, (gxi, gsc), gp = oracle_grads(lambda p, a, b: oracle.expansion_block_3d(p, '_e', a, b), [xi, sc], params, wo)
    assert relative_error(out, ref) <= 1e-4
    assert relative_error(xi.grad, gxi) <= REL_TOL and relative_error(sc.grad, gsc) <= REL_TOL
    check_param_grads(exp, '_e', gp)


def test_standalone_blocks_backward_eight_features_odd_sizes(dev):
    """The round-4 backward kernels behind 8-channel layers (tap pairs / tap groups in the MFMA columns of the 3-D weight
    gradients, column-pair data gradients with 8-channel blocks) on odd depths, heights and widths: the last plane, row
    and column pair are partial, and an odd plane / row has two contributing taps per axis in the strided convolution."""
    g = torch.Generator().manual_seed(21)
    con = helpers.seeded(lambda: pds.ContractionBlock3d(8), seed=22).to(dev)
    x = torch.randn(1, 8, 7, 9, 15, generator=g).to(dev).requires_grad_(True)
    wd, wsm = torch.randn(1, 16, 4, 5, 8, generator=g), torch.randn(1, 16, 4, 5, 8, generator=g)
    down, smooth = con(x)
    ((down * wd.to(dev)).sum() + (smooth * wsm.to(dev)).sum()).backward()
    params = helpers.prefixed(con.state_dict(), '_c')
    x64 = x.detach().double().cpu().requires_grad_(True)
    p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
    d64, s64 = oracle.contraction_block_3d(p64, '_c', x64)
    ((d64 * wd.double()).sum() + (s64 * wsm.double()).sum()).backward()
    assert relative_error(x.grad, x64.grad) <= REL_TOL
    check_param_grads(con, '_c', {k: v.grad for k, v in p64.items()})

    exp = helpers.seeded(lambda: pds.ExpansionBlock3d(8), seed=23).to(dev)
    xi = torch.randn(1, 8, 3, 5, 7, generator=g).to(dev).requires_grad_(True)
    sc = torch.randn(1, 4, 6, 10, 14, generator=g).to(dev).requires_grad_(True)
    wo = torch.randn(1, 4, 6, 10, 14, generator=g)
    out = exp(xi, sc)
    (out * wo.to(dev)).sum().backward()
    params = helpers.prefixed(exp.state_dict(), '_e')
    ref, (gxi, gsc), gp = oracle_grads(lambda p, a, b: oracle.expansion_block_3d(p, '_e', a, b), [xi, sc], params, wo)
    assert relative_error(out, ref) <= 1e-4
    assert relative_error(xi.grad, gxi) <= REL_TOL and relative_error(sc.grad, gsc) <= REL_TOL
    check_param_grads(exp, '_e', gp)

    # shapes the rolling stride-2 weight-gradient kernel takes (widths that are multiples of 4 on both grids; the switch
    # test runs this test with PDS_WGRAD3D_S2_ROLLING=2, which sends them there however small they are)
    for features, shape in ((8, (1, 8, 6, 10, 16)), (8, (2, 8, 5, 7, 8))):
        con = helpers.seeded(lambda: pds.ContractionBlock3d(features), seed=25).to(dev)
        x = torch.randn(*shape, generator=g).to(dev).requires_grad_(True)
        down, smooth = con(x)
        wd, wsm = torch.randn(*down.shape, generator=g), torch.randn(*smooth.shape, generator=g)
        ((down * wd.to(dev)).sum() + (smooth * wsm.to(dev)).sum()).backward()
        params = helpers.prefixed(con.state_dict(), '_c')
        x64 = x.detach().double().cpu().requires_grad_(True)
        p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
        d64, s64 = oracle.contraction_block_3d(p64, '_c', x64)
        ((d64 * wd.double()).sum() + (s64 * wsm.double()).sum()).backward()
        assert relative_error(x.grad, x64.grad) <= REL_TOL
        check_param_grads(con, '_c', {k: v.grad for k, v in p64.items()})
    for features, shape in ((8, (1, 8, 3, 5, 8)), (16, (2, 16, 3, 4, 8))):
        exp = helpers.seeded(lambda: pds.ExpansionBlock3d(features), seed=26).to(dev)
        xi = torch.randn(*shape, generator=g).to(dev).requires_grad_(True)
        big = (shape[0], features // 2, 2 * shape[2], 2 * shape[3], 2 * shape[4])
        sc = torch.randn(*big, generator=g).to(dev).requires_grad_(True)
        wo = torch.randn(*big, generator=g)
        out = exp(xi, sc)
        (out * wo.to(dev)).sum().backward()
        params = helpers.prefixed(exp.state_dict(), '_e')
        ref, (gxi, gsc), gp = oracle_grads(lambda p, a, b: oracle.expansion_block_3d(p, '_e', a, b), [xi, sc], params, wo)
        assert relative_error(out, ref) <= 1e-4
        assert relative_error(xi.grad, gxi) <= REL_TOL and relative_error(sc.grad, gsc) <= REL_TOL
        check_param_grads(exp, '_e', gp)

    # a 16 -> 8 expansion: the transposed layer's dz has 8 channels (two taps per column group in its weight gradient)
    exp = helpers.seeded(lambda: pds.ExpansionBlock3d(16), seed=24).to(dev)
    xi = torch.randn(2, 16, 3, 4, 9, generator=g).to(dev).requires_grad_(True)
    sc = torch.randn(2, 8, 6, 8, 18, generator=g).to(dev).requires_grad_(True)
    wo = torch.randn(2, 8, 6, 8, 18, generator=g)
    out = exp(xi, sc)
    (out * wo.to(dev)).sum().backward()
    params = helpers.prefixed(exp.state_dict(), '_e')
    ref, (gxi, gsc), gp = oracle_grads(lambda p, a, b: oracle.expansion_block_3d(p, '_e', a, b), [xi, sc], params, wo)
    assert relative_error(out, ref) <= 1e-4
    assert relative_error(xi.grad, gxi) <= REL_TOL and relative_error(sc.grad, gsc) <= REL_TOL
    check_param_grads(exp, '_e', gp)


def test_config5_full_size_training_step(dev):
    """BASELINE configs[4] on one GPU: the reference's training step (pds_trainer.py:35-46: train-mode network ->
    SubpixelCrossEntropy -> backward; RMSprop lr 1e-2, train_on_flyingthings3d.py:68) at the full 960x540, D=192 size.
    The loss must equal the oracle's (fp32 on the host), every parameter must receive a finite gradient, and two
    optimizer steps on the same pair must lower the loss."""
    torch.manual_seed(0)
    net = pds.PdsNetwork.default(191)
    left, right = helpers.images(1, 540, 960)
    g = torch.Generator().manual_seed(21)
    gt = torch.rand(1, 540, 960, generator=g) * 190.0
    gt[:, :, :40] = float('inf')          # unknown ground truth band (errors.py / loss.py mask it)
    params = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.to(dev).train()
    criterion = pds.SubpixelCrossEntropy()
    optimizer = torch.optim.RMSprop(net.parameters(), lr=1e-2)
    left_g, right_g, gt_g = left.to(dev), right.to(dev), gt.to(dev)

    def step():
        optimizer.zero_grad()
        cost = net(left_g, right_g)
        assert cost.shape == (1, 96, 540, 960)       # training mode returns the cropped cost volume (network.py:50-52)
        loss = criterion(cost, gt_g)
        loss.backward()
        return loss, cost

    loss0, cost0 = step()
    with torch.no_grad():
        ref_cost = oracle.network_training_output(params, left, right, 191)
        ref_loss = oracle.subpixel_cross_entropy(ref_cost, gt)
    print('config5 loss: gpu %.6f oracle %.6f' % (loss0.item(), ref_loss.item()))
    assert abs(loss0.item() - ref_loss.item()) <= 1e-4 * abs(ref_loss.item())
    assert helpers.maxdiff(cost0.detach(), ref_cost) <= 1e-4
    grads = [p.grad for p in net.parameters()]
    assert all(gr is not None and bool(torch.isfinite(gr).all()) for gr in grads)
    assert sum(float(gr.abs().sum()) for gr in grads) > 0.0
    del cost0
    optimizer.step()
    loss1, _ = step()
    optimizer.step()
    loss2, _ = step()
    print('config5 losses', loss0.item(), loss1.item(), loss2.item())
    assert loss2.item() < loss0.item()


def test_config5_gradients_against_reference_fp64_at_full_size(dev):
    """VERDICT r4 item 3 / fixture G13 (tests/golden/g13_config5_gradients.npz, written by make_golden.py from the
    REFERENCE's own fp32 and fp64 training steps at 960x540, D=192): EVERY parameter gradient of the GPU step (all 122
    tensors), element-wise on a strided sub-sample of at most 512 entries per tensor, against the fp64 gradient, relative
    to the tensor's largest entry:
      * every entry within max(5e-3, 3 x the reference's own fp32-vs-fp64 distance) -- EXCEPT at most one entry per tensor,
        which may reach 5e-2: a LeakyReLU whose argument is within rounding of zero takes the other slope in one of two
        fp32 forward passes, and that single activation moves ONE channel's bias / weight-slice gradient by ~1/sqrt(N) of
        its size (the backward counterpart of the arg-max flips of the forward tests; measured: one channel of one bias
        vector, 2.5e-2, identical under every alternative kernel);
      * the rms error within max(2e-3, 3 x the reference's own rms error);
      * the norm within the first gate.
    The 64-channel weight gradients sum 1.6 M sign-cancelling terms per entry here -- where a 22-bit product (wgrad2d_x3:
    fp16-split operands) would drift if it did."""
    import numpy as np
    with np.load(os.path.join(helpers.GOLDEN, 'g13_config5_gradients.npz')) as z:
        g = {k: np.array(z[k]) for k in z.files}
    torch.manual_seed(0)
    net = pds.PdsNetwork.default(191)
    assert abs(helpers.checksum(net.state_dict()) - float(g['weight_checksum'])) < 1e-9
    names = [n for n, _ in net.named_parameters()]
    assert names == [str(n) for n in g['parameter_names']]
    left, right = helpers.images(1, 540, 960)
    gen = torch.Generator().manual_seed(int(g['ground_truth_seed'][0]))
    gt = torch.rand(1, 540, 960, generator=gen) * 190.0
    gt[:, :17] = float('inf')
    net = net.to(dev).train()
    cost = net(left.to(dev), right.to(dev))
    loss = pds.SubpixelCrossEntropy()(cost, gt.to(dev))
    loss.backward()
    assert abs(loss.item() - float(g['loss_fp64'][0])) <= 2e-5 * abs(float(g['loss_fp64'][0])), loss.item()
    assert helpers.maxdiff(cost.detach()[:, ::8, ::36, ::64], torch.from_numpy(g['cost_sub_fp64']).float()) <= 1e-4
    del cost
    offsets = g['grad_sub_offsets']
    rows, failed, flips = [], [], 0
    for i, (name, p) in enumerate(net.named_parameters()):
        flat = p.grad.detach().flatten()
        sub = flat[::max(1, -(-flat.numel() // 512))].double().cpu().numpy()
        want = g['grad_sub_fp64'][offsets[i]:offsets[i + 1]]
        ref32 = g['grad_sub'][offsets[i]:offsets[i + 1]].astype(np.float64)
        assert sub.shape == want.shape, name
        scale = float(g['grad_abs_max_fp64'][i])
        if not bool(g['live'][i]):     # a gradient that is zero in exact arithmetic (the bias in front of the soft-max)
            assert float(np.abs(sub).max()) <= 1e-6, name
            continue
        err = np.sort(np.abs(sub - want) / scale)[::-1]
        ref_err = np.abs(ref32 - want) / scale
        gate_max = max(5e-3, 3.0 * float(g['grad_reference_vs_fp64_rel'][i]))
        gate_rms = max(2e-3, 3.0 * float(np.sqrt(np.mean(ref_err ** 2))))
        rms = float(np.sqrt(np.mean(err ** 2)))
        nerr = abs(float(p.grad.double().norm()) - float(g['grad_norms_fp64'][i])) / float(g['grad_norms_fp64'][i])
        second = float(err[1]) if err.size > 1 else 0.0
        flipped = float(err[0]) > gate_max
        flips += int(flipped)
        ok = (second if flipped else float(err[0])) <= gate_max and float(err[0]) <= 5e-2 and rms <= gate_rms and nerr <= gate_max
        rows.append((float(err[0]) / gate_max, float(err[0]), gate_max, rms, gate_rms, nerr, name))
        if not ok:
            failed.append(rows[-1])
    rows.sort(reverse=True)
    print('config5 full-size gradients vs the reference\'s fp64 run: %d tensors, %d with one entry beyond the element gate; '
          'worst (max error / gate, max error, gate, rms, rms gate, norm error):' % (len(rows), flips))
    for r in rows[:6]:
        print('   x%.2f  %.2e (%.2e)  rms %.2e (%.2e)  norm %.2e  %s' % r)
    own = sorted(r[1] / max(float(g['grad_reference_vs_fp64_rel'][names.index(r[6])]), 1e-30) for r in rows)
    print('GPU error / reference-fp32 error per tensor (both against fp64): median %.2f, 90 %% %.2f, max %.2f; the GPU is '
          'closer to fp64 than the reference\'s fp32 run on %d of %d tensors' %
          (own[len(own) // 2], own[int(len(own) * 0.9)], own[-1], sum(1 for r in own if r < 1.0), len(own)))
    assert not failed, failed
    assert flips <= 3, flips


def test_training_step_against_reference_fixture(dev):
    """SURVEY.md 8c fixture G9 (tests/golden/g11_training_step.npz, written by make_golden.py from the REFERENCE):
    one training step of train-mode PdsNetwork.default(63) on the 128x256 pair with SubpixelCrossEntropy -- loss,
    dL/dcost, and the gradient norm of every parameter tensor.  Weight gradients sum sign-cancelling terms, so the gate
    per tensor is the distance of its NORM to the reference's fp64 run: within 1e-2 (the reference's own fp32 run is up to
    1.5e-2 of a tensor's largest entry away from its fp64 run element-wise, pinning_report.json), or three times the
    reference's own fp32 distance where that is larger."""
    g = helpers.golden('g11_training_step')
    names = [str(n) for n in np.load(os.path.join(helpers.GOLDEN, 'g11_training_step.npz'))['parameter_names']]
    net = helpers.seeded(lambda: pds.PdsNetwork.default(63))
    assert abs(helpers.checksum(net.state_dict()) - g['weight_checksum'].item()) < 1e-9
    net = net.to(dev).train()
    left, right = helpers.images(1, 128, 256)
    cost = net(left.to(dev), right.to(dev))
    cost.retain_grad()
    loss = pds.SubpixelCrossEntropy()(cost, g['ground_truth'].to(dev))
    loss.backward()
    assert abs(loss.item() - g['loss'].item()) <= 1e-5 * abs(g['loss'].item())
    assert helpers.maxdiff(cost.detach()[:, ::4, ::8, ::8], g['cost_sub']) <= 1e-4
    scale = float(g['dcost_sub'].abs().max())
    assert helpers.maxdiff(cost.grad[:, ::4, ::8, ::8], g['dcost_sub']) <= 1e-3 * scale
    assert [n for n, _ in net.named_parameters()] == names
    norms32, norms64 = g['grad_norms'].double(), g['grad_norms_fp64'].double()
    worst, failures = 0.0, []
    for i, (name, p) in enumerate(net.named_parameters()):
        if norms64[i] < 1e-9:      # true zero gradient (the bias in front of the soft-max): rounding noise only
            assert float(p.grad.double().norm()) <= 1e-5, name
            continue
        mine = abs(float(p.grad.double().norm()) - float(norms64[i])) / float(norms64[i])
        theirs = abs(float(norms32[i]) - float(norms64[i])) / float(norms64[i])
        worst = max(worst, mine)
        if mine > max(1e-2, 3.0 * theirs):
            failures.append((name, mine, theirs))
    assert not failures, failures
    print('training step vs reference fixture: loss %.6f, worst gradient-norm error vs fp64 %.2e' % (loss.item(), worst))
    # element-wise: a strided sub-sample of every gradient tensor against the reference's fp64 run, for every
    # tensor the reference's OWN fp32 run reproduces to better than 1e-3 of its largest entry.  These gradients pass
    # through every InstanceNorm backward (sign-cancelling sums), so an fp32 evaluation in another summation order lands
    # a few 1e-3 of the largest entry away: measured worst 4.2e-3 with the round-3 kernels (tools/g11_probe.py; the
    # round-2 Winograd data-gradient path was at 6.9e-2).  Bar per tensor: 5e-3, or three times the reference's own
    # fp32 distance on that sub-sample where that is larger.
    offsets = [int(v) for v in g['grad_sub_offsets']]
    checked, worst_elem, bad = 0, 0.0, []
    for i, (name, p) in enumerate(net.named_parameters()):
        if norms64[i] < 1e-9 or float(g['grad_reference_vs_fp64_rel'][i]) >= 1e-3:
            continue
        flat = p.grad.detach().flatten()
        mine = flat[::max(1, -(-flat.numel() // 512))].double().cpu()
        want64 = g['grad_sub_fp64'][offsets[i]:offsets[i + 1]].double()
        want32 = g['grad_sub'][offsets[i]:offsets[i + 1]].double()
        assert mine.numel() == want64.numel(), name
        top = float(want64.abs().max()) + 1e-30
        err = float((mine - want64).abs().max()) / top
        theirs = float((want32 - want64).abs().max()) / top
        checked += 1
        worst_elem = max(worst_elem, err)
        if err > max(5e-3, 3.0 * theirs):
            bad.append((name, err, theirs))
    assert checked >= 15, checked     # 21 of the 122 tensors qualify (weight gradients sum sign-cancelling terms)
    assert not bad, bad
    print('element-wise: %d tensors, worst error vs fp64 relative to the largest entry %.2e' % (checked, worst_elem))


def test_unsupported_autograd_uses_fail_loudly(dev):
    """A second backward through a node is refused with a message instead of crashing or silently returning
    nothing."""
    op = helpers.seeded(pds.MatchingOperation, seed=3).to(dev)
    x = torch.randn(1, 128, 8, 12, generator=torch.Generator().manual_seed(0)).to(dev).requires_grad_(True)
    out = op(x).sum()
    out.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='second time'):
        out.backward()


def test_subpixel_cross_entropy_weight_gradient(dev):
    """loss.py:73-77 under autograd: the gradient reaching ``weights`` -- the reference's own known-answer case and the
    seeded random case of G8 (reference autograd), then a larger case against the fp64 oracle."""
    g = helpers.golden('g8_loss')
    sim = g['ref_sim'].to(dev).requires_grad_(True)
    w = g['ref_weights'].to(dev).requires_grad_(True)
    pds.SubpixelCrossEntropy(diversity=2.0, disparity_step=1)(sim, g['ref_gt'].to(dev), w).backward()
    assert helpers.maxdiff(w.grad, g['ref_weights_grad']) <= 1e-6
    assert helpers.maxdiff(sim.grad, g['ref_grad']) <= 1e-6
    sim = g['random_sim'].to(dev).requires_grad_(True)
    w = g['random_weights'].to(dev).requires_grad_(True)
    (3.0 * pds.SubpixelCrossEntropy()(sim, g['random_gt'].to(dev), w)).backward()
    assert helpers.maxdiff(w.grad, 3.0 * g['random_weighted_weights_grad']) <= 1e-6
    assert helpers.maxdiff(sim.grad, 3.0 * g['random_weighted_grad']) <= 1e-6
    assert float(w.grad[:, 2:4].abs().max()) == 0.0      # unknown ground truth: no gradient
    gen = torch.Generator().manual_seed(5)
    sim = torch.randn(2, 24, 33, 47, generator=gen)
    gt = torch.rand(2, 33, 47, generator=gen) * 46
    gt[0, :5] = float('inf')
    weights = torch.rand(2, 33, 47, generator=gen) + 0.1
    w64 = weights.double().requires_grad_(True)
    oracle.subpixel_cross_entropy(sim.double(), gt.double(), w64).backward()
    wd = weights.to(dev).requires_grad_(True)
    pds.SubpixelCrossEntropy()(sim.to(dev), gt.to(dev), wd).backward()
    assert helpers.maxdiff(wd.grad, w64.grad.float()) <= 1e-7 + 1e-5 * float(w64.grad.abs().max())


def test_eval_mode_with_gradients_warns_once(dev):
    import warnings
    from practicaldeepstereo_nips2018_amd import _lib
    _lib._warned_eval_with_grad.discard('Embedding')
    emb = helpers.seeded(pds.Embedding, seed=1).to(dev).eval()
    image = (torch.rand(1, 3, 32, 48) * 255).to(dev)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        emb(image)
        emb(image)
    assert sum('torch.no_grad' in str(w.message) for w in caught) == 1
    with warnings.catch_warnings(record=True) as caught, torch.no_grad():
        warnings.simplefilter('always')
        emb(image)
    assert not caught
