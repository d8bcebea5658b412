"""GPU (-m gpu): the speckle filter (speckle_filter, region_sizes, StereoRig.reconstruct(speckle_size=...);
pds_speckle_filter_fwd).

Sizes, masks and labels are integers: everything is compared exactly (torch.equal / numpy array_equal), there is no
tolerance in this feature.  The arbiter is the numpy hook-and-jump union-find of tests/test_speckle_host.py, which is
itself held to hand-written answers there.  The kernel labels tiles of TILE_W x TILE_H = 64 x 32 pixels (csrc/speckle.hip:
kTileW, kTileH) and joins them across their seams, so the shapes below sit around multiples of the tile and the patterns
are chosen to break a tiled union-find: paths that cross every seam many times, labels that must travel the whole image,
as many roots as there are pixels, one root for everything.
"""
import time

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from tests import helpers
from tests.test_speckle_host import BLOBS, JUST_ABOVE_ONE, KNOWN, oracle_filter, oracle_sizes

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 64, 32
NAN = float('nan')


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def bits(t):
    return t.contiguous().view(torch.int32)


def gpu_sizes(dev, d, max_difference=1.0, valid=None):
    """region_sizes of one numpy image [H, W] -> numpy int32 [H, W]."""
    v = None if valid is None else torch.from_numpy(np.ascontiguousarray(valid)).to(dev)[None]
    out = pds.region_sizes(torch.from_numpy(np.ascontiguousarray(d)).to(dev)[None], max_difference, valid=v)
    assert out.dtype == torch.int32 and out.shape == (1,) + d.shape
    return out[0].cpu().numpy()


# ------------------------------------------------------------------------------------------------ patterns
def serpentine(height, width):
    """One path, one pixel wide, along every second row and down alternate ends; the rows between are other regions."""
    d = np.full((height, width), 100.0, dtype=np.float32)
    d[0::2] = 5.0
    d[1::4, -1] = 5.0
    d[3::4, 0] = 5.0
    return d


def spiral(height, width):
    """A one-pixel path winding inwards with a one-pixel gap, which is a second spiral."""
    d = np.full((height, width), 100.0, dtype=np.float32)
    y, x, dy, dx = 0, 0, 0, 1
    d[0, 0] = 5.0

    def free(v, u):
        return not (0 <= v < height and 0 <= u < width) or d[v, u] != 5.0

    while True:
        for _ in range(2):   # straight on, else one turn to the right
            if 0 <= y + dy < height and 0 <= x + dx < width and free(y + dy, x + dx) and free(y + 2 * dy, x + 2 * dx):
                break
            dy, dx = dx, -dy
        else:
            return d
        y, x = y + dy, x + dx
        d[y, x] = 5.0


def comb(height, width):
    """Teeth on every second column that join only in the last row: labels must travel up the whole image."""
    d = np.full((height, width), 100.0, dtype=np.float32)
    d[:, 0::2] = 5.0
    d[-1] = 5.0
    return d


def checkerboard(height, width):
    yy, xx = np.mgrid[0:height, 0:width]
    return np.where((yy + xx) % 2 == 0, 0.0, 50.0).astype(np.float32)


def constant(height, width):
    return np.full((height, width), 7.25, dtype=np.float32)


def noise(height, width, seed=0):
    return (np.random.RandomState(seed).rand(height, width) * 16).astype(np.float32)


def plane_scene(height, width, seed=0, speckles=0.02):
    """A slanted plane with a step edge, 2 % single-pixel outliers, a few small blobs and non-finite holes."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float32)
    d = (20.0 + 0.05 * xx + 0.02 * yy).astype(np.float32)
    d[:, width // 2:] += 30.0
    outliers = rng.rand(height, width) < speckles
    d[outliers] += (rng.rand(int(outliers.sum())) * 60 + 5).astype(np.float32)
    for _ in range(max(1, height * width // 4000)):
        y, x = rng.randint(0, height), rng.randint(0, width)
        d[y:y + rng.randint(1, 5), x:x + rng.randint(1, 7)] = 150.0 + rng.rand() * 50
    for _ in range(max(1, height * width // 20000)):
        y, x = rng.randint(0, height), rng.randint(0, width)
        d[y:y + rng.randint(1, 20), x:x + rng.randint(1, 30)] = rng.choice([np.nan, np.inf, -np.inf])
    d[rng.rand(height, width) < 0.005] = np.nan
    return d


PATTERNS = {
    'serpentine': (serpentine, 1.0), 'spiral': (spiral, 1.0), 'comb': (comb, 1.0), 'checkerboard': (checkerboard, 1.0),
    'constant': (constant, 1.0), 'noise 1': (noise, 1.0), 'noise 8': (noise, 8.0), 'plane scene': (plane_scene, 1.0),
}
# one more and one less than the tile in either direction, degenerate images, the benchmark sizes (1242: the scalar store
# form, w % 4 != 0) and a large image
SHAPES = [(1, 1), (1, 300), (300, 1), (7, 5), (63, 65), (TILE_H, TILE_W), (64, 64), (TILE_H + 1, TILE_W + 1), (65, 129),
          (540, 960), (375, 1242), (1080, 1920)]


# ------------------------------------------------------------------------------------------------ known answers
def test_known_answers(dev):
    for name, (d, valid, md, expected) in KNOWN.items():
        d = np.array(d, dtype=np.float32)
        valid = None if valid is None else np.array(valid, dtype=np.uint8)
        got = gpu_sizes(dev, d, md, valid)
        assert np.array_equal(got, np.array(expected)), (name, got)
        if valid is not None:   # torch.bool as well as uint8
            assert np.array_equal(gpu_sizes(dev, d, md, valid != 0), np.array(expected)), name


def test_known_answer_thresholds_and_fill_values(dev):
    d = torch.tensor(BLOBS[0], dtype=torch.float32, device=dev)[None]
    sizes = torch.tensor(BLOBS[1], dtype=torch.int32, device=dev)[None]
    assert torch.equal(pds.region_sizes(d), sizes)
    for max_size, kept in ((0, 48), (2, 48), (3, 45), (4, 41), (40, 41), (41, 0), (1000, 0)):   # size == max_size goes
        for fill in (NAN, 0.0, -1.0):
            out = pds.speckle_filter(d, max_size, fill_value=fill)
            assert isinstance(out, pds.SpeckleFiltered) and out.keep.dtype == torch.bool
            assert out.disparity.dtype == torch.float32 and out.disparity.shape == d.shape == out.keep.shape
            assert int(out.keep.sum()) == kept, (max_size, fill)
            assert torch.equal(out.keep, sizes > max_size)
            expected = torch.where(sizes > max_size, d, torch.full_like(d, fill))
            assert torch.equal(bits(out.disparity), bits(expected)), (max_size, fill)
    assert torch.isnan(pds.speckle_filter(d, 3).disparity[0, 1, 1]).item()   # the default fill is NaN


def test_the_link_threshold_is_inclusive_in_fp32(dev):
    for other, linked in ((1.0, True), (JUST_ABOVE_ONE, False), (-1.0, True), (-JUST_ABOVE_ONE, False)):
        for d in (torch.tensor([[[0.0, other]]]), torch.tensor([[[0.0], [other]]])):   # across and down
            sizes = pds.region_sizes(d.to(dev), 1.0)
            assert sizes.flatten().tolist() == ([2, 2] if linked else [1, 1]), (other, d.shape)
    ramp = (torch.arange(960, dtype=torch.float32) * 0.9)[None, None].to(dev)   # 863 from end to end, one region
    assert torch.equal(pds.region_sizes(ramp), torch.full((1, 1, 960), 960, dtype=torch.int32, device=dev))
    assert torch.equal(pds.region_sizes(ramp.transpose(1, 2).contiguous()),
                       torch.full((1, 960, 1), 960, dtype=torch.int32, device=dev))
    steep = ramp * 1.2   # 1.08 per pixel: nothing is linked
    assert torch.equal(pds.region_sizes(steep), torch.ones((1, 1, 960), dtype=torch.int32, device=dev))


def test_not_eligible_pixels(dev):
    d = torch.full((1, 40, 70), 3.0, device=dev)
    d[0, :, 33] = NAN            # a wall next to a tile seam
    d[0, 20, :] = float('inf')   # and one across
    d[0, 5, 5] = float('-inf')
    valid = torch.ones((1, 40, 70), dtype=torch.bool, device=dev)
    valid[0, 30, 40:] = False
    out = pds.speckle_filter(d, 0, valid=valid)
    sizes = pds.region_sizes(d, valid=valid)
    eligible = torch.isfinite(d) & valid
    assert torch.equal(out.keep, eligible)            # max_size = 0 keeps every eligible pixel
    assert torch.equal(sizes == 0, ~eligible)
    assert torch.isnan(out.disparity[~eligible]).all() and torch.equal(out.disparity[eligible], d[eligible])
    expected = oracle_sizes(d[0].cpu().numpy(), valid[0].cpu().numpy())
    assert np.array_equal(sizes[0].cpu().numpy(), expected)
    # four quadrants: the one with the -inf pixel, two whole ones, and one whose masked row leaves a bridge of 6 pixels
    assert sorted(set(expected.flatten().tolist())) == sorted([0, 20 * 33 - 1, 20 * 36, 19 * 33, 19 * 36 - 30])
    # uint8 masks: any non-zero byte is "valid"
    assert torch.equal(pds.region_sizes(d, valid=valid.to(torch.uint8) * 7), sizes)


# ------------------------------------------------------------------------------------------------ against the oracle
def cases_for(shape):
    height, width = shape
    names = ['noise 1', 'noise 8', 'plane scene', 'constant', 'checkerboard', 'serpentine', 'comb', 'spiral']
    if height * width > 1000 * 1000:
        names = ['noise 1', 'noise 8', 'serpentine', 'plane scene']   # (the oracle takes seconds per image here)
    return names


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_region_sizes_against_the_oracle(dev, shape):
    height, width = shape
    for name in cases_for(shape):
        make, md = PATTERNS[name]
        d = make(height, width)
        t0 = time.time()
        expected = oracle_sizes(d, None, md)
        t1 = time.time()
        got = gpu_sizes(dev, d, md)
        wrong = int((got != expected).sum())
        print('%-12s %4dx%-4d largest region %8d, regions of one pixel %7d, oracle %.2f s, wrong %d' %
              (name, height, width, int(expected.max()), int((expected == 1).sum()), t1 - t0, wrong))
        assert wrong == 0, (name, shape, np.argwhere(got != expected)[:5].tolist())
        if name == 'serpentine' and shape == (540, 960):
            # one region, across every seam many times (the last row's connector dangles)
            assert int(expected.max()) == int((d == 5.0).sum()) == 270 * 960 + 270 >= 250000
        if name == 'checkerboard':
            assert int(expected.max()) == 1
        if name == 'constant':
            assert int(expected.min()) == height * width


def test_valid_mask_against_the_oracle(dev):
    rng = np.random.RandomState(11)
    for shape in ((65, 129), (375, 1242)):
        d = plane_scene(*shape, seed=3)
        valid = rng.rand(*shape) > 0.15
        expected = oracle_sizes(d, valid, 1.0)
        assert np.array_equal(gpu_sizes(dev, d, 1.0, valid), expected), shape
        assert np.array_equal(gpu_sizes(dev, d, 1.0, valid.astype(np.uint8) * 200), expected), shape


@pytest.mark.parametrize('shape', [(65, 129), (375, 1242), (270, 480)], ids=lambda s: '%dx%d' % s)
def test_images_of_a_batch_are_independent(dev, shape):
    images = [noise(*shape, seed=1), serpentine(*shape), plane_scene(*shape, seed=2), comb(*shape)]
    singles = [pds.region_sizes(torch.from_numpy(im).to(dev)[None], 1.0) for im in images]
    for im, single in zip(images, singles):
        assert np.array_equal(single[0].cpu().numpy(), oracle_sizes(im, None, 1.0))
    for batch in (2, 4):
        stacked = torch.from_numpy(np.stack(images[:batch])).to(dev)
        got = pds.region_sizes(stacked, 1.0)
        assert got.shape == (batch,) + shape
        for k in range(batch):
            assert torch.equal(got[k], singles[k][0]), (batch, k)
        out = pds.speckle_filter(stacked, 6)
        assert torch.equal(out.keep, got > 6)


def test_non_contiguous_and_wrong_inputs(dev):
    d = torch.from_numpy(noise(129, 65, seed=4)).to(dev)[None]
    view = d.transpose(1, 2)   # [1, 65, 129], not contiguous
    assert not view.is_contiguous()
    expected = oracle_sizes(d[0].cpu().numpy().T, None, 2.0)
    assert np.array_equal(pds.region_sizes(view, 2.0)[0].cpu().numpy(), expected)
    valid = (torch.from_numpy(noise(129, 65, seed=5)).to(dev)[None] > 3).transpose(1, 2)
    expected = oracle_sizes(d[0].cpu().numpy().T, valid[0].cpu().numpy(), 2.0)
    assert np.array_equal(pds.region_sizes(view, 2.0, valid=valid)[0].cpu().numpy(), expected)
    sliced = torch.from_numpy(noise(70, 140, seed=6)).to(dev)[None][:, 3:68, 5:134]   # rows with a stride
    assert np.array_equal(pds.region_sizes(sliced)[0].cpu().numpy(), oracle_sizes(sliced[0].cpu().numpy()))
    with pytest.raises(TypeError, match='float32'):
        pds.region_sizes(d.double())
    with pytest.raises(ValueError, match='empty input'):
        pds.speckle_filter(torch.zeros(0, 4, 5, device=dev), 3)
    with pytest.raises(ValueError, match='empty input'):
        pds.region_sizes(torch.zeros(1, 0, 5, device=dev))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pds.region_sizes(d, valid=torch.ones(1, 129, 65, dtype=torch.bool))


@pytest.mark.parametrize('shape', [(65, 129), (540, 960), (375, 1242)], ids=lambda s: '%dx%d' % s)
def test_speckle_filter_is_the_threshold_of_region_sizes(dev, shape):
    d = torch.from_numpy(np.stack([plane_scene(*shape, seed=7), noise(*shape, seed=8)])).to(dev)
    sizes = pds.region_sizes(d, 1.0)
    for max_size in (0, 1, 2, 10, 200, 10 ** 6):
        for fill in (NAN, 0.0, -1.0):
            out = pds.speckle_filter(d, max_size, fill_value=fill)
            keep = sizes > max_size
            assert torch.equal(out.keep, keep), (max_size, fill)
            assert torch.equal(bits(out.disparity), bits(torch.where(keep, d, torch.full_like(d, fill)))), (max_size, fill)
    # against the oracle end to end, NaN pattern included
    filtered, keep = oracle_filter(d[0].cpu().numpy(), 10, fill_value=NAN)
    out = pds.speckle_filter(d[:1], 10)
    assert np.array_equal(out.keep[0].cpu().numpy(), keep)
    assert np.array_equal(out.disparity[0].cpu().numpy().view(np.int32), filtered.view(np.int32))


def test_run_twice_same_bytes_and_on_a_side_stream(dev):
    """The atomics may land in any order; the outputs may not depend on it.  (A plain repeat of a passing call.)"""
    for name in ('noise 8', 'serpentine'):
        make, md = PATTERNS[name]
        d = torch.from_numpy(make(540, 960)).to(dev)[None]
        first, second = pds.region_sizes(d, md), pds.region_sizes(d, md)
        assert torch.equal(first, second), name
        a, b = pds.speckle_filter(d, 50, md), pds.speckle_filter(d, 50, md)
        assert torch.equal(a.keep, b.keep) and torch.equal(bits(a.disparity), bits(b.disparity)), name
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            other = pds.region_sizes(d, md)
            total = other.sum(dtype=torch.int64)   # consumed on that stream
        stream.synchronize()
        assert torch.equal(other, first) and int(total) == int(first.sum(dtype=torch.int64)), name
        torch.cuda.current_stream(dev).wait_stream(stream)


def test_in_place_gives_the_same_result(dev):
    """The alias contract of include/pds_hip.h: `filtered` may be `disparity` itself."""
    import ctypes
    from practicaldeepstereo_nips2018_amd import _lib
    lib = _lib.load()
    for shape in ((65, 129), (375, 1242), (540, 960)):
        d = torch.from_numpy(plane_scene(*shape, seed=9)).to(dev)[None]
        out = pds.speckle_filter(d, 20, fill_value=-3.0)
        buffer = d.clone()
        keep = torch.empty(d.shape, dtype=torch.bool, device=dev)
        nbytes = lib.pds_speckle_filter_workspace_bytes(1, *shape)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.pds_speckle_filter_fwd(_lib.ptr(buffer), None, _lib.ptr(keep), _lib.ptr(buffer), None, 1, *shape,
                                              1.0, 20, -3.0, _lib.ptr(ws), nbytes, _lib.stream_handle(dev)),
                   'pds_speckle_filter_fwd')
        torch.cuda.synchronize()
        assert torch.equal(keep, out.keep) and torch.equal(bits(buffer), bits(out.disparity)), shape
        # a shifted overlap is refused
        shifted = ctypes.c_void_p(buffer.data_ptr() + 16)
        assert lib.pds_speckle_filter_fwd(_lib.ptr(buffer), None, _lib.ptr(keep), shifted, None, 1, *shape, 1.0, 20,
                                          -3.0, _lib.ptr(ws), nbytes, _lib.stream_handle(dev)) != 0
        assert b'filtered overlaps disparity' in lib.pds_last_error()


# ------------------------------------------------------------------------------------------------ integration
def simple_rig(width, height):
    K = np.array([[0.7 * width, 0.0, 0.5 * width - 0.5], [0.0, 0.7 * width, 0.5 * height - 0.5], [0.0, 0.0, 1.0]])
    return pds.StereoRig(K, np.array([-0.05, 0.01, 1e-3, -5e-4]), K, np.array([-0.04, 0.02, -4e-4, 6e-4]), np.eye(3),
                         np.array([-0.12, 0.0, 0.0]), (width, height))


def same(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def test_reconstruct_with_the_speckle_filter_equals_the_steps_by_hand(dev):
    torch.manual_seed(0)
    net = pds.PdsNetwork.default(63).eval().to(dev)
    rig = simple_rig(256, 128)
    g = torch.Generator().manual_seed(3)
    left = torch.randint(0, 256, (1, 128, 256, 3), generator=g, dtype=torch.uint8).to(dev)
    right = torch.randint(0, 256, (1, 128, 256, 3), generator=g, dtype=torch.uint8).to(dev)
    with torch.no_grad():
        l, r = rig.rectify(left, right)
        checked = net.forward_left_right(l, r, max_difference=1.0)
        plain = net(l, r)

    # (random weights: the check leaves scattered pixels, so small sizes are where the filter decides anything)
    for size, difference in ((0, 1.0), (1, 2.0), (2, 8.0), (5, 1.0)):
        out = rig.reconstruct(net, left, right, max_difference=1.0, speckle_size=size, speckle_difference=difference)
        filtered = pds.speckle_filter(checked.left, size, max_difference=difference, valid=checked.left_valid)
        points = rig.reproject(checked.left, valid=filtered.keep)
        assert torch.equal(out.left_image, l) and torch.equal(out.right_image, r)
        assert torch.equal(out.disparity, checked.left)   # the network's map, unfiltered
        assert out.valid.dtype == torch.bool and torch.equal(out.valid, filtered.keep)
        assert same(out.points, points) and torch.isnan(out.points[~out.valid]).all()
        assert not (filtered.keep & ~checked.left_valid).any()
        if size == 0:
            assert torch.equal(filtered.keep, checked.left_valid & torch.isfinite(checked.left))
        print('reconstruct: check keeps %d of %d pixels, speckle filter (size %d, difference %g) keeps %d' %
              (int(checked.left_valid.sum()), checked.left_valid.numel(), size, difference, int(filtered.keep.sum())))

    # without the check the filter sees every finite pixel
    out = rig.reconstruct(net, left, right, speckle_size=5)
    filtered = pds.speckle_filter(plain, 5)
    assert torch.equal(out.disparity, plain) and torch.equal(out.valid, filtered.keep)
    assert same(out.points, rig.reproject(plain, valid=filtered.keep))

    # the defaults are those of the parent commit
    out = rig.reconstruct(net, left, right)
    assert out.valid is None and torch.equal(out.disparity, plain) and same(out.points, rig.reproject(plain))
    out = rig.reconstruct(net, left, right, max_difference=1.0)
    assert torch.equal(out.valid, checked.left_valid)
    assert same(out.points, rig.reproject(checked.left, valid=checked.left_valid))


def test_network_disparity_against_the_oracle(dev):
    """The scene of test_gpu_left_right.py::test_forward_left_right (random weights: the count removed means nothing and
    is only reported); the filter must agree exactly with the oracle run on the downloaded disparity."""
    net = helpers.seeded(lambda: pds.PdsNetwork.default(63)).eval().to(dev)
    left, right = [x.to(dev) for x in helpers.images(2, 93, 157)]
    with torch.no_grad():
        out = net.forward_left_right(left, right, max_difference=1.0)
    for max_size, difference, masked in ((1, 1.0, True), (4, 1.0, True), (25, 2.0, True), (10, 1.0, False),
                                         (100, 2.0, False)):
        mask = out.left_valid if masked else None
        got = pds.speckle_filter(out.left, max_size, max_difference=difference, valid=mask)
        sizes = pds.region_sizes(out.left, difference, valid=mask)
        for k in range(2):
            d = out.left[k].cpu().numpy()
            valid = out.left_valid[k].cpu().numpy() if masked else np.ones(d.shape, dtype=bool)
            filtered, keep = oracle_filter(d, max_size, valid, difference)
            assert np.array_equal(sizes[k].cpu().numpy(), oracle_sizes(d, valid, difference))
            assert np.array_equal(got.keep[k].cpu().numpy(), keep)
            assert np.array_equal(got.disparity[k].cpu().numpy().view(np.int32), filtered.view(np.int32))
            print('image %d: %s %d of %d pixels; the filter (size %d, difference %g) removes %d of them' %
                  (k, 'the check keeps' if masked else 'without the check,', int(valid.sum()), valid.size, max_size,
                   difference, int(valid.sum()) - int(keep.sum())))
