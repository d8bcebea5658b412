"""GPU (-m gpu): TSDF fusion (TsdfVolume.integrate, TsdfVolume.extract_points, StereoRig.integrate;
pds_tsdf_integrate_fwd, pds_tsdf_extract_fwd).

The arbiters are the numpy fp64 oracles of tests/test_tsdf_host.py (themselves held to hand-written answers there).
integrate: no voxel is left out; the weight is exact, the tsdf within EPS (Z + z_c) / truncation, a voxel the oracle does
not update keeps its bits, and a voxel fp32 cannot decide (within TAU of a pixel border, within EPS (Z + z_c) of
-truncation) must equal one of its admissible outcomes.  extract_points: count and index exact, points within 1e-5
voxel_size + 4 ulp, NaN normals exactly where the oracle has them, the others within 2.28e-5 rad (the bound
tests/test_gpu_surface_normals.py derives for float32 normals).  The extraction works on tiles of TILE = 1024 voxels and
integrate on quads of four voxels, so the shapes sit around both."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib
from tests.test_gpu_register_depth import off_by_one, rig_pair
from tests.test_register_depth_host import EPS, simple_rig
from tests.test_tsdf_host import (GENERAL, MAX_GROUPS, TILE, WALL, camera_of, check_integration, fresh_state,
                                  general_case, general_disparity, general_pose, oracle_extract, oracle_integrate, q_of,
                                  surface_gap, wall_layers, wall_volume)

pytestmark = pytest.mark.gpu

NAN = float('nan')
ANGLE = 2.28e-5   # rad: tests/test_gpu_surface_normals.py, 4 eps32


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def put(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def state_of(volume):
    assert volume.tsdf.dtype == volume.weight.dtype == torch.float32 and volume.tsdf.shape == volume.shape
    return volume.tsdf.cpu().numpy(), volume.weight.cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_state(a, b):
    return torch.equal(bits(a.tsdf), bits(b.tsdf)) and torch.equal(bits(a.weight), bits(b.weight))


# ------------------------------------------------------------------------------------------------ 1. known answer
@pytest.mark.parametrize('dims', [(1, 1, 1), (5, 3, 2), (33, 7, 9), (257, 3, 5)], ids=lambda d: '%dx%dx%d' % d)
def test_wall_known_answer(dev, dims):
    nx, ny, nz = dims
    origin, Q = wall_volume(dims)
    height, width = WALL['height'], WALL['width']
    d = np.full((1, height, width), WALL['disparity'], dtype=np.float32)
    by_hand_t, by_hand_w = wall_layers(nz)
    # EPS (Z + z_c) / truncation with the layer's own z_c = z0 + (k + 0.5) voxel_size
    layer_z = WALL['z0'] + (np.arange(nz) + 0.5) * WALL['voxel_size']
    bound = np.broadcast_to((EPS * (WALL['depth'] + layer_z) / WALL['truncation'])[:, None, None], (nz, ny, nx))
    rng = np.random.RandomState(nx)
    valid = rng.rand(1, height, width) > 0.3
    confidence = rng.rand(1, height, width).astype(np.float32)
    for use_valid, use_confidence in ((False, False), (True, False), (True, True)):
        kw = dict(valid=valid[0] if use_valid else None, confidence=confidence[0] if use_confidence else None,
                  min_confidence=0.25)
        volume = pds.TsdfVolume(origin, WALL['voxel_size'], dims, WALL['truncation'], device=dev)
        old = state_of(volume)
        assert (old[0] == 1.0).all() and (old[1] == 0.0).all() and old[0].shape == (nz, ny, nx)
        oracle = oracle_integrate(*old, d[0], Q, origin, WALL['voxel_size'], WALL['truncation'], **kw)
        for frame in range(1, 4):
            volume.integrate(put(dev, d), Q, valid=put(dev, valid) if use_valid else None,
                             confidence=put(dev, confidence) if use_confidence else None, min_confidence=0.25)
            got_t, got_w = state_of(volume)
            case = (dims, use_valid, use_confidence, frame)
            # where the oracle is sure: the hand values of the layer, the weight exact; elsewhere 1.0 / 0.0 bit for bit
            # (behind -truncation, outside the image, under valid == False, under a low confidence)
            sure_on, sure_off = oracle.updated, ~oracle.updated & ~oracle.ambiguous
            layer_t = np.broadcast_to(by_hand_t[:, None, None], got_t.shape)
            layer_w = np.broadcast_to(by_hand_w[:, None, None], got_t.shape)
            assert np.array_equal(got_w[sure_on], frame * layer_w[sure_on]), case
            allowed = bound + 1e-6 * (frame - 1)   # (the running average is rounded from the second frame on)
            assert (np.abs(got_t - layer_t) <= allowed)[sure_on].all(), case
            assert (got_t[sure_off].view(np.int32) == np.float32(1.0).view(np.int32)).all() and (got_w[sure_off] == 0.0).all(), case
            # an ambiguous voxel reads one of two pixels of the same wall: the layer's values or, under a mask, nothing
            undecided = oracle.ambiguous
            assert (((got_w == frame * layer_w) & (np.abs(got_t - layer_t) <= allowed)) |
                    ((got_w == 0.0) & (got_t == 1.0)))[undecided].all(), case
        if not use_valid:
            assert oracle.updated.any() and (nz < 4 or not oracle.updated[3:].any()), dims
            if nx > 20:
                assert not oracle.projects.all()   # (the volume is wider than the image sees)
        # reset() restores the initial state
        volume.reset()
        assert (volume.tsdf == 1.0).all() and (volume.weight == 0.0).all()


# ------------------------------------------------------------------------------------------------ 2. the general case
def general_volume(dev, max_weight=64.0):
    return pds.TsdfVolume(GENERAL['origin'], GENERAL['voxel_size'], GENERAL['dims'], GENERAL['truncation'],
                          max_weight=max_weight, device=dev)


@functools.lru_cache(maxsize=None)
def general_oracle():
    return oracle_integrate(*fresh_state(GENERAL['dims']), **general_case())


def integrate_case(dev, volume, case, **kw):
    return volume.integrate(put(dev, case['disparity'][None]), case['matrix'], pose=case['pose'], **kw)


def test_general_case_against_fp64(dev):
    case = general_case()
    assert case['disparity'].shape == (48, 64) and np.abs(case['pose'][:, :3] - np.eye(3)).max() > 0.02
    oracle = general_oracle()
    voxels = oracle.tsdf.size
    ambiguous = float((oracle.ambiguous & oracle.projects).sum()) / float(oracle.projects.sum())
    crossings = len(oracle_extract(oracle.tsdf.astype(np.float32), oracle.weight.astype(np.float32), GENERAL['origin'],
                                   GENERAL['voxel_size']).index)
    print('%.2f %% of the projecting voxels ambiguous, %.1f %% updated, %d crossings' %
          (100 * ambiguous, 100 * oracle.updated.sum() / voxels, crossings))
    assert ambiguous <= 0.05 and oracle.updated.sum() / voxels >= 0.20 and crossings >= 1000
    volume = general_volume(dev)
    old = state_of(volume)
    integrate_case(dev, volume, case)
    got = state_of(volume)
    sure = ~oracle.ambiguous
    error = np.abs(got[0] - oracle.tsdf)[sure & oracle.updated]
    print('tsdf: largest error %.3g, largest share of its bound %.3g' %
          (error.max(), (error / oracle.bound[sure & oracle.updated]).max()))
    assert check_integration(*got, *old, oracle, case='general') > 8000
    assert np.array_equal(got[1][sure], oracle.weight[sure])   # (the weight is exact)


def test_three_poses_in_sequence(dev):
    """valid, confidence and weight_by_confidence on the second frame.  Each frame is checked against the oracle applied
    to the state the GPU had before it (every voxel); the voxels that were never ambiguous also against the fp64 chain."""
    rng = np.random.RandomState(7)
    valid = rng.rand(48, 64) > 0.1
    confidence = (0.05 + 0.95 * rng.rand(48, 64)).astype(np.float32)
    confidence[rng.rand(48, 64) < 0.03] = NAN
    extras = ({}, dict(valid=valid, confidence=confidence, min_confidence=0.2, weight_by_confidence=True), {})
    for max_weight in (64.0, 2.0):
        volume = general_volume(dev, max_weight)
        chain = fresh_state(GENERAL['dims'])
        never_ambiguous = np.ones(chain[0].shape, dtype=bool)
        largest = np.zeros(chain[0].shape)
        for k in range(3):
            case = general_case(k)
            old = state_of(volume)
            oracle = oracle_integrate(*old, max_weight=max_weight, **case, **extras[k])
            integrate_case(dev, volume, case, **{name: put(dev, v[None]) if isinstance(v, np.ndarray) else v
                                                 for name, v in extras[k].items()})
            got = state_of(volume)
            assert check_integration(*got, *old, oracle, extra=1e-6, weight_rtol=1e-6, case=(max_weight, k)) > 5000
            step = oracle_integrate(*chain, max_weight=max_weight, **case, **extras[k])
            chain = (step.tsdf, step.weight)
            never_ambiguous &= ~step.ambiguous
            largest = np.maximum(largest, step.bound)
            assert (np.abs(got[0] - chain[0]) <= largest + 1e-6 * (k + 1))[never_ambiguous].all(), (max_weight, k)
            assert (np.abs(got[1] - chain[1]) <= 1e-6 * chain[1])[never_ambiguous].all(), (max_weight, k)
        assert got[1].max() <= max_weight
        if max_weight == 2.0:
            assert (got[1] == 2.0).sum() > 1000   # the cap holds exactly, and it is reached
        else:
            assert got[1].max() > 2.0 and never_ambiguous.mean() > 0.9


# ------------------------------------------------------------------------------------------------ 3. batch
def test_a_batch_is_its_entries_in_order(dev):
    frames = put(dev, np.stack([general_disparity(k) for k in range(3)]))
    poses = np.stack([general_pose(k) for k in range(3)])
    Q = general_case()['matrix']
    rng = np.random.RandomState(11)
    confidence = put(dev, (0.1 + 0.9 * rng.rand(3, 48, 64)).astype(np.float32))
    kw = dict(confidence=confidence, weight_by_confidence=True)
    batched = general_volume(dev, 2.5).integrate(frames, Q, pose=poses, **kw)
    one_by_one = general_volume(dev, 2.5)
    for k in range(3):
        one_by_one.integrate(frames[k:k + 1], Q, pose=poses[k], confidence=confidence[k:k + 1], weight_by_confidence=True)
    assert same_state(batched, one_by_one) and float(batched.weight.max()) == 2.5
    # B = 2 with the entries swapped: the order the doc promises, entry 0 first -- and with the cap at work it matters
    for order in ((0, 1), (1, 0)):
        index = list(order)
        both = general_volume(dev, 0.75).integrate(frames[index], Q, pose=poses[index], confidence=confidence[index],
                                                    weight_by_confidence=True)
        apart = general_volume(dev, 0.75)
        for k in order:
            apart.integrate(frames[k:k + 1], Q, pose=poses[k], confidence=confidence[k:k + 1], weight_by_confidence=True)
        assert same_state(both, apart), order
        if order == (0, 1):
            forward = both
    assert not same_state(both, forward)
    # one pose for every entry
    shared = general_volume(dev).integrate(frames[:2], Q, pose=poses[0])
    apart = general_volume(dev).integrate(frames[:1], Q, pose=poses[0]).integrate(frames[1:2], Q, pose=poses[0])
    assert same_state(shared, apart)


# ------------------------------------------------------------------------------------------------ 4. extraction
def random_volume(dims, seed, min_weight=1.0, observed=0.6):
    """Random float32 tsdf in [-1, 1] with -0.0, 0.0 and 1.0 among them, random weights around min_weight of which the
    share `observed` reaches it (a normal needs twelve observed voxels: few have one unless most voxels are observed)."""
    nx, ny, nz = dims
    rng = np.random.RandomState(seed)
    tsdf = rng.uniform(-1.0, 1.0, (nz, ny, nx)).astype(np.float32)
    special = rng.rand(nz, ny, nx)
    tsdf[special < 0.03] = -0.0
    tsdf[(special >= 0.03) & (special < 0.06)] = 0.0
    tsdf[(special >= 0.06) & (special < 0.09)] = 1.0
    above = rng.choice(np.array([min_weight, min_weight, 2.0 * min_weight, 64.0], dtype=np.float32), (nz, ny, nx))
    below = rng.choice(np.array([0.0, 0.5 * min_weight, np.nextafter(np.float32(min_weight), np.float32(0.0))],
                                dtype=np.float32), (nz, ny, nx))
    weight = np.where(rng.rand(nz, ny, nx) < observed, above, below)
    return tsdf, weight


def check_surface(got, oracle, voxel_size, case=''):
    """got: SurfacePoints (trimmed); -> the number of points with a normal."""
    points, index = got.cloud.points.cpu().numpy(), got.cloud.index.cpu().numpy()
    assert got.cloud.colors is None and got.cloud.offsets.cpu().tolist() == [0, len(oracle.index)], case
    assert index.dtype == np.int32 and np.array_equal(index, oracle.index), case
    assert points.dtype == np.float32 and points.shape == (len(oracle.index), 3), case
    tolerance = 1e-5 * voxel_size + 4 * np.spacing(np.abs(oracle.points).astype(np.float32)).astype(np.float64)
    assert (np.abs(points - oracle.points) <= tolerance).all(), case
    if got.normals is None:
        return 0, 0
    normals = got.normals.cpu().numpy().astype(np.float64)
    assert normals.shape == points.shape, case
    missing = np.isnan(oracle.normals).any(axis=1)
    assert np.array_equal(np.isnan(normals), np.isnan(oracle.normals)), case
    with np.errstate(invalid='ignore'):
        checked = ~missing & (oracle.gradient_norm >= 1e-4)
    cross = np.linalg.norm(np.cross(normals[checked], oracle.normals[checked]), axis=1)
    dot = (normals[checked] * oracle.normals[checked]).sum(axis=1)
    angle = np.arctan2(cross, dot)
    assert angle.max(initial=0.0) <= ANGLE, (case, float(angle.max(initial=0.0)))
    assert np.abs(np.linalg.norm(normals[~missing], axis=1) - 1.0).max(initial=0.0) <= 1e-6, case
    return int(checked.sum()), int((~missing).sum())


@pytest.mark.parametrize('dims', [(1, 1, 1), (2, 1, 1), (1023, 1, 1), (1025, 1, 1), (5, 4, 3), (9, 2, 7), (17, 9, 5),
                                  (40, 36, 28)], ids=lambda d: '%dx%dx%d' % d)
def test_extraction_on_hand_made_volumes(dev, dims):
    origin, voxel_size = (-1.5, 0.25, 3.0), 0.03
    for min_weight, observed in ((1.0, 0.6), (0.375, 0.97)):
        tsdf, weight = random_volume(dims, sum(dims), min_weight, observed)
        oracle = oracle_extract(tsdf, weight, origin, voxel_size, min_weight)
        volume = pds.TsdfVolume(origin, voxel_size, dims, 0.1, device=dev)
        volume.tsdf, volume.weight = put(dev, tsdf), put(dev, weight)
        got = volume.extract_points(min_weight=min_weight)
        checked = check_surface(got, oracle, voxel_size, (dims, min_weight))
        count = len(oracle.index)
        if dims == (40, 36, 28):
            # the inputs avoid a gradient too small to normalise to 2.28e-5 rad: every normal there is was compared
            assert count > 10000 and checked[0] == checked[1] > (50 if observed < 0.9 else 5000)
        if min(dims) == 1:
            assert checked == (0, 0)   # (no stencil fits)
        # without normals; and trim=False: full-capacity tensors, no host read, the same rows
        plain = volume.extract_points(min_weight=min_weight, with_normals=False)
        assert plain.normals is None and torch.equal(bits(plain.cloud.points), bits(got.cloud.points))
        untrimmed = volume.extract_points(min_weight=min_weight, capacity=count + 5, trim=False)
        assert untrimmed.cloud.points.shape == (count + 5, 3) and untrimmed.normals.shape == (count + 5, 3)
        assert untrimmed.cloud.index.shape == (count + 5,) and untrimmed.cloud.offsets.tolist() == [0, count]
        assert torch.equal(bits(untrimmed.cloud.points[:count]), bits(got.cloud.points))
        assert torch.equal(bits(untrimmed.normals[:count]), bits(got.normals))
        # a capacity below the count: exactly `capacity` rows are written, the true count is reported
        if count >= 2:
            lib = _lib.load()
            capacity = count // 2
            nbytes = lib.pds_tsdf_extract_workspace_bytes(*dims)
            buffers = [torch.full((3 * (capacity + 8),), -7.0, device=dev), torch.full((3 * (capacity + 8),), -7.0, device=dev),
                       torch.full((capacity + 8,), -5, dtype=torch.int32, device=dev)]
            offsets = torch.full((2,), -1, dtype=torch.int32, device=dev)
            workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.pds_tsdf_extract_fwd(
                _lib.ptr(volume.tsdf), _lib.ptr(volume.weight), (ctypes.c_float * 3)(*origin), voxel_size, min_weight,
                _lib.ptr(buffers[0]), _lib.ptr(buffers[1]), _lib.ptr(buffers[2]), _lib.ptr(offsets), capacity, *dims,
                _lib.ptr(workspace), nbytes, _lib.stream_handle(dev)), 'pds_tsdf_extract_fwd')
            assert offsets.tolist() == [0, count]
            assert torch.equal(bits(buffers[0][:3 * capacity]), bits(got.cloud.points[:capacity].reshape(-1)))
            assert torch.equal(bits(buffers[1][:3 * capacity]), bits(got.normals[:capacity].reshape(-1)))
            assert torch.equal(buffers[2][:capacity], got.cloud.index[:capacity])
            assert bool((buffers[0][3 * capacity:] == -7.0).all()) and bool((buffers[1][3 * capacity:] == -7.0).all())
            assert bool((buffers[2][capacity:] == -5).all())
            with pytest.raises(RuntimeError, match='do not fit capacity %d' % capacity):
                volume.extract_points(min_weight=min_weight, capacity=capacity)
            cut = volume.extract_points(min_weight=min_weight, capacity=capacity, trim=False)
            assert cut.cloud.points.shape == (capacity, 3) and cut.cloud.offsets.tolist() == [0, count]
    # no crossing; nothing observed
    volume.reset()
    empty = volume.extract_points(min_weight=0.0)
    assert empty.cloud.points.shape == (0, 3) and empty.normals.shape == (0, 3) and empty.cloud.offsets.tolist() == [0, 0]
    volume.tsdf = put(dev, tsdf)
    assert volume.extract_points().cloud.points.shape == (0, 3)   # (weights 0: unobserved)


# ------------------------------------------------------------------------------------------------ 5. end to end
def test_end_to_end_surface_and_ply(dev, tmp_path):
    case = general_case()
    volume = integrate_case(dev, general_volume(dev), case)
    got = volume.extract_points()
    oracle = oracle_extract(*state_of(volume), GENERAL['origin'], GENERAL['voxel_size'])
    check_surface(got, oracle, GENERAL['voxel_size'], 'end to end')
    points = got.cloud.points.cpu().numpy().astype(np.float64)
    assert len(points) >= 1000
    # The fp64 surface along the ray of a point is the depth its own edge was measured against (surface_gap): the voxel
    # of the edge with the negative tsdf has sdf in [-truncation, 0) against the Z of its pixel, and the point lies at
    # most one voxel along the edge's axis from that voxel's centre, which moves its depth by voxel_size |R[2, a]|.  On
    # the fp64 oracle's own surface the largest gap is 0.0603 m, 0.0007 m inside what this allows.
    R, t = case['pose'][:, :3], case['pose'][:, 3]
    gap, read, reach = surface_gap(points, got.cloud.index.cpu().numpy(), state_of(volume)[0], case['disparity'],
                                   case['matrix'], GENERAL['origin'], GENERAL['voxel_size'], pose=case['pose'])
    allowed = GENERAL['truncation'] + reach + EPS * 2.0 * read
    print('end to end: %d points, at most %.4f m from the depth their edge was measured against, %.4f m more than '
          'allowed' % (len(points), gap.max(), (gap - allowed).max()))
    assert np.isfinite(gap).all() and (gap <= allowed).all(), float((gap - allowed).max())
    # the normals face the camera, whose centre is -R^T t in the world frame
    normals = got.normals.cpu().numpy().astype(np.float64)
    has = ~np.isnan(normals).any(axis=1)
    to_camera = -R.T @ t - points
    assert has.sum() > 500 and ((normals[has] * to_camera[has]).sum(axis=1) > 0).all()
    # through save_ply and back
    path = str(tmp_path / 'surface.ply')
    pds.save_ply(path, got.cloud, normals=got.normals)
    raw = open(path, 'rb').read()
    header, body = raw.split(b'end_header\n', 1)
    assert b'element vertex %d\n' % len(points) in header and b'property float nx' in header
    vertices = np.frombuffer(body, dtype=np.dtype([(n, '<f4') for n in ('x', 'y', 'z', 'nx', 'ny', 'nz')]))
    assert len(vertices) == len(points) and np.array_equal(vertices['x'], got.cloud.points[:, 0].cpu().numpy())
    assert np.array_equal(vertices['nz'], got.normals[:, 2].cpu().numpy(), equal_nan=True)


# ------------------------------------------------------------------------------------------------ 6. the same bits
def big_case(dev):
    """540 x 960 into 256 x 256 x 128: a slanted wall with a box, seen from a slightly turned camera."""
    height, width = 540, 960
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    d = 60.0 + 0.02 * xx - 0.015 * yy
    d[150:400, 300:700] = 90.0
    d[np.random.RandomState(6).rand(height, width) < 0.02] = NAN
    Q = q_of(height, width, 700.0, 0.12)   # depth 84 / d: 0.93 .. 1.6 m
    pose = np.hstack([pds.rectification.rodrigues(np.array([0.02, -0.03, 0.01])), [[0.01], [-0.02], [0.02]]])
    return put(dev, d.astype(np.float32)[None]), Q, pose, dict(origin=(-0.64, -0.64, 0.8), voxel_size=0.005,
                                                                dims=(256, 256, 128), truncation=0.02)


def test_same_bits_on_every_run_and_stream(dev):
    d, Q, pose, geometry = big_case(dev)
    make = (lambda: pds.TsdfVolume(device=dev, **geometry))
    first = make().integrate(d, Q, pose=pose)
    assert 0.02 < float((first.weight > 0).float().mean()) < 0.9
    surface = first.extract_points(capacity=1 << 21)
    assert surface.cloud.points.shape[0] > 10000
    for _ in range(2):
        again = make().integrate(d, Q, pose=pose)
        assert same_state(again, first)
        other = again.extract_points(capacity=1 << 21)
        assert torch.equal(other.cloud.index, surface.cloud.index)
        assert torch.equal(bits(other.cloud.points), bits(surface.cloud.points))
        assert torch.equal(bits(other.normals), bits(surface.normals))
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        aside = make().integrate(d, Q, pose=pose)
        other = aside.extract_points(capacity=1 << 21)
    stream.synchronize()
    torch.cuda.current_stream(dev).wait_stream(stream)
    assert same_state(aside, first) and torch.equal(other.cloud.index, surface.cloud.index)
    assert torch.equal(bits(other.cloud.points), bits(surface.cloud.points))
    assert torch.equal(bits(other.normals), bits(surface.normals))


def guarded(t, lead, fill):
    """-> (buffer, view): a copy of t between two guard regions of 64 elements, beginning `lead` elements behind a 16-byte
    boundary."""
    buffer = torch.full((t.numel() + 128 + lead,), fill, dtype=t.dtype, device=t.device)
    view = buffer[64 + lead:64 + lead + t.numel()]
    view.copy_(t.reshape(-1))
    return buffer, view.view(t.shape)


def guards_untouched(buffer, lead, count, fill):
    head, tail = buffer[:64 + lead], buffer[64 + lead + count:]
    return bool((head == fill).all()) and bool((tail == fill).all())


def test_unaligned_state_and_outputs_agree_and_guards_stay(dev):
    lib = _lib.load()
    frames = put(dev, np.stack([general_disparity(k) for k in range(2)]))
    poses = np.stack([general_pose(k) for k in range(2)])
    Q = general_case()['matrix']
    rng = np.random.RandomState(5)
    confidence = put(dev, (0.1 + 0.9 * rng.rand(2, 48, 64)).astype(np.float32))
    for dims in ((40, 36, 28), (33, 7, 9), (1023, 3, 1)):
        geometry = dict(origin=(-0.01 * dims[0], -0.01 * dims[1], 0.35), voxel_size=0.02, dims=dims, truncation=0.06)
        for kw in ({}, dict(confidence=confidence, weight_by_confidence=True)):
            aligned = pds.TsdfVolume(device=dev, **geometry).integrate(frames, Q, pose=poses, **kw)
            assert bool((aligned.weight > 0).any())
            # the two tensors one element behind a boundary (one 16-byte grid fits both), and each alone (none does)
            for lead_t, lead_w in ((1, 1), (3, 3), (1, 0), (0, 2)):
                volume = pds.TsdfVolume(device=dev, **geometry)
                tsdf_buffer, tsdf_view = guarded(volume.tsdf, lead_t, -7.0)
                weight_buffer, weight_view = guarded(volume.weight, lead_w, -9.0)
                volume.tsdf, volume.weight = tsdf_view, weight_view
                assert volume.tsdf.data_ptr() % 16 == 4 * lead_t and volume.weight.data_ptr() % 16 == 4 * lead_w
                # unaligned inputs as well (the scalar form of tsdf_depth)
                volume.integrate(off_by_one(frames), Q, pose=poses,
                                 **{k: off_by_one(v) if isinstance(v, torch.Tensor) else v for k, v in kw.items()})
                where = (dims, sorted(kw), lead_t, lead_w)
                assert same_state(volume, aligned), where
                count = volume.tsdf.numel()
                assert guards_untouched(tsdf_buffer, lead_t, count, -7.0), where
                assert guards_untouched(weight_buffer, lead_w, count, -9.0), where
        # extraction from the unaligned state (both forms of the kernels: one misalignment for both tensors, and two)
        # into unaligned outputs between guards, the workspace between guards too
        surface = aligned.extract_points()
        count = surface.cloud.points.shape[0]
        assert count > 100 or dims != (40, 36, 28)
        if count == 0:   # (a volume in front of every surface: nothing to write)
            continue
        nbytes = lib.pds_tsdf_extract_workspace_bytes(*dims)
        origin = (ctypes.c_float * 3)(*np.asarray(geometry['origin'], dtype=np.float32).tolist())
        for lead, (lead_t, lead_w) in enumerate(((0, 0), (1, 1), (3, 3), (0, 2))):
            tsdf_buffer, tsdf_view = guarded(aligned.tsdf, lead_t, -7.0)
            weight_buffer, weight_view = guarded(aligned.weight, lead_w, -9.0)
            assert tsdf_view.data_ptr() % 16 == 4 * lead_t and weight_view.data_ptr() % 16 == 4 * lead_w
            workspace = torch.full((nbytes + 512,), 0x5A, dtype=torch.uint8, device=dev)
            points_buffer, points = guarded(torch.zeros(3 * count, device=dev), lead, -7.0)
            normals_buffer, normals = guarded(torch.zeros(3 * count, device=dev), (lead + 1) % 4, -8.0)
            index_buffer, index = guarded(torch.zeros(count, dtype=torch.int32, device=dev), (lead + 2) % 4, -5)
            offsets = torch.full((2,), -1, dtype=torch.int32, device=dev)
            _lib.check(lib.pds_tsdf_extract_fwd(
                _lib.ptr(tsdf_view), _lib.ptr(weight_view), origin, geometry['voxel_size'], 1.0, _lib.ptr(points),
                _lib.ptr(normals), _lib.ptr(index), _lib.ptr(offsets), count, *dims, _lib.ptr(workspace[256:]), nbytes,
                _lib.stream_handle(dev)), 'pds_tsdf_extract_fwd')
            torch.cuda.synchronize()
            where = (dims, lead, lead_t, lead_w)
            assert offsets.tolist() == [0, count], where
            assert torch.equal(bits(points), bits(surface.cloud.points.reshape(-1))), where
            assert torch.equal(bits(normals), bits(surface.normals.reshape(-1))), where
            assert torch.equal(index, surface.cloud.index), where
            assert guards_untouched(points_buffer, lead, 3 * count, -7.0), where
            assert guards_untouched(normals_buffer, (lead + 1) % 4, 3 * count, -8.0), where
            assert guards_untouched(index_buffer, (lead + 2) % 4, count, -5), where
            assert bool((workspace[:256] == 0x5A).all()) and bool((workspace[256 + nbytes:] == 0x5A).all()), where
            # the state is read only: its bits and its guards are what they were
            assert torch.equal(bits(tsdf_view), bits(aligned.tsdf)) and torch.equal(bits(weight_view), bits(aligned.weight))
            assert guards_untouched(tsdf_buffer, lead_t, aligned.tsdf.numel(), -7.0), where
            assert guards_untouched(weight_buffer, lead_w, aligned.weight.numel(), -9.0), where
    # the bytes around the workspace of integrate
    nbytes = lib.pds_tsdf_integrate_workspace_bytes(48, 64)
    workspace = torch.full((nbytes + 512,), 0x5A, dtype=torch.uint8, device=dev)
    volume = pds.TsdfVolume(device=dev, **geometry)
    rows = volume.transforms(poses, 2).astype(np.float32).reshape(-1)
    floats = (lambda values: (ctypes.c_float * len(values))(*[float(x) for x in values]))
    _lib.check(lib.pds_tsdf_integrate_fwd(
        _lib.ptr(frames), None, _lib.ptr(confidence), 0.0, 1, floats(Q.astype(np.float32).reshape(-1)), floats(rows),
        floats(camera_of(Q)), geometry['truncation'], 64.0, _lib.ptr(volume.tsdf), _lib.ptr(volume.weight), *dims, 2, 48,
        64, _lib.ptr(workspace[256:]), nbytes, _lib.stream_handle(dev)), 'pds_tsdf_integrate_fwd')
    torch.cuda.synchronize()
    assert same_state(volume, aligned)
    assert bool((workspace[:256] == 0x5A).all()) and bool((workspace[256 + nbytes:] == 0x5A).all())


# ------------------------------------------------------------------------------------------------ 7. probes, the rig
def probe(lib, name, run):
    _lib.check(lib.pds_probe_begin(name.encode(), 16), 'pds_probe_begin')
    try:
        run()
        torch.cuda.synchronize()
    finally:
        workgroups, ms = (ctypes.c_int * 16)(), (ctypes.c_float * 16)()
        count = lib.pds_probe_end(ms, workgroups, 16)
    assert count >= 0 and all(t >= 0 for t in ms[:count]), (name, lib.pds_last_error())
    return list(workgroups[:count])


def test_the_kernels_ran(dev):
    lib = _lib.load()
    frames = put(dev, np.stack([general_disparity(k) for k in range(2)]))
    poses = np.stack([general_pose(k) for k in range(2)])
    Q = general_case()['matrix']
    volume = general_volume(dev)
    depth = (48 * 64 + TILE - 1) // TILE
    voxels = 40 * 36 * 28
    groups = min(((voxels + 3) // 4 + 255) // 256, MAX_GROUPS)
    tiles = (voxels + TILE - 1) // TILE
    integrate = (lambda: volume.integrate(frames, Q, pose=poses))
    assert probe(lib, 'tsdf_depth', integrate) == [depth, depth]
    assert probe(lib, 'tsdf_integrate', integrate) == [groups, groups]
    assert probe(lib, 'tsdf_', integrate) == [depth, groups, depth, groups]
    extract = (lambda: volume.extract_points(trim=False, capacity=4096))
    assert probe(lib, 'tsdf_extract_count', extract) == [tiles]
    assert probe(lib, 'tsdf_extract_scan', extract) == [1]
    assert probe(lib, 'tsdf_extract_scatter', extract) == [tiles]
    assert probe(lib, 'tsdf_extract', extract) == [tiles, 1, tiles]
    # a volume larger than one grid: tsdf_integrate strides
    d, Q, pose, geometry = big_case(dev)
    big = pds.TsdfVolume(device=dev, **geometry)
    assert probe(lib, 'tsdf_integrate', lambda: big.integrate(d, Q, pose=pose)) == [MAX_GROUPS]


def test_through_the_rig(dev):
    torch.manual_seed(0)
    net = pds.PdsNetwork.default(63).eval().to(dev)
    left, right = rig_pair(dev)
    rig = simple_rig(256, 128)
    r = rig.reconstruct(net, left, right, max_difference=1.0)
    assert r.valid is not None and int(r.valid.sum()) > 100
    depth = rig.reproject(r.disparity, valid=r.valid, depth_only=True)
    near = float(depth[~depth.isnan()].median())
    geometry = dict(origin=(-0.5 * near, -0.3 * near, 0.7 * near), voxel_size=near / 64, dims=(64, 40, 40),
                    truncation=near / 16)
    pose = general_pose(1)
    through = rig.integrate(rig.tsdf_volume(device=dev, **geometry), r.disparity, pose, r.valid)
    camera = (rig.P1[0, 0], rig.P1[1, 1], rig.P1[0, 2], rig.P1[1, 2], 0.0)
    explicit = pds.TsdfVolume(device=dev, **geometry).integrate(r.disparity, rig.reprojection_matrix('rectified'),
                                                                pose=pose, camera=camera, valid=r.valid)
    assert isinstance(through, pds.TsdfVolume) and same_state(through, explicit)
    assert int((through.weight > 0).sum()) > 100
    # the rig's Q is of the canonical form: camera=None reads the same pinhole off it
    implied = pds.TsdfVolume(device=dev, **geometry).integrate(r.disparity, rig.reprojection_matrix('rectified'),
                                                               pose=pose, valid=r.valid)
    assert same_state(implied, explicit)
