"""GPU (-m gpu): depth registration (register_depth, StereoRig.register_depth; pds_register_depth_fwd).

Where the answer is known in integers (the identity round trip, the right view of integer disparities, the contention on
one pixel) `index` and `valid` are compared exactly and `depth` to 4 ulp of the existing `reproject` on the same inputs.
In the general case the arbiter is the numpy fp64 oracle of tests/test_register_depth_host.py (itself held to hand-written
answers there): no pixel is left out; a source whose fp64 u or v lies within TAU = 2^-8 px of a border of its footprint
is an ambiguous candidate on either side, and depths are held to EPS = 1e-5 (relative).  The kernels work on tiles of
TILE = 1024 pixels (csrc/common.hpp: kRegisterDepthTile), so the shapes sit around it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib, registration
from tests.test_gpu_speckle import plane_scene
from tests.test_register_depth_host import (DISTORTION, EPS, GENERAL_SHAPE, IDENTITY, TARGETS, TAU, TILE,
                                            check_registration, general_case, oracle_registration, simple_rig,
                                            statistics)

pytestmark = pytest.mark.gpu

NAN, INF = float('nan'), float('inf')


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def q_of(height, width, focal=140.0, baseline=0.12):
    """A Q of a rig with that focal length (px) and baseline (m): depth = focal * baseline / d."""
    return np.array([[1.0, 0.0, 0.0, -0.5 * (width - 1)], [0.0, 1.0, 0.0, -0.5 * (height - 1)], [0.0, 0.0, 0.0, focal],
                     [0.0, 0.0, 1.0 / baseline, 0.0]])


def camera_of(Q):
    """The rectified left camera itself, from Q."""
    return (Q[2, 3], Q[2, 3], -Q[0, 3], -Q[1, 3], 0.0)


def put(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def numpy_of(result):
    assert isinstance(result, pds.RegisteredDepth)
    assert result.depth.dtype == torch.float32 and result.index.dtype == torch.int32 and result.valid.dtype == torch.bool
    assert result.depth.is_contiguous() and result.index.is_contiguous() and result.valid.is_contiguous()
    return result.depth.cpu().numpy(), result.index.cpu().numpy(), result.valid.cpu().numpy()


def run(dev, case, **kw):
    """register_depth on a dictionary of numpy arguments (tests/test_register_depth_host.py: general_case)."""
    tensors = {k: put(dev, case[k]) if k in ('disparity', 'valid', 'confidence') else case[k] for k in case}
    tensors.update(kw)
    return pds.register_depth(**tensors)


def ulps(a, b):
    """Distance in units of the last place between float32 arrays of positive finite numbers."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def scene(shape, seed):
    return np.stack([plane_scene(shape[1], shape[2], seed=seed + b) for b in range(shape[0])])


# ------------------------------------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 1, 255), (1, 1, 256), (1, 1, 257), (2, 3, 5), (3, 65, 129),
                                   (1, 1, TILE - 1), (1, 1, TILE + 1), (1, 3, TILE // 3 + 1), (2, 17, 61)],
                         ids=lambda s: '%dx%dx%d' % s)
def test_identity_round_trip(dev, shape):
    """The target is the rectified left camera itself: u, v sit within 1e-3 px of the source's own integers, so every
    kept pixel lands on itself."""
    batch, height, width = shape
    Q = q_of(height, width)
    rng = np.random.RandomState(sum(shape))
    d = scene(shape, 1)
    d[0, 0, 0] = 33.0   # (at least one kept pixel, also in 1 x 1 x 1)
    valid = rng.rand(*shape) > 0.3
    confidence = rng.rand(*shape).astype(np.float32)
    confidence[rng.rand(*shape) < 0.05] = NAN
    own = np.broadcast_to(np.arange(height * width, dtype=np.int32).reshape(1, height, width), shape)
    for use_valid in (False, True):
        for use_confidence in (False, True):
            for splat in (1, 2) if (use_valid and use_confidence) else (1,):
                v, c = put(dev, valid if use_valid else None), put(dev, confidence if use_confidence else None)
                reference = pds.reproject(put(dev, d), Q, valid=v, confidence=c, min_confidence=0.25,
                                          depth_only=True).cpu().numpy()
                kept = ~np.isnan(reference)
                assert kept.any() or use_valid or use_confidence
                result = pds.register_depth(put(dev, d), Q, IDENTITY, camera_of(Q), None, (width, height), valid=v,
                                            confidence=c, min_confidence=0.25, splat=splat)
                depth, index, hit = numpy_of(result)
                case = (shape, use_valid, use_confidence, splat)
                if splat == 1:
                    assert np.array_equal(hit, kept), case
                    assert np.array_equal(index, np.where(kept, own, -1)), case
                    assert np.isnan(depth[~kept]).all() and ulps(depth[kept], reference[kept]).max(initial=0) <= 4, case
                else:
                    # the 2 x 2 footprint of a kept pixel always holds the pixel itself (u within 1e-3 of x: floor(u) is
                    # x or x - 1), so every kept pixel is hit, by itself or by something at most as far
                    assert hit[kept].all(), case
                    assert (depth[kept] <= reference[kept] * (1 + 1e-6)).all(), case
                    assert np.array_equal(index >= 0, hit) and np.isnan(depth[~hit]).all(), case
                    flat = reference.reshape(batch, -1)
                    for b in range(batch):
                        won = index[b][hit[b]]
                        assert ulps(depth[b][hit[b]], flat[b][won]).max(initial=0) <= 4, case


# ------------------------------------------------------------------------------------------------ 2. the right view
def box_scene(height, width, wall, boxes):
    """Integer disparities: a wall of disparity `wall` with boxes (y0, y1, x0, x1, d) in front of it."""
    d = np.full((height, width), wall, dtype=np.int64)
    for y0, y1, x0, x1, value in boxes:
        d[y0:y1, x0:x1] = value
    return d


def right_view_in_integers(d):
    """-> (index, valid) [H, W]: the source x lands on column x - d of its row; the larger disparity (the nearer
    surface) wins.  Two sources of one row with the same disparity never meet."""
    height, width = d.shape
    index = np.full((height, width), -1, dtype=np.int32)
    best = np.zeros((height, width), dtype=np.int64)
    for y in range(height):
        for x in range(width):
            tx = x - d[y, x]
            if d[y, x] > 0 and 0 <= tx < width and d[y, x] > best[y, tx]:
                best[y, tx], index[y, tx] = d[y, x], y * width + x
    return index, index >= 0


def test_right_view_known_answer(dev):
    height, width = 40, 150
    scenes = [box_scene(height, width, 4, [(10, 30, 60, 100, 12)]),
              box_scene(height, width, 3, [(0, 15, 20, 50, 9), (20, 40, 90, 149, 17), (5, 35, 70, 80, 0)])]
    d = np.stack(scenes).astype(np.float32)
    Q = q_of(height, width)
    to_the_right = np.hstack([np.eye(3), [[-0.12], [0.0], [0.0]]])
    result = pds.register_depth(put(dev, d), Q, to_the_right, camera_of(Q), None, (width, height))
    depth, index, hit = numpy_of(result)
    reference = pds.reproject(put(dev, d), Q, depth_only=True).cpu().numpy().reshape(2, -1)   # (a pure x shift keeps Z)
    for b in range(2):
        expected_index, expected_valid = right_view_in_integers(scenes[b])
        assert np.array_equal(index[b], expected_index) and np.array_equal(hit[b], expected_valid), b
        assert ulps(depth[b][hit[b]], reference[b][index[b][hit[b]]]).max() <= 4 and np.isnan(depth[b][~hit[b]]).all(), b
    # scene 0 by hand, on a row through the box: the wall (x - 4) up to the box, the box (x - 12) on columns 48 .. 87
    # in front of the wall it overlaps, then the strip the box occludes, 88 .. 95, then the wall again
    row = index[0, 20] - 20 * width
    assert row[:48].tolist() == list(range(4, 52)) and row[48:88].tolist() == list(range(60, 100))
    assert not hit[0, 20, 88:96].any() and row[96:146].tolist() == list(range(100, 150)) and not hit[0, 20, 146:].any()
    assert hit[0, 5, :146].all()   # (a row beside the box: nothing is occluded)


# ------------------------------------------------------------------------------------------------ 3. the general case
@functools.lru_cache(maxsize=None)
def general_oracle(target, splat):
    return oracle_registration(splat=splat, tau=TAU, **general_case(target))


@pytest.mark.parametrize('splat', [1, 2])
@pytest.mark.parametrize('target', sorted(TARGETS))
def test_general_case_against_fp64(dev, target, splat):
    case = general_case(target)
    assert case['distortion'] == DISTORTION and case['disparity'].shape == GENERAL_SHAPE
    oracle = general_oracle(target, splat)
    ambiguous, contested = statistics(oracle)
    print('%s, splat %d: %.2f %% of the pairs ambiguous, %.1f %% of the hit pixels contested' %
          (target, splat, 100 * ambiguous, 100 * contested))
    assert ambiguous <= 0.05 and contested >= 0.30
    depth, index, hit = numpy_of(run(dev, case, splat=splat))
    assert check_registration(depth, index, hit, oracle, EPS, (target, splat)) > 1000


# ------------------------------------------------------------------------------------------------ 4. contention, emptiness
def test_every_source_on_one_pixel(dev):
    rng = np.random.RandomState(4)
    d = rng.choice(np.array([3.0, 5.0, 8.0, 8.0, NAN], dtype=np.float32), (2, 64, 64))
    d[0, :20] = np.minimum(d[0, :20], 5.0)   # entry 0: the first 8.0 comes late
    Q = q_of(64, 64)
    result = pds.register_depth(put(dev, d), Q, IDENTITY, (1e-3, 1e-3, 0.0, 0.0, 0.0), None, (1, 1))
    depth, index, hit = numpy_of(result)
    reference = pds.reproject(put(dev, d), Q, depth_only=True).cpu().numpy().reshape(2, -1)
    for b in range(2):
        first = int(np.flatnonzero(d[b].reshape(-1) == 8.0)[0])   # the global minimum of Z, the smallest index
        assert hit[b, 0, 0] and index[b, 0, 0] == first, (b, index[b, 0, 0], first)
        assert reference[b, first] == np.nanmin(reference[b]) and ulps(depth[b, 0, 0], reference[b, first]).max() <= 4
    assert index[0, 0, 0] >= 20 * 64


def test_everything_behind_the_camera(dev):
    d = put(dev, scene((2, 33, 70), 2))
    Q = q_of(33, 70)
    about_face = np.hstack([np.diag([-1.0, 1.0, -1.0]), np.zeros((3, 1))])
    for fill in (NAN, -1.0, 0.0):
        for splat in (1, 2):
            result = pds.register_depth(d, Q, about_face, camera_of(Q), None, (70, 33), splat=splat, fill_value=fill)
            depth, index, hit = numpy_of(result)
            assert not hit.any() and (index == -1).all(), (fill, splat)
            assert np.isnan(depth).all() if fill != fill else (depth == fill).all(), (fill, splat)
    # with_index=False leaves index None and changes nothing else
    result = pds.register_depth(d, Q, IDENTITY, camera_of(Q), None, (70, 33), fill_value=-1.0, with_index=False)
    assert result.index is None
    full = pds.register_depth(d, Q, IDENTITY, camera_of(Q), None, (70, 33), fill_value=-1.0)
    assert torch.equal(result.depth, full.depth) and torch.equal(result.valid, full.valid)
    assert bool((full.depth[~full.valid] == -1.0).all()) and bool(full.valid.any()) and not bool(full.valid.all())


def test_only_a_corner_is_hit(dev):
    shape = (1, 30, 50)
    d = np.full(shape, 14.0, dtype=np.float32)   # a wall 1.2 m away
    Q = q_of(30, 50)
    # the camera moved by 0.36 m right and 0.18 m down sees the wall 42 px to the left and 21 px up
    pose = np.hstack([np.eye(3), [[-0.36], [-0.18], [0.0]]])
    case = dict(disparity=d, matrix=Q, pose=pose, camera=camera_of(Q), distortion=None, size=(50, 30))
    for splat in (1, 2):
        depth, index, hit = numpy_of(run(dev, case, splat=splat))
        oracle = oracle_registration(splat=splat, tau=TAU, **case)
        check_registration(depth, index, hit, oracle, EPS, splat)
        assert hit[0, :8, :7].all() and not hit[0, 10:].any() and not hit[0, :, 9:].any(), splat
        assert 7 * 8 <= int(hit.sum()) <= 9 * 10


def test_fold_back_points_do_not_appear(dev):
    # k1 = -0.5 folds back from r2 = 2/3 on.  Source and target: 41 x 41 around (20, 20) with a focal length of 20 px, so
    # r2 = (i^2 + j^2) / 400 with integers i, j is never within 8e-4 of 2/3 and the fp32 decision is the fp64 one
    d = np.full((1, 41, 41), 2.0, dtype=np.float32)
    d[0, ::3, ::2] = 4.0
    Q = q_of(41, 41, focal=20.0)
    case = dict(disparity=d, matrix=Q, pose=IDENTITY, camera=camera_of(Q), distortion=(-0.5, 0.0, 0.0, 0.0), size=(41, 41))
    yy, xx = np.mgrid[0:41, 0:41]
    r2 = ((xx - 20.0) ** 2 + (yy - 20.0) ** 2) / 400.0
    assert np.abs(1.0 - 1.5 * r2).min() > 1e-3
    folded = (r2 >= 2.0 / 3.0).reshape(-1)
    radius = np.sqrt(r2) * (1.0 - 0.5 * r2) * 20.0   # where the model puts them: inside the image, without the guard
    assert folded.sum() > 400 and (radius.reshape(-1)[folded] < 11.0).all()
    for splat in (1, 2):
        oracle = oracle_registration(splat=splat, tau=TAU, **case)
        assert np.array_equal(oracle.kept[0].reshape(-1), ~folded)
        depth, index, hit = numpy_of(run(dev, case, splat=splat))
        assert check_registration(depth, index, hit, oracle, EPS, splat) > 300
        assert not folded[index[hit]].any(), splat
    # the same call without the distortion keeps them all
    case['distortion'] = None
    assert numpy_of(run(dev, case))[2].all()


# ------------------------------------------------------------------------------------------------ 5. the same bits
def distorted_target_case(shape, size, seed):
    batch, height, width = shape
    Q = q_of(height, width, focal=0.7 * width)
    rotation = pds.rectification.rodrigues(np.array([0.02, -0.03, 0.01]))
    rng = np.random.RandomState(seed)
    return dict(disparity=scene(shape, seed), matrix=Q, pose=np.hstack([rotation, [[0.03], [-0.01], [0.02]]]),
                camera=(0.8 * size[0], 0.8 * size[0], 0.5 * size[0] - 0.5, 0.5 * size[1] - 0.5, 0.0),
                distortion=DISTORTION, size=size, valid=rng.rand(*shape) > 0.1,
                confidence=rng.rand(*shape).astype(np.float32), min_confidence=0.1)


def same_bits(a, b):
    return (torch.equal(a.depth.view(torch.int32), b.depth.view(torch.int32)) and torch.equal(a.index, b.index) and
            torch.equal(a.valid, b.valid))


def test_same_bits_on_every_run_and_stream(dev):
    case = distorted_target_case((4, 540, 960), (1280, 720), 5)
    tensors = {k: put(dev, case[k]) if k in ('disparity', 'valid', 'confidence') else case[k] for k in case}
    for splat in (1, 2):
        first = pds.register_depth(splat=splat, **tensors)
        assert first.depth.shape == (4, 720, 1280) and 0.2 < float(first.valid.float().mean()) < 1.0
        for _ in range(2):
            assert same_bits(pds.register_depth(splat=splat, **tensors), first), splat
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            other = pds.register_depth(splat=splat, **tensors)
        stream.synchronize()
        torch.cuda.current_stream(dev).wait_stream(stream)
        assert same_bits(other, first), splat


def off_by_one(t):
    """A contiguous copy of t that begins one element behind a 16-byte boundary."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:]
    flat.copy_(t.reshape(-1))
    return flat.view(t.shape)


def test_unaligned_inputs_and_outputs_agree_and_guards_stay(dev):
    lib = _lib.load()
    floats = (lambda values: (ctypes.c_float * np.size(values))(*np.asarray(values, dtype=np.float32).reshape(-1).tolist()))
    for shape, size in (((2, 65, 129), (97, 61)), ((1, 33, 64), (64, 33)), ((3, 2, 342), (343, 16))):
        # (a two-row source seen from a camera a centimetre lower lands some five rows up: the target needs the rows)
        case = distorted_target_case(shape, size, 3)
        tensors = {k: put(dev, case[k]) if k in ('disparity', 'valid', 'confidence') else case[k] for k in case}
        targets = shape[0] * size[0] * size[1]
        for splat in (1, 2):
            aligned = pds.register_depth(splat=splat, **tensors)
            assert bool(aligned.valid.any())
            # unaligned INPUTS: the scalar load form
            shifted = dict(tensors, **{k: off_by_one(tensors[k]) for k in ('disparity', 'valid', 'confidence')})
            assert shifted['disparity'].data_ptr() % 16 == 4 and shifted['valid'].data_ptr() % 4 == 1
            assert same_bits(pds.register_depth(splat=splat, **shifted), aligned), (shape, splat)
            # unaligned OUTPUTS between guard rows: the entry point itself
            composed = registration.compose(case['pose'], case['matrix'])
            nbytes = lib.pds_register_depth_workspace_bytes(shape[0], size[1], size[0])
            workspace = torch.full((nbytes + 512,), 0x5A, dtype=torch.uint8, device=dev)
            for guard in (size[0] + (-size[0]) % 4, size[0] + (-size[0]) % 4 + 1, size[0] + (-size[0]) % 4 + 3):
                depth = torch.full((targets + 2 * guard,), -7.0, device=dev)
                index = torch.full((targets + 2 * guard,), -5, dtype=torch.int32, device=dev)
                hit = torch.full((targets + 2 * guard,), 99, dtype=torch.uint8, device=dev)
                _lib.check(lib.pds_register_depth_fwd(
                    _lib.ptr(tensors['disparity']), _lib.ptr(tensors['valid']), _lib.ptr(tensors['confidence']),
                    case['min_confidence'], floats(composed), floats(case['camera']), floats(case['distortion']), splat,
                    NAN, _lib.ptr(depth[guard:]), _lib.ptr(index[guard:]), _lib.ptr(hit[guard:]), *shape, size[1],
                    size[0], _lib.ptr(workspace[256:]), nbytes, _lib.stream_handle(dev)), 'pds_register_depth_fwd')
                torch.cuda.synchronize()
                where = (shape, splat, guard)
                assert depth[guard:].data_ptr() % 16 == 4 * (guard % 4)
                inner = slice(guard, guard + targets)
                assert torch.equal(depth[inner].view(torch.int32), aligned.depth.reshape(-1).view(torch.int32)), where
                assert torch.equal(index[inner], aligned.index.reshape(-1)), where
                assert torch.equal(hit[inner], aligned.valid.reshape(-1).to(torch.uint8)), where
                # nothing beside the outputs is written, nor beside the key buffer
                for buffer, sentinel in ((depth, -7.0), (index, -5), (hit, 99)):
                    assert bool((buffer[:guard] == sentinel).all()) and bool((buffer[guard + targets:] == sentinel).all()), where
                assert bool((workspace[:256] == 0x5A).all()) and bool((workspace[256 + nbytes:] == 0x5A).all()), where


# ------------------------------------------------------------------------------------------------ 6. the kernels ran
def test_the_two_kernels_ran(dev):
    lib = _lib.load()
    case = general_case('smaller')
    tensors = {k: put(dev, case[k]) if k in ('disparity', 'valid', 'confidence') else case[k] for k in case}
    scatter = (2 * 65 * 129 + TILE - 1) // TILE
    resolve = (2 * 61 * 97 + TILE - 1) // TILE
    for name, expected in (('register_depth', [scatter, resolve]), ('register_depth_scatter', [scatter]),
                           ('register_depth_resolve', [resolve])):
        for splat in (1, 2):
            _lib.check(lib.pds_probe_begin(name.encode(), 16), 'pds_probe_begin')
            try:
                pds.register_depth(splat=splat, **tensors)
                torch.cuda.synchronize()
            finally:
                workgroups, ms = (ctypes.c_int * 16)(), (ctypes.c_float * 16)()
                count = lib.pds_probe_end(ms, workgroups, 16)
            assert count == len(expected), (name, count, lib.pds_last_error())
            assert list(workgroups[:count]) == expected and all(t >= 0 for t in ms[:count]), name


# ------------------------------------------------------------------------------------------------ 7. through the rig
def rig_pair(dev):
    g = torch.Generator().manual_seed(3)
    left = torch.randint(0, 256, (1, 128, 256, 3), generator=g, dtype=torch.uint8).to(dev)
    right = torch.randint(0, 256, (1, 128, 256, 3), generator=g, dtype=torch.uint8).to(dev)
    return left, right


def test_through_the_rig(dev):
    torch.manual_seed(0)
    net = pds.PdsNetwork.default(63).eval().to(dev)
    left, right = rig_pair(dev)
    rig = simple_rig(256, 128)
    r = rig.reconstruct(net, left, right, max_difference=1.0)
    assert r.valid is not None and int(r.valid.sum()) > 100
    K3 = np.array([[150.0, 0.3, 159.5], [0.0, 152.0, 99.5], [0.0, 0.0, 1.0]])
    third = (K3, np.array(DISTORTION), pds.rectification.rodrigues([0.01, np.radians(4.0), -0.02]),
             np.array([0.02, -0.06, 0.01]), (320, 200))
    for kwargs in ({'view': 'left'}, {'view': 'right'}, {'camera': third}, {'camera': third, 'splat': 2}):
        result = rig.register_depth(r.disparity, valid=r.valid, **kwargs)
        pose, camera, distortion, size = rig.registration_target(kwargs.get('view', 'left'), kwargs.get('camera'))
        oracle = oracle_registration(r.disparity.cpu().numpy(), rig.reprojection_matrix('rectified'), pose, camera,
                                     distortion, size, valid=r.valid.cpu().numpy(), splat=kwargs.get('splat', 1), tau=TAU)
        depth, index, hit = numpy_of(result)
        assert depth.shape == (1, size[1], size[0])
        hits = check_registration(depth, index, hit, oracle, EPS, sorted(kwargs))
        print('register_depth %s: %d of %d target pixels hit by %d sources, %.2f %% of the pairs ambiguous' %
              (sorted(kwargs), hits, size[0] * size[1], int(oracle.kept.sum()), 100 * statistics(oracle)[0]))
        assert hits > 50

    # a rig without distortion or rotation: the raw left camera IS the rectified one, so the result is case 1
    plain = simple_rig(256, 128, distortion=False)
    assert np.allclose(plain.R1, np.eye(3), atol=1e-15) and np.allclose(plain.P1[:, :3], plain.K1, atol=1e-9)
    r = plain.reconstruct(net, left, right, max_difference=1.0)
    result = plain.register_depth(r.disparity, 'left', r.valid)
    depth, index, hit = numpy_of(result)
    reference = plain.reproject(r.disparity, valid=r.valid, depth_only=True).cpu().numpy()
    kept = ~np.isnan(reference)
    own = np.arange(128 * 256, dtype=np.int32).reshape(1, 128, 256)
    assert kept.sum() > 100 and np.array_equal(hit, kept) and np.array_equal(index, np.where(kept, own, -1))
    assert np.isnan(depth[~kept]).all() and ulps(depth[kept], reference[kept]).max() <= 4
