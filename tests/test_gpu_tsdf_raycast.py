"""GPU (-m gpu): TSDF raycast (TsdfVolume.raycast, StereoRig.raycast, depth_to_disparity; pds_tsdf_raycast_fwd).

The arbiter is oracle_raycast of tests/test_tsdf_raycast_host.py (held to hand-written answers there), with its margins and
per-pixel bounds as derived in that file's text: decided pixels agree exactly in hit or miss, the depth lies within its
bound, NaN normals sit where the oracle has them and the others within the angle bound; an undecided pixel holds NaN or a
depth in [s0, s1].  The scenes are the ones whose undecided share that file caps on the CPU.  The kernel works on tiles of
16 x 16 pixels in waves of 8 x 8, so the image sizes sit around both."""
import ctypes

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib
from tests.test_gpu_tsdf import big_case, bits, guarded, guards_untouched, probe, put
from tests.test_register_depth_host import simple_rig
from tests.test_tsdf_host import GENERAL, general_case, general_disparity, general_pose
from tests.test_tsdf_raycast_host import (GENERAL_SIZE, RANDOM, RANDOM_CASES, RANDOM_DIMS, RAYWALL, TILE, WALL_DIMS,
                                          WALL_SIZES, check_raycast, end_to_end_gap, fourth_pose, general_camera,
                                          general_oracle, random_oracle, raycast_random_volume, raywall_camera,
                                          raywall_oracle, raywall_volume)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def host(result, entry=0):
    normals = None if result.normals is None else result.normals[entry].cpu().numpy()
    return result.depth[entry].cpu().numpy(), normals


def same_maps(a, b):
    return torch.equal(bits(a.depth), bits(b.depth)) and torch.equal(bits(a.normals), bits(b.normals))


def groups(batch, height, width):
    return batch * ((height + TILE - 1) // TILE) * ((width + TILE - 1) // TILE)


def wall_on(dev, dims):
    origin, z0, tsdf, weight = raywall_volume(dims)
    volume = pds.TsdfVolume(origin, RAYWALL['voxel_size'], dims, RAYWALL['truncation'], device=dev)
    volume.tsdf, volume.weight = put(dev, tsdf), put(dev, weight)
    return volume, z0


# ------------------------------------------------------------------------------------------------ 1. known answer
@pytest.mark.parametrize('dims', WALL_DIMS, ids=lambda d: '%dx%dx%d' % d)
def test_wall_known_answer(dev, dims):
    volume, z0 = wall_on(dev, dims)
    for size in WALL_SIZES:
        width, height = size
        got = volume.raycast(raywall_camera(size), size, step=RAYWALL['step'], near=RAYWALL['near'])
        assert got.depth.shape == (1, height, width) and got.normals.shape == (1, height, width, 3)
        assert got.depth.dtype == got.normals.dtype == torch.float32
        depth, normals = host(got)
        oracle, _ = raywall_oracle(dims, size, near=RAYWALL['near'])
        hits, _ = check_raycast(depth, normals, oracle, (dims, size))
        sure = oracle.hit & ~oracle.undecided
        assert hits == sure.sum() >= 1, (dims, size)
        # by hand: the wall's own depth, which the oracle has to 1e-12 (asserted on the CPU), within the oracle's bound,
        # and the normal (0, 0, -1)
        assert (np.abs(depth[sure] - z0) <= oracle.depth_bound[sure] + 1e-12).all(), (dims, size)
        assert np.abs(normals[sure] - np.array([0.0, 0.0, -1.0], dtype=np.float32)).max() <= 1e-6, (dims, size)
        assert np.isnan(depth[~oracle.enters & ~oracle.undecided]).all(), (dims, size)


def test_a_volume_with_a_dimension_of_one_is_all_nan(dev):
    for dims in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (1, 1, 1)):
        volume, _ = wall_on(dev, dims)
        got = volume.raycast(raywall_camera((17, 9)), (17, 9), step=RAYWALL['step'])
        assert bool(got.depth.isnan().all()) and bool(got.normals.isnan().all()), dims


# ------------------------------------------------------------------------------------------------ 2. against the oracle
def general_volume(dev, frames=3):
    volume = pds.TsdfVolume(GENERAL['origin'], GENERAL['voxel_size'], GENERAL['dims'], GENERAL['truncation'], device=dev)
    for k in range(frames):
        case = general_case(k)
        volume.integrate(put(dev, case['disparity'][None]), case['matrix'], pose=case['pose'])
    return volume


def test_general_case_against_fp64(dev):
    volume = general_volume(dev)
    state = volume.tsdf.cpu().numpy(), volume.weight.cpu().numpy()
    poses = [fourth_pose()] + [general_pose(k) for k in range(3)]
    single = volume.raycast(general_camera(), GENERAL_SIZE, pose=poses[0])
    batched = volume.raycast(general_camera(), GENERAL_SIZE, pose=np.stack(poses[1:]))
    assert batched.depth.shape == (3, 48, 64) and batched.normals.shape == (3, 48, 64, 3)
    for name, result, entry, pose in [('fourth', single, 0, poses[0])] + [(k, batched, k, poses[1 + k]) for k in range(3)]:
        oracle = general_oracle(*state, pose)
        depth, normals = host(result, entry)
        hits, compared = check_raycast(depth, normals, oracle, name)
        sure = oracle.hit & ~oracle.undecided
        error = np.abs(depth - oracle.depth)[sure]
        print('pose %s: %d decided hits, %d normals compared, largest depth error %.3g m, largest share of its bound %.3g'
              % (name, hits, compared, error.max(), (error / oracle.depth_bound[sure]).max()))
        assert hits >= 0.2 * 48 * 64 and compared >= 0.8 * hits, name
        # the camera centre is -R^T t: every normal faces it, n . dir < 0
        has = ~np.isnan(normals).any(axis=2)
        assert has.sum() > 500 and ((normals[has].astype(np.float64) * oracle.direction[has]).sum(axis=1) < 0).all(), name


def test_random_volumes_against_fp64(dev):
    for min_weight, observed in RANDOM_CASES:
        tsdf, weight = raycast_random_volume(RANDOM_DIMS, sum(RANDOM_DIMS), min_weight, observed)
        volume = pds.TsdfVolume(RANDOM['origin'], RANDOM['voxel_size'], RANDOM_DIMS, RANDOM['truncation'], device=dev)
        volume.tsdf, volume.weight = put(dev, tsdf), put(dev, weight)
        got = volume.raycast(general_camera(), GENERAL_SIZE, pose=fourth_pose(), min_weight=min_weight)
        oracle = random_oracle(tsdf, weight, min_weight, fourth_pose())
        hits, compared = check_raycast(*host(got), oracle, (min_weight, observed))
        assert hits >= 0.2 * 48 * 64 and compared >= 0.8 * hits, (min_weight, observed)
        # the volume is read only
        assert torch.equal(bits(volume.tsdf), bits(put(dev, tsdf))) and torch.equal(bits(volume.weight), bits(put(dev, weight)))
        # another min_weight is another answer
        other = volume.raycast(general_camera(), GENERAL_SIZE, pose=fourth_pose(), min_weight=65.0)
        assert bool(other.depth.isnan().all())


# ------------------------------------------------------------------------------------------------ 3. end to end
def test_end_to_end_against_the_integrated_frame(dev):
    """The bound and its derivation: test_end_to_end_bound_on_the_oracle in tests/test_tsdf_raycast_host.py."""
    case = general_case()
    volume = general_volume(dev, frames=1)
    state = volume.tsdf.cpu().numpy(), volume.weight.cpu().numpy()
    gap, allowed, count = end_to_end_gap(*state, None)
    print('the fp64 oracle: %d hits, largest gap %.4f m, %.4f m inside what the bound allows' %
          (count, gap.max(), (allowed - gap).min()))
    got = volume.raycast(general_camera(), GENERAL_SIZE, pose=case['pose'])
    gap, allowed, count = end_to_end_gap(*state, host(got)[0])
    print('the kernel: %d hits, largest gap %.4f m, %.4f m inside what the bound allows' %
          (count, gap.max(), (allowed - gap).min()))
    assert count >= 0.2 * 48 * 64 and (gap <= allowed).all()


# ------------------------------------------------------------------------------------------------ 4. batch, bits
def test_a_batch_is_its_entries(dev):
    volume = general_volume(dev)
    poses = np.stack([general_pose(k) for k in range(3)] + [fourth_pose()])
    batched = volume.raycast(general_camera(), GENERAL_SIZE, pose=poses)
    plain = volume.raycast(general_camera(), GENERAL_SIZE, pose=poses, with_normals=False)
    assert plain.normals is None and torch.equal(bits(plain.depth), bits(batched.depth))
    for k in range(4):
        one = volume.raycast(general_camera(), GENERAL_SIZE, pose=poses[k])
        assert torch.equal(bits(one.depth[0]), bits(batched.depth[k])), k
        assert torch.equal(bits(one.normals[0]), bits(batched.normals[k])), k
    assert not torch.equal(bits(batched.depth[0]), bits(batched.depth[3]))
    # more entries than one launch carries, at a size that is no multiple of the tile
    many = np.stack([poses[k % 4] for k in range(19)])
    wide = volume.raycast(general_camera(), (37, 21), pose=many)
    for k in (0, 15, 16, 18):
        one = volume.raycast(general_camera(), (37, 21), pose=many[k])
        assert torch.equal(bits(one.depth[0]), bits(wide.depth[k])) and torch.equal(bits(one.normals[0]), bits(wide.normals[k])), k
    # [1, 3, 4] and 3x4 and, for the identity, None
    assert same_maps(volume.raycast(general_camera(), GENERAL_SIZE, pose=poses[:1]),
                     volume.raycast(general_camera(), GENERAL_SIZE, pose=poses[0]))
    assert same_maps(volume.raycast(general_camera(), GENERAL_SIZE),
                     volume.raycast(general_camera(), GENERAL_SIZE, pose=np.hstack([np.eye(3), np.zeros((3, 1))])))


def test_same_bits_on_every_run_and_stream(dev):
    d, Q, pose, geometry = big_case(dev)
    volume = pds.TsdfVolume(device=dev, **geometry).integrate(d, Q, pose=pose)
    camera, size = (700.0, 700.0, 0.5 * 959, 0.5 * 539, 0.0), (960, 540)
    first = volume.raycast(camera, size, pose=pose)
    assert first.depth.shape == (1, 540, 960) and 0.05 < float((~first.depth.isnan()).float().mean())
    assert same_maps(volume.raycast(camera, size, pose=pose), first)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        aside = volume.raycast(camera, size, pose=pose)
    stream.synchronize()
    torch.cuda.current_stream(dev).wait_stream(stream)
    assert same_maps(aside, first)


# ------------------------------------------------------------------------------------------------ 5. alignment, guards
def test_unaligned_volume_and_outputs_agree_and_guards_stay(dev):
    lib = _lib.load()
    volume = general_volume(dev)
    width, height = 37, 21
    poses = np.stack([fourth_pose(), general_pose(1)])
    aligned = volume.raycast(general_camera(), (width, height), pose=poses)
    assert int((~aligned.depth.isnan()).sum()) > 100
    rows = volume.rays(poses, 2).astype(np.float32)
    floats = (lambda values: (ctypes.c_float * len(values))(*[float(x) for x in values]))
    count = 2 * height * width
    for lead in (1, 3):
        tsdf_buffer, tsdf_view = guarded(volume.tsdf, lead, -7.0)
        weight_buffer, weight_view = guarded(volume.weight, lead, -9.0)
        depth_buffer, depth = guarded(torch.zeros(count, device=dev), lead, -5.0)
        normals_buffer, normals = guarded(torch.zeros(3 * count, device=dev), lead, -3.0)
        for t in (tsdf_view, weight_view, depth, normals):
            assert t.data_ptr() % 16 == 4 * lead
        _lib.check(lib.pds_tsdf_raycast_fwd(
            _lib.ptr(tsdf_view), _lib.ptr(weight_view), *volume.dims, volume.voxel_size, floats(rows[:, :12].reshape(-1)),
            floats(rows[:, 12:].reshape(-1)), floats(general_camera()), 0.5 * volume.truncation, 0.0, float('inf'), 1.0,
            _lib.ptr(depth), _lib.ptr(normals), 2, height, width, _lib.stream_handle(dev)), 'pds_tsdf_raycast_fwd')
        torch.cuda.synchronize()
        assert torch.equal(bits(depth), bits(aligned.depth.reshape(-1))), lead
        assert torch.equal(bits(normals), bits(aligned.normals.reshape(-1))), lead
        assert guards_untouched(depth_buffer, lead, count, -5.0) and guards_untouched(normals_buffer, lead, 3 * count, -3.0)
        # the volume is read only: its bits and its guards are what they were
        assert torch.equal(bits(tsdf_view), bits(volume.tsdf)) and torch.equal(bits(weight_view), bits(volume.weight))
        assert guards_untouched(tsdf_buffer, lead, volume.tsdf.numel(), -7.0)
        assert guards_untouched(weight_buffer, lead, volume.weight.numel(), -9.0)


# ------------------------------------------------------------------------------------------------ 6. probes, the rig
def test_the_kernel_ran(dev):
    lib = _lib.load()
    volume = general_volume(dev, frames=0)
    poses = np.stack([general_pose(k) for k in range(3)])
    for batch, size in ((1, (64, 48)), (3, (64, 48)), (3, (37, 21)), (1, (1, 1))):
        run = (lambda: volume.raycast(general_camera(), size, pose=poses[:batch]))
        assert probe(lib, 'tsdf_raycast', run) == [groups(batch, size[1], size[0])], (batch, size)
    assert groups(3, 21, 37) == 3 * 2 * 3
    # integrate under the prefix tsdf_ still reports its own launches only
    frames = put(dev, np.stack([general_disparity(k) for k in range(2)]))
    reported = probe(lib, 'tsdf_', lambda: volume.integrate(frames, general_case()['matrix'], pose=poses[:2]))
    assert len(reported) == 4 and reported[0] == reported[2] == 3 and reported[1] == reported[3]


def test_through_the_rig(dev):
    # a slanted wall with a box in front of it, as the rig's rectified left camera sees it (a network with random weights
    # leaves too few pixels valid for a cell of eight observed voxels)
    rig = simple_rig(256, 128)
    yy, xx = np.mgrid[0:128, 0:256].astype(np.float64)
    d = 20.0 + 0.02 * xx - 0.01 * yy
    d[40:90, 100:180] = 26.0
    d = put(dev, d.astype(np.float32)[None])
    depth = rig.reproject(d, depth_only=True)
    near = float(depth.median())
    geometry = dict(origin=(-0.5 * near, -0.3 * near, 0.7 * near), voxel_size=near / 64, dims=(64, 40, 40),
                    truncation=near / 16)
    pose = general_pose(1)
    volume = rig.integrate(rig.tsdf_volume(device=dev, **geometry), d, pose)
    through = rig.raycast(volume, pose, min_weight=1.0)
    camera = (rig.P1[0, 0], rig.P1[1, 1], rig.P1[0, 2], rig.P1[1, 2], 0.0)
    explicit = volume.raycast(camera, (256, 128), pose=pose)
    assert isinstance(through, pds.Raycast) and through.depth.shape == (1, 128, 256) and same_maps(through, explicit)
    kept = ~through.depth.isnan()
    assert int(kept.sum()) > 0.2 * 128 * 256
    # at the integration pose the model is the frame again, to the truncation (the end-to-end test has the derivation)
    assert float((through.depth - depth).abs()[kept].median()) < geometry['voxel_size']
    # the rendered model as a frame: through the parts of the library that work on disparity images
    Q = rig.reprojection_matrix('rectified')
    disparity = pds.depth_to_disparity(through.depth, Q)
    assert disparity.dtype == torch.float32 and torch.equal(disparity.isnan(), ~kept)
    back = rig.reproject(disparity, depth_only=True)
    assert torch.equal(back.isnan(), ~kept)
    # Z -> d -> Z: two divisions and a rounded Q, a few roundings of 6e-8 each
    assert float(((back - through.depth).abs() / through.depth)[kept].max()) <= 1e-6
    fitted = rig.surface_normals(disparity)
    assert fitted.normals.shape == (1, 128, 256, 3) and int(fitted.valid.sum()) > 50
    mesh = rig.triangle_mesh(disparity)
    assert mesh.points.shape[0] > 100 and mesh.faces.shape[0] > 50
