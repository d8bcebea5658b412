"""GPU: frame-to-model tracking (pds_icp_system_fwd: icp_rows, icp_reduce; icp_system, TsdfVolume.track, StereoRig.track)
against the fp64 oracle of tests/test_icp_host.py, whose text says what is compared, what is undecided and where the bounds
come from.  The image sizes sit around the tile of 1024 pixels and the wave of 64 lanes; batches of 1, 3 and 19 entries (one
launch of icp_rows carries 16).  Measured on an MI355X: the largest share of a row's bound the kernel used was 0.234, and
the tracked pose of the corner scene lay 1.31e-03 rad and 8.20e-04 m from the truth (the fp64 oracle loop: 1.68e-03 rad and
8.35e-04 m; the start: 2.08e-02 rad and 4.39e-02 m)."""
import ctypes

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib, tracking
from tests.test_gpu_tsdf import big_case, bits, guarded, guards_untouched, probe, put
from tests.test_icp_host import (CORNER, IDENTITY, POSE0, POSE1, SYSTEM, TILE, TRACK, camera_of, check_rows, corner_disparity,
                                 corner_matrix, corner_tracked, exact_system, gpu_scenes, oracle_rows, pose_error, wall_case)
from tests.test_register_depth_host import simple_rig
from tests.test_tsdf_host import general_case, general_disparity, general_pose

pytestmark = pytest.mark.gpu

NAN = float('nan')
SIZES = ((1, 1), (37, 21), (41, 25), (64, 48))   # (width, height): one pixel, under a tile, one over it, three tiles
BATCHES = (1, 3, 19)


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def tiles(height, width):
    return (height * width + TILE - 1) // TILE


def doubles(t):
    return t.contiguous().view(torch.int64)


def entry_transform(k):
    """A few milliradians and millimetres, another for every entry; entry 0 of a single pixel stays inside its model."""
    rng = np.random.RandomState(100 + k)
    return np.hstack([pds.rectification.rodrigues(0.01 * rng.randn(3)), 0.004 * rng.randn(3, 1)])


def wall_batch(dev, batch, width, height, with_normals=False, model_batch=None):
    """-> (the arguments of icp_system on the device, the same per entry on the host)."""
    rng = np.random.RandomState(7 * batch + width)
    d, Q, depth, normals, camera = wall_case(height, width, slope=0.0005)
    model_batch = model_batch or batch
    frames = np.stack([d + 0.02 * rng.rand(height, width).astype(np.float32) for _ in range(batch)])
    depths = np.stack([depth + np.float32(0.001 * k) for k in range(model_batch)])
    model_normals = np.stack([normals for _ in range(model_batch)])
    if height > 1:   # (a single pixel keeps its row)
        frames[rng.rand(*frames.shape) < 0.03] = NAN
        depths[rng.rand(*depths.shape) < 0.02] = NAN
    transforms = np.stack([entry_transform(k) if height > 1 else IDENTITY for k in range(batch)])
    frame_normals = None
    if with_normals:
        frame_normals = np.zeros((batch, height, width, 3), dtype=np.float32)
        frame_normals[..., 2] = np.where((rng.rand(batch, height, width) < 0.1) & (height > 1), 1.0, -1.0)
        frame_normals[(rng.rand(batch, height, width) < 0.05) & (height > 1)] = NAN
    host = dict(disparity=frames, matrix=Q, depth=depths, normals=model_normals, camera=camera, transform=transforms,
                frame_normals=frame_normals, max_distance=0.1, min_cosine=0.5 if with_normals else 0.0)
    kw = dict(transform=transforms, normals=put(dev, frame_normals), max_distance=0.1, min_cosine=host['min_cosine'])
    return (put(dev, frames), Q, pds.Raycast(put(dev, depths), put(dev, model_normals)), camera), kw, host


def oracle_of(host, b):
    model = b if len(host['depth']) > 1 else 0
    return oracle_rows(host['disparity'][b], host['matrix'], host['depth'][model], host['normals'][model], host['camera'],
                       transform=host['transform'][b],
                       frame_normals=None if host['frame_normals'] is None else host['frame_normals'][b],
                       max_distance=host['max_distance'], min_cosine=host['min_cosine'])


def check_system(system, rows, where=''):
    """system float64 [B, 29] against the exact sums of the products of the float32 rows [B, H, W, 7] the call returned."""
    system, rows = system.cpu().numpy(), rows.cpu().numpy()
    assert system.dtype == np.float64 and system.shape == (rows.shape[0], SYSTEM)
    for b in range(rows.shape[0]):
        sums, terms, count = exact_system(rows[b])
        assert system[b, 28] == count, (where, b)
        slack = count * 2.0 ** -53 * terms
        assert (np.abs(system[b] - sums) <= slack).all(), (where, b, np.abs(system[b] - sums) - slack)
    return int(system[:, 28].sum())


# ------------------------------------------------------------------------------------------------ 1. rows
def test_rows_against_the_oracle(dev):
    worst = 0.0
    for name, kw in gpu_scenes().items():
        got = pds.icp_system(put(dev, kw['disparity'][None]), kw['matrix'],
                             pds.Raycast(put(dev, kw['depth'][None]), put(dev, kw['normals'][None])), kw['camera'],
                             transform=kw['transform'], normals=put(dev, kw['frame_normals'][None]) if 'frame_normals' in kw
                             else None, max_distance=kw['max_distance'], min_cosine=kw.get('min_cosine', 0.0), with_rows=True)
        o = oracle_rows(**kw)
        count, share = check_rows(got.rows[0].cpu().numpy(), o, name)
        print('%s: %d decided rows compared, the largest share of the bound %.3f' % (name, count, share))
        assert count >= (1 if name.startswith('wall 1x1') else 500), name
        assert check_system(got.system, got.rows, name) >= count
        worst = max(worst, share)
    print('the largest share of the bound: %.3f' % worst)
    # the batched wall scenes: NaN disparities, NaN model pixels, frame normals that look away or are NaN
    for with_normals in (False, True):
        args, kw, host = wall_batch(dev, 3, 41, 25, with_normals=with_normals)
        got = pds.icp_system(*args, with_rows=True, **kw)
        for b in range(3):
            count, share = check_rows(got.rows[b].cpu().numpy(), oracle_of(host, b), (with_normals, b))
            assert count > 300


# ------------------------------------------------------------------------------------------------ 2. - 4. the system
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_system_against_its_own_rows_and_a_batch_is_its_entries(dev, size):
    width, height = size
    for batch in BATCHES:
        for with_normals in (False, True):
            for model_batch in (1, batch):
                args, kw, host = wall_batch(dev, batch, width, height, with_normals=with_normals, model_batch=model_batch)
                where = (size, batch, with_normals, model_batch)
                got = pds.icp_system(*args, with_rows=True, **kw)
                assert got.rows.shape == (batch, height, width, 7) and got.rows.dtype == torch.float32
                rows = check_system(got.system, got.rows, where)
                assert rows >= (1 if size == (1, 1) else 0.3 * batch * height * width), where
                # 3. without rows: the same bits
                plain = pds.icp_system(*args, **kw)
                assert plain.rows is None and torch.equal(doubles(plain.system), doubles(got.system)), where
                # 4. a batch is its entries, bit for bit
                frames, Q, model, camera = args
                for b in sorted({0, batch // 2, min(15, batch - 1), min(16, batch - 1), batch - 1}):
                    m = b if model_batch > 1 else 0
                    one = pds.icp_system(frames[b:b + 1], Q, pds.Raycast(model.depth[m:m + 1], model.normals[m:m + 1]),
                                         camera, with_rows=True,
                                         **dict(kw, transform=kw['transform'][b],
                                                normals=None if kw['normals'] is None else kw['normals'][b:b + 1]))
                    assert torch.equal(doubles(one.system[0]), doubles(got.system[b])), (where, b)
                    assert torch.equal(bits(one.rows[0]), bits(got.rows[b])), (where, b)
    # the corner scene too, with valid and confidence
    scene = gpu_scenes()['corner aligned']
    rng = np.random.RandomState(2)
    valid, confidence = rng.rand(1, 48, 64) < 0.9, rng.rand(1, 48, 64).astype(np.float32)
    if size == SIZES[-1]:
        got = pds.icp_system(put(dev, scene['disparity'][None]), scene['matrix'],
                             pds.Raycast(put(dev, scene['depth'][None]), put(dev, scene['normals'][None])),
                             scene['camera'], transform=scene['transform'], valid=put(dev, valid),
                             confidence=put(dev, confidence), min_confidence=0.2, max_distance=scene['max_distance'],
                             with_rows=True)
        assert check_system(got.system, got.rows, 'corner') > 1000
        o = oracle_rows(valid=valid[0], confidence=confidence[0], min_confidence=0.2, **scene)
        assert check_rows(got.rows[0].cpu().numpy(), o, 'corner, masked')[0] > 1000


# ------------------------------------------------------------------------------------------------ 5. the same bits
def test_same_bits_on_every_run_and_stream(dev):
    args, kw, _ = wall_batch(dev, 19, 41, 25, with_normals=True)
    first = pds.icp_system(*args, with_rows=True, **kw)
    again = pds.icp_system(*args, with_rows=True, **kw)
    assert torch.equal(doubles(again.system), doubles(first.system)) and torch.equal(bits(again.rows), bits(first.rows))
    # 960 x 540 against a model raycast from the big case
    d, Q, pose, geometry = big_case(dev)
    volume = pds.TsdfVolume(device=dev, **geometry).integrate(d, Q, pose=pose)
    camera = (700.0, 700.0, 0.5 * 959, 0.5 * 539, 0.0)
    model = volume.raycast(camera, (960, 540), pose=pose)
    run = (lambda: pds.icp_system(d, Q, model, camera, transform=entry_transform(0), max_distance=0.04, with_rows=True))
    first = run()
    assert float(first.system[0, 28]) > 0.05 * 540 * 960
    check_system(first.system, first.rows, 'big')
    again = run()
    assert torch.equal(doubles(again.system), doubles(first.system)) and torch.equal(bits(again.rows), bits(first.rows))
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        aside = run()
    stream.synchronize()
    torch.cuda.current_stream(dev).wait_stream(stream)
    assert torch.equal(doubles(aside.system), doubles(first.system)) and torch.equal(bits(aside.rows), bits(first.rows))


# ------------------------------------------------------------------------------------------------ 6. alignment, guards
def test_unaligned_buffers_agree_and_guards_stay(dev):
    lib = _lib.load()
    batch, width, height = 3, 41, 25
    args, kw, host = wall_batch(dev, batch, width, height, with_normals=True)
    frames, Q, model, camera = args
    rng = np.random.RandomState(4)
    confidence = put(dev, rng.rand(batch, height, width).astype(np.float32))
    valid = put(dev, rng.rand(batch, height, width) < 0.9)
    aligned = pds.icp_system(*args, valid=valid, confidence=confidence, min_confidence=0.1, with_rows=True, **kw)
    assert float(aligned.system[:, 28].min()) > 100
    floats = (lambda values: (ctypes.c_float * len(values))(*[float(x) for x in values]))
    transforms = np.concatenate([kw['transform'][:, :, :3].reshape(batch, 9), kw['transform'][:, :, 3]], axis=1)
    nbytes = lib.pds_icp_workspace_bytes(batch, height, width)
    count = batch * height * width
    for lead in (1, 3):
        inputs = {}
        for name, t, fill in (('disparity', frames, -7.0), ('confidence', confidence, -6.0), ('normals', kw['normals'], -5.0),
                              ('depth', model.depth, -4.0), ('model_normals', model.normals, -3.0)):
            inputs[name] = guarded(t, lead, fill) + (t, fill)
        valid_buffer, valid_view = guarded(valid.view(torch.uint8), lead, 77)
        rows_buffer, rows = guarded(torch.zeros(7 * count, device=dev), lead, -2.0)
        system_buffer, system = guarded(torch.zeros(2 * SYSTEM * batch, dtype=torch.int32, device=dev), lead, -1)
        workspace = torch.full((nbytes + 512,), 0x5A, dtype=torch.uint8, device=dev)
        for t in [v[1] for v in inputs.values()] + [rows, system]:
            assert t.data_ptr() % 16 == 4 * lead
        _lib.check(lib.pds_icp_system_fwd(
            _lib.ptr(inputs['disparity'][1]), _lib.ptr(valid_view), _lib.ptr(inputs['confidence'][1]), 0.1,
            floats(Q.astype(np.float32).reshape(-1)), _lib.ptr(inputs['normals'][1]), _lib.ptr(inputs['depth'][1]),
            _lib.ptr(inputs['model_normals'][1]), batch, height, width, floats(camera),
            floats(transforms.astype(np.float32).reshape(-1)), kw['max_distance'], kw['min_cosine'], _lib.ptr(system),
            _lib.ptr(rows), batch, height, width, _lib.ptr(workspace[256:]), nbytes, _lib.stream_handle(dev)),
            'pds_icp_system_fwd')
        torch.cuda.synchronize()
        assert torch.equal(bits(rows), bits(aligned.rows.reshape(-1))), lead
        assert torch.equal(system, aligned.system.contiguous().view(torch.int32).reshape(-1)), lead
        assert guards_untouched(rows_buffer, lead, 7 * count, -2.0) and guards_untouched(system_buffer, lead, system.numel(), -1)
        assert bool((workspace[:256] == 0x5A).all()) and bool((workspace[256 + nbytes:] == 0x5A).all()), lead
        # the inputs are read only: their bits and their guards are what they were
        for name, (buffer, view, original, fill) in inputs.items():
            assert torch.equal(bits(view), bits(original)) and guards_untouched(buffer, lead, original.numel(), fill), name
        assert torch.equal(valid_view, valid.view(torch.uint8)) and guards_untouched(valid_buffer, lead, count, 77)


# ------------------------------------------------------------------------------------------------ 7. probes
def test_the_kernels_ran(dev):
    lib = _lib.load()
    for batch in BATCHES:
        for width, height in SIZES:
            args, kw, _ = wall_batch(dev, batch, width, height)
            run = (lambda: pds.icp_system(*args, **kw))
            per_launch = [min(16, batch - first) * tiles(height, width) for first in range(0, batch, 16)]
            assert probe(lib, 'icp_rows', run) == per_launch, (batch, width, height)
            assert sum(per_launch) == batch * tiles(height, width)
            assert probe(lib, 'icp_reduce', run) == [batch], (batch, width, height)
            assert probe(lib, 'icp_', run) == per_launch + [batch]
    assert tiles(25, 41) == 2 and tiles(48, 64) == 3 and tiles(21, 37) == 1
    # integrate under the prefix tsdf_ still reports its own launches only
    volume = pds.TsdfVolume(device=dev, origin=(-0.40, -0.36, 0.35), voxel_size=0.02, dims=(40, 36, 28), truncation=0.06)
    frames = put(dev, np.stack([general_disparity(k) for k in range(2)]))
    poses = np.stack([general_pose(k) for k in range(2)])
    reported = probe(lib, 'tsdf_', lambda: volume.integrate(frames, general_case()['matrix'], pose=poses))
    assert len(reported) == 4 and reported[0] == reported[2] == 3 and reported[1] == reported[3]


# ------------------------------------------------------------------------------------------------ 8. - 10. tracking
def corner_volume(dev):
    volume = pds.TsdfVolume(CORNER['origin'], CORNER['voxel_size'], CORNER['dims'], CORNER['truncation'], device=dev)
    return volume.integrate(put(dev, corner_disparity(POSE0)[None]), corner_matrix(), pose=POSE0)


def test_tracking_the_corner_scene(dev):
    volume = corner_volume(dev)
    frame = put(dev, corner_disparity(POSE1)[None])
    t = volume.track(frame, corner_matrix(), POSE0, **TRACK)
    assert isinstance(t, pds.Tracking) and t.pose.shape == (1, 3, 4) and t.pose.dtype == np.float64
    assert t.status.tolist() == [tracking.TRACKED] and 1 <= t.iterations <= 10 and t.inliers[0] >= 0.2 * 48 * 64
    oracle_pose, _, status = corner_tracked()
    assert status == tracking.TRACKED
    start, want, got = pose_error(POSE0, POSE1), pose_error(oracle_pose, POSE1), pose_error(t.pose[0], POSE1)
    print('start %.3e rad %.3e m; the fp64 oracle loop %.3e rad %.3e m; the GPU %.3e rad %.3e m, rmse %.3e, %d inliers, '
          '%d iterations' % (start + want + got + (t.rmse[0], t.inliers[0], t.iterations)))
    assert got[0] <= 2 * want[0] and got[1] <= 2 * want[1]
    # a rotation stays a rotation
    R = t.pose[0, :, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12
    # the returned pose is what integrate takes, and the loop goes on
    volume.integrate(frame, corner_matrix(), pose=t.pose)
    model = volume.raycast(camera_of(corner_matrix()), (64, 48), pose=t.pose)
    assert int((~model.depth.isnan()).sum()) > 0.2 * 48 * 64
    # a batch of frames: the tracked frame and the frame the model was made of
    both = volume.track(torch.cat([frame, put(dev, corner_disparity(POSE0)[None])]), corner_matrix(),
                        np.stack([POSE0, POSE0]), **TRACK)
    assert both.status.tolist() == [tracking.TRACKED] * 2 and pose_error(both.pose[1], POSE0)[1] < 0.01


def test_refusals_do_not_raise(dev):
    # a single wall: three motions are free
    volume = pds.TsdfVolume(CORNER['origin'], CORNER['voxel_size'], CORNER['dims'], CORNER['truncation'], device=dev)
    wall = put(dev, np.full((1, 48, 64), 6.0, dtype=np.float32))   # Z = 7.2 / 6 = 1.2
    volume.integrate(wall, corner_matrix(), pose=POSE0)
    t = volume.track(wall, corner_matrix(), POSE0)
    assert t.status.tolist() == [tracking.DEGENERATE] and (t.pose[0] == POSE0).all() and t.inliers[0] > 0.2 * 48 * 64
    assert t.iterations == 1 and t.rmse[0] < 0.01
    # nothing to see
    blind = volume.track(torch.full_like(wall, NAN), corner_matrix(), POSE0)
    assert blind.status.tolist() == [tracking.TOO_FEW_ROWS] and (blind.pose[0] == POSE0).all()
    assert blind.inliers.tolist() == [0] and np.isnan(blind.rmse[0])
    # one of each in a batch, beside a frame that can be tracked
    corner = corner_volume(dev)
    frames = torch.cat([put(dev, corner_disparity(POSE1)[None]), torch.full_like(wall, NAN)])
    mixed = corner.track(frames, corner_matrix(), np.stack([POSE0, POSE0]), **TRACK)
    assert mixed.status.tolist() == [tracking.TRACKED, tracking.TOO_FEW_ROWS] and (mixed.pose[1] == POSE0).all()
    assert pose_error(mixed.pose[0], POSE1)[1] < 0.005


def test_through_the_rig(dev):
    rig = simple_rig(256, 128)
    yy, xx = np.mgrid[0:128, 0:256].astype(np.float64)
    d = 20.0 + 0.02 * xx - 0.01 * yy
    d[40:90, 100:180] = 26.0
    d = put(dev, d.astype(np.float32)[None])
    near = float(rig.reproject(d, depth_only=True).median())
    geometry = dict(origin=(-0.5 * near, -0.3 * near, 0.7 * near), voxel_size=near / 64, dims=(64, 40, 40),
                    truncation=near / 16)
    pose = general_pose(1)
    volume = rig.integrate(rig.tsdf_volume(device=dev, **geometry), d, pose)
    through = rig.track(volume, d, pose, iterations=3)
    camera = (rig.P1[0, 0], rig.P1[1, 1], rig.P1[0, 2], rig.P1[1, 2], 0.0)
    explicit = volume.track(d, rig.reprojection_matrix('rectified'), pose, camera=camera, size=(256, 128), iterations=3)
    assert isinstance(through, pds.Tracking) and through.inliers[0] > 1000
    assert through.pose.tobytes() == explicit.pose.tobytes() and through.rmse.tobytes() == explicit.rmse.tobytes()
    assert through.inliers.tolist() == explicit.inliers.tolist() and through.status.tolist() == explicit.status.tolist()
    assert through.iterations == explicit.iterations
