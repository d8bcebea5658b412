"""GPU: colour tracking (pds_intensity_pyramid_fwd: intensity_pyramid; pds_icp_color_system_fwd: icp_color_rows, icp_reduce;
intensity_pyramid, icp_color_system, ColorTsdfVolume.track_color, StereoRig.track_color) against the oracles of
tests/test_icp_color_host.py, whose text says what is compared, what is undecided and where the bounds come from."""
import ctypes

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib, tracking
from tests.test_gpu_icp import check_system, doubles, tiles, wall_batch
from tests.test_gpu_tsdf import bits, guarded, guards_untouched, probe, put
from tests.test_icp_color_host import (ORACLE_CORNER, ORACLE_END, TEXTURED, colour_scenes, corner_camera, corner_color,
                                       corner_colour_frame, oracle_color_rows, oracle_intensity_pyramid, textured,
                                       textured_camera, textured_truth, textured_wall_frame, textured_wall_state)
from tests.test_icp_host import (CORNER, IDENTITY, POSE0, POSE1, TRACK, check_rows, corner_disparity, corner_matrix,
                                 corner_state, pose_error)
from tests.test_register_depth_host import simple_rig
from tests.test_tsdf_host import WALL as TSDF_WALL, general_pose, wall_volume

pytestmark = pytest.mark.gpu

NAN, INF = float('nan'), float('inf')
F = np.float32


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------ 1. the intensity pyramid
@pytest.mark.parametrize('size', ((37, 29), (64, 48)), ids=lambda s: '%dx%d' % s)
def test_intensity_pyramid_bit_for_bit(dev, size):
    width, height = size
    lib = _lib.load()
    rng = np.random.RandomState(width)
    picture = rng.randint(0, 256, size=(2, height, width, 3)).astype(np.uint8)
    floats = (picture.astype(F) + rng.rand(2, height, width, 3).astype(F))
    floats[rng.rand(2, height, width, 3) < 0.01] = NAN
    cases = (('uint8', picture, None, 1), ('nchw', np.ascontiguousarray(floats.transpose(0, 3, 1, 2)), 'nchw', 0),
             ('nhwc', floats, 'nhwc', 2))
    for name, image, layout, code in cases:
        for levels in (1, 3, 4):
            want = oracle_intensity_pyramid(image, levels, layout=layout or 'nhwc')
            got = pds.intensity_pyramid(put(dev, image), levels, layout=layout)
            assert len(got) == levels
            for l in range(levels):
                assert got[l].shape == (2, height >> l, width >> l) and got[l].dtype == torch.float32
                assert got[l].cpu().numpy().tobytes() == want[l].tobytes(), (name, levels, l)
        # a buffer offset by 4 bytes (the scalar form), with guard bands around the image and every level
        want = oracle_intensity_pyramid(image, 4, layout=layout or 'nhwc')
        source = put(dev, image)
        if code == 1:
            buffer, view = guarded(source.reshape(-1), 4, 77)   # (uint8: 4 elements are 4 bytes)
            lead = 4
        else:
            buffer, view = guarded(source.reshape(-1), 1, -7.0)
            lead = 1
        outputs = [guarded(torch.zeros(2 * (height >> l) * (width >> l), device=dev), 1, -3.0) for l in range(4)]
        pointers = (ctypes.c_void_p * 4)(*[o[1].data_ptr() for o in outputs])
        _lib.check(lib.pds_intensity_pyramid_fwd(_lib.ptr(view), code, pointers, 4, 2, height, width, _lib.stream_handle(dev)),
                   'pds_intensity_pyramid_fwd')
        torch.cuda.synchronize()
        for l, (out_buffer, out) in enumerate(outputs):
            assert out.cpu().numpy().tobytes() == want[l].tobytes(), (name, 'offset', l)
            assert guards_untouched(out_buffer, 1, out.numel(), -3.0), (name, l)
        assert guards_untouched(buffer, lead, source.numel(), 77 if code == 1 else -7.0), name
        assert torch.equal(bits(view) if code != 1 else view, bits(source.reshape(-1)) if code != 1 else source.reshape(-1))


# ------------------------------------------------------------------------------------------------ 2. rows
def run_scene(dev, kw, with_rows=True, **more):
    args = dict(transform=kw.get('transform'), max_distance=kw['max_distance'], min_cosine=kw.get('min_cosine', 0.0))
    for name in ('valid', 'confidence'):
        if name in kw:
            args[name] = put(dev, kw[name][None])
    if 'frame_normals' in kw:
        args['normals'] = put(dev, kw['frame_normals'][None])
    if 'min_confidence' in kw:
        args['min_confidence'] = kw['min_confidence']
    args.update(more)
    model = pds.Raycast(put(dev, kw['depth'][None]), put(dev, kw['normals'][None]))
    return pds.icp_color_system(put(dev, kw['disparity'][None]), put(dev, kw['intensity'][None]), kw['matrix'], model,
                                put(dev, kw['model_intensity'][None]), kw['camera'], with_rows=with_rows, **args), model, args


def test_rows_against_the_oracle(dev):
    worst = 0.0
    for name, kw in colour_scenes().items():
        got, model, args = run_scene(dev, kw)
        o = oracle_color_rows(**kw)
        rows = got.rows[0].cpu().numpy()
        assert rows.shape == kw['disparity'].shape + (14,)
        geometric, share_g = check_rows(np.ascontiguousarray(rows[..., :7]), o.geometric, name)
        # the photometric half is decided only where the geometric row is: an undecided geometric row takes it along
        count, share = check_rows(np.ascontiguousarray(rows[..., 7:]), o, name + ' (photometric)')
        print('%s: %d geometric and %d photometric decided rows compared, shares of the bound %.3f and %.3f' %
              (name, geometric, count, share_g, share))
        assert count >= 500, name
        worst = max(worst, share)
        # 3. the geometric half has the bits of icp_system on the same arguments, rows and sums
        plain = pds.icp_system(put(dev, kw['disparity'][None]), kw['matrix'], model, kw['camera'], with_rows=True, **args)
        assert torch.equal(bits(got.rows[..., :7].contiguous()), bits(plain.rows)), name
        assert torch.equal(doubles(got.system), doubles(plain.system)), name
        # 4. the photometric sums are the exact ordered sums of their own rows
        assert check_system(got.color_system, got.rows[..., 7:].contiguous(), name) >= count
    print('the largest share of the photometric bound: %.3f' % worst)


def test_systems_huber_and_their_bits(dev):
    kw = colour_scenes()['corner']
    base, model, args = run_scene(dev, kw)
    frame = put(dev, kw['disparity'][None])
    for huber in (None, INF, 0.01):
        got, _, _ = run_scene(dev, kw, huber=huber)
        want = pds.icp_system_robust(frame, kw['matrix'], model, kw['camera'], huber, **args)
        assert torch.equal(doubles(got.system), doubles(want.system)), huber
        assert torch.equal(doubles(got.color_system), doubles(base.color_system)), huber   # (its own threshold only)
    for color_huber in (None, INF):
        got, _, _ = run_scene(dev, kw, color_huber=color_huber, huber=0.01)
        assert torch.equal(doubles(got.color_system), doubles(base.color_system)), color_huber
    # a finite threshold: the weighted sums of the kernel's own rows, term by term as it forms them, any order
    residuals = base.rows[0, ..., 13].cpu().numpy()
    threshold = float(np.median(np.abs(residuals[~np.isnan(residuals)])))   # half of the rows are weighted
    got, _, _ = run_scene(dev, kw, color_huber=threshold)
    assert torch.equal(bits(got.rows), bits(base.rows))
    rows = got.rows[0, ..., 7:].cpu().numpy().reshape(-1, 7)
    rows = rows[~np.isnan(rows[:, 6])].astype(np.float64)
    size = np.abs(rows[:, 6].astype(F))
    with np.errstate(all='ignore'):
        weight = np.where(size <= F(threshold), F(1.0), F(threshold) / size).astype(np.float64)
    assert (weight < 1).sum() > 50 and (weight == 1).sum() > 50
    pairs = [(i, j) for i in range(6) for j in range(i, 6)] + [(i, 6) for i in range(6)] + [(6, 6)]
    system = got.color_system[0].cpu().numpy()
    assert system[28] == len(rows)
    for k, (i, j) in enumerate(pairs):
        terms = weight * (rows[:, i] * rows[:, j])
        # each term is rounded once (the weight), then n additions in fp64
        slack = (len(rows) + 1) * 2.0 ** -53 * np.abs(terms).sum()
        assert abs(system[k] - float(np.sum(terms))) <= 2 * slack, (k, system[k], float(np.sum(terms)))
    without = run_scene(dev, kw, with_rows=False, color_huber=threshold)[0]
    assert without.rows is None and torch.equal(doubles(without.color_system), doubles(got.color_system))


# ------------------------------------------------------------------------------------------------ 5. tiles, batches
def colour_batch(dev, batch, width, height, model_batch=None):
    args, kw, host = wall_batch(dev, batch, width, height, with_normals=True, model_batch=model_batch)
    frames, Q, model, camera = args
    rng = np.random.RandomState(batch + width)
    L = np.stack([textured(height, width).astype(F) + F(k) for k in range(model.depth.shape[0])])
    image = np.stack([textured(height, width).astype(F) + rng.randn(height, width).astype(F) for _ in range(batch)])
    if height > 1:
        L[rng.rand(*L.shape) < 0.02] = NAN
        image[rng.rand(*image.shape) < 0.02] = NAN
    return (frames, put(dev, image), Q, model, put(dev, L), camera), kw


@pytest.mark.parametrize('size', ((33, 31), (32, 32), (41, 25)), ids=lambda s: '%dx%d' % s)
def test_tile_and_batch_edges(dev, size):
    width, height = size
    assert height * width in (1023, 1024, 1025)
    for model_batch in (1, 17):
        args, kw = colour_batch(dev, 17, width, height, model_batch=model_batch)
        got = pds.icp_color_system(*args, with_rows=True, color_huber=20.0, **kw)
        assert got.rows.shape == (17, height, width, 14)
        assert check_system(got.system, got.rows[..., :7].contiguous(), size) > 0.3 * 17 * height * width
        assert float(got.color_system[:, 28].min()) > 0.2 * height * width
        plain = pds.icp_color_system(*args, color_huber=20.0, **kw)
        assert plain.rows is None and torch.equal(doubles(plain.system), doubles(got.system))
        assert torch.equal(doubles(plain.color_system), doubles(got.color_system))
        frames, image, Q, model, L, camera = args
        for b in (0, 8, 15, 16):
            m = b if model_batch > 1 else 0
            one = pds.icp_color_system(frames[b:b + 1], image[b:b + 1], Q,
                                       pds.Raycast(model.depth[m:m + 1], model.normals[m:m + 1]), L[m:m + 1], camera,
                                       with_rows=True, color_huber=20.0,
                                       **dict(kw, transform=kw['transform'][b], normals=kw['normals'][b:b + 1]))
            assert torch.equal(doubles(one.system[0]), doubles(got.system[b])), (size, model_batch, b)
            assert torch.equal(doubles(one.color_system[0]), doubles(got.color_system[b])), (size, model_batch, b)
            assert torch.equal(bits(one.rows[0]), bits(got.rows[b])), (size, model_batch, b)


def test_same_bits_on_every_run_and_stream(dev):
    args, kw = colour_batch(dev, 17, 41, 25)
    run = (lambda: pds.icp_color_system(*args, with_rows=True, huber=0.02, color_huber=10.0, **kw))
    first = run()
    for _ in range(2):
        again = run()
        assert torch.equal(doubles(again.system), doubles(first.system)) and torch.equal(bits(again.rows), bits(first.rows))
        assert torch.equal(doubles(again.color_system), doubles(first.color_system))
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        aside = run()
        pyramid_aside = pds.intensity_pyramid(args[1][:, None].expand(-1, 3, -1, -1).contiguous(), 3)
    stream.synchronize()
    torch.cuda.current_stream(dev).wait_stream(stream)
    assert torch.equal(doubles(aside.system), doubles(first.system)) and torch.equal(bits(aside.rows), bits(first.rows))
    assert torch.equal(doubles(aside.color_system), doubles(first.color_system))
    here = pds.intensity_pyramid(args[1][:, None].expand(-1, 3, -1, -1).contiguous(), 3)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(here, pyramid_aside))


def test_the_kernels_ran(dev):
    lib = _lib.load()
    for batch, width, height in ((1, 37, 21), (3, 41, 25), (17, 64, 48)):
        args, kw = colour_batch(dev, batch, width, height)
        run = (lambda: pds.icp_color_system(*args, **kw))
        per_launch = [min(16, batch - first) * tiles(height, width) for first in range(0, batch, 16)]
        assert probe(lib, 'icp_color_rows', run) == per_launch, (batch, width, height)
        assert probe(lib, 'icp_reduce', run) == [2 * batch], (batch, width, height)
        assert probe(lib, 'icp_rows', run) == []   # the geometric kernel of icp_system does not run
        image = args[1][:, None].expand(-1, 3, -1, -1).contiguous()
        groups = batch * ((height + 31) // 32) * ((width + 31) // 32)
        for levels in (1, 3):
            assert probe(lib, 'intensity_pyramid', lambda: pds.intensity_pyramid(image, levels)) == [groups]


# ------------------------------------------------------------------------------------------------ 8. tracking
def textured_volume(dev, flat=False):
    tsdf, weight, color = textured_wall_state()
    if flat:
        color = np.full_like(color, 128.0)
    origin, Q = wall_volume(TEXTURED['dims'])
    volume = pds.ColorTsdfVolume(origin, TSDF_WALL['voxel_size'], TEXTURED['dims'], TSDF_WALL['truncation'], device=dev)
    volume.tsdf, volume.weight, volume.color = put(dev, tsdf), put(dev, weight), put(dev, color)
    return volume, Q


@pytest.mark.parametrize('levels', (1, 3))
def test_the_textured_wall_is_tracked_with_colour_and_refused_without(dev, levels):
    volume, Q = textured_volume(dev)
    disparity, image = textured_wall_frame(levels)
    frame, picture = put(dev, disparity[None]), put(dev, image[None])
    truth = textured_truth(levels)
    keywords = dict(camera=textured_camera(), iterations=TEXTURED['iterations'])
    # geometry alone: three motions are free
    plain = volume.track(frame, Q, IDENTITY, **keywords)
    assert plain.status.tolist() == [tracking.DEGENERATE] and (plain.pose[0] == IDENTITY).all()
    t = volume.track_color(frame, picture, Q, IDENTITY, levels=levels, color_weight=TEXTURED['color_weight'], **keywords)
    assert isinstance(t, pds.ColorTracking) and t.status.tolist() == [tracking.TRACKED]
    assert t.color_inliers[0] >= 0.2 * 48 * 64 and t.inliers[0] >= t.color_inliers[0] and t.color_rmse[0] < 30.0
    start, got = pose_error(IDENTITY, truth)[1], pose_error(t.pose[0], truth)[1]
    # the GPU follows the fp64 oracle loop in fp32 with a few undecided rows: twice its recorded end error, plus the
    # rounding of the pose to float32 on its way into the kernel (2^-24 of a translation below 2 m)
    bound = 2 * ORACLE_END[levels] + 2.0 * 2.0 ** -24
    print('levels %d: start %.3e m, the GPU ends %.3e m from the truth, the oracle loop recorded %.3e m: ratio %.2f' %
          (levels, start, got, ORACLE_END[levels], got / ORACLE_END[levels]))
    assert got <= bound   # measured on an MI355X: ratio got / ORACLE_END 0.97 (levels 1: 2.909e-04 m), 0.98 (levels 3: 1.082e-04 m)
    R = t.pose[0, :, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12


def test_no_behaviour_change_and_refusals(dev):
    # color_weight = 0, levels = 1: track_pyramid byte for byte, on the corner scene with a colour volume
    volume = pds.ColorTsdfVolume(CORNER['origin'], CORNER['voxel_size'], CORNER['dims'], CORNER['truncation'], device=dev)
    rng = np.random.RandomState(1)
    picture0 = put(dev, rng.randint(0, 256, size=(1, 48, 64, 3)).astype(np.uint8))
    volume.integrate(put(dev, corner_disparity(POSE0)[None]), corner_matrix(), pose=POSE0, image=picture0)
    frame = put(dev, corner_disparity(POSE1)[None])
    for huber in (None, 0.01):
        want = volume.track_pyramid(frame, corner_matrix(), POSE0, levels=1, huber=huber, **TRACK)
        got = volume.track_color(frame, picture0, corner_matrix(), POSE0, levels=1, huber=huber, color_weight=0.0, **TRACK)
        assert got.pose.tobytes() == want.pose.tobytes() and got.rmse.tobytes() == want.rmse.tobytes(), huber
        assert got.inliers.tolist() == want.inliers.tolist() and got.status.tolist() == want.status.tolist()
        assert got.iterations == want.iterations and want.status.tolist() == [tracking.TRACKED]
    # an untextured wall is still degenerate and does not raise; nothing to see is too few rows
    flat, Q = textured_volume(dev, flat=True)
    disparity, image = textured_wall_frame(1, True)
    refused = flat.track_color(put(dev, disparity[None]), put(dev, image[None]), Q, IDENTITY, camera=textured_camera())
    assert refused.status.tolist() == [tracking.DEGENERATE] and (refused.pose[0] == IDENTITY).all()
    assert refused.iterations == 1 and refused.color_inliers[0] > 0.2 * 48 * 64
    blind = flat.track_color(torch.full((1, 48, 64), NAN, device=dev), put(dev, image[None]), Q, IDENTITY)
    assert blind.status.tolist() == [tracking.TOO_FEW_ROWS] and blind.color_inliers.tolist() == [0]
    assert np.isnan(blind.color_rmse[0]) and (blind.pose[0] == IDENTITY).all()


def test_the_corner_scene_with_colour(dev):
    """track_color with the default colour weight ends no farther from the truth than track_pyramid on the same arguments,
    by more than the two fp64 oracle loops differ (tests/test_icp_color_host.py: ORACLE_CORNER).  Measured on an MI355X:
    1.583e-03 rad, 2.577e-03 m without colour and 1.184e-03 rad, 2.469e-03 m with it, the figures of the two oracle loops."""
    tsdf, weight = corner_state()
    volume = pds.ColorTsdfVolume(CORNER['origin'], CORNER['voxel_size'], CORNER['dims'], CORNER['truncation'], device=dev)
    volume.tsdf, volume.weight, volume.color = put(dev, tsdf), put(dev, weight), put(dev, corner_color())
    frame, picture = put(dev, corner_disparity(POSE1)[None]), put(dev, corner_colour_frame()[None])
    keywords = dict(TRACK, camera=corner_camera())
    plain = volume.track_pyramid(frame, corner_matrix(), POSE0, levels=1, **keywords)
    colour = volume.track_color(frame, picture, corner_matrix(), POSE0, levels=1, **keywords)
    assert plain.status.tolist() == colour.status.tolist() == [tracking.TRACKED]
    assert colour.color_inliers[0] >= 0.2 * 48 * 64
    a, b = pose_error(plain.pose[0], POSE1), pose_error(colour.pose[0], POSE1)
    print('geometric %.3e rad %.3e m (oracle %.3e, %.3e); with colour %.3e rad %.3e m (oracle %.3e, %.3e)' %
          (a + ORACLE_CORNER['geometric'] + b + ORACLE_CORNER['colour']))
    for k in range(2):
        assert b[k] <= a[k] + abs(ORACLE_CORNER['colour'][k] - ORACLE_CORNER['geometric'][k]), (k, a, b)


def test_through_the_rig(dev):
    rig = simple_rig(256, 128)
    yy, xx = np.mgrid[0:128, 0:256].astype(np.float64)
    d = 20.0 + 0.02 * xx - 0.01 * yy
    d[40:90, 100:180] = 26.0
    d = put(dev, d.astype(F)[None])
    picture = put(dev, np.stack([textured(128, 256)] * 3)[None].astype(F))
    near = float(rig.reproject(d, depth_only=True).median())
    geometry = dict(origin=(-0.5 * near, -0.3 * near, 0.7 * near), voxel_size=near / 64, dims=(64, 40, 40),
                    truncation=near / 16)
    pose = general_pose(1)
    volume = rig.integrate_color(rig.color_tsdf_volume(device=dev, **geometry), d, picture, pose)
    through = rig.track_color(volume, d, picture, pose, iterations=3)
    camera = (rig.P1[0, 0], rig.P1[1, 1], rig.P1[0, 2], rig.P1[1, 2], 0.0)
    explicit = volume.track_color(d, picture, rig.reprojection_matrix('rectified'), pose, camera=camera, size=(256, 128),
                                  iterations=3)
    assert isinstance(through, pds.ColorTracking) and through.inliers[0] > 1000 and through.color_inliers[0] > 1000
    assert through.pose.tobytes() == explicit.pose.tobytes() and through.rmse.tobytes() == explicit.rmse.tobytes()
    assert through.color_rmse.tobytes() == explicit.color_rmse.tobytes() and through.iterations == explicit.iterations
    assert through.status.tolist() == explicit.status.tolist() == [tracking.TRACKED]
