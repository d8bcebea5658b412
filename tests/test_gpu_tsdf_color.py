"""GPU: colour in TSDF fusion (ColorTsdfVolume: pds_tsdf_color_integrate_fwd, pds_tsdf_color_gather_fwd,
pds_tsdf_color_render_fwd) against the fp64 oracles of tests/test_tsdf_color_host.py, whose bounds are derived there.

1. the geometry of a ColorTsdfVolume is that of a TsdfVolume, bit for bit; 2. known answers, exact; 3. every frame against
fp64; 4. the gather on hand-made volumes; 5. the render; 6. the same bits on every run, stream and alignment, the launch
probes, and one pass through the rig."""
import ctypes

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib
from tests.test_gpu_tsdf import bits, guarded, guards_untouched, probe, put, random_volume, same_state, state_of
from tests.test_gpu_register_depth import off_by_one, rig_pair
from tests.test_register_depth_host import simple_rig
from tests.test_tsdf_color_host import (RENDER_CASES, check_render, holed_weight, oracle_color_integrate, oracle_gather,
                                        random_colors, random_image, render_oracle, render_scene)
from tests.test_tsdf_host import (GENERAL, MAX_GROUPS, fresh_state, general_case, general_disparity, general_pose,
                                  oracle_extract)
from tests.test_tsdf_raycast_host import GENERAL_SIZE, RANDOM, RANDOM_DIMS, fourth_pose, general_camera

pytestmark = pytest.mark.gpu

NAN = float('nan')


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def volumes(dev, max_weight=64.0, geometry=None):
    geometry = geometry or dict(origin=GENERAL['origin'], voxel_size=GENERAL['voxel_size'], dims=GENERAL['dims'],
                                truncation=GENERAL['truncation'])
    return (pds.ColorTsdfVolume(max_weight=max_weight, device=dev, **geometry),
            pds.TsdfVolume(max_weight=max_weight, device=dev, **geometry))


def sequence_extras():
    """valid, confidence and weight_by_confidence on the second of three frames (tests/test_gpu_tsdf.py)."""
    rng = np.random.RandomState(7)
    valid = rng.rand(48, 64) > 0.1
    confidence = (0.05 + 0.95 * rng.rand(48, 64)).astype(np.float32)
    confidence[rng.rand(48, 64) < 0.03] = NAN
    return ({}, dict(valid=valid, confidence=confidence, min_confidence=0.2, weight_by_confidence=True), {})


def on_device(dev, extras):
    return {name: put(dev, v[None]) if isinstance(v, np.ndarray) else v for name, v in extras.items()}


# ------------------------------------------------------------------------------------------------ 1. the same geometry
@pytest.mark.parametrize('layout', [0, 1], ids=['float32_nchw', 'uint8_nhwc'])
def test_the_geometry_is_the_parents_bit_for_bit(dev, layout):
    case = general_case()
    colored, plain = volumes(dev)
    d = put(dev, case['disparity'][None])
    colored.integrate(d, case['matrix'], pose=case['pose'], image=put(dev, random_image(0, layout)[None]))
    plain.integrate(d, case['matrix'], pose=case['pose'])
    assert same_state(colored, plain) and int((plain.weight > 0).sum()) > 8000
    assert float(colored.color.abs().max()) > 0 and bool((colored.color[colored.weight == 0] == 0).all())
    extras = sequence_extras()
    for max_weight in (64.0, 2.0):
        colored, plain = volumes(dev, max_weight)
        for k in range(3):
            case = general_case(k)
            d, kw = put(dev, case['disparity'][None]), on_device(dev, extras[k])
            colored.integrate(d, case['matrix'], pose=case['pose'], image=put(dev, random_image(k, layout)[None]), **kw)
            plain.integrate(d, case['matrix'], pose=case['pose'], **kw)
            assert same_state(colored, plain), (max_weight, k)
    # the products: the raycast's depth and normals, the points, normals, index and faces of the two extractions
    camera, pose = general_camera(), np.stack([fourth_pose(), general_pose(0)])
    ours, theirs = colored.raycast(camera, GENERAL_SIZE, pose=pose), plain.raycast(camera, GENERAL_SIZE, pose=pose)
    assert isinstance(ours, pds.ColorRaycast) and ours.colors.shape == (2, 48, 64, 3) and ours.colors.dtype == torch.float32
    assert torch.equal(bits(ours.depth), bits(theirs.depth)) and torch.equal(bits(ours.normals), bits(theirs.normals))
    assert int((~ours.depth.isnan()).sum()) > 1000
    bare = colored.raycast(camera, GENERAL_SIZE, pose=pose, with_colors=False, with_normals=False)
    assert bare.colors is None and bare.normals is None and torch.equal(bits(bare.depth), bits(theirs.depth))
    ours, theirs = colored.extract_points(), plain.extract_points()
    assert theirs.cloud.colors is None and ours.cloud.colors.shape == ours.cloud.points.shape
    assert ours.cloud.colors.dtype == torch.float32 and ours.cloud.points.shape[0] > 1000
    for a, b in ((ours.cloud.points, theirs.cloud.points), (ours.normals, theirs.normals)):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(ours.cloud.index, theirs.cloud.index) and torch.equal(ours.cloud.offsets, theirs.cloud.offsets)
    assert colored.extract_points(with_colors=False).cloud.colors is None
    ours, theirs = colored.extract_mesh(), plain.extract_mesh()
    assert theirs.mesh.colors is None and ours.mesh.colors.shape == ours.mesh.points.shape and ours.mesh.face_count() > 1000
    for a, b in ((ours.mesh.points, theirs.mesh.points), (ours.normals, theirs.normals)):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(ours.mesh.index, theirs.mesh.index) and torch.equal(ours.mesh.faces, theirs.mesh.faces)
    assert ours.mesh.host_offsets() == theirs.mesh.host_offsets()
    assert ours.mesh.host_face_offsets() == theirs.mesh.host_face_offsets()
    # the axis edges of the mesh carry the colours of the points (d = 1, 2, 4 <-> a = 0, 1, 2), bit for bit
    points = colored.extract_points()
    d = ours.mesh.index % 7 + 1
    axis = (d == 1) | (d == 2) | (d == 4)
    assert int(axis.sum()) == points.cloud.points.shape[0]
    assert torch.equal(bits(ours.mesh.colors[axis]), bits(points.cloud.colors))


# ------------------------------------------------------------------------------------------------ 2. known answers
def test_known_answers_are_exact(dev):
    case = general_case()
    camera = general_camera()
    value = (255.0, 1.0, 100.0)
    for layout in (0, 1):
        picture = np.zeros((48, 64, 3), dtype=np.uint8)
        picture[...] = value
        image = picture if layout == 1 else np.ascontiguousarray(picture.transpose(2, 0, 1)).astype(np.float32)
        colored, _ = volumes(dev, max_weight=3.0)
        d, image = put(dev, case['disparity'][None]), put(dev, image[None])
        expected = torch.tensor(value, device=dev)
        for frame in range(5):   # once, up to max_weight = 3 and beyond it
            colored.integrate(d, case['matrix'], pose=case['pose'], image=image)
            seen = colored.weight > 0
            assert int(seen.sum()) > 8000 and float(colored.weight.max()) == min(frame + 1.0, 3.0)
            assert bool((colored.color[seen] == expected).all()) and bool((colored.color[~seen] == 0.0).all()), (layout, frame)
        surface, mesh = colored.extract_points(), colored.extract_mesh()
        assert surface.cloud.colors.shape[0] > 1000 and bool((surface.cloud.colors == expected).all())
        assert mesh.mesh.colors.shape[0] > 3000 and bool((mesh.mesh.colors == expected).all())
        cast = colored.raycast(camera, GENERAL_SIZE, pose=case['pose'])
        has = ~cast.colors.isnan().any(dim=3)
        assert int(has.sum()) > 500 and bool((cast.colors[has] == expected).all())
        assert bool(cast.colors[cast.depth.isnan()].isnan().all())
    # an image that names its pixel, fused once into a fresh volume: each updated voxel holds the pixel the oracle says it
    # projects to (ambiguous voxels aside), exactly
    yy, xx = np.mgrid[0:48, 0:64]
    named = np.stack([3.0 * xx + yy, xx, yy]).astype(np.float32)
    colored, _ = volumes(dev)
    colored.integrate(put(dev, case['disparity'][None]), case['matrix'], pose=case['pose'], image=put(dev, named[None]))
    state = fresh_state(GENERAL['dims'], np.float32)
    oracle = oracle_color_integrate(np.zeros(state[0].shape + (3,), dtype=np.float32), *state, named, **case)
    got = colored.color.cpu().numpy()
    keep = oracle.updated & ~oracle.ambiguous
    px, py = oracle.pixel % 64, oracle.pixel // 64
    assert keep.sum() > 8000 and len(np.unique(oracle.pixel[keep])) > 1000
    assert np.array_equal(got[keep], np.stack([3.0 * px + py, px, py], axis=3)[keep].astype(np.float32))
    assert (got[~oracle.updated & ~oracle.ambiguous] == 0.0).all()


# ------------------------------------------------------------------------------------------------ 3. against fp64
def test_every_frame_against_fp64(dev):
    """Each frame is compared with the oracle applied to the state the GPU had before it (test_three_poses_in_sequence
    of tests/test_gpu_tsdf.py), over all voxels oracle_integrate does not mark ambiguous: its mask covers the rounding of
    (u, v) to a pixel.  On an MI355X at most 1.58 % of the projecting voxels were left out, 7318 to 10155 kept per frame,
    and the largest error was 3.09e-05 on colours up to 255: 0.612 of the bound at most."""
    largest = 0.0
    # the three frames as they are: more than 8000 voxels kept in each; and with valid, confidence and
    # weight_by_confidence on the second, which drop pixels (tests/test_gpu_tsdf.py asks more than 5000 of those frames)
    for extras, least, max_weight in ((({}, {}, {}), 8000, 64.0), (({}, {}, {}), 8000, 2.0),
                                      (sequence_extras(), 5000, 64.0), (sequence_extras(), 5000, 2.0)):
        colored, _ = volumes(dev, max_weight)
        for k in range(3):
            case, layout = general_case(k), k % 2
            image = random_image(k, layout)
            old = state_of(colored) + (colored.color.cpu().numpy(),)
            oracle = oracle_color_integrate(old[2], old[0], old[1], image, max_weight=max_weight, **case, **extras[k])
            colored.integrate(put(dev, case['disparity'][None]), case['matrix'], pose=case['pose'],
                              image=put(dev, image[None]), **on_device(dev, extras[k]))
            got = colored.color.cpu().numpy()
            keep = ~oracle.ambiguous
            left_out = float((oracle.ambiguous & oracle.projects).sum()) / float(oracle.projects.sum())
            assert left_out <= 0.05 and int((keep & oracle.updated).sum()) > least, (max_weight, k)
            error = np.abs(got.astype(np.float64) - oracle.color)
            share = float((error / np.where(oracle.bound > 0, oracle.bound, np.inf))[oracle.updated & keep].max())
            largest = max(largest, share)
            print('max_weight %g, frame %d: %.2f %% left out, %d kept, largest error %.3g, largest share of the bound %.3g'
                  % (max_weight, k, 100 * left_out, int((keep & oracle.updated).sum()),
                     error[oracle.updated & keep].max(), share))
            assert (error <= oracle.bound)[keep].all(), (max_weight, k, share)
            # a voxel that is not updated keeps its bits
            quiet = keep & ~oracle.updated
            assert np.array_equal(got.view(np.int32)[quiet], old[2].view(np.int32)[quiet]), (max_weight, k)
    print('the largest share of the bound: %.3g' % largest)


# ------------------------------------------------------------------------------------------------ 4. the gather
def gather_direct(dev, index, offsets, edges, tsdf, color, capacity, dims, fill=-7.0, spare=8):
    """The entry point on buffers of the test's own: -> colors [capacity + spare, 3] pre-filled with `fill`."""
    lib = _lib.load()
    colors = torch.full((capacity + spare, 3), fill, device=dev)
    _lib.check(lib.pds_tsdf_color_gather_fwd(_lib.ptr(index), _lib.ptr(offsets), edges, _lib.ptr(tsdf), _lib.ptr(color),
                                             _lib.ptr(colors), capacity, *dims, _lib.stream_handle(dev)),
               'pds_tsdf_color_gather_fwd')
    return colors


@pytest.mark.parametrize('dims', [(2, 1, 1), (1023, 1, 1), (1025, 1, 1), (5, 4, 3), (9, 2, 7), (17, 9, 5), (40, 36, 28)],
                         ids=lambda d: '%dx%dx%d' % d)
def test_gather_on_hand_made_volumes(dev, dims):
    origin, voxel_size = (-1.5, 0.25, 3.0), 0.03
    for min_weight, observed in ((1.0, 0.6), (0.375, 0.97)):
        tsdf, weight = random_volume(dims, sum(dims), min_weight, observed)
        color = random_colors(dims, sum(dims) + 3)
        volume = pds.ColorTsdfVolume(origin, voxel_size, dims, 0.1, device=dev)
        volume.tsdf, volume.weight, volume.color = put(dev, tsdf), put(dev, weight), put(dev, color)
        expected = oracle_extract(tsdf, weight, origin, voxel_size, min_weight)
        for edges, found in ((3, volume.extract_points(min_weight=min_weight).cloud),
                             (7, volume.extract_mesh(min_weight=min_weight).mesh)):
            where = (dims, min_weight, edges)
            index = found.index.cpu().numpy()
            count = len(index)
            if edges == 3:
                assert np.array_equal(index, expected.index), where
            else:
                assert count >= len(expected.index) and found.host_offsets() == [0, count], where
            colors, bound = oracle_gather(index, edges, tsdf, color)
            got = found.colors.cpu().numpy()
            assert got.dtype == np.float32 and got.shape == (count, 3), where
            error = np.abs(got.astype(np.float64) - colors)
            assert (error <= bound).all(), (where, float((error / bound).max(initial=0.0)))
            if dims == (40, 36, 28):
                assert count > 10000 and count % 1024 != 0 and (3 * count) % 256 != 0, where
                print('%s: %d rows, largest share of the bound %.3g' % (where, count, (error / bound).max()))
            # trim=False into a guarded buffer: the rows beyond offsets[1] are untouched; a capacity below the count
            # writes `capacity` rows and no more
            device_index = torch.cat([found.index, torch.full((5,), -3, dtype=torch.int32, device=dev)])
            whole = gather_direct(dev, device_index, found.offsets, edges, volume.tsdf, volume.color, count + 5, dims)
            assert torch.equal(bits(whole[:count]), bits(found.colors)) and bool((whole[count:] == -7.0).all()), where
            if count >= 2:
                half = gather_direct(dev, device_index, found.offsets, edges, volume.tsdf, volume.color, count // 2, dims)
                assert torch.equal(bits(half[:count // 2]), bits(found.colors[:count // 2])), where
                assert bool((half[count // 2:] == -7.0).all()), where
            none = gather_direct(dev, device_index, found.offsets, edges, volume.tsdf, volume.color, 0, dims)
            assert bool((none == -7.0).all()), where
        # through the Python surface: untrimmed buffers, an explicit capacity, and without colours
        count = len(expected.index)
        loose = volume.extract_points(min_weight=min_weight, capacity=count + 5, trim=False)
        assert loose.cloud.colors.shape == (count + 5, 3) and loose.cloud.offsets.tolist() == [0, count]
        assert torch.equal(bits(loose.cloud.colors[:count]), bits(volume.extract_points(min_weight=min_weight).cloud.colors))
        if count >= 2:
            with pytest.raises(RuntimeError, match='do not fit capacity %d' % (count // 2)):
                volume.extract_points(min_weight=min_weight, capacity=count // 2)
            cut = volume.extract_points(min_weight=min_weight, capacity=count // 2, trim=False)
            assert cut.cloud.colors.shape == (count // 2, 3) and cut.cloud.offsets.tolist() == [0, count]
    volume.reset()
    empty = volume.extract_points(min_weight=0.0)
    assert empty.cloud.colors.shape == (0, 3) and empty.cloud.offsets.tolist() == [0, 0]
    assert float(volume.color.abs().max()) == 0.0 and volume.extract_mesh(min_weight=0.0).mesh.colors.shape == (0, 3)


# ------------------------------------------------------------------------------------------------ 5. the render
def render_direct(dev, volume, weight, depth, poses, min_weight):
    """The entry point on a depth map and weights of the test's choice -> colors [B, H, W, 3]."""
    lib = _lib.load()
    batch, height, width = depth.shape
    rows = volume.rays(poses, batch).astype(np.float32)
    colors = torch.full((batch, height, width, 3), -7.0, device=dev)
    _lib.check(lib.pds_tsdf_color_render_fwd(
        _lib.ptr(weight), _lib.ptr(volume.color), *volume.dims, (ctypes.c_float * (12 * batch))(*rows[:, :12].reshape(-1).tolist()),
        (ctypes.c_float * 5)(*[float(np.float32(v)) for v in general_camera()]), min_weight, _lib.ptr(depth),
        _lib.ptr(colors), batch, height, width, _lib.stream_handle(dev)), 'pds_tsdf_color_render_fwd')
    return colors


def test_render_against_fp64(dev):
    poses = np.stack([fourth_pose(), general_pose(0)])
    for min_weight, observed in RENDER_CASES:
        tsdf, weight, color = render_scene(min_weight, observed)
        volume = pds.ColorTsdfVolume(RANDOM['origin'], RANDOM['voxel_size'], RANDOM_DIMS, RANDOM['truncation'], device=dev)
        volume.tsdf, volume.weight, volume.color = put(dev, tsdf), put(dev, weight), put(dev, color)
        cast = volume.raycast(general_camera(), GENERAL_SIZE, pose=poses, min_weight=min_weight)
        depth, got = cast.depth.cpu().numpy(), cast.colors.cpu().numpy()
        assert bool(cast.colors[cast.depth.isnan()].isnan().all())   # a pixel with NaN depth has NaN colour
        for b in range(2):
            oracle = render_oracle(color, weight, depth[b], poses[b], min_weight)
            has = ~np.isnan(depth[b])
            assert has.sum() > 500 and float(oracle.undecided[has].mean()) <= 0.05, (observed, b)
            compared, share = check_render(got[b], oracle, (observed, b))
            print('render %g, pose %d: %d colours compared, largest share of the bound %.3g' % (observed, b, compared, share))
            assert compared > 400
        if observed == 1.0:
            # the depth of the fully observed volume against the weights of a partly observed one: where a corner of the
            # cell is unobserved there is no colour, and nowhere else
            holed = holed_weight()
            colors = render_direct(dev, volume, put(dev, holed), cast.depth, poses, 1.0).cpu().numpy()
            for b in range(2):
                oracle = render_oracle(color, holed, depth[b], poses[b], 1.0)
                has = ~np.isnan(depth[b])
                assert float(oracle.undecided[has].mean()) <= 0.05 and (has & oracle.absent & ~oracle.undecided).sum() > 400
                compared, share = check_render(colors[b], oracle, ('holed', b))
                print('render, holed, pose %d: %d colours compared, largest share of the bound %.3g' % (b, compared, share))
                assert compared > 200
    # seventeen poses: two launches; and a volume without cells has no colour
    many = np.stack([general_pose(k % 3) for k in range(17)])
    cast = volume.raycast(general_camera(), GENERAL_SIZE, pose=many, min_weight=min_weight)
    assert torch.equal(bits(cast.colors[16]), bits(cast.colors[1])) and torch.equal(bits(cast.colors[3]), bits(cast.colors[0]))
    flat = pds.ColorTsdfVolume((0.0, 0.0, 0.5), 0.02, (5, 4, 1), 0.06, device=dev)
    depth = torch.full((1, 5, 7), 0.51, device=dev)
    assert bool(render_direct(dev, flat, flat.weight, depth, fourth_pose(), 0.0).isnan().all())


# ------------------------------------------------------------------------------------------------ 6. housekeeping
def colored_state(volume):
    return [bits(volume.tsdf).clone(), bits(volume.weight).clone(), bits(volume.color).clone()]


def products(volume, poses):
    surface, mesh = volume.extract_points(), volume.extract_mesh()
    cast = volume.raycast(general_camera(), GENERAL_SIZE, pose=poses)
    return [bits(surface.cloud.colors), bits(mesh.mesh.colors), bits(cast.colors)]


def test_the_same_bits_on_every_run_and_stream(dev):
    frames = put(dev, np.stack([general_disparity(k) for k in range(2)]))
    images = put(dev, np.stack([random_image(k, 1) for k in range(2)]))
    poses = np.stack([general_pose(k) for k in range(2)])
    Q = general_case()['matrix']
    run = (lambda: volumes(dev)[0].integrate(frames, Q, pose=poses, image=images))
    first = run()
    state, made = colored_state(first), products(first, poses)
    assert made[0].shape[0] > 1000 and made[1].shape[0] > 3000
    again = run()
    assert all(torch.equal(a, b) for a, b in zip(colored_state(again), state))
    assert all(torch.equal(a, b) for a, b in zip(products(again, poses), made))
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        aside = run()
        other = products(aside, poses)
    stream.synchronize()
    torch.cuda.current_stream(dev).wait_stream(stream)
    assert all(torch.equal(a, b) for a, b in zip(colored_state(aside), state))
    assert all(torch.equal(a, b) for a, b in zip(other, made))


def test_unaligned_state_agrees_and_guards_stay(dev):
    """The pattern of test_unaligned_state_and_outputs_agree_and_guards_stay (tests/test_gpu_tsdf.py).  With tsdf and weight
    `lead` elements behind a 16-byte boundary the colour of a quad is 16-byte aligned iff color sits 3 * lead elements
    (mod 4) behind one: both cases are taken, and the scalar walk of tsdf and weight with either colour form."""
    frames = put(dev, np.stack([general_disparity(k) for k in range(2)]))
    images = {1: put(dev, np.stack([random_image(k, 1) for k in range(2)])),
              0: put(dev, np.stack([random_image(k, 0) for k in range(2)]))}
    poses = np.stack([general_pose(k) for k in range(2)])
    Q = general_case()['matrix']
    rng = np.random.RandomState(5)
    confidence = put(dev, (0.1 + 0.9 * rng.rand(2, 48, 64)).astype(np.float32))
    for dims in ((40, 36, 28), (33, 7, 9), (1023, 3, 1)):
        geometry = dict(origin=(-0.01 * dims[0], -0.01 * dims[1], 0.35), voxel_size=0.02, dims=dims, truncation=0.06)
        for layout, kw in ((1, {}), (0, dict(confidence=confidence, weight_by_confidence=True))):
            aligned = pds.ColorTsdfVolume(device=dev, **geometry).integrate(frames, Q, pose=poses, image=images[layout], **kw)
            assert bool((aligned.weight > 0).any()) and float(aligned.color.max()) > 0
            # (tsdf, weight, color) in elements behind a boundary.  (1, 1, 3) and (3, 3, 1): one grid for all three, the
            # colour in 16-byte accesses; (1, 1, 0) and (2, 2, 3): tsdf and weight in 16 bytes, the colour voxel by voxel;
            # (1, 0, 0): tsdf and weight disagree, the colour of the quads [4 q, 4 q + 4) is aligned; (0, 2, 1): nothing is
            for lead_t, lead_w, lead_c in ((1, 1, 3), (3, 3, 1), (1, 1, 0), (2, 2, 3), (1, 0, 0), (0, 2, 1)):
                volume = pds.ColorTsdfVolume(device=dev, **geometry)
                tsdf_buffer, tsdf_view = guarded(volume.tsdf, lead_t, -7.0)
                weight_buffer, weight_view = guarded(volume.weight, lead_w, -9.0)
                color_buffer, color_view = guarded(volume.color, lead_c, -11.0)
                volume.tsdf, volume.weight, volume.color = tsdf_view, weight_view, color_view
                assert volume.tsdf.data_ptr() % 16 == 4 * lead_t and volume.color.data_ptr() % 16 == 4 * lead_c
                image = images[layout]
                volume.integrate(off_by_one(frames), Q, pose=poses, image=off_by_one(image) if layout == 0 else image,
                                 **{k: off_by_one(v) if isinstance(v, torch.Tensor) else v for k, v in kw.items()})
                where = (dims, layout, lead_t, lead_w, lead_c)
                assert same_state(volume, aligned) and torch.equal(bits(volume.color), bits(aligned.color)), where
                count = volume.tsdf.numel()
                assert guards_untouched(tsdf_buffer, lead_t, count, -7.0), where
                assert guards_untouched(weight_buffer, lead_w, count, -9.0), where
                assert guards_untouched(color_buffer, lead_c, 3 * count, -11.0), where
        # the gather and the render from the unaligned state into unaligned outputs between guards
        surface = aligned.extract_mesh()
        count = surface.mesh.points.shape[0]
        if count == 0:
            continue
        lib = _lib.load()
        cast = aligned.raycast(general_camera(), GENERAL_SIZE, pose=poses) if min(dims) >= 2 else None
        for lead in range(4):
            tsdf_buffer, tsdf_view = guarded(aligned.tsdf, lead, -7.0)
            weight_buffer, weight_view = guarded(aligned.weight, (lead + 1) % 4, -9.0)
            color_buffer, color_view = guarded(aligned.color, (lead + 2) % 4, -11.0)
            index_buffer, index = guarded(surface.mesh.index, (lead + 3) % 4, -5)
            out_buffer, out = guarded(torch.zeros(3 * count, device=dev), lead, -13.0)
            _lib.check(lib.pds_tsdf_color_gather_fwd(
                _lib.ptr(index), _lib.ptr(surface.mesh.offsets), 7, _lib.ptr(tsdf_view), _lib.ptr(color_view), _lib.ptr(out),
                count, *dims, _lib.stream_handle(dev)), 'pds_tsdf_color_gather_fwd')
            torch.cuda.synchronize()
            assert torch.equal(bits(out), bits(surface.mesh.colors.reshape(-1))), (dims, lead)
            assert guards_untouched(out_buffer, lead, 3 * count, -13.0), (dims, lead)
            if cast is not None:
                depth_buffer, depth = guarded(cast.depth, (lead + 1) % 4, NAN)
                rows = aligned.rays(poses, 2).astype(np.float32)
                pixels = cast.depth.numel()
                image_buffer, image = guarded(torch.zeros(3 * pixels, device=dev), (lead + 3) % 4, -13.0)
                _lib.check(lib.pds_tsdf_color_render_fwd(
                    _lib.ptr(weight_view), _lib.ptr(color_view), *dims,
                    (ctypes.c_float * 24)(*rows[:, :12].reshape(-1).tolist()),
                    (ctypes.c_float * 5)(*[float(np.float32(v)) for v in general_camera()]), 1.0, _lib.ptr(depth),
                    _lib.ptr(image), 2, 48, 64, _lib.stream_handle(dev)), 'pds_tsdf_color_render_fwd')
                torch.cuda.synchronize()
                assert torch.equal(bits(image), bits(cast.colors.reshape(-1))), (dims, lead)
                assert guards_untouched(image_buffer, (lead + 3) % 4, 3 * pixels, -13.0), (dims, lead)
            # the state is read only
            assert torch.equal(bits(color_view), bits(aligned.color)) and torch.equal(bits(tsdf_view), bits(aligned.tsdf))
            assert guards_untouched(color_buffer, (lead + 2) % 4, 3 * aligned.tsdf.numel(), -11.0), (dims, lead)
            assert guards_untouched(tsdf_buffer, lead, aligned.tsdf.numel(), -7.0), (dims, lead)
            assert guards_untouched(weight_buffer, (lead + 1) % 4, aligned.tsdf.numel(), -9.0), (dims, lead)


def test_the_three_kernels_ran(dev):
    lib = _lib.load()
    frames = put(dev, np.stack([general_disparity(k) for k in range(2)]))
    images = put(dev, np.stack([random_image(k, 1) for k in range(2)]))
    poses = np.stack([general_pose(k) for k in range(2)])
    Q = general_case()['matrix']
    volume, _ = volumes(dev)
    depth = (48 * 64 + 1023) // 1024
    voxels = 40 * 36 * 28
    groups = min(((voxels + 3) // 4 + 255) // 256, MAX_GROUPS)
    integrate = (lambda: volume.integrate(frames, Q, pose=poses, image=images))
    assert probe(lib, 'tsdf_color_integrate', integrate) == [groups, groups]
    assert probe(lib, 'tsdf_', integrate) == [depth, groups, depth, groups]
    assert probe(lib, 'tsdf_integrate', integrate) == []   # (the plain kernel does not run for a colour volume)
    for edges, extract in ((3, lambda: volume.extract_points(trim=False, capacity=4096)),
                           (7, lambda: volume.extract_mesh(trim=False, capacity=4096, face_capacity=8192))):
        assert probe(lib, 'tsdf_color_gather', extract) == [3 * 4096 // 256], edges
    cast = (lambda: volume.raycast(general_camera(), GENERAL_SIZE, pose=poses))
    assert probe(lib, 'tsdf_color_render', cast) == [2 * 3 * 4]
    assert probe(lib, 'tsdf_raycast', cast) == [2 * 3 * 4]
    many = np.stack([general_pose(k % 3) for k in range(17)])
    assert probe(lib, 'tsdf_color_render', lambda: volume.raycast(general_camera(), GENERAL_SIZE, pose=many)) == [16 * 12, 12]
    assert probe(lib, 'tsdf_color', lambda: volume.extract_points(with_colors=False)) == []


def test_through_the_rig_to_a_coloured_ply(dev, tmp_path):
    torch.manual_seed(0)
    net = pds.PdsNetwork.default(63).eval().to(dev)
    left, right = rig_pair(dev)
    rig = simple_rig(256, 128)
    r = rig.reconstruct(net, left, right, max_difference=1.0)
    depth = rig.reproject(r.disparity, valid=r.valid, depth_only=True)
    near = float(depth[~depth.isnan()].median())
    geometry = dict(origin=(-0.5 * near, -0.3 * near, 0.7 * near), voxel_size=near / 64, dims=(64, 40, 40),
                    truncation=near / 16)
    volume = rig.color_tsdf_volume(device=dev, **geometry)
    assert isinstance(volume, pds.ColorTsdfVolume)
    plain = rig.tsdf_volume(device=dev, **geometry)
    for k in (1, 2):
        assert rig.integrate_color(volume, r.disparity, r.left_image, general_pose(k), r.valid) is volume
        rig.integrate(plain, r.disparity, general_pose(k), r.valid)
    assert same_state(volume, plain) and float(volume.weight.max()) == 2.0
    seen = volume.weight > 0
    low, high = float(r.left_image.min()), float(r.left_image.max())
    assert int(seen.sum()) > 100 and float(volume.color[seen].min()) >= low - 1e-3 and float(volume.color[seen].max()) <= high + 1e-3
    surface = volume.extract_mesh()
    count, faces = surface.mesh.points.shape[0], surface.mesh.face_count()
    # (a network of random weights gives a ragged surface: many vertices, few of them joined into faces)
    assert count > 100 and faces >= 1 and surface.mesh.colors.shape == (count, 3)
    path = str(tmp_path / 'model.ply')
    surface.mesh.save_ply(path, normals=surface.normals)
    raw = open(path, 'rb').read()
    header, body = raw.split(b'end_header\n', 1)
    assert b'property uchar red\nproperty uchar green\nproperty uchar blue\n' in header
    assert b'element vertex %d\n' % count in header and b'element face %d\n' % faces in header
    record = np.dtype([(n, '<f4') for n in ('x', 'y', 'z', 'nx', 'ny', 'nz')] + [(n, 'u1') for n in ('red', 'green', 'blue')])
    assert len(body) == count * record.itemsize + faces * 13
    vertices = np.frombuffer(body[:count * record.itemsize], dtype=record)
    assert np.array_equal(vertices['x'], surface.mesh.points[:, 0].cpu().numpy())
    expected = np.rint(np.clip(np.nan_to_num(surface.mesh.colors.cpu().numpy().astype(np.float64)), 0, 255)).astype(np.uint8)
    assert np.array_equal(np.stack([vertices['red'], vertices['green'], vertices['blue']], axis=1), expected)
    triangles = np.frombuffer(body[count * record.itemsize:], dtype=np.dtype([('n', 'u1'), ('v', '<i4', (3,))]))
    assert (triangles['n'] == 3).all() and np.array_equal(triangles['v'], surface.mesh.faces.cpu().numpy())
    # the rig's raycast forwards with_colors
    cast = rig.raycast(volume, general_pose(1))
    assert isinstance(cast, pds.ColorRaycast) and cast.colors.shape == (1, 128, 256, 3)
    assert rig.raycast(volume, general_pose(1), with_colors=False).colors is None
