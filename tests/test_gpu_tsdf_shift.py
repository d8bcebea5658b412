"""GPU (-m gpu): the rolling volume (TsdfVolume.shift / follow, ColorTsdfVolume.shift; pds_tsdf_shift_fwd,
pds_tsdf_extract_leaving_fwd).

A shift is a copy, so everything here is compared bit for bit: the shifted state with the numpy oracle of
tests/test_tsdf_shift_host.py (held to hand-written answers there), the leaving rows with the rows of extract_points
that the oracle's predicate on ``index`` selects.  tsdf_shift works on quads of four voxels and the extraction on tiles
of 1024, so the dims sit around both; the state tensors are views at every element offset of a 16-byte granule, in
buffers that end where the view ends."""
import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib
from tests.test_gpu_tsdf import bits, guarded, guards_untouched, probe, put, random_volume
from tests.test_register_depth_host import EPS
from tests.test_tsdf_color_host import random_colors, random_image
from tests.test_tsdf_host import GENERAL, TILE, WALL, camera_of, general_case, wall_volume
from tests.test_tsdf_shift_host import flat_offset, oracle_leaves, oracle_shift, pose_at

pytestmark = pytest.mark.gpu

DIMS = [(1, 1, 1), (5, 3, 2), (33, 7, 9), (257, 3, 5), (64, 5, 4)]
SHIFT_GROUPS = 2048   # csrc/common.hpp: kTsdfShiftMaxGroups


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def deltas_of(dims):
    every = [(0, 0, 0), (3, -2, 1), (4, 0, 0), (-8, 0, 1)]
    for axis in range(3):
        for d in (1, -1, dims[axis] - 1, dims[axis], dims[axis] + 5):
            every.append(tuple(d if m == axis else 0 for m in range(3)))
    every.append((-dims[0], 0, 0))
    return [d for k, d in enumerate(every) if d not in every[:k]]


def random_state(dims, seed, color):
    """float32 tsdf, weight (and colour) of random values with NaNs of several payloads, -0.0 and both infinities among
    them."""
    nx, ny, nz = dims
    rng = np.random.RandomState(seed)
    odd = np.array([0x7fc00123, 0xffc00001, 0x7f800001, 0x80000000, 0x7f800000, 0xff800000], dtype=np.uint32)
    out = []
    for shape in ((nz, ny, nx), (nz, ny, nx)) + (((nz, ny, nx, 3),) if color else ()):
        a = rng.standard_normal(shape).astype(np.float32)
        special = rng.rand(*shape) < 0.1
        a.view(np.uint32)[special] = rng.choice(odd, int(special.sum()))
        out.append(a)
    return out + ([] if color else [None])


def view_at(dev, a, lead):
    """`a` on the device as a view `lead` elements into a buffer that ends where the view ends -> (buffer, view)."""
    buffer = torch.empty(lead + a.size, dtype=torch.float32, device=dev)
    buffer[:lead] = -7.0
    view = buffer[lead:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 * (lead % 4) and view.is_contiguous()
    return buffer, view


def make_volume(dev, dims, color, **kw):
    cls = pds.ColorTsdfVolume if color else pds.TsdfVolume
    return cls(kw.pop('origin', (-0.3, 0.1, 0.7)), kw.pop('voxel_size', 0.05), dims, kw.pop('truncation', 0.15),
               device=dev, **kw)


def set_state(volume, views):
    volume.tsdf, volume.weight = views[0], views[1]
    if views[2] is not None:
        volume.color = views[2]


def state(volume):
    return volume.tsdf, volume.weight, getattr(volume, 'color', None)


def equal_bits(got, want, where):
    for name, g, w in zip(('tsdf', 'weight', 'color'), got, want):
        assert (g is None) == (w is None), (where, name)
        if g is not None:
            w = w if isinstance(w, torch.Tensor) else torch.from_numpy(w).to(g.device)
            assert g.shape == w.shape and torch.equal(bits(g), bits(w)), (where, name)


# ------------------------------------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize('color', [False, True], ids=['plain', 'coloured'])
@pytest.mark.parametrize('dims', DIMS, ids=lambda d: '%dx%dx%d' % d)
def test_shift_bit_for_bit(dev, dims, color):
    host = random_state(dims, sum(dims), color)
    volume = make_volume(dev, dims, color)
    # leads of tsdf, weight, colour: every offset of a granule with all agreeing, then tsdf and weight disagreeing
    for leads in ((0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 0, 2), (0, 2, 1), (3, 1, 0), (0, 0, 1)):
        held = [None if a is None else view_at(dev, a, lead) for a, lead in zip(host, leads)]
        views = [None if h is None else h[1] for h in held]
        for delta in deltas_of(dims):
            set_state(volume, views)
            before = volume.offset
            assert volume.shift(delta) is None
            assert volume.offset == tuple(o + d for o, d in zip(before, delta))
            got = state(volume)
            where = (dims, color, leads, delta)
            equal_bits(got, oracle_shift(*host, delta), where)
            if delta != (0, 0, 0):
                assert all(g is None or g.data_ptr() != v.data_ptr() for g, v in zip(got, views)), where   # fresh tensors
        # the inputs are what they were, and so is what lies before them
        equal_bits(views, host, (dims, color, leads, 'inputs'))
        assert all(h is None or bool((h[0][:lead] == -7.0).all()) for h, lead in zip(held, leads))
    volume.reset()
    assert volume.offset != (0, 0, 0) and bool((volume.weight == 0).all())   # reset() empties the box where it stands


@pytest.mark.parametrize('color', [False, True], ids=['plain', 'coloured'])
def test_shift_into_unaligned_outputs_between_guards(dev, color):
    """The entry point itself, with outputs at every misalignment: one grid of quads fits both (all three) outputs, or
    none does and the launch goes voxel by voxel.  Nothing outside the outputs is written."""
    lib = _lib.load()
    for dims in ((33, 7, 9), (5, 3, 2)):
        host = random_state(dims, 11 + dims[0], color)
        inputs = [None if a is None else view_at(dev, a, lead)[1] for a, lead in zip(host, (2, 2, 1))]
        # (leads of tsdf_out, weight_out, color_out): quads fit (the colour's need (lead_c + lead) % 4 == 0), or not
        for leads in ((0, 0, 0), (1, 1, 3), (2, 2, 2), (3, 3, 1), (1, 1, 1), (1, 0, 0), (0, 2, 0), (0, 0, 2)):
            for delta in ((0, 0, 0), (1, 0, 0), (3, -2, 1), (4, 0, 0), (-8, 0, 1), (0, 0, dims[2])):
                held = [None if a is None else guarded(torch.zeros(a.shape, device=dev), lead, -3.0)
                        for a, lead in zip(host, leads)]
                pointer = (lambda t: None if t is None else _lib.ptr(t))
                _lib.check(lib.pds_tsdf_shift_fwd(
                    *[pointer(t) for t in inputs], *[pointer(None if h is None else h[1]) for h in held], *delta, *dims,
                    _lib.stream_handle(dev)), 'pds_tsdf_shift_fwd')
                where = (dims, color, leads, delta)
                equal_bits([None if h is None else h[1] for h in held], oracle_shift(*host, delta), where)
                for h, a, lead in zip(held, host, leads):
                    assert h is None or guards_untouched(h[0], lead, a.size, -3.0), where
        equal_bits(inputs, host, (dims, color, 'inputs'))


# ------------------------------------------------------------------------------------------------ 2. composition
@pytest.mark.parametrize('dims', [(33, 7, 9), (64, 5, 4)], ids=lambda d: '%dx%dx%d' % d)
def test_shifts_compose(dev, dims):
    host = random_state(dims, 3, True)
    host[1] = np.abs(np.nan_to_num(host[1])) + 1.0   # (a weight that is never 0: the voxels that stayed are marked)
    on_device = [put(dev, a) for a in host]
    for a, b in (((3, -2, 1), (-8, 0, 1)), ((1, 1, 1), (2, -3, 0)), ((4, 0, 0), (-4, 0, 0)), ((0, 3, -2), (0, -3, 2)),
                 ((-5, 2, 3), (5, -2, -3))):
        two = make_volume(dev, dims, True)
        set_state(two, on_device)
        two.shift(a)
        two.shift(b)
        total = tuple(x + y for x, y in zip(a, b))
        one = make_volume(dev, dims, True)
        set_state(one, on_device)
        one.shift(total)
        assert two.offset == one.offset == total and np.array_equal(two.origin, one.origin)
        equal_bits(state(two), oracle_shift(*oracle_shift(*host, a), b), (dims, a, b))
        stayed = two.weight != 0
        assert bool(stayed.any()) and bool((one.weight != 0)[stayed].all())
        for got, want in zip(state(two), state(one)):
            assert torch.equal(bits(got)[stayed], bits(want)[stayed]), (dims, a, b)
        if total == (0, 0, 0):
            # there and back: the interior is restored, the rim holds the empty state
            for got, want, empty in zip(state(two), on_device, (1.0, 0.0, 0.0)):
                assert torch.equal(bits(got)[stayed], bits(want)[stayed]), (dims, a)
                assert bool((got[~stayed] == empty).all()) and bool((~stayed).any()), (dims, a)
            nx, ny, nz = dims
            inside = np.zeros((nz, ny, nx), dtype=bool)
            inside[max(0, a[2]):nz - max(0, -a[2]), max(0, a[1]):ny - max(0, -a[1]), max(0, a[0]):nx - max(0, -a[0])] = True
            assert np.array_equal(stayed.cpu().numpy(), inside), (dims, a)


# ------------------------------------------------------------------------------------------------ 3. equivariance
def general_volume(dev, origin=None):
    return pds.ColorTsdfVolume(GENERAL['origin'] if origin is None else origin, GENERAL['voxel_size'], GENERAL['dims'],
                               GENERAL['truncation'], device=dev)


def integrate_general(dev, volume, k):
    case = general_case(k)
    return volume.integrate(put(dev, case['disparity'][None]), case['matrix'], pose=case['pose'],
                            image=put(dev, random_image(k, 1)[None]))


@pytest.fixture(scope='module')
def general_state(dev):
    """The coloured GENERAL volume after its first frame, as numpy arrays (never changed)."""
    volume = integrate_general(dev, general_volume(dev), 0)
    return tuple(t.cpu().numpy() for t in state(volume))


def test_shift_then_integrate_is_integrate_at_the_shifted_origin(dev, general_state):
    for delta in ((4, -3, 2), (-8, 0, 1), (1, 0, 0)):
        moved = general_volume(dev)
        set_state(moved, [put(dev, a) for a in general_state])
        moved.shift(delta)
        fresh = general_volume(dev, origin=moved.origin)
        set_state(fresh, [put(dev, a) for a in oracle_shift(*general_state, delta)])
        assert np.array_equal(fresh.origin, np.array(GENERAL['origin']) + GENERAL['voxel_size'] * np.array(delta))
        integrate_general(dev, moved, 1)
        integrate_general(dev, fresh, 1)
        equal_bits(state(moved), state(fresh), delta)
        assert not torch.equal(bits(moved.weight), bits(put(dev, oracle_shift(*general_state, delta)[1])))   # it did integrate
        case = general_case(1)
        a = moved.raycast(camera_of(case['matrix']), (GENERAL['width'], GENERAL['height']), pose=case['pose'])
        b = fresh.raycast(camera_of(case['matrix']), (GENERAL['width'], GENERAL['height']), pose=case['pose'])
        assert int((~a.depth.isnan()).sum()) > 100
        for x, y in zip(a, b):
            assert torch.equal(bits(x), bits(y)), delta
        a, b = moved.extract_points(), fresh.extract_points()
        assert a.cloud.points.shape[0] > 500 and torch.equal(a.cloud.index, b.cloud.index)
        for x, y in ((a.cloud.points, b.cloud.points), (a.cloud.colors, b.cloud.colors), (a.normals, b.normals)):
            assert torch.equal(bits(x), bits(y)), delta


# ------------------------------------------------------------------------------------------------ 4. leaving: a partition
def leaving_cases(general_state):
    yield 'general', GENERAL['dims'], general_state, 1.0
    for dims, min_weight, observed in (((33, 7, 9), 1.0, 0.6), ((64, 5, 4), 0.375, 0.97), ((257, 3, 5), 1.0, 0.6)):
        tsdf, weight = random_volume(dims, 5 + dims[0], min_weight, observed)
        yield 'random %dx%dx%d' % dims, dims, (tsdf, weight, random_colors(dims, 2)), min_weight


def test_leaving_rows_and_the_rest_partition_the_surface(dev, general_state):
    for name, dims, host, min_weight in leaving_cases(general_state):
        on_device = [put(dev, a) for a in host]
        old = make_volume(dev, dims, True)
        set_state(old, on_device)
        full = old.extract_points(min_weight=min_weight)
        index = full.cloud.index.cpu().numpy()
        count = len(index)
        assert count > (1000 if name == 'general' else 50), name
        for delta in ((1, 0, 0), (0, -1, 0), (0, 0, 2), (3, -2, 1), (-8, 0, 1), (dims[0], 0, 0), (0, 0, 0)):
            where = (name, delta)
            volume = make_volume(dev, dims, True)
            set_state(volume, on_device)
            leaving = volume.shift(delta, leaving=True, min_weight=min_weight)
            leaves = oracle_leaves(index, dims, delta)
            rows = torch.from_numpy(np.flatnonzero(leaves)).to(dev)
            assert leaving.cloud.offsets.tolist() == [0, int(leaves.sum())], where
            assert leaving.cloud.index.dtype == torch.int32 and torch.equal(leaving.cloud.index, full.cloud.index[rows]), where
            assert torch.equal(bits(leaving.cloud.points), bits(full.cloud.points[rows])), where
            assert torch.equal(bits(leaving.normals), bits(full.normals[rows])), where
            assert torch.equal(bits(leaving.cloud.colors), bits(full.cloud.colors[rows])), where
            if delta == (dims[0], 0, 0):
                assert leaves.all()
            if delta == (3, -2, 1):
                assert leaves.any() and not leaves.all(), where
            # what extract_points finds afterwards is exactly the rest, in the new numbering
            equal_bits(state(volume), oracle_shift(*host, delta), where)
            rest = volume.extract_points(min_weight=min_weight).cloud.index.cpu().numpy().astype(np.int64)
            assert np.array_equal(rest + 3 * flat_offset(dims, delta), index[~leaves]), where
        # trim=False with a capacity below the count: the true count in offsets, the first rows as they are
        delta = (3, -2, 1)
        leaves = np.flatnonzero(oracle_leaves(index, dims, delta))
        capacity = len(leaves) // 2
        assert capacity >= 1, name
        volume = make_volume(dev, dims, True)
        set_state(volume, on_device)
        cut = volume.shift(delta, leaving=True, min_weight=min_weight, capacity=capacity, trim=False)
        rows = torch.from_numpy(leaves[:capacity]).to(dev)
        assert cut.cloud.offsets.tolist() == [0, len(leaves)] and cut.cloud.points.shape == (capacity, 3), name
        assert torch.equal(cut.cloud.index, full.cloud.index[rows]) and torch.equal(bits(cut.cloud.points), bits(full.cloud.points[rows]))
        assert torch.equal(bits(cut.normals), bits(full.normals[rows])) and torch.equal(bits(cut.cloud.colors), bits(full.cloud.colors[rows]))
        assert volume.offset == delta
        # trim=True refuses it, as extract_points does, BEFORE anything moves; without normals and colours
        volume = make_volume(dev, dims, True)
        set_state(volume, on_device)
        with pytest.raises(RuntimeError, match='do not fit capacity %d' % capacity):
            volume.shift(delta, leaving=True, min_weight=min_weight, capacity=capacity)
        assert volume.offset == (0, 0, 0) and all(a.data_ptr() == b.data_ptr() for a, b in zip(state(volume), on_device))
        bare = volume.shift(delta, leaving=True, min_weight=min_weight, with_normals=False, with_colors=False)
        assert bare.normals is None and bare.cloud.colors is None and bare.cloud.points.shape == (len(leaves), 3)
        # a plain volume gives the same rows without colours
        plain = make_volume(dev, dims, False)
        set_state(plain, on_device[:2] + [None])
        got = plain.shift(delta, leaving=True, min_weight=min_weight)
        rows = torch.from_numpy(leaves).to(dev)
        assert got.cloud.colors is None and torch.equal(bits(got.cloud.points), bits(full.cloud.points[rows]))
        assert torch.equal(bits(got.normals), bits(full.normals[rows]))


# ------------------------------------------------------------------------------------------------ 5. every edge once
def test_a_rig_passing_a_wall_hands_out_every_edge_exactly_once(dev):
    dims = (24, 8, 8)                      # 3 m along x; the path below is 3.75 m and the image sees 1 m of the wall
    origin, Q = wall_volume(dims)
    vs, frames, stride = WALL['voxel_size'], 6, 0.75
    d = put(dev, np.full((1, WALL['height'], WALL['width']), WALL['disparity'], dtype=np.float32))
    poses = [pose_at((stride * k, 0.0, 0.0)) for k in range(frames)]
    volume = pds.TsdfVolume(origin, vs, dims, WALL['truncation'], device=dev)
    edges, points, shifts = [], [], 0

    def collect(surface, offset):
        index = surface.cloud.index.cpu().numpy().astype(np.int64)
        v, a = index // 3, index % 3
        at = np.stack([v % dims[0], (v // dims[0]) % dims[1], v // (dims[0] * dims[1])], axis=1) + np.array(offset)
        edges.extend(map(tuple, np.concatenate([at, a[:, None]], axis=1).tolist()))
        points.append(surface.cloud.points.cpu().numpy().astype(np.float64))

    for pose in poses:
        offset = volume.offset
        # (the camera stands in front of the box, 7.5 voxels before its near face: an anchor that keeps z where it is)
        leaving = volume.follow(pose, anchor=(0.5, 0.5, -0.9375), step=4, leaving=True)
        assert (volume.offset[0] - offset[0]) % 4 == 0 and volume.offset[1:] == (0, 0)
        shifts += volume.offset != offset
        collect(leaving, offset)
        volume.integrate(d, Q, pose=pose)
    assert shifts >= 4 and volume.offset[0] >= 24   # the box has left the place where it began
    collect(volume.extract_points(), volume.offset)
    points = np.concatenate(points)
    assert len(edges) == len(points) > 150 and len(set(edges)) == len(edges)   # no edge twice
    # the whole path in x: the image sees +- 0.43 m of the wall around each camera, and no column of voxels in between
    # is missing
    assert points[:, 0].min() < -0.375 and points[:, 0].max() > stride * (frames - 1) + 0.375
    columns = sorted({e[0] for e in edges})
    assert columns == list(range(columns[0], columns[-1] + 1)) and len(columns) >= 34
    assert all(e[3] == 2 and e[2] == 1 for e in edges)   # the crossing between layers 1 and 2, along z
    # z: the wall, within the bound test_wall_known_answer puts on the two layers' tsdf (EPS (Z + z_c) / truncation, and
    # 1e-6 per further frame), carried through r = t1 / (t1 - t2), |t1 - t2| = 1, and the point's own rounding
    layer_z = WALL['z0'] + (np.arange(1, 3) + 0.5) * vs
    bound = (EPS * (WALL['depth'] + layer_z) / WALL['truncation'] + 1e-6 * (frames - 1)).sum()
    assert np.abs(points[:, 2] - WALL['depth']).max() <= vs * 2.0 * bound + 4 * np.spacing(np.float32(WALL['depth']))
    # the defect: a volume that stays where it is takes nothing from the last frames
    fixed = pds.TsdfVolume(origin, vs, dims, WALL['truncation'], device=dev)
    for pose in poses[:4]:
        fixed.integrate(d, Q, pose=pose)
    kept = fixed.tsdf.clone(), fixed.weight.clone()
    assert bool((kept[1] > 0).any())
    for pose in poses[4:]:
        fixed.integrate(d, Q, pose=pose)
    assert torch.equal(bits(fixed.tsdf), bits(kept[0])) and torch.equal(bits(fixed.weight), bits(kept[1]))
    assert fixed.extract_points().cloud.points[:, 0].max() < 1.5 + vs


# ------------------------------------------------------------------------------------------------ 6. launch probes
def test_the_kernels_ran(dev, general_state):
    lib = _lib.load()
    dims = GENERAL['dims']
    voxels = dims[0] * dims[1] * dims[2]
    groups = min(((voxels + 3) // 4 + 255) // 256, SHIFT_GROUPS)
    tiles = (voxels + TILE - 1) // TILE
    for color in (False, True):
        volume = make_volume(dev, dims, color)
        views = [put(dev, a) for a in general_state[:2]] + [put(dev, general_state[2]) if color else None]
        set_state(volume, views)
        assert probe(lib, 'tsdf_shift', lambda: volume.shift((4, 0, -1))) == [groups]       # one launch for 2 and for 3
        assert probe(lib, 'tsdf_', lambda: volume.shift((3, -2, 1))) == [groups]            # ... and no other
        assert probe(lib, 'tsdf_', lambda: volume.shift((0, 0, 0))) == []
        assert probe(lib, 'tsdf_', lambda: volume.shift((0, 0, 0), leaving=True)) == []
        set_state(volume, views)
        run = (lambda: volume.shift((4, 0, -1), leaving=True, trim=False, capacity=4096))
        assert probe(lib, 'tsdf_extract_leaving_count', run) == [tiles]
        assert probe(lib, 'tsdf_extract_leaving_scan', run) == [1]
        assert probe(lib, 'tsdf_extract_leaving_scatter', run) == [tiles]
        assert probe(lib, 'tsdf_extract', run) == [tiles, 1, tiles]
        assert probe(lib, 'tsdf_shift', run) == [groups]
        assert len(probe(lib, 'tsdf_color_gather', run)) == (1 if color else 0)   # the colours of the leaving rows
        # extract_points still runs under its old names, and only those
        extract = (lambda: volume.extract_points(trim=False, capacity=4096))
        assert probe(lib, 'tsdf_extract_count', extract) == [tiles]
        assert probe(lib, 'tsdf_extract_scan', extract) == [1]
        assert probe(lib, 'tsdf_extract_scatter', extract) == [tiles]
        assert probe(lib, 'leaving', extract) == [] and probe(lib, 'tsdf_shift', extract) == []
    # a volume larger than one grid: tsdf_shift strides
    big = pds.TsdfVolume((0.0, 0.0, 0.0), 0.01, (256, 256, 40), 0.03, device=dev)
    assert probe(lib, 'tsdf_shift', lambda: big.shift((8, 0, 0))) == [SHIFT_GROUPS]


# ------------------------------------------------------------------------------------------------ 7. the same bits
def test_same_bits_on_every_run_and_stream(dev, general_state):
    on_device = [put(dev, a) for a in general_state]
    delta = (3, -2, 1)

    def run():
        volume = general_volume(dev)
        set_state(volume, on_device)
        leaving = volume.shift(delta, leaving=True, trim=False, capacity=1 << 15)
        return state(volume) + (leaving.cloud.points, leaving.cloud.index, leaving.cloud.colors, leaving.normals,
                                leaving.cloud.offsets)

    first = run()
    count = int(first[-1][1])
    assert 0 < count < (1 << 15)   # (something leaves, and all of it fits)
    equal_bits(first[:3], oracle_shift(*general_state, delta), 'first')
    again = run()
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        aside = run()
    stream.synchronize()
    torch.cuda.current_stream(dev).wait_stream(stream)
    for other in (again, aside):
        for k, (a, b) in enumerate(zip(first, other)):
            rows = slice(None) if k < 3 or k == 7 else slice(0, count)
            assert torch.equal(bits(a[rows]) if a.dtype == torch.float32 else a[rows],
                               bits(b[rows]) if b.dtype == torch.float32 else b[rows]), k
