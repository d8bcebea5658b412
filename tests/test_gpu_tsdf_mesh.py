"""GPU (-m gpu): the triangle mesh of a TSDF volume (TsdfVolume.extract_mesh; pds_tsdf_mesh_fwd).

The arbiter is the numpy oracle of tests/test_tsdf_mesh_host.py (held there to a closed, consistently wound sphere).
Integers -- index, both offsets, faces -- are exactly the oracle's.  Points and normals get the bound
tests/test_gpu_tsdf.py gives extract_points, derived the same way: r = t_v / (t_v - t_n) is two float32 roundings of a
value in [0, 1] (2^-23 of a voxel at most), (i + 0.5) + r is rounded once (half an ulp of a number below 256: 7.7e-6 of a
voxel at these sizes), together below 1e-5 voxel_size; the one fmaf that follows rounds the point once, and the oracle's
own float32 origin and voxel_size agree with the kernel's, which 4 ulp of the point cover with room.  A diagonal edge adds
the same r to two or three coordinates instead of one: the same bound per coordinate.  Normals: NaN exactly where the
oracle has them, the others within 2.28e-5 rad (4 eps32, tests/test_gpu_surface_normals.py) where |g| >= 1e-4.  The state
is set through the public volume.tsdf and volume.weight.  Tiles are TILE = 1024 voxels and at most MAX_GROUPS workgroups
run, so the shapes sit around both."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib
from tests.test_tsdf_mesh_host import (MAX_GROUPS, TILE, check_closed_sphere, check_open_edges_border_the_unobserved,
                                       mesh_topology, oracle_mesh, pattern_volume, sphere_volume)

pytestmark = pytest.mark.gpu

ANGLE = 2.28e-5   # rad: tests/test_gpu_surface_normals.py, 4 eps32
ORIGIN, VOXEL = (-1.5, 0.25, 3.0), 0.03


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def put(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(t):
    return t.contiguous().view(torch.int32)


def volume_of(dev, tsdf, weight, origin=ORIGIN, voxel_size=VOXEL):
    nz, ny, nx = tsdf.shape
    volume = pds.TsdfVolume(origin, voxel_size, (nx, ny, nz), 0.1, device=dev)
    volume.tsdf, volume.weight = put(dev, tsdf), put(dev, weight)
    return volume


def check_mesh(got, oracle, voxel_size, case=''):
    """got: SurfaceMesh (trimmed) -> (share of the point bound reached, largest angle / ANGLE, normals compared)."""
    mesh = got.mesh
    assert mesh.colors is None and mesh.offsets.cpu().tolist() == [0, len(oracle.index)], case
    assert mesh.face_offsets.cpu().tolist() == [0, len(oracle.faces)], case
    index, faces, points = mesh.index.cpu().numpy(), mesh.faces.cpu().numpy(), mesh.points.cpu().numpy()
    assert index.dtype == np.int32 and np.array_equal(index, oracle.index), case
    assert faces.dtype == np.int32 and faces.shape == oracle.faces.shape and np.array_equal(faces, oracle.faces), case
    assert points.dtype == np.float32 and points.shape == (len(oracle.index), 3), case
    tolerance = 1e-5 * voxel_size + 4 * np.spacing(np.abs(oracle.points).astype(np.float32)).astype(np.float64)
    share = (np.abs(points - oracle.points) / tolerance).max(initial=0.0)
    print('%s: %d vertices, %d faces, points reach %.3f of their bound' % (case, len(index), len(faces), share))
    assert share <= 1.0, (case, share)
    if got.normals is None:
        return share, 0.0, 0
    normals = got.normals.cpu().numpy().astype(np.float64)
    assert normals.shape == points.shape, case
    missing = np.isnan(oracle.normals).any(axis=1)
    assert np.array_equal(np.isnan(normals), np.isnan(oracle.normals)), case
    with np.errstate(invalid='ignore'):
        checked = ~missing & (oracle.gradient_norm >= 1e-4)
    cross = np.linalg.norm(np.cross(normals[checked], oracle.normals[checked]), axis=1)
    angle = np.arctan2(cross, (normals[checked] * oracle.normals[checked]).sum(axis=1)).max(initial=0.0)
    print('%s: %d normals compared, the largest angle %.3f of its bound' % (case, int(checked.sum()), angle / ANGLE))
    assert angle <= ANGLE, (case, float(angle))
    assert np.abs(np.linalg.norm(normals[~missing], axis=1) - 1.0).max(initial=0.0) <= 1e-6, case
    return share, angle / ANGLE, int(checked.sum())


# ------------------------------------------------------------------------------------------------ 1. one cell
def test_all_256_patterns_of_one_cell(dev):
    for pattern in range(256):
        tsdf, weight = pattern_volume(pattern)
        oracle = oracle_mesh(tsdf, weight, ORIGIN, VOXEL)
        got = volume_of(dev, tsdf, weight).extract_mesh(capacity=28, face_capacity=12)
        mesh = got.mesh
        assert mesh.offsets.tolist() == [0, len(oracle.index)] and mesh.face_offsets.tolist() == [0, len(oracle.faces)]
        assert np.array_equal(mesh.index.cpu().numpy(), oracle.index), pattern
        assert np.array_equal(mesh.faces.cpu().numpy(), oracle.faces.astype(np.int32).reshape(-1, 3)), pattern
        tolerance = 1e-5 * VOXEL + 4 * np.spacing(np.abs(oracle.points).astype(np.float32)).astype(np.float64)
        assert (np.abs(mesh.points.cpu().numpy() - oracle.points) <= tolerance).all(), pattern
        assert bool(got.normals.isnan().all())   # (no stencil fits a 2 x 2 x 2 volume)


# ------------------------------------------------------------------------------------------------ 2. random volumes
def block_volume(dims, seed, min_weight):
    """Random float32 tsdf in [-1, 1] with -0.0, 0.0 and 1.0 among them; weights drawn per 4 x 4 x 4 block around
    min_weight, so that whole cells are observed, with single voxels knocked out."""
    nx, ny, nz = dims
    rng = np.random.RandomState(seed)
    tsdf = rng.uniform(-1.0, 1.0, (nz, ny, nx)).astype(np.float32)
    special = rng.rand(nz, ny, nx)
    tsdf[special < 0.02] = -0.0
    tsdf[(special >= 0.02) & (special < 0.04)] = 0.0
    tsdf[(special >= 0.04) & (special < 0.06)] = 1.0
    blocks = [(n + 3) // 4 for n in (nz, ny, nx)]
    below = np.nextafter(np.float32(min_weight), np.float32(0.0))
    per_block = rng.choice(np.array([min_weight, 2.0 * min_weight, 64.0, below, 0.0], dtype=np.float32), blocks,
                           p=[0.3, 0.2, 0.2, 0.15, 0.15])
    weight = np.repeat(np.repeat(np.repeat(per_block, 4, 0), 4, 1), 4, 2)[:nz, :ny, :nx].copy()
    weight[rng.rand(nz, ny, nx) < 0.02] = below
    return tsdf, weight


RANDOM_DIMS = [(33, 5, 7), (7, 33, 5), (3, 3, 130), (1, 5, 5)]


@functools.lru_cache(maxsize=None)
def random_case(dims, min_weight):
    tsdf, weight = block_volume(dims, sum(dims), min_weight)
    return tsdf, weight, oracle_mesh(tsdf, weight, ORIGIN, VOXEL, min_weight)


@pytest.mark.parametrize('dims', RANDOM_DIMS, ids=lambda d: '%dx%dx%d' % d)
def test_random_volumes_against_the_oracle(dev, dims):
    for min_weight in (1.0, 0.375):
        tsdf, weight, oracle = random_case(dims, min_weight)
        observed = weight >= np.float32(min_weight)
        assert observed.any() and not observed.all()   # both branches
        if min(dims) > 1:
            assert len(oracle.faces) >= 300 and (dims[0] * dims[1] * dims[2] > TILE)
        else:
            assert len(oracle.faces) == 0 and len(oracle.index) > 0   # vertices, no cell: not an error
        volume = volume_of(dev, tsdf, weight)
        got = volume.extract_mesh(min_weight=min_weight)
        check_mesh(got, oracle, VOXEL, 'random %s min_weight %g' % (dims, min_weight))
        plain = volume.extract_mesh(min_weight=min_weight, with_normals=False)
        assert plain.normals is None and torch.equal(bits(plain.mesh.points), bits(got.mesh.points))
        assert torch.equal(plain.mesh.faces, got.mesh.faces)
        # the axis edges are extract_points' points, bit for bit: index // 7 * 3 + {0, 1, 2}
        cloud = volume.extract_points(min_weight=min_weight)
        index = got.mesh.index.to(torch.int64)
        d = index % 7 + 1
        axis = (d == 1) | (d == 2) | (d == 4)
        mapped = index[axis] // 7 * 3 + torch.log2(d[axis].double()).long()
        assert int(axis.sum()) == cloud.cloud.points.shape[0] and torch.equal(mapped, cloud.cloud.index.to(torch.int64))
        assert torch.equal(bits(got.mesh.points[axis]), bits(cloud.cloud.points))
        assert torch.equal(bits(got.normals[axis]), bits(cloud.normals))


def test_a_volume_of_more_tiles_than_workgroups(dev):
    """(130, 130, 130): 2146 tiles on MAX_GROUPS = 2048 workgroups, the first 98 of which take a second tile.  A sphere in
    two opposite corners of it, so that the oracle stays quick; an unobserved block cuts each."""
    n, dims = 20, (130, 130, 130)
    small, weight_small, _ = sphere_volume()
    weight_small[2:6, 8:12, 8:12] = 0.0
    tsdf = np.ones((dims[2], dims[1], dims[0]), dtype=np.float32)
    weight = np.ones_like(tsdf)
    assert (tsdf.size + TILE - 1) // TILE > MAX_GROUPS
    for corner in ((0, 0, 0), (dims[2] - n, dims[1] - n, dims[0] - n)):   # the first tiles and the strided ones
        k, j, i = corner
        tsdf[k:k + n, j:j + n, i:i + n] = small
        weight[k:k + n, j:j + n, i:i + n] = weight_small
    oracle = oracle_mesh(tsdf, weight, ORIGIN, VOXEL)
    assert len(oracle.faces) > 5000 and oracle.keys.max() // 6 > MAX_GROUPS * TILE
    got = volume_of(dev, tsdf, weight).extract_mesh(capacity=len(oracle.index) + 3, face_capacity=len(oracle.faces) + 3)
    check_mesh(got, oracle, VOXEL, 'strided')


# ------------------------------------------------------------------------------------------------ 3. the sphere
def test_the_sphere_is_closed_on_the_gpu(dev):
    tsdf, weight, centre = sphere_volume()
    got = volume_of(dev, tsdf, weight).extract_mesh(capacity=8192, face_capacity=16384)
    mesh = got.mesh
    vertices, edges, faces = check_closed_sphere(mesh.index.cpu().numpy(), mesh.points.cpu().numpy(),
                                                 mesh.faces.cpu().numpy(), centre, ORIGIN, VOXEL)
    assert vertices > 1500 and faces == 2 * vertices - 4 and mesh.face_count() == faces
    # the normals look the way the faces do
    normals = got.normals.cpu().numpy().astype(np.float64)
    outward = mesh.points.cpu().numpy() - (np.asarray(ORIGIN) + VOXEL * centre)
    assert not np.isnan(normals).any() and ((normals * outward).sum(axis=1) > 0).all()
    # with an unobserved block the mesh is open exactly along the block
    weight[2:6, 8:12, 8:12] = 0.0
    cut = volume_of(dev, tsdf, weight).extract_mesh(capacity=8192, face_capacity=16384).mesh
    assert check_open_edges_border_the_unobserved(cut.index.cpu().numpy(), cut.faces.cpu().numpy(), weight >= 1.0) >= 8


# ------------------------------------------------------------------------------------------------ 4. capacities
def raw_mesh(dev, volume, min_weight, capacity, face_capacity, normals=True):
    """The entry point itself into prefilled buffers of 8 rows more than the capacities."""
    lib = _lib.load()
    dims = volume.dims
    nbytes = lib.pds_tsdf_mesh_workspace_bytes(*dims)
    points = torch.full((capacity + 8, 3), float('nan'), device=dev)
    normal = torch.full((capacity + 8, 3), float('nan'), device=dev) if normals else None
    index = torch.full((capacity + 8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    faces = torch.full((face_capacity + 8, 3), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    offsets = torch.full((2, 2), -1, dtype=torch.int32, device=dev)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    origin = (ctypes.c_float * 3)(*np.asarray(volume.origin, dtype=np.float32).tolist())
    _lib.check(lib.pds_tsdf_mesh_fwd(
        _lib.ptr(volume.tsdf), _lib.ptr(volume.weight), origin, volume.voxel_size, min_weight, _lib.ptr(points),
        None if normal is None else _lib.ptr(normal), _lib.ptr(index), _lib.ptr(offsets[0]), capacity, _lib.ptr(faces),
        _lib.ptr(offsets[1]), face_capacity, *dims, _lib.ptr(workspace), nbytes, _lib.stream_handle(dev)),
        'pds_tsdf_mesh_fwd')
    return points, normal, index, faces, offsets


def test_capacities(dev):
    tsdf, weight, oracle = random_case((33, 5, 7), 1.0)
    volume = volume_of(dev, tsdf, weight)
    full = volume.extract_mesh()
    count, face_count = full.mesh.points.shape[0], full.mesh.faces.shape[0]
    assert count == len(oracle.index) > 8 and face_count == len(oracle.faces) > 8
    for capacity, face_capacity in ((0, 0), (count - 1, face_count - 1), (count, 0), (0, face_count), (count, face_count)):
        points, normals, index, faces, offsets = raw_mesh(dev, volume, 1.0, capacity, face_capacity)
        where = (capacity, face_capacity)
        assert offsets.tolist() == [[0, count], [0, face_count]], where   # the TRUE counts
        assert torch.equal(bits(points[:capacity]), bits(full.mesh.points[:capacity])), where
        assert torch.equal(bits(normals[:capacity]), bits(full.normals[:capacity])), where
        assert torch.equal(index[:capacity], full.mesh.index[:capacity]), where
        # a row of faces is the same whether or not the vertices were cut
        assert torch.equal(faces[:face_capacity], full.mesh.faces[:face_capacity]), where
        assert bool(points[capacity:].isnan().all()) and bool(normals[capacity:].isnan().all()), where
        assert bool((index[capacity:] == 0x5A5A5A5A).all()) and bool((faces[face_capacity:] == 0x5A5A5A5A).all()), where
    with pytest.raises(RuntimeError, match='%d vertices do not fit capacity %d' % (count, count - 1)):
        volume.extract_mesh(capacity=count - 1)
    with pytest.raises(RuntimeError, match='%d faces do not fit face_capacity %d' % (face_count, face_count - 1)):
        volume.extract_mesh(face_capacity=face_count - 1)
    with pytest.raises(RuntimeError, match='do not fit capacity 0'):
        volume.extract_mesh(capacity=0, face_capacity=0)
    # trim=False: the full-capacity buffers, the device offsets, and no synchronisation
    torch.cuda.synchronize()
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        cut = volume.extract_mesh(capacity=count - 1, face_capacity=face_count + 5, trim=False)
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    assert cut.mesh.points.shape == (count - 1, 3) and cut.normals.shape == (count - 1, 3)
    assert cut.mesh.faces.shape == (face_count + 5, 3) and cut.mesh.index.shape == (count - 1,)
    assert cut.mesh.offsets.tolist() == [0, count] and cut.mesh.face_offsets.tolist() == [0, face_count]
    assert torch.equal(cut.mesh.faces[:face_count], full.mesh.faces) and cut.mesh.face_count() == face_count
    assert cut.mesh.size() == count - 1
    # nothing observed: an empty mesh
    volume.weight = torch.zeros_like(volume.weight)
    empty = volume.extract_mesh()
    assert empty.mesh.points.shape == (0, 3) and empty.mesh.faces.shape == (0, 3) and empty.normals.shape == (0, 3)


# ------------------------------------------------------------------------------------------------ 5. streams
def test_same_bytes_on_every_run_and_stream(dev):
    tsdf, weight, _ = random_case((3, 3, 130), 1.0)
    volume = volume_of(dev, tsdf, weight)
    first = volume.extract_mesh()
    assert first.mesh.faces.shape[0] > 300

    def same(other):
        return (torch.equal(bits(other.mesh.points), bits(first.mesh.points)) and
                torch.equal(bits(other.normals), bits(first.normals)) and torch.equal(other.mesh.index, first.mesh.index)
                and torch.equal(other.mesh.faces, first.mesh.faces))

    for _ in range(2):
        assert same(volume.extract_mesh())
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    results = []
    for stream in streams:
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            results.append(volume.extract_mesh())
    for stream, other in zip(streams, results):
        stream.synchronize()
        torch.cuda.current_stream(dev).wait_stream(stream)
        assert same(other)


# ------------------------------------------------------------------------------------------------ 6. alignment, guards
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


def test_unaligned_tensors_agree_and_guards_stay(dev):
    lib = _lib.load()
    for dims in ((33, 5, 7), (3, 3, 130)):
        tsdf, weight, oracle = random_case(dims, 1.0)
        aligned = volume_of(dev, tsdf, weight)
        full = aligned.extract_mesh()
        count, face_count = len(oracle.index), len(oracle.faces)
        nbytes = lib.pds_tsdf_mesh_workspace_bytes(*dims)
        origin = (ctypes.c_float * 3)(*np.asarray(ORIGIN, dtype=np.float32).tolist())
        for lead, (lead_t, lead_w) in enumerate(((0, 0), (1, 1), (3, 3), (0, 2))):
            tsdf_buffer, tsdf_view = guarded(aligned.tsdf, lead_t, -7.0)
            weight_buffer, weight_view = guarded(aligned.weight, lead_w, -9.0)
            assert tsdf_view.data_ptr() % 16 == 4 * lead_t and weight_view.data_ptr() % 16 == 4 * lead_w
            workspace = torch.full((nbytes + 512,), 0x5A, dtype=torch.uint8, device=dev)
            points_buffer, points = guarded(torch.zeros(3 * count, device=dev), lead, -7.0)
            normals_buffer, normals = guarded(torch.zeros(3 * count, device=dev), (lead + 1) % 4, -8.0)
            index_buffer, index = guarded(torch.zeros(count, dtype=torch.int32, device=dev), (lead + 2) % 4, -5)
            faces_buffer, faces = guarded(torch.zeros(3 * face_count, dtype=torch.int32, device=dev), (lead + 3) % 4, -6)
            offsets = torch.full((2, 2), -1, dtype=torch.int32, device=dev)
            _lib.check(lib.pds_tsdf_mesh_fwd(
                _lib.ptr(tsdf_view), _lib.ptr(weight_view), origin, VOXEL, 1.0, _lib.ptr(points), _lib.ptr(normals),
                _lib.ptr(index), _lib.ptr(offsets[0]), count, _lib.ptr(faces), _lib.ptr(offsets[1]), face_count, *dims,
                _lib.ptr(workspace[256:]), nbytes, _lib.stream_handle(dev)), 'pds_tsdf_mesh_fwd')
            torch.cuda.synchronize()
            where = (dims, lead, lead_t, lead_w)
            assert offsets.tolist() == [[0, count], [0, face_count]], where
            assert torch.equal(bits(points), bits(full.mesh.points.reshape(-1))), where
            assert torch.equal(bits(normals), bits(full.normals.reshape(-1))), where
            assert torch.equal(index, full.mesh.index) and torch.equal(faces, full.mesh.faces.reshape(-1)), where
            assert guards_untouched(points_buffer, lead, 3 * count, -7.0), where
            assert guards_untouched(normals_buffer, (lead + 1) % 4, 3 * count, -8.0), where
            assert guards_untouched(index_buffer, (lead + 2) % 4, count, -5), where
            assert guards_untouched(faces_buffer, (lead + 3) % 4, 3 * face_count, -6), where
            assert bool((workspace[:256] == 0x5A).all()) and bool((workspace[256 + nbytes:] == 0x5A).all()), where
            # the state is read only: its bits and its guards are what they were
            assert torch.equal(bits(tsdf_view), bits(aligned.tsdf)) and torch.equal(bits(weight_view), bits(aligned.weight))
            assert guards_untouched(tsdf_buffer, lead_t, aligned.tsdf.numel(), -7.0), where
            assert guards_untouched(weight_buffer, lead_w, aligned.weight.numel(), -9.0), where


# ------------------------------------------------------------------------------------------------ 7. probes
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
    tsdf, weight, _ = random_case((33, 5, 7), 1.0)
    volume = volume_of(dev, tsdf, weight)
    tiles = (33 * 5 * 7 + TILE - 1) // TILE
    assert tiles == 2
    mesh = (lambda: volume.extract_mesh(trim=False, capacity=4096, face_capacity=4096))
    for name in ('count', 'scatter', 'face_count', 'face_scatter'):
        assert probe(lib, 'tsdf_mesh_' + name, mesh) == [tiles], name
    assert probe(lib, 'tsdf_mesh_scan', mesh) == [1] and probe(lib, 'tsdf_mesh_face_scan', mesh) == [1]
    assert probe(lib, 'tsdf_mesh', mesh) == [tiles, 1, tiles, tiles, 1, tiles]
    # extract_points is what it was: its three launches, none of the mesh's
    assert probe(lib, 'tsdf_extract', lambda: volume.extract_points(trim=False, capacity=4096)) == [tiles, 1, tiles]
    assert probe(lib, 'tsdf_extract', mesh) == []
    # more tiles than workgroups: the tile kernels stride
    big = pds.TsdfVolume(ORIGIN, VOXEL, (130, 130, 130), 0.1, device=dev)
    assert probe(lib, 'tsdf_mesh', lambda: big.extract_mesh(trim=False, capacity=16, face_capacity=16)) == [
        MAX_GROUPS, 1, MAX_GROUPS, MAX_GROUPS, 1, MAX_GROUPS]


# ------------------------------------------------------------------------------------------------ 8. end to end
# The synthetic wall of tests/test_gpu_tsdf.py, restated: focal 74 px, baseline 1/8 m, disparity 8: Z = 74 / 64 = 1.15625 m;
# voxels of 1/8 m whose layers lie at z = 1, 1.125, 1.25, ...; truncation 1/8.
WALL = dict(height=48, width=64, focal=74.0, baseline=0.125, disparity=8.0, depth=1.15625, voxel_size=0.125, z0=0.9375,
            truncation=0.125)


def test_end_to_end_wall_mesh_and_ply(dev, tmp_path):
    dims = (17, 9, 5)
    height, width, vs = WALL['height'], WALL['width'], WALL['voxel_size']
    Q = np.array([[1.0, 0.0, 0.0, -0.5 * (width - 1)], [0.0, 1.0, 0.0, -0.5 * (height - 1)],
                  [0.0, 0.0, 0.0, WALL['focal']], [0.0, 0.0, 1.0 / WALL['baseline'], 0.0]])
    origin = np.array([-0.5 * dims[0] * vs + 0.015625, -0.5 * dims[1] * vs + 0.015625, WALL['z0']])
    volume = pds.TsdfVolume(origin, vs, dims, WALL['truncation'], device=dev)
    d = torch.full((1, height, width), WALL['disparity'], device=dev)
    # two poses: the camera at the origin, and moved 1/16 m to the side (a wall parallel to the image stays where it is)
    shifted = np.hstack([np.eye(3), [[0.0625], [0.0], [0.0]]])
    volume.integrate(d, Q).integrate(d, Q, pose=shifted)
    got = volume.extract_mesh(capacity=4096, face_capacity=8192)
    mesh = got.mesh
    vertices, faces = mesh.points.shape[0], mesh.faces.shape[0]
    assert vertices > 50 and faces > 50 and mesh.face_count() == faces and mesh.size() == vertices
    oracle = oracle_mesh(volume.tsdf.cpu().numpy(), volume.weight.cpu().numpy(), origin, vs)
    check_mesh(got, oracle, vs, 'wall')
    points = mesh.points.cpu().numpy().astype(np.float64)
    assert np.abs(points[:, 2] - WALL['depth']).max() < 1e-5   # the wall, a quarter of the way between two layers
    # every face looks at the cameras, which stand on the side of the positive values: z below the wall's
    corner = points[mesh.faces.cpu().numpy()]
    normal = np.cross(corner[:, 1] - corner[:, 0], corner[:, 2] - corner[:, 0])
    for centre in (np.zeros(3), -shifted[:, 3]):
        assert ((normal * (centre - corner.mean(axis=1))).sum(axis=1) > 0).all()
    assert mesh.entry(0).faces.shape == (faces, 3) and mesh.cloud().points.shape == (vertices, 3)
    # through save_ply and back
    path = str(tmp_path / 'model.ply')
    mesh.save_ply(path, normals=got.normals)
    raw = open(path, 'rb').read()
    header, body = raw.split(b'end_header\n', 1)
    assert b'element vertex %d\n' % vertices in header and b'element face %d\n' % faces in header
    assert b'property float nx' in header and b'property list uchar int vertex_indices' in header
    assert len(body) == 24 * vertices + 13 * faces
    stored = np.frombuffer(body[:24 * vertices], dtype=np.dtype([(n, '<f4') for n in ('x', 'y', 'z', 'nx', 'ny', 'nz')]))
    assert np.array_equal(stored['x'], mesh.points[:, 0].cpu().numpy())
    triangles = np.frombuffer(body[24 * vertices:], dtype=np.dtype([('n', 'u1'), ('v', '<i4', (3,))]))
    assert (triangles['n'] == 3).all() and np.array_equal(triangles['v'], mesh.faces.cpu().numpy())
