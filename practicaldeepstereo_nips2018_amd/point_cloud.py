"""Packed, coloured point cloud: the kept points of ``reproject`` without the rejected pixels (not in the reference).

``reproject`` returns points [B, H, W, 3] with NaN wherever a pixel was rejected.  A mesher, a registration step or a
viewer wants the kept points only, packed, with their colours and a way back to the pixel.  ``point_cloud`` is that last
stage as one entry point (``pds_point_cloud_fwd``: three launches, an ordered stream compaction fused with the
reprojection and the colour gather) instead of ``~isnan``, two boolean indexings and ``nonzero``:

    keep(p)      = reproject's point at p is not NaN:  d finite and d > 0 and W > 0 and (valid is None or valid[p]) and
                   (confidence is None or confidence[p] >= min_confidence)           (a NaN confidence fails)
                   and min_depth <= Z/W <= max_depth on the fp32 quotient itself (a depth EQUAL to a bound is kept)
    order        = raster order within a batch entry, entries in batch order
    points       [N, 3] float32, bit-identical to ``reproject(...)[b, y, x]`` of the kept pixels
    colors       [N, 3], the pixel of ``image`` at the same position, copied, not rescaled: float32 [B, 3, H, W] gives
                 float32, uint8 [B, H, W, 3] gives uint8 (``remap``'s two layouts); None without an image
    index        [N] int32, y * W + x of the pixel within its entry; None without ``with_index``
    offsets      [B + 1] int32: entry b owns rows [offsets[b], offsets[b + 1]); offsets[B] is the TRUE number of kept
                 pixels even when it exceeds ``capacity``

Exact and reproducible: integers only in the ordering, the same bits on every run.  There is no CPU fallback.
"""
import collections
import ctypes
import math
import operator

import numpy as np
import torch

from practicaldeepstereo_nips2018_amd import _lib

_Float16 = ctypes.c_float * 16

# PointCloud.entry: the rows of one batch entry (views)
PointCloudEntry = collections.namedtuple('PointCloudEntry', ['points', 'colors', 'index'])


class PointCloud(collections.namedtuple('PointCloud', ['points', 'colors', 'index', 'offsets'])):
    """``points`` [N, 3] float32, ``colors`` [N, 3] float32 / uint8 or None, ``index`` [N] int32 or None, ``offsets``
    [B + 1] int32 (see the module text).  From ``point_cloud(..., trim=False)`` the first three are the full-capacity
    buffers, of which only the first ``min(offsets[B], capacity)`` rows are defined."""

    def host_offsets(self):
        """``offsets`` as a list of Python ints.  The first call on a cloud whose offsets live on the GPU copies them
        to the host, which waits for the stream; the list is kept."""
        cached = self.__dict__.get('_host_offsets')
        if cached is None:
            cached = self.__dict__['_host_offsets'] = [int(v) for v in self.offsets.detach().cpu().tolist()]
        return cached

    def size(self):
        """Rows that hold a point: offsets[B], or the buffers' rows where the cloud was cut at ``capacity``."""
        return min(self.host_offsets()[-1], int(self.points.shape[0]))

    def entry(self, b):
        """``PointCloudEntry(points, colors, index)`` of batch entry ``b``: views, no copy.  Needs the host offsets
        (``host_offsets``: one read on an untrimmed cloud).  Rows cut off at ``capacity`` are missing from the views."""
        offsets = self.host_offsets()
        b = operator.index(b)
        if not 0 <= b < len(offsets) - 1:
            raise IndexError('entry %d of a cloud of %d entries' % (b, len(offsets) - 1))
        rows = int(self.points.shape[0])
        first, last = min(offsets[b], rows), min(offsets[b + 1], rows)
        return PointCloudEntry(self.points[first:last], None if self.colors is None else self.colors[first:last],
                               None if self.index is None else self.index[first:last])

    def save_ply(self, path, entry=None):
        """Writes the cloud (or batch entry ``entry`` alone) as a binary little-endian PLY: ``x y z`` float32, then
        ``red green blue`` uchar when the cloud has colours.  uint8 colours are written as they are; float colours are
        clamped to 0 .. 255 and rounded to the nearest integer (ties to even; NaN becomes 0).  Written on the host with
        numpy: the tensors are copied from the GPU, which waits for the stream."""
        if entry is None:
            rows = self.size()
            points, colors = self.points[:rows], None if self.colors is None else self.colors[:rows]
        else:
            points, colors, _ = self.entry(entry)
        xyz = points.detach().cpu().numpy().astype('<f4', copy=False).reshape(-1, 3)
        fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
        header = ['ply', 'format binary_little_endian 1.0', 'element vertex %d' % xyz.shape[0],
                  'property float x', 'property float y', 'property float z']
        if colors is not None:
            rgb = colors.detach().cpu().numpy().reshape(-1, 3)
            if rgb.dtype != np.uint8:
                rgb = np.rint(np.clip(np.nan_to_num(rgb.astype(np.float64), nan=0.0), 0.0, 255.0)).astype(np.uint8)
            fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
            header += ['property uchar red', 'property uchar green', 'property uchar blue']
        vertices = np.empty(xyz.shape[0], dtype=np.dtype(fields))   # (packed: 12 or 15 bytes per vertex)
        vertices['x'], vertices['y'], vertices['z'] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        if colors is not None:
            vertices['red'], vertices['green'], vertices['blue'] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
        with open(path, 'wb') as f:
            f.write(('\n'.join(header + ['end_header']) + '\n').encode('ascii'))
            f.write(vertices.tobytes())

    def gather(self, dense):
        """The rows of a dense per-pixel map at the cloud's pixels, in the cloud's order: ``dense`` [B, H, W, C] gives
        [N, C], [B, H, W] gives [N] (e.g. ``cloud.gather(surface_normals(...).normals)``: one normal per point).  Needs a
        cloud built ``with_index=True``.  The position of row r in the dense map is ``b * H * W + index[r]`` with b the
        entry whose ``offsets`` hold r; both are taken from the device tensors, without any host synchronisation.  Rows
        of an untrimmed cloud past ``offsets[B]`` are undefined in the cloud and undefined here (they read some pixel of
        the map, never outside it)."""
        if self.index is None:
            raise ValueError('gather needs the pixel indices: build the cloud with with_index=True')
        if not isinstance(dense, torch.Tensor):
            raise TypeError('dense must be a torch.Tensor')
        if dense.dim() not in (3, 4):
            raise ValueError('dense must be [B, H, W] or [B, H, W, C], got %s' % (tuple(dense.shape),))
        batch = int(self.offsets.shape[0]) - 1
        if dense.shape[0] != batch or dense.numel() == 0:
            raise ValueError('dense %s does not match a cloud of %d entries' % (tuple(dense.shape), batch))
        if dense.device != self.index.device:
            raise ValueError('dense and the cloud live on different devices')
        pixels = int(dense.shape[1]) * int(dense.shape[2])
        rows = torch.arange(self.index.shape[0], dtype=torch.int64, device=self.index.device)
        # the entry of row r: how many of offsets[1 .. B] are <= r (entries without points own no row)
        entry = torch.bucketize(rows, self.offsets[1:].to(torch.int64), right=True).clamp_(max=batch - 1)
        position = (entry * pixels + self.index.to(torch.int64)).clamp_(0, batch * pixels - 1)
        packed = dense.reshape(batch * pixels, -1).index_select(0, position)
        return packed[:, 0] if dense.dim() == 3 else packed


def save_ply(path, cloud, normals=None, entry=None):
    """Writes ``cloud`` (or its batch entry ``entry`` alone) as a binary little-endian PLY, as ``PointCloud.save_ply``
    does, with one normal per point when ``normals`` is given: ``x y z`` float32, then ``nx ny nz`` float32, then
    ``red green blue`` uchar when the cloud has colours (the order MeshLab and CloudCompare write).  ``normals``: [N, 3]
    float32, one row per row of the cloud's buffers in the cloud's order -- what ``cloud.gather(dense_normals)``
    returns.  Colours are converted as ``PointCloud.save_ply`` converts them.  Written on the host with numpy: the
    tensors are copied from the GPU, which waits for the stream.

    ``cloud`` may also be a ``TriangleMesh`` (``mesh.triangle_mesh``): after the vertices the file then holds
    ``element face F`` with ``property list uchar int vertex_indices``, 13 bytes per face (the count byte 3, then three
    little-endian int32 rows of the vertices written: with ``entry`` the faces of that entry, rebased to it).  A mesh whose
    vertices were cut at ``capacity`` is refused: its faces name vertices the file would not hold."""
    from practicaldeepstereo_nips2018_amd.mesh import TriangleMesh   # (mesh.py imports this module)
    is_mesh = isinstance(cloud, TriangleMesh)
    if not is_mesh and not isinstance(cloud, PointCloud):
        raise TypeError('cloud must be a PointCloud or a TriangleMesh')
    if normals is not None:
        if not isinstance(normals, torch.Tensor):
            raise TypeError('normals must be a torch.Tensor')
        if normals.dim() != 2 or normals.shape[1] != 3 or normals.shape[0] != cloud.points.shape[0]:
            raise ValueError('normals must be [%d, 3], one row per row of the cloud, got %s' %
                             (cloud.points.shape[0], tuple(normals.shape)))
        if normals.dtype != torch.float32:
            raise TypeError('normals must be float32, got %s' % normals.dtype)
    if entry is None:
        first, last = 0, cloud.size()
    else:
        offsets = cloud.host_offsets()
        entry = operator.index(entry)
        if not 0 <= entry < len(offsets) - 1:
            raise IndexError('entry %d of a cloud of %d entries' % (entry, len(offsets) - 1))
        rows = int(cloud.points.shape[0])
        first, last = min(offsets[entry], rows), min(offsets[entry + 1], rows)
    if is_mesh:
        if cloud.host_offsets()[-1] > int(cloud.points.shape[0]):
            raise ValueError('the vertices of this mesh were cut at capacity %d (%d were found): its faces cannot be '
                             'written' % (int(cloud.points.shape[0]), cloud.host_offsets()[-1]))
        face_offsets, face_rows = cloud.host_face_offsets(), int(cloud.faces.shape[0])
        face_first = 0 if entry is None else min(face_offsets[entry], face_rows)
        face_last = cloud.face_count() if entry is None else min(face_offsets[entry + 1], face_rows)
        triangles = cloud.faces[face_first:face_last].detach().cpu().numpy().reshape(-1, 3).astype(np.int64) - first
    xyz = cloud.points[first:last].detach().cpu().numpy().astype('<f4', copy=False).reshape(-1, 3)
    fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    header = ['ply', 'format binary_little_endian 1.0', 'element vertex %d' % xyz.shape[0],
              'property float x', 'property float y', 'property float z']
    if normals is not None:
        nxyz = normals[first:last].detach().cpu().numpy().astype('<f4', copy=False).reshape(-1, 3)
        fields += [('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')]
        header += ['property float nx', 'property float ny', 'property float nz']
    if cloud.colors is not None:
        rgb = cloud.colors[first:last].detach().cpu().numpy().reshape(-1, 3)
        if rgb.dtype != np.uint8:
            rgb = np.rint(np.clip(np.nan_to_num(rgb.astype(np.float64), nan=0.0), 0.0, 255.0)).astype(np.uint8)
        fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
        header += ['property uchar red', 'property uchar green', 'property uchar blue']
    vertices = np.empty(xyz.shape[0], dtype=np.dtype(fields))   # (packed: 12, 15, 24 or 27 bytes per vertex)
    vertices['x'], vertices['y'], vertices['z'] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if normals is not None:
        vertices['nx'], vertices['ny'], vertices['nz'] = nxyz[:, 0], nxyz[:, 1], nxyz[:, 2]
    if cloud.colors is not None:
        vertices['red'], vertices['green'], vertices['blue'] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    if is_mesh:
        header += ['element face %d' % triangles.shape[0], 'property list uchar int vertex_indices']
        records = np.empty(triangles.shape[0], dtype=np.dtype([('n', 'u1'), ('v', '<i4', (3,))]))   # (packed: 13 bytes)
        records['n'], records['v'] = 3, triangles
    with open(path, 'wb') as f:
        f.write(('\n'.join(header + ['end_header']) + '\n').encode('ascii'))
        f.write(vertices.tobytes())
        if is_mesh:
            f.write(records.tobytes())


_workspace = _lib.Workspace()


def _gpu_device(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor' % name)
    if not t.is_cuda:
        raise RuntimeError('%s must live on an MI355X (cuda) device: the HIP path has no CPU fallback' % name)
    return t.device


def _depth_bound(value, name, absent):
    if value is None:
        return absent
    value = float(value)
    if math.isnan(value):
        raise ValueError('%s is NaN' % name)
    return value


def _rows(capacity, name, default):
    if capacity is None:
        return default
    try:
        rows = operator.index(None if isinstance(capacity, bool) else capacity)
    except TypeError:
        raise TypeError('%s must be an integer or None, got %r' % (name, capacity))
    if rows < 0:
        raise ValueError('%s must be >= 0, got %r' % (name, capacity))
    return rows


def _host_checks(disparity, matrix, image, valid, confidence, min_confidence, min_depth, max_depth, capacity):
    """What can be judged without a GPU (types, shapes, thresholds), for ``point_cloud`` and ``mesh.triangle_mesh``
    -> (shape, matrix as fp64 4x4, min_confidence, min_depth, max_depth, rows, image layout)."""
    for name, t in (('disparity', disparity),) + ((('confidence', confidence),) if confidence is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError('%s must be a torch.Tensor' % name)
        if t.dtype != torch.float32:
            raise TypeError('%s must be float32, got %s' % (name, t.dtype))
        if t.dim() != 3:
            raise ValueError('%s must have 3 dimensions, got %d' % (name, t.dim()))
    shape = tuple(disparity.shape)
    m = np.asarray(matrix, dtype=np.float64)
    if m.shape != (4, 4) or not np.all(np.isfinite(m)):
        raise ValueError('matrix must be a finite 4x4, got shape %s' % (m.shape,))
    min_confidence = float(min_confidence)
    if math.isnan(min_confidence):
        raise ValueError('min_confidence is NaN')
    min_depth = _depth_bound(min_depth, 'min_depth', -math.inf)
    max_depth = _depth_bound(max_depth, 'max_depth', math.inf)
    if min_depth > max_depth:
        raise ValueError('min_depth %r > max_depth %r' % (min_depth, max_depth))
    batch, height, width = shape
    rows = _rows(capacity, 'capacity', batch * height * width)
    layout = 0
    if image is not None:
        if not isinstance(image, torch.Tensor):
            raise TypeError('image must be a torch.Tensor')
        if image.dtype == torch.uint8:
            if image.dim() != 4 or image.shape[-1] != 3:
                raise ValueError('a uint8 image must be [B, H, W, 3], got %s' % (tuple(image.shape),))
            layout, size = 1, tuple(image.shape[:3])
        elif image.dtype == torch.float32:
            if image.dim() != 4 or image.shape[1] != 3:
                raise ValueError('a float32 image must be [B, 3, H, W], got %s' % (tuple(image.shape),))
            layout, size = 0, (image.shape[0],) + tuple(image.shape[2:])
        else:
            raise TypeError('image must be uint8 [B, H, W, 3] or float32 [B, 3, H, W], got %s' % (image.dtype,))
        if size != shape:
            raise ValueError('image %s does not match disparity %s in (B, H, W)' % (tuple(image.shape), shape))
    if valid is not None:
        if not isinstance(valid, torch.Tensor):
            raise TypeError('valid must be a torch.Tensor')
        if valid.dtype != torch.bool or tuple(valid.shape) != shape:
            raise ValueError('valid must be torch.bool %s, got %s %s' % (shape, valid.dtype, tuple(valid.shape)))
    if confidence is not None and tuple(confidence.shape) != shape:
        raise ValueError('confidence %s and disparity %s differ in shape' % (tuple(confidence.shape), shape))
    return shape, m, min_confidence, min_depth, max_depth, rows, layout


def _device_checks(what, disparity, image, valid, confidence):
    """Where the tensors live -> (disparity, image, valid, confidence), detached and contiguous."""
    d = _lib.require_gpu_tensor(disparity.detach(), 'disparity', 3)
    if d.numel() == 0:
        raise ValueError('%s: empty input %s' % (what, tuple(disparity.shape)))
    if image is not None:
        _gpu_device(image, 'image')
        image = image.detach().contiguous()
    if valid is not None:
        _gpu_device(valid, 'valid')
        valid = valid.contiguous()
    if confidence is not None:
        confidence = _lib.require_gpu_tensor(confidence.detach(), 'confidence', 3)
    for name, t in (('image', image), ('valid', valid), ('confidence', confidence)):
        if t is not None and t.device != d.device:
            raise ValueError('%s and disparity live on different devices' % name)
    return d, image, valid, confidence


def point_cloud(disparity, matrix, image=None, valid=None, confidence=None, min_confidence=0.0, min_depth=None,
                max_depth=None, with_index=False, capacity=None, trim=True):
    """Disparity float32 [B, H, W] -> ``PointCloud(points, colors, index, offsets)``: the kept points of
    ``reproject(disparity, matrix, valid, confidence, min_confidence)``, packed (see the module text).

    ``image``: the rectified left image, uint8 [B, H, W, 3] or float32 [B, 3, H, W], for ``colors``.  ``min_depth`` /
    ``max_depth``: keep only points whose depth Z / W lies in the closed interval (None: no bound).  ``with_index``:
    also return ``index``.  ``capacity``: rows of the output buffers; None means B * H * W, which can never overflow.

    ``trim=True`` reads ``offsets`` once on the host -- the ONLY synchronisation of the call -- and returns tensors of
    exactly N rows; it raises if an explicit ``capacity`` was smaller than N.  ``trim=False`` returns the full-capacity
    buffers and the device ``offsets`` without any synchronisation: only the first ``min(offsets[B], capacity)`` rows
    are defined, and ``offsets[B] > capacity`` tells that the cloud was cut.  Runs on the current stream, without
    autograd."""
    # what can be judged without a GPU comes first: types, shapes, thresholds
    shape, m, min_confidence, min_depth, max_depth, rows, layout = _host_checks(
        disparity, matrix, image, valid, confidence, min_confidence, min_depth, max_depth, capacity)
    batch, height, width = shape
    # then where the tensors live
    d, image, valid, confidence = _device_checks('point_cloud', disparity, image, valid, confidence)
    c_matrix = _Float16(*m.astype(np.float32).reshape(-1).tolist())
    lib = _lib.load()
    nbytes = int(lib.pds_point_cloud_workspace_bytes(batch, height, width))
    if nbytes == 0:
        raise ValueError('point_cloud: %s' % lib.pds_last_error().decode(errors='replace'))
    held = max(rows, 1)   # (a buffer of no rows has no address)
    points = torch.empty((held, 3), dtype=torch.float32, device=d.device)
    colors = None if image is None else torch.empty((held, 3), dtype=image.dtype, device=d.device)
    index = torch.empty((held,), dtype=torch.int32, device=d.device) if with_index else None
    offsets = torch.empty((batch + 1,), dtype=torch.int32, device=d.device)
    with torch.cuda.device(d.device):
        workspace = _workspace.get(nbytes, d.device)
        _lib.check(lib.pds_point_cloud_fwd(
            _lib.ptr(d), None if valid is None else _lib.ptr(valid),
            None if confidence is None else _lib.ptr(confidence), min_confidence, c_matrix, min_depth, max_depth,
            None if image is None else _lib.ptr(image), layout, _lib.ptr(points),
            None if colors is None else _lib.ptr(colors), None if index is None else _lib.ptr(index),
            _lib.ptr(offsets), rows, batch, height, width, _lib.ptr(workspace), workspace.numel(),
            _lib.stream_handle(d.device)), 'pds_point_cloud_fwd')
    cut = (lambda t: None if t is None else t[:rows])
    cloud = PointCloud(cut(points), cut(colors), cut(index), offsets)
    if not trim:
        return cloud
    count = cloud.host_offsets()[-1]   # the one synchronisation
    if count > rows:
        raise RuntimeError('point_cloud: %d points do not fit capacity %d (trim=False returns the first %d and the '
                           'true count in offsets)' % (count, rows, rows))
    cut = (lambda t: None if t is None else t[:count])
    trimmed = PointCloud(cut(points), cut(colors), cut(index), offsets)
    trimmed.__dict__['_host_offsets'] = cloud.host_offsets()
    return trimmed
