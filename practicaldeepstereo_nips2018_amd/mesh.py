"""Triangle mesh from disparity: the packed cloud plus edge-aware faces (not in the reference).

``point_cloud`` ends in points; a mesher, a viewer that shades, Poisson reconstruction want a surface.  A disparity map is
a regular grid, so the natural mesh is two triangles per 2 x 2 cell of pixels, cut wherever a depth edge runs through the
cell.  ``triangle_mesh`` is that as one entry point (``pds_triangle_mesh_fwd``: six launches, the three of the cloud and
an ordered compaction of the faces) instead of a rank map scattered from ``index``, six shifted comparisons, two
``nonzero``, gathers, a ``cat`` and an argsort:

    vertices     exactly the rows of ``point_cloud(...)`` on the same arguments: ``points``, ``colors``, ``index``,
                 ``offsets``, bit for bit and in the same order (the same kernels).  A kept pixel that ends up in no face
                 stays a vertex.
    edges        two kept pixels p, q of one entry are joined iff fabsf(D[p] - D[q]) <= max_difference: ONE fp32
                 subtraction of the input disparities (the rule of ``surface_normals``)
    cells        for x in [0, W - 2] and y in [0, H - 2] of entry b the corners  a = (x, y)      b = (x + 1, y)
                                                                                c = (x, y + 1)  e = (x + 1, y + 1)
                 (no cell at x = W - 1 or y = H - 1: none spans two rows' ends or two entries).  A triangle is emitted
                 iff its three corners are kept and its three edges are joined, the diagonal included.
                   four corners kept:   the diagonal is a-e iff fabsf(D[a] - D[e]) < fabsf(D[b] - D[c]); otherwise, ties
                                        included, it is b-c.  Diagonal b-c: the candidates (a, c, b) then (b, c, e);
                                        diagonal a-e: (a, c, e) then (a, e, b).  No fallback to the other diagonal.
                   three corners kept:  the one candidate of the lists above that avoids the missing corner:
                                        e missing: (a, c, b)   a missing: (b, c, e)   b missing: (a, c, e)
                                        c missing: (a, e, b)
                   fewer:               nothing
    winding      the vertex order is as listed; ``flip=True`` swaps the second and the third vertex of every face.  The
                 listed order faces a camera at the origin, ((p1 - p0) x (p2 - p0)) . p0 < 0, for a matrix with X right,
                 Y down, Z forward (``StereoRig.reprojection_matrix``).
    order        faces are ordered by the flat index of their corner a (raster order within an entry, entries in batch
                 order); within a cell the first candidate comes before the second
    faces        [F, 3] int32: rows of ``points``, counted over the whole batch (``entry(b)`` subtracts ``offsets[b]``).
                 With a vertex ``capacity`` smaller than N the faces still hold the true rows.
    face_offsets [B + 1] int32: entry b owns faces [face_offsets[b], face_offsets[b + 1]); face_offsets[B] is the TRUE
                 number of faces even when it exceeds ``face_capacity``

Exact and reproducible: every output is an integer or a bit-copy, the same bits on every run and on every stream.  Shapes
with 2 * B * H * W > 2^31 - 1 are refused.  There is no CPU fallback.
"""
import collections
import importlib
import math
import operator

import numpy as np
import torch

from practicaldeepstereo_nips2018_amd import _lib

# (the package's attribute ``point_cloud`` is the function, which hides the module of that name)
_pc = importlib.import_module('practicaldeepstereo_nips2018_amd.point_cloud')

# TriangleMesh.entry: the rows of one batch entry (views of the vertices; the faces rebased to the entry: a copy)
TriangleMeshEntry = collections.namedtuple('TriangleMeshEntry', ['points', 'colors', 'index', 'faces'])


class TriangleMesh(collections.namedtuple('TriangleMesh', ['points', 'colors', 'index', 'offsets', 'faces',
                                                            'face_offsets'])):
    """``points``, ``colors``, ``index``, ``offsets`` as ``PointCloud``; ``faces`` [F, 3] int32 rows of ``points``,
    ``face_offsets`` [B + 1] int32 (see the module text).  From ``triangle_mesh(..., trim=False)`` the buffers have their
    full capacity, of which only the first ``min(offsets[B], capacity)`` and ``min(face_offsets[B], face_capacity)`` rows
    are defined."""

    def _host(self):
        """Both offset vectors as lists of Python ints.  ``triangle_mesh`` allocates them as one [2, B + 1] tensor: the
        first call on a mesh whose offsets live on the GPU copies that tensor to the host in ONE read, which waits for
        the stream; the lists are kept."""
        cached = self.__dict__.get('_host_both')
        if cached is None:
            both = self.__dict__.get('_both')
            if both is None:
                both = torch.stack([self.offsets, self.face_offsets])
            rows = both.detach().cpu().tolist()
            cached = self.__dict__['_host_both'] = ([int(v) for v in rows[0]], [int(v) for v in rows[1]])
        return cached

    def host_offsets(self):
        """``offsets`` as a list of Python ints (one read for both offset vectors on the first call, then kept)."""
        return self._host()[0]

    def host_face_offsets(self):
        """``face_offsets`` as a list of Python ints (one read for both offset vectors on the first call, then kept)."""
        return self._host()[1]

    def size(self):
        """Rows that hold a vertex: offsets[B], or the buffers' rows where the vertices were cut at ``capacity``."""
        return min(self.host_offsets()[-1], int(self.points.shape[0]))

    def face_count(self):
        """Rows that hold a face: face_offsets[B], or the buffer's rows where the faces were cut at ``face_capacity``."""
        return min(self.host_face_offsets()[-1], int(self.faces.shape[0]))

    def cloud(self):
        """The ``PointCloud`` over the same tensors (``gather``, ``entry``, ``save_ply`` without faces ...); host
        offsets that were read already are shared, not read again."""
        cloud = _pc.PointCloud(self.points, self.colors, self.index, self.offsets)
        if '_host_both' in self.__dict__:
            cloud.__dict__['_host_offsets'] = self.__dict__['_host_both'][0]
        return cloud

    def entry(self, b):
        """``TriangleMeshEntry(points, colors, index, faces)`` of batch entry ``b``: views of the vertices, and the
        entry's faces with ``offsets[b]`` subtracted, so that they index the entry's own points.  Needs the host offsets
        (one read on an untrimmed mesh).  Rows cut off at a capacity are missing."""
        offsets, face_offsets = self._host()
        b = operator.index(b)
        if not 0 <= b < len(offsets) - 1:
            raise IndexError('entry %d of a mesh of %d entries' % (b, len(offsets) - 1))
        points, colors, index = self.cloud().entry(b)
        rows = int(self.faces.shape[0])
        first, last = min(face_offsets[b], rows), min(face_offsets[b + 1], rows)
        return TriangleMeshEntry(points, colors, index, self.faces[first:last] - offsets[b])

    def save_ply(self, path, normals=None, entry=None):
        """Writes the mesh (or batch entry ``entry`` alone) as a binary little-endian PLY: the vertices as the module
        function ``save_ply`` writes a cloud, then ``element face`` with ``property list uchar int vertex_indices``."""
        _pc.save_ply(path, self, normals=normals, entry=entry)


_workspace = _lib.Workspace()


def triangle_mesh(disparity, matrix, image=None, valid=None, confidence=None, min_confidence=0.0, min_depth=None,
                  max_depth=None, max_difference=1.0, flip=False, with_index=False, capacity=None, face_capacity=None,
                  trim=True):
    """Disparity float32 [B, H, W] -> ``TriangleMesh(points, colors, index, offsets, faces, face_offsets)``: the cloud
    ``point_cloud`` gives for the same arguments, and two triangles per 2 x 2 cell of kept pixels whose disparities differ
    by at most ``max_difference`` along every edge (see the module text).

    ``max_difference``: a float >= 0, ``inf`` allowed.  ``flip``: swap the second and third vertex of every face.
    ``capacity``: rows of the vertex buffers (None: B * H * W).  ``face_capacity``: rows of ``faces``; None means
    2 * B * (H - 1) * (W - 1), which can never overflow.  The other arguments are ``point_cloud``'s.

    ``trim=True`` reads both offset vectors in one host read -- the ONLY synchronisation of the call -- and returns
    tensors of exactly N and F rows; it raises if an explicit capacity was too small.  ``trim=False`` returns the
    full-capacity buffers and the device offsets without any synchronisation.  Runs on the current stream, without
    autograd."""
    # what can be judged without a GPU comes first: types, shapes, thresholds
    shape, m, min_confidence, min_depth, max_depth, rows, layout = _pc._host_checks(
        disparity, matrix, image, valid, confidence, min_confidence, min_depth, max_depth, capacity)
    batch, height, width = shape
    max_difference = float(max_difference)
    if math.isnan(max_difference) or max_difference < 0.0:
        raise ValueError('max_difference must be >= 0 and not NaN, got %r' % (max_difference,))
    if not isinstance(flip, (bool, np.bool_)):
        raise TypeError('flip must be a bool, got %r' % (flip,))
    face_rows = _pc._rows(face_capacity, 'face_capacity', 2 * batch * max(height - 1, 0) * max(width - 1, 0))
    if 2 * batch * height * width > 2 ** 31 - 1:
        raise ValueError('triangle_mesh: 2 * B * H * W = %d does not fit 32-bit indices' % (2 * batch * height * width))
    # then where the tensors live
    d, image, valid, confidence = _pc._device_checks('triangle_mesh', disparity, image, valid, confidence)
    c_matrix = _pc._Float16(*m.astype(np.float32).reshape(-1).tolist())
    lib = _lib.load()
    nbytes = int(lib.pds_triangle_mesh_workspace_bytes(batch, height, width))
    if nbytes == 0:
        raise ValueError('triangle_mesh: %s' % lib.pds_last_error().decode(errors='replace'))
    held, face_held = max(rows, 1), max(face_rows, 1)   # (a buffer of no rows has no address)
    points = torch.empty((held, 3), dtype=torch.float32, device=d.device)
    colors = None if image is None else torch.empty((held, 3), dtype=image.dtype, device=d.device)
    index = torch.empty((held,), dtype=torch.int32, device=d.device) if with_index else None
    faces = torch.empty((face_held, 3), dtype=torch.int32, device=d.device)
    both = torch.empty((2, batch + 1), dtype=torch.int32, device=d.device)   # offsets, face_offsets: one host read
    with torch.cuda.device(d.device):
        workspace = _workspace.get(nbytes, d.device)
        _lib.check(lib.pds_triangle_mesh_fwd(
            _lib.ptr(d), None if valid is None else _lib.ptr(valid),
            None if confidence is None else _lib.ptr(confidence), min_confidence, c_matrix, min_depth, max_depth,
            max_difference, int(bool(flip)), None if image is None else _lib.ptr(image), layout, _lib.ptr(points),
            None if colors is None else _lib.ptr(colors), None if index is None else _lib.ptr(index),
            _lib.ptr(both[0]), rows, _lib.ptr(faces), _lib.ptr(both[1]), face_rows, batch, height, width,
            _lib.ptr(workspace), workspace.numel(), _lib.stream_handle(d.device)), 'pds_triangle_mesh_fwd')
    cut = (lambda t, n: None if t is None else t[:n])
    mesh = TriangleMesh(cut(points, rows), cut(colors, rows), cut(index, rows), both[0], cut(faces, face_rows), both[1])
    mesh.__dict__['_both'] = both
    if not trim:
        return mesh
    offsets, face_offsets = mesh._host()   # the one synchronisation
    count, face_count = offsets[-1], face_offsets[-1]
    if count > rows:
        raise RuntimeError('triangle_mesh: %d points do not fit capacity %d (trim=False returns the first %d and the '
                           'true count in offsets)' % (count, rows, rows))
    if face_count > face_rows:
        raise RuntimeError('triangle_mesh: %d faces do not fit face_capacity %d (trim=False returns the first %d and '
                           'the true count in face_offsets)' % (face_count, face_rows, face_rows))
    trimmed = TriangleMesh(cut(points, count), cut(colors, count), cut(index, count), both[0], cut(faces, face_count),
                           both[1])
    trimmed.__dict__['_both'] = both
    trimmed.__dict__['_host_both'] = mesh.__dict__['_host_both']
    return trimmed
