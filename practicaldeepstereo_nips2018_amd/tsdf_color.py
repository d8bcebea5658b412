"""Colour in TSDF fusion: coloured integration, the colours of the extracted surface and of a raycast (not in the
reference).

A single frame already carries the rectified left image into its products (``PointCloud.colors``,
``TriangleMesh.colors``).  ``ColorTsdfVolume`` keeps it through the fusion (KinectFusion, Open3D ``TSDFVolume`` with
colour): a ``TsdfVolume`` with one more tensor, ``color``, float32 [nz, ny, nx, 3], interleaved, 0.0 at the start.  The
colour shares the volume's ``weight``; it has no weight of its own, which is why every frame must bring its image.

``integrate(..., image=...)`` (``pds_tsdf_color_integrate_fwd``).  ``image``: uint8 [B, H, W, 3] or float32 [B, 3, H, W],
the two layouts of ``point_cloud`` and ``remap``; the values are taken as they are, not rescaled.  Per voxel the kernel
makes the decisions of ``TsdfVolume.integrate``, steps 1 to 9 of ``tsdf.py``, through the same device functions, so
``tsdf`` and ``weight`` get the bits a ``TsdfVolume`` fed the same frames holds.  Where the voxel is updated, per
channel, with x the image value at the pixel the Z was read from and W_old the weight before step 9:

    color = fmaf(color, W_old, x * w) / (W_old + w)

A skipped voxel is neither read nor written in any of the three tensors.  No atomics: the same bits on every run and
stream.

``extract_points(..., with_colors=True)`` / ``extract_mesh(..., with_colors=True)`` (``pds_tsdf_color_gather_fwd``).  The
parent's extraction runs as it is; then one kernel reads the ``index`` it returned: row ``index = 3 v + a`` (d = 1 << a)
or ``7 v + (d - 1)`` names the edge from voxel v to ``n = v + offset(d)``, and the row's colour is, per channel,
``fmaf(r, c_n - c_v, c_v)`` with ``r = tsdf[v] / (tsdf[v] - tsdf[n])``, the expression the extraction placed the point
with.  Rows beyond ``min(offsets[1], capacity)`` are not written; no host synchronisation.  ``cloud.colors`` /
``mesh.colors`` are float32 [N, 3], and ``save_ply`` writes them as ``red green blue``.

``raycast(..., with_colors=True)`` -> ``ColorRaycast(depth, normals, colors)`` (``pds_tsdf_color_render_fwd``).  The
parent's raycast runs as it is; then one kernel per pixel, given ``depth``: ``g = o + depth * d`` with the rows and the ray
of steps 1 and 6 of ``tsdf_raycast.py``, the cell ``c_a = min(floor(g_a), n_a - 2)``, and the colour the trilinear
interpolant over the cell's eight corners, in x, then y, then z, each lerp ``fmaf(t, b - a, a)``.  (NaN, NaN, NaN) where
``depth`` is NaN or a corner has ``weight < min_weight``: the rule of the normal, so colour and normal exist at the same
pixels, except where the gradient is zero.

``track_color(disparity, image, matrix, pose, ...)`` tracks a frame against the coloured raycast with a photometric term
beside the point-to-plane one (``tracking.py``).

Out of scope: a colour weight of its own, colour only inside the truncation band, uint8 colour
storage, sparse volumes.  There is no CPU fallback.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from practicaldeepstereo_nips2018_amd import _lib, tsdf as _tsdf, tsdf_raycast as _raycast
from practicaldeepstereo_nips2018_amd.point_cloud import PointCloud
from practicaldeepstereo_nips2018_amd.tsdf import SurfaceMesh, SurfacePoints, TsdfVolume

# depth float32 [B, H, W] (NaN: no surface); normals float32 [B, H, W, 3] or None; colors float32 [B, H, W, 3] or None
ColorRaycast = collections.namedtuple('ColorRaycast', ['depth', 'normals', 'colors'])

_Float5 = ctypes.c_float * 5


def image_layout(image, shape):
    """``image`` for frames of ``shape = (B, H, W)`` -> 1 for uint8 [B, H, W, 3], 0 for float32 [B, 3, H, W] (the
    ``image_layout`` of the entry points); judged without a GPU."""
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
    if size != tuple(shape):
        raise ValueError('image %s does not match disparity %s in (B, H, W)' % (tuple(image.shape), tuple(shape)))
    return layout


class ColorTsdfVolume(TsdfVolume):
    """``ColorTsdfVolume(origin, voxel_size, dims, truncation, max_weight=64.0, device='cuda')``: a ``TsdfVolume`` that
    also fuses the image (see the module text).  ``color`` (float32 [nz, ny, nx, 3]) is public and may be set under the
    rules of ``tsdf`` and ``weight``; ``reset()`` restores 0.0."""

    def reset(self):
        """1.0, 0.0 and colour 0.0 everywhere, in fresh tensors."""
        super(ColorTsdfVolume, self).reset()
        self._color = torch.zeros(self.shape + (3,), dtype=torch.float32, device=self.device)
        return self

    def _color_state(self, t):
        if not isinstance(t, torch.Tensor):
            raise TypeError('color must be a torch.Tensor')
        shape = self.shape + (3,)
        if t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise ValueError('color must be float32 %s, got %s %s' % (shape, t.dtype, tuple(t.shape)))
        if t.device != self.device:
            raise ValueError('color must live on %s, got %s' % (self.device, t.device))
        if not t.is_contiguous():
            raise ValueError('color must be contiguous')
        return t.detach()

    color = property(lambda self: self._color, lambda self, t: setattr(self, '_color', self._color_state(t)))

    def integrate(self, disparity, matrix, pose=None, camera=None, valid=None, confidence=None, min_confidence=0.0,
                  weight_by_confidence=False, image=None):
        """Integrates disparity float32 [B, H, W] and its ``image`` into the volume, entry after entry -> self.  The
        arguments of ``TsdfVolume.integrate``, and ``image``: uint8 [B, H, W, 3] or float32 [B, 3, H, W], required
        (the colour shares the weight, so every frame carries its image); the values are taken as they are.  Runs on
        the current stream, without autograd and without any synchronisation."""
        if image is None:
            raise ValueError('a ColorTsdfVolume needs the image of every frame: the colour shares the weight')
        layout = []
        a = self._integrate_arguments(disparity, matrix, pose, camera, valid, confidence, min_confidence,
                                      weight_by_confidence, host_check=lambda s: layout.append(image_layout(image, s)))
        if not image.is_cuda:
            raise RuntimeError('image must live on an MI355X (cuda) device: the HIP path has no CPU fallback')
        if image.device != self.device:
            raise ValueError('image and the volume live on different devices')
        image = image.detach().contiguous()
        nx, ny, nz = self.dims
        lib = _lib.load()
        nbytes = int(lib.pds_tsdf_integrate_workspace_bytes(a.height, a.width))
        if nbytes == 0:
            raise ValueError('integrate: %s' % lib.pds_last_error().decode(errors='replace'))
        with torch.cuda.device(self.device):
            workspace = _tsdf._workspace.get(nbytes, self.device)
            _lib.check(lib.pds_tsdf_color_integrate_fwd(
                _lib.ptr(a.disparity), None if a.valid is None else _lib.ptr(a.valid),
                None if a.confidence is None else _lib.ptr(a.confidence), a.min_confidence,
                int(bool(weight_by_confidence)), _lib.ptr(image), layout[0], a.matrix, a.transforms, a.camera,
                self.truncation, self.max_weight, _lib.ptr(self._tsdf), _lib.ptr(self._weight), _lib.ptr(self._color),
                nx, ny, nz, a.batch, a.height, a.width, _lib.ptr(workspace), workspace.numel(),
                _lib.stream_handle(self.device)), 'pds_tsdf_color_integrate_fwd')
        return self

    def _gather(self, index, offsets, edges_per_voxel):
        """-> colors float32 [rows of index, 3] (one row where index has none: a buffer of no rows has no address)"""
        rows = int(index.shape[0])
        if not self._color.is_cuda:
            raise RuntimeError('the volume must live on an MI355X (cuda) device: the HIP path has no CPU fallback')
        colors = torch.empty((max(rows, 1), 3), dtype=torch.float32, device=self.device)
        nx, ny, nz = self.dims
        lib = _lib.load()
        with torch.cuda.device(self.device):
            _lib.check(lib.pds_tsdf_color_gather_fwd(
                _lib.ptr(index), _lib.ptr(offsets), edges_per_voxel, _lib.ptr(self._tsdf), _lib.ptr(self._color),
                _lib.ptr(colors), rows, nx, ny, nz, _lib.stream_handle(self.device)), 'pds_tsdf_color_gather_fwd')
        return colors[:rows]

    def extract_points(self, min_weight=1.0, with_normals=True, capacity=None, trim=True, with_colors=True):
        """``TsdfVolume.extract_points`` with ``cloud.colors`` float32 [N, 3] (None without ``with_colors``): the
        parent's entry point, then the gather on the same stream (see the module text).  ``trim=True`` still makes
        exactly one host read."""
        found = super(ColorTsdfVolume, self).extract_points(min_weight=min_weight, with_normals=with_normals,
                                                            capacity=capacity, trim=False)
        cloud = found.cloud
        if with_colors:
            cloud = PointCloud(cloud.points, self._gather(cloud.index, cloud.offsets, 3), cloud.index, cloud.offsets)
        found = SurfacePoints(cloud, found.normals)
        return _tsdf._trimmed_points(found) if trim else found

    def shift(self, delta, leaving=False, min_weight=1.0, with_normals=True, capacity=None, trim=True, with_colors=True):
        """``TsdfVolume.shift`` with ``color`` moved in the same launch; with ``leaving`` and ``with_colors`` the
        leaving cloud carries ``cloud.colors`` float32 [N, 3], gathered from the old state before it is replaced (the
        colours ``extract_points`` gives the same rows).  ``trim=True`` still makes exactly one host read."""
        return self._shift(delta, leaving, min_weight, with_normals, capacity, trim, bool(with_colors))

    def _leaving_surface(self, delta, min_weight, with_normals, rows, with_colors):
        found = super(ColorTsdfVolume, self)._leaving_surface(delta, min_weight, with_normals, rows, False)
        if not with_colors:
            return found
        cloud = found.cloud
        return SurfacePoints(PointCloud(cloud.points, self._gather(cloud.index, cloud.offsets, 3), cloud.index,
                                        cloud.offsets), found.normals)

    def _state_tensors(self):
        return self._tsdf, self._weight, self._color

    def _shift_state(self, delta):
        self._color = super(ColorTsdfVolume, self)._shift_state(delta)

    def extract_mesh(self, min_weight=1.0, with_normals=True, capacity=None, face_capacity=None, trim=True,
                     with_colors=True):
        """``TsdfVolume.extract_mesh`` with ``mesh.colors`` float32 [N, 3] (None without ``with_colors``): the parent's
        entry point, then the gather on the same stream (see the module text).  ``trim=True`` still makes exactly one
        host read."""
        from practicaldeepstereo_nips2018_amd.mesh import TriangleMesh
        found = super(ColorTsdfVolume, self).extract_mesh(min_weight=min_weight, with_normals=with_normals,
                                                          capacity=capacity, face_capacity=face_capacity, trim=False)
        mesh = found.mesh
        if with_colors:
            colored = TriangleMesh(mesh.points, self._gather(mesh.index, mesh.offsets, 7), mesh.index, mesh.offsets,
                                   mesh.faces, mesh.face_offsets)
            colored.__dict__['_both'] = mesh.__dict__['_both']
            mesh = colored
        found = SurfaceMesh(mesh, found.normals)
        return _tsdf._trimmed_mesh(found) if trim else found

    def raycast(self, camera, size, pose=None, min_weight=1.0, step=None, near=0.0, far=math.inf, with_normals=True,
                with_colors=True):
        """``TsdfVolume.raycast`` -> ``ColorRaycast(depth, normals, colors)``: ``colors`` float32 [B, H, W, 3], the
        trilinear interpolant of ``color`` at the surface, (NaN, NaN, NaN) where there is no surface or the cell has an
        unobserved corner; None without ``with_colors``.  ``depth`` and ``normals`` are those of the parent, bit for
        bit: its raycast runs first, then one kernel per pixel on the same stream (see the module text)."""
        cast = _raycast.raycast(self, camera, size, pose=pose, min_weight=min_weight, step=step, near=near, far=far,
                                with_normals=with_normals)
        if not with_colors:
            return ColorRaycast(cast.depth, cast.normals, None)
        if not self._color.is_cuda:
            raise RuntimeError('the volume must live on an MI355X (cuda) device: the HIP path has no CPU fallback')
        batch, height, width = cast.depth.shape
        rows = self.rays(pose, batch).astype(np.float32)
        c_rays = (ctypes.c_float * (12 * batch))(*rows[:, :12].reshape(-1).tolist())
        c_camera = _Float5(*np.asarray(camera, dtype=np.float64).reshape(-1).astype(np.float32).tolist())
        colors = torch.empty((batch, height, width, 3), dtype=torch.float32, device=self.device)
        nx, ny, nz = self.dims
        lib = _lib.load()
        with torch.cuda.device(self.device):
            _lib.check(lib.pds_tsdf_color_render_fwd(
                _lib.ptr(self._weight), _lib.ptr(self._color), nx, ny, nz, c_rays, c_camera, float(min_weight),
                _lib.ptr(cast.depth), _lib.ptr(colors), batch, height, width, _lib.stream_handle(self.device)),
                'pds_tsdf_color_render_fwd')
        return ColorRaycast(cast.depth, cast.normals, colors)

    def track_color(self, disparity, image, matrix, pose, levels=1, huber=None, color_huber=None, color_weight=1e-3, **kw):
        """``track_pyramid`` with a photometric term on the coloured raycast -> ``ColorTracking(pose, rmse, inliers,
        iterations, status, color_rmse, color_inliers)`` (see ``tracking``).  ``image``: the frame's image as ``integrate``
        takes it, uint8 [B, H, W, 3] or float32 [B, 3, H, W].  ``kw``: the other keywords of ``track`` and
        ``max_difference``.  Per iteration one launch forms the point-to-plane and the photometric system
        (``icp_color_system``), and the host solves A + w^2 A_c, g + w^2 g_c with ``w = color_weight`` in metres per
        intensity level: the default 1e-3 equates 5 levels of a 0 .. 255 image with 5 mm; an image in 0 .. 1 wants 0.255.
        ``huber`` / ``color_huber``: the Huber thresholds of the two kinds of rows, in metres and in intensity levels.
        A textured wall, which ``track`` refuses as ``DEGENERATE``, is tracked; ``color_weight=0, levels=1`` is
        ``track_pyramid(levels=1)``, byte for byte.  A frame that cannot be tracked says so in ``status``."""
        from practicaldeepstereo_nips2018_amd import tracking
        return tracking.track_color(self, disparity, image, matrix, pose, levels=levels, huber=huber,
                                    color_huber=color_huber, color_weight=color_weight, **kw)
