"""Surface normals from disparity: an edge-aware plane fit on the GPU (not in the reference).

Everything else behind the network rejects pixels, repairs them or moves them to another grid; ``surface_normals`` says
how the surface at a pixel is oriented, which a mesher, point-to-plane ICP, a viewer that shades and Poisson
reconstruction ask for.  Finite differences of the dense ``reproject`` output smear across depth edges and their noise
grows with Z^2.  Stereo noise is uniform in disparity, not in depth, and a projective map takes planes to planes: so a
plane is fitted to d(x, y) over a small window, and its image under the matrix is a 3-D plane whose normal is the answer
(``pds_surface_normals_fwd``: one launch, no atomics, no workspace).  With M = ``matrix`` rounded once to float32, per
image and per pixel p = (x0, y0) with d0 = D[p], k = ``kernel_size`` and r = k // 2:

    kept(p)      = reproject keeps p (the same device function): d0 finite and d0 > 0 and W > 0 and (valid is None or
                   valid[p]) and (confidence is None or confidence[p] >= min_confidence)
    eligible(q)  = D[q] finite and D[q] > 0 and (valid is None or valid[q]) and (confidence is None or
                   confidence[q] >= min_confidence)                                      (a NaN confidence fails)
    delta(q)     = D[q] - d0                                                             (ONE fp32 subtraction)
    W(p)         = {q : |qx - x0| <= r, |qy - y0| <= r, q inside the image (CLIPPED, nothing mirrored), eligible(q),
                   |delta(q)| <= max_difference}
    i, j         = qx - x0, qy - y0                                                      (integers)
    n, Si, Sj, Sii, Sij, Sjj = the sums of 1, i, j, i i, i j, j j over W(p)              (integers)
    A = n Sii - Si^2, Bm = n Sij - Si Sj, C = n Sjj - Sj^2, det = A C - Bm^2             (exact integers)
    degenerate(p) = not kept(p) or n < min_valid or det == 0     (det == 0 <=> the pixels of W(p) are collinear)
    Sd, Sid, Sjd = the fp32 sums of delta, i delta, j delta over W(p)
    u = n Sid - Si Sd,  v = n Sjd - Sj Sd
    a = (C u - Bm v) / det,  b = (A v - Bm u) / det,  c0 = (Sd - a Si - b Sj) / n        (the plane delta = a i + b j + c0)
    dh = d0 + c0;  H = M (x0, y0, dh, 1);  X = H[:3] / H[3]      (degenerate too if H[3] <= 0 or not finite)
    t_x = (M[:3, 0] - X M[3, 0]) + a (M[:3, 2] - X M[3, 2])
    t_y = (M[:3, 1] - X M[3, 1]) + b (M[:3, 2] - X M[3, 2])      (the Jacobian of the division, its common 1 / H[3] dropped)
    N = t_x x t_y;  degenerate if |N|^2 is 0 or not finite;  N /= |N|;  N = -N if N . (X - viewpoint) > 0
                   (a component that is -0 is written as +0)

    normals      [B, H, W, 3] float32: a unit vector that faces ``viewpoint``; ``fill_value`` in all three where degenerate
    valid        [B, H, W] bool: not degenerate

The test on delta keeps the fit on p's side of a depth edge.  Membership of W(p), n and the degeneracy test are exact, and
no atomic is involved: the output has the same bits on every run and on every stream, and the images of a batch are
independent.  There is no CPU fallback, no autograd and no synchronisation.
"""
import collections
import ctypes
import math
import operator

import numpy as np
import torch

from practicaldeepstereo_nips2018_amd import _lib

SurfaceNormals = collections.namedtuple('SurfaceNormals', ['normals', 'valid'])

_Float16 = ctypes.c_float * 16
_Float3 = ctypes.c_float * 3


def _gpu_device(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor' % name)
    if not t.is_cuda:
        raise RuntimeError('%s must live on an MI355X (cuda) device: the HIP path has no CPU fallback' % name)
    return t.device


def surface_normals(disparity, matrix, kernel_size=5, max_difference=1.0, valid=None, confidence=None,
                    min_confidence=0.0, min_valid=None, viewpoint=None, fill_value=math.nan):
    """Disparity float32 [B, H, W] -> ``SurfaceNormals(normals, valid)``: per pixel the unit normal of the plane fitted
    to the disparities of its ``kernel_size`` x ``kernel_size`` window (3, 5 or 7), in the frame of ``matrix`` (the 4x4
    of ``reproject``), facing ``viewpoint`` (3 numbers; None: the origin of that frame).  See the module text.

    ``max_difference`` (>= 0, ``inf`` allowed): only window pixels whose disparity is within it of the centre's enter
    the fit.  ``valid`` / ``confidence`` / ``min_confidence``: as ``reproject`` takes them.  ``min_valid``: the fewest
    window pixels a fit needs, 3 .. k * k (None: k * k // 2 + 1).  ``fill_value``: what a pixel without a normal holds.
    Runs on the current stream, without autograd and without any synchronisation."""
    # what can be judged without a GPU comes first: types, shapes, thresholds
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
    if isinstance(kernel_size, bool) or kernel_size not in (3, 5, 7):
        raise ValueError('kernel_size must be 3, 5 or 7, got %r' % (kernel_size,))
    kernel_size = int(kernel_size)
    try:
        max_difference = float(max_difference)
    except (TypeError, ValueError):
        raise TypeError('max_difference must be a number, got %r' % (max_difference,))
    if not max_difference >= 0.0:
        raise ValueError('max_difference must be >= 0 and not NaN, got %r' % (max_difference,))
    min_confidence = float(min_confidence)
    if not math.isfinite(min_confidence):
        raise ValueError('min_confidence must be finite, got %r' % (min_confidence,))
    if min_valid is None:
        min_valid = kernel_size * kernel_size // 2 + 1
    else:
        try:
            min_valid = operator.index(None if isinstance(min_valid, bool) else min_valid)
        except TypeError:
            raise TypeError('min_valid must be an integer or None, got %r' % (min_valid,))
        if not 3 <= min_valid <= kernel_size * kernel_size:
            raise ValueError('min_valid must be in 3 .. %d, got %d' % (kernel_size * kernel_size, min_valid))
    if viewpoint is None:
        view = np.zeros(3)
    else:
        try:
            view = np.asarray(viewpoint, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise TypeError('viewpoint must be a sequence of 3 numbers, got %r' % (viewpoint,))
        if view.size != 3 or not np.all(np.isfinite(view)):
            raise ValueError('viewpoint must hold 3 finite values, got %r' % (viewpoint,))
    fill_value = float(fill_value)
    if valid is not None:
        if not isinstance(valid, torch.Tensor):
            raise TypeError('valid must be a torch.Tensor')
        if valid.dtype != torch.bool or tuple(valid.shape) != shape:
            raise ValueError('valid must be torch.bool %s, got %s %s' % (shape, valid.dtype, tuple(valid.shape)))
    if confidence is not None and tuple(confidence.shape) != shape:
        raise ValueError('confidence %s and disparity %s differ in shape' % (tuple(confidence.shape), shape))
    # then where the tensors live
    d = _lib.require_gpu_tensor(disparity.detach(), 'disparity', 3)
    if d.numel() == 0:
        raise ValueError('surface_normals: empty input %s' % (shape,))
    if valid is not None:
        _gpu_device(valid, 'valid')
        valid = valid.contiguous()
    if confidence is not None:
        confidence = _lib.require_gpu_tensor(confidence.detach(), 'confidence', 3)
    for name, t in (('valid', valid), ('confidence', confidence)):
        if t is not None and t.device != d.device:
            raise ValueError('%s and disparity live on different devices' % name)
    batch, height, width = shape
    c_matrix = _Float16(*m.astype(np.float32).reshape(-1).tolist())
    c_viewpoint = _Float3(*view.astype(np.float32).tolist())
    normals = torch.empty((batch, height, width, 3), dtype=torch.float32, device=d.device)
    good = torch.empty((batch, height, width), dtype=torch.bool, device=d.device)
    lib = _lib.load()
    with torch.cuda.device(d.device):
        _lib.check(lib.pds_surface_normals_fwd(
            _lib.ptr(d), None if valid is None else _lib.ptr(valid),
            None if confidence is None else _lib.ptr(confidence), min_confidence, c_matrix, c_viewpoint, kernel_size,
            max_difference, min_valid, fill_value, _lib.ptr(normals), _lib.ptr(good), batch, height, width,
            _lib.stream_handle(d.device)), 'pds_surface_normals_fwd')
    return SurfaceNormals(normals, good)
