"""Speckle filter: disparity regions by connected components (not in the reference).

After a left-right check the surviving disparity still holds small isolated blobs (a few occluded pixels that happen to
point back, mismatches on repetitive texture, slivers at depth edges); each is self-consistent, so neither the check nor
the confidence rejects it, and after ``reproject`` it floats in free space.  ``speckle_filter`` removes every region of at
most ``max_size`` pixels, as OpenCV's ``filterSpeckles`` does.  Per image of the batch:

    eligible(p)  = D[p] finite and (valid is None or valid[p] != 0)
    linked(p, q) = p, q eligible horizontal or vertical neighbours and fabsf(D[p] - D[q]) <= max_difference
                   (one fp32 subtraction; per neighbour pair: a smooth ramp is one region)
    region       = connected component of eligible pixels under these links (4-connectivity)
    size[p]      = pixels of p's region, 0 where p is not eligible             (``region_sizes``)
    keep[p]      = eligible(p) and size[p] > max_size       (a region of exactly max_size pixels is removed;
                   max_size = 0 keeps every eligible pixel)
    filtered[p]  = D[p] if keep[p] else fill_value

One entry point does all of it (``pds_speckle_filter_fwd``: a tiled union-find in four launches, integer atomics only, so
the result is exact and the same on every run).  There is no CPU fallback.
"""
import collections
import math
import operator

import torch

from practicaldeepstereo_nips2018_amd import _lib
from practicaldeepstereo_nips2018_amd.consistency import _check_max_difference

# speckle_filter: the disparity with removed pixels set to fill_value, and the mask (torch.bool) of the pixels kept
SpeckleFiltered = collections.namedtuple('SpeckleFiltered', ['disparity', 'keep'])

_workspace = _lib.Workspace()   # labels and counts, 8 bytes per pixel; one buffer per (device, stream), grow-only


def _check_max_size(max_size):
    try:
        value = None if isinstance(max_size, bool) else operator.index(max_size)
    except TypeError:
        value = None
    if value is None or value < 0 or value > 0x7fffffff:
        raise ValueError('max_size must be a non-negative integer (below 2^31), got %r' % (max_size,))
    return value


def _run(name, disparity, valid, max_difference, max_size, fill_value, want_filtered, want_sizes):
    if not isinstance(disparity, torch.Tensor):
        raise TypeError('disparity must be a torch.Tensor')
    if disparity.dim() != 3:
        raise ValueError('disparity must be [batch, H, W], got %d dimensions' % disparity.dim())
    if valid is not None:
        if not isinstance(valid, torch.Tensor):
            raise TypeError('valid must be a torch.Tensor or None')
        if valid.dtype not in (torch.bool, torch.uint8):
            raise TypeError('valid must be torch.bool or torch.uint8, got %s' % (valid.dtype,))
        if valid.shape != disparity.shape:
            raise ValueError('valid %s and disparity %s differ in shape' % (tuple(valid.shape), tuple(disparity.shape)))
    max_difference = _check_max_difference(max_difference)
    max_size = _check_max_size(max_size)
    fill_value = float(fill_value)
    d = _lib.require_gpu_tensor(disparity.detach(), 'disparity', 3)
    if valid is not None:
        if not valid.is_cuda:
            raise RuntimeError('valid must live on an MI355X (cuda) device: the HIP path has no CPU fallback')
        if valid.device != d.device:
            raise ValueError('valid and disparity live on different devices (%s, %s)' % (valid.device, d.device))
        valid = valid.contiguous()
    if d.numel() == 0:
        raise ValueError('%s: empty input %s' % (name, tuple(d.shape)))
    batch, height, width = d.shape
    lib = _lib.load()
    nbytes = _lib.planned_bytes(lib.pds_speckle_filter_workspace_bytes(batch, height, width), name)
    keep = torch.empty(d.shape, dtype=torch.bool, device=d.device)
    filtered = torch.empty_like(d) if want_filtered else None
    sizes = torch.empty(d.shape, dtype=torch.int32, device=d.device) if want_sizes else None
    with torch.cuda.device(d.device):
        ws = _workspace.get(nbytes, d.device)
        _lib.check(lib.pds_speckle_filter_fwd(
            _lib.ptr(d), None if valid is None else _lib.ptr(valid), _lib.ptr(keep),
            None if filtered is None else _lib.ptr(filtered), None if sizes is None else _lib.ptr(sizes),
            batch, height, width, max_difference, max_size, fill_value, _lib.ptr(ws), ws.numel(),
            _lib.stream_handle(d.device)), 'pds_speckle_filter_fwd')
    return keep, filtered, sizes


def speckle_filter(disparity, max_size, max_difference=1.0, valid=None, fill_value=float('nan')):
    """disparity [batch, H, W] float32 on the GPU -> ``SpeckleFiltered(disparity, keep)``: every region (see the module
    text) of at most ``max_size`` pixels is removed.  ``valid``: torch.bool or torch.uint8 of the same shape and device
    (e.g. the mask of ``left_right_check``), or None; a pixel it rejects belongs to no region and splits regions.
    ``keep`` is torch.bool; the returned disparity holds ``fill_value`` (NaN by default, which ``reproject`` treats as
    "no point") wherever ``keep`` is False."""
    keep, filtered, _ = _run('speckle_filter', disparity, valid, max_difference, max_size, fill_value, True, False)
    return SpeckleFiltered(filtered, keep)


def region_sizes(disparity, max_difference=1.0, valid=None):
    """disparity [batch, H, W] float32 on the GPU -> int32 [batch, H, W]: the number of pixels of every pixel's region,
    0 where the pixel is not eligible (for thresholds of one's own, and for display)."""
    return _run('region_sizes', disparity, valid, max_difference, 0, math.nan, False, True)[2]
