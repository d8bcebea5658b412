"""Hole-aware median filter of a disparity map (not in the reference).

The stages behind the network so far only reject pixels (the left-right check and the speckle filter turn them into
NaN, ``reproject`` drops them).  ``median_filter`` repairs the map: it removes single-pixel outliers that sit within the
speckle filter's ``max_difference`` of their neighbours, and with ``fill_holes`` it closes the small holes the two
filters punch, where enough neighbours agree.  OpenCV's ``medianBlur`` (the stage behind ``filterSpeckles`` there) knows
nothing of NaN or masks; this one does.  Per image of the batch:

    k            = kernel_size, one of 3, 5, 7;  r = k // 2
    eligible(q)  = D[q] finite and (valid is None or valid[q] != 0)          (the speckle filter's rule)
    W(p)         = { q : |qx - px| <= r, |qy - py| <= r, q inside the image, eligible(q) }
                   (the window is CLIPPED at the border: nothing is replicated or mirrored)
    n(p)         = |W(p)|                                                      0 .. k*k
    median(p)    = the value of rank (n - 1) // 2 (0-based, ascending) among D[W(p)]:  the LOWER median.
                   No two samples are ever averaged, so the output never invents a disparity between a
                   foreground and a background surface, and for even n the farther surface wins, as in the
                   left-right check's fill.
    out[p], ok[p] =  median(p), 1      if eligible(p)                                   (n >= 1: p is in W)
                     median(p), 1      if not eligible(p) and fill_holes and n(p) >= min_valid
                     fill_value, 0     otherwise
    min_valid    in 1 .. k*k, default k*k // 2 + 1 (a majority of the full window)

``-0.0`` and ``+0.0`` compare equal, and either may be returned when both are in the window; apart from that the output
is one of the window's inputs bit for bit.  One entry point, one launch (``pds_median_filter_fwd``): a selection, not
arithmetic, so the result is exact.  There is no CPU fallback.
"""
import collections
import operator

import torch

from practicaldeepstereo_nips2018_amd import _lib

# median_filter: the filtered disparity, and the mask (torch.bool) of the pixels that hold a median (the others hold
# fill_value)
MedianFiltered = collections.namedtuple('MedianFiltered', ['disparity', 'valid'])

KERNEL_SIZES = (3, 5, 7)


def _index(value):
    """The integer value of ``value``, or None (bool is not an integer here, nor is 3.0)."""
    if isinstance(value, bool):
        return None
    try:
        return operator.index(value)
    except TypeError:
        return None


def _check_kernel_size(kernel_size):
    value = _index(kernel_size)
    if value is None:
        raise TypeError('kernel_size must be an integer (3, 5 or 7), got %r' % (kernel_size,))
    if value not in KERNEL_SIZES:
        raise ValueError('kernel_size must be 3, 5 or 7, got %r' % (kernel_size,))
    return value


def _check_min_valid(min_valid, kernel_size):
    if min_valid is None:
        return kernel_size * kernel_size // 2 + 1
    value = _index(min_valid)
    if value is None:
        raise TypeError('min_valid must be an integer or None, got %r' % (min_valid,))
    if not 1 <= value <= kernel_size * kernel_size:
        raise ValueError('min_valid must be in 1 .. %d for kernel_size %d, got %r'
                         % (kernel_size * kernel_size, kernel_size, min_valid))
    return value


def median_filter(disparity, kernel_size=3, valid=None, fill_holes=False, min_valid=None, fill_value=float('nan')):
    """disparity [batch, H, W] float32 on the GPU -> ``MedianFiltered(disparity, valid)``: the hole-aware lower median
    over a ``kernel_size`` x ``kernel_size`` window (3, 5 or 7; see the module text).  ``valid``: torch.bool or
    torch.uint8 of the same shape and device (e.g. the ``keep`` of ``speckle_filter``), or None; a pixel it rejects is a
    hole like a NaN.  With ``fill_holes`` a hole with at least ``min_valid`` (default: a majority of the full window)
    eligible pixels in its window receives their median.  The returned ``valid`` is torch.bool; the returned disparity
    holds ``fill_value`` (NaN by default, which ``reproject`` treats as "no point") wherever it is False.  Runs on the
    current stream, without autograd."""
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
    kernel_size = _check_kernel_size(kernel_size)
    min_valid = _check_min_valid(min_valid, kernel_size)
    if not isinstance(fill_holes, (bool, int)):
        raise TypeError('fill_holes must be a bool, got %r' % (fill_holes,))
    fill_value = float(fill_value)
    d = _lib.require_gpu_tensor(disparity.detach(), 'disparity', 3)
    if valid is not None:
        if not valid.is_cuda:
            raise RuntimeError('valid must live on an MI355X (cuda) device: the HIP path has no CPU fallback')
        if valid.device != d.device:
            raise ValueError('valid and disparity live on different devices (%s, %s)' % (valid.device, d.device))
        valid = valid.contiguous()
    if d.numel() == 0:
        raise ValueError('median_filter: empty input %s' % (tuple(d.shape),))
    batch, height, width = d.shape
    lib = _lib.load()
    filtered = torch.empty(d.shape, dtype=d.dtype, device=d.device)
    ok = torch.empty(d.shape, dtype=torch.bool, device=d.device)
    with torch.cuda.device(d.device):
        _lib.check(lib.pds_median_filter_fwd(
            _lib.ptr(d), None if valid is None else _lib.ptr(valid), _lib.ptr(filtered), _lib.ptr(ok), batch, height,
            width, kernel_size, 1 if fill_holes else 0, min_valid, fill_value, _lib.stream_handle(d.device)),
            'pds_median_filter_fwd')
    return MedianFiltered(filtered, ok)
