"""CPU: the median filter's entry point (pds_median_filter_fwd) is declared, exported and bound and validates its
arguments without a GPU, and the Python surface (median_filter, StereoRig.reconstruct(median_size=...)) refuses what it
cannot run.

The numpy oracle of tests/test_gpu_median.py lives here and is itself held to hand-written answers, so that a wrong
oracle cannot pass a wrong kernel.  Semantics (include/pds_hip.h): a pixel is eligible iff its disparity is finite and
its `valid` entry, if any, is non-zero; W(p) is the set of eligible pixels of the k x k window around p, clipped at the
border; median(p) is the value of rank (n - 1) // 2 among them (the lower median); an eligible pixel receives it, a
hole only with fill_holes and n >= min_valid."""
import ctypes
import inspect
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch
from numpy.lib.stride_tricks import sliding_window_view

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib

NAN, INF = float('nan'), float('inf')
_pool = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))   # numpy sorts without the GIL


# ------------------------------------------------------------------------------------------------ the oracle
def oracle_parts(disparity, k, valid=None):
    """(median, n, eligible) of one image [H, W]: gather every clipped window, sort it, take rank (n - 1) // 2.
    Samples that are not eligible or lie outside the image are gathered as +inf (an eligible sample is finite), so
    they sort behind the n real ones.  median is arbitrary (+inf) where n == 0."""
    d = np.asarray(disparity, dtype=np.float32)
    assert d.ndim == 2 and k in (3, 5, 7)
    r = k // 2
    eligible = np.isfinite(d)
    if valid is not None:
        eligible &= np.asarray(valid).reshape(d.shape) != 0
    padded = np.full((d.shape[0] + 2 * r, d.shape[1] + 2 * r), np.inf, dtype=np.float32)
    padded[r:r + d.shape[0], r:r + d.shape[1]] = np.where(eligible, d, np.float32(np.inf))
    windows = sliding_window_view(padded, (k, k))   # [H, W, k, k], a view

    def rows(span):
        w = np.array(windows[span[0]:span[1]]).reshape(-1, k * k)   # the gather (a copy)
        w.sort(axis=1)
        n = (w < np.inf).sum(axis=1)
        rank = np.maximum(n - 1, 0) // 2
        return np.take_along_axis(w, rank[:, None], axis=1)[:, 0], n

    step = max(1, (1 << 18) // d.shape[1])
    spans = [(y, min(y + step, d.shape[0])) for y in range(0, d.shape[0], step)]
    parts = list(_pool.map(rows, spans)) if len(spans) > 1 else [rows(spans[0])]
    median = np.concatenate([p[0] for p in parts]).reshape(d.shape)
    n = np.concatenate([p[1] for p in parts]).reshape(d.shape)
    return median, n, eligible


def oracle_finish(parts, k, fill_holes=False, min_valid=None, fill_value=NAN):
    median, n, eligible = parts
    if min_valid is None:
        min_valid = k * k // 2 + 1
    assert 1 <= min_valid <= k * k
    ok = eligible | (bool(fill_holes) & (n >= min_valid))
    return np.where(ok, median, np.float32(fill_value)), ok


def oracle_median(d, k, valid=None, fill_holes=False, min_valid=None, fill_value=NAN):
    """-> (filtered float32 [H, W], ok bool [H, W])."""
    return oracle_finish(oracle_parts(d, k, valid), k, fill_holes, min_valid, fill_value)


def same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32), equal_nan=True)


def test_oracle_3x3_by_hand_with_corners_and_edges():
    d = [[1, 2, 3], [4, 100, 6], [7, 8, 9]]
    # centre: 1 2 3 4 [6] 7 8 9 100; corner (0, 0): {1, 2, 4, 100} -> rank 1; edge (0, 1): {1, 2, 3, 4, 6, 100} -> rank 2
    out, ok = oracle_median(d, 3)
    assert same(out, [[2, 3, 3], [4, 6, 6], [7, 7, 8]]) and ok.all() and ok.dtype == np.bool_
    assert out.dtype == np.float32


def test_oracle_5x5_by_hand_and_the_lower_median_of_an_even_count():
    d = np.arange(25, dtype=np.float32).reshape(5, 5)
    d[2, 2] = 1000.0
    # 0 .. 11, 13 .. 24, 1000: rank 12 is 13
    assert oracle_median(d, 5)[0][2, 2] == 13.0
    # without the 24: 0 .. 11, 13 .. 23, 1000 are 24 samples, ranks 11 and 12 are 11 and 13; the lower one wins
    d[4, 4] = NAN
    out, ok = oracle_median(d, 5)
    assert out[2, 2] == 11.0 and not ok[4, 4] and np.isnan(out[4, 4])
    # k = 3 on the same image, pixel (1, 1): {0, 1, 2, 5, 6, 7, 10, 11, 1000} -> 6
    assert oracle_median(d, 3)[0][1, 1] == 6.0
    # two samples: the smaller (the farther surface) wins
    assert same(oracle_median([[30.0, 10.0]], 3)[0], [[10.0, 10.0]])


def test_oracle_holes_are_filled_from_min_valid_samples_on():
    d = [[1, NAN, 3], [NAN, NAN, NAN], [7, 8, NAN]]
    # the centre sees {1, 3, 7, 8}: n = 4, the lower median is 3
    out, ok = oracle_median(d, 3, fill_holes=True, min_valid=4, fill_value=-1.0)
    assert out[1, 1] == 3.0 and ok[1, 1]
    out, ok = oracle_median(d, 3, fill_holes=True, min_valid=5, fill_value=-1.0)
    assert out[1, 1] == -1.0 and not ok[1, 1]
    out, ok = oracle_median(d, 3, fill_holes=True, fill_value=-1.0)   # the default is 5 of 9
    assert out[1, 1] == -1.0 and not ok[1, 1]
    out, ok = oracle_median(d, 3, fill_holes=False, min_valid=1, fill_value=-1.0)
    assert out[1, 1] == -1.0 and not ok[1, 1]
    # (0, 1) sees {1, 3}; (1, 0) sees {1, 7, 8}; (2, 2) sees {8}
    out, ok = oracle_median(d, 3, fill_holes=True, min_valid=1)
    assert same(out, [[1, 1, 3], [7, 3, 3], [7, 7, 8]]) and ok.all()
    out, ok = oracle_median(d, 3, fill_holes=True, min_valid=3)
    assert same(out, [[1, NAN, 3], [7, 3, NAN], [7, 7, NAN]])
    assert np.array_equal(ok, [[1, 0, 1], [1, 1, 0], [1, 1, 0]])


def test_oracle_an_eligible_pixel_among_holes_keeps_its_value():
    d = np.full((3, 3), NAN, dtype=np.float32)
    d[1, 1] = 42.0
    out, ok = oracle_median(d, 3)
    assert out[1, 1] == 42.0 and int(ok.sum()) == 1 and np.isnan(out).sum() == 8
    out, ok = oracle_median(d, 3, fill_holes=True)   # one sample is no majority
    assert int(ok.sum()) == 1
    out, ok = oracle_median(d, 3, fill_holes=True, min_valid=1)
    assert same(out, np.full((3, 3), 42.0)) and ok.all()
    out, ok = oracle_median(np.full((4, 5), NAN), 5, fill_holes=True, min_valid=1, fill_value=7.0)   # n = 0 everywhere
    assert same(out, np.full((4, 5), 7.0)) and not ok.any()


def test_oracle_leaves_out_non_finite_and_masked_samples():
    d = [[1, INF, 3], [-INF, 5, 6], [7, 8, 9]]
    valid = [[1, 1, 1], [1, 1, 0], [1, 200, 1]]
    # the centre sees {1, 3, 5, 7, 8, 9} (the 6 is masked): rank 2 is 5
    out, ok = oracle_median(d, 3, valid=valid)
    assert out[1, 1] == 5.0
    assert np.array_equal(ok, [[1, 0, 1], [0, 1, 0], [1, 1, 1]])
    assert np.isnan(out[0, 1]) and np.isnan(out[1, 0]) and np.isnan(out[1, 2])
    # (1, 2) is masked; its window holds {3, 5, 8, 9}
    out, ok = oracle_median(d, 3, valid=np.array(valid, dtype=bool), fill_holes=True, min_valid=4)
    assert out[1, 2] == 5.0 and ok[1, 2]
    # without the mask the 6 counts: {1, 3, 5, 6, 7, 8, 9} -> 6
    assert oracle_median(d, 3)[0][1, 1] == 6.0


def test_oracle_image_smaller_than_the_window():
    out, ok = oracle_median([[4, 1], [3, 2]], 7)
    assert same(out, [[2, 2], [2, 2]]) and ok.all()
    out, ok = oracle_median([[4, NAN], [3, 2]], 7, fill_holes=True, min_valid=3)
    assert same(out, [[3, 3], [3, 3]]) and ok.all()
    assert same(oracle_median([[5.5]], 5)[0], [[5.5]])


def test_the_sentinel_identity_for_every_window_population():
    """What the kernel relies on: with n real samples in a window of K = k * k = 2 c + 1, replace the K - n missing ones
    by c - (n - 1) // 2 copies of -inf and the rest by +inf; the lower median of the real samples then has rank c.  That
    count is ceil((K - n) / 2): every second missing sample, beginning with the first."""
    rng = np.random.RandomState(0)
    for k in (3, 5, 7):
        K, c = k * k, (k * k - 1) // 2
        for n in range(1, K + 1):
            low = c - (n - 1) // 2
            assert 0 <= low <= K - n and low == (K - n + 1) // 2, (k, n)
            for trial in range(3):
                real = (rng.randint(0, 4, n) if trial == 0 else rng.randn(n) * 100).astype(np.float32)   # with ties
                padded = np.concatenate([real, np.full(low, -np.inf), np.full(K - n - low, np.inf)]).astype(np.float32)
                assert padded.size == K
                assert np.sort(padded)[c] == np.sort(real)[(n - 1) // 2], (k, n, trial)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_median_symbol_declared_exported_and_bound(hip_library):
    header = open(_lib.HEADER_PATH).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert 'pds_median_filter_fwd(' in header and hasattr(raw, 'pds_median_filter_fwd')
    assert 'pds_median_filter_fwd' in _lib.SIGNATURES
    assert hip_library.pds_abi_version() == 7
    assert 'median_filter' in pds.__all__ and 'MedianFiltered' in pds.__all__
    assert pds.MedianFiltered._fields == ('disparity', 'valid')
    for line in ('median(p)    = the value of rank (n - 1) // 2 (0-based, ascending) among D[W(p)]:  the LOWER median.',
                 '(the window is CLIPPED at the border: nothing is replicated or mirrored)'):
        assert line in pds.median.__doc__
        assert line.replace('//', '/') in header


def test_median_filter_validation_needs_no_gpu(hip_library):
    lib = hip_library
    big = 1 << 20
    d, v, f, o = [ctypes.c_void_p(big * n) for n in range(1, 5)]   # never dereferenced; far apart

    def call(disparity=d, valid=v, filtered=f, ok=o, shape=(1, 2, 3), k=3, fill_holes=0, min_valid=5, fill=math.nan):
        return lib.pds_median_filter_fwd(disparity, valid, filtered, ok, *shape, k, fill_holes, min_valid, fill, None)

    assert call(disparity=None) != 0 and lib.pds_last_error() == b'median_filter: null pointer'
    assert call(filtered=None) != 0 and lib.pds_last_error() == b'median_filter: null pointer'
    for shape in [(0, 2, 3), (1, 0, 3), (1, 2, 0), (-1, 2, 3), (1, -2, 3), (1, 2, -3)]:
        assert call(shape=shape) != 0 and b'median_filter: bad shape' in lib.pds_last_error(), shape
    assert call(shape=(1, 1 << 16, 1 << 16)) != 0 and b'32-bit indices' in lib.pds_last_error()
    assert call(shape=(4, 1 << 15, 1 << 14)) != 0 and b'32-bit indices' in lib.pds_last_error()   # 2^31 in all
    for k in (0, 1, 2, 4, 6, 8, 9, -3):
        assert call(k=k) != 0 and b'median_filter: kernel_size' in lib.pds_last_error(), k
    for k, min_valid in ((3, 0), (3, 10), (3, -1), (5, 26), (7, 50), (7, 0)):
        assert call(k=k, min_valid=min_valid) != 0 and b'median_filter: min_valid' in lib.pds_last_error(), (k, min_valid)
    # neighbours are read: out may not overlap D, ok may not overlap valid, nor anything else
    assert call(filtered=d) != 0 and b'filtered overlaps disparity' in lib.pds_last_error()
    assert call(filtered=ctypes.c_void_p(d.value + 4)) != 0 and b'filtered overlaps disparity' in lib.pds_last_error()
    assert call(filtered=ctypes.c_void_p(d.value - 4)) != 0 and b'filtered overlaps disparity' in lib.pds_last_error()
    assert call(ok=v) != 0 and b'ok overlaps valid' in lib.pds_last_error()
    assert call(ok=ctypes.c_void_p(v.value + 5)) != 0 and b'ok overlaps valid' in lib.pds_last_error()
    assert call(ok=d) != 0 and b'aliases' in lib.pds_last_error()
    assert call(ok=ctypes.c_void_p(f.value + 8)) != 0 and b'aliases' in lib.pds_last_error()
    assert call(filtered=v) != 0 and b'aliases' in lib.pds_last_error()


# ------------------------------------------------------------------------------------------------ Python
def test_median_python_errors():
    ok = torch.zeros(1, 4, 5)
    with pytest.raises(TypeError, match='torch.Tensor'):
        pds.median_filter(np.zeros((1, 4, 5), dtype=np.float32))
    for bad in (torch.zeros(4, 5), torch.zeros(1, 1, 4, 5)):
        with pytest.raises(ValueError, match='dimensions'):
            pds.median_filter(bad)
    for k in (0, 1, 2, 4, 6, 9, -3, np.int64(8)):
        with pytest.raises(ValueError, match='kernel_size must be 3, 5 or 7'):
            pds.median_filter(ok, k)
    for k in (True, 3.0, 2.5, '3', None, (3,)):   # bool is not an integer
        with pytest.raises(TypeError, match='kernel_size must be an integer'):
            pds.median_filter(ok, k)
    for k, min_valid in ((3, 0), (3, 10), (5, 26), (7, 50), (7, -1)):
        with pytest.raises(ValueError, match='min_valid must be in 1 ..'):
            pds.median_filter(ok, k, fill_holes=True, min_valid=min_valid)
    for min_valid in (True, 2.0, '2'):
        with pytest.raises(TypeError, match='min_valid must be an integer'):
            pds.median_filter(ok, 3, min_valid=min_valid)
    with pytest.raises(TypeError, match='fill_holes must be a bool'):
        pds.median_filter(ok, 3, fill_holes='yes')
    with pytest.raises(TypeError, match='valid must be torch.bool or torch.uint8'):
        pds.median_filter(ok, valid=torch.ones(1, 4, 5))
    with pytest.raises(TypeError, match='valid must be a torch.Tensor'):
        pds.median_filter(ok, valid=np.ones((1, 4, 5), dtype=bool))
    with pytest.raises(ValueError, match='differ in shape'):
        pds.median_filter(ok, valid=torch.ones(1, 4, 6, dtype=torch.bool))
    # every argument in order, and still no CPU fallback
    for kwargs in ({}, {'kernel_size': np.int64(7), 'min_valid': 49, 'fill_holes': True, 'fill_value': 0.0},
                   {'valid': torch.ones(1, 4, 5, dtype=torch.bool)}):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            pds.median_filter(ok, **kwargs)
    defaults = inspect.signature(pds.median_filter).parameters
    assert [(n, p.default) for n, p in defaults.items()][1:5] == [('kernel_size', 3), ('valid', None),
                                                                  ('fill_holes', False), ('min_valid', None)]
    assert math.isnan(defaults['fill_value'].default)


def test_reconstruct_takes_the_median_arguments():
    parameters = inspect.signature(pds.StereoRig.reconstruct).parameters
    assert parameters['median_size'].default is None and parameters['median_fill_holes'].default is False
    assert parameters['median_min_valid'].default is None
    # the positional order of the parent commit is unchanged
    assert list(parameters)[:8] == ['self', 'network', 'left', 'right', 'max_difference', 'reverse_channels',
                                    'speckle_size', 'speckle_difference']
    assert 'FILTERED' in pds.StereoRig.reconstruct.__doc__
