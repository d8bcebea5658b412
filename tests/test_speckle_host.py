"""CPU: the speckle filter's entry points (pds_speckle_filter_workspace_bytes, pds_speckle_filter_fwd) are declared,
exported and bound, validate their arguments without a GPU, and the Python surface (speckle_filter, region_sizes,
StereoRig.reconstruct(speckle_size=...)) refuses what it cannot run.

The numpy oracle of tests/test_gpu_speckle.py lives here and is itself held to hand-written answers, so that a wrong
oracle cannot pass a wrong kernel.  Semantics (include/pds_hip.h): a pixel is eligible iff its disparity is finite and
its `valid` entry, if any, is non-zero; eligible 4-neighbours are linked iff fabsf(D[p] - D[q]) <= max_difference in fp32;
a region is a connected component; size = its pixels, 0 where not eligible; keep = size > max_size."""
import ctypes
import math

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib

NEW_SYMBOLS = ['pds_speckle_filter_workspace_bytes', 'pds_speckle_filter_fwd']
NAN, INF = float('nan'), float('inf')


# ------------------------------------------------------------------------------------------------ the oracle
def links(disparity, valid=None, max_difference=1.0):
    """(eligible [H, W], a, b): flat indices of the two ends of every link."""
    d = np.asarray(disparity, dtype=np.float32)
    assert d.ndim == 2
    height, width = d.shape
    eligible = np.isfinite(d)
    if valid is not None:
        eligible &= np.asarray(valid).reshape(d.shape) != 0
    t = np.float32(max_difference)
    index = np.arange(height * width).reshape(height, width)
    with np.errstate(invalid='ignore'):   # inf - inf
        across = eligible[:, 1:] & eligible[:, :-1] & (np.abs(d[:, 1:] - d[:, :-1]) <= t)
        down = eligible[1:] & eligible[:-1] & (np.abs(d[1:] - d[:-1]) <= t)
    a = np.concatenate([index[:, 1:][across], index[1:][down]])
    b = np.concatenate([index[:, :-1][across], index[:-1][down]])
    return eligible, a, b


def oracle_sizes(disparity, valid=None, max_difference=1.0):
    """int32 [H, W]: hook-and-jump union-find over the links, then the population of every label."""
    eligible, a, b = links(disparity, valid, max_difference)
    n = eligible.size
    label = np.arange(n)
    while True:
        la, lb = label[a], label[b]
        if np.array_equal(la, lb):
            break
        m = np.minimum(la, lb)
        np.minimum.at(label, la, m)   # hook: the larger label of a link points at the smaller one
        np.minimum.at(label, lb, m)
        while True:                   # jump
            jumped = label[label]
            if np.array_equal(jumped, label):
                break
            label = jumped
    sizes = np.bincount(label, minlength=n)[label].reshape(eligible.shape)
    sizes[~eligible] = 0
    return sizes.astype(np.int32)


def oracle_filter(disparity, max_size, valid=None, max_difference=1.0, fill_value=NAN):
    d = np.asarray(disparity, dtype=np.float32)
    keep = oracle_sizes(d, valid, max_difference) > max_size
    return np.where(keep, d, np.float32(fill_value)), keep


# hand-written cases: (disparity rows, valid rows or None, max_difference, expected sizes)
BLOBS = ([[1, 1, 1, 1, 1, 1, 1, 1],
          [1, 9, 9, 1, 1, 1, 1, 1],
          [1, 9, 1, 1, 1, 20, 20, 1],
          [1, 1, 1, 1, 1, 20, 20, 1],
          [1, 1, 1, 1, 1, 1, 1, 1],
          [1, 1, 1, 1, 1, 1, 1, 1]],
         [[41, 41, 41, 41, 41, 41, 41, 41],
          [41, 3, 3, 41, 41, 41, 41, 41],
          [41, 3, 41, 41, 41, 4, 4, 41],
          [41, 41, 41, 41, 41, 4, 4, 41],
          [41, 41, 41, 41, 41, 41, 41, 41],
          [41, 41, 41, 41, 41, 41, 41, 41]])
JUST_ABOVE_ONE = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
KNOWN = {
    'blobs': (BLOBS[0], None, 1.0, BLOBS[1]),
    'one apart is linked': ([[4.0, 5.0]], None, 1.0, [[2, 2]]),
    'a hair more is not': ([[0.0, JUST_ABOVE_ONE]], None, 1.0, [[1, 1]]),
    'ramp': ([[0.9 * k for k in range(12)]], None, 1.0, [[12] * 12]),
    'diagonal neighbours': ([[5, 50, 5], [50, 5, 50], [5, 50, 5]], None, 1.0, [[1, 1, 1], [1, 1, 1], [1, 1, 1]]),
    'non-finite pixels split': ([[2, NAN, 2, 2], [2, INF, 2, 2], [2, -INF, 2, 2], [2, 2, 2, INF]], None, 1.0,
                                [[12, 0, 12, 12], [12, 0, 12, 12], [12, 0, 12, 12], [12, 12, 12, 0]]),
    'a wall of non-finite pixels': ([[2, NAN, 2], [2, INF, 2], [2, -INF, 2]], None, 1.0, [[3, 0, 3], [3, 0, 3], [3, 0, 3]]),
    'valid splits too': ([[2, 2, 2], [2, 2, 2]], [[1, 0, 1], [1, 0, 255]], 1.0, [[2, 0, 2], [2, 0, 2]]),
    'max_difference zero': ([[1, 1, 2], [1, 2, 2]], None, 0.0, [[3, 3, 3], [3, 3, 3]]),
}


def test_oracle_on_hand_written_answers():
    for name, (d, valid, md, expected) in KNOWN.items():
        got = oracle_sizes(np.array(d, dtype=np.float32), None if valid is None else np.array(valid), md)
        assert got.dtype == np.int32 and np.array_equal(got, np.array(expected)), (name, got)
    d = np.array(BLOBS[0], dtype=np.float32)
    for max_size, kept in ((0, 48), (2, 48), (3, 45), (4, 41), (41, 0)):   # size == max_size is removed
        filtered, keep = oracle_filter(d, max_size, fill_value=-1.0)
        assert int(keep.sum()) == kept, (max_size, int(keep.sum()))
        assert np.array_equal(filtered[keep], d[keep]) and np.all(filtered[~keep] == -1.0)


def test_oracle_labels_travel_across_the_image():
    """A serpentine and a comb: one region however long the path, the rest in pieces of known size."""
    d = np.full((9, 7), 50.0, dtype=np.float32)
    d[0::2] = 5.0
    d[1::4, -1] = 5.0
    d[3::4, 0] = 5.0
    sizes = oracle_sizes(d)
    assert np.all(sizes[d == 5.0] == 5 * 7 + 4) and np.all(sizes[d == 50.0] == 6)
    comb = np.full((6, 9), 50.0, dtype=np.float32)
    comb[:, 0::2] = 5.0
    comb[-1] = 5.0
    sizes = oracle_sizes(comb)
    assert np.all(sizes[comb == 5.0] == 5 * 5 + 9) and np.all(sizes[comb == 50.0] == 5)


def test_oracle_against_scipy():
    csgraph = pytest.importorskip('scipy.sparse.csgraph')
    sparse = pytest.importorskip('scipy.sparse')
    rng = np.random.RandomState(5)
    for shape, md in (((40, 70), 1.0), ((40, 70), 8.0), ((1, 50), 4.0), ((33, 1), 4.0)):
        d = (rng.rand(*shape) * 16).astype(np.float32)
        d[rng.rand(*shape) < 0.05] = np.nan
        valid = rng.rand(*shape) > 0.1
        eligible, a, b = links(d, valid, md)
        graph = sparse.coo_matrix((np.ones(a.size), (a, b)), shape=(d.size, d.size))
        _, label = csgraph.connected_components(graph, directed=False)
        expected = np.bincount(label)[label].reshape(shape)
        expected[~eligible] = 0
        assert np.array_equal(oracle_sizes(d, valid, md), expected), (shape, md)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_speckle_symbols_declared_exported_and_bound(hip_library):
    header = open(_lib.HEADER_PATH).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + '(' in header, name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert hip_library.pds_abi_version() == 7
    assert 'speckle_filter' in pds.__all__ and 'region_sizes' in pds.__all__


def test_speckle_workspace_bytes(hip_library):
    lib = hip_library
    query = lib.pds_speckle_filter_workspace_bytes
    base = query(1, 540, 960)
    assert base >= 8 * 540 * 960
    assert query(2, 540, 960) > base and query(1, 541, 960) > base and query(1, 540, 961) > base
    assert query(1, 1, 1) > 0
    previous = 0
    for k in range(1, 6):   # monotone in each argument
        assert query(k, 7, 5) > previous
        previous = query(k, 7, 5)
    assert query(4, 375, 1242) >= 4 * query(1, 375, 1242) - 4 * 256
    for shape in [(0, 2, 3), (1, 0, 3), (1, 2, 0), (-1, 2, 3), (1, -2, 3), (1, 2, -3)]:
        assert query(*shape) == 0 and b'speckle_filter: bad shape' in lib.pds_last_error(), shape
    assert query(1, 1 << 16, 1 << 16) == 0 and b'32-bit labels' in lib.pds_last_error()
    assert query(1, 1 << 15, 1 << 16) == 0 and b'32-bit labels' in lib.pds_last_error()     # 2^31 pixels
    assert query(4, 1 << 15, 1 << 14) == 0 and b'32-bit indices' in lib.pds_last_error()    # 2^29 each, 2^31 in all


def test_speckle_filter_validation_needs_no_gpu(hip_library):
    lib = hip_library
    big = 1 << 20
    d, v, k, f, s, ws = [ctypes.c_void_p(big * n) for n in range(1, 7)]   # never dereferenced; far apart
    need = lib.pds_speckle_filter_workspace_bytes(1, 2, 3)
    assert need > 0

    def call(disparity=d, valid=v, keep=k, filtered=f, sizes=s, shape=(1, 2, 3), md=1.0, max_size=2, fill=math.nan,
             workspace=ws, ws_bytes=need):
        return lib.pds_speckle_filter_fwd(disparity, valid, keep, filtered, sizes, *shape, md, max_size, fill,
                                          workspace, ws_bytes, None)

    assert call(disparity=None) != 0 and lib.pds_last_error() == b'speckle_filter: null pointer'
    assert call(keep=None) != 0 and lib.pds_last_error() == b'speckle_filter: null pointer'
    assert call(workspace=None) != 0 and lib.pds_last_error() == b'speckle_filter: null pointer'
    for shape in [(0, 2, 3), (1, 0, 3), (1, 2, 0), (-1, 2, 3)]:
        assert call(shape=shape) != 0 and b'speckle_filter: bad shape' in lib.pds_last_error(), shape
    assert call(shape=(1, 1 << 16, 1 << 16)) != 0 and b'32-bit labels' in lib.pds_last_error()
    assert call(shape=(4, 1 << 15, 1 << 14)) != 0 and b'32-bit indices' in lib.pds_last_error()
    for md in [-1.0, -1e-30, math.nan, math.inf, -math.inf]:
        assert call(md=md) != 0 and b'speckle_filter: max_difference' in lib.pds_last_error(), md
    for max_size in [-1, -(1 << 31)]:
        assert call(max_size=max_size) != 0 and b'speckle_filter: max_size' in lib.pds_last_error(), max_size
    assert call(ws_bytes=need - 1) != 0 and b'speckle_filter: workspace too small' in lib.pds_last_error()
    assert call(ws_bytes=0) != 0 and b'speckle_filter: workspace too small' in lib.pds_last_error()
    # the alias contract: filtered may be disparity itself, nothing else may overlap
    assert call(filtered=ctypes.c_void_p(d.value + 4)) != 0 and b'filtered overlaps disparity' in lib.pds_last_error()
    assert call(keep=d) != 0 and b'aliases' in lib.pds_last_error()
    assert call(sizes=d) != 0 and b'aliases' in lib.pds_last_error()
    assert call(keep=v) != 0 and b'aliases' in lib.pds_last_error()
    assert call(sizes=f) != 0 and b'aliases' in lib.pds_last_error()
    assert call(keep=ctypes.c_void_p(s.value + 8)) != 0 and b'aliases' in lib.pds_last_error()


# ------------------------------------------------------------------------------------------------ Python
def test_speckle_python_errors():
    ok = torch.zeros(1, 4, 5)
    for fn in (lambda *a, **kw: pds.speckle_filter(a[0], 3, *a[1:], **kw), pds.region_sizes):
        with pytest.raises(TypeError, match='torch.Tensor'):
            fn(np.zeros((1, 4, 5), dtype=np.float32))
        with pytest.raises(ValueError, match='dimensions'):
            fn(torch.zeros(4, 5))
        with pytest.raises(ValueError, match='dimensions'):
            fn(torch.zeros(1, 1, 4, 5))
        for md in [-0.5, math.nan, math.inf]:
            with pytest.raises(ValueError, match='max_difference'):
                fn(ok, max_difference=md)
        with pytest.raises(TypeError, match='valid must be torch.bool or torch.uint8'):
            fn(ok, valid=torch.ones(1, 4, 5))
        with pytest.raises(TypeError, match='valid must be a torch.Tensor'):
            fn(ok, valid=np.ones((1, 4, 5), dtype=bool))
        with pytest.raises(ValueError, match='differ in shape'):
            fn(ok, valid=torch.ones(1, 4, 6, dtype=torch.bool))
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            fn(ok)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            fn(ok, valid=torch.ones(1, 4, 5, dtype=torch.bool))
    for max_size in [-1, 2.5, 3.0, '3', None, True, 1 << 31]:
        with pytest.raises(ValueError, match='max_size must be a non-negative integer'):
            pds.speckle_filter(ok, max_size)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pds.speckle_filter(ok, np.int64(3), fill_value=0.0)
    with pytest.raises(TypeError):
        pds.speckle_filter(ok)   # max_size has no default
    assert pds.SpeckleFiltered._fields == ('disparity', 'keep')


def test_reconstruct_takes_the_speckle_arguments():
    import inspect
    parameters = inspect.signature(pds.StereoRig.reconstruct).parameters
    assert parameters['speckle_size'].default is None and parameters['speckle_difference'].default == 1.0
    # the positional order of the parent commit is unchanged
    assert list(parameters)[:6] == ['self', 'network', 'left', 'right', 'max_difference', 'reverse_channels']
