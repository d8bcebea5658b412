"""In-situ duration of the conv2d_t8w launch (the 64 -> 8 layer that ends Matching) inside sequential pairs of the hot
path (launch probe), for A/B runs of library variants (PDS_HIP_LIB=build/variants/libpds_NAME.so):
    python tools/t8w_in_situ.py [launches]
One launch per pair; the first two pairs warm up.  Prints one line: mean, min, max in microseconds."""
import ctypes, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from practicaldeepstereo_nips2018_amd import _lib

pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 30
dev = torch.device('cuda:0')
net, descriptors, images = bench.make_inputs(dev)
reg, est = net._regularization, net._estimator
lib = _lib.load()


def run_pair(i):
    ld, rd, sc = descriptors[i % bench.PAIRS]
    return reg.forward_with_estimator(net._matching(ld, rd), sc, est)


with torch.no_grad():
    for i in range(2):
        run_pair(i)
    torch.cuda.synchronize(dev)
    capacity = 256
    _lib.check(lib.pds_probe_begin(b'conv2d_t8w', capacity), 'pds_probe_begin')
    t0 = time.perf_counter()
    for i in range(pairs):
        run_pair(i)
    ms = (ctypes.c_float * capacity)()
    wgs = (ctypes.c_int * capacity)()
    n = lib.pds_probe_end(ms, wgs, capacity)
    torch.cuda.synchronize(dev)
    seq = (time.perf_counter() - t0) / pairs * 1e3
if n < 0:
    _lib.check(n, 'pds_probe_end')
times = sorted(ms[i] * 1e3 for i in range(n))
tiles = sorted(set(wgs[i] for i in range(n)))
if not times:
    print('%-28s no conv2d_t8w launch seen' % os.path.basename(os.environ.get('PDS_HIP_LIB', 'tree')))
    sys.exit(1)
print('%-28s t8w in situ %.1f us (min %.1f, median %.1f, max %.1f, %d launches, tiles %s)   sequential pair %.3f ms' % (
    os.path.basename(os.environ.get('PDS_HIP_LIB', 'tree')), sum(times) / len(times), times[0], times[len(times) // 2],
    times[-1], len(times), tiles, seq))
