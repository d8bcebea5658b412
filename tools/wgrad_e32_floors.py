"""The fp32 floors quoted in tests/test_gpu_wgrad_layers.py: for every case of its table, the distance of the CPU's fp32
autograd from the fp64 autograd of the same module, inputs and upstream weights (e32), per parameter tensor -- relative to
the tensor's largest entry, and mean error relative to the mean magnitude for the convolution weights -- and the floors
F / F_MEAN that follow, per group of cases (layers.GROUPS: the 2-D modules, the 3-D blocks, the whole hourglass -- whose
ill-conditioned deep levels put its e32 three orders of magnitude above the others'): the largest value of either column
over the group, rounded up to one significant digit.
With -x it also prints, for every layer `expected_wgrad_kernel` sends to wgrad2d_x3, the distance from fp64 of a numpy
emulation of that kernel's number format (`x3_emulation`): the figure that would replace e32 in that kernel's gate if its
arithmetic, and not a bug, kept it from 3 * e32.  (It does not: tests/test_gpu_wgrad_layers.py holds the kernel to the same
3 * e32 as every other; the emulation stays as the yardstick for the day the operands change.)
Needs no GPU:  python tools/wgrad_e32_floors.py [-v] [-x]"""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch   # noqa: E402

from tests import test_gpu_wgrad_layers as layers   # noqa: E402


def round_up(value):
    """`value` rounded up to one significant digit."""
    exponent = math.floor(math.log10(value))
    return math.ceil(value / 10.0 ** exponent - 1e-9) * 10.0 ** exponent


def pow2_scale(bound, target=16384.0):
    """csrc/common.hpp pow2_scale / kHalfTarget: the largest power of two f with f * bound <= target."""
    if not 0.0 < bound < 3.0e38:
        return 1.0
    f = min(max(target / bound, 2.0 ** -60), 2.0 ** 60)
    return 2.0 ** math.floor(math.log2(f))


def split_f16(v):
    """hi = fp16(v), lo = fp16(v - hi), round to nearest even (csrc/wgrad2d_x3.hip split4)."""
    hi = v.to(torch.float32).to(torch.float16)
    lo = (v.to(torch.float32) - hi.to(torch.float32)).to(torch.float16)
    return hi.to(torch.float32), lo.to(torch.float32)


def x3_emulation(case, module, inputs, weights):
    """The weight gradients of the 3x3 convolutions of a 2-D case in the number format of wgrad2d_x3: both operands of
    dW[oc][c][tap] = sum_p dz[oc][p] * xhat[c][p + tap] scaled by a power of two taken from their largest magnitude, split
    into two fp16 parts, hi * lo + lo * hi + hi * hi (the lo * lo term is dropped; a product of two fp16 values is exact in
    fp32) accumulated in fp32 -- here by a float32 matrix product, per batch entry and plane, summed in fp64 like the
    partials of the kernel (the order inside a workgroup's partial differs; only the format is emulated).  xhat and dz
    are those of the fp64 run.  -> {parameter name: emulated gradient (fp64 tensor)}."""
    F = layers.oracle.F
    records, real = [], F.conv2d

    def recording(x, weight, bias=None, **kw):
        out = real(x, weight, bias, **kw)
        if weight.shape[-1] == 3 and kw.get('stride', 1) == 1:
            entry = {'x': x.detach(), 'weight': weight}
            out.register_hook(lambda grad, entry=entry: entry.__setitem__('dz', grad.detach()))
            records.append(entry)
        return out

    F.conv2d = recording
    try:
        layers.cpu_gradients(case, module, inputs, weights, torch.float64)
    finally:
        F.conv2d = real
    out = {}
    for entry in records:
        x, dz = entry['x'], entry['dz']
        sx, sz = pow2_scale(float(x.abs().max())), pow2_scale(float(dz.abs().max()))
        xh, xl = split_f16(x * sx)
        zh, zl = split_f16(dz * sz)
        total = torch.zeros(entry['weight'].shape, dtype=torch.float64)
        for n in range(x.shape[0]):
            cols = [torch.nn.functional.unfold(t[n:n + 1], 3, padding=1)[0] for t in (xh, xl)]   # [c * 9, positions]
            zs = [t[n].reshape(t.shape[1], -1) for t in (zh, zl)]                               # [oc, positions]
            acc = zs[0] @ cols[1].t() + zs[1] @ cols[0].t()     # fp32: the small partial products first, as the kernel
            acc = acc + zs[0] @ cols[0].t()
            total += acc.double().reshape(total.shape)
        # (cpu_gradients casts the parameters: the module's name of a weight is found by its values)
        key = [k for k, v in module.state_dict().items() if v.shape == entry['weight'].shape
               and torch.equal(v.double(), entry['weight'].detach())][0]
        out[key] = out.get(key, 0.0) + total / (sx * sz)
    return out


def main(verbose, emulate=False):
    worst, worst_mean, total = {}, {}, 0.0
    for case in layers.CASES:
        t0 = time.time()
        module = layers.make_module(case)
        inputs, weights = layers.make_inputs(case)
        want, _ = layers.cpu_gradients(case, module, inputs, weights, torch.float64)
        theirs, _ = layers.cpu_gradients(case, module, inputs, weights, torch.float32)
        rows = {name: layers.distance(theirs[name], want[name]) for name in want}
        conv = [name for name in rows if want[name].dim() > 1]
        e32 = [v[0] for v in rows.values()]
        e32_mean = [rows[name][1] for name in conv]
        dt = time.time() - t0
        total += dt
        group = layers.GROUPS[case[0]]
        worst[group] = max(worst.get(group, 0.0), max(e32))
        worst_mean[group] = max(worst_mean.get(group, 0.0), max(e32_mean))
        print('    %-36s %2d tensors  e32 %.1e .. %.1e | mean %.1e .. %.1e   %5.1f s'
              % (layers.case_id(case), len(rows), min(e32), max(e32), min(e32_mean), max(e32_mean), dt))
        if verbose:
            for name, (a, b) in rows.items():
                print('        %-60s %.2e  %.2e' % (name, a, b))
        if emulate and layers.GROUPS[case[0]] == '2-D modules' and case[0] != 'embedding':
            emulated = x3_emulation(case, module, inputs, weights)
            for L in layers.case_layers(case):
                name = L['prefix'] + '.weight' if L['prefix'] + '.weight' in want else L['prefix'] + '.0.weight'
                if layers.expected_wgrad_kernel(L, {}) == layers.X3:
                    a, b = layers.distance(emulated[name], want[name])
                    print('        x3 emulation %-47s %.2e  %.2e   (e32 %.2e  %.2e)' % ((name, a, b) + rows[name]))
    for group in worst:
        print('    %-12s largest e32 %.2e -> F = %.0e;  largest mean %.2e -> F_MEAN = %.0e'
              % (group + ':', worst[group], round_up(worst[group]), worst_mean[group], round_up(worst_mean[group])))
        assert layers.F_FLOOR[group] == round_up(worst[group]) and layers.F_MEAN[group] == round_up(worst_mean[group])
    print('CPU references of the whole table: %.1f s' % total)


if __name__ == '__main__':
    main('-v' in sys.argv[1:], '-x' in sys.argv[1:])
