"""A/B of the large-kernel-volume convolution (csrc/conv_lk.hip behind ConvolutionFunction, the weight gradient by offset blocks)
against two yardsticks that need no new kernel, forward + backward of ONE layer on 80 000 voxels of u2mkd_amd.synth:

    kernel   ConvolutionFunction on the whole map (the route under test)
    torch    (a) the v1.4.0 formulation on torch's GPU operators: per offset gather -> mm -> index_add_, from the map's rulebook
    blocks   (b) the block composite: the sum of ConvolutionFunction over at-most-31-offset slices of the map on the existing
             engine, torch adds between them

    python tools/ab_conv_lk.py OUT.json [samples]

Per sample one version runs one forward + backward between two device events; the three versions alternate sample by sample
(40 samples each by default); median / min / p90 per version.  The results of the three versions are compared at the size that
is timed.  A shape class "ships" if the kernel's median beats BOTH yardsticks by more than the larger of their min-to-p90
spreads."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from u2mkd_amd.synth import synth_batch
from u2mkd_amd.torchsparse.nn import functional as F

VOXELS = 80000
SHAPES = [  # (name, kernel_size, stride, cin, cout)
    ('k5 4->32', (5, 5, 5), (1, 1, 1), 4, 32),
    ('k5 32->32', (5, 5, 5), (1, 1, 1), 32, 32),
    ('k3x3x5 64->64', (3, 3, 5), (1, 1, 1), 64, 64),
    ('k4s4 32->64', (4, 4, 4), (4, 4, 4), 32, 64),
]
BLOCK = 31


def sub_maps(kmap):
    """the map cut into slices of at most 31 offsets, each a KernelMap of the existing engine"""
    inv = kmap.nbr_inv
    if inv is None:       # symmetric map: materialise the inverse table of the slices from the mirrored forward table
        inv = torch.full((kmap.k, kmap.n_in), -1, dtype=torch.int32, device=kmap.nbr.device)
        F.L.call('u2mkd_kmap_invert', F.L.ptr(kmap.nbr), kmap.n_out, kmap.k, kmap.n_in, F.L.ptr(inv), F.L.stream())
    return [(b0, F.KernelMap(kmap.nbr[b0:b0 + BLOCK].contiguous(), inv[b0:b0 + BLOCK].contiguous(), kmap.n_in, kmap.n_out, False,
                             kmap.out_coords)) for b0 in range(0, kmap.k, BLOCK)]


def forward(version, x, w, kmap, subs, rule):
    if version == 'kernel':
        return F.ConvolutionFunction.apply(x, w, kmap, False)
    if version == 'blocks':
        out = None
        for b0, sub in subs:
            y = F.ConvolutionFunction.apply(x, w[b0:b0 + sub.k], sub, False)
            out = y if out is None else out + y
        return out
    pairs, starts = rule
    out = torch.zeros(kmap.n_out, w.shape[2], device=x.device)
    for k in range(kmap.k):
        lo, hi = starts[k], starts[k + 1]
        if hi > lo:
            out = out.index_add(0, pairs[lo:hi, 1], x[pairs[lo:hi, 0]].mm(w[k]))
    return out


def step(version, x, w, kmap, subs, rule, dy):
    x = x.detach().requires_grad_()
    w = w.detach().requires_grad_()
    y = forward(version, x, w, kmap, subs, rule)
    y.backward(dy)
    return y.detach(), x.grad, w.grad


def timed(*args):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    step(*args)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3      # us


def main():
    assert torch.cuda.is_available(), 'needs a GPU'
    out_path, samples = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 40
    coords = torch.from_numpy(synth_batch(VOXELS, 1, seed=5)['coords']).int().contiguous().cuda()
    result = {'voxels': VOXELS, 'samples': samples, 'unit': 'us per forward + backward', 'shapes': []}
    versions = ('kernel', 'torch', 'blocks')
    for name, ks, st, cin, cout in SHAPES:
        kmap = F.build_kmap(coords, (1, 1, 1), ks, st)
        subs = sub_maps(kmap)
        pairs, nbsizes = kmap.rulebook()
        starts = [0] + torch.cumsum(nbsizes, 0).tolist()
        rule = (pairs.long(), starts)
        g = torch.Generator().manual_seed(cin + cout)
        x = torch.randn(kmap.n_in, cin, generator=g).cuda()
        w = (torch.randn(kmap.k, cin, cout, generator=g) / (kmap.k * cin) ** 0.5).cuda()
        dy = torch.randn(kmap.n_out, cout, generator=g).cuda()
        for _ in range(3):      # warm-up of every version (code objects, schedules, plans, the allocator)
            res = {v: step(v, x, w, kmap, subs, rule, dy) for v in versions}
        diff = {v: [float((a.double() - b.double()).abs().max()) for a, b in zip(res['kernel'], res[v])] for v in versions[1:]}
        times = {v: [] for v in versions}
        for _ in range(samples):
            for v in versions:
                times[v].append(timed(v, x, w, kmap, subs, rule, dy))
        med = {v: float(np.median(t)) for v, t in times.items()}
        spread = {v: float(np.percentile(times[v], 90) - min(times[v])) for v in versions}
        need = max(spread['torch'], spread['blocks'])
        entry = {'shape': name, 'k': kmap.k, 'n_in': kmap.n_in, 'n_out': kmap.n_out, 'pairs': int(pairs.shape[0]),
                 'median_us': med, 'min_us': {v: float(min(t)) for v, t in times.items()},
                 'p90_us': {v: float(np.percentile(t, 90)) for v, t in times.items()}, 'min_to_p90_us': spread,
                 'ships': bool(med['torch'] - med['kernel'] > need and med['blocks'] - med['kernel'] > need),
                 # (the weaker statement, for a class where one yardstick's spread exceeds the other yardstick's whole time)
                 'beats_each_by_its_own_spread': bool(med['torch'] - med['kernel'] > spread['torch']
                                                      and med['blocks'] - med['kernel'] > spread['blocks']),
                 'max_abs_difference_to_kernel': {v: dict(zip(('y', 'dfeats', 'dkernel'), d)) for v, d in diff.items()}}
        result['shapes'].append(entry)
        print(json.dumps(entry))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
