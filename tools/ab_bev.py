"""A/B of the four BEV modules of the torchsparse drop-in (csrc/bev.hip + the conv engine) against the upstream text on torch's GPU
operators -- what torchsparse v1.4.0 runs: ``torch.sparse_coo_tensor(...).coalesce()`` / ``.to_dense()``, ``index_select`` of the
kernel into an [N, Cin, Cout] tensor, ``permute`` + ``view``, with its ``.item()`` for the batch size -- forward + backward at one
detection-like size: B = 2 x 40 000 rows, a 128 x 128 grid, Z = n_kernels = 5, C = Cout = 64.

    python tools/ab_bev.py OUT.json [samples]        the A/B: device events, versions alternated, medians with min and p90
    python tools/ab_bev.py --kernels [iterations]    the dense modules' kernel route alone, for a kernel trace (rocprofv3 --kernel-trace)

Per sample one version runs one forward + backward between two device events (the yardstick's host read is inside its window);
the versions alternate sample by sample.  The outputs of the two versions are compared at the size that is timed.  BYTES of the
dense store / gather: ``store_bytes`` -- the rows read (and the slot table), every element of the NCHW tensor written once; the
gather moves the same bytes the other way."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from u2mkd_amd import torchsparse as ts
from u2mkd_amd.torchsparse import nn as spnn

ROWS, SCENES, GRID, Z, C = 40000, 2, 128, 5, 64
DIM, BEV = 1, [0, 2]
SHAPE = (GRID, Z, GRID)
MODULES = ('reduction', 'convolution', 'dense', 'height')


def make(seed=0):
    g = torch.Generator().manual_seed(seed)
    coords = []
    for b in range(SCENES):       # 40 000 of the 128 x 128 x 5 slots of every scene: a (cell, height) pair holds one row
        slot = torch.randperm(GRID * GRID * Z, generator=g)[:ROWS]
        coords.append(torch.stack([slot // (GRID * Z), slot % Z, (slot // Z) % GRID, torch.full_like(slot, b)], 1))
    coords = torch.cat(coords).int().contiguous().cuda()
    return coords, torch.randn(ROWS * SCENES, C, generator=g).cuda()


def module(name):
    torch.manual_seed(1)
    if name == 'reduction':
        return spnn.ToBEVReduction(DIM)
    if name == 'convolution':
        return spnn.ToBEVConvolution(C, C, Z, dim=DIM, bias=True).cuda()
    if name == 'dense':
        return spnn.ToDenseBEVConvolution(C, C, SHAPE, dim=DIM, bias=True).cuda()
    return spnn.ToBEVHeightCompression(C, SHAPE, dim=DIM).cuda()


def _coalesced_rows(coords_t, feats):
    t = torch.sparse_coo_tensor(coords_t, feats).coalesce()
    return t.values()


def upstream(name, mod, feats, coords):
    """torchsparse v1.4.0's forward of the module, on torch operators (stride 1, offset 0)"""
    if name == 'reduction':
        c = coords.clone()
        c[:, DIM] = 0
        f = _coalesced_rows(c.t().long(), torch.cat([torch.ones_like(feats[:, :1]), feats], 1))
        return f[:, 1:] / f[:, :1]
    if name == 'height':
        c = coords.t()[[3] + BEV + [DIM]].long()
        c[-1] = torch.clamp(c[-1], 0, Z - 1)
        idx = c[0] * (GRID * GRID * Z) + c[1] * (GRID * Z) + c[2] * Z + c[3]
        batch_size = c[0].max().item() + 1
        bev = torch.sparse_coo_tensor(idx[None], feats, torch.Size([batch_size * GRID * GRID * Z, feats.size(-1)])).to_dense()
        bev = bev.view(batch_size, GRID, GRID, Z, -1)
        return bev.permute(0, 4, 3, 1, 2).contiguous().view(batch_size, -1, GRID, GRID)
    kernels = torch.index_select(mod.kernel, 0, coords[:, DIM].long())
    y = (feats.unsqueeze(-1) * kernels).sum(1) + mod.bias
    if name == 'convolution':
        c = coords.t().long().clone()
        c[DIM, :] = 0
        return _coalesced_rows(c, y)
    c = coords.t()[[3] + BEV].long()
    idx = c[0] * (GRID * GRID) + c[1] * GRID + c[2]
    batch_size = c[0].max().item() + 1
    bev = torch.sparse_coo_tensor(idx[None], y, torch.Size([batch_size * GRID * GRID, y.size(-1)])).to_dense()
    return bev.view(batch_size, GRID, GRID, -1).permute(0, 3, 1, 2).contiguous()


def step(version, name, mod, coords, x, dy=None):
    x = x.detach().requires_grad_()
    mod.zero_grad(set_to_none=True)
    if version == 'kernels':
        y = mod(ts.SparseTensor(x, coords))
        y = y.feats if name in ('reduction', 'convolution') else y
    else:
        y = upstream(name, mod, x, coords)
    if dy is None:
        return y.detach()
    y.backward(dy)
    grads = [x.grad] + [p.grad for p in mod.parameters()]
    return [y.detach()] + grads


def timed(*args):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    step(*args)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3      # us


def store_bytes(name):
    n, cells = ROWS * SCENES, SCENES * GRID * GRID
    if name == 'dense':          # [cells, C] rows in, [B, C, H, W] out
        return 2 * cells * C * 4
    return n * C * 4 + (cells * Z + 1) * 4 + n * 4 + cells * Z * C * 4      # rows, seg, order in; [B, C * Z, H, W] out


def main():
    assert torch.cuda.is_available(), 'needs a GPU'
    coords, x = make()
    if sys.argv[1] == '--kernels':
        iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
        for name in ('dense', 'height'):
            mod = module(name)
            dy = torch.randn_like(step('kernels', name, mod, coords, x))
            for _ in range(iters):
                step('kernels', name, mod, coords, x, dy)
        torch.cuda.synchronize()
        return
    out, samples = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 40
    result = {'rows_per_scene': ROWS, 'scenes': SCENES, 'grid': GRID, 'heights': Z, 'c': C, 'samples': samples,
              'unit': 'us per forward + backward', 'modules': []}
    for name in MODULES:
        mod = module(name)
        dy = torch.randn_like(step('kernels', name, mod, coords, x))
        sparse = name in ('reduction', 'convolution')
        if sparse:      # the two versions order their rows differently ((b, x, y, z) here, (x, y, z, b) upstream): one dy row for all
            dy = dy[:1].expand_as(dy).contiguous()
        for _ in range(5):      # warm-up of both versions (code objects, the plan, the allocator)
            ref = step('upstream', name, mod, coords, x, dy)
            got = step('kernels', name, mod, coords, x, dy)
        if sparse:              # ... and the results are compared by their column sums
            got[0], ref[0] = got[0].double().sum(0), ref[0].double().sum(0)
        diff = [float((a.double() - b.double()).abs().max()) for a, b in zip(got, ref)]
        times = {'kernels': [], 'upstream': []}
        for _ in range(samples):
            for version in ('kernels', 'upstream'):
                times[version].append(timed(version, name, mod, coords, x, dy))
        plan_us = []
        for _ in range(10):      # the plan of a FRESH coordinate tensor: once per batch, its one host read inside
            fresh = coords.clone()
            a0, b0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a0.record()
            step('kernels', name, mod, fresh, x)
            b0.record()
            b0.synchronize()
            plan_us.append(a0.elapsed_time(b0) * 1e3)
        med = {v: float(np.median(t)) for v, t in times.items()}
        up = times['upstream']
        entry = {'module': name, 'median_us': med, 'min_us': {v: float(min(t)) for v, t in times.items()},
                 'p90_us': {v: float(np.percentile(t, 90)) for v, t in times.items()},
                 'kernels_over_upstream': med['kernels'] / med['upstream'],
                 'upstream_min_to_p90_us': float(np.percentile(up, 90) - min(up)),
                 'faster_by_more_than_the_spread': med['upstream'] - med['kernels'] > float(np.percentile(up, 90) - min(up)),
                 'first_forward_with_plan_us_median': float(np.median(plan_us)),
                 'max_abs_difference': dict(zip(('y', 'dfeats', 'dkernel', 'dbias'), diff))}
        if name in ('dense', 'height'):
            entry['store_bytes'] = store_bytes(name)
        result['modules'].append(entry)
        print(json.dumps(entry))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
