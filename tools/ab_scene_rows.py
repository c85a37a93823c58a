"""A/B of spnn.GroupNorm on the scene kernels (csrc/gn.hip) against the loop formulation on torch's GPU operators -- what
torchsparse v1.4.0 runs: ``coords[:, -1].max().item()``, then per batch index a boolean mask, ``feats[mask]``, F.group_norm and
``nfeats[mask] = ...`` -- forward + backward, at B = 2 scenes of 40 000 rows, (C, G) = (64, 8) and (256, 32).

    python tools/ab_scene_rows.py OUT.json [samples]        the A/B: device events, versions alternated, medians
    python tools/ab_scene_rows.py --kernels [iterations]    the kernel route alone, for a kernel trace (rocprofv3 --kernel-trace)

Per sample one version runs one forward + backward between two device events (the loop's host read is inside its window: it is
part of what a layer costs there); the versions alternate sample by sample.  The outputs of the two versions are compared at the
sizes that are timed.  BYTES of the apply pass: it reads and writes every row once (2 N C elements) and one batch index per
row (``apply_pass_bytes``); its rate is that over gn_apply_kernel's time in a kernel trace, against the 6.29 TB/s copy rate of the
MI355X."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from u2mkd_amd import torchsparse as ts
from u2mkd_amd.torchsparse import nn as spnn
from u2mkd_amd.torchsparse.nn import functional as F

ROWS, SCENES = 40000, 2
SHAPES = ((64, 8), (256, 32))


def loop_group_norm(feats, coords, gn):
    """torchsparse v1.4.0's GroupNorm.forward on a SparseTensor's feats / coords"""
    batch_size = int(coords[:, -1].max().item()) + 1
    nfeats = torch.zeros_like(feats)
    c = feats.shape[1]
    for k in range(batch_size):
        mask = coords[:, -1] == k
        bfeats = feats[mask].transpose(0, 1).reshape(1, c, -1)
        bfeats = torch.nn.functional.group_norm(bfeats, gn.num_groups, gn.weight, gn.bias, gn.eps)
        nfeats[mask] = bfeats.reshape(c, -1).transpose(0, 1)
    return nfeats


def make(c, groups, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = ROWS * SCENES
    i = torch.arange(n, dtype=torch.int32)
    coords = torch.stack([i % 211, (i // 211) % 223, i // (211 * 223), i // ROWS], 1).contiguous().cuda()
    x = torch.randn(n, c, generator=g).cuda()
    dy = torch.randn(n, c, generator=g).cuda()
    gn = spnn.GroupNorm(groups, c).cuda()
    with torch.no_grad():
        gn.weight.copy_(1.0 + 0.5 * torch.randn(c, generator=g))
        gn.bias.copy_(torch.randn(c, generator=g))
    return coords, x, dy, gn


def step(version, coords, x, dy, gn):
    x = x.detach().requires_grad_()
    gn.zero_grad(set_to_none=True)
    if version == 'kernels':
        y = gn(ts.SparseTensor(x, coords)).feats
    else:
        y = loop_group_norm(x, coords, gn)
    y.backward(dy)
    return y.detach(), x.grad, gn.weight.grad, gn.bias.grad


def timed(version, *case):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    step(version, *case)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3      # us


def main():
    assert torch.cuda.is_available(), 'needs a GPU'
    if sys.argv[1] == '--kernels':
        iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
        for c, groups in SHAPES:
            case = make(c, groups)
            for _ in range(iters):
                step('kernels', *case)
        torch.cuda.synchronize()
        return
    out, samples = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 40
    result = {'rows_per_scene': ROWS, 'scenes': SCENES, 'samples': samples, 'unit': 'us per forward + backward', 'shapes': []}
    for c, groups in SHAPES:
        case = make(c, groups)
        for _ in range(5):      # warm-up of both versions (code objects, the scene plan, the allocator)
            ref = step('loop', *case)
            got = step('kernels', *case)
        diff = [float((a.double() - b.double()).abs().max()) for a, b in zip(got, ref)]
        times = {'kernels': [], 'loop': []}
        for _ in range(samples):
            for version in ('kernels', 'loop'):
                times[version].append(timed(version, *case))
        med = {v: float(np.median(t)) for v, t in times.items()}
        plan_us = []
        for _ in range(10):      # the scene plan of a FRESH coordinate tensor: once per batch, its one host read inside
            fresh = case[0].clone()
            a0, b0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a0.record()
            F.scene_plan(fresh)
            b0.record()
            b0.synchronize()
            plan_us.append(a0.elapsed_time(b0) * 1e3)
        n = ROWS * SCENES
        result['shapes'].append({
            'c': c, 'groups': groups, 'median_us': med, 'min_us': {v: float(min(t)) for v, t in times.items()},
            'p90_us': {v: float(np.percentile(t, 90)) for v, t in times.items()},
            'kernels_over_loop': med['kernels'] / med['loop'], 'scene_plan_build_us_median': float(np.median(plan_us)),
            'max_abs_difference': dict(zip(('y', 'dx', 'dgamma', 'dbeta'), diff)),
            'apply_pass_bytes': 2 * n * c * 4 + n * 4})
        print(json.dumps(result['shapes'][-1]))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
