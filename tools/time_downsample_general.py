"""Time the general branch of F.spdownsample (k = 3, s = 2) on the device.

  (a) torchsparse v1.4.0's own formulation on the device: repeat the rows K = 27 times, add the offsets, mask, unique(dim=0)
  (b) F.spdownsample: u2mkd_downsample_keys_general (<= 8 keys per row) + unique of int64 keys + u2mkd_unpack_keys
  (c) forward + backward of one 64 -> 64 convolution on the k = 3, s = 2 map next to one on the k = 2, s = 2 map of the scene

Medians of --runs runs after --warmup warm-up runs, one synchronisation per run, wall clock around it (both formulations stop
the host for the output size, so device-only event times would leave that out).  One JSON line per scene.

    python tools/time_downsample_general.py [--runs 30] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from u2mkd_amd.synth import synth_batch                       # noqa: E402
from u2mkd_amd.torchsparse.nn import functional as F         # noqa: E402
from u2mkd_amd.torchsparse.nn.utils import get_kernel_offsets  # noqa: E402


def torch_formulation(coords, stride, kernel_size, tensor_stride):
    """the general branch as torchsparse runs it, on the device; (x, y, z, b) rows sorted by (b, x, y, z)"""
    offsets = get_kernel_offsets(kernel_size, tensor_stride, device=coords.device)
    k = offsets.shape[0]
    ss = torch.tensor([stride * tensor_stride] * 3, dtype=torch.int32, device=coords.device)
    cmin = coords[:, :3].amin(0, keepdim=True)
    xyz = coords[:, :3].unsqueeze(1).repeat(1, k, 1) + offsets
    b = coords[:, 3:].repeat(1, k)
    xyz, b = xyz.view(-1, 3), b.view(-1, 1)
    mask = ((xyz % ss == 0) & (xyz >= cmin)).all(1)
    rows = torch.cat([b[mask], xyz[mask]], 1)
    return torch.unique(rows, dim=0)[:, [1, 2, 3, 0]].contiguous()


def median_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def conv_step(km, x, w, g):
    x.grad = w.grad = None
    F.ConvolutionFunction.apply(x, w, km, False).backward(g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    assert args.runs >= 20
    for n in (80000, 16000):
        for ts in (1, 2):
            c = torch.from_numpy(synth_batch(n, 1, seed=5)['coords']).cuda()
            if ts > 1:
                c = F.spdownsample(c, ts, ts, 1)
            want = torch_formulation(c, 2, 3, ts)
            got = F.spdownsample(c, 2, 3, ts)
            assert torch.equal(want, got)
            res = {'n_in': c.shape[0], 'tensor_stride': ts, 'n_out': got.shape[0],
                   'torch_repeat_mask_unique_ms': median_ms(lambda: torch_formulation(c, 2, 3, ts), args.runs, args.warmup),
                   'spdownsample_ms': median_ms(lambda: F.spdownsample(c, 2, 3, ts), args.runs, args.warmup)}
            for name, ks in (('k3s2', 3), ('k2s2', 2)):
                km = F.build_kmap(c, (ts,) * 3, (ks,) * 3, (2,) * 3)
                torch.manual_seed(0)
                x = torch.randn(km.n_in, 64, device='cuda', requires_grad=True)
                w = (torch.randn(ks ** 3, 64, 64, device='cuda') / (ks ** 3 * 64) ** 0.5).requires_grad_(True)
                g = torch.randn(km.n_out, 64, device='cuda')
                res['conv64_%s_fwd_bwd_ms' % name] = median_ms(lambda: conv_step(km, x, w, g), args.runs, args.warmup)
                res['n_out_' + name] = km.n_out
            print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
