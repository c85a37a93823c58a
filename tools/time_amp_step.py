"""Training steps under each amp mode, one process, same box: the LidarStep at BASELINE.json configs[1] size (80 000 voxels,
cr 1.0) and the KD step at the default configs[2] size, each under amp in {False, 'fp16', 'bf16'} (fresh batches every step,
median of K steps after warm-up, as tools/time_configs4.py), and the 16-bit-storage north-star group (64 -> 64, k = 3, 80 000
voxels: forward + input gradient + weight gradient, microseconds) on bf16 and on fp16 rows side by side.  Also one launch
on rows of magnitude 2^-20 (fp16 subnormals) against the fp32 product of the same values: does the matrix instruction keep them?

    python tools/time_amp_step.py [--steps 40] [--warmup 8] [--legs lidar,kd,group,subnormal] [--out FILE.json]

Runs on any commit that has train.LidarStep / train.KDStep (put the tree to measure first on PYTHONPATH): a tree without fp16
rows reports its fp32-row formulation under amp='fp16', and no fp16 group."""
import argparse
import json
import os
import sys

ROOT = os.environ.get('U2MKD_TREE') or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=40)
ap.add_argument('--warmup', type=int, default=8)
ap.add_argument('--legs', default='lidar,kd,group,subnormal')
ap.add_argument('--out', default=None)
opt = ap.parse_args()
sys.argv = sys.argv[:1]

import torch  # noqa: E402

import bench  # noqa: E402
from u2mkd_amd import _lib as L, train as T  # noqa: E402
from u2mkd_amd.torchsparse.nn import functional as F  # noqa: E402

legs = opt.legs.split(',')
result = {'tree': ROOT, 'steps': opt.steps, 'warmup': opt.warmup, 'fp16_rows': hasattr(F, 'row_dtype') and getattr(F, '_F16_ROWS', False)}


def timed_step(workload, amp):
    """median / min / max ms of `steps` steps of bench.py's step closure with the runner's amp mode replaced"""
    args = bench.parse()
    real = {'LidarStep': T.LidarStep, 'KDStep': T.KDStep}
    try:
        for name, cls in real.items():
            setattr(T, name, lambda *a, _cls=cls, **k: _cls(*a, **dict(k, amp=amp)))
        step, _, _ = bench.build_step(args, 0, workload, args.image_hw, watch=False)
    finally:
        for name, cls in real.items():
            setattr(T, name, cls)
    bench.timed_run(step, opt.warmup, opt.steps, 1)
    lo, hi = bench.timed_run.min_max_ms
    out = {'median_ms': round(bench.timed_run.median_ms, 3), 'min_ms': round(lo, 3), 'max_ms': round(hi, 3)}
    del step
    torch.cuda.empty_cache()
    return out


for leg, workload in (('lidar', 'spvcnn'), ('kd', 'kd')):
    if leg in legs:
        result[leg] = {}
        for amp in (False, 'fp16', 'bf16'):
            result[leg][str(amp)] = timed_step(workload, amp)
            print(leg, amp, result[leg][str(amp)], flush=True)


def storage_group(dtype, iters=200):
    """fwd / dgrad / wgrad of Conv3d(64, 64, 3) on the 80 000-voxel scene's stride-1 map on rows of `dtype`, microseconds"""
    from u2mkd_amd.synth import synth_batch
    suffix, arith = {torch.bfloat16: ('_bf16', 3), torch.float16: ('_f16', 5)}[dtype]
    lib = L.load()
    cin = cout = 64
    coords = torch.from_numpy(synth_batch(80000, 1, seed=1234)['coords']).cuda()
    km = F.build_kmap(coords, (1, 1, 1), (3, 3, 3), (1, 1, 1))
    n = km.n_out
    sch = km.schedule(False)
    pairs, _, plan = km.pairs_plan()
    nbytes = lib.u2mkd_conv_wgrad_pairs_workspace_bytes(n, cin, cout, 27)
    st = L.stream()
    g = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randn(n, cin, device='cuda', generator=g).to(dtype)
    gy = torch.randn(n, cout, device='cuda', generator=g).to(dtype)
    w = torch.randn(27, cin, cout, device='cuda', generator=g) / (27 * cin) ** 0.5
    wf = torch.empty(2, lib.u2mkd_weight_fragments_bytes(27, cin, cout, arith), dtype=torch.uint8, device='cuda')
    out, dx = torch.empty(n, cout, device='cuda', dtype=dtype), torch.empty(n, cin, device='cuda', dtype=dtype)
    dw, ws = torch.empty_like(w), torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    L.call('u2mkd_weight_fragments', L.ptr(w), 27, cin, cout, 2, arith, L.ptr(wf), st)

    def conv(a, frag, flip, o):
        L.call('u2mkd_conv_forward_tiles' + suffix, L.ptr(a), n, cin, L.ptr(wf[frag]), cout, L.ptr(sch.nbr_s), L.ptr(sch.order),
               L.ptr(sch.items), L.ptr(sch.n_items), n, 27, flip, L.ptr(o), st)
    t = {'fwd': bench.time_events([lambda: conv(x, 0, 0, out)], iters), 'dgrad': bench.time_events([lambda: conv(gy, 1, 1, dx)], iters),
         'wgrad': bench.time_events([lambda: L.call('u2mkd_conv_wgrad_pairs' + suffix, L.ptr(x), cin, L.ptr(gy), cout, L.ptr(pairs),
                                                    L.ptr(plan), n, 27, 0, L.ptr(ws), nbytes, L.ptr(dw), st)], iters)}
    t = {k: round(v * 1e3, 1) for k, v in t.items()}
    t['total'] = round(sum(t.values()), 1)
    t['rows'] = n
    return t


if 'group' in legs:
    result['group_us'] = {'bf16': storage_group(torch.bfloat16)}
    if 'u2mkd_conv_forward_tiles_f16' in L.SIGNATURES:
        result['group_us']['fp16'] = storage_group(torch.float16)
    print('group', result['group_us'], flush=True)


if 'subnormal' in legs and 'u2mkd_linear_forward_f16' in L.SIGNATURES:
    # rows of magnitude 2^-20 (fp16 subnormals: multiples of 2^-24) times weights of magnitude 2^4: the products are normal fp16
    # numbers if the matrix instruction reads the subnormal operands, and zero if it flushes them
    lib = L.load()
    n, cin, cout = 256, 64, 64
    g = torch.Generator(device='cuda').manual_seed(1)
    x = (torch.randint(-31, 32, (n, cin), device='cuda', generator=g).float() * 2.0 ** -24).half()
    w = (torch.randint(-31, 32, (cout, cin), device='cuda', generator=g).float())
    wf = torch.empty(2, lib.u2mkd_weight_fragments_bytes(1, cout, cin, 5), dtype=torch.uint8, device='cuda')
    L.call('u2mkd_weight_fragments', L.ptr(w), 1, cout, cin, 2, 5, L.ptr(wf), L.stream())
    y = torch.empty(n, cout, dtype=torch.float16, device='cuda')
    L.call('u2mkd_linear_forward_f16', L.ptr(x), n, cin, L.ptr(wf[1]), cout, None, L.ptr(y), L.stream())
    want = x.float() @ w.t()
    result['fp16_subnormal_operands'] = {
        'max_abs_row_value': float(x.float().abs().max()), 'max_abs_want': float(want.abs().max()),
        'max_abs_got': float(y.float().abs().max()), 'max_abs_error': float((y.float() - want).abs().max()),
        'kept': bool(float(y.float().abs().max()) > 0 and float((y.float() - want).abs().max()) <= 2.0 ** -11 * float(want.abs().max()))}
    print('subnormal', result['fp16_subnormal_operands'], flush=True)

line = json.dumps(result)
print(line)
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, 'w') as f:
        f.write(line + '\n')
