"""The LidarStep of the SPVCNN + SphereFormer teacher under ``make_optimizer(name='adamw_spformer')`` -- SphereFormer's own recipe,
transformer blocks at a reduced learning rate -- under amp in {False, 'fp16', 'bf16'}: fresh batches every step, the median of K
steps after warm-up (as tools/time_amp_step.py), and with ``--census`` the kernel launches and copies of ONE step after four
warm-up steps (torch.profiler, as NOTES N17.4).

    python tools/time_adamw_step.py [--steps 30] [--warmup 6] [--voxels 80000] [--amps False,fp16,bf16] [--census] [--out FILE.json]

Runs on any commit that has train.LidarStep and lidar.SPVCNN_SPFORMER: set U2MKD_TREE to the checkout to measure (a parent
commit's ``make_optimizer`` hands back torch.optim.AdamW, this tree's optim.FusedAdamW; U2MKD_FUSED_ADAM=0 is the same A/B inside
one tree)."""
import argparse
import collections
import json
import os
import sys

ROOT = os.environ.get('U2MKD_TREE') or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=30)
ap.add_argument('--warmup', type=int, default=6)
ap.add_argument('--voxels', type=int, default=80000)
ap.add_argument('--batches', type=int, default=4)
ap.add_argument('--amps', default='False,fp16,bf16')
ap.add_argument('--census', action='store_true')
ap.add_argument('--out', default=None)
opt = ap.parse_args()
sys.argv = sys.argv[:1]

import torch  # noqa: E402

import bench  # noqa: E402
from u2mkd_amd import lidar, train as T  # noqa: E402
from u2mkd_amd.synth import synth_batch  # noqa: E402

result = {'tree': 'the checkout named by U2MKD_TREE' if os.environ.get('U2MKD_TREE') else 'this checkout', 'steps': opt.steps, 'warmup': opt.warmup, 'voxels': opt.voxels, 'legs': {}}


def build(amp):
    torch.manual_seed(0)
    res = [tuple(torch.from_numpy(b[k]).cuda() for k in ('feats', 'coords', 'labels'))
           for b in (synth_batch(opt.voxels, 1, seed=1234 + 97 * i) for i in range(opt.batches))]
    model = lidar.SPVCNN_SPFORMER(**lidar.spformer_kwargs(cr=1.0)).cuda().train()
    runner = T.LidarStep(model, num_epochs=25, batch_size=1, amp=amp,
                         optimizer=lambda net: T.make_optimizer(net, name='adamw_spformer', lr=6e-3, weight_decay=0.01))
    counter, nxt = [0], [None]

    def step():
        feats, coords, labels = nxt[0] or tuple(t.clone() for t in res[counter[0] % opt.batches])
        counter[0] += 1
        nxt[0] = tuple(t.clone() for t in res[counter[0] % opt.batches])
        return runner(feats, coords, labels, prefetch=nxt[0][:2])
    step.runner = runner
    return step


def census(step):
    """kernel launches and copies of one step, and those issued inside the optimizer's step (between its two profiler marks)"""
    from torch.profiler import ProfilerActivity, profile
    for _ in range(4):
        step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    events = prof.events()
    spans = [(e.time_range.start, e.time_range.end) for e in events if e.name.startswith('Optimizer.step#')]
    kinds = collections.Counter()
    for e in events:
        if e.name in ('hipLaunchKernel', 'hipModuleLaunchKernel', 'hipExtModuleLaunchKernel', 'hipExtLaunchKernel', 'cudaLaunchKernel'):
            kinds['launches'] += 1
            kinds['launches_in_optimizer_step'] += any(a <= e.time_range.start <= b for a, b in spans)
        elif e.name in ('hipMemcpyAsync', 'hipMemcpyWithStream', 'hipMemcpy', 'cudaMemcpyAsync'):
            kinds['copies'] += 1
            kinds['copies_in_optimizer_step'] += any(a <= e.time_range.start <= b for a, b in spans)
        elif e.name in ('hipStreamSynchronize', 'hipDeviceSynchronize', 'hipEventSynchronize'):
            kinds['host_waits_in_optimizer_step'] += any(a <= e.time_range.start <= b for a, b in spans)
    return dict(kinds)


for amp in opt.amps.split(','):
    amp = False if amp == 'False' else amp
    step = build(amp)
    if opt.census:
        out = census(step)
    else:
        bench.timed_run(step, opt.warmup, opt.steps, 1)
        lo, hi = bench.timed_run.min_max_ms
        out = {'median_ms': round(bench.timed_run.median_ms, 3), 'min_ms': round(lo, 3), 'max_ms': round(hi, 3),
               'host_issue_ms': round(bench.timed_run.host_issue_ms, 3)}
    out['optimizer'] = type(step.runner.opt).__module__ + '.' + type(step.runner.opt).__name__
    result['legs'][str(amp)] = out
    print(amp, out, flush=True)
    del step
    torch.cuda.empty_cache()

line = json.dumps(result)
print(line)
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, 'w') as f:
        f.write(line + '\n')
