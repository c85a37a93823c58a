"""The voting tail of the evaluator at the loader's real size (one scan of 34 720 key-frame points with 9 sweeps of the same size
behind it -- the teacher's multi-sweep input --, 17 classes, V in {1, 4, 12} copies through ``device_prep.prepare_lidar_batch``,
random logits), two ways:

(a) ``evaluate.vote_point_predictions``: one launch, counters included, nothing read back;
(b) what the code before it offered: per copy the gather of ``voxel_logits_to_point_predictions`` (two stable argsorts, a
    bincount, two blocking host reads) without its arg-max, then ``torch.stack(...).sum(0).argmax(-1)`` and
    ``MeanIoU.after_step``'s three bincounts.

Alternated, ``--samples`` each after ``--warmup`` (measuring-on-mi355x 5): device events around each leg and its host time;
median (min, p90); the host reads of each way, counted in a pass of its own; whether the two ways predict the same classes.
Then a whole ``Evaluator`` step (geometry by device_prep, full-size teacher with random weights, forward, voting tail) for
V = 1 and V = 4.  Needs the GPU.

    python tools/time_vote_eval.py [--samples 20] [--warmup 3] [--points 34720] [--sweeps 9] [--no-step] [--out profiles/vote_eval.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from u2mkd_amd.data import device_prep, nuscenes_lc as D  # noqa: E402
from u2mkd_amd.evaluate import Evaluator, MeanIoU, vote_point_predictions  # noqa: E402
from u2mkd_amd.synth import synth_raw_sample  # noqa: E402

HOST_READS = ('item', 'tolist', 'cpu', '__bool__', '__int__', '__index__')


def votes(points, sweeps, num_vote, seed=100):
    base = synth_raw_sample(points, [points] * sweeps, seed=seed, train=False)
    base['train'] = True
    rng = np.random.default_rng(seed)
    out = [base]
    for _ in range(1, num_vote):
        th = rng.uniform(0, 2 * np.pi)
        rot = np.array([[np.cos(th), np.sin(th), 0], [-np.sin(th), np.cos(th), 0], [0, 0, 1]])
        out.append(dict(base, teacher={'rot': rot, 'scale': float(rng.uniform(0.95, 1.05)), 'flip': int(rng.integers(0, 4))}))
    return D.VoteBatch(out, num_vote)


def gather_rows(logits, voxel_batch, inverse_map, inverse_batch, keyframe_mask_full):
    """``voxel_logits_to_point_predictions`` up to its arg-max: the per-point logits (the same calls, the same host reads)."""
    voxel_batch = voxel_batch.long()
    inverse_batch = inverse_batch.long()
    n_scene = int(max(int(voxel_batch.max()) if voxel_batch.numel() else -1, int(inverse_batch.max()) if inverse_batch.numel() else -1)) + 1
    order = torch.argsort(voxel_batch, stable=True)
    counts = torch.bincount(voxel_batch, minlength=n_scene)
    starts = torch.cumsum(counts, 0) - counts
    p_order = torch.argsort(inverse_batch, stable=True)
    rows = order[starts[inverse_batch[p_order]] + inverse_map.long()[p_order]]
    return logits[rows][keyframe_mask_full[p_order]]


def parent_tail(logits, d, metric):
    """The formulation without the kernel: per copy the gather, then stack, sum, arg-max and the metric's bincounts."""
    nb, per_copy = len(d['num_pts']), []
    p_off, v_off = np.cumsum([0] + d['num_pts']), np.cumsum([0] + d['num_vox'])
    for b in range(nb):
        ps, vs = slice(p_off[b], p_off[b + 1]), slice(v_off[b], v_off[b + 1])
        zeros_v = torch.zeros(d['num_vox'][b], dtype=torch.int64, device=logits.device)
        zeros_p = torch.zeros(d['num_pts'][b], dtype=torch.int64, device=logits.device)
        per_copy.append(gather_rows(logits[vs], zeros_v, d['inverse_map'][ps], zeros_p, d['keyframe_mask_full'][ps]))
    pred = torch.stack(per_copy, 0).sum(0).argmax(-1) if nb > 1 else per_copy[0].argmax(-1)
    metric.after_step({'outputs_vox': pred, 'targets': d['vote']['targets']})
    return pred


def new_tail(logits, d, counts):
    v = d['vote']
    return vote_point_predictions(logits, v['inverse_map'], v['copy_point_off'], v['copy_voxel_off'], v['scan_seg'], v['num_vote'],
                                  targets=v['targets'], ignore_label=0, counts=counts)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    host = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1), host, (time.perf_counter() - t0) * 1e3


def count_host_reads(fn):
    calls, saved = [], {}
    for name in HOST_READS:
        saved[name] = getattr(torch.Tensor, name)
        setattr(torch.Tensor, name, (lambda real, nm: lambda self, *a, **kw: (calls.append(nm) if self.is_cuda else None, real(self, *a, **kw))[1])(saved[name], name))
    try:
        fn()
    finally:
        for name, real in saved.items():
            setattr(torch.Tensor, name, real)
    return len(calls)


def stats(ms):
    s = sorted(ms)
    return {'median_ms': round(float(np.median(s)), 4), 'min_ms': round(s[0], 4), 'p90_ms': round(s[min(len(s) - 1, int(0.9 * len(s)))], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--points', type=int, default=34720)
    ap.add_argument('--sweeps', type=int, default=9)
    ap.add_argument('--classes', type=int, default=17)
    ap.add_argument('--no-step', action='store_true', help='skip the whole-Evaluator-step legs')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vote_eval.json'))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_vote_eval.py times the GPU path: no GPU is visible')
    result = {'config': {'key_points': opt.points, 'sweeps': opt.sweeps, 'classes': opt.classes, 'samples': opt.samples,
                         'warmup': opt.warmup, 'device': torch.cuda.get_device_name(0)}, 'tail': {}, 'step': {}}

    def write():                               # (after the tail legs and again after the step legs)
        line = json.dumps(result)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, 'w') as f:
            f.write(line + '\n')

    for num_vote in (1, 4, 12):
        d = device_prep.prepare_lidar_batch(votes(opt.points, opt.sweeps, num_vote))
        logits = torch.randn(sum(d['num_vox']), opt.classes, device='cuda') * 3
        legs = {'new_events': [], 'new_host': [], 'new_wall': [], 'parent_events': [], 'parent_host': [], 'parent_wall': []}
        for i in range(opt.warmup + opt.samples):
            counts, metric = torch.zeros(3, opt.classes, dtype=torch.int64, device='cuda'), MeanIoU(opt.classes, 0, 'outputs_vox', 'targets')
            p_new, ev_n, host_n, wall_n = timed(lambda: new_tail(logits, d, counts))
            p_old, ev_o, host_o, wall_o = timed(lambda: parent_tail(logits, d, metric))
            if i >= opt.warmup:
                for key, val in (('new_events', ev_n), ('new_host', host_n), ('new_wall', wall_n), ('parent_events', ev_o),
                                 ('parent_host', host_o), ('parent_wall', wall_o)):
                    legs[key].append(val)
        reads = {'new': count_host_reads(lambda: new_tail(logits, d, counts)), 'parent': count_host_reads(lambda: parent_tail(logits, d, metric))}
        result['tail']['V=%d' % num_vote] = {
            'points_all_copies': sum(d['num_pts']), 'voxels_all_copies': sum(d['num_vox']), 'legs': {k: stats(v) for k, v in legs.items()},
            'host_reads': reads, 'predictions_equal': bool(torch.equal(p_new, p_old)),
            'predictions_differing': int((p_new != p_old).sum()),
            'counters_equal': bool(torch.equal(counts.double(), metric._dev))}
        del d, logits
    write()
    if not opt.no_step:
        from u2mkd_amd import lidar
        torch.manual_seed(0)
        model = lidar.SPVCNN_SPFORMER(**lidar.spformer_kwargs(cr=1.0, num_classes=opt.classes)).cuda()
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, 'w.pt')
            torch.save({'model': model.state_dict()}, path)
            ev = Evaluator(model, path, opt.classes)
        for num_vote in (1, 4):
            raws, walls = votes(opt.points, opt.sweeps, num_vote), []
            ev.before_epoch()
            for i in range(2 + max(3, opt.samples // 4)):
                _, _, _, wall = timed(lambda: ev(device_prep.prepare_lidar_batch(raws)))
                if i >= 2:
                    walls.append(wall)
            result['step']['V=%d' % num_vote] = dict(stats(walls), what='prepare_lidar_batch + forward + voting tail, host clock to the synchronise')
    write()


if __name__ == '__main__':
    main()
