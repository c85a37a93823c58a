"""Evaluation entry point: a checkpoint's mIoU with test-time voting, and the files the nuScenes lidarseg server takes -- the
reference's `NuScenes_Evaluator` (core/nusc_trainers.py:441-551) on the HIP operators.

    python run_evaluation.py configs/nuscenes/train/spformer_tsd_full_ours_star.yaml --weight-path runs/kd/checkpoints/max-iou-vox-val.pt \\
        [--split val|test] [--submission-dir DIR] [--synthetic N_VOXELS] [--max-iters K] [--dataset.num_vote V ...]

The configuration is read as run_training.py reads it (file, recursive defaults, `--key.sub value` overrides); the evaluated
network follows `model.name`: `spvcnn_spformer` is fed the teacher input, `spvcnn_swiftnet18_spformer_tsd_full` the student
input with all cameras.  `dataset.num_vote` (default 1: the shipped files have none) copies of every scan -- the first as it is,
the others rotated, scaled and flipped as training samples are -- go through the network in one batch; their per-point logits
are summed on the device and arg-maxed (u2mkd_amd.evaluate.vote_point_predictions), and the MeanIoU counters stay there until
the end.  The loader delivers raw samples, the batch geometry runs on the GPU (data/device_prep.py).  Single process.

`--submission-dir DIR` writes `DIR/lidarseg/<split>/<lidar_token>_lidarseg.bin` (one uint8 per key-frame point, the ignored
class never predicted) and `DIR/<split>/submission.json`; the copy of the predictions to the host for these files is the only
host read the voting tail makes.  `--synthetic` replaces the on-disk dataset by seeded synthetic raw scans of that many points."""
import argparse
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from u2mkd_amd import builder, distributed as D                                          # noqa: E402
from u2mkd_amd.evaluate import MAX_COPIES, Evaluator, SubmissionWriter                   # noqa: E402

KD_MODEL = 'spvcnn_swiftnet18_spformer_tsd_full'


def log(*a):
    print('[run_evaluation]', *a, flush=True)


def num_vote_of(cfg):
    """`dataset.num_vote`, 1 when the configuration has none (the reference's shipped files have none)."""
    v = cfg.get('dataset', {}).get('num_vote', 1)
    v = 1 if v is None else int(v)
    if not 1 <= v <= MAX_COPIES:
        raise ValueError('dataset.num_vote must be 1..%d, got %d' % (MAX_COPIES, v))
    return v


class SyntheticScans(torch.utils.data.Dataset):
    """Seeded synthetic raw scans (synth.synth_raw_sample) behind the interface `VoteView` wraps: `raw_votes`, `rng`."""

    def __init__(self, n_points, length, image_hw, seed, voxel_size, sweeps, flip=True):
        self.n, self.length, self.hw, self.seed, self.voxel_size, self.sweeps, self.flip = n_points, length, image_hw, seed, voxel_size, sweeps, flip
        self.rng = np.random.default_rng(seed)

    def __len__(self):
        return self.length

    def raw_votes(self, index, num_vote):
        from u2mkd_amd.data.nuscenes_lc import draw_sample_parameters
        from u2mkd_amd.synth import synth_raw_sample
        base = synth_raw_sample(self.n, [self.n // 2, self.n // 3] if self.sweeps else None, seed=self.seed + 7919 * int(index),
                                image_hw=self.hw, voxel_size=self.voxel_size, train=False)
        base['train'] = True                           # (the identity parameters of vote 0 are applied, as the others' draws)
        votes = [base]
        for _ in range(1, num_vote):               # the on-disk dataset's draw order (nuscenes_lc.draw_sample_parameters)
            teacher, _unused, student = draw_sample_parameters(self.rng, self.flip, 0)
            votes.append(dict(base, teacher=teacher, student=student))
        return votes


def main(argv=None):
    was = torch.backends.cudnn.deterministic
    try:
        return _evaluate(argv)
    finally:
        torch.backends.cudnn.deterministic = was      # (a caller in the same process, e.g. a test, keeps its setting)


def _evaluate(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument('config', metavar='FILE')
    ap.add_argument('--weight-path', metavar='FILE', required=True)
    ap.add_argument('--split', choices=('val', 'test'), default='val')
    ap.add_argument('--submission-dir', metavar='DIR', default=None)
    ap.add_argument('--synthetic', type=int, default=0, metavar='N_VOXELS', help='synthetic scans instead of dataset.root')
    ap.add_argument('--max-iters', type=int, default=0, help='stop after K batches')
    args, opts = ap.parse_known_args(argv)

    cfg = builder.Config.load(args.config, recursive=True)
    cfg.update(opts)
    cfg.update({k: v for k, v in vars(args).items() if k != 'config'})
    cfg.setdefault('debug', builder.Config())['debug_val'] = False      # (the in-view labels are the training eval branch's)
    num_vote = num_vote_of(cfg)
    D.configure_runtime()                      # (before the first HIP call of the process)
    if not torch.cuda.is_available():
        raise RuntimeError('run_evaluation.py drives the HIP operators: no GPU is visible (there is no CPU fallback)')
    if not os.path.exists(args.weight_path):
        raise FileNotFoundError(args.weight_path)

    seed = cfg.get('train', {}).get('seed')
    seed = 0 if seed is None else int(seed)
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed); torch.cuda.manual_seed(seed)
    # the camera branch's MIOpen convolutions: the deterministic choices, so that a checkpoint's number does not move in the
    # last bits of the logits from one forward to the next (NOTES N6; the LiDAR side is order-deterministic by construction)
    torch.backends.cudnn.deterministic = True

    from u2mkd_amd.data import device_prep
    from u2mkd_amd.data.nuscenes_lc import VoteView
    is_kd = cfg.model.name == KD_MODEL
    ignore = cfg.data.ignore_label
    scans = max(1, min(int(cfg.batch_size), MAX_COPIES // num_vote))
    workers = cfg.get('workers_per_gpu', 4)
    if args.synthetic:
        hw = tuple(int(x * cfg.dataset.get('im_cr', 0.4)) for x in (900, 1600))
        sweeps = cfg.dataset.get('multisweeps', {}).get('num_sweeps', 0) != 0
        dataset = SyntheticScans(args.synthetic, max(scans * max(args.max_iters, 2), 4), hw, seed, cfg.dataset.voxel_size, sweeps)
        workers = 0
    else:
        dataset = builder.make_dataset(cfg, rng=np.random.default_rng(seed), splits=(args.split,))[args.split]
    view = VoteView(dataset, num_vote)

    def seed_worker(wid):                      # core/nusc_trainers.py:489-490 (epoch 1); the worker's copy of the view
        torch.utils.data.get_worker_info().dataset.rng = np.random.default_rng(seed + wid)
    flow = torch.utils.data.DataLoader(view, batch_size=scans, shuffle=False, num_workers=workers, collate_fn=view.collate_fn,
                                       worker_init_fn=seed_worker)

    model = builder.make_model(cfg).cuda()
    submit = SubmissionWriter(args.submission_dir, args.split, use_camera=is_kd) if args.submission_dir else None
    ev = Evaluator(model, args.weight_path, cfg.data.num_classes, amp=bool(cfg.get('amp_enabled', False)), ignore_label=ignore,
                   skip_class=cfg.criterion.ignore_index if submit is not None else -1)
    log('weights: %s; model %s, split %s, %d vote(s), %d scan(s) per step' % (args.weight_path, cfg.model.name, args.split, num_vote, scans))
    ev.before_epoch()
    steps = 0
    for i, raws in enumerate(flow):
        if args.max_iters and i >= args.max_iters:
            break
        d = device_prep.prepare_kd_batch(raws) if is_kd else device_prep.prepare_lidar_batch(raws)
        ret = ev(d)
        if submit is not None:
            submit.add(ret)
        steps += 1
    miou, ious = ev.after_epoch()
    log('%d steps: mIoU %.17g' % (steps, miou))
    log('per-class IoU:', ' '.join('%.6f' % float(x) for x in ious))
    result = {'miou': miou, 'ious': [float(x) for x in ious], 'steps': steps, 'num_vote': num_vote}
    if submit is not None:
        result['submission'] = submit.close()
        log('submission: %d files under %s, %s' % (len(submit.written), submit.bin_dir, result['submission']))
    return result


if __name__ == '__main__':
    main()
