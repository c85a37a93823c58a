"""Evaluation path: the eval branch of the reference trainers and the MeanIoU callback.

* :func:`voxel_logits_to_point_predictions` -- what ``_run_step`` does when the model is not training
  (core/nusc_trainers.py:367-418, core/spformer_trainer.py:95-117): per scene, the voxel logits are gathered back
  to the raw points through ``inverse_map`` and arg-maxed; multi-sweep inputs keep the key-frame points only.
* :class:`MeanIoU` -- core/callbacks.py:91-171: per-class seen / correct / predicted counters over an epoch,
  summed over the ranks, IoU_c = correct / (seen + predicted - correct), classes never seen count as 1 except the
  ignore label, mean over the kept classes.  The counters are three ``bincount`` calls on the device per step
  instead of 3 x num_classes host round trips, and one all_reduce of [3, num_classes] instead of 3 x num_classes.
* :func:`vote_point_predictions` -- the tail of ``NuScenes_Evaluator._run_step`` (core/nusc_trainers.py:523-550) with test-time
  voting in ONE launch (csrc/vote.hip): gather through each copy's inverse map, fp32 sum in vote order, arg-max, the three
  MeanIoU counters; nothing is read back.
* :class:`Evaluator` -- ``NuScenes_Evaluator`` (core/nusc_trainers.py:441-551) on the device batches of ``data.device_prep``;
  :class:`SubmissionWriter` -- the files the nuScenes lidarseg server takes."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from . import _lib as L

__all__ = ['voxel_logits_to_point_predictions', 'MeanIoU', 'vote_point_predictions', 'Evaluator', 'SubmissionWriter',
           'MAX_CLASSES', 'MAX_COPIES']

MAX_CLASSES = 64           # csrc/vote.hip keeps a point's class sums in registers
MAX_COPIES = 64            # scans x votes of one call = data.device_prep.MAX_BATCH
_ROW_TYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def voxel_logits_to_point_predictions(logits, voxel_batch, inverse_map, inverse_batch, keyframe_mask_full=None):
    """Per-point class predictions of a batch.

    logits [Nv, C] per voxel; voxel_batch [Nv] scene of every voxel (``lidar.C[:, -1]``); inverse_map [Np] index of
    every raw point's voxel WITHIN its scene (``inverse_map.F``); inverse_batch [Np] scene of every point
    (``inverse_map.C[:, -1]``).  Equals the reference's loop ``outputs[cur_scene_pts][cur_inv].argmax(1)`` over the
    scenes, concatenated in scene order; ``keyframe_mask_full`` (multisweeps != 0) keeps the key-frame points."""
    voxel_batch = voxel_batch.long()
    inverse_batch = inverse_batch.long()
    n_scene = int(max(int(voxel_batch.max()) if voxel_batch.numel() else -1,
                      int(inverse_batch.max()) if inverse_batch.numel() else -1)) + 1
    # global row of the j-th voxel of scene s: a stable sort by scene keeps the in-scene order of boolean indexing
    order = torch.argsort(voxel_batch, stable=True)
    counts = torch.bincount(voxel_batch, minlength=n_scene)
    starts = torch.cumsum(counts, 0) - counts
    # points must come out scene by scene as well (the reference concatenates per scene)
    p_order = torch.argsort(inverse_batch, stable=True)
    rows = order[starts[inverse_batch[p_order]] + inverse_map.long()[p_order]]
    pred = logits[rows].argmax(1)
    if keyframe_mask_full is not None:
        pred = pred[keyframe_mask_full[p_order]]
    return pred


class MeanIoU:
    """core/callbacks.py:91-171 without the torchpack Callback plumbing: ``before_epoch`` / ``after_step`` /
    ``after_epoch`` carry the same arithmetic; ``after_epoch`` returns (mIoU, per-class IoUs of the kept classes)."""

    def __init__(self, num_classes: int, ignore_label: int, output_tensor: str = 'outputs', target_tensor: str = 'targets',
                 name: str = 'iou'):
        self.num_classes, self.ignore_label, self.name = num_classes, ignore_label, name
        self.output_tensor, self.target_tensor = output_tensor, target_tensor
        self.before_epoch()

    def before_epoch(self):
        self.total_seen = np.zeros(self.num_classes)
        self.total_correct = np.zeros(self.num_classes)
        self.total_positive = np.zeros(self.num_classes)
        self._dev = None

    def after_step(self, output_dict):
        outputs = torch.as_tensor(output_dict[self.output_tensor])
        targets = torch.as_tensor(output_dict[self.target_tensor]).to(outputs.device)
        keep = targets != self.ignore_label
        outputs, targets = outputs[keep].long(), targets[keep].long()
        c = self.num_classes
        upd = torch.stack([torch.bincount(targets, minlength=c)[:c],
                           torch.bincount(targets[outputs == targets], minlength=c)[:c],
                           torch.bincount(outputs.clamp(0, c - 1), minlength=c)[:c]]).double()
        self._dev = upd if self._dev is None else self._dev + upd.to(self._dev.device)

    def add_counts(self, counts):
        """Add a device [3, num_classes] tensor (seen, correct, predicted: what ``vote_point_predictions`` counts) to what
        ``after_step`` accumulates.  No host read."""
        if tuple(counts.shape) != (3, self.num_classes):
            raise ValueError('add_counts: expected [3, %d], got %s' % (self.num_classes, tuple(counts.shape)))
        upd = counts.double()
        self._dev = upd if self._dev is None else self._dev + upd.to(self._dev.device)

    def after_epoch(self):
        import torch.distributed as dist
        acc = self._dev if self._dev is not None else torch.zeros(3, self.num_classes, dtype=torch.float64)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dev = 'cuda' if dist.get_backend() == 'nccl' else 'cpu'
            acc = acc.to(dev)
            dist.all_reduce(acc)                       # the reference: 3 x num_classes scalar all-reduces
        acc = acc.cpu().numpy()
        self.total_seen, self.total_correct, self.total_positive = (self.total_seen + acc[0], self.total_correct + acc[1],
                                                                     self.total_positive + acc[2])
        self._dev = None
        ious = []
        for i in range(self.num_classes):
            if self.total_seen[i] == 0:
                if i == self.ignore_label:
                    continue
                ious.append(1)
            else:
                ious.append(self.total_correct[i] / (self.total_seen[i] + self.total_positive[i] - self.total_correct[i]))
        return float(np.mean(ious)), ious


def vote_point_predictions(logits, inverse_map, copy_point_off, copy_voxel_off, scan_seg, n_votes, targets=None, ignore_label=0,
                           skip_class=-1, want_sums=False, counts=None, num_points=None):
    """Per-point predictions of a batch of S scans with ``n_votes`` augmented copies each (sample ``s * n_votes + v`` of the
    device batch is copy v of scan s), in one launch of ``u2mkd_vote_points`` and with no host read.

    logits [Nv, C] voxel rows (fp32 / bf16 / fp16); inverse_map [Np_all] int64 voxel rank of every point within its sample;
    copy_point_off / copy_voxel_off [S * n_votes] int32 first point row / first voxel row of each copy; scan_seg [S + 1] int32
    key-frame point offsets of the scans in the output (all device tensors: ``data.device_prep`` returns them for a
    ``VoteView`` batch).  A sample's key-frame points come first, so its sweep points are never read.

    Per output point the copies' logits are summed in fp32 in vote order, ``(((0 + x_0) + x_1) + ...)``, and the prediction is
    the lowest class among the maxima of the sum (a NaN is maximal, as ``torch.argmax`` on the CPU); ``skip_class >= 0`` leaves
    that class out (submission mode: class 0 is no legal submission value).  ``counts`` [3, C] int64 is ADDED to: seen, correct
    and predicted per class over the points with ``targets != ignore_label`` (``MeanIoU.after_step``'s bincounts; a target
    outside [0, C) that is not ``ignore_label`` is counted nowhere) -- it needs ``targets`` [P] int64.

    The number of output points P is ``targets.shape[0]``, else ``num_points`` (a Python int: it is not read from scan_seg).
    Like the offsets and the inverse map, P is TRUSTED: the kernel writes ``pred[p]`` for every ``p < scan_seg[-1]``, so P must
    equal ``scan_seg[-1]`` (``device_prep`` builds both from the same host counts); a shorter ``targets`` is written past.
    Returns ``pred`` [P] int64, or ``(pred, sums [P, C] fp32)`` with ``want_sums``."""
    if logits.dim() != 2:
        raise ValueError('vote_point_predictions: logits must be [Nv, C], got %s' % (tuple(logits.shape),))
    c, n_votes = int(logits.shape[1]), int(n_votes)
    if not 1 <= c <= MAX_CLASSES:
        raise ValueError('vote_point_predictions: 1 <= C <= %d classes, got %d' % (MAX_CLASSES, c))
    if n_votes < 1:
        raise ValueError('vote_point_predictions: n_votes >= 1, got %d' % n_votes)
    if scan_seg.dim() != 1 or scan_seg.numel() < 1:
        raise ValueError('vote_point_predictions: scan_seg must be [S + 1]')
    n_scans = int(scan_seg.numel()) - 1
    if n_scans * n_votes > MAX_COPIES:
        raise ValueError('vote_point_predictions: scans x votes <= %d, got %d x %d' % (MAX_COPIES, n_scans, n_votes))
    for name, t in (('copy_point_off', copy_point_off), ('copy_voxel_off', copy_voxel_off)):
        if t.dim() != 1 or t.numel() != n_scans * n_votes:
            raise ValueError('vote_point_predictions: %s must be [S * n_votes] = [%d], got %s' % (name, n_scans * n_votes, tuple(t.shape)))
    skip_class = int(skip_class)
    if skip_class >= c or (skip_class >= 0 and c < 2):
        raise ValueError('vote_point_predictions: skip_class %d leaves no class of %d to predict' % (skip_class, c))
    if logits.dtype not in _ROW_TYPES:
        raise ValueError('vote_point_predictions: logits must be float32, bfloat16 or float16, got %s' % logits.dtype)
    if counts is not None and targets is None:
        raise ValueError('vote_point_predictions: counts needs targets')
    if targets is None and num_points is None:
        raise ValueError('vote_point_predictions: pass targets or num_points (the point count is not read back from scan_seg)')
    n_points = int(targets.shape[0]) if targets is not None else int(num_points)
    if num_points is not None and int(num_points) != n_points:
        raise ValueError('vote_point_predictions: num_points %d but %d targets' % (int(num_points), n_points))
    if n_scans == 0 and n_points:
        raise ValueError('vote_point_predictions: %d points but no scan' % n_points)
    if counts is not None and (tuple(counts.shape) != (3, c) or counts.dtype != torch.int64 or not counts.is_contiguous()):
        raise ValueError('vote_point_predictions: counts must be a contiguous int64 [3, %d]' % c)
    for name, t, dt in (('inverse_map', inverse_map, torch.int64), ('copy_point_off', copy_point_off, torch.int32),
                        ('copy_voxel_off', copy_voxel_off, torch.int32), ('scan_seg', scan_seg, torch.int32), ('targets', targets, torch.int64)):
        if t is not None and t.dtype != dt:
            raise ValueError('vote_point_predictions: %s must be %s, got %s' % (name, dt, t.dtype))
    L.require_cuda(logits, inverse_map, copy_point_off, copy_voxel_off, scan_seg, targets, counts)
    logits, inverse_map = logits.contiguous(), inverse_map.contiguous()
    copy_point_off, copy_voxel_off, scan_seg = copy_point_off.contiguous(), copy_voxel_off.contiguous(), scan_seg.contiguous()
    targets = targets.contiguous() if targets is not None else None
    pred = torch.empty(n_points, dtype=torch.int64, device=logits.device)
    sums = torch.empty(n_points, c, dtype=torch.float32, device=logits.device) if want_sums else None
    if n_points == 0 or n_scans == 0:              # nothing to launch (and an empty tensor has no address to pass)
        return (pred, sums) if want_sums else pred
    L.call('u2mkd_vote_points', L.ptr(logits), _ROW_TYPES[logits.dtype], c, L.ptr(inverse_map), L.ptr(copy_point_off),
           L.ptr(copy_voxel_off), L.ptr(scan_seg), n_scans, n_votes, L.ptr(targets), int(ignore_label), skip_class, L.ptr(sums),
           L.ptr(pred), L.ptr(counts), L.stream())
    return (pred, sums) if want_sums else pred


class Evaluator:
    """``NuScenes_Evaluator`` (core/nusc_trainers.py:441-551): a checkpoint's ``model`` entry (``module.`` stripped) into the
    model, ``eval()``, and per step the forward under the amp setting, ``x_vox`` alone, and the voting tail.

    ``model``: ``spvcnn_spformer`` (lidar.SPVCNN_SPFORMER, fed the teacher input of ``device_prep.prepare_lidar_batch``) or
    ``spvcnn_swiftnet18_spformer_tsd_full`` (kd.TSDFull, fed the student input of ``device_prep.prepare_kd_batch``); the batch
    comes from a ``data.nuscenes_lc.VoteView`` loader, so it carries the ``vote`` tables.  ``num_vote`` is the batch's.
    ``skip_class >= 0``: submission mode, that class is never predicted.  The MeanIoU counters stay on the device until
    ``after_epoch``."""

    def __init__(self, model, weight_path, num_classes, amp=False, ignore_label=0, skip_class=-1):
        from . import kd as KD
        from .train import _Amp
        if weight_path is None or not os.path.exists(weight_path):
            raise FileNotFoundError('Evaluator: no checkpoint at %r' % (weight_path,))
        state = torch.load(weight_path, map_location='cpu', weights_only=False)
        model.load_state_dict({k.replace('module.', ''): v for k, v in state['model'].items()})
        model.eval()
        self.model, self.amp, self.is_kd = model, _Amp(amp), isinstance(model, KD.TSDFull)
        self.num_classes, self.ignore_label, self.skip_class = int(num_classes), int(ignore_label), int(skip_class)
        self.metric = MeanIoU(self.num_classes, self.ignore_label, 'outputs_vox', 'targets', name='iou/vox')
        self.counts = None

    def before_epoch(self):
        self.model.eval()
        self.metric.before_epoch()
        self.counts = None

    @torch.no_grad()
    def logits(self, d):
        """The voxel logits ``x_vox`` of the device batch ``d`` (all copies of all scans: one forward)."""
        from . import deferred, torchsparse as ts
        from .train import KDStep
        deferred.set_reduced_precision(self.amp.enabled)
        with self.amp.autocast():
            if self.is_kd:
                return self.model(KDStep._in_mod(d))['stu']['x_vox']
            return self.model({'lidar': ts.SparseTensor(d['feats'], d['coords'])})['x_vox']

    @torch.no_grad()
    def __call__(self, d):
        """One step: the reference's dictionary, tensors on the device -- ``outputs_vox`` [P] and ``targets`` [P] over the
        key-frame points of the batch's scans in scan order, ``lidar_token_list`` and ``num_pts`` per scan."""
        assert not self.model.training, 'Evaluator: the model left eval() (core/nusc_trainers.py:486-487)'
        v = d['vote']
        out = self.logits(d)
        if self.counts is None:
            self.counts = torch.zeros(3, self.num_classes, dtype=torch.int64, device=out.device)
        pred = vote_point_predictions(out, v['inverse_map'], v['copy_point_off'], v['copy_voxel_off'], v['scan_seg'], v['num_vote'],
                                      targets=v['targets'], ignore_label=self.ignore_label, skip_class=self.skip_class,
                                      counts=self.counts)
        return {'outputs_vox': pred, 'targets': v['targets'], 'lidar_token_list': list(v['lidar_tokens']), 'num_pts': list(v['num_pts'])}

    def after_epoch(self):
        """(mIoU, per-class IoUs) of ``MeanIoU`` over the steps since ``before_epoch``."""
        if self.counts is not None:
            self.metric.add_counts(self.counts)
            self.counts = None
        return self.metric.after_epoch()


class SubmissionWriter:
    """The nuScenes lidarseg submission layout: ``DIR/lidarseg/<split>/<lidar_token>_lidarseg.bin`` (one uint8 class per
    key-frame point, in file order) and ``DIR/<split>/submission.json`` with the five ``meta`` booleans."""

    def __init__(self, root, split, use_camera):
        self.root, self.split, self.use_camera = root, split, bool(use_camera)
        self.bin_dir = os.path.join(root, 'lidarseg', split)
        os.makedirs(self.bin_dir, exist_ok=True)
        os.makedirs(os.path.join(root, split), exist_ok=True)
        self.written = []

    def add(self, ret):
        """The scans of one ``Evaluator`` step (its returned dictionary): the one copy to the host of this mode."""
        pred = ret['outputs_vox'].cpu().numpy()
        if pred.shape[0] != sum(ret['num_pts']):
            raise ValueError('SubmissionWriter: %d predictions for %d points' % (pred.shape[0], sum(ret['num_pts'])))
        if pred.size and (pred.min() < 1 or pred.max() > 255):
            raise ValueError('SubmissionWriter: class %d is no legal submission value' % (pred.min() if pred.min() < 1 else pred.max()))
        at = 0
        for token, n in zip(ret['lidar_token_list'], ret['num_pts']):
            path = os.path.join(self.bin_dir, '%s_lidarseg.bin' % token)
            pred[at:at + n].astype(np.uint8).tofile(path)
            self.written.append(path)
            at += n

    def close(self):
        path = os.path.join(self.root, self.split, 'submission.json')
        with open(path, 'w') as f:
            json.dump({'meta': {'use_camera': self.use_camera, 'use_lidar': True, 'use_radar': False, 'use_map': False,
                                'use_external': False}}, f, indent=1)
        return path
