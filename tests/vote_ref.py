"""The voting tail of the reference's evaluator (core/nusc_trainers.py:523-550) in numpy: per copy ``outputs[scene][inv]``,
stack, float32 sum in vote order, first-max arg-max, and MeanIoU's three bincounts -- what csrc/vote.hip is held to, bit for bit.

float32 additions only, one per vote, in vote order, so numpy's elementwise float32 add reproduces the kernel exactly."""
import numpy as np


def vote_scan(logits_per_copy, inverse_per_copy, n_key, skip_class=-1):
    """One scan.  ``logits_per_copy[v]`` [nv_v, C] the voxel logits of copy v (any float dtype numpy can widen exactly to
    float32), ``inverse_per_copy[v]`` [np_v] the voxel of every point of copy v, key-frame points first: only the first
    ``n_key`` take part.  Returns (sums [n_key, C] float32, pred [n_key] int64)."""
    c = logits_per_copy[0].shape[1]
    mapped = [np.asarray(lg, dtype=np.float32)[np.asarray(inv)[:n_key]] for lg, inv in zip(logits_per_copy, inverse_per_copy)]
    stack = np.stack(mapped, 0)                                   # torch.stack(_outputs_vox, 0)
    sums = np.zeros((n_key, c), dtype=np.float32)
    for v in range(stack.shape[0]):                               # torch.sum(dim=0) written in vote order
        sums = sums + stack[v]
    assert sums.dtype == np.float32
    if n_key == 0:
        return sums, np.zeros(0, np.int64)
    if skip_class >= 0:
        rest = np.delete(sums, skip_class, axis=1)
        pred = np.argmax(rest, axis=1)                            # first maximum; the first NaN if there is one
        pred = pred + (pred >= skip_class)
    else:
        pred = np.argmax(sums, axis=1)
    return sums, pred.astype(np.int64)


def counters(pred, targets, num_classes, ignore_label):
    """[3, C] int64: seen, correct, predicted over the points whose target is a class other than ``ignore_label`` (a target
    outside [0, C) is counted nowhere)."""
    pred, targets = np.asarray(pred, np.int64), np.asarray(targets, np.int64)
    keep = (targets != ignore_label) & (targets >= 0) & (targets < num_classes)
    p, t = pred[keep], targets[keep]
    return np.stack([np.bincount(t, minlength=num_classes), np.bincount(t[p == t], minlength=num_classes),
                     np.bincount(p, minlength=num_classes)]).astype(np.int64)


def vote_batch(logits, inverse_map, copy_point_off, copy_voxel_off, scan_seg, n_votes, targets=None, ignore_label=0, skip_class=-1):
    """The kernel's layout: S scans x ``n_votes`` copies, copy (s, v) = sample s * n_votes + v; ``logits`` [Nv, C] float32.
    Returns (sums [P, C], pred [P], counts [3, C] or None)."""
    logits, inverse_map = np.asarray(logits, np.float32), np.asarray(inverse_map)
    c, n_scans = logits.shape[1], len(scan_seg) - 1
    sums, pred = [np.zeros((0, c), np.float32)], [np.zeros(0, np.int64)]
    for s in range(n_scans):
        n_key = int(scan_seg[s + 1] - scan_seg[s])
        lg, inv = [], []
        for v in range(n_votes):
            b = s * n_votes + v
            rows = inverse_map[int(copy_point_off[b]):int(copy_point_off[b]) + n_key]
            inv.append(rows)
            # (the copy's voxel rows start at copy_voxel_off[b]; its row count is whatever the inverse map reaches)
            hi = int(rows.max()) + 1 if n_key else 0
            lg.append(logits[int(copy_voxel_off[b]):int(copy_voxel_off[b]) + hi])
        a, b_ = vote_scan(lg, inv, n_key, skip_class)
        sums.append(a); pred.append(b_)
    sums, pred = np.concatenate(sums, 0), np.concatenate(pred, 0)
    counts = counters(pred, targets, c, ignore_label) if targets is not None else None
    return sums, pred, counts
