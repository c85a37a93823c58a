"""csrc/vote.hip (``evaluate.vote_point_predictions``) against the numpy restatement of the reference's voting tail
(tests/vote_ref.py), EXACTLY: sums, predictions and the three MeanIoU counters.  The kernel only adds, in vote order, in fp32 --
there is nothing to tolerate."""
import warnings

import numpy as np
import pytest
import torch

import vote_ref as V
from u2mkd_amd.evaluate import MeanIoU, vote_point_predictions, voxel_logits_to_point_predictions

pytestmark = pytest.mark.gpu

HOST_READS = ('item', 'tolist', 'cpu', '__bool__')
SIZES = [0, 1, 63, 64, 65, 257, 1000]
SCANS = [(n,) for n in SIZES] + [(63, 0, 257), (1000, 1, 65), (0, 64, 0)]      # one scan of every size; three unequal scans
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}


def make_case(rng, scan_sizes, n_votes, c, dtype, dense, integer=False):
    """A batch in the kernel's layout.  Every copy has its own voxel count and its own number of sweep points behind the
    key-frame points; ``dense``: many points per voxel, else one point per voxel (the inverse map is a permutation)."""
    inv, cpo, cvo, n_pts, n_vox = [], [], [], 0, 0
    for s, n_key in enumerate(scan_sizes):
        for v in range(n_votes):
            n_sweep = int(rng.integers(0, 40))
            n = n_key + n_sweep
            nv = max(1, n // 7 + v) if dense else max(1, n)
            rows = rng.integers(0, nv, n) if dense else rng.permutation(nv)[:n]
            inv.append(rows.astype(np.int64)); cpo.append(n_pts); cvo.append(n_vox)
            n_pts += n; n_vox += nv
    if integer:
        logits = rng.integers(-2, 3, (n_vox, c)).astype(np.float32)              # small integers: many exact ties
    else:
        logits = (rng.standard_normal((n_vox, c)) * 3).astype(np.float32)
    logits = torch.from_numpy(logits).to(dtype)
    p = int(sum(scan_sizes))
    targets = rng.integers(0, max(c, 2), p).astype(np.int64)                      # (0 = the ignore label; c = 1: 1 is out of range)
    host = dict(logits=logits.float().numpy(), inverse_map=np.concatenate(inv) if inv else np.zeros(0, np.int64),
                copy_point_off=np.asarray(cpo, np.int32), copy_voxel_off=np.asarray(cvo, np.int32), scan_seg=np.cumsum([0] + list(scan_sizes)).astype(np.int32),
                n_votes=n_votes, targets=targets)
    dev = {k: (torch.from_numpy(np.ascontiguousarray(x)).cuda() if isinstance(x, np.ndarray) else x) for k, x in host.items()}
    dev['logits'] = logits.cuda()
    return host, dev


def same_sums(got, want):
    want = torch.from_numpy(want)
    g = got.cpu()
    return g.shape == want.shape and bool(((g == want) | (torch.isnan(g) & torch.isnan(want))).all())


def run_and_compare(host, dev, ignore_label=0, skip_class=-1):
    c = host['logits'].shape[1]
    counts = torch.zeros(3, c, dtype=torch.int64, device='cuda')
    pred, sums = vote_point_predictions(**dev, ignore_label=ignore_label, skip_class=skip_class, want_sums=True, counts=counts)
    w_sums, w_pred, w_counts = V.vote_batch(**host, ignore_label=ignore_label, skip_class=skip_class)
    assert pred.dtype == torch.int64 and sums.dtype == torch.float32 and sums.shape == (w_pred.shape[0], c)
    assert torch.equal(sums.cpu(), torch.from_numpy(w_sums))
    assert torch.equal(pred.cpu(), torch.from_numpy(w_pred))
    assert torch.equal(counts.cpu(), torch.from_numpy(w_counts))
    return pred, sums, counts


@pytest.mark.parametrize('row', sorted(DTYPES))
@pytest.mark.parametrize('c', [1, 2, 17, 20, 64])
def test_against_the_reference(hip, c, row):
    rng = np.random.default_rng(100 * c + len(row))
    n = 0
    for n_votes in (1, 2, 3, 12):
        for k, scan_sizes in enumerate(SCANS):
            host, dev = make_case(rng, scan_sizes, n_votes, c, DTYPES[row], dense=bool((k + n_votes) % 2))
            run_and_compare(host, dev)
            n += 1
    assert n == 40


def test_counts_accumulate_and_optional_outputs(hip):
    rng = np.random.default_rng(1)
    host, dev = make_case(rng, (257, 65), 3, 17, torch.float32, dense=True)
    pred, sums, counts = run_and_compare(host, dev)
    once = counts.clone()
    assert int(once.sum()) > 0
    p2 = vote_point_predictions(**dev, counts=counts)                                # no sums; the counters are ADDED to
    assert torch.equal(p2, pred) and torch.equal(counts, 2 * once)
    p3 = vote_point_predictions(**dev)                                                # neither
    p4 = vote_point_predictions(**{k: v for k, v in dev.items() if k != 'targets'}, num_points=pred.shape[0])   # no targets at all
    assert torch.equal(p3, pred) and torch.equal(p4, pred) and torch.equal(counts, 2 * once)
    p5, s5 = vote_point_predictions(**dev, want_sums=True)
    assert torch.equal(p5, pred) and torch.equal(s5, sums)
    # another ignore label: class 0 is counted, class 3 is not
    run_and_compare(host, dev, ignore_label=3)
    # targets outside the classes (and not the ignore label) are counted nowhere
    host['targets'][::5] = 17
    host['targets'][1::5] = -1
    dev['targets'] = torch.from_numpy(host['targets']).cuda()
    run_and_compare(host, dev)


@pytest.mark.parametrize('row', sorted(DTYPES))
def test_ties_take_the_lowest_class(hip, row):
    rng = np.random.default_rng(2)
    for n_votes in (1, 2, 3):
        host, dev = make_case(rng, (1000, 63), n_votes, 20, DTYPES[row], dense=True, integer=True)
        pred, sums, _ = run_and_compare(host, dev)
        top = sums.max(1, keepdim=True).values
        tied = (sums == top).sum(1) > 1
        assert int(tied.sum()) > 100                                              # the case does force ties
        first = (sums == top).float().cpu().argmax(1)
        assert torch.equal(pred.cpu(), first)


def test_a_nan_row_is_maximal(hip):
    rng = np.random.default_rng(3)
    host, dev = make_case(rng, (300,), 3, 17, torch.float32, dense=True)
    row = int(host['copy_voxel_off'][1]) + int(host['inverse_map'][int(host['copy_point_off'][1]) + 5])   # point 5's voxel in copy 1
    host['logits'][row, 4] = np.nan
    host['logits'][row, 9] = np.nan
    dev['logits'] = torch.from_numpy(host['logits']).cuda()
    counts = torch.zeros(3, 17, dtype=torch.int64, device='cuda')
    pred, sums = vote_point_predictions(**dev, want_sums=True, counts=counts)
    w_sums, w_pred, w_counts = V.vote_batch(**host)
    assert np.isnan(w_sums[5, 4]) and w_pred[5] == 4 and int(torch.isnan(sums).sum()) >= 2
    assert same_sums(sums, w_sums) and torch.equal(pred.cpu(), torch.from_numpy(w_pred)) and torch.equal(counts.cpu(), torch.from_numpy(w_counts))
    assert torch.equal(pred.cpu(), torch.from_numpy(w_sums).argmax(1))            # torch.argmax on the CPU, NaN included


def test_skip_class(hip):
    rng = np.random.default_rng(4)
    host, dev = make_case(rng, (257, 64), 2, 17, torch.float32, dense=True)
    host['logits'][::2, 0] = 50.0                                                 # class 0 holds the maximum of half the rows
    dev['logits'] = torch.from_numpy(host['logits']).cuda()
    plain, _, _ = run_and_compare(host, dev)
    assert int((plain == 0).sum()) > 50
    pred, sums, _ = run_and_compare(host, dev, skip_class=0)
    assert int(pred.min()) >= 1 and torch.equal(pred[plain != 0], plain[plain != 0])
    assert torch.equal(pred, sums[:, 1:].argmax(1) + 1)
    run_and_compare(host, dev, skip_class=16)
    run_and_compare(*make_case(rng, (65,), 3, 2, torch.bfloat16, dense=False), skip_class=1)


def test_one_vote_is_the_existing_eval_branch(hip):
    """V = 1: ``pred`` = voxel_logits_to_point_predictions (key-frame points only) and ``counts`` = MeanIoU.after_step's update."""
    rng = np.random.default_rng(5)
    for dtype in DTYPES.values():
        host, dev = make_case(rng, (257, 1, 1000), 1, 17, dtype, dense=True)
        n_pts = np.diff(np.append(host['copy_point_off'], host['inverse_map'].shape[0]))
        n_key = np.diff(host['scan_seg'])
        voxel_batch = torch.from_numpy(np.repeat(np.arange(3), np.diff(np.append(host['copy_voxel_off'], host['logits'].shape[0])))).cuda()
        inverse_batch = torch.from_numpy(np.repeat(np.arange(3), n_pts)).cuda()
        keyframe = torch.from_numpy(np.concatenate([np.arange(n) < k for n, k in zip(n_pts, n_key)])).cuda()
        want = voxel_logits_to_point_predictions(dev['logits'], voxel_batch, dev['inverse_map'], inverse_batch, keyframe)
        counts = torch.zeros(3, 17, dtype=torch.int64, device='cuda')
        pred = vote_point_predictions(**dev, counts=counts)
        assert torch.equal(pred, want)
        m = MeanIoU(17, 0, 'outputs_vox', 'targets')
        m.after_step({'outputs_vox': want, 'targets': dev['targets']})
        assert torch.equal(counts.double(), m._dev)
        n = MeanIoU(17, 0, 'outputs_vox', 'targets')
        n.add_counts(counts)
        assert n.after_epoch() == m.after_epoch()


def _sync_debug_mode_works():
    t = torch.ones(1, device='cuda')
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            t.item()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    return any('synchroniz' in str(w.message) for w in seen)


def test_no_host_read(hip):
    """The call reads nothing back: zero calls of Tensor.item / tolist / cpu / __bool__ and, where
    ``torch.cuda.set_sync_debug_mode('warn')`` reports a host read on this build (probed first), no synchronising call."""
    rng = np.random.default_rng(6)
    host, dev = make_case(rng, (1000, 257), 4, 17, torch.bfloat16, dense=True)
    counts = torch.zeros(3, 17, dtype=torch.int64, device='cuda')
    vote_point_predictions(**dev, counts=counts, want_sums=True)                  # (library and allocator warmed up)
    torch.cuda.synchronize()
    sync_mode = _sync_debug_mode_works()
    print('set_sync_debug_mode reports host reads on this build:', sync_mode)
    calls = []
    with pytest.MonkeyPatch.context() as mp, warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        for name in HOST_READS:
            real = getattr(torch.Tensor, name)
            mp.setattr(torch.Tensor, name, lambda self, *a, _real=real, _name=name, **kw: (calls.append(_name), _real(self, *a, **kw))[1])
        if sync_mode:
            torch.cuda.set_sync_debug_mode('warn')
        try:
            pred, sums = vote_point_predictions(**dev, counts=counts, want_sums=True)
            m = MeanIoU(17, 0)
            m.add_counts(counts)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    reported = [str(w.message) for w in seen if 'synchroniz' in str(w.message)]
    assert calls == [] and reported == [], (calls, reported)
    w_sums, w_pred, w_counts = V.vote_batch(**host)
    assert torch.equal(pred.cpu(), torch.from_numpy(w_pred)) and torch.equal(counts.cpu(), torch.from_numpy(2 * w_counts))


def test_the_kernel_itself_on_scans_without_points(hip):
    """``vote_point_predictions`` launches nothing for P = 0; the C entry with scans and no point does launch (the point count
    lives on the device) and must touch nothing: no prediction, no sum, no counter."""
    from u2mkd_amd import _lib as L
    logits = torch.randn(5, 17, device='cuda')
    inverse_map = torch.zeros(9, dtype=torch.int64, device='cuda')                 # sweep points only
    off = torch.tensor([0, 4, 0, 2], dtype=torch.int32, device='cuda')             # two scans x two votes
    seg = torch.zeros(3, dtype=torch.int32, device='cuda')
    targets = torch.ones(1, dtype=torch.int64, device='cuda')
    pred = torch.full((4,), -7, dtype=torch.int64, device='cuda')
    sums = torch.full((4, 17), -7.0, device='cuda')
    counts = torch.zeros(3, 17, dtype=torch.int64, device='cuda')
    L.call('u2mkd_vote_points', L.ptr(logits), 0, 17, L.ptr(inverse_map), L.ptr(off), L.ptr(off), L.ptr(seg), 2, 2, L.ptr(targets), 0, -1,
           L.ptr(sums), L.ptr(pred), L.ptr(counts), L.stream())
    torch.cuda.synchronize()
    assert bool((pred == -7).all()) and bool((sums == -7.0).all()) and int(counts.abs().sum()) == 0
    empty = vote_point_predictions(logits, inverse_map, off, off, seg, 2, targets=targets[:0], counts=counts, want_sums=True)
    assert empty[0].shape == (0,) and empty[1].shape == (0, 17) and int(counts.abs().sum()) == 0
