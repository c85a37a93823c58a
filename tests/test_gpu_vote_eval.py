"""The voting evaluator end to end on the GPU: voting batches through the device loader path against its numpy specification,
``evaluate.Evaluator`` against the existing eval branch (one vote) and against the numpy restatement of the reference's voting
tail (tests/vote_ref.py) applied to the logits the model produced, and ``run_evaluation.py`` as a child process.  Every
comparison is exact."""
import json
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import vote_ref as V
from nusc_tree import build_tree
from test_gpu_device_prep import compare, spec_batch
from test_gpu_run_training import _configs
from u2mkd_amd.data import nuscenes_lc as D

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return build_tree(str(tmp_path_factory.mktemp('nusc')))


@pytest.fixture(scope='module')
def tables(tree):
    return D.NuScenesTables(*tree)


def dataset(tables, seed, multisweeps=1, im_cr=0.08):
    return D.LCNuScenesDataset(tables, voxel_size=0.05, split='val', im_cr=im_cr, im_drop=3, flip=True, multisweeps=multisweeps,
                               only_past=False, rng=np.random.default_rng(seed))


def vote_batch(tables, seed, num_vote, **kw):
    view = D.VoteView(dataset(tables, seed, **kw), num_vote)
    return view.collate_fn([view[i] for i in range(len(view))])


# ------------------------------------------------------------------------------------------------ the device batch
def _check_tables(vote, samples, side, num_vote, batch):
    """The voting tables against the specification's per-copy sizes (``side``: the network input they describe)."""
    n_pts = [s[side]['inverse_map'].shape[0] for s in samples]
    n_vox = [s[side]['num_vox'] for s in samples]
    n_key = [batch[b]['points'].shape[0] for b in range(0, len(batch), num_vote)]
    assert vote['num_vote'] == num_vote and vote['num_pts'] == n_key
    assert vote['lidar_tokens'] == [batch[b]['lidar_token'] for b in range(0, len(batch), num_vote)]
    for key, want in (('copy_point_off', np.cumsum([0] + n_pts)[:-1]), ('copy_voxel_off', np.cumsum([0] + n_vox)[:-1]),
                      ('scan_seg', np.cumsum([0] + n_key))):
        assert vote[key].is_cuda and vote[key].dtype == torch.int32 and vote[key].tolist() == want.tolist(), key
    assert torch.equal(vote['inverse_map'].cpu(), torch.from_numpy(np.concatenate([s[side]['inverse_map'] for s in samples])))
    assert torch.equal(vote['targets'].cpu(), torch.from_numpy(np.concatenate([batch[b]['labels'] for b in range(0, len(batch), num_vote)])))


@pytest.mark.parametrize('multisweeps', [0, 1])
def test_a_voting_batch_equals_the_specification_copy_by_copy(hip, tables, multisweeps):
    from u2mkd_amd.data import device_prep
    batch = vote_batch(tables, 11, 3, multisweeps=multisweeps, im_cr=0.04)
    assert len(batch) == 6
    want, samples = spec_batch(list(batch))
    got = device_prep.prepare_kd_batch(batch)
    torch.cuda.synchronize()
    _check_tables(got.pop('vote'), samples, 'student', 3, batch)
    compare(got, want)
    lid = device_prep.prepare_lidar_batch(batch)
    _check_tables(lid.pop('vote'), samples, 'teacher', 3, batch)
    names = {'feats': 't_feats', 'coords': 't_coords', 'targets': 'targets_t', 'keyframe_mask_full': 'keyframe_mask_full',
             'inverse_map': 'inverse_map', 'num_pts': 'num_pts', 'num_vox': 'num_vox_t'}
    compare({k: lid[k] for k in names}, {k: want[v] for k, v in names.items()}, '/lidar')
    if multisweeps:
        assert lid['num_pts'][0] > batch[0]['points'].shape[0]                    # sweep points sit behind the key-frame points
    # the copies differ (drawn parameters), and the same samples as a plain list carry no tables
    nv = samples[0]['teacher']['num_vox']
    assert not np.array_equal(samples[0]['teacher']['coords'], samples[1]['teacher']['coords'][:nv])
    assert 'vote' not in device_prep.prepare_lidar_batch(list(batch))
    with pytest.raises(ValueError, match='voting batch'):
        device_prep.prepare_lidar_batch(D.VoteBatch([batch[0], batch[3]], 2))      # two different scans are not two votes of one


def _host_reads(fn):
    """(wait_counts calls, Tensor.item / tolist / cpu / __bool__ calls, synchronising calls torch reports) of ``fn()``."""
    from test_gpu_device_prep import HOST_READS, _sync_debug_mode_works
    from u2mkd_amd.torchsparse.nn import functional as spf
    sync_mode = _sync_debug_mode_works()
    calls, waits = [], []
    real_wait = spf.wait_counts
    with pytest.MonkeyPatch.context() as mp, warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        mp.setattr(spf, 'wait_counts', lambda h, *a: (waits.append(h.seq), real_wait(h, *a))[1])
        for name in HOST_READS:
            real = getattr(torch.Tensor, name)
            mp.setattr(torch.Tensor, name, lambda self, *a, _real=real, _name=name, **kw: (calls.append(_name), _real(self, *a, **kw))[1])
        if sync_mode:
            torch.cuda.set_sync_debug_mode('warn')
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode('default')
    reported = [str(w.message) for w in seen if 'synchroniz' in str(w.message)]
    return out, len(waits), calls, reported


@pytest.mark.parametrize('kd', [False, True])
def test_the_voting_tables_add_no_host_read(hip, tables, kd):
    """``prepare_*_batch`` of a ``VoteBatch`` reads back exactly what it reads for the same samples as a plain list -- the one
    read of the sizes -- and building the tables themselves (``_vote_tables``) reads nothing."""
    from u2mkd_amd.data import device_prep
    prepare = device_prep.prepare_kd_batch if kd else device_prep.prepare_lidar_batch
    batch = vote_batch(tables, 12, 3, im_cr=0.04)
    prepare(batch)                                                                # (library, mailbox and allocator warmed up)
    torch.cuda.synchronize()
    _, plain_waits, plain_calls, plain_reported = _host_reads(lambda: prepare(list(batch)))
    got, waits, calls, reported = _host_reads(lambda: prepare(batch))
    print('plain list:', plain_waits, plain_calls, plain_reported, 'voting batch:', waits, calls, reported)
    assert 'vote' in got and waits == plain_waits == 1 and calls == plain_calls and len(reported) == len(plain_reported)
    # the tables alone, on the state of a call: nothing at all
    seen = {}
    real = device_prep._vote_tables
    def spy(u, st, inverse_map):
        seen['args'] = (u, st, inverse_map)
        return real(u, st, inverse_map)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(device_prep, '_vote_tables', spy)
        prepare(batch)
    torch.cuda.synchronize()
    vote, waits, calls, reported = _host_reads(lambda: real(*seen['args']))
    assert waits == 0 and calls == [] and reported == [], (waits, calls, reported)
    assert torch.equal(vote['scan_seg'], got['vote']['scan_seg']) and vote['num_pts'] == got['vote']['num_pts']


# ------------------------------------------------------------------------------------------------ the evaluator
def _save(model, path):
    torch.save({'model': {'module.' + k: v for k, v in model.state_dict().items()}}, path)      # as a DDP-wrapped trainer saves it


def _capture(ev):
    seen, real = [], ev.logits
    ev.logits = lambda d: (seen.append(real(d)), seen[-1])[1]
    return seen


def _reference(logits, vote, skip_class=-1):
    cpu = lambda t: t.cpu().numpy()
    return V.vote_batch(logits.float().cpu().numpy(), cpu(vote['inverse_map']), cpu(vote['copy_point_off']), cpu(vote['copy_voxel_off']),
                        cpu(vote['scan_seg']), vote['num_vote'], targets=cpu(vote['targets']), ignore_label=0, skip_class=skip_class)


def _run_votes(ev, prepare, tables, seed, num_vote, skip_class=-1):
    """One epoch of one step over the tree's two scans: (returned dictionary, counters, the logits the model produced, tables)."""
    seen = _capture(ev)
    ev.skip_class = skip_class
    ev.before_epoch()
    d = prepare(vote_batch(tables, seed, num_vote))
    ret = ev(d)
    del ev.logits                                    # (the instance attribute: the method is back)
    counts = ev.counts.clone()
    return ret, counts, seen[-1], d['vote'], ev.after_epoch()


def _check_against_reference(ret, counts, logits, vote, skip_class=-1):
    _, w_pred, w_counts = _reference(logits, vote, skip_class)
    assert torch.equal(ret['outputs_vox'].cpu(), torch.from_numpy(w_pred))
    assert torch.equal(counts.cpu(), torch.from_numpy(w_counts))
    assert torch.equal(ret['targets'], vote['targets']) and ret['num_pts'] == vote['num_pts']
    assert ret['lidar_token_list'] == vote['lidar_tokens'] and sum(ret['num_pts']) == ret['outputs_vox'].shape[0]


def test_teacher_evaluator(hip, tables, tmp_path):
    from u2mkd_amd import lidar, train as T
    from u2mkd_amd.data import device_prep
    from u2mkd_amd.evaluate import Evaluator, MeanIoU
    torch.manual_seed(0)
    model = lidar.SPVCNN_SPFORMER(**lidar.spformer_kwargs(cr=0.5)).cuda()
    path = str(tmp_path / 'teacher.pt')
    _save(model, path)
    torch.manual_seed(1)
    other = lidar.SPVCNN_SPFORMER(**lidar.spformer_kwargs(cr=0.5)).cuda().train()      # other weights, training mode
    ev = Evaluator(other, path, 17)
    assert not other.training and all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), model.state_dict().values()))
    with pytest.raises(FileNotFoundError):
        Evaluator(other, str(tmp_path / 'none.pt'), 17)

    # one vote = the existing eval branch on the plain evaluation samples
    ret, counts, logits, vote, (miou, ious) = _run_votes(ev, device_prep.prepare_lidar_batch, tables, 21, 1)
    ds = dataset(tables, 21)
    plain = device_prep.prepare_lidar_batch([ds.raw(0), ds.raw(1)])
    runner = T.LidarStep(model)
    model.eval()
    want = runner.evaluate(plain['feats'], plain['coords'], plain['inverse_map'], plain['inverse_batch'], plain['targets_mapped'],
                           plain['keyframe_mask_full'])
    assert torch.equal(ret['outputs_vox'], want['outputs_vox']) and torch.equal(ret['targets'], want['targets'])
    m = MeanIoU(17, 0, 'outputs_vox', 'targets')
    m.after_step(want)
    assert (miou, ious) == m.after_epoch() and 0.0 <= miou <= 1.0
    _check_against_reference(ret, counts, logits, vote)

    # four votes: twice with equal seeds bit for bit, and the reference's tail on the logits the model produced
    a = _run_votes(ev, device_prep.prepare_lidar_batch, tables, 22, 4)
    b = _run_votes(ev, device_prep.prepare_lidar_batch, tables, 22, 4)
    assert a[2].shape[0] > 3 * logits.shape[0]                                     # (four copies went through the network)
    assert torch.equal(a[0]['outputs_vox'], b[0]['outputs_vox']) and torch.equal(a[1], b[1]) and a[4] == b[4]
    _check_against_reference(*a[:4])
    assert a[0]['num_pts'] == ret['num_pts'] and torch.equal(a[0]['targets'], ret['targets'])
    # submission mode, and 16-bit logits under autocast
    s = _run_votes(ev, device_prep.prepare_lidar_batch, tables, 22, 4, skip_class=0)
    _check_against_reference(*s[:4], skip_class=0)
    assert int(s[0]['outputs_vox'].min()) >= 1
    ev16 = Evaluator(other, path, 17, amp='bf16')
    h = _run_votes(ev16, device_prep.prepare_lidar_batch, tables, 22, 4)
    assert h[2].dtype == torch.bfloat16
    _check_against_reference(*h[:4])


def test_kd_evaluator(hip, tables, tmp_path):
    from u2mkd_amd import kd as KD, lidar, train as T
    from u2mkd_amd.data import device_prep
    from u2mkd_amd.evaluate import Evaluator, MeanIoU
    sp = {k: v for k, v in lidar.spformer_kwargs().items() if k not in ('cr', 'in_channel', 'num_classes')}
    build = lambda: KD.TSDFull(cr=0.5, cr_t=0.5, in_channel=4, in_channel_t=4, num_classes=17, spformer=sp).cuda()
    torch.manual_seed(0)
    model = build()
    path = str(tmp_path / 'kd.pt')
    _save(model, path)
    saved = {k: v.clone() for k, v in model.state_dict().items()}
    # ONE model object on both sides, its weights spoiled before the evaluator loads the checkpoint into it: the camera branch
    # runs on MIOpen, whose choices make the first model objects of a process at a new set of shapes differ in the third digit
    # although their weights are equal, and two forwards of one object differ in the last bits unless its deterministic
    # choices are asked for (NOTES N6, N30.3) -- none of which is the evaluator's
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(0.5)
    ev = Evaluator(model.train(), path, 17)
    assert ev.is_kd and not ev.model.training and all(torch.equal(v, saved[k]) for k, v in model.state_dict().items())
    was, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    try:
        ret, counts, logits, vote, (miou, ious) = _run_votes(ev, device_prep.prepare_kd_batch, tables, 31, 1)
        ds = dataset(tables, 31)
        d, f = device_prep.prepare_kd_batch([ds.raw(0), ds.raw(1)], with_eval=True)
        runner = T.KDStep(model)
        model.eval()
        want = runner.evaluate(d, f['s_inverse_map'], f['s_inverse_batch'], f['targets_mapped'], f['label_fov'])
        assert torch.equal(ret['outputs_vox'], want['outputs_vox']) and torch.equal(ret['targets'], want['targets'])
        m = MeanIoU(17, 0, 'outputs_vox', 'targets')
        m.after_step(want)
        assert (miou, ious) == m.after_epoch()
        _check_against_reference(ret, counts, logits, vote)
        a = _run_votes(ev, device_prep.prepare_kd_batch, tables, 32, 4)
        b = _run_votes(ev, device_prep.prepare_kd_batch, tables, 32, 4)
    finally:
        torch.backends.cudnn.deterministic = was
    assert a[2].shape[0] > 3 * logits.shape[0]
    assert torch.equal(a[0]['outputs_vox'], b[0]['outputs_vox']) and torch.equal(a[1], b[1]) and a[4] == b[4]
    _check_against_reference(*a[:4])
    _check_against_reference(*b[:4])


# ------------------------------------------------------------------------------------------------ the entry script
def test_run_evaluation_as_a_child_process(hip, tree, tmp_path):
    import run_evaluation
    from u2mkd_amd import builder
    root, ver = tree
    cfgs = _configs(tmp_path, root=root, version=ver, im_cr=0.08)
    cfg_file = os.path.join(cfgs, 'spformer.yaml')
    torch.manual_seed(0)
    ckpt = str(tmp_path / 'teacher.pt')
    _save(builder.make_model(builder.Config.load(cfg_file, recursive=True)), ckpt)
    args = [cfg_file, '--weight-path', ckpt, '--dataset.num_vote', '3', '--train.seed', '7']
    cwd = os.getcwd()
    os.chdir(tmp_path)                      # no ./data/nuscenes/*_official.npy here: the split holds every sample
    try:
        here = run_evaluation.main(args + ['--submission-dir', str(tmp_path / 'sub_here')])
    finally:
        os.chdir(cwd)
    assert here['steps'] == 1 and here['num_vote'] == 3 and 0.0 <= here['miou'] <= 1.0 and len(here['ious']) == 16
    r = subprocess.run(['timeout', '-k', '10', '300', sys.executable, os.path.join(REPO, 'run_evaluation.py')] + args
                       + ['--submission-dir', str(tmp_path / 'sub_child')], cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    printed = re.search(r'mIoU (\S+)', r.stdout)
    assert printed and float(printed.group(1)) == here['miou'], (r.stdout[-2000:], here['miou'])
    tables = D.NuScenesTables(root, ver)
    for sub in ('sub_here', 'sub_child'):
        meta = json.load(open(tmp_path / sub / 'val' / 'submission.json'))['meta']
        assert meta == {'use_camera': False, 'use_lidar': True, 'use_radar': False, 'use_map': False, 'use_external': False}
        files = sorted(os.listdir(tmp_path / sub / 'lidarseg' / 'val'))
        assert files == sorted('%s_lidarseg.bin' % s['data']['LIDAR_TOP'] for s in tables.sample)
        for s in tables.sample:
            token = s['data']['LIDAR_TOP']
            n_key = os.path.getsize(os.path.join(root, tables.get('sample_data', token)['filename'])) // 20      # [N, 5] float32
            got = np.fromfile(str(tmp_path / sub / 'lidarseg' / 'val' / ('%s_lidarseg.bin' % token)), dtype=np.uint8)
            assert got.shape[0] == n_key and got.min() >= 1 and got.max() <= 16
    # --synthetic: seeded synthetic scans instead of the tree, one step of two votes
    syn = run_evaluation.main([cfg_file, '--weight-path', ckpt, '--dataset.num_vote', '2', '--synthetic', '2500', '--max-iters', '1',
                               '--submission-dir', str(tmp_path / 'sub_syn')])
    assert syn['steps'] == 1 and syn['num_vote'] == 2 and 0.0 <= syn['miou'] <= 1.0
    syn_files = sorted(os.listdir(tmp_path / 'sub_syn' / 'lidarseg' / 'val'))
    assert len(syn_files) == 2 and all(os.path.getsize(tmp_path / 'sub_syn' / 'lidarseg' / 'val' / f) == 2500 for f in syn_files)
    for name in os.listdir(tmp_path / 'sub_here' / 'lidarseg' / 'val'):
        assert open(tmp_path / 'sub_here' / 'lidarseg' / 'val' / name, 'rb').read() == open(tmp_path / 'sub_child' / 'lidarseg' / 'val' / name, 'rb').read()
