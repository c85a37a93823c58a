"""Test-time voting, host side (no GPU): the numpy restatement of the reference's voting tail (tests/vote_ref.py), the votes as
raw samples (``LCNuScenesDataset.raw_votes``, ``VoteView``), the submission files, the ``dataset.num_vote`` setting and the
argument checks of ``evaluate.vote_point_predictions``."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

import device_prep_ref as R
import vote_ref as V
from nusc_tree import build_tree
from test_builder import ROOT as CFG_ROOT, SPFORMER, TRAIN_DEFAULT
from u2mkd_amd import _lib, builder
from u2mkd_amd.data import nuscenes_lc as D
from u2mkd_amd.evaluate import MeanIoU, SubmissionWriter, vote_point_predictions

IM_CR = 0.04


@pytest.fixture(scope='module')
def tables(tmp_path_factory):
    root, ver = build_tree(str(tmp_path_factory.mktemp('nusc')))
    return D.NuScenesTables(root, ver)


def dataset(tables, split, seed, multisweeps=1, im_drop=3):
    return D.LCNuScenesDataset(tables, voxel_size=0.05, split=split, im_cr=IM_CR, im_drop=im_drop, flip=True,
                               multisweeps=multisweeps, only_past=False, rng=np.random.default_rng(seed))


# ------------------------------------------------------------------------------------------------ the reference function
def test_reference_on_a_hand_written_case():
    """Two votes, three classes, three key-frame points (copy 1 has a sweep point behind them).  Point 2 is class 1 for copy 0
    alone and class 0 for copy 1 alone; the sum ties classes 0 and 1 -> the lower one.  Point 1's target is the ignore label."""
    l0 = np.float32([[1, 2, 0], [0, 0, 5]])
    l1 = np.float32([[1, 0, 2], [2, 1, 0], [0, 5, 0]])
    inv0, inv1 = np.array([0, 1, 0]), np.array([2, 0, 1, 1])
    sums, pred = V.vote_scan([l0, l1], [inv0, inv1], 3)
    assert sums.dtype == np.float32 and sums.tolist() == [[1, 7, 0], [1, 0, 7], [3, 3, 0]]
    assert pred.tolist() == [1, 2, 0]
    assert V.vote_scan([l0], [inv0], 3)[1].tolist() == [1, 2, 1] and V.vote_scan([l1], [inv1], 3)[1].tolist() == [1, 2, 0]
    counts = V.counters(pred, [1, 0, 1], 3, ignore_label=0)
    assert counts.tolist() == [[0, 2, 0], [0, 1, 0], [1, 1, 0]]
    # the kernel's layout: the same scan as a batch of two samples
    logits = np.concatenate([l0, l1])
    s2, p2, c2 = V.vote_batch(logits, np.concatenate([inv0, inv1]), [0, 3], [0, 2], [0, 3], 2, targets=np.array([1, 0, 1]))
    assert np.array_equal(s2, sums) and np.array_equal(p2, pred) and np.array_equal(c2, counts)
    # class 0 left out (submission mode): the tie is gone, and a point whose maximum is class 0 takes its runner-up
    assert V.vote_scan([l0, l1], [inv0, inv1], 3, skip_class=0)[1].tolist() == [1, 2, 1]
    assert V.vote_scan([np.float32([[9, 1, 2]])], [np.array([0])], 1, skip_class=0)[1].tolist() == [2]
    # a target outside the classes is counted nowhere; NaN is maximal
    assert V.counters([1, 2], [7, 2], 3, 0).tolist() == [[0, 0, 1], [0, 0, 1], [0, 0, 1]]
    assert V.vote_scan([np.float32([[1, np.nan, 5]])], [np.array([0])], 1)[1].tolist() == [1]


def test_counters_are_mean_iou_after_step():
    rng = np.random.default_rng(0)
    pred, tgt = rng.integers(0, 17, 500), rng.integers(0, 17, 500)
    m = MeanIoU(17, 0, 'outputs_vox', 'targets')
    m.after_step({'outputs_vox': torch.from_numpy(pred), 'targets': torch.from_numpy(tgt)})
    want = m._dev.clone()
    assert torch.equal(want, torch.from_numpy(V.counters(pred, tgt, 17, 0)).double())
    n = MeanIoU(17, 0, 'outputs_vox', 'targets')
    n.add_counts(torch.from_numpy(V.counters(pred[:200], tgt[:200], 17, 0)))
    n.add_counts(torch.from_numpy(V.counters(pred[200:], tgt[200:], 17, 0)))
    assert torch.equal(n._dev, want) and n.after_epoch() == m.after_epoch()
    with pytest.raises(ValueError):
        n.add_counts(torch.zeros(3, 16, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ votes as raw samples
def _same_params(a, b):
    return (np.array_equal(a['teacher']['rot'], b['teacher']['rot']) and a['teacher']['scale'] == b['teacher']['scale']
            and a['teacher']['flip'] == b['teacher']['flip'] and np.array_equal(a['student']['rot'], b['student']['rot'])
            and a['student']['scale'] == b['student']['scale'])


def test_raw_votes(tables):
    nv = 4
    val = dataset(tables, 'val', 5)
    votes = val.raw_votes(0, nv)
    assert len(votes) == nv and all(v['train'] is True for v in votes)
    # vote 0: identity parameters; the others: drawn
    t0, s0 = votes[0]['teacher'], votes[0]['student']
    assert np.array_equal(t0['rot'], np.eye(3)) and t0['scale'] == 1.0 and t0['flip'] == 0
    assert np.array_equal(s0['rot'], np.eye(3)) and s0['scale'] == 1.0
    assert all(not np.array_equal(v['teacher']['rot'], np.eye(3)) and v['teacher']['scale'] != 1.0 for v in votes[1:])
    # arrays are shared by reference, no camera is dropped (the dataset drops three in training)
    for v in votes[1:]:
        for key in ('points', 'labels', 'sweeps', 'cams', 'images'):
            assert v[key] is votes[0][key], key
        assert v['lidar_token'] == votes[0]['lidar_token']
    assert len(votes[0]['cams']) == 6 and votes[0]['images'].shape[0] == 6
    # labels as in the split; zeros for the test split
    plain = dataset(tables, 'val', 5).raw(0)
    assert np.array_equal(votes[0]['labels'], plain['labels']) and votes[0]['labels'].any()
    test_votes = dataset(tables, 'test', 5).raw_votes(0, 2)
    assert not test_votes[0]['labels'].any() and test_votes[0]['labels'].shape == plain['labels'].shape
    # equal seeds, equal draws; another seed, other draws
    again = dataset(tables, 'val', 5).raw_votes(0, nv)
    assert all(_same_params(a, b) for a, b in zip(votes, again))
    assert not _same_params(votes[1], dataset(tables, 'val', 6).raw_votes(0, nv)[1])
    # the rng is consumed as nv - 1 training raw() calls consume it: same parameters, same state afterwards
    train = dataset(tables, 'train', 5)
    drawn = [train.raw(0) for _ in range(nv - 1)]
    assert all(_same_params(a, b) for a, b in zip(votes[1:], drawn))
    assert train.rng.uniform() == val.rng.uniform()
    # one vote draws nothing
    one = dataset(tables, 'val', 5)
    assert len(one.raw_votes(1, 1)) == 1 and one.rng.uniform() == np.random.default_rng(5).uniform()
    with pytest.raises(ValueError):
        one.raw_votes(0, 0)


@pytest.mark.parametrize('multisweeps', [0, 1])
def test_vote_0_is_the_plain_evaluation_sample(tables, multisweeps):
    """The identity parameters, APPLIED (train = True), leave the specification's batch as the eval split's."""
    vote0 = dataset(tables, 'val', 3, multisweeps).raw_votes(1, 2)[0]
    plain = dataset(tables, 'val', 3, multisweeps).raw(1)
    assert plain['train'] is False and len(plain['cams']) == 6
    a, b = R.prepare_numpy(vote0), R.prepare_numpy(plain)
    for side in ('teacher', 'student'):
        for key in ('feats', 'coords', 'targets', 'inverse_map'):
            assert np.array_equal(a[side][key], b[side][key]), (side, key)
    assert np.array_equal(a['student']['pixel_coordinates'], b['student']['pixel_coordinates'], equal_nan=True)


def test_vote_view_collates_scan_major(tables):
    ds = dataset(tables, 'val', 1)
    view = D.VoteView(ds, 3)
    assert len(view) == len(ds) == 2 and view.rng is ds.rng
    batch = view.collate_fn([view[0], view[1]])
    assert isinstance(batch, D.VoteBatch) and isinstance(batch, list) and batch.num_vote == 3 and len(batch) == 6
    tokens = [ds.sample[i]['data']['LIDAR_TOP'] for i in range(2)]
    assert [r['lidar_token'] for r in batch] == [tokens[0]] * 3 + [tokens[1]] * 3
    assert batch[1]['points'] is batch[0]['points'] and batch[4]['points'] is batch[3]['points']
    assert batch[3]['points'] is not batch[0]['points']
    assert np.array_equal(batch[0]['teacher']['rot'], np.eye(3)) and np.array_equal(batch[3]['teacher']['rot'], np.eye(3))
    loader = torch.utils.data.DataLoader(D.VoteView(dataset(tables, 'val', 1), 3), batch_size=2, collate_fn=view.collate_fn)
    got = next(iter(loader))
    assert isinstance(got, D.VoteBatch) and all(_same_params(a, b) for a, b in zip(got, batch))
    with pytest.raises(ValueError):
        D.VoteBatch(list(batch)[:5], 3)


def test_synthetic_scans_draw_as_the_dataset_does():
    """run_evaluation.SyntheticScans: the on-disk dataset's interface and draw order (nuscenes_lc.draw_sample_parameters)."""
    import run_evaluation
    ds = run_evaluation.SyntheticScans(300, 4, (36, 64), 9, 0.05, sweeps=True)
    votes = D.VoteView(ds, 3)[1]
    assert len(votes) == 3 and all(v['train'] is True for v in votes) and votes[0]['sweeps'] is not None
    assert np.array_equal(votes[0]['teacher']['rot'], np.eye(3)) and votes[0]['teacher']['flip'] == 0 and votes[0]['student']['scale'] == 1.0
    assert all(v[k] is votes[0][k] for v in votes[1:] for k in ('points', 'labels', 'sweeps', 'cams', 'images'))
    rng = np.random.default_rng(9)
    for v in votes[1:]:
        teacher, _, student = D.draw_sample_parameters(rng, True, 0)
        assert _same_params(v, {'teacher': teacher, 'student': student})
    assert ds.rng.uniform() == rng.uniform()
    again = run_evaluation.SyntheticScans(300, 4, (36, 64), 9, 0.05, sweeps=False).raw_votes(1, 3)
    assert again[0]['sweeps'] is None and again[0]['multisweeps'] == 0 and len(again) == 3
    R.prepare_numpy(votes[2])                                                     # a sample the specification accepts


def test_debug_datasets_are_refused_before_any_draw(tables):
    ds = D.LCNuScenesDataset(tables, voxel_size=0.05, split='train', im_cr=IM_CR, debug=True, rng=np.random.default_rng(4))
    for call in (lambda: ds.raw(0), lambda: ds.raw_votes(0, 3)):
        with pytest.raises(NotImplementedError):
            call()
    assert ds.rng.uniform() == np.random.default_rng(4).uniform()


# ------------------------------------------------------------------------------------------------ submission files
def test_submission_writer_round_trip(tmp_path):
    w = SubmissionWriter(str(tmp_path / 'sub'), 'test', use_camera=True)
    w.add({'outputs_vox': torch.tensor([1, 16, 3, 4, 5]), 'targets': None, 'lidar_token_list': ['aaa', 'bbb'], 'num_pts': [3, 2]})
    w.add({'outputs_vox': torch.tensor([7]), 'targets': None, 'lidar_token_list': ['ccc'], 'num_pts': [1]})
    path = w.close()
    assert path == str(tmp_path / 'sub' / 'test' / 'submission.json')
    assert sorted(os.listdir(tmp_path / 'sub' / 'lidarseg' / 'test')) == ['aaa_lidarseg.bin', 'bbb_lidarseg.bin', 'ccc_lidarseg.bin']
    read = lambda t: np.fromfile(str(tmp_path / 'sub' / 'lidarseg' / 'test' / ('%s_lidarseg.bin' % t)), dtype=np.uint8)
    assert read('aaa').tolist() == [1, 16, 3] and read('bbb').tolist() == [4, 5] and read('ccc').tolist() == [7]
    assert all(0 not in read(t) for t in ('aaa', 'bbb', 'ccc'))
    meta = json.load(open(path))
    assert meta == {'meta': {'use_camera': True, 'use_lidar': True, 'use_radar': False, 'use_map': False, 'use_external': False}}
    lidar_only = SubmissionWriter(str(tmp_path / 'sub2'), 'val', use_camera=False)
    assert json.load(open(lidar_only.close()))['meta']['use_camera'] is False
    with pytest.raises(ValueError, match='legal'):
        lidar_only.add({'outputs_vox': torch.tensor([1, 0]), 'lidar_token_list': ['x'], 'num_pts': [2]})
    with pytest.raises(ValueError):
        lidar_only.add({'outputs_vox': torch.tensor([1, 2]), 'lidar_token_list': ['x'], 'num_pts': [3]})


# ------------------------------------------------------------------------------------------------ the setting
def test_num_vote_default_and_override(tmp_path):
    import run_evaluation
    d = tmp_path / 'configs' / 'nuscenes' / 'train'
    d.mkdir(parents=True)
    for path, content in ((tmp_path / 'configs' / 'nuscenes' / 'default.yaml', CFG_ROOT), (d / 'default.yaml', TRAIN_DEFAULT),
                          (d / 'spformer.yaml', SPFORMER)):
        path.write_text(yaml.safe_dump(content))
    cfg = builder.Config.load(str(d / 'spformer.yaml'), recursive=True)
    assert 'num_vote' not in cfg.dataset and run_evaluation.num_vote_of(cfg) == 1
    cfg.update(['--dataset.num_vote', '4'])
    assert run_evaluation.num_vote_of(cfg) == 4 and cfg.dataset.voxel_size == 0.05
    cfg.update(['--dataset.num_vote=12'])
    assert run_evaluation.num_vote_of(cfg) == 12
    for bad in (0, 65):
        cfg.update(['--dataset.num_vote', str(bad)])
        with pytest.raises(ValueError, match='num_vote'):
            run_evaluation.num_vote_of(cfg)
    with pytest.raises(SystemExit):
        run_evaluation.main([str(d / 'spformer.yaml')])                    # --weight-path is required


# ------------------------------------------------------------------------------------------------ argument checks
def _args(c=3, n_votes=2, n_scans=1, n_points=4):
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    return dict(logits=torch.zeros(5, c), inverse_map=torch.zeros(n_points * n_scans * n_votes, dtype=torch.int64),
                copy_point_off=i32(n_scans * max(n_votes, 0)), copy_voxel_off=i32(n_scans * max(n_votes, 0)), scan_seg=i32(n_scans + 1),
                n_votes=n_votes, num_points=n_points)


@pytest.mark.parametrize('kw,match', [(dict(c=0), 'classes'), (dict(c=65), 'classes'), (dict(n_votes=0), 'n_votes'),
                                      (dict(n_scans=33, n_votes=2), 'scans x votes'), (dict(n_scans=1, n_votes=65), 'scans x votes')])
def test_shape_rules_raise_value_error(kw, match):
    with pytest.raises(ValueError, match=match):
        vote_point_predictions(**_args(**kw))


def test_other_argument_errors():
    a = _args()
    with pytest.raises(ValueError, match='skip_class'):
        vote_point_predictions(**a, skip_class=3)
    with pytest.raises(ValueError, match='skip_class'):
        vote_point_predictions(**_args(c=1), skip_class=0)
    with pytest.raises(ValueError, match='counts needs targets'):
        vote_point_predictions(**a, counts=torch.zeros(3, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match='targets or num_points'):
        vote_point_predictions(**dict(a, num_points=None))
    with pytest.raises(ValueError, match='copy_point_off'):
        vote_point_predictions(**dict(a, copy_point_off=torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(ValueError, match='int32'):
        vote_point_predictions(**dict(a, scan_seg=torch.zeros(2, dtype=torch.int64)))
    with pytest.raises(ValueError, match='float32, bfloat16 or float16'):
        vote_point_predictions(**dict(a, logits=torch.zeros(5, 3, dtype=torch.float64)))


def test_cpu_tensors_have_no_fallback():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        vote_point_predictions(**_args())
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        vote_point_predictions(**dict(_args(), num_points=None), targets=torch.ones(4, dtype=torch.int64),
                               counts=torch.zeros(3, 3, dtype=torch.int64))


def test_the_entry_is_declared_exported_and_bound():
    from test_cabi_symbols import _declared, test_header_symbols_exported_and_typed
    assert 'u2mkd_vote_points' in _declared() and 'u2mkd_vote_points' in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['u2mkd_vote_points'][1]) == 16
    test_header_symbols_exported_and_typed()
    # the library's own checks come before any launch: they answer without a device
    lib = _lib.load()
    null = [None] * 4
    assert lib.u2mkd_vote_points(None, 0, 0, *null, 1, 1, None, 0, -1, None, None, None, None) == 2
    assert b'1 <= c <= 64' in lib.u2mkd_last_error()
    assert lib.u2mkd_vote_points(None, 0, 65, *null, 1, 1, None, 0, -1, None, None, None, None) == 2
    assert lib.u2mkd_vote_points(None, 0, 17, *null, 1, 0, None, 0, -1, None, None, None, None) == 2
    assert lib.u2mkd_vote_points(None, 0, 17, *null, 33, 2, None, 0, -1, None, None, None, None) == 2
    assert lib.u2mkd_vote_points(None, 3, 17, *null, 1, 1, None, 0, -1, None, None, None, None) == 2
    assert lib.u2mkd_vote_points(None, 0, 17, *null, 1, 1, None, 0, 17, None, None, None, None) == 2
    assert lib.u2mkd_vote_points(None, 0, 17, *null, 0, 1, None, 0, -1, None, None, None, None) == 0      # no scans: nothing to launch
