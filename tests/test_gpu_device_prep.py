"""The loader's geometry on the GPU (u2mkd_amd/data/device_prep.py, csrc/prep.hip) against its numpy specification
(tests/device_prep_ref.py) BIT FOR BIT: every tensor of the batch, floats compared as integers (a NaN only where the
specification has one too), host lists included.  The kernels' arithmetic rule (one IEEE operation per written operation,
nothing contracted) is what makes that possible; a tensor that misses it points at a contracted or reordered operation."""
import warnings

import numpy as np
import pytest
import torch

import device_prep_ref as R
from nusc_tree import build_tree
from test_device_prep_host import SETTINGS, dataset
from u2mkd_amd.data import nuscenes_lc as D
from u2mkd_amd.synth import synth_raw_sample

pytestmark = pytest.mark.gpu

HOST_READS = ('item', 'tolist', 'cpu', '__bool__')


@pytest.fixture(scope='module')
def tables(tmp_path_factory):
    root, ver = build_tree(str(tmp_path_factory.mktemp('nusc')))
    return D.NuScenesTables(root, ver)


def spec_batch(raws):
    """The specification's batch as ``kd_batch_to_device`` lays it out (CPU tensors), and the per-sample results."""
    from u2mkd_amd import train as T
    samples = [R.prepare_numpy(r) for r in raws]
    return T.kd_batch_to_device(R.collate(samples), device='cpu'), samples


def same_bits(got, want, path):
    assert torch.is_tensor(got) and got.is_cuda and got.is_contiguous(), path
    g = got.cpu()
    assert g.dtype == want.dtype and g.shape == want.shape, (path, g.dtype, want.dtype, tuple(g.shape), tuple(want.shape))
    if want.dtype.is_floating_point:
        assert want.dtype == torch.float32, path
        ok = (g.view(torch.int32) == want.view(torch.int32)) | (torch.isnan(g) & torch.isnan(want))
        assert bool(ok.all()), '%s: %d of %d elements differ in bits' % (path, int((~ok).sum()), ok.numel())
    else:
        assert torch.equal(g, want), path


def compare(got, want, path=''):
    if isinstance(want, dict):
        assert set(got) == set(want), (path, sorted(got), sorted(want))
        for k in want:
            compare(got[k], want[k], path + '/' + k)
    elif isinstance(want, (list, tuple)):
        assert isinstance(got, (list, tuple)) and len(got) == len(want), path
        for i, (g, w) in enumerate(zip(got, want)):
            compare(g, w, '%s[%d]' % (path, i))
    elif torch.is_tensor(want):
        same_bits(got, want, path)
    else:
        assert type(got) is type(want) and got == want, (path, got, want)      # host lists of ints, None


def check(raws):
    from u2mkd_amd.data import device_prep
    want, samples = spec_batch(raws)
    got, ev = device_prep.prepare_kd_batch(raws, with_eval=True)
    torch.cuda.synchronize()
    compare(got, want)
    compare(ev, {k: torch.from_numpy(v) for k, v in R.eval_feed(samples).items()}, '/eval')
    # the teacher-only trainer's batch: the teacher half of the same specification
    lid = device_prep.prepare_lidar_batch(raws)
    names = {'feats': 't_feats', 'coords': 't_coords', 'targets': 'targets_t', 'keyframe_mask_full': 'keyframe_mask_full',
             'inverse_map': 'inverse_map', 'num_pts': 'num_pts', 'num_vox': 'num_vox_t'}
    compare({k: lid[k] for k in names}, {k: want[v] for k, v in names.items()}, '/lidar')
    compare(lid['keyframe_mask'], want.get('keyframe_mask'), '/lidar/keyframe_mask')
    compare(lid['inverse_batch'], torch.from_numpy(R.eval_feed(samples)['t_inverse_batch']), '/lidar/inverse_batch')
    compare(lid['targets_mapped'], torch.from_numpy(R.eval_feed(samples)['targets_mapped_t']), '/lidar/targets_mapped')
    return got, want, samples


# ------------------------------------------------------------------------------------------------ the on-disk tree
@pytest.mark.parametrize('batch', [1, 2])
@pytest.mark.parametrize('multisweeps,im_drop', sorted(SETTINGS))
def test_tree_samples(hip, tables, multisweeps, im_drop, batch):
    ds = dataset(tables, multisweeps, im_drop, SETTINGS[(multisweeps, im_drop)])
    raws = D.raw_collate_fn([ds.raw(i) for i in range(batch)])
    got, want, samples = check(raws)
    assert got['num_pts'] == [s['teacher']['num_pts'] for s in samples] and ('keyframe_mask' in got) == bool(multisweeps)
    assert got['images'].shape == (batch, 6 - im_drop, 3, 36, 64) and got['masks'][0].shape[0] == 6 - im_drop


def test_eval_split(hip, tables):
    ds = D.LCNuScenesDataset(tables, voxel_size=0.05, split='val', im_cr=0.04, multisweeps=1)
    check([ds.raw(0), ds.raw(1)])


# ------------------------------------------------------------------------------------------------ synthetic raws
def _close(raw, which):
    """Make the sweep points `which` (bool over all sweep points) "close": |x| < 1 and |y| < 1."""
    p = raw['sweeps']['points']
    p[which, :2] = (p[which, :2] / 41.0).astype(np.float32)
    return raw


def test_sweep_sizes_around_the_wave_and_workgroup_sizes(hip):
    sizes = [0, 1, 63, 64, 65, 257, 1025]
    a = synth_raw_sample(300, sizes, seed=1)
    b = synth_raw_sample(129, sizes[::-1], seed=2)
    got, want, samples = check([a, b])
    assert samples[0]['teacher']['num_pts'] > 300 + 1400
    check([a])


def test_a_sweep_that_is_empty_after_the_filter(hip):
    raw = synth_raw_sample(200, [70, 300, 65], seed=3)
    seg = raw['sweeps']['seg']
    which = np.zeros(seg[-1], bool)
    which[seg[1]:seg[2]] = True
    _close(raw, which)
    spec = R.prepare_numpy(raw)
    assert spec['teacher']['num_pts'] <= 200 + 70 + 65
    check([raw])
    every = _close(synth_raw_sample(50, [64, 1], seed=4), np.ones(65, bool))          # nothing survives at all
    assert R.prepare_numpy(every)['teacher']['num_pts'] == 50
    check([every, raw])


def test_alternate_points_close_compaction_crosses_every_boundary(hip):
    raw = synth_raw_sample(100, [2500, 2101], seed=5)          # (more than two scan blocks of 2048)
    which = np.arange(4601) % 2 == 0
    _close(raw, which)
    n = R.prepare_numpy(raw)['teacher']['num_pts']
    assert 100 + 2260 <= n <= 100 + 2300
    check([raw])
    check([synth_raw_sample(64, [65], seed=6), raw])


def test_no_sweeps_with_a_multisweep_teacher(hip):
    raw = synth_raw_sample(150, [], seed=7)
    assert raw['multisweeps'] != 0 and raw['sweeps']['tm'].shape == (0, 4, 4)
    got, want, _ = check([raw])
    assert bool(got['keyframe_mask_full'].all()) and got['num_pts'] == [150]


def _voxel_case(kind, n=600, seed=8):
    raw = synth_raw_sample(n, [40], seed=seed, train=kind != 'one')
    rng = np.random.default_rng(seed)
    p = raw['points']
    if kind == 'one':                        # every point in one voxel: the first point wins everything
        p[:, :3] = np.float32([10.0, 5.0, 1.0]) + rng.uniform(-0.004, 0.004, (n, 3)).astype(np.float32)
    elif kind == 'distinct':                 # a 1 m lattice: as many voxels as points
        i = np.arange(n)
        p[:, 0], p[:, 1], p[:, 2] = (i % 25) - 12.0, (i // 25) - 12.0 + 20.0, 1.0
    else:                                    # the second half repeats the first, far away in the input
        p[n // 2:, :3] = p[:n // 2, :3]
    raw['labels'] = (np.arange(n) % 16 + 1).astype(np.int64)          # duplicates carry different labels and intensities
    p[:, 3] = np.arange(n, dtype=np.float32)
    return raw


@pytest.mark.parametrize('kind', ['one', 'distinct', 'far'])
def test_voxel_sets_first_point_wins(hip, kind):
    raw = _voxel_case(kind)
    got, want, samples = check([raw])
    nv = got['s_coords'].shape[0]
    assert {'one': nv == 1, 'distinct': nv == 600, 'far': 290 <= nv <= 300}[kind], nv
    if kind == 'one':
        assert got['inds'][0][0].tolist() == [0] and float(got['s_feats'][0, 3]) == 0.0 and int(got['targets'][0]) == 1
    if kind == 'far':
        assert int(got['inds'][0][0].max()) < 300                       # never the later copy


def test_one_point(hip):
    raw = synth_raw_sample(1, None, seed=9)
    raw['points'][0, :3] = [3.0, 20.0, 0.5]
    got, _, _ = check([raw])
    assert got['s_coords'].tolist() == [[0, 0, 0, 0]] and got['num_pts'] == [1]
    check([synth_raw_sample(1, [1], seed=10)])


def test_cameras_that_see_nothing_and_a_single_camera(hip):
    near = synth_raw_sample(120, None, seed=11, cams=(0, 3))
    near['points'][:, :3] *= np.float32(0.01)                           # everything within half a metre: no depth above 1 m
    got, _, _ = check([near])
    assert not bool(got['masks'][0].any()) and not bool(got['fov_mask'].any())
    half = synth_raw_sample(400, None, seed=12, cams=(1, 4))            # points ahead only: the back camera sees none
    half['points'][:, 1] = np.abs(half['points'][:, 1]) + np.float32(6.0)
    half['points'][:, 0] *= np.float32(0.2)
    got, _, _ = check([half])
    assert bool(got['masks'][0][0].any()) and not bool(got['masks'][0][1].any())
    one = synth_raw_sample(400, [30], seed=13, cams=(2,))               # five of six cameras dropped
    got, _, _ = check([one, synth_raw_sample(77, [5], seed=14, cams=(5,))])
    assert got['images'].shape[:2] == (2, 1) and got['masks'][1].shape[0] == 1


# ------------------------------------------------------------------------------------------------ exact decisions
def _pinhole(fx, fy, tz=0.0):
    eye, zero = np.eye(3), np.zeros(3)
    return {'channel': 0, 'steps': [(eye, zero), (eye, zero), (eye, zero), (eye, np.array([0.0, 0.0, tz]))],
            'K': np.array([[fx, 0.0, 512.0], [0.0, fy, 256.0], [0.0, 0.0, 1.0]]), 'size': (1025, 513)}


def test_decisions_exactly_on_the_boundary_and_one_step_inside(hip):
    """Identity rotations, zero translations, K = (512, 512; 512, 256), image 1025 x 513: every value below is exact.
    Camera 0: depth == 1, u == -1, u == +1, v == -1, v == +1 -> excluded (strict comparisons).  Camera 1 (focal lengths
    512 - 2^-43): the same four image points land one representable step inside +-1 -> included.  Camera 2 (translated by
    -2^-52 along z): depth 1 + 2^-52 -> included."""
    raw = synth_raw_sample(7, None, seed=15)
    raw['points'][:, :3] = np.float32([[0, 0, 1], [2, 0, 2], [-2, 0, 2], [0, 1, 2], [0, -1, 2], [0, 0, 2], [0, 0, 0.5]])
    f = 512.0 - 2.0 ** -43
    raw['cams'] = [_pinhole(512.0, 512.0), _pinhole(f, f), _pinhole(512.0, 512.0, tz=-2.0 ** -52)]
    raw['images'] = raw['images'][:3]
    for c, cam in enumerate(raw['cams']):
        uv, mask, _ = R._project(raw['points'], cam)
        if c == 0:
            assert uv[1:5].tolist() == [[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]]
            assert mask.tolist() == [False, False, False, False, False, True, False]
        if c == 1:
            e = 2.0 ** -52
            assert uv[1:5].tolist() == [[1.0 - e, 0.0], [-1.0 + e, 0.0], [0.0, 1.0 - e], [0.0, -1.0 + e]]
            assert mask.tolist() == [False, True, True, True, True, True, False]
        if c == 2:
            assert mask.tolist() == [True, False, False, False, False, True, False]
    raw['student'] = {'rot': np.eye(3), 'scale': 1.0}                   # (the student's voxels: one per point, in input order)
    got, want, samples = check([raw])
    inds = samples[0]['student']['inds']
    full = torch.zeros(3, 7, dtype=torch.bool)
    full[:, inds] = got['masks'][0].cpu()
    assert full.tolist() == [[False, False, False, False, False, True, False], [False, True, True, True, True, True, False],
                             [True, False, False, False, False, True, False]]


def _float32_ties():
    """float32 coordinates v with float32(v / float32(0.05)) == k + 0.5 exactly, one for an even and one for an odd k."""
    vs, found = np.float32(0.05), {}
    for k in range(8, 400):
        v = np.float32((k + 0.5) * 0.05)
        for _ in range(8):
            v = np.nextafter(v, np.float32(-np.inf))
        for _ in range(17):
            if np.float32(v / vs) == np.float32(k + 0.5) and k % 2 not in found:
                found[k % 2] = (k, v)
            v = np.nextafter(v, np.float32(np.inf))
        if len(found) == 2:
            return found
    raise AssertionError('no float32 tie found')


def test_float32_ties_round_half_to_even(hip):
    ties = _float32_ties()
    (ke, ve), (ko, vo) = ties[0], ties[1]
    raw = synth_raw_sample(5, None, seed=16, train=False)               # eval mode: the coordinates reach the division as they are
    raw['points'][:, :3] = np.float32([[0, 0, 0], [ve, 0, 0], [vo, 0, 0], [0, ve, vo], [0, 0, 0]])
    raw['points'][4, :3] = np.float32([-ve, -vo, 0])
    got, want, samples = check([raw])
    vox = np.round(raw['points'][:, :3] / np.float32(0.05)).astype(np.int64)
    assert vox[1, 0] == ke and vox[2, 0] == ko + 1 and vox[4].tolist() == [-ke, -(ko + 1), 0]      # half to even, both ways
    coords = got['s_coords'].cpu().numpy()[:, :3] + vox.min(0)
    assert set(map(tuple, coords.tolist())) == set(map(tuple, vox.tolist()))
    assert torch.equal(got['s_coords'], got['t_coords'])                 # the float32 teacher (no sweeps) takes the same path


def test_a_span_beyond_the_key_raises_and_the_next_call_succeeds(hip):
    from u2mkd_amd.data import device_prep
    raw = synth_raw_sample(40, [10], seed=17)
    raw['points'][0, 2], raw['points'][1, 2] = 0.0, 4000.0                # 80 000 voxels along z: beyond 2^16
    with pytest.raises(ValueError, match='sort key'):
        device_prep.prepare_kd_batch([raw])
    with pytest.raises(ValueError, match='sort key'):
        device_prep.prepare_lidar_batch([raw])
    check([synth_raw_sample(40, [10], seed=17)])                          # the flag does not outlive the call


def test_three_runs_are_identical(hip):
    from u2mkd_amd.data import device_prep
    raws = [synth_raw_sample(3000, [900, 1100], seed=18), synth_raw_sample(2500, [1300], seed=19)]
    runs = [device_prep.prepare_kd_batch(raws) for _ in range(3)]
    torch.cuda.synchronize()

    def equal(a, b):
        if torch.is_tensor(a):
            return torch.equal(a, b)
        if isinstance(a, (list, tuple)):
            return len(a) == len(b) and all(equal(x, y) for x, y in zip(a, b))
        return a == b
    for other in runs[1:]:
        assert set(other) == set(runs[0]) and all(equal(runs[0][k], other[k]) for k in runs[0])


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


def test_one_host_read_per_call(hip, monkeypatch):
    """The sizes of a batch come back in one read: one ``wait_counts`` (the mailbox poll) or, with the mailbox switched off or
    more than 32 values, the one ``tolist`` it falls back to -- and nothing else (Tensor.item / tolist / cpu / __bool__, and no
    synchronising call where ``set_sync_debug_mode('warn')`` reports them on this build)."""
    from u2mkd_amd.data import device_prep
    from u2mkd_amd.torchsparse.nn import functional as spf
    raws = [synth_raw_sample(500, [200, 100], seed=20), synth_raw_sample(400, [50], seed=21)]
    device_prep.prepare_kd_batch(raws)                                    # (library, mailbox and allocator warmed up)
    torch.cuda.synchronize()
    sync_mode = _sync_debug_mode_works()
    print('set_sync_debug_mode reports host reads on this build:', sync_mode)
    calls, waits = [], []
    real_wait = spf.wait_counts
    monkeypatch.setattr(spf, 'wait_counts', lambda h, *a: (waits.append(h.seq), real_wait(h, *a))[1])
    with pytest.MonkeyPatch.context() as mp, warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        for name in HOST_READS:
            real = getattr(torch.Tensor, name)
            mp.setattr(torch.Tensor, name, lambda self, *a, _real=real, _name=name, **kw: (calls.append(_name), _real(self, *a, **kw))[1])
        if sync_mode:
            torch.cuda.set_sync_debug_mode('warn')
        try:
            out = device_prep.prepare_kd_batch(raws)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    reported = [str(w.message) for w in seen if 'synchroniz' in str(w.message)]
    print('wait_counts:', waits, 'tensor reads:', calls, 'reported:', reported)
    assert len(waits) == 1
    mailbox = waits[0] is not None
    assert calls == ([] if mailbox else ['tolist'])
    assert reported == [] if mailbox else len(reported) <= 1
    compare(out, spec_batch(raws)[0])


# ------------------------------------------------------------------------------------------------ end to end
def _to_cpu(v):
    if torch.is_tensor(v):
        return v.cpu()
    if isinstance(v, dict):
        return {k: _to_cpu(x) for k, x in v.items()}
    if isinstance(v, list) and v and not isinstance(v[0], int):
        return [_to_cpu(x) for x in v]
    return v


def test_a_kd_step_on_the_device_batch_equals_one_on_the_loader_batch(hip, tables):
    from u2mkd_amd import kd as KD, lidar, train as T
    from u2mkd_amd.data import device_prep
    seed = SETTINGS[(1, 3)]
    mk = lambda: D.LCNuScenesDataset(tables, voxel_size=0.05, split='train', im_cr=0.08, im_drop=3, flip=True, multisweeps=1,
                                     only_past=False, rng=np.random.default_rng(seed))
    a, b = mk(), mk()
    dev_batch = device_prep.prepare_kd_batch([a.raw(0), a.raw(1)])
    ref_batch = T.kd_batch_to_device(D.collated_to_kd_batch(D.collate_fn([b[0], b[1]])))
    compare(dev_batch, _to_cpu(ref_batch))
    losses = []
    sp = {k: v for k, v in lidar.spformer_kwargs().items() if k not in ('cr', 'in_channel', 'num_classes')}
    # One step of a freshly built, seeded model is not a pure function of the batch from the start of a process (NOTES N30.3):
    # with MIOpen's default choices two steps on the SAME loader batch differ in the fourth digit, and even with its
    # deterministic ones the first three models built at a new set of shapes give 14.8089, 14.8182, 14.8168 on this very
    # loader batch (whatever ran before; further steps of ONE model do not settle it), every later one 14.8162947 -- loader
    # and device batch alike.  So: deterministic choices, four throw-away models on the loader batch, then the comparison,
    # which is exact.
    def runner():
        torch.manual_seed(0)
        model = KD.TSDFull(cr=0.5, cr_t=0.5, in_channel=4, in_channel_t=4, num_classes=17, spformer=sp).cuda()
        run = T.KDStep(model, num_epochs=50, batch_size=2)
        run.train_mode()
        return run
    was, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    try:
        settle = [float(runner()(T.fresh_batch(ref_batch))) for _ in range(4)]
        for batch in (dev_batch, ref_batch):
            # (the device batch as prepare_kd_batch returned it: views of its buffers; the loader batch a fresh copy)
            losses.append(runner()(batch if batch is dev_batch else T.fresh_batch(batch)).clone())
    finally:
        torch.backends.cudnn.deterministic = was
    print('settling steps:', settle, 'losses (device batch, loader batch):', [float(x) for x in losses])
    assert bool(torch.isfinite(losses[0])) and torch.equal(losses[0], losses[1])
