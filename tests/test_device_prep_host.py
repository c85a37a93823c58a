"""The device loader path, host side (no GPU): raw samples (`LCNuScenesDataset.raw`), the numpy specification of the
kernels (tests/device_prep_ref.py) against the loader itself, the rng order, worker safety and the entry points."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import device_prep_ref as R
from nusc_tree import build_tree
from u2mkd_amd import _lib
from u2mkd_amd.data import nuscenes_lc as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (multisweeps, im_drop) -> augmentation seed of the fixture: seeds at which no point of either sample sits within 1e-9
# (relative) of a voxel, depth or image-border decision -- found by running the margin check below over seeds 0, 1, 2, ...
# (float32 points tie exactly at k + .5 about once in 10 000 coordinates, so most seeds fail it: the first that pass)
SETTINGS = {(0, 0): 6, (0, 3): 6, (1, 0): 1, (1, 3): 0}
IM_CR = 0.04               # 36 x 64 images


@pytest.fixture(scope='module')
def tables(tmp_path_factory):
    root, ver = build_tree(str(tmp_path_factory.mktemp('nusc')))
    return D.NuScenesTables(root, ver)


def dataset(tables, multisweeps, im_drop, seed, **kw):
    return D.LCNuScenesDataset(tables, voxel_size=0.05, split='train', im_cr=IM_CR, im_drop=im_drop, flip=True,
                               multisweeps=multisweeps, only_past=False, rng=np.random.default_rng(seed), **kw)


def _ulps(a, b):
    """Distance in float32 ulps (NaN == NaN, equal infinities 0, anything else non-finite: huge)."""
    a, b = a.astype(np.float32).reshape(-1), b.astype(np.float32).reshape(-1)
    same = (np.isnan(a) & np.isnan(b)) | (a == b)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    d = np.abs(ia - ib)
    d[~(np.isfinite(a) & np.isfinite(b))] = 1 << 40
    d[same] = 0
    return d


def _bits_differ(a, b):
    a, b = a.astype(np.float32).reshape(-1), b.astype(np.float32).reshape(-1)
    return int(((a.view(np.int32) != b.view(np.int32)) & ~(np.isnan(a) & np.isnan(b))).sum())


def _compare(got, want, path=''):
    if isinstance(want, dict):
        assert set(got) == set(want), (path, sorted(got), sorted(want))
        for k in want:
            _compare(got[k], want[k], path + '/' + k)
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), path
        for i, (g, w) in enumerate(zip(got, want)):
            _compare(g, w, '%s[%d]' % (path, i))
    elif isinstance(want, np.ndarray):
        assert got.dtype == want.dtype and got.shape == want.shape, (path, got.dtype, want.dtype, got.shape, want.shape)
        if want.dtype.kind == 'f':
            worst, differ = int(_ulps(got, want).max(initial=0)), _bits_differ(got, want)
            print('%s: %d elements, worst %d ulp, %d not bit-identical' % (path, want.size, worst, differ))
            assert worst <= 1, (path, worst)
            assert differ <= 8, (path, differ)
        else:
            assert np.array_equal(got, want), path
    else:
        assert got == want, (path, got, want)


@pytest.mark.parametrize('multisweeps,im_drop', sorted(SETTINGS))
def test_specification_against_the_loader(tables, multisweeps, im_drop):
    seed = SETTINGS[(multisweeps, im_drop)]
    a, b = dataset(tables, multisweeps, im_drop, seed), dataset(tables, multisweeps, im_drop, seed)
    for i in (0, 1):
        raw = a.raw(i)
        spec = R.prepare_numpy(raw)
        assert spec['margin'] >= 1e-9, ('sample %d of setting %r has a point %.3g (relative) from a decision: change its seed in '
                                        'SETTINGS' % (i, (multisweeps, im_drop), spec['margin']))
        item = b[i]
        assert raw['lidar_token'] == item['lidar_token']
        _compare(R.collate([spec]), D.collated_to_kd_batch(D.collate_fn([item])))
        assert raw['images'].dtype == np.uint8 and raw['images'].shape == (6 - im_drop, 36, 64, 3)
        assert raw['points'].dtype == np.float32 and raw['labels'].dtype == np.int64
        assert len(raw['cams']) == 6 - im_drop and all(len(c['steps']) == 4 for c in raw['cams'])
        if multisweeps:
            sw = raw['sweeps']
            assert sw['points'].dtype == np.float32 and sw['seg'].dtype == np.int32 and sw['tm'].dtype == np.float64
            assert sw['tm'].shape == (2, 4, 4) and sw['lag'].shape == (2,) and sw['seg'][-1] == sw['points'].shape[0] == 3000
            assert (sw['lag'] != 0).all()
        else:
            assert raw['sweeps'] is None


def test_batch_of_two_collates_like_the_loader(tables):
    a, b = dataset(tables, 1, 3, SETTINGS[(1, 3)]), dataset(tables, 1, 3, SETTINGS[(1, 3)])
    raws = D.raw_collate_fn([a.raw(0), a.raw(1)])
    assert isinstance(raws, list) and len(raws) == 2 and raws[0]['points'].dtype == np.float32
    _compare(R.collate([R.prepare_numpy(r) for r in raws]), D.collated_to_kd_batch(D.collate_fn([b[0], b[1]])))


def test_eval_split_is_not_rotated(tables):
    a = D.LCNuScenesDataset(tables, voxel_size=0.05, split='val', im_cr=IM_CR, multisweeps=1)
    raw = a.raw(1)
    assert not raw['train'] and len(raw['cams']) == 6 and np.array_equal(raw['teacher']['rot'], np.eye(3)) and raw['teacher']['flip'] == 0
    _compare(R.collate([R.prepare_numpy(raw)]), D.collated_to_kd_batch(D.collate_fn([a[1]])))


@pytest.mark.parametrize('multisweeps,im_drop', sorted(SETTINGS))
def test_raw_consumes_the_generator_in_getitem_order(tables, multisweeps, im_drop):
    a, b = dataset(tables, multisweeps, im_drop, 11), dataset(tables, multisweeps, im_drop, 11)
    for i in (0, 1, 0):
        a.raw(i)
        b[i]
        assert a.rng.bit_generator.state == b.rng.bit_generator.state
    assert a.rng.uniform() == b.rng.uniform()


def test_raw_refuses_debug(tables):
    with pytest.raises(NotImplementedError):
        dataset(tables, 0, 0, 0, debug=True).raw(0)


def test_raw_never_opens_the_device(tables):
    """A loader worker calls raw() and raw_collate_fn(): neither may initialise the GPU runtime."""
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n'
            'import numpy as np, torch\n'
            'from u2mkd_amd.data import nuscenes_lc as D\n'
            'tb = D.NuScenesTables(%r, %r)\n'
            'ds = D.LCNuScenesDataset(tb, split="train", im_cr=0.04, im_drop=3, multisweeps=1, rng=np.random.default_rng(0))\n'
            'batch = D.raw_collate_fn([ds.raw(0), D.RawView(ds)[1]])\n'
            'assert len(batch) == 2 and not torch.cuda.is_initialized()\n'
            'print("clean")\n') % (ROOT, os.path.join(ROOT, 'tests'), tables.dataroot, tables.version)
    p = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and 'clean' in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def test_prepare_on_the_cpu_raises(tables):
    from u2mkd_amd.data import device_prep
    raws = [dataset(tables, 1, 3, 0).raw(0)]
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        device_prep.prepare_kd_batch(raws, device='cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        device_prep.prepare_lidar_batch(raws, device='cpu')


def test_entries_are_declared_and_bound():
    text = open(os.path.join(ROOT, 'include', 'u2mkd_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = _lib.load()
    for name in ('u2mkd_prep_scan_workspace_bytes', 'u2mkd_prep_key_bits', 'u2mkd_prep_sweep_compact', 'u2mkd_prep_points',
                 'u2mkd_prep_project', 'u2mkd_prep_voxel_keys', 'u2mkd_prep_voxel_sets'):
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert [lib.u2mkd_prep_key_bits(a) for a in range(4)] == list(R.KEY_BITS) + [7]
    assert lib.u2mkd_prep_scan_workspace_bytes(5000) == (5000 + 3) * 4


def test_synthetic_raw_samples_follow_the_schema(tables):
    from u2mkd_amd.synth import synth_raw_sample
    real, syn = dataset(tables, 1, 3, 0).raw(0), synth_raw_sample(50, [7, 0, 9], seed=3, cams=(0, 2, 5))
    assert set(real) == set(syn)
    for k in ('points', 'labels', 'images'):
        assert real[k].dtype == syn[k].dtype and real[k].ndim == syn[k].ndim, k
    assert set(real['sweeps']) == set(syn['sweeps']) and set(real['cams'][0]) == set(syn['cams'][0])
    assert R.prepare_numpy(syn)['teacher']['num_pts'] <= 50 + 16
