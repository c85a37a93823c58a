"""run_training.py --device-prep on the on-disk tree: both stages of the pipeline (the teacher, then the KD student on the
teacher's best checkpoint) with the loaders delivering raw samples and the batch geometry done by csrc/prep.hip."""
import os

import pytest

from test_gpu_run_training import _configs
from test_nuscenes_loader import tree  # noqa: F401  (module-scoped fixture: the on-disk tables, sweeps, images)

pytestmark = pytest.mark.gpu


def test_both_stages_with_device_prep(hip, tmp_path, tree, capsys):  # noqa: F811
    import run_training
    root, ver = tree
    cfgs = _configs(tmp_path, root=root, version=ver, im_cr=0.08)
    cwd = os.getcwd()
    os.chdir(tmp_path)                      # no ./data/nuscenes/*_official.npy here: both splits hold every sample
    try:
        run1 = str(tmp_path / 'teacher')
        h = run_training.main([os.path.join(cfgs, 'spformer.yaml'), '--run-dir', run1, '--non-dist', '--device-prep',
                               '--max-iters', '2', '--optimizer.lr', '0.01', '--debug.debug_val', 'false'])
        assert len(h) == 1 and h[0]['loss'] == h[0]['loss'] and 0.0 <= h[0]['iou/val/vox'] <= 1.0
        best = os.path.join(run1, 'checkpoints', 'max-iou-val-vox.pt')
        assert os.path.isfile(best)
        h = run_training.main([os.path.join(cfgs, 'tsd.yaml'), '--run-dir', str(tmp_path / 'kd'), '--non-dist', '--device-prep',
                               '--max-iters', '2', '--model.in_channel_t', '4', '--model.teacher_pretrain', best,
                               '--optimizer.lr', '0.01', '--debug.debug_val', 'false'])
    finally:
        os.chdir(cwd)
    assert 'weights: teacher_pretrain_weight' in capsys.readouterr().out
    assert len(h) == 1 and h[0]['loss'] == h[0]['loss']
    assert all(0.0 <= h[0][k] <= 1.0 for k in ('iou-vox/val', 'iou-pix/val'))
    assert os.path.isfile(tmp_path / 'kd' / 'checkpoints' / 'step-1.pt') and os.path.isfile(tmp_path / 'kd' / 'history.json')


def test_device_prep_refuses_synthetic_scenes(hip, tmp_path):
    import run_training
    cfgs = _configs(tmp_path, im_cr=0.08)
    with pytest.raises(SystemExit, match='--device-prep'):
        run_training.main([os.path.join(cfgs, 'tsd.yaml'), '--run-dir', str(tmp_path / 'x'), '--non-dist', '--device-prep',
                           '--synthetic', '2000', '--model.in_channel_t', '4'])
