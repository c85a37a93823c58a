"""KD path (rows a13-a18).  CPU: the batched point<->pixel transfers and the one-gather
teacher->student re-index equal the reference's loops (oracle.fusion_ref); SwiftNet / fusion /
student state-dict keys equal the reference's.  GPU: the whole student + teacher + KD losses on
the HIP operators vs golden vectors made by the reference's own model class."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import fusion_ref as FR
from u2mkd_amd import fusion as PF
from u2mkd_amd.synth import synth_kd_batch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _kd_tensors(b, dev='cpu'):
    s = b['student']
    pc = [torch.from_numpy(c).to(dev) for c in s['pixel_coordinates']]
    ms = [torch.from_numpy(m).to(dev) for m in s['masks']]
    return pc, ms


@pytest.mark.parametrize('idx', [0, 2, 3])
def test_l2c_scatter_equals_reference_loop(idx):
    b = synth_kd_batch(700, 2, seed=3, image_hw=(64, 112))
    pc, ms = _kd_tensors(b)
    ms[1][2] = False                       # a camera that sees nothing -> zero map
    torch.manual_seed(idx)
    feats = torch.randn(sum(m.shape[1] for m in ms), 24, dtype=torch.float64)
    ifh, ifw = (32, 56) if idx == 0 else (8, 14)
    want = FR.l2c_loop(feats, [c.double() for c in pc], ms, ifh, ifw, 4, idx)
    got = PF.l2c_scatter_torch(feats, [c.double() for c in pc], ms, ifh, ifw, 4 - idx)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) < 1e-12
    with pytest.raises(RuntimeError):
        PF.l2c_scatter(feats, [c.double() for c in pc], ms, ifh, ifw, 4 - idx)     # product path: HIP device only


def test_c2l_gather_equals_reference_loop():
    b = synth_kd_batch(700, 2, seed=4, image_hw=(64, 112))
    pc, ms = _kd_tensors(b)
    fmaps = torch.randn(2, 6, 10, 16, 28, dtype=torch.float64)
    want = FR.c2l_loop(fmaps, [c.double() for c in pc], ms)
    got = PF.c2l_gather_torch(fmaps, [c.double() for c in pc], ms)
    assert float((got - want).abs().max()) < 1e-12
    fov = torch.from_numpy(b['student']['fov_mask'])
    assert float(got[~fov].abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize('idx', [0, 2, 3])
def test_hip_l2c_scatter_matches_reference_loop(hip, idx):
    """Segment-sum form of the pixel mean (and its gradient) on the GPU vs the reference loop in fp64."""
    b = synth_kd_batch(700, 2, seed=3, image_hw=(64, 112))
    pc, ms = _kd_tensors(b)
    ms[1][2] = False
    torch.manual_seed(idx)
    n = sum(m.shape[1] for m in ms)
    feats = torch.randn(n, 24, dtype=torch.float64, requires_grad=True)
    ifh, ifw = (32, 56) if idx == 0 else (8, 14)
    want = FR.l2c_loop(feats, [c.double() for c in pc], ms, ifh, ifw, 4, idx)
    g = torch.randn_like(want)
    want.backward(g)
    fd = feats.detach().float().cuda().requires_grad_(True)
    got = PF.l2c_scatter(fd, [c.cuda() for c in pc], [m.cuda() for m in ms], ifh, ifw, 4 - idx)
    assert got.shape == want.shape
    assert float((got.detach().cpu().double() - want.detach()).abs().max()) < 1e-5
    got.backward(g.float().cuda())
    assert float((fd.grad.cpu().double() - feats.grad).abs().max()) < 1e-5
    # deterministic: no atomics anywhere in the map or its gradient
    fd2 = feats.detach().float().cuda().requires_grad_(True)
    got2 = PF.l2c_scatter(fd2, [c.cuda() for c in pc], [m.cuda() for m in ms], ifh, ifw, 4 - idx)
    got2.backward(g.float().cuda())
    assert torch.equal(got, got2) and torch.equal(fd.grad, fd2.grad)


@pytest.mark.gpu
@pytest.mark.parametrize('channels', [12, 17])
def test_hip_c2l_gather_matches_reference_loop(hip, channels):
    b = synth_kd_batch(700, 2, seed=4, image_hw=(64, 112))
    pc, ms = _kd_tensors(b)
    fmaps = torch.randn(2, 6, channels, 16, 28, dtype=torch.float64, requires_grad=True)
    want = FR.c2l_loop(fmaps, [c.double() for c in pc], ms)
    g = torch.randn_like(want)
    want.backward(g)
    fm = fmaps.detach().float().cuda().requires_grad_(True)
    got = PF.c2l_gather(fm, [c.cuda() for c in pc], [m.cuda() for m in ms])
    assert float((got.detach().cpu().double() - want.detach()).abs().max()) < 1e-5
    got.backward(g.float().cuda())
    assert float((fm.grad.cpu().double() - fmaps.grad).abs().max()) < 1e-4
    fov = torch.from_numpy(b['student']['fov_mask'])
    assert float(got[~fov.cuda()].abs().max()) == 0.0


def test_teacher_to_student_equals_reference_loop():
    from u2mkd_amd.kd import teacher_to_student
    b = synth_kd_batch(900, 3, seed=5, image_hw=(32, 56))
    s, t = b['student'], b['teacher']
    x_t = torch.randn(sum(t['num_vox']), 7)
    inv = torch.from_numpy(t['inverse_map'])
    inds = [[torch.from_numpy(i[0])] for i in s['inds']]
    want = FR.t2s_loop(x_t, inv, inds, t['num_pts'], t['num_vox'])
    got = teacher_to_student(x_t, inv, inds, t['num_pts'], t['num_vox'])
    assert torch.equal(got, want)
    kfm = torch.rand(len(inv)) < 0.9
    # with a key-frame mask the student indices address the masked points
    inds2 = []
    cur = 0
    for n_p in t['num_pts']:
        k = int(kfm[cur:cur + n_p].sum())
        inds2.append([torch.randint(0, k, (50,))])
        cur += n_p
    assert torch.equal(teacher_to_student(x_t, inv, inds2, t['num_pts'], t['num_vox'], kfm),
                       FR.t2s_loop(x_t, inv, inds2, t['num_pts'], t['num_vox'], kfm))


def _build(dev, cr=1.0, cr_t=1.0):
    from u2mkd_amd import kd, lidar
    sp = {k: v for k, v in lidar.spformer_kwargs(drop_path_rate=0.0).items() if k not in ('cr', 'in_channel', 'num_classes')}
    return kd.TSDFull(cr=cr, cr_t=cr_t, in_channel=4, in_channel_t=4, num_classes=17, spformer=sp)


def test_kd_state_dict_keys_match_reference():
    with open(os.path.join(G, 'kd_cr10_keys.json')) as f:
        keys = json.load(f)
    sd = _build('cpu').state_dict()
    assert list(sd.keys()) == list(keys.keys())
    assert {k: list(v.shape) for k, v in sd.items()} == keys


# (student cr, teacher cr_t, fixture, voxels per sample): the first fixture, the shipped student / teacher widths
# (configs/nuscenes/train/spformer_tsd_full_ours_star.yaml:32-43: 512-channel teacher convs, 16 heads per attention
# branch) and the `_B` student (spformer_tsd_full_ours_star_B.yaml:34-36)
KD_GOLDENS = [(1.0, 1.0, 'kd_cr10_3000', 1500), (1.0, 2.0, 'kd_cr10_t20_2000', 1000), (2.0, 2.0, 'kd_cr20_t20_2000', 1000)]


@pytest.mark.gpu
def test_edge_scene_meets_the_gate_once_the_angles_come_from_the_cpu_libm(hip, monkeypatch):
    """What a quantiser edge does, kept as a fixture of its own (round 2's first KD fixture, seed 77): SphereFormer
    quantises atan2-derived angles into windows and relative-position bins; the reference (and the golden) computed
    them with the CPU libm, the product with the GPU's, and the two differ in the last place on a few tokens of THIS
    scene that sit within rounding of a bin edge (unpatched: 0.2 % of the rows move by up to 4e-2).  With the spherical
    coordinates taken from the CPU (same fp32 formula, spherical_transformer.py:31-36) -- nothing else changed, every
    kernel of the path still the HIP one -- EVERY row of the student's logits and of the distilled features is within
    1e-3 of the golden and the losses within 1e-3.  The fixtures the gate is stated on (KD_GOLDENS) are scenes without
    such a token (tests/golden/make_golden.py asserts a 4-ulp margin) and are held without patch or allowance."""
    from u2mkd_amd.lidar import sphereformer as SFM
    gpu_fn = SFM.cart2sphere
    monkeypatch.setattr(SFM, 'cart2sphere', lambda xyz: gpu_fn(xyz.detach().cpu()).to(xyz.device))
    _kd_golden_check(1.0, 1.0, 'kd_cr10_3000_edge_seed77', 1500)


@pytest.mark.gpu
@pytest.mark.parametrize('cr,cr_t,fixture,n_vox', KD_GOLDENS)
def test_hip_kd_step_matches_reference_golden(hip, cr, cr_t, fixture, n_vox):
    _kd_golden_check(cr, cr_t, fixture, n_vox)


@pytest.mark.gpu
def test_loader_fed_kd_step_matches_the_reference_golden(hip, tmp_path):
    """Row f1 end to end: the batch comes from the nuScenes loader (u2mkd_amd/data/nuscenes_lc.py on the synthetic tree of
    tests/nusc_tree.py -- validation split: no augmentation, so the scene is the one the fixture was generated on), goes
    through collate_fn / collated_to_kd_batch into the HIP KD model, and every output the other KD fixtures check
    (student / teacher logits, distilled features, stage losses, the five loss terms, four parameter gradients) is held
    to the same 1e-3 against the reference's own model class fed with the same loader batch
    (tests/golden/make_golden.py kd_loader; the tree seed was chosen on the CPU by the +-4 ulp criterion alone)."""
    from nusc_tree import build_tree
    from u2mkd_amd.data import nuscenes_lc as D

    def batch_of(tree_seed):
        root, ver = build_tree(str(tmp_path / ('tree%d' % tree_seed)), seed=tree_seed)
        ds = D.LCNuScenesDataset(D.NuScenesTables(root, ver), split='val', im_cr=0.08)
        return D.collated_to_kd_batch(D.collate_fn([ds[0], ds[1]]))
    # gradients: 5e-3 on this fixture (the sweep files carry raw 0..255 intensities as a LiDAR feature, as nuScenes does:
    # activations ~1e2-1e3; the four sampled gradients measure 5e-4 .. 2e-3 on MI355X; the well-scaled fixtures above hold 1e-3)
    _kd_golden_check(0.5, 0.5, 'kd_loader_cr05', None, batch_of, pix_row_rel=1e-5, grad_gate=5e-3)


def _load_golden(fixture):
    """A fixture with its continuation files (``<fixture>.1.npz`` ...: make_golden.save_golden) as one mapping."""
    gold, i = {}, 0
    while os.path.exists(os.path.join(G, fixture + ('.%d.npz' % i if i else '.npz'))):
        with np.load(os.path.join(G, fixture + ('.%d.npz' % i if i else '.npz'))) as f:
            gold.update(f)
        i += 1
    assert gold, fixture
    return gold


def _kd_golden_check(cr, cr_t, fixture, n_vox, batch_of=None, pix_row_rel=0.0, grad_gate=1e-3):
    from oracle.spvcnn_ref import fill_state_by_name
    from u2mkd_amd import kd, torchsparse as ts
    gold = _load_golden(fixture)
    model = fill_state_by_name(_build('cuda', cr, cr_t)).cuda().train()
    model.model_t.eval()
    model.model_s.dropout.p = 0.0
    seed = int(gold['seed']) if 'seed' in gold else 77
    b = synth_kd_batch(n_vox, 2, seed=seed, image_hw=(64, 112)) if batch_of is None else batch_of(seed)
    s, t = b['student'], b['teacher']
    pc, ms = _kd_tensors(b, 'cuda')
    stu = {'lidar': ts.SparseTensor(torch.from_numpy(s['feats']).cuda(), torch.from_numpy(s['coords']).cuda()),
           'images': torch.from_numpy(s['images']).permute(0, 1, 4, 2, 3).contiguous().cuda(),
           'pixel_coordinates': pc, 'masks': ms, 'fov_mask': torch.from_numpy(s['fov_mask']).cuda()}
    tea = {'lidar': ts.SparseTensor(torch.from_numpy(t['feats']).cuda(), torch.from_numpy(t['coords']).cuda())}
    out = model({'student': stu, 'teacher': tea})
    crit = kd.KDCriterion(ignore_index=0, w_kl=1.0, w_feat=1.0)
    inds = [[torch.from_numpy(i[0]).cuda()] for i in s['inds']]
    ld = kd.kd_losses(out, torch.from_numpy(s['targets']).cuda(), stu['fov_mask'],
                      torch.from_numpy(t['inverse_map']).cuda(), inds, t['num_pts'], t['num_vox'], crit)
    ld['total'].backward()

    def err(a, key):
        return float((a.detach().cpu() - torch.from_numpy(gold[key])).abs().max())

    def rows_off(a, key):
        e = (a.detach().cpu() - torch.from_numpy(gold[key])).abs()
        return float((e.max(1)[0] > 1e-3).float().mean()), float(e.median()), float(e.max())
    assert err(out['t']['x_vox'], 'x_vox_t') < 1e-3
    # (pix_row_rel: the pixel head's logits are 128-term sums of features that reach ~1e3 on un-normalised 0..255 images -- the
    # logits themselves reach 1.1e3 -- and a row's small logits are what is left after cancellation; a fixture may state its
    # bound as 1e-3 + rel * the largest logit of the fixture = fp32 rounding at the scale of the terms.  The loader-fed fixture
    # needs it (raw intensities 0..255 as a LiDAR feature, smooth resized images): its stage losses, which read the same
    # camera maps at the same points, agree to 2e-6 relative, the voxel logits to 4e-4.)
    e_pix = (out['stu']['x_pix'].detach().cpu() - torch.from_numpy(gold['x_pix'])).abs()
    bound = 1e-3 + pix_row_rel * float(np.abs(gold['x_pix']).max())
    print('KD-PARITY', fixture, 'x_pix: median %.2e max %.2e; max of err / row-max %.2e; rows above 1e-3: %.4f'
          % (float(e_pix.median()), float(e_pix.max()), float((e_pix / torch.from_numpy(gold['x_pix']).abs().max(1, keepdim=True)[0].clamp(min=1)).max()),
             float((e_pix.max(1)[0] > 1e-3).float().mean())))
    pix_ok = bool((e_pix <= bound).all()) and float(e_pix.median()) < 1e-4
    # North-star gate: every row within 1e-3, no exception on any fixture
    for a, key in ((out['stu']['x_vox'], 'x_vox'), (out['stu']['pts_feats'][0][::16], 'pts_feats_s')):
        frac, med, mx = rows_off(a, key)
        print('KD-PARITY', fixture, key, 'rows above 1e-3: %.5f' % frac, 'median %.2e' % med, 'max %.2e' % mx)
        assert mx < 1e-3, (key, frac, med, mx)
    mse = torch.stack([m.detach() for m in out['stu']['mse_loss']]).cpu().numpy()
    print('KD-PARITY', fixture, 'stage mse', mse, gold['mse'])
    assert pix_ok, float((e_pix - bound).max())
    assert np.abs(mse - gold['mse']).max() < 1e-3
    got = np.array([float(ld[k].detach()) for k in ('ce_vox', 'ce_pix', 'kl', 'feat', 'total')])
    assert np.abs(got - gold['losses']).max() < 1e-3, (got, gold['losses'])
    g = dict(model.named_parameters())
    for name, key, sl in (('model_s.l2c_fusion_blocks.1.conv1.weight', 'grad_l2c', slice(None)),
                          ('model_s.c2l_fusion_blocks.2.conv1.weight', 'grad_c2l', slice(None)),
                          ('model_s.pix_branch.layer2.0.conv1.weight', 'grad_layer2', slice(0, 8)),
                          ('model_s.stem.3.kernel', 'grad_stem', slice(None))):
        a, bb = g[name].grad.cpu().double()[sl], torch.from_numpy(gold[key]).double()
        # parameter gradients within 1e-3 (L2-relative) of the reference class's (measured on MI355X:
        # 2e-5 .. 3.5e-4 over the three fixtures)
        rel = float((a - bb).norm() / bb.norm())
        print('KD-GRAD', fixture, name, '%.3e' % rel)
        assert rel < grad_gate, (name, rel)
    assert all(p.grad is None for p in model.model_t.parameters())
