"""State across the training loop's phases: evaluate -> train -> evaluate, as run_training.py does every epoch.

The library writes parameters, momentum buffers and BatchNorm running statistics in place through raw pointers
(optim.FusedSGD, the BatchNorm kernels), and caches values derived from them (the folded eval-mode BatchNorm affine of
functional.eval_bn_affine, the weight re-layouts of functional._weight_layout) under the tensors' in-place versions.
These tests hold the rule that makes those caches sound -- whatever the library writes in place, it bumps the version
of, as torch's own in-place operations do -- from the whole trainers down to each writer, against float64 formulas of
the tensors as they are at that moment and against the CPU oracle."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import spformer_ref as R, spvcnn_ref as O, torchsparse_cpu as ots
from u2mkd_amd.synth import synth_batch, synth_eval_feed, synth_kd_batch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
LR = 0.02


def _fold_spy(monkeypatch):
    """conv_eval_affine wrapped: the list receives True per Conv3d -> BatchNorm pair that ran folded."""
    from u2mkd_amd.lidar import blocks
    calls = []
    orig = blocks.spf.conv_eval_affine

    def spy(*a, **k):
        out = orig(*a, **k)
        calls.append(out is not None)
        return out
    monkeypatch.setattr(blocks.spf, 'conv_eval_affine', spy)
    return calls


def _unfolded(fn):
    """fn() with the eval-mode BatchNorm fold off (its two-pass form: the BatchNorm reads the running statistics itself)."""
    from u2mkd_amd.lidar import blocks
    blocks._FOLD_EVAL_BN = False
    try:
        return fn()
    finally:
        blocks._FOLD_EVAL_BN = True


def _bn_state(model):
    """(affine, running statistics) of every BatchNorm, flattened, on the host."""
    bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.running_mean is not None]
    aff = torch.cat([torch.cat([m.weight.detach().flatten(), m.bias.detach().flatten()]) for m in bns]).double().cpu()
    stats = torch.cat([torch.cat([m.running_mean.flatten(), m.running_var.flatten()]) for m in bns]).double().cpu()
    return aff, stats


def _rel_change(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _constant_lr(opt):
    return torch.optim.lr_scheduler.LambdaLR(opt, lambda k: 1.0)


def _teacher(monkeypatch_env=None):
    """SPVCNN_SPFORMER (cr 1.0, no drop-path) with the oracle's deterministic fill, its LidarStep with the default
    optimizer (FusedSGD) at a small learning rate, and the oracle model."""
    from u2mkd_amd import lidar, optim, train as T
    ref = O.fill_state_by_name(R.SPVCNN_SPFORMER(**R.default_spformer_kwargs(cr=1.0, drop_path_rate=0.0))).eval()
    model = lidar.SPVCNN_SPFORMER(**lidar.spformer_kwargs(cr=1.0, drop_path_rate=0.0))
    model.load_state_dict(ref.state_dict())
    model.cuda()
    run = T.LidarStep(model, optimizer=lambda net: T.make_optimizer([p for p in net.parameters() if p.requires_grad], lr=LR),
                      scheduler=_constant_lr)
    assert type(run.opt) is optim.FusedSGD
    return run, model, ref


def _teacher_scene():
    """The multi-sweep golden's scene (seed known to sit off the quantiser edges), identity point -> voxel feed."""
    seed = int(np.load(os.path.join(G, 'teacher_multisweep_cr10_6000.npz'))['seed'])
    b = synth_batch(3000, 2, seed=seed, sweeps=3)
    feats, coords = torch.from_numpy(b['feats']), torch.from_numpy(b['coords'])
    vb = coords[:, -1].long()
    inv = torch.cat([torch.arange(int((vb == i).sum())) for i in range(2)])
    labels = torch.from_numpy(b['labels']).long()
    return feats, coords, inv, vb, labels


def _teacher_evaluate(run, model, scene):
    from u2mkd_amd import torchsparse as ts
    feats, coords, inv, vb, labels = (t.cuda() for t in scene)
    model.eval()
    ret = run.evaluate(feats, coords, inv, vb, labels)
    assert ret['outputs_vox'].shape == labels.shape
    with torch.no_grad():
        return model({'lidar': ts.SparseTensor(feats, coords)})['x_vox']


def _logits_tol(x):
    return 2e-5 * max(1.0, float(x.abs().max()))


def test_teacher_trainer_evaluate_train_evaluate(hip, monkeypatch):
    """LidarStep: evaluate, three FusedSGD training steps, evaluate again.  The second evaluation with the folded
    eval BatchNorm equals the two-pass form and the CPU oracle built from the model's current state."""
    from u2mkd_amd import torchsparse as ts
    run, model, ref = _teacher()
    scene = _teacher_scene()
    first = _teacher_evaluate(run, model, scene)
    aff0, stats0 = _bn_state(model)
    feats, coords, _, _, labels = (t.cuda() for t in scene)
    model.train()
    losses = [float(run(feats, coords, labels)) for _ in range(3)]
    assert all(np.isfinite(losses)), losses
    calls = _fold_spy(monkeypatch)
    folded = _teacher_evaluate(run, model, scene)
    n_folded = sum(calls)
    aff1, stats1 = _bn_state(model)
    with torch.no_grad():
        plain = _unfolded(lambda: model({'lidar': ts.SparseTensor(feats, coords)})['x_vox'])
    # guards: the fold ran, the training moved both halves of the folded affine, and the logits with it
    assert n_folded >= 30, (n_folded, len(calls))
    assert _rel_change(aff1, aff0) > 1e-3 and _rel_change(stats1, stats0) > 1e-3, (_rel_change(aff1, aff0), _rel_change(stats1, stats0))
    tol = _logits_tol(plain)
    moved = float((folded - first).abs().max())
    assert moved > 100 * tol, (moved, tol)
    err = float((folded - plain).abs().max())
    print('STATE-COHERENCE teacher: %d pairs folded, folded vs two-pass %.2e (tol %.2e), logits moved %.2e' % (n_folded, err, tol, moved))
    assert err < tol, (err, tol)
    ref.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    with torch.no_grad():
        want = ref.eval()({'lidar': ots.SparseTensor(scene[0], scene[1])})['x_vox']
    err_ref = float((folded.cpu() - want).abs().max())
    print('STATE-COHERENCE teacher vs oracle max abs err %.2e (range %.1f)' % (err_ref, float(want.abs().max())))
    assert err_ref < 1e-3 * max(1.0, float(want.abs().max()))


def test_batchnorm_recalibration_between_evaluations(hip, monkeypatch):
    """evaluate -> train-mode forwards under no_grad (no optimizer step: only the BatchNorm kernels' running-statistics
    writes change the model) -> evaluate: the folded form equals the two-pass form on the recalibrated statistics."""
    from u2mkd_amd import torchsparse as ts
    run, model, _ = _teacher()
    scene = _teacher_scene()
    feats, coords = scene[0].cuda(), scene[1].cuda()
    first = _teacher_evaluate(run, model, scene)
    aff0, stats0 = _bn_state(model)
    model.train()
    with torch.no_grad():
        for _ in range(2):
            model({'lidar': ts.SparseTensor(feats, coords)})
    calls = _fold_spy(monkeypatch)
    folded = _teacher_evaluate(run, model, scene)
    aff1, stats1 = _bn_state(model)
    with torch.no_grad():
        plain = _unfolded(lambda: model({'lidar': ts.SparseTensor(feats, coords)})['x_vox'])
    assert sum(calls) >= 30, (sum(calls), len(calls))
    assert torch.equal(aff1, aff0) and _rel_change(stats1, stats0) > 1e-3
    tol = _logits_tol(plain)
    assert float((folded - first).abs().max()) > 100 * tol
    err = float((folded - plain).abs().max())
    print('STATE-COHERENCE recalibrated statistics: folded vs two-pass %.2e (tol %.2e)' % (err, tol))
    assert err < tol, (err, tol)


def test_kd_trainer_evaluate_train_evaluate(hip, monkeypatch):
    """KDStep (cr 1.0 / 1.0): evaluate, two KD steps, evaluate again.  The student's folded logits equal its two-pass
    logits; the frozen teacher's logits are bit-identical across the two evaluations."""
    from u2mkd_amd import kd, lidar, optim, train as T
    seed = int(np.load(os.path.join(G, 'kd_eval_cr10_3000.npz'))['seed'])
    b = synth_kd_batch(1500, 2, seed=seed, image_hw=(64, 112))
    b['student']['images'] = ((b['student']['images'] / 255.0 - 0.45) / 0.225).astype(np.float32)
    f = {k: torch.from_numpy(v).cuda() for k, v in synth_eval_feed(b, seed).items()}
    sp = {k: v for k, v in lidar.spformer_kwargs(drop_path_rate=0.0).items() if k not in ('cr', 'in_channel', 'num_classes')}
    model = O.fill_state_by_name(kd.TSDFull(cr=1.0, cr_t=1.0, in_channel=4, in_channel_t=4, num_classes=17, spformer=sp,
                                            debug_val=True), conv2d_he=True).cuda()
    run = T.KDStep(model, optimizer=lambda net: T.make_optimizer([p for p in net.parameters() if p.requires_grad], lr=LR),
                   scheduler=_constant_lr)
    assert type(run.opt) is optim.FusedSGD
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if hasattr(m, 'drop_prob'):
            m.drop_prob = 0.0
    d = T.kd_batch_to_device(b)

    def evaluate():
        model.eval()
        run.evaluate(d, f['s_inverse_map'], f['s_inverse_batch'], f['targets_mapped'], f['label_fov'],
                     f['t_inverse_batch'], f['targets_mapped_t'])
        with torch.no_grad():
            out = model(run._in_mod(d))
        return out['stu']['x_vox'], out['t']['x_vox']
    s0, t0 = evaluate()
    aff0, stats0 = _bn_state(model.model_s)
    run.train_mode()
    losses = [float(run(d)) for _ in range(2)]
    assert all(np.isfinite(losses)), losses
    calls = _fold_spy(monkeypatch)
    s1, t1 = evaluate()
    n_folded = sum(calls)
    aff1, stats1 = _bn_state(model.model_s)
    with torch.no_grad():
        plain = _unfolded(lambda: model(run._in_mod(d))['stu']['x_vox'])
    assert n_folded >= 30, (n_folded, len(calls))
    assert _rel_change(aff1, aff0) > 1e-3 and _rel_change(stats1, stats0) > 1e-3
    tol = _logits_tol(plain)
    assert float((s1 - s0).abs().max()) > 100 * tol
    err = float((s1 - plain).abs().max())
    print('STATE-COHERENCE KD student: folded vs two-pass %.2e (tol %.2e)' % (err, tol))
    assert err < tol, (err, tol)
    assert torch.equal(t1, t0)


# ------------------------------------------------------------------------------------------------ per writer
def _bn(c=96, seed=0):
    torch.manual_seed(seed)
    bn = torch.nn.BatchNorm1d(c).cuda()
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.5)
        bn.running_var.uniform_(0.5, 2.0)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.3)
    return bn


def _affine_f64(bn):
    rm, rv = bn.running_mean.double(), bn.running_var.double()
    scale = bn.weight.detach().double() / torch.sqrt(rv + bn.eps)
    return scale, bn.bias.detach().double() - rm * scale


def _write_fused_sgd(bn, F, monkeypatch):
    from u2mkd_amd.optim import FusedSGD
    opt = FusedSGD([bn.weight, bn.bias], lr=LR, momentum=0.9, weight_decay=1e-4, nesterov=True)
    for _ in range(2):
        bn.weight.grad = torch.randn_like(bn.weight)
        bn.bias.grad = torch.randn_like(bn.bias)
        opt.step()


def _write_train(bn, F, x, **kw):
    bn.train()
    F.batch_norm(x, bn, **kw)
    bn.eval()


def _write_host(bn, F, monkeypatch):
    assert F.host_ops() is not None            # (the C++ host path is the one under test)
    _write_train(bn, F, torch.randn(3000, 96, device='cuda') * 2 + 1, relu=True)


def _write_python(bn, F, monkeypatch):
    monkeypatch.setattr(F, '_HOST', None)
    _write_train(bn, F, torch.randn(3000, 96, device='cuda') * 2 + 1, relu=True)


def _write_residual(bn, F, monkeypatch):
    x = torch.randn(3000, 96, device='cuda') * 2 + 1
    _write_train(bn, F, x, relu=True, residual=torch.randn_like(x))


def _write_momentum_none(bn, F, monkeypatch):
    bn.momentum = None
    _write_train(bn, F, torch.randn(3000, 96, device='cuda') * 2 + 1, relu=False)


def _write_bf16(bn, F, monkeypatch):
    with torch.autocast('cuda', dtype=torch.bfloat16):
        assert F.bf16_rows()
        _write_train(bn, F, (torch.randn(3000, 96, device='cuda') * 2 + 1).bfloat16(), relu=True)


def _write_data(bn, F, monkeypatch):
    bn.running_var.data.mul_(1.5)
    bn.running_mean.data.add_(0.25)
    bn.weight.data.mul_(0.8)
    bn.bias.data.sub_(0.1)
    F.invalidate_weight_caches()


WRITERS = {'fused_sgd': _write_fused_sgd, 'host': _write_host, 'python': _write_python, 'residual': _write_residual,
           'momentum_none': _write_momentum_none, 'bf16_rows': _write_bf16, 'data_then_invalidate': _write_data}


@pytest.mark.parametrize('writer', list(WRITERS))
def test_eval_bn_affine_follows_every_writer(hip, monkeypatch, writer):
    """eval_bn_affine (cached on the module) after each kind of in-place write equals w / sqrt(rv + eps) and
    b - rm * scale in float64 of the tensors as they are now."""
    from u2mkd_amd.torchsparse.nn import functional as F
    bn = _bn().eval()
    s0, b0 = (t.clone() for t in F.eval_bn_affine(bn))
    WRITERS[writer](bn, F, monkeypatch)
    want_s, want_b = _affine_f64(bn)
    assert _rel_change(want_s.cpu(), s0.double().cpu()) > 1e-3 or _rel_change(want_b.cpu(), b0.double().cpu()) > 1e-3
    scale, shift = F.eval_bn_affine(bn)
    es = float((scale.double() - want_s).abs().max() / want_s.abs().max())
    eb = float((shift.double() - want_b).abs().max() / want_b.abs().max())
    assert es < 2e-7 and eb < 2e-7, (writer, es, eb)


@pytest.mark.parametrize('kind', ['tiles', 'pairs', 'linear'])
def test_frozen_weight_rewritten_through_data_then_invalidated(hip, kind):
    """A frozen weight (the KD teacher, an EMA copy) rewritten through .data keeps its storage and version; after
    invalidate_weight_caches() its layer equals a twin that holds the new values in a fresh tensor."""
    import u2mkd_amd.torchsparse.nn as spnn
    from u2mkd_amd import torchsparse as ts
    from u2mkd_amd.torchsparse.nn import functional as F
    torch.manual_seed(11)
    if kind == 'linear':
        c = 64
        layer = torch.nn.Linear(c, 96).cuda().requires_grad_(False)
        x = torch.randn(2000, c, device='cuda')

        def run(m):
            return F.linear(x, m.weight, m.bias)
    else:
        c = 32 if kind == 'tiles' else 128
        assert F._pairs_mode(c, c) == (kind == 'pairs')
        layer = spnn.Conv3d(c, c, 3).cuda().requires_grad_(False)
        b = synth_batch(3000, 2, seed=7)
        coords = torch.from_numpy(b['coords']).cuda()
        x = torch.randn(len(coords), c, device='cuda')

        def run(m):
            return m(ts.SparseTensor(x, coords)).F
    with torch.no_grad():
        old = run(layer)
        run(layer)                                   # (the cached layout is the one in use)
        w = [p for n, p in layer.named_parameters() if 'bias' not in n][0]
        new_w = torch.randn_like(w) * w.abs().mean()
        w.data.copy_(new_w)
        F.invalidate_weight_caches()
        got = run(layer)
        twin = copy.deepcopy(layer)
        tw = [p for n, p in twin.named_parameters() if 'bias' not in n][0]
        tw.data = new_w.clone()
        want = run(twin)
    assert not torch.equal(want, old)
    assert torch.equal(got, want), float((got - want).abs().max())


def _versions(ts_):
    return [t._version for t in ts_]


def test_fused_sgd_bumps_versions_as_torch_sgd_does(hip):
    """After a FusedSGD step, every parameter torch's SGD bumps is bumped and no other, every momentum buffer torch's
    SGD bumps is bumped; a backward through a tensor saved before the step raises under both optimizers."""
    from u2mkd_amd.optim import FusedSGD
    torch.manual_seed(4)
    a = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Linear(16, 4), torch.nn.Linear(4, 4)).cuda()
    b = copy.deepcopy(a)
    kw = dict(lr=LR, momentum=0.9, weight_decay=1e-4, nesterov=True)
    nets = ((a, FusedSGD(a.parameters(), **kw)), (b, torch.optim.SGD(b.parameters(), **kw)))
    x = torch.randn(32, 8, device='cuda')
    for step in range(3):
        saved = []
        for net, opt in nets:
            opt.zero_grad()
            loss = net[1](net[0](x)).square().mean()     # net[2] receives no gradient
            loss.backward(retain_graph=True)
            saved.append(loss)
        before = []
        for net, opt in nets:
            ps = list(net.parameters())
            bufs = [opt.state.get(p, {}).get('momentum_buffer') for p in ps]
            before.append((_versions(ps), [None if t is None else t._version for t in bufs]))
            opt.step()
        (pa0, ba0), (pb0, bb0) = before
        pa1, pb1 = _versions(a.parameters()), _versions(b.parameters())
        bumped_a = [v1 > v0 for v0, v1 in zip(pa0, pa1)]
        bumped_b = [v1 > v0 for v0, v1 in zip(pb0, pb1)]
        assert bumped_a == bumped_b, (step, bumped_a, bumped_b)
        assert bumped_b == [True] * 4 + [False] * 2
        for i, (pa, pb) in enumerate(zip(a.parameters(), b.parameters())):
            buf_b = nets[1][1].state.get(pb, {}).get('momentum_buffer')
            if bb0[i] is not None and buf_b._version > bb0[i]:
                assert nets[0][1].state[pa]['momentum_buffer']._version > ba0[i], (step, i)
        for loss in saved:
            with pytest.raises(RuntimeError, match='modified by an inplace operation'):
                loss.backward()


def test_forward_after_fused_sgd_step_uses_the_batched_fragment_refresh(hip, monkeypatch):
    """The version bumps come before the optimizer's post hook re-stamps the fragment images: the forward after a
    FusedSGD step issues the one batched refresh launch and no per-weight re-layout (as with torch.optim.SGD)."""
    from u2mkd_amd import _lib as L, torchsparse
    from u2mkd_amd.optim import FusedSGD
    import u2mkd_amd.torchsparse.nn as spnn
    b = synth_batch(4000, 1, seed=5)
    coords = torch.from_numpy(b['coords']).cuda()
    torch.manual_seed(2)
    net = torch.nn.ModuleList([spnn.Conv3d(32, 64, 3), spnn.Conv3d(64, 64, 3), spnn.Conv3d(64, 32, 3)]).cuda()
    x0 = torchsparse.SparseTensor(torch.randn(len(coords), 32, device='cuda'), coords)
    opt = FusedSGD(net.parameters(), lr=LR, momentum=0.9)
    calls = []
    real = L.call

    def counting(name, *a):
        if name.startswith('u2mkd_weight_fragments'):
            calls.append(name)
        return real(name, *a)
    monkeypatch.setattr(L, 'call', counting)

    def step():
        y = x0
        for m in net:
            y = m(y)
        opt.zero_grad()
        (y.F ** 2).mean().backward()
        v = [p._version for p in net.parameters()]
        opt.step()
        assert all(p._version > v0 for p, v0 in zip(net.parameters(), v))
    step()
    assert calls.count('u2mkd_weight_fragments') == 3 and calls.count('u2mkd_weight_fragments_batch') == 1
    del calls[:]
    step()
    assert calls == ['u2mkd_weight_fragments_batch'], calls
