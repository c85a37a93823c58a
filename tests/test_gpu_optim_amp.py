"""optim.FusedSGD driven by a GradScaler (fp16 autocast, the reference's amp mode): unscale, non-finite check and the decision
to skip a step on the device (csrc/optim.hip: u2mkd_grads_unscale_check, u2mkd_sgd_batch_amp), against
``torch.optim.SGD(foreach=True)`` driven by ``torch.amp.GradScaler('cuda')`` in the ordinary way -- EXACT after every step of a
script with non-finite steps (the first one included), parameters whose first gradient arrives late (in a finite and in a
non-finite step), a scale that grows and backs off, power-of-two and inexact scales.

Routes: (a) ``u2mkd_amd.optim.GradScaler`` -- ``.grad`` after ``step`` is what torch's SGD leaves, unscaled, on skipped steps
too; (b) a plain ``torch.amp.GradScaler`` -- the step kernel unscales, and on a SKIPPED step the gradients stay scaled, as
with torch's fused optimizers (asserted here).  Each with and without an explicit ``scaler.unscale_(opt)`` before ``step``."""
import os
import subprocess
import sys
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KWS = [dict(momentum=0.9, weight_decay=1e-4, nesterov=True), dict(momentum=0.9, weight_decay=0.0, nesterov=False),
       dict(momentum=0.0, weight_decay=5e-4), dict(momentum=0.5, weight_decay=1e-2, nesterov=True)]      # tests/test_gpu_optim.py's
SCALERS = [dict(), dict(init_scale=3000.0, growth_factor=1.7)]      # power-of-two scales | 1 / scale inexact
INF, NAN = float('inf'), float('nan')
I_ONE, I_TAIL, I_TWO, I_MIS, I_LATE_OK, I_LATE_BAD = 1, 3, 5, 6, 7, 8
# step -> (parameter, flat index or None = the last element, value); the FIRST step is not finite
BAD = {0: (0, 17, INF), 3: (I_TAIL, None, -INF), 6: (I_MIS, 100, NAN), 9: (I_TWO, None, NAN)}
STEPS = 10


def _chunk():
    from u2mkd_amd import _lib
    return int(_lib.load().u2mkd_sgd_chunk_elements())


def _shapes():
    c = _chunk()
    return [(27, 64, 64), (1,), (3,), (c + 1,), (17, 96), (2 * c + 5,), (5, 7, 3, 3), (12289,), (64,), (2, 4096)]


def _params(seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(*s, generator=g) * 10 ** float(torch.randint(-3, 3, (1,), generator=g))).cuda())
            for s in _shapes()]


def _skipped_grad(k, i):
    """I_LATE_OK has no gradient until step 5 (finite), I_LATE_BAD none until step 6 (not finite); (3,) none in step 8."""
    return (i == I_LATE_OK and k < 5) or (i == I_LATE_BAD and k < 6) or (i == 2 and k == 8)


def _assign_grads(ps, k, scale, bad=BAD):
    """The scripted gradients of step k times ``scale``, as fp32 tensors; I_MIS's is a 4-byte offset into a larger buffer (the
    scalar path of the kernels)."""
    g = torch.Generator().manual_seed(1000 + k)
    for i, p in enumerate(ps):
        v = torch.randn(p.numel() + 1, generator=g) * 0.3
        if _skipped_grad(k, i):
            p.grad = None
            continue
        v = v.cuda() * scale
        v = v[1:] if i == I_MIS else v[:-1].clone()
        if k in bad and bad[k][0] == i:
            v[v.numel() - 1 if bad[k][1] is None else bad[k][1]] = bad[k][2]
        p.grad = v.view_as(p)
        assert (p.grad.data_ptr() % 16 != 0) == (i == I_MIS)


def _bits(t):
    return None if t is None else t.detach().clone().view(torch.int32)      # (bit patterns: a NaN equals itself)


def _run(opt_cls, scaler_cls, kw, scaler_kw, explicit=False, clip=False, steps=STEPS):
    ps = _params()
    opt = opt_cls(ps, lr=0.24, **kw) if opt_cls is not torch.optim.SGD else opt_cls(ps, lr=0.24, foreach=True, **kw)
    scaler = scaler_cls('cuda', growth_interval=2, **scaler_kw)
    trace = []
    for k in range(steps):
        scale = float(scaler.scale(torch.ones((), device='cuda')))
        _assign_grads(ps, k, scale)
        assigned = [_bits(p.grad) for p in ps]
        if explicit or clip:
            scaler.unscale_(opt)
        if clip:
            torch.nn.utils.clip_grad_norm_(ps, 1.0)
        scaler.step(opt)
        scaler.update()
        trace.append(dict(params=[_bits(p) for p in ps], grads=[_bits(p.grad) for p in ps], assigned=assigned,
                          bufs=[_bits(opt.state[p]['momentum_buffer']) if 'momentum_buffer' in opt.state.get(p, {}) else None for p in ps],
                          scale=scaler.get_scale(), tracker=scaler._get_growth_tracker()))
    return trace, opt, scaler


_REF = {}


def _reference(ki, si, explicit, clip=False):
    """torch.optim.SGD(foreach=True) under torch.amp.GradScaler: computed once per setting, shared, never modified."""
    key = (ki, si, explicit, clip)
    if key not in _REF:
        _REF[key] = _run(torch.optim.SGD, torch.amp.GradScaler, KWS[ki], SCALERS[si], explicit, clip)[0]
    return _REF[key]


def _same(x, y):
    return (x is None and y is None) or (x is not None and y is not None and torch.equal(x, y))


def _compare(want, got, route, explicit):
    for k, (w, g) in enumerate(zip(want, got)):
        assert (w['scale'], w['tracker']) == (g['scale'], g['tracker']), (k, w['scale'], g['scale'])
        for key in ('params', 'bufs'):      # (bufs: the same parameters have a momentum_buffer -- none after the skipped first step)
            for i, (x, y) in enumerate(zip(w[key], g[key])):
                assert _same(x, y), (k, key, i)
        if k not in BAD or explicit or route == 'own':
            for i, (x, y) in enumerate(zip(w['grads'], g['grads'])):
                assert _same(x, y), (k, 'grads', i)
        else:      # a skipped step through a plain torch.amp.GradScaler: nothing was written, the gradients are still scaled
            for i, (x, y) in enumerate(zip(g['assigned'], g['grads'])):
                assert _same(x, y), (k, 'grads stay scaled', i)
            assert not _same(w['grads'][0], g['grads'][0])


def _scaler_cls(route):
    from u2mkd_amd import optim
    return optim.GradScaler if route == 'own' else torch.amp.GradScaler


def test_the_script_does_what_it_says(hip):
    """The reference's own trace: which steps are skipped, when buffers appear, the scale growing and backing off."""
    want = _reference(0, 0, False)
    assert all(b is None for b in want[0]['bufs']), 'a skipped first step leaves no state'
    have = [[b is not None for b in t['bufs']] for t in want]
    assert have[1].count(True) == 8 and not have[4][I_LATE_OK] and have[5][I_LATE_OK]
    assert not have[6][I_LATE_BAD] and have[7][I_LATE_BAD]
    scales = [t['scale'] for t in want]
    assert scales[0] < 65536.0 and scales[2] > scales[1] and scales[3] < scales[2] and scales[5] > scales[4], scales
    for k in range(1, STEPS):
        moved = not _same(want[k]['params'][0], want[k - 1]['params'][0])
        assert moved == (k not in BAD), k


@pytest.mark.parametrize('si', range(len(SCALERS)), ids=['pow2', 'inexact'])
@pytest.mark.parametrize('ki', range(len(KWS)))
@pytest.mark.parametrize('explicit', [False, True], ids=['step', 'unscale_then_step'])
@pytest.mark.parametrize('route', ['own', 'torch'])
def test_fused_sgd_under_a_grad_scaler_equals_torch_sgd_exactly(hip, route, explicit, ki, si):
    """On a skipped step through route 'torch' (b) without an explicit unscale_ the gradients stay scaled, as with torch's
    fused optimizers; everywhere else ``.grad`` equals the reference's."""
    from u2mkd_amd.optim import FusedSGD
    got, opt, _ = _run(FusedSGD, _scaler_cls(route), KWS[ki], SCALERS[si], explicit)
    assert opt._fused_groups, 'the fused path did not run'
    _compare(_reference(ki, si, explicit), got, route, explicit)


@pytest.mark.parametrize('si', range(len(SCALERS)), ids=['pow2', 'inexact'])
@pytest.mark.parametrize('route', ['own', 'torch'])
def test_unscale_then_clip_then_step(hip, route, si):
    from u2mkd_amd.optim import FusedSGD
    got, opt, _ = _run(FusedSGD, _scaler_cls(route), KWS[0], SCALERS[si], clip=True)
    assert opt._fused_groups
    _compare(_reference(0, si, True, clip=True), got, route, True)


def _sync_debug_mode_works():
    """Does torch.cuda.set_sync_debug_mode('warn') report a host read on this build?"""
    t = torch.ones(1, device='cuda')
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            t.item()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    return any('synchroniz' in str(w.message) for w in seen)


HOST_READS = ('item', 'tolist', 'cpu', '__bool__')


@pytest.mark.parametrize('route', ['own', 'torch'])
def test_no_host_read_in_steady_state(hip, route):
    """Once every parameter has its momentum buffer, ``scaler.step(opt); scaler.update()`` reads nothing back: zero calls of
    Tensor.item / tolist / cpu / __bool__ over three consecutive steps, the middle one not finite (and skipped: the parameters
    do not move).  Where ``torch.cuda.set_sync_debug_mode('warn')`` reports a host read on this build (probed first with an
    ``.item()``; the outcome is printed), no synchronising call is reported within those steps either; where it does not,
    the wrapper count stands alone."""
    from u2mkd_amd.optim import FusedSGD
    ps = _params()
    opt = FusedSGD(ps, lr=0.24, **KWS[0])
    scaler = _scaler_cls(route)('cuda', growth_interval=2)
    snaps, calls, reported = [], [], []
    sync_mode = _sync_debug_mode_works()
    print('set_sync_debug_mode reports host reads on this build:', sync_mode)
    # three finite steps (step 7's gradients: every parameter has one), then the three that are watched
    for k, bad in enumerate([None, None, None, None, (I_TWO, None, INF), None]):
        scale = float(scaler.scale(torch.ones((), device='cuda')))
        _assign_grads(ps, 7, scale, bad={7: bad} if bad else {})
        torch.cuda.synchronize()
        if k < 3:
            scaler.step(opt)
            scaler.update()
            continue
        assert all('momentum_buffer' in opt.state[p] for p in ps)
        with pytest.MonkeyPatch.context() as mp, warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            for name in HOST_READS:
                real = getattr(torch.Tensor, name)
                mp.setattr(torch.Tensor, name, lambda self, *a, _real=real, _name=name, **kw: (calls.append(_name), _real(self, *a, **kw))[1])
            if sync_mode:
                torch.cuda.set_sync_debug_mode('warn')
            try:
                scaler.step(opt)
                scaler.update()
            finally:
                torch.cuda.set_sync_debug_mode('default')
        reported += [str(w.message) for w in seen if 'synchroniz' in str(w.message)]
        snaps.append(ps[0].detach().clone())
    assert calls == [], calls
    assert reported == [], reported
    assert torch.equal(snaps[0], snaps[1]) and not torch.equal(snaps[1], snaps[2])      # (skipped on the device | applied)


def _table(ps, grads, chunk):
    rows, first = [], 0
    for p, g in zip(ps, grads):
        rows.append([p.data_ptr(), 0 if g is None else g.data_ptr(), 0, p.numel(), first, 1])
        first += (p.numel() + chunk - 1) // chunk
    return torch.tensor(rows, dtype=torch.int64).cuda(), first


def test_grads_unscale_check_kernel(hip):
    """u2mkd_grads_unscale_check through _lib against torch._amp_foreach_non_finite_check_and_unscale_ on clones: a table of
    one 1-element tensor, a null-gradient job between two others, found_inf pre-set, inverse scale 1 (no store)."""
    L = hip
    chunk = _chunk()
    gen = torch.Generator().manual_seed(5)

    def launch(ps, grads, inv, found):
        tab, total = _table(ps, grads, chunk)
        L.call('u2mkd_grads_unscale_check', L.ptr(tab), len(ps), total, L.ptr(inv), L.ptr(found), L.stream())
        torch.cuda.synchronize()

    def torch_says(grads, inv, found_before):
        clones = [g.clone() for g in grads if g is not None]
        found = torch.full((), found_before, device='cuda')
        torch._amp_foreach_non_finite_check_and_unscale_(clones, found, inv)
        return clones, float(found)

    # one 1-element tensor: finite, then inf
    for value, want_found in ((0.75, 0.0), (INF, 1.0)):
        p, g = torch.zeros(1, device='cuda'), torch.full((1,), value, device='cuda')
        inv, found = torch.full((), 1.0 / 3000.0, device='cuda'), torch.zeros((), device='cuda')
        want, wf = torch_says([g], inv, 0.0)
        launch([p], [g], inv, found)
        assert float(found) == want_found == wf and torch.equal(_bits(g), _bits(want[0]))
    # a null-gradient job between two others (the second spans three chunks, from a misaligned address); found_inf 1 stays 1
    sizes = [chunk + 1, 77, 2 * chunk + 5]
    ps = [torch.zeros(n, device='cuda') for n in sizes]
    big = torch.randn(sizes[2] + 1, generator=gen).cuda() * 100
    grads = [torch.randn(sizes[0], generator=gen).cuda() * 100, None, big[1:]]
    for inv_value, pre, plant in ((1.0 / 3000.0, 0.0, None), (0.25, 1.0, None), (1.0 / 3000.0, 0.0, NAN), (0.5, 0.0, -INF)):
        gs = [None if g is None else g.clone() for g in grads]
        gs[2] = big.clone()[1:]
        if plant is not None:      # NaN: the single element of the first tensor's tail chunk; -inf: the end of the misaligned one
            gs[0 if plant != plant else 2][-1] = plant
        inv, found = torch.full((), inv_value, device='cuda'), torch.full((), pre, device='cuda')
        want, wf = torch_says(gs, inv, pre)
        launch(ps, gs, inv, found)
        assert float(found) == wf == (1.0 if (pre or plant is not None) else 0.0), (inv_value, pre, plant)
        for a, b in zip([g for g in gs if g is not None], want):
            assert torch.equal(_bits(a), _bits(b))
    # inverse scale 1: check only -- the buffer keeps its bits (NaN payloads included), the NaN is found
    g = torch.randn(chunk + 3, generator=gen).cuda()
    g.view(torch.int32)[5] = 0x7fc12345
    g.view(torch.int32)[chunk + 2] = 0x7f812345      # (a signalling NaN: any arithmetic on it would set its quiet bit)
    before = _bits(g)
    found = torch.zeros((), device='cuda')
    launch([torch.zeros_like(g)], [g], torch.ones((), device='cuda'), found)
    assert float(found) == 1.0 and torch.equal(_bits(g), before)
    g = torch.randn(chunk + 3, generator=gen).cuda()
    before, found = _bits(g), torch.zeros((), device='cuda')
    launch([torch.zeros_like(g)], [g], torch.ones((), device='cuda'), found)
    assert float(found) == 0.0 and torch.equal(_bits(g), before)


CHILD = '''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import test_gpu_optim_amp as T
params, run, applied = T._lidar_steps(plain=True)
assert type(run.opt) is torch.optim.SGD and type(run.amp.scaler) is torch.amp.GradScaler and applied >= 1, applied
torch.save([p.detach().cpu() for p in params], sys.argv[1])
print("ok")
'''


def _lidar_steps(plain=False):
    """Three LidarStep(amp='fp16') steps on the scene of tests/test_gpu_f16_rows.py's trainer test.  ``plain``: with torch's own
    optimizer and scaler in the trainer -- ``torch.optim.SGD`` at the shipped settings (train.make_optimizer's) behind
    ``torch.amp.GradScaler``, whose ``_maybe_opt_step`` reads found_inf on the host: none of this package's optimizer code."""
    from u2mkd_amd import lidar, train
    from u2mkd_amd.synth import synth_batch
    b = synth_batch(3000, 1, 9)
    feats, coords, labels = (torch.from_numpy(b[k]).cuda() for k in ('feats', 'coords', 'labels'))
    torch.manual_seed(0)
    model = lidar.SPVCNN(cr=0.5, in_channel=4, num_classes=17, pres=0.05, vres=0.05).cuda().train()
    if plain:
        run = train.LidarStep(model, amp='fp16', optimizer=lambda net: torch.optim.SGD(
            [p for p in net.parameters() if p.requires_grad], lr=0.24, momentum=0.9, weight_decay=1.0e-4, nesterov=True))
        run.amp.scaler = torch.amp.GradScaler('cuda')
    else:
        run = train.LidarStep(model, amp='fp16')
    applied, before = 0, [p.detach().clone() for p in model.parameters()]
    for _ in range(3):
        run(feats, coords, labels)
        now = [p.detach().clone() for p in model.parameters()]
        applied += any(not torch.equal(a, b_) for a, b_ in zip(before, now))
        before = now
    print('LidarStep fp16: %d of 3 steps applied, scale %g' % (applied, run.amp.scaler.get_scale()))
    return [p.detach() for p in model.parameters()], run, applied


def test_lidar_step_fp16_equals_torchs_step_and_scaler_route(hip, tmp_path):
    """Three LidarStep(amp='fp16') steps: the scaler is this package's, at least one step is applied (a run of skipped steps
    would compare untouched parameters), and the parameters equal those of the same run on torch's route -- a fresh process with
    U2MKD_FUSED_SGD=0 (read at import) whose trainer holds a plain ``torch.optim.SGD`` and a plain ``torch.amp.GradScaler``, so
    that nothing of the code under test is in the reference.  It hands its parameters back in a file."""
    from u2mkd_amd import optim
    params, run, applied = _lidar_steps()
    assert type(run.amp.scaler) is optim.GradScaler and run.opt._fused_groups
    assert applied >= 1, applied
    out = str(tmp_path / 'params.pt')
    r = subprocess.run([sys.executable, '-c', CHILD % (ROOT, os.path.join(ROOT, 'tests')), out],
                       env=dict(os.environ, U2MKD_FUSED_SGD='0'), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    want = torch.load(out)
    assert len(want) == len(params)
    for i, (a, b) in enumerate(zip(want, params)):
        assert torch.equal(a, b.cpu()), (i, float((a - b.cpu()).abs().max()))


def test_a_step_in_which_no_parameter_has_a_gradient(hip):
    """torch's scaler then hands over ``found_inf = sum([])``, the int 0: no check ran, and the step neither raises nor writes."""
    from u2mkd_amd.optim import FusedSGD
    for route in ('own', 'torch'):
        ps = _params()
        before = [p.detach().clone() for p in ps]
        opt = FusedSGD(ps, lr=0.24, **KWS[0])
        scaler = _scaler_cls(route)('cuda')
        scaler.scale(torch.ones((), device='cuda'))
        scaler.step(opt)
        assert not opt.state and all(torch.equal(a, b) for a, b in zip(before, ps))
