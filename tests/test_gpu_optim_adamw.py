"""optim.FusedAdam / optim.FusedAdamW (csrc/optim.hip: u2mkd_adam_batch, u2mkd_adam_batch_amp -- torch's Adam / AdamW update over all
parameters of a group in one launch) against ``torch.optim.Adam`` / ``torch.optim.AdamW`` on the device, BIT FOR BIT: parameters,
both moments and step counts after every step; each kernel stage against the single ``torch._foreach_*`` call it restates; the
state_dict round trip; the fall-backs; the global step hooks; and under a GradScaler (``torch.amp.GradScaler`` and
``optim.GradScaler``, with and without an explicit ``unscale_``) through a script with skipped steps -- the first one, two in a
row -- where the device alone knows each parameter's step count, also with the outcomes reaching the host as late as the
bookkeeping allows."""
import copy
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(27, 64, 64), (1,), (3,), (4097,), (17, 96), (8192,), (5, 7, 3, 3), (12289,), (64,), (2, 4096)]      # tests/test_gpu_optim.py's
KWS = [dict(weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8), dict(weight_decay=0.0), dict(betas=(0.8, 0.95), eps=1e-6),
       dict(betas=(0.4, 0.999))]      # the last: the lerp's other branch (weight 0.6)
INF, NAN = float('inf'), float('nan')


def _classes(which):
    from u2mkd_amd import optim
    return {'adamw': (optim.FusedAdamW, torch.optim.AdamW), 'adam': (optim.FusedAdam, torch.optim.Adam)}[which]


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(*s, generator=g) * 10 ** float(torch.randint(-3, 3, (1,), generator=g))).cuda()) for s in SHAPES]


def _grads(ps, seed, skip=(), misalign=False):
    g = torch.Generator().manual_seed(1000 + seed)
    for i, p in enumerate(ps):
        if i in skip:
            p.grad = None
            continue
        v = torch.randn(p.numel() + 1, generator=g).cuda() * 0.3
        p.grad = (v[1:] if misalign else v[:-1].clone()).view_as(p)          # (misalign: a 4-byte offset into a larger buffer)


def _state(opt, ps):
    """[(exp_avg, exp_avg_sq, step) or None per parameter], cloned."""
    out = []
    for p in ps:
        st = opt.state.get(p, {})
        out.append((st['exp_avg'].clone(), st['exp_avg_sq'].clone(), float(st['step'])) if 'exp_avg' in st else None)
    return out


def _run(opt_cls, kw, steps, groups=False, misalign=False, lr=1e-2):
    ps = _params(3)
    if groups:
        opt = opt_cls([dict(params=ps[:4], lr=lr), dict(params=ps[4:], lr=lr * 0.1)], lr=lr, **kw)
    else:
        opt = opt_cls(ps, lr=lr, **kw)
    out = []
    for k in range(steps):
        for g in opt.param_groups:
            g['lr'] = np.float64(g['lr'] * 0.9 + 1e-4 * k) if k % 2 else float(g['lr'] * 0.9 + 1e-4 * k)      # (LambdaLR hands over numpy floats)
        _grads(ps, k, skip=((1, 5) if k == 0 else (2,) if k == 2 else ()), misalign=misalign)
        opt.step()
        out.append(([p.detach().clone() for p in ps], _state(opt, ps)))
        opt.zero_grad()
        assert all(p.grad is None for p in ps)
    return out, opt, ps


def _assert_same_state(a, b, where, absent_is_zero=False):
    if absent_is_zero and a is None and b is not None:      # torch's unfused route: no state yet | zero moments at step 0
        assert b[2] == 0 and not bool(b[0].any()) and not bool(b[1].any()), where
        return
    assert (a is None) == (b is None), where
    if a is not None:
        assert torch.equal(a[0], b[0]), (where, 'exp_avg', float((a[0] - b[0]).abs().max()))
        assert torch.equal(a[1], b[1]), (where, 'exp_avg_sq', float((a[1] - b[1]).abs().max()))
        assert a[2] == b[2], (where, 'step', a[2], b[2])


# ------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize('ki', range(len(KWS)))
@pytest.mark.parametrize('groups,misalign', [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize('which', ['adamw', 'adam'])
def test_fused_adam_equals_torch_bit_for_bit(hip, which, groups, misalign, ki):
    fused, plain = _classes(which)
    want, _, _ = _run(plain, KWS[ki], 6, groups, misalign)
    got, opt, _ = _run(fused, KWS[ki], 6, groups, misalign)
    assert opt._fused_groups, 'the fused path did not run'
    for k, ((pa, sa), (pb, sb)) in enumerate(zip(want, got)):
        for i, (x, y) in enumerate(zip(pa, pb)):
            assert torch.equal(x, y), (k, i, float((x - y).abs().max()))
        for i, (x, y) in enumerate(zip(sa, sb)):
            _assert_same_state(x, y, (k, i))
    steps = [s[2] for s in got[-1][1]]
    assert steps[1] == 5 and steps[2] == 5 and steps[0] == 6      # (the per-parameter counts have diverged)


# ------------------------------------------------------------------ 2. stage probes
def _stage(L, stage, form, a, b=None, c=None, s=0.0):
    out = torch.empty_like(a)
    L.call('u2mkd_debug_adam_stage', stage, form, L.ptr(a), L.ptr(b), L.ptr(c), float(s), L.ptr(out), a.numel(), L.stream())
    return out


def _bits(t):
    return None if t is None else t.detach().clone().view(torch.int32)      # (bit patterns: a NaN equals itself)


def _probe(L, name, stage, forms, want, a, b=None, c=None, s=0.0):
    """Run the stage in every candidate form; print which equal torch's result and how many elements tell the forms apart (an
    equal result means something only where they differ); the form the optimizer uses must equal torch's everywhere."""
    from u2mkd_amd import optim
    outs = {label: _stage(L, stage, form, a, b, c, s) for label, (form, _) in forms.items()}
    labels = list(forms)
    for label in labels:
        wrong = int((_bits(outs[label]) != _bits(want)).sum())
        apart = {o: int((_bits(outs[label]) != _bits(outs[o])).sum()) for o in labels if o != label}
        print('stage %-22s form %-12s differs from torch in %7d of %d elements; from the other forms in %s'
              % (name, label, wrong, a.numel(), apart))
    used = [label for label, (form, mask) in forms.items() if (optim.ADAM_FORM & mask) == (form & mask)]
    assert len(used) == 1, used
    others = [o for o in labels if o != used[0]]
    assert all(int((_bits(outs[used[0]]) != _bits(outs[o])).sum()) > 0 for o in others), 'the probe does not tell the forms apart'
    assert torch.equal(_bits(outs[used[0]]), _bits(want)), (name, used[0])


def test_each_stage_equals_the_single_foreach_call(hip):
    L = hip
    n = 1 << 18
    g = torch.Generator(device='cuda').manual_seed(7)

    def rnd(scale_lo=-3, scale_hi=3):
        return torch.randn(n, device='cuda', generator=g) * 10 ** (torch.rand(n, device='cuda', generator=g) * (scale_hi - scale_lo) + scale_lo)

    fma = {'two roundings': 0, 'one fma': 1}
    m, gr = rnd(), rnd()
    for w in (1 - 0.9, 1 - 0.4):                       # the lerp at a weight below and above 0.5
        want = m.clone()
        torch._foreach_lerp_([want], [gr], w)
        _probe(L, 'lerp w=%.1f' % w, 0, {k: (2 * v, 2) for k, v in fma.items()}, want, m, gr, None, w)
    v = rnd().abs()
    want = v.clone()
    torch._foreach_addcmul_([want], [gr], [gr], 1 - 0.999)
    _probe(L, 'addcmul', 1, {k: (4 * v_, 4) for k, v_ in fma.items()}, want, v, gr, gr, 1 - 0.999)
    v = rnd(-12, 3).abs()
    want = torch._foreach_sqrt([v])[0]
    _probe(L, 'sqrt', 2, {'correct': (0 << 4, 3 << 4), 'approximate': (1 << 4, 3 << 4)}, want, v)
    s = (1 - 0.999 ** 3) ** 0.5
    x = rnd().abs()
    want = x.clone()
    torch._foreach_div_([want], [s])
    _probe(L, 'div by scalar', 3, {'correct': (0 << 6, 3 << 6), 'reciprocal': (1 << 6, 3 << 6), 'hw reciprocal': (2 << 6, 3 << 6)}, want, x, s=s)
    p, d = rnd(), rnd(-6, 2).abs() + 1e-8
    step_size = (1e-2 / (1 - 0.9 ** 3)) * -1
    want = p.clone()
    torch._foreach_addcdiv_([want], [m], [d], [step_size])
    forms = {'%s, %s' % (dk, fk): ((dv << 8) | (8 * fv), (3 << 8) | 8)
             for dk, dv in (('correct', 0), ('reciprocal', 1), ('hw reciprocal', 2)) for fk, fv in fma.items()}
    _probe(L, 'addcdiv', 4, forms, want, p, m, d, step_size)


# ------------------------------------------------------------------ 3. state_dict
@pytest.mark.parametrize('which', ['adamw', 'adam'])
def test_state_dict_round_trips_with_torchs_class(hip, which):
    fused_cls, plain_cls = _classes(which)
    kw = KWS[0]
    _, fused, ps_f = _run(fused_cls, kw, 3)
    _, plain, ps_p = _run(plain_cls, kw, 3)
    sd_f, sd_p = fused.state_dict(), plain.state_dict()
    assert sd_f['param_groups'] == sd_p['param_groups'] and sd_f['state'].keys() == sd_p['state'].keys()
    for k in sd_p['state']:
        assert sd_f['state'][k].keys() == sd_p['state'][k].keys()
        for key in ('exp_avg', 'exp_avg_sq', 'step'):
            assert torch.equal(sd_f['state'][k][key], sd_p['state'][k][key]), (k, key)
        assert sd_f['state'][k]['step'].device.type == 'cpu' and sd_f['state'][k]['step'].dtype == torch.float32
    # a torch checkpoint into the fused optimizer and the other way round, then two more steps each: same parameters
    ps_a, ps_b = _params(3), _params(3)
    for a, b, src in zip(ps_a, ps_b, ps_p):
        a.data.copy_(src.data); b.data.copy_(src.data)
    oa, ob = fused_cls(ps_a, lr=1e-2, **kw), plain_cls(ps_b, lr=1e-2, **kw)
    oa.load_state_dict(copy.deepcopy(sd_p)); ob.load_state_dict(copy.deepcopy(sd_f))
    for k in range(3, 5):
        for o, ps in ((oa, ps_a), (ob, ps_b)):
            _grads(ps, k)
            o.step()
    for a, b in zip(ps_a, ps_b):
        assert torch.equal(a, b)
    for x, y in zip(_state(ob, ps_b), _state(oa, ps_a)):
        _assert_same_state(x, y, 'after the round trip')
    fg = oa._fused_groups[0]
    assert all(oa.state[p]['exp_avg'].data_ptr() == b1.data_ptr() and oa.state[p]['exp_avg_sq'].data_ptr() == b2.data_ptr()
               for p, b1, b2 in zip(ps_a, fg.bufs, fg.bufs2))


# ------------------------------------------------------------------ 4. fall-backs
def test_falls_back_to_torch_where_the_kernel_does_not_apply(hip):
    from u2mkd_amd.optim import FusedAdam, FusedAdamW
    for fused_cls, plain_cls in ((FusedAdamW, torch.optim.AdamW), (FusedAdam, torch.optim.Adam)):
        for kw in (dict(amsgrad=True), dict(maximize=True), dict(lr=torch.tensor(1e-2), capturable=True)):
            kw = dict(dict(lr=1e-2, weight_decay=0.01), **kw)
            ps = _params(5)
            twin = [torch.nn.Parameter(p.detach().clone()) for p in ps]
            opt, plain = fused_cls(ps, **kw), plain_cls(twin, **kw)
            for k in range(2):
                _grads(ps, k); _grads(twin, k)
                opt.step(); plain.step()
            assert not opt._fused_groups, kw
            for a, b in zip(ps, twin):
                assert torch.equal(a, b), kw
        cpu = [torch.nn.Parameter(torch.randn(5, generator=torch.Generator().manual_seed(1)))]
        twin = [torch.nn.Parameter(cpu[0].detach().clone())]
        o2, p2 = fused_cls(cpu, lr=1e-2), plain_cls(twin, lr=1e-2)
        cpu[0].grad, twin[0].grad = torch.ones(5), torch.ones(5)
        o2.step(); p2.step()                                         # CPU parameters: torch's own step, no error
        assert not o2._fused_groups and torch.equal(cpu[0], twin[0])


# ------------------------------------------------------------------ 5. hooks
def test_global_step_hooks_fire_once_per_step(hip):
    from torch.optim.optimizer import register_optimizer_step_post_hook
    from u2mkd_amd.optim import FusedAdamW
    calls = []
    h = register_optimizer_step_post_hook(lambda *a: calls.append(1))
    try:
        ps = _params(7)
        opt = FusedAdamW(ps, lr=1e-2)
        _grads(ps, 0)
        opt.step()
        assert opt._fused_groups
        o2 = FusedAdamW(_params(8), lr=1e-2, amsgrad=True)      # (torch's own step behind the same wrapper)
        _grads(o2.param_groups[0]['params'], 0)
        o2.step()
        assert not o2._fused_groups
    finally:
        h.remove()
    assert len(calls) == 2


# ------------------------------------------------------------------ 6. under a scaler
SCALERS = [dict(), dict(init_scale=3000.0, growth_factor=1.7)]      # power-of-two scales | 1 / scale inexact
BAD = {0: (0, 17, INF), 3: (3, None, -INF), 4: (6, 100, NAN), 6: (5, None, NAN)}      # step -> (parameter, flat index or None = last, value)
AMP_STEPS = 8
I_MIS, I_LATE = 6, 7


def _no_grad_in(k, i):
    return i == I_LATE and k < 5              # (a parameter whose first gradient arrives late: the gradient set changes at step 5)


_BASE = {}


def _base_grads(bad):
    """The unscaled gradients of every step, on the device, made once (tuple ``bad``: the planted values); I_MIS's are 4-byte
    offset views of a larger buffer."""
    key = tuple(sorted(bad.items()))
    if key not in _BASE:
        out = []
        for k in range(AMP_STEPS):
            g = torch.Generator().manual_seed(2000 + k)
            row = []
            for i, s in enumerate(SHAPES):
                n = int(np.prod(s))
                v = torch.randn(n + 1, generator=g).cuda() * 0.3
                if _no_grad_in(k, i):
                    row.append(None)
                    continue
                v = v[1:] if i == I_MIS else v[:-1].clone()
                if k in bad and bad[k][0] == i:
                    v[n - 1 if bad[k][1] is None else bad[k][1]] = bad[k][2]
                row.append(v)
            out.append(row)
        _BASE[key] = out
        torch.cuda.synchronize()
    return _BASE[key]


def _assign(ps, scaler, base_row):
    """``.grad`` = the step's gradients times the scaler's scale, multiplied on the device (no host read)."""
    scale = scaler._scale if scaler._scale is not None else None
    for i, (p, b) in enumerate(zip(ps, base_row)):
        if b is None:
            p.grad = None
            continue
        if i == I_MIS:                        # keep the misalignment: scale into a 4-byte offset view
            buf = torch.empty(b.numel() + 1, device='cuda')
            torch.mul(b, scale, out=buf[1:])
            p.grad = buf[1:].view_as(p)
            assert p.grad.data_ptr() % 16 != 0
        else:
            p.grad = (b * scale).view_as(p)


def _run_amp(opt_cls, scaler_cls, kw, scaler_kw, explicit=False, bad=BAD, lagged=False, steps=AMP_STEPS):
    ps = _params(3)
    opt = opt_cls(ps, lr=1e-2, **kw)
    scaler = scaler_cls('cuda', growth_interval=2, **scaler_kw)
    scaler.scale(torch.ones((), device='cuda'))      # (creates the scale tensor)
    if lagged:
        # the outcomes reach the host only where the bookkeeping has to wait for them: the window grows to the ring's size
        real = opt._resolve
        opt._resolve = lambda k, wait: real(k, wait) if wait else None
        windows = []
        prepare = opt._prepare
        opt._prepare = lambda plans, scaled: (lambda d: (windows.append(d['window']), d)[1])(prepare(plans, scaled))
    base = _base_grads(bad)
    trace = []
    for k in range(steps):
        _assign(ps, scaler, base[k])
        assigned = [_bits(p.grad) for p in ps]
        if explicit:
            scaler.unscale_(opt)
        scaler.step(opt)
        scaler.update()
        trace.append(dict(params=[_bits(p) for p in ps], grads=[_bits(p.grad) for p in ps], assigned=assigned,
                          moments=[(opt.state[p]['exp_avg'].clone(), opt.state[p]['exp_avg_sq'].clone()) if 'exp_avg' in opt.state.get(p, {})
                                   else None for p in ps],
                          scale=None if lagged else scaler.get_scale(), tracker=None if lagged else scaler._get_growth_tracker()))
    sd = opt.state_dict()                     # (waits for the outstanding outcomes)
    steps_of = [float(sd['state'][i]['step']) if i in sd['state'] else 0.0 for i in range(len(ps))]
    final = dict(steps=steps_of, scale=scaler.get_scale(), tracker=scaler._get_growth_tracker())
    if lagged:
        final['windows'] = windows
    return trace, final, opt


_REF = {}


def _reference(ki, si, explicit, bad=BAD):
    """torch.optim.AdamW under torch.amp.GradScaler: computed once per setting, shared, never modified."""
    key = (ki, si, explicit, tuple(sorted(bad.items())))
    if key not in _REF:
        _REF[key] = _run_amp(torch.optim.AdamW, torch.amp.GradScaler, KWS[ki], SCALERS[si], explicit, bad)[:2]
    return _REF[key]


def _same(x, y):
    return (x is None and y is None) or (x is not None and y is not None and torch.equal(x, y))


def _compare_amp(want, got, route, explicit, bad=BAD, lagged=False):
    (wt, wf), (gt, gf) = want, got
    for k, (w, g) in enumerate(zip(wt, gt)):
        if not lagged:
            assert (w['scale'], w['tracker']) == (g['scale'], g['tracker']), (k, w['scale'], g['scale'])
        for i, (x, y) in enumerate(zip(w['params'], g['params'])):
            assert _same(x, y), (k, 'params', i)
        for i, (x, y) in enumerate(zip(w['moments'], g['moments'])):
            if x is None:                     # no state in torch's unfused route: none here, or zero moments
                assert y is None or (not bool(y[0].any()) and not bool(y[1].any())), (k, 'moments', i)
            else:
                assert y is not None and torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]), (k, 'moments', i)
        if k not in bad or explicit or route == 'own':
            for i, (x, y) in enumerate(zip(w['grads'], g['grads'])):
                assert _same(x, y), (k, 'grads', i)
        else:      # a skipped step through a plain torch.amp.GradScaler: nothing was written, the gradients are still scaled
            for i, (x, y) in enumerate(zip(g['assigned'], g['grads'])):
                assert _same(x, y), (k, 'grads stay scaled', i)
            assert not _same(w['grads'][0], g['grads'][0])
    assert wf['steps'] == gf['steps'], (wf['steps'], gf['steps'])
    assert (wf['scale'], wf['tracker']) == (gf['scale'], gf['tracker'])


def _scaler_cls(route):
    from u2mkd_amd import optim
    return optim.GradScaler if route == 'own' else torch.amp.GradScaler


def test_the_amp_script_does_what_it_says(hip):
    trace, final = _reference(0, 0, False)
    assert all(m is None for m in trace[0]['moments']), 'a skipped first step leaves no state'
    for k in range(1, AMP_STEPS):
        moved = not _same(trace[k]['params'][0], trace[k - 1]['params'][0])
        assert moved == (k not in BAD), k
    assert final['steps'][0] == AMP_STEPS - len(BAD) and final['steps'][I_LATE] == 2      # (steps 5 and 7)
    scales = [t['scale'] for t in trace]
    assert scales[0] < 65536.0 and scales[2] > scales[1] and scales[4] < scales[3] < scales[2], scales


@pytest.mark.parametrize('si', range(len(SCALERS)), ids=['pow2', 'inexact'])
@pytest.mark.parametrize('explicit', [False, True], ids=['step', 'unscale_then_step'])
@pytest.mark.parametrize('route', ['own', 'torch'])
def test_fused_adamw_under_a_grad_scaler_equals_torch_exactly(hip, route, explicit, si):
    from u2mkd_amd.optim import FusedAdamW
    got = _run_amp(FusedAdamW, _scaler_cls(route), KWS[0], SCALERS[si], explicit)
    assert got[2]._fused_groups, 'the fused path did not run'
    _compare_amp(_reference(0, si, explicit), got[:2], route, explicit)


@pytest.mark.parametrize('route', ['own', 'torch'])
def test_under_a_grad_scaler_with_outcomes_that_arrive_as_late_as_allowed(hip, route):
    """The same script (and a second one without a late parameter's change of the gradient set in its first seven steps) with
    the host folding outcomes in only where it must: the window of candidate step counts grows, the kernel picks its row by the
    device's own count, and everything still equals torch's run."""
    from u2mkd_amd.optim import FusedAdamW
    got = _run_amp(FusedAdamW, _scaler_cls(route), KWS[0], SCALERS[0], lagged=True)
    assert got[2]._fused_groups
    print('windows:', got[1]['windows'])
    assert max(got[1]['windows']) >= 5 and got[1]['windows'][:5] == [1, 2, 3, 4, 5], got[1]['windows']
    _compare_amp(_reference(0, 0, False), got[:2], route, False, lagged=True)


@pytest.mark.parametrize('route', ['own', 'torch'])
def test_add_param_group_while_outcomes_are_outstanding(hip, route):
    """Three scaled steps (the first skipped) whose outcomes the host has not seen, then ``add_param_group``: the counts of the
    outstanding steps reach the ``state`` of the first group's parameters, and the run goes on equal to torch's."""
    from u2mkd_amd.optim import FusedAdamW

    def run(opt_cls, scaler_cls, lagged):
        ps = _params(3)
        opt = opt_cls(ps[:6], lr=1e-2, **KWS[0])
        scaler = scaler_cls('cuda', growth_interval=2)
        scaler.scale(torch.ones((), device='cuda'))
        if lagged:
            real = opt._resolve
            opt._resolve = lambda k, wait: real(k, wait) if wait else None
        base = _base_grads(BAD)
        for k in range(5):
            if k == 3:
                opt.add_param_group(dict(params=ps[6:], lr=1e-3))
            _assign(ps, scaler, base[k if k < 3 else 7])      # (step 7: finite, every parameter has a gradient)
            scaler.step(opt)
            scaler.update()
        sd = opt.state_dict()
        return [p.detach().clone() for p in ps], [float(sd['state'][i]['step']) for i in range(len(ps))], opt

    want_p, want_s, _ = run(torch.optim.AdamW, torch.amp.GradScaler, False)
    got_p, got_s, opt = run(FusedAdamW, _scaler_cls(route), True)
    assert len(opt._fused_groups) == 2
    assert want_s == got_s == [4.0] * 6 + [2.0] * 4, (want_s, got_s)
    for i, (a, b) in enumerate(zip(want_p, got_p)):
        assert torch.equal(a, b), i


# ------------------------------------------------------------------ 7. no host read
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
    """From the fourth step of a run without planted values on, ``scaler.step(opt); scaler.update()`` reads nothing back: zero
    calls of Tensor.item / tolist / cpu / __bool__ and, where ``torch.cuda.set_sync_debug_mode('warn')`` reports a host read on
    this build (probed first; the outcome is printed), no synchronising call reported either."""
    from u2mkd_amd.optim import FusedAdamW
    ps = _params(3)
    opt = FusedAdamW(ps, lr=1e-2, **KWS[0])
    scaler = _scaler_cls(route)('cuda', growth_interval=2)
    scaler.scale(torch.ones((), device='cuda'))
    calls, reported, snaps = [], [], []
    sync_mode = _sync_debug_mode_works()
    print('set_sync_debug_mode reports host reads on this build:', sync_mode)
    base = _base_grads({})
    for k in range(6):
        _assign(ps, scaler, base[7])          # (step 7's gradients: every parameter has one)
        torch.cuda.synchronize()
        if k < 3:
            scaler.step(opt)
            scaler.update()
            continue
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
    assert not torch.equal(snaps[0], snaps[1]) and not torch.equal(snaps[1], snaps[2])      # (applied)
    opt.sync_steps()
    assert float(opt.state[ps[0]]['step']) == 6.0


# ------------------------------------------------------------------ 8. no gradient anywhere
def test_a_step_in_which_no_parameter_has_a_gradient(hip):
    from u2mkd_amd.optim import FusedAdamW
    for route in ('own', 'torch'):
        ps = _params(3)
        before = [p.detach().clone() for p in ps]
        opt = FusedAdamW(ps, lr=1e-2)
        scaler = _scaler_cls(route)('cuda')
        scaler.scale(torch.ones((), device='cuda'))
        scaler.step(opt)
        assert not opt.state and all(torch.equal(a, b) for a, b in zip(before, ps))
    opt = FusedAdamW(ps, lr=1e-2)
    opt.step()
    assert not opt.state and all(torch.equal(a, b) for a, b in zip(before, ps))


# ------------------------------------------------------------------ 9. LidarStep with adamw_spformer
CHILD = '''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import test_gpu_optim_adamw as T
from u2mkd_amd import optim
assert not optim._ADAM_ENABLED
out = {}
for amp in (False, 'fp16'):
    params, losses, run = T._lidar_steps(amp)
    assert not run.opt._fused_groups
    out[str(amp)] = ([p.cpu() for p in params], losses)
torch.save(out, sys.argv[1])
print("ok")
'''


def _lidar_steps(amp):
    """Three LidarStep steps of the SPVCNN + SphereFormer teacher under make_optimizer('adamw_spformer') on the 3000-point scene
    of tests/test_gpu_optim_amp.py's trainer test."""
    from u2mkd_amd import lidar, train
    from u2mkd_amd.synth import synth_batch
    b = synth_batch(3000, 1, 9)
    feats, coords, labels = (torch.from_numpy(b[k]).cuda() for k in ('feats', 'coords', 'labels'))
    torch.manual_seed(0)
    model = lidar.SPVCNN_SPFORMER(**lidar.spformer_kwargs(cr=1.0, drop_path_rate=0.0)).cuda().train()
    model.dropout.p = 0.0
    run = train.LidarStep(model, amp=amp, optimizer=lambda net: train.make_optimizer(net, name='adamw_spformer', lr=1e-3, weight_decay=0.01))
    losses = [float(run(feats, coords, labels)) for _ in range(3)]
    if hasattr(run.opt, 'sync_steps'):
        run.opt.sync_steps()
    print('LidarStep adamw_spformer amp=%s: losses %s' % (amp, losses))
    return [p.detach() for p in model.parameters()], losses, run


def test_lidar_step_adamw_spformer_equals_torchs_step(hip, tmp_path):
    """fp32 and amp='fp16': losses and final parameters equal those of the same run with U2MKD_FUSED_ADAM=0 (read at import) in a
    fresh process, where the same classes run torch's own step."""
    from u2mkd_amd import optim
    out = str(tmp_path / 'params.pt')
    r = subprocess.run([sys.executable, '-c', CHILD % (ROOT, os.path.join(ROOT, 'tests')), out],
                       env=dict(os.environ, U2MKD_FUSED_ADAM='0'), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    want = torch.load(out)
    for amp in (False, 'fp16'):
        params, losses, run = _lidar_steps(amp)
        assert type(run.opt) is optim.FusedAdamW and run.opt._fused_groups and len(run.opt.param_groups) == 2
        assert all(len(g['params']) > 0 for g in run.opt.param_groups)
        w_params, w_losses = want[str(amp)]
        assert losses == w_losses, (amp, losses, w_losses)
        assert len(w_params) == len(params)
        for i, (a, b) in enumerate(zip(w_params, params)):
            assert torch.equal(a, b.cpu()), (amp, i, float((a - b.cpu()).abs().max()))
        assert any(float(st['step']) >= 1 for st in run.opt.state.values()), 'no step was applied'
