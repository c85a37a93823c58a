"""optim.FusedSGD under a GradScaler away from the HIP device (CPU parameters: torch's own step, ``FusedSGD._torch_step``):
the optimizer announces ``_step_supports_amp_scaling``, so the scaler calls ``step()`` unconditionally with ``grad_scale`` /
``found_inf`` set, and the fall-back has to do what the scaler's generic route does around torch's unfused step -- unscale,
read ``found_inf``, skip.  Against ``torch.optim.SGD`` under ``torch.amp.GradScaler('cpu')``, exact: parameters, momentum
buffers, the keys of ``state`` (none after a skipped first step), gradients, scale and growth tracker."""
import pytest
import torch

from u2mkd_amd import optim

KW = dict(lr=0.24, momentum=0.9, weight_decay=1e-4, nesterov=True)
SHAPES = [(7, 3), (5,), (1,), (2, 3, 4)]
BAD = {0: float('inf'), 3: float('nan')}          # step -> the value planted in one gradient (the FIRST step is skipped)
STEPS = 6


def _params():
    g = torch.Generator().manual_seed(11)
    return [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in SHAPES]


def _grad(k, i, p, scale):
    if i == 3 and k < 2:
        return None                                # (a parameter whose first gradient comes later)
    g = torch.randn(p.shape, generator=torch.Generator().manual_seed(100 * k + i)) * 0.3 * scale
    if k in BAD and i == 1:
        g.view(-1)[2] = BAD[k]
    return g


def _run(opt_cls, scaler_cls, explicit_unscale=False, **scaler_kw):
    ps = _params()
    opt = opt_cls(ps, **KW)
    scaler = scaler_cls('cpu', growth_interval=2, **scaler_kw)
    trace = []
    for k in range(STEPS):
        scale = float(scaler.scale(torch.ones(())))
        for i, p in enumerate(ps):
            p.grad = _grad(k, i, p, scale)
        if explicit_unscale:
            scaler.unscale_(opt)
        scaler.step(opt)
        scaler.update()
        trace.append(dict(
            params=[p.detach().clone() for p in ps],
            bufs=[opt.state[p]['momentum_buffer'].clone() if 'momentum_buffer' in opt.state.get(p, {}) else None for p in ps],
            grads=[None if p.grad is None else p.grad.clone() for p in ps],
            scale=scaler.get_scale(), tracker=scaler._get_growth_tracker()))
    return trace


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return torch.equal(a.view(torch.int32), b.view(torch.int32))          # (bit patterns: NaN equals NaN)


def _assert_equal_traces(want, got):
    for k, (w, g) in enumerate(zip(want, got)):
        assert (w['scale'], w['tracker']) == (g['scale'], g['tracker']), k
        for key in ('params', 'bufs', 'grads'):
            for i, (x, y) in enumerate(zip(w[key], g[key])):
                assert _same(x, y), (k, key, i)


@pytest.fixture(scope='module')
def reference():
    return {(e, s): _run(torch.optim.SGD, torch.amp.GradScaler, explicit_unscale=e, **dict(s))
            for e in (False, True) for s in ((), (('init_scale', 3000.0), ('growth_factor', 1.7)))}


def test_reference_script_skips_the_first_step_and_creates_no_state(reference):
    t = reference[(False, ())]
    assert all(b is None for b in t[0]['bufs']) and t[0]['scale'] == 32768.0
    assert all(b is not None for b in t[1]['bufs'][:3]) and t[1]['bufs'][3] is None and t[2]['bufs'][3] is not None
    assert t[3]['scale'] < t[2]['scale']


@pytest.mark.parametrize('scaler_kw', [(), (('init_scale', 3000.0), ('growth_factor', 1.7))], ids=['pow2', 'inexact'])
@pytest.mark.parametrize('explicit', [False, True], ids=['step', 'unscale_then_step'])
@pytest.mark.parametrize('scaler', ['torch', 'own'])
def test_fused_sgd_fallback_under_a_grad_scaler_equals_torch_sgd(reference, scaler, explicit, scaler_kw):
    cls = torch.amp.GradScaler if scaler == 'torch' else optim.GradScaler
    got = _run(optim.FusedSGD, cls, explicit_unscale=explicit, **dict(scaler_kw))
    _assert_equal_traces(reference[(explicit, scaler_kw)], got)


def test_protocol_attributes_and_class_hierarchy():
    assert optim.FusedSGD._step_supports_amp_scaling is True
    assert issubclass(optim.GradScaler, torch.amp.GradScaler)
    assert optim.GradScaler('cpu').state_dict().keys() == torch.amp.GradScaler('cpu').state_dict().keys()
    a, b = optim.GradScaler('cpu', init_scale=512.0), torch.amp.GradScaler('cpu', init_scale=512.0)
    a.scale(torch.ones(())); b.scale(torch.ones(()))
    assert a.state_dict() == b.state_dict()
    c = optim.GradScaler('cpu')
    c.load_state_dict(b.state_dict())
    assert c.state_dict() == b.state_dict()


def test_own_scaler_with_a_plain_torch_optimizer_is_the_parent(reference):
    got = _run(torch.optim.SGD, optim.GradScaler)
    _assert_equal_traces(reference[(False, ())], got)
    got = _run(torch.optim.SGD, optim.GradScaler, explicit_unscale=True, init_scale=3000.0, growth_factor=1.7)
    _assert_equal_traces(reference[(True, (('init_scale', 3000.0), ('growth_factor', 1.7)))], got)


@pytest.mark.parametrize('scaler', ['torch', 'own'])
def test_a_step_in_which_no_parameter_has_a_gradient(scaler):
    """torch's scaler then hands over ``found_inf = sum([])``, the int 0: the step neither raises nor writes."""
    cls = torch.amp.GradScaler if scaler == 'torch' else optim.GradScaler
    ps = _params()
    before = [p.detach().clone() for p in ps]
    opt = optim.FusedSGD(ps, **KW)
    sc = cls('cpu')
    sc.scale(torch.ones(()))
    sc.step(opt)
    assert not opt.state and all(torch.equal(a, b) for a, b in zip(before, ps))
