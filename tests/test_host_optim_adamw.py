"""optim.FusedAdam / optim.FusedAdamW away from the HIP device: the class hierarchy and the scaler protocol's attribute, CPU
parameters (torch's own step, exactly, without a scaler and under ``GradScaler('cpu')``), ``train.make_optimizer``, the host's
step scalars against torch's expressions, and the bookkeeping of step counts under a scaler (``optim.StepLedger``) driven with
scripted outcomes that arrive late and in batches."""
import numpy as np
import pytest
import torch

from u2mkd_amd import optim

SHAPES = [(7, 3), (5,), (1,), (2, 3, 4)]
BAD = {0: float('inf'), 3: float('nan')}          # step -> the value planted in one gradient (the FIRST step is skipped)
STEPS = 6
PAIRS = [(optim.FusedAdamW, torch.optim.AdamW), (optim.FusedAdam, torch.optim.Adam)]


def test_class_hierarchy_and_protocol_attribute():
    assert issubclass(optim.FusedAdamW, torch.optim.AdamW) and issubclass(optim.FusedAdamW, torch.optim.Adam)
    assert issubclass(optim.FusedAdam, torch.optim.Adam) and not issubclass(optim.FusedAdam, torch.optim.AdamW)
    assert optim.FusedAdam._step_supports_amp_scaling is True and optim.FusedAdamW._step_supports_amp_scaling is True
    assert optim.FusedSGD._step_supports_amp_scaling is True and issubclass(optim.FusedSGD, torch.optim.SGD)
    p = [torch.nn.Parameter(torch.zeros(3))]
    a, b = optim.FusedAdamW(p, lr=1e-3, weight_decay=0.05), torch.optim.AdamW(p, lr=1e-3, weight_decay=0.05)
    assert a.state_dict()['param_groups'] == b.state_dict()['param_groups']
    assert a.param_groups[0]['decoupled_weight_decay'] is True
    assert not optim.FusedAdam(p, lr=1e-3).param_groups[0]['decoupled_weight_decay']


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


def _state(opt, ps):
    return [tuple(opt.state[p][k].clone() for k in ('exp_avg', 'exp_avg_sq', 'step')) if 'exp_avg' in opt.state.get(p, {}) else None
            for p in ps]


def _run(opt_cls, scaler_cls=None, explicit_unscale=False, **scaler_kw):
    ps = _params()
    opt = opt_cls(ps, lr=1e-2, weight_decay=0.01)
    scaler = None if scaler_cls is None else scaler_cls('cpu', growth_interval=2, **scaler_kw)
    trace = []
    for k in range(STEPS):
        scale = 1.0 if scaler is None else float(scaler.scale(torch.ones(())))
        for i, p in enumerate(ps):
            p.grad = _grad(k, i, p, scale) if scaler is not None or k not in BAD else _grad(k + 50, i, p, scale)
        if scaler is None:
            opt.step()
        else:
            if explicit_unscale:
                scaler.unscale_(opt)
            scaler.step(opt)
            scaler.update()
        trace.append(dict(params=[p.detach().clone() for p in ps], state=_state(opt, ps),
                          grads=[None if p.grad is None else p.grad.clone() for p in ps],
                          scale=None if scaler is None else scaler.get_scale(),
                          tracker=None if scaler is None else scaler._get_growth_tracker()))
    assert not getattr(opt, '_fused_groups', None)
    return trace


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return torch.equal(a.view(torch.int32), b.view(torch.int32))          # (bit patterns: NaN equals NaN)


def _assert_equal_traces(want, got):
    for k, (w, g) in enumerate(zip(want, got)):
        assert (w['scale'], w['tracker']) == (g['scale'], g['tracker']), k
        for key in ('params', 'grads'):
            for i, (x, y) in enumerate(zip(w[key], g[key])):
                assert _same(x, y), (k, key, i)
        for i, (x, y) in enumerate(zip(w['state'], g['state'])):
            assert (x is None) == (y is None), (k, 'state', i)
            if x is not None:
                assert all(_same(a, b) for a, b in zip(x, y)), (k, 'state', i)


@pytest.mark.parametrize('fused,plain', PAIRS, ids=['adamw', 'adam'])
def test_cpu_parameters_are_torchs_step_exactly(fused, plain):
    _assert_equal_traces(_run(plain), _run(fused))


@pytest.mark.parametrize('scaler_kw', [(), (('init_scale', 3000.0), ('growth_factor', 1.7))], ids=['pow2', 'inexact'])
@pytest.mark.parametrize('explicit', [False, True], ids=['step', 'unscale_then_step'])
@pytest.mark.parametrize('scaler', ['torch', 'own'])
@pytest.mark.parametrize('fused,plain', PAIRS, ids=['adamw', 'adam'])
def test_cpu_parameters_under_a_grad_scaler_are_torchs_route_exactly(fused, plain, scaler, explicit, scaler_kw):
    cls = torch.amp.GradScaler if scaler == 'torch' else optim.GradScaler
    want = _run(plain, torch.amp.GradScaler, explicit_unscale=explicit, **dict(scaler_kw))
    assert all(s is None for s in want[0]['state']) and want[3]['scale'] < want[2]['scale']      # (the script skips steps 0 and 3)
    _assert_equal_traces(want, _run(fused, cls, explicit_unscale=explicit, **dict(scaler_kw)))


def test_make_optimizer_returns_the_fused_classes_with_the_references_groups():
    from u2mkd_amd import train as T

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.stem = torch.nn.Linear(3, 4)
            self.transformer_block = torch.nn.Linear(4, 4)
            self.frozen = torch.nn.Linear(2, 2)
            for p in self.frozen.parameters():
                p.requires_grad = False

    net = Net()
    opt = T.make_optimizer(net, name='adamw_spformer', lr=1e-3, weight_decay=0.05, transformer_lr_scale=0.5)
    assert type(opt) is optim.FusedAdamW and isinstance(opt, torch.optim.AdamW)
    assert [len(g['params']) for g in opt.param_groups] == [2, 2]
    assert [g['lr'] for g in opt.param_groups] == [1e-3, 5e-4] and all(g['weight_decay'] == 0.05 for g in opt.param_groups)
    assert {id(p) for p in opt.param_groups[1]['params']} == {id(p) for p in net.transformer_block.parameters()}
    plain = torch.optim.AdamW([dict(params=list(net.stem.parameters()), lr=1e-3, weight_decay=0.05),
                               dict(params=list(net.transformer_block.parameters()), lr=5e-4, weight_decay=0.05)], lr=1e-3, weight_decay=0.05)
    assert opt.state_dict()['param_groups'] == plain.state_dict()['param_groups']
    a = T.make_optimizer(net, name='adam', lr=2e-3, weight_decay=1e-4)
    assert type(a) is optim.FusedAdam and not isinstance(a, torch.optim.AdamW) and a.param_groups[0]['lr'] == 2e-3
    assert len(a.param_groups[0]['params']) == 6 and a.param_groups[0]['weight_decay'] == 1e-4
    w = T.make_optimizer(net.parameters(), name='adamw', lr=2e-3, weight_decay=1e-2)
    assert type(w) is optim.FusedAdamW and w.param_groups[0]['weight_decay'] == 1e-2


@pytest.mark.parametrize('betas', [(0.9, 0.999), (0.8, 0.95), (0.4, 0.999)])
def test_step_scalars_are_torchs_expressions(betas):
    """torch/optim/adam.py:_multi_tensor_adam, non-capturable: written out here as torch writes them, for a float and a numpy lr."""
    from torch.optim.optimizer import _get_value
    beta1, beta2 = betas
    for lr in (1e-3, np.float64(0.24 * 0.37)):
        for t in range(1, 2001):
            step = torch.tensor(float(t), dtype=torch.float32)
            bias_correction1 = 1 - beta1 ** _get_value(step)
            bias_correction2 = 1 - beta2 ** _get_value(step)
            want = ((lr / bias_correction1) * -1, bias_correction2 ** 0.5)
            got = optim.adam_scalars(lr, beta1, beta2, float(t))
            assert got == want and np.float32(got[0]) == np.float32(want[0]), (t, got, want)


# ------------------------------------------------------------------ the bookkeeping of step counts
class _Device:
    """What the device does with a scaled call: counts the applied ones, and picks the candidate row by its own count."""

    def __init__(self, n):
        self.count = 0
        self.true = np.zeros(n, dtype=np.int64)

    def run(self, mask, applied, candidates, count_known):
        row = self.count - count_known
        assert 0 <= row < candidates.shape[1], (row, candidates.shape)
        assert np.array_equal(candidates[mask, row], self.true[mask] + 1), 'the true count is not at the true offset'
        if applied:
            self.true[mask] += 1
            self.count += 1
        return self.count


def _drive(lag, script, n=5, ring=8):
    """``script``: [(gradient set, applied)] per call.  Outcomes become visible ``lag`` calls late and are folded in batches (all
    visible ones at once); where the ledger says the host must wait, the oldest pending outcomes are handed over at once."""
    led = optim.StepLedger(n, ring=ring)
    dev = _Device(n)
    outcomes = {}                                  # call -> the device's count after it
    waits = 0
    for call, (mask, applied) in enumerate(script):
        mask = np.array(mask, dtype=bool)
        visible = [c for c, _ in led.pending if c <= call - 1 - lag]
        if visible:
            led.fold([outcomes[c] for c in visible])
        k = led.must_resolve(mask)
        if k:
            waits += 1
            led.fold([outcomes[c] for c, _ in led.pending[:k]])
        assert led.must_resolve(mask) == 0
        assert 1 <= led.window() <= ring
        cand = led.candidates()
        assert cand.shape == (n, led.window())
        number = led.issue(mask)
        assert number == call and (number & 1) == (call & 1)
        outcomes[call] = dev.run(mask, applied, cand, led.applied_known)
    led.fold([outcomes[c] for c, _ in led.pending])
    assert not led.pending and led.applied_known == dev.count
    replay = np.zeros(n, dtype=np.int64)
    for mask, applied in script:
        if applied:
            replay[np.array(mask, dtype=bool)] += 1
    assert np.array_equal(led.known, replay) and np.array_equal(dev.true, replay)
    return waits


ALL, SOME = [1, 1, 1, 1, 1], [1, 0, 1, 1, 0]


@pytest.mark.parametrize('lag', [0, 1, 3, 7, 100])
def test_step_ledger_with_late_outcomes_in_batches(lag):
    rng = np.random.RandomState(lag)
    # skipped first call, two skipped in a row, a changing gradient set inside the window, then a long run with one set
    script = [(ALL, False), (ALL, True), (ALL, True), (ALL, False), (ALL, False), (SOME, True), (SOME, False), (ALL, True)]
    script += [(ALL, bool(rng.rand() < 0.8)) for _ in range(30)] + [(SOME, True), (SOME, True), (ALL, False), (ALL, True)]
    waits = _drive(lag, script)
    if lag == 0:
        assert waits == 0                          # (every outcome is known before the next call: never a wait, window 1)
    if lag == 100:
        assert waits >= 4 + 3                      # (nothing ever arrives by itself: the ring fills, and every change of the set waits)


def test_step_ledger_window_and_refusals():
    led = optim.StepLedger(2, ring=4)
    m = np.array([True, True])
    for k in range(4):
        assert led.must_resolve(m) == 0 and led.window() == k + 1      # (the fourth call goes out with a window of 4 = the ring)
        led.issue(m)
    assert led.must_resolve(m) == 1                                         # (a fifth would need a window above the ring)
    assert led.must_resolve(np.array([True, False])) == 4                   # (another gradient set: the window has to be empty)
    with pytest.raises(AssertionError):
        led.issue(m)
    led.fold([1])
    assert list(led.known) == [1, 1] and led.applied_known == 1 and led.window() == 4
    assert led.candidates().tolist() == [[2, 3, 4, 5], [2, 3, 4, 5]]
    with pytest.raises(RuntimeError):
        led.fold([3])                                                          # (a count that no single call can produce)
    with pytest.raises(AssertionError):
        led.advance(m)                                                         # (a host-known step while outcomes are outstanding)
