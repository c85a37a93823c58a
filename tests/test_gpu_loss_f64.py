"""The loss kernels on the device (csrc/lovasz.hip behind losses._LovaszFunction, _CrossEntropyFunction, _KLDivFunction) against
the float64 evaluation and the derived elementwise bound of tests/loss_f64_ref.py.

  1  every case of ``CASES``: the Function is called directly, so the leaf is the kernel's own input (a column slice of a wider
     tensor in the 'wide' cases); the loss and every element of the gradient inside the bound, a zero bound meaning equality;
     for Lovasz the undecided entries of a tie inside their envelope and every run's sum inside the sum of its bounds; two
     calls give the same bits;
  2  one case through softmax and MixLovaszCrossEntropy;
  3  the argument checks that return before any launch, and Lovasz_softmax's torch path above 4096 classes.

Each case prints one ``LOSSF64 <kernel> <case> <output> err/bound = ...`` line per output; the figures on the MI355X: NOTES N27."""
import pytest
import torch

import loss_f64_ref as R

pytestmark = pytest.mark.gpu

PAD = 3                                                 # columns around a 'wide' input


def _leaf(t, wide):
    """(the kernel's input on the device, the leaf whose .grad is read, the columns of the input in the leaf)"""
    if not wide:
        leaf = t.cuda().requires_grad_(True)
        return leaf, leaf, slice(None)
    n, c = t.shape
    base = torch.full((n, c + PAD), 0.25, dtype=t.dtype)
    base[:, 1:c + 1] = t
    leaf = base.cuda().requires_grad_(True)
    view = leaf[:, 1:c + 1]
    assert not view.is_contiguous()
    return view, leaf, slice(1, c + 1)


def _run(case):
    """{output: CPU tensor} of one case: the loss and the gradient of the kernel's own input for the upstream gradient g"""
    from u2mkd_amd import losses
    k, wide = case['kernel'], case['wide']
    if k == 'lovasz':
        inp, leaf, cols = _leaf(case['probas'], wide)
        loss = losses._LovaszFunction.apply(inp, case['labels'].cuda(), case['ignore'])
        name = 'd'
    elif k == 'ce':
        inp, leaf, cols = _leaf(case['x'], wide)
        loss = losses._CrossEntropyFunction.apply(inp, case['labels'].cuda(), case['ignore'])
        name = 'dx'
    else:
        inp, leaf, cols = _leaf(case['s'], wide)
        t = _leaf(case['t'], wide)[0].detach()
        loss = losses._KLDivFunction.apply(inp, t, case['index'].cuda() if case['index'] is not None else None)
        name = 'ds'
    loss.backward(torch.tensor(case['g'], dtype=torch.float32, device='cuda'))
    torch.cuda.synchronize()
    grad = leaf.grad.cpu()
    if wide:                                            # nothing reaches the columns around the input
        rest = torch.ones(grad.shape[1], dtype=torch.bool)
        rest[cols] = False
        assert float(grad[:, rest].abs().max()) == 0.0
    return {'loss': loss.detach().cpu(), name: grad[:, cols].contiguous()}


# ------------------------------------------------------------------ 1. every case against float64
@pytest.mark.parametrize('name', R.CASES)
def test_loss_kernels_inside_the_float64_bound(hip, name):
    """Loss and gradient of every case inside the derived bound -- no element excluded; the undecided entries of a Lovasz tie
    inside their envelope (loss_f64_ref L5), every run's sum inside the sum of its bounds -- and the same bits from a second call."""
    case = R.make_case(name)
    ref = R.evaluate64(case)
    if case['kernel'] == 'lovasz':
        assert ref['share'] <= R.TIE_CASES.get(name, R.UNDECIDED_CAP), ref['share']
    got = _run(case)
    res = R.check(case, ref, got)
    print('\n' + '\n'.join('LOSSF64 %s %s %s err/bound = %.4f' % (case['kernel'], name, out, over) for out, (_, over) in res.items()))
    failed = {out: over for out, (ok, over) in res.items() if not ok}
    assert not failed, failed
    again = _run(case)
    assert all(torch.equal(got[k], again[k]) or (k == 'loss' and bool(torch.isnan(got[k])) and bool(torch.isnan(again[k])))
               for k in got), name


# ------------------------------------------------------------------ 2. through softmax and the module
def test_mix_lovasz_cross_entropy_through_softmax(hip):
    """MixLovaszCrossEntropy(ignore_index=255)(x, y) = Lovasz(softmax(x)) + CE(x).  The Lovasz kernel sees the fp32 probabilities
    torch's softmax stores, so its reference is taken on THOSE; torch's softmax backward is dx = p (dp - sum_c p dp) on the stored
    p: the Lovasz bound passes through it as p (b + sum_c p b), the arithmetic adds g(C + 4) p (|dp| + sum_c p |dp|), the sum
    of the two gradients one rounding."""
    from u2mkd_amd import losses
    case = R.make_case('ce-1500x17-i255')
    x, y, ignore, g = case['x'], case['labels'], case['ignore'], 65536.0
    assert ignore == 255
    xg = x.cuda().requires_grad_(True)
    crit = losses.MixLovaszCrossEntropy(ignore_index=ignore)
    loss = crit(xg, y.cuda())
    loss.backward(torch.tensor(g, dtype=torch.float32, device='cuda'))
    p = torch.softmax(x.cuda(), 1).cpu()                # the probabilities the Lovasz kernel was given
    lv, ce = R.lovasz64(p, y, ignore, g), R.ce64(x, y, ignore, g)
    assert lv['share'] == 0.0
    C = x.shape[1]
    pd, dp, b = p.double(), lv['d'], lv['b_d']
    dx_sm = pd * (dp - (pd * dp).sum(1, keepdim=True))
    b_sm = pd * (b + (pd * b).sum(1, keepdim=True)) + R.g_(C + 4) * pd * (dp.abs() + (pd * dp.abs()).sum(1, keepdim=True))
    want = dx_sm + ce['dx']
    bound = b_sm + ce['b_dx']
    bound = bound + R.U32 * (want.abs() + bound)
    total, b_total = lv['loss'] + ce['loss'], lv['b_loss'] + ce['b_loss']
    res = {'loss': R._scalar(loss.detach().cpu(), total, b_total + R.U32 * (abs(total) + b_total)),
           'dx': R._tensor(xg.grad.cpu(), want, bound)}
    print('\n' + '\n'.join('LOSSF64 mix ce-1500x17-i255 %s err/bound = %.4f' % (out, over) for out, (_, over) in res.items()))
    assert all(ok for ok, _ in res.values()), res
    assert float(xg.grad[(y == ignore).cuda()].abs().max()) == 0.0


# ------------------------------------------------------------------ 3. argument checks, and the path above 4096 classes
def test_argument_checks_return_before_any_launch(hip):
    L = hip
    f = torch.zeros(64, dtype=torch.float32, device='cuda')
    d = torch.zeros(64, dtype=torch.float64, device='cuda')
    i = torch.zeros(64, dtype=torch.int64, device='cuda')
    with pytest.raises(RuntimeError, match='u2mkd_lovasz_errors'):
        L.call('u2mkd_lovasz_errors', L.ptr(f), L.ptr(i), 0, 1, 4097, L.ptr(f), L.ptr(d), L.stream())
    with pytest.raises(RuntimeError, match='u2mkd_ce_forward'):
        L.call('u2mkd_ce_forward', L.ptr(f), L.ptr(i), 0, 0, 17, L.ptr(f), L.ptr(f), L.ptr(f), L.stream())
    with pytest.raises(RuntimeError, match='u2mkd_kl_forward'):
        L.call('u2mkd_kl_forward', L.ptr(f), L.ptr(f), None, 0, 17, L.ptr(f), L.ptr(f), L.ptr(f), L.stream())
    torch.cuda.synchronize()
    assert float(f.abs().max()) == 0.0 and float(d.abs().max()) == 0.0


def test_lovasz_above_4096_classes_takes_the_torch_path(hip, monkeypatch):
    """Lovasz_softmax with C = 4097: the torch formulation (torch's own order of summation: the depth of L3 is taken as P + C + 2,
    every addition there could be), the same reference and bound"""
    from u2mkd_amd import losses
    P, C, ignore, g = 5, 4097, 255, -0.37
    gen = torch.Generator().manual_seed(4097)
    p = torch.softmax(torch.randn(P, C, generator=gen) * 2, 1)
    y = torch.tensor([0, 4096, ignore, 7, 7])
    calls, real = [], hip.call
    monkeypatch.setattr(hip, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    pg = p.cuda().requires_grad_(True)
    loss = losses.Lovasz_softmax(ignore_index=ignore)(pg, y.cuda())
    loss.backward(torch.tensor(g, dtype=torch.float32, device='cuda'))
    assert not [c for c in calls if 'lovasz' in c], calls
    ref = R.lovasz64(p, y, ignore, g, depth=P + C + 2)
    assert ref['npresent'] == 3.0 and ref['share'] <= R.UNDECIDED_CAP
    res = R.check_lovasz(ref, loss.detach().cpu(), pg.grad.cpu())
    print('\n' + '\n'.join('LOSSF64 lovasz-torch 5x4097 %s err/bound = %.4f' % (out, over) for out, (_, over) in res.items()))
    assert all(ok for ok, _ in res.values()), res
