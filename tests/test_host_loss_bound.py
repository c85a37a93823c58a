"""The float64 reference and bound of the loss kernels (tests/loss_f64_ref.py) on the CPU: the bound can fail.

  1  every formulation of ``WRONG`` is rejected on its named case, on the outputs it should break; the honest fp32 evaluation in
     the kernels' order is admitted on the same case;
  2  the honest fp32 evaluation is admitted on EVERY case of ``CASES``, also with the entries of equal error ordered the other
     way round; the share of undecided entries stays at or below UNDECIDED_CAP on every case not built to tie, the tie cases
     have the share they state;
  3  the reference agrees with torch in float64 -- F.cross_entropy, nn.KLDivLoss(reduction='batchmean'), the oracle's
     lovasz_softmax_flat on .double() inputs -- to 1e-12 relative, values and gradients;
  4  every row ignored: nan and a zero gradient for cross entropy, 0 and 0 for Lovasz, as torch gives them;
  5  the package's torch formulation of Lovasz (losses.lovasz_softmax_flat, the path above 4096 classes) on the CPU, every case."""
import math

import pytest
import torch

import loss_f64_ref as R

_REF = {}


def _ref(name):
    if name not in _REF:
        case = R.make_case(name)
        _REF[name] = (case, R.evaluate64(case))
    return _REF[name]


# ------------------------------------------------------------------ 1. the wrong formulations
@pytest.mark.parametrize('wrong', list(R.WRONG))
def test_wrong_formulation_is_rejected_where_the_honest_one_is_admitted(wrong):
    kernel, name, broken = R.WRONG[wrong]
    case, ref = _ref(name)
    assert case['kernel'] == kernel
    honest = R.check(case, ref, R.honest_fp32(case))
    assert all(ok for ok, _ in honest.values()), honest
    res = R.check(case, ref, R.honest_fp32(case, wrong=wrong))
    print('\n%s on %s: %s' % (wrong, name, {k: '%.3g' % v[1] for k, v in res.items()}))
    for out in broken:
        assert not res[out][0], (wrong, out, res)


def test_every_wrong_formulation_of_the_list_is_there():
    assert len(R.WRONG) == 12 and sorted(k for k, _, _ in R.WRONG.values()) == ['ce'] * 3 + ['kl'] * 3 + ['lovasz'] * 6


# ------------------------------------------------------------------ 2. the honest evaluation, every case
@pytest.mark.parametrize('name', R.CASES)
def test_honest_fp32_is_admitted_on_every_case(name):
    case, ref = _ref(name)
    res = R.check(case, ref, R.honest_fp32(case))
    print('\n%s: %s' % (name, {k: '%.3f' % v[1] for k, v in res.items()}))
    assert all(ok for ok, _ in res.values()), res
    if case['kernel'] == 'lovasz':
        if name in R.TIE_CASES:
            assert R.UNDECIDED_CAP < ref['share'] <= R.TIE_CASES[name], ref['share']
        else:
            assert ref['share'] <= R.UNDECIDED_CAP, ref['share']
        other = R.check(case, ref, R.honest_fp32(case, reverse_ties=True))
        assert all(ok for ok, _ in other.values()), other


def test_the_tie_cases_change_with_the_order_of_their_ties():
    """the envelope is needed: with the ties the other way round, undecided entries leave the bound of the reference's own order
    (so a check without L5 would reject an honest evaluation), while the run sums and the loss stay inside"""
    for name in R.TIE_CASES:
        case, ref = _ref(name)
        got = R.honest_fp32(case, reverse_ties=True)
        strict = R._tensor(got['d'], ref['d'], ref['b_d'])
        assert not strict[0], name
        res = R.check(case, ref, got)
        assert res['d_run_sum'][0] and res['loss'][0] and res['d_undecided'][0] and res['d'][0], res


def test_an_undecided_entry_outside_its_envelope_is_rejected():
    name = 'lv-512x2-i255-tied'
    case, ref = _ref(name)
    got = R.honest_fp32(case)
    row, col = [int(v) for v in ref['und'].nonzero()[0]]
    d = got['d'].clone()
    width = float(ref['hi'][row, col] - ref['lo'][row, col])
    assert width > 100 * float(ref['b_env'][row, col])
    d[row, col] = d[row, col] + math.copysign(2 * width, float(d[row, col]))
    res = R.check(case, ref, {'loss': got['loss'], 'd': d})
    assert not res['d_undecided'][0] and not res['d_run_sum'][0] and res['d'][0]


# ------------------------------------------------------------------ 3. the reference against torch in float64
def _close(a, b, what):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    scale = float(b.abs().max()) if b.numel() else 0.0
    assert float((a - b).abs().max() if b.numel() else 0.0) <= 1e-12 * max(scale, 1e-300), (what, float((a - b).abs().max()), scale)


@pytest.mark.parametrize('name', [n for n in R.CASES if R.SPECS[n]['kernel'] == 'ce' and R.SPECS[n]['pattern'] != 'allignored'])
def test_cross_entropy_reference_is_torchs_in_float64(name):
    case, ref = _ref(name)
    x = case['x'].double().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(x, case['labels'], ignore_index=case['ignore'])
    (loss * R.f32(case['g'])).backward()
    _close(ref['loss'], loss.detach(), 'loss')
    _close(ref['dx'], x.grad, 'dx')


@pytest.mark.parametrize('name', [n for n in R.CASES if R.SPECS[n]['kernel'] == 'kl'])
def test_kl_reference_is_torchs_in_float64(name):
    case, ref = _ref(name)
    s = case['s'].double().requires_grad_(True)
    t = case['t'].double() if case['index'] is None else case['t'].double().index_select(0, case['index'])
    loss = torch.nn.KLDivLoss(reduction='batchmean')(torch.log_softmax(s, 1), torch.softmax(t, 1))
    (loss * R.f32(case['g'])).backward()
    _close(ref['loss'], loss.detach(), 'loss')
    _close(ref['ds'], s.grad, 'ds')


@pytest.mark.parametrize('name', [n for n in R.CASES if R.SPECS[n]['kernel'] == 'lovasz' and n not in R.TIE_CASES
                                  and R.SPECS[n]['pattern'] != 'allignored'])
def test_lovasz_reference_is_the_oracles_in_float64(name):
    from oracle import spvcnn_ref as O
    case, ref = _ref(name)
    assert ref['share'] == 0.0                          # tie-free: the oracle's own (unstable) sort has no freedom that matters
    p = case['probas'].double().requires_grad_(True)
    valid = case['labels'] != case['ignore']
    loss = O.lovasz_softmax_flat(p[valid], case['labels'][valid])
    (loss * R.f32(case['g'])).backward()
    _close(ref['loss'], loss.detach(), 'loss')
    _close(ref['d'], p.grad, 'd')
    assert float(p.grad[~valid].abs().max() if bool((~valid).any()) else 0.0) == 0.0


# ------------------------------------------------------------------ 4. every row ignored
def test_every_row_ignored():
    case, ref = _ref('ce-256x17-i255-allignored')
    x = case['x'].double().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(x, case['labels'], ignore_index=case['ignore'])
    loss.backward()
    assert math.isnan(float(loss.detach())) and float(x.grad.abs().max()) == 0.0              # torch: nan, zero gradient
    assert math.isnan(ref['loss']) and float(ref['dx'].abs().max()) == 0.0 and float(ref['b_dx'].max()) == 0.0
    got = R.honest_fp32(case)
    assert math.isnan(float(got['loss'])) and float(got['dx'].abs().max()) == 0.0
    assert all(ok for ok, _ in R.check(case, ref, got).values())
    assert not R.check(case, ref, {'loss': 0.0, 'dx': got['dx']})['loss'][0]           # a finite loss is rejected there
    case, ref = _ref('lv-256x17-i255-allignored')
    assert ref['loss'] == 0.0 and ref['b_loss'] == 0.0 and float(ref['d'].abs().max()) == 0.0 and float(ref['b_d'].max()) == 0.0
    got = R.honest_fp32(case)
    assert float(got['loss']) == 0.0 and float(got['d'].abs().max()) == 0.0


def test_a_nan_is_never_inside():
    case, ref = _ref('ce-257x2-i255')
    got = R.honest_fp32(case)
    dx = got['dx'].clone()
    dx[3, 1] = float('nan')
    res = R.check(case, ref, {'loss': float('nan'), 'dx': dx})
    assert not res['loss'][0] and not res['dx'][0]


# ------------------------------------------------------------------ 5. the package's torch formulation
@pytest.mark.parametrize('name', [n for n in R.CASES if R.SPECS[n]['kernel'] == 'lovasz'])
def test_the_torch_formulation_of_lovasz_is_inside_the_bound(name):
    """losses.lovasz_softmax_flat in fp32 on the CPU: one flat sort of a composite (class, error) key.  The saturated case holds
    errors down to 1e-45 next to errors of exactly 0 -- the key 4 c - error in float64 merged them (NOTES N27) --; torch's own
    order of summation: the depth of L3 is taken as P + C + 2."""
    from u2mkd_amd.losses import lovasz_softmax_flat
    case, _ = _ref(name)
    P, C = case['probas'].shape
    ref = R.lovasz64(case['probas'], case['labels'], case['ignore'], case['g'], depth=P + C + 2)
    p = case['probas'].clone().requires_grad_(True)
    loss = lovasz_softmax_flat(p, case['labels'], case['labels'] != case['ignore'])
    loss.backward(torch.tensor(case['g']))
    res = R.check_lovasz(ref, loss.detach(), p.grad)
    assert all(ok for ok, _ in res.values()), res
