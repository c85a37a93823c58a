"""The float64 reference of the table-free window attention (tests/sptr_plain_f64_ref.py) checked on the CPU: its explicit
gradient formulas against autograd, the whole statement against tests/sptr_f64_ref.py with all-zero tables, the coefficients of
the GPU gate against the fp32 evaluation of the same formulation, and the gate itself against three corruptions it must
reject."""
import numpy as np
import pytest
import torch

import sptr_f64_ref as R
import sptr_plain_f64_ref as P

GRADS = ('dq', 'dk', 'dv')


def test_explicit_gradients_equal_autograd_through_a_dense_float64_softmax():
    case = R.Case(4, False, h=3, lens=[1, 2, 65, 5, 17, 33, 9, 3, 1, 40])
    qs = 0.25
    ref, mag, _ = P.reference(case, qs)
    q, k, v = (t.double().requires_grad_(True) for t in (case.q, case.k, case.v))
    out = torch.zeros_like(q)
    lse = torch.zeros(case.n, case.h, dtype=torch.float64)
    order = torch.as_tensor(case.sort_idx, dtype=torch.int64)
    starts = np.concatenate([[0], np.cumsum(case.window_lengths)])
    rows = []
    for a, b in zip(starts[:-1], starts[1:]):                      # an independent statement: torch.softmax per window
        tok = order[a:b]
        s = torch.einsum('ihd,jhd->hij', q[tok] * qs, k[tok])
        rows.append((tok, torch.einsum('hij,jhd->ihd', torch.softmax(s, -1), v[tok])))
        lse[a:b] = torch.logsumexp(s.detach(), -1).T
    out = torch.zeros_like(q).index_add(0, torch.cat([t for t, _ in rows]), torch.cat([o for _, o in rows]))
    assert not bool(P.violations('out', out.detach(), ref['out'], mag['out'], kappa=1e-12).any())
    assert not bool(P.violations('lse', lse, ref['lse'], mag['lse'], kappa=1e-12).any())
    out.backward(case.dout.double())
    for kind, leaf in zip(GRADS, (q, k, v)):
        assert not bool(P.violations(kind, leaf.grad, ref[kind], mag[kind], kappa=1e-12).any()), kind


def test_equals_the_contextual_reference_with_all_zero_tables():
    case = R.Case(2, False, h=2, lens=[3, 1, 37, 8, 2, 64])
    case.tq, case.tk, case.tv = (torch.zeros_like(t) for t in (case.tq, case.tk, case.tv))
    want, wmag, wabs = R.reference(case)
    got, mag, mag_abs = P.reference(case, case.q_scale)
    for kind in P.KINDS:
        assert torch.equal(got[kind], want[kind]), kind
        assert torch.equal(mag[kind], wmag[kind]) and torch.equal(mag_abs[kind], wabs[kind]), kind


def test_the_gpu_cases_are_those_of_the_issue():
    cases = P.gpu_cases()
    assert len(cases) == 10 and len(set(cases)) == 10
    assert {c[0] for c in cases} == set(R.SPLITS) and {c[2] for c in cases} == {0.25, 1.0}
    assert all(h == (3 if S == 4 else 2) for S, h, _ in cases)
    for S, h, _ in cases:
        case = P.get_case(S, h)
        lens = set(case.window_lengths.tolist())
        assert {1, S, S + 1, 2 * S + 1, 3 * S - 1, 37, 64, 65, 129, 385} | ({S - 1} if S > 1 else set()) <= lens
        tpb = 128 // S
        assert case.n % tpb != 0 and 1100 <= case.n <= 8400            # no multiple of the tokens per workgroup
        if S > 1:
            assert case.n > 128 * tpb                                   # past one pass of a 128-workgroup grid


def test_kappa_is_eight_rho_of_the_fp32_evaluation():
    """rho per kind over every case of the GPU file: this formulation in fp32 against float64, never a kernel."""
    rho = {k: 0.0 for k in P.KINDS}
    rho_abs = dict(rho)
    for S, h, qs in P.gpu_cases():
        case = P.get_case(S, h)
        ref, mag, mag_abs = P.reference(case, qs)
        r32 = P.reference(case, qs, dtype=torch.float32, magnitudes=False)
        for k in P.KINDS:
            rho[k] = max(rho[k], P.worst(k, r32[k], ref[k], mag[k]))
            rho_abs[k] = max(rho_abs[k], P.worst(k, r32[k], ref[k], mag_abs[k]))
    print('rho    ', {k: '%.3g' % v for k, v in rho.items()})
    print('rho_abs', {k: '%.3g' % v for k, v in rho_abs.items()})
    for got, rec, kap in ((rho, P.RHO, P.KAPPA), (rho_abs, P.RHO_ABS, P.KAPPA_ABS)):
        for k in P.KINDS:
            assert rec[k] / 2 <= got[k] <= rec[k] * 2, (k, got[k], rec[k])
            assert kap[k] == R.pow2_ceil(8 * rec[k]) and 8 * rec[k] <= kap[k] < 16 * rec[k]


def _rejected(ref, mags, got):
    mag, mag_abs = mags
    a = {k for k in P.KINDS if bool(P.violations(k, got[k], ref[k], mag[k]).any())}
    b = {k for k in P.KINDS if bool(P.violations(k, got[k], ref[k], mag_abs[k], kappa=P.KAPPA_ABS[k]).any())}
    return a, b


@pytest.fixture(scope='module')
def checked():
    case = P.get_case(16, 2)
    ref, mag, mag_abs = P.reference(case, 0.25)
    assert _rejected(ref, (mag, mag_abs), ref) == (set(), set())              # the reference itself passes
    return case, ref, (mag, mag_abs)


def _window(case, length):
    w = int(np.flatnonzero(case.window_lengths == length)[0])
    return w, np.flatnonzero(case.window_of == w)


@pytest.mark.parametrize('length', [385, 17, 2])
def test_gate_rejects_one_dropped_pair(checked, length):
    """ONE (query, key) pair missing: the last key of the window for its first query."""
    case, ref, mags = checked
    _, pos = _window(case, length)
    keep = ~((case.i0 == pos[0]) & (case.i1 == pos[-1]))
    assert (~keep).sum() == 1
    got = P.reference(case, 0.25, i0=case.i0[keep], i1=case.i1[keep], magnitudes=False)
    a, b = _rejected(ref, mags, got)
    assert a and b, (a, b)
    assert {'out', 'lse'} <= a | b, (a, b)


@pytest.mark.parametrize('length', [37, 3])
def test_gate_rejects_a_key_taken_from_the_neighbouring_window(checked, length):
    """one pair reads the first token of the NEXT window where the last key of its own belongs (a walk one position too far)"""
    case, ref, mags = checked
    _, pos = _window(case, length)
    assert pos[-1] + 1 < case.n
    i1 = case.i1.copy()
    m = int(np.flatnonzero((case.i0 == pos[1]) & (case.i1 == pos[-1]))[0])
    i1[m] = pos[-1] + 1
    got = P.reference(case, 0.25, i1=i1, magnitudes=False)
    a, b = _rejected(ref, mags, got)
    assert a and b, (a, b)
    assert {'dk', 'dv'} <= a | b, (a, b)


def test_gate_rejects_q_scale_off_by_2_to_minus_10(checked):
    case, ref, mags = checked
    got = P.reference(case, 0.25 * (1 + 2.0 ** -10), magnitudes=False)
    a, b = _rejected(ref, mags, got)
    assert a and b, (a, b)
    assert 'dq' in a and 'dq' in b, (a, b)
