"""The float64 reference of the window attention (tests/sptr_f64_ref.py) checked on the CPU: its explicit gradient
formulas against autograd, its rows and outputs against oracle.sptr_ref on coordinate scenes, the coefficients of the GPU
gate against the fp32 evaluation of the same formulation, and the gate itself against four corruptions it must reject."""
import numpy as np
import pytest
import torch

import sptr_f64_ref as R
from oracle import sptr_ref as S

GRADS = ('dq', 'dk', 'dv', 'dTq', 'dTk', 'dTv')


@pytest.mark.parametrize('sphere', [False, True], ids=['cubic', 'sphere'])
def test_explicit_gradients_equal_autograd_through_the_float64_forward(sphere):
    case = R.Case(4, sphere, h=3, lens=[1, 2, 65, 5, 17, 33, 9, 3, 1, 40])
    ref, mag, _ = R.reference(case)
    leaves = [t.double().requires_grad_(True) for t in (case.q, case.k, case.v, case.tq, case.tk, case.tv)]
    ix = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.int64)
    out, lse, _ = R.forward(*leaves, ix(case.sort_idx), ix(case.i0), ix(case.i1), ix(case.rows), case.q_scale)
    assert torch.equal(out.detach(), ref['out']) and torch.equal(lse.detach(), ref['lse'])
    out.backward(case.dout.double())
    for kind, leaf in zip(GRADS, leaves):
        bad = R.violations(kind, leaf.grad, ref[kind], mag[kind], kappa=1e-12)
        assert not bool(bad.any()), (kind, R.worst(kind, leaf.grad, ref[kind], mag[kind]))


def _scene(sphere, n, seed):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(n, 3, generator=g) * torch.tensor([8.0, 8.0, 2.0])
    batch = torch.sort(torch.randint(0, 2, (n,), generator=g))[0]
    if sphere:
        xyz = S.cart2sphere(xyz - torch.tensor([4.0, 4.0, 1.0]))
    return xyz, batch, g


@pytest.mark.parametrize('sphere,window,quant', [(False, [2.4, 2.4, 2.4], [0.1, 0.1, 0.1]),
                                                 (True, [16.0, 16.0, 120.0], [16 / 24, 16 / 24, 5.0])],
                         ids=['cubic', 'sphere'])
def test_rows_and_outputs_equal_the_oracle_on_a_coordinate_scene(sphere, window, quant):
    n, h, qgl = 160, 2, 24
    a = R.SPLIT_A if sphere else None
    L = 2 * qgl if sphere else 2 * qgl - 1
    xyz, batch, g = _scene(sphere, n, 4)
    window, quant = np.array(window), np.array(quant)
    i0, i0o, n_max, i1, i1o, sort_idx = S.get_indices_params(xyz, batch, window)
    case = R.Case.__new__(R.Case)                 # the plan the kernels would be given, from the oracle's window partition
    counts = (i0o[1:] - i0o[:-1]).numpy()         # window length of every sorted position
    xs = xyz[sort_idx]
    case.sort_idx = sort_idx.numpy().astype(np.int32)
    case.wlen = counts.astype(np.int32)
    case.wstart = (i1[i0o[:-1]]).numpy().astype(np.int32)     # the first key of a query's pairs = its window's first position
    wq = torch.as_tensor(window).float()
    case.qc = torch.div((xs - xs.min(0)[0] + 0.0) % wq, torch.as_tensor(quant).float(), rounding_mode='floor').int().numpy()
    case.radial = xs[:, 2].numpy() if sphere else None
    case.i0, case.i1 = R.pair_lists(case.wstart, case.wlen)
    assert np.array_equal(case.i0, i0.numpy()) and np.array_equal(case.i1, i1.numpy())       # precompute_all's lists
    if sphere:
        assert not R.near_edge(case.radial, case.i0, case.i1, R.SPLIT_A).any()      # (this scene: no pair on a bin edge)
    case.rows = R.rel_rows(case.qc, case.radial, case.i0, case.i1, qgl, a or 0.0)
    want = S.relative_position_index(xs, i0, i1, window, quant, qgl, a)
    assert np.array_equal(case.rows, want.numpy())
    assert case.rows.min() >= 0 and case.rows.max() < L and len(np.unique(case.rows[:, 2])) > 3
    case.q, case.k, case.v, case.dout = (torch.randn(n, h, 16, generator=g) for _ in range(4))
    case.tq, case.tk, case.tv = (0.3 * torch.randn(L, 3, h, 16, generator=g) for _ in range(3))
    case.q_scale = 0.25
    ref, mag, _ = R.reference(case)
    leaves = [t.double().requires_grad_(True) for t in (case.q, case.k, case.v, case.tq, case.tk, case.tv)]
    out = S.sparse_self_attention(leaves[0] * case.q_scale, leaves[1], leaves[2], xyz, i0, i0o, n_max, i1, i1o, sort_idx,
                                  window, quant, qgl, *leaves[3:], a)
    assert out.dtype == torch.float64
    out.backward(case.dout.double())
    assert not bool(R.violations('out', out.detach(), ref['out'], mag['out'], kappa=1e-12).any())
    for kind, leaf in zip(GRADS, leaves):
        assert not bool(R.violations(kind, leaf.grad, ref[kind], mag[kind], kappa=1e-12).any()), kind


def _inputs():
    return sorted({(S_, sphere, h, big) for S_, sphere, _, h, big in R.gpu_cases()})


def test_the_gpu_cases_are_the_twenty_of_the_issue_and_no_pair_is_near_a_bin_edge():
    cases = R.gpu_cases()
    assert len(cases) == 20 and len(set(cases)) == 20
    assert sum(1 for c in cases if not c[4]) == 18 and sum(1 for c in cases if not c[2]) == 8
    for sphere in (False, True):
        assert sum(1 for c in cases if c[1] == sphere and c[3] == 3) == 1
    for key in _inputs():
        S_, sphere, h, big = key
        case = R.get_case(*key)                                      # (raises if the radial redraw does not terminate)
        lens = set(case.window_lengths.tolist())
        if big:
            assert case.n == 66000 and 129 in lens and lens <= set(range(1, 10)) | {129}
            assert -(-case.n // 128) > 512 and case.n % 128                 # the 512-workgroup grid takes a second pass
        else:
            want = {1, S_, S_ + 1, 2 * S_ + 1, 3 * S_ - 1, 37, 64, 65, 129, 385} | ({S_ - 1} if S_ > 1 else set())
            assert want <= lens
            tpb = 128 // S_
            assert case.n % tpb != 0 and 1100 <= case.n <= 8400
            if S_ > 1:
                assert 128 * tpb < case.n < 128 * tpb + 128                 # just past one pass of the 128-workgroup grid
            # workgroup boundaries fall inside windows, large ones included
            inside = [b for b in range(tpb, case.n, tpb) if case.wstart[b] != b]
            assert len(inside) > case.n // tpb // 2 and any(case.wlen[b] >= 37 for b in inside)
        assert sorted(case.sort_idx.tolist()) == list(range(case.n))
        assert case.qc.min() == 0 and case.qc.max() == case.qc_span - 1
        assert case.rows.min() == 0 and case.rows.max() == (47 if sphere else 46)
        if sphere:
            assert case.edge_slack() > 1.0
            assert {0, 47} <= set(np.unique(case.rows[:, 2]).tolist())      # both clamp ends of the radial split
            assert len(np.unique(case.rows[:, 2])) >= 40


def test_kappa_is_eight_rho_of_the_fp32_evaluation():
    """rho per kind over every case of the GPU file: this formulation in fp32 against float64, never a kernel."""
    rho = {k: 0.0 for k in R.KINDS}
    rho_abs = dict(rho)
    for key in _inputs():
        case = R.get_case(*key)
        ref, mag, mag_abs = R.reference(case)
        r32 = R.reference(case, dtype=torch.float32, magnitudes=False)
        for k in R.KINDS:
            rho[k] = max(rho[k], R.worst(k, r32[k], ref[k], mag[k]))
            rho_abs[k] = max(rho_abs[k], R.worst(k, r32[k], ref[k], mag_abs[k]))
    print('rho    ', {k: '%.3g' % v for k, v in rho.items()})
    print('rho_abs', {k: '%.3g' % v for k, v in rho_abs.items()})
    for got, rec, kap in ((rho, R.RHO, R.KAPPA), (rho_abs, R.RHO_ABS, R.KAPPA_ABS)):
        for k in R.KINDS:
            assert rec[k] / 2 <= got[k] <= rec[k] * 2, (k, got[k], rec[k])
            assert kap[k] == R.pow2_ceil(8 * rec[k]) and 8 * rec[k] <= kap[k] < 16 * rec[k]


def _rejected(case, ref, mags, got):
    """({kind} rejected by the factor magnitudes with KAPPA, {kind} rejected by the term-wise ones with KAPPA_ABS); the GPU
    gate asserts both lines, so a corruption is rejected when either set is non-empty."""
    mag, mag_abs = mags
    a = {k for k in R.KINDS if bool(R.violations(k, got[k], ref[k], mag[k]).any())}
    b = {k for k in R.KINDS if bool(R.violations(k, got[k], ref[k], mag_abs[k], kappa=R.KAPPA_ABS[k]).any())}
    return a, b


@pytest.fixture(scope='module', params=[False, True], ids=['cubic', 'sphere'])
def checked(request):
    case = R.get_case(16, request.param)
    ref, mag, mag_abs = R.reference(case)
    assert _rejected(case, ref, (mag, mag_abs), ref) == (set(), set())        # the reference itself passes
    return case, ref, (mag, mag_abs)


def _window(case, length):
    w = int(np.flatnonzero(case.window_lengths == length)[0])
    return np.flatnonzero(case.window_of == w)


@pytest.mark.parametrize('length', [385, 17, 2])
def test_gate_rejects_the_last_key_of_a_window_dropped(checked, length):
    case, ref, mags = checked
    pos = _window(case, length)
    keep = ~((case.i1 == pos[-1]) & np.isin(case.i0, pos))
    assert (~keep).sum() == length
    got = R.reference(case, i0=case.i0[keep], i1=case.i1[keep], rows=case.rows[keep], magnitudes=False)
    a, b = _rejected(case, ref, mags, got)
    assert {'dk', 'dv'} <= a and {'out', 'dq', 'dk', 'dv'} <= b, (a, b)


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_gate_rejects_one_pair_whose_row_moved_by_one(checked, axis):
    case, ref, mags = checked
    pos = _window(case, 37)
    m = int(np.flatnonzero((case.i0 == pos[3]) & (case.i1 == pos[20]))[0])
    rows = case.rows.copy()
    rows[m, axis] += 1 if rows[m, axis] < case.L - 1 else -1
    got = R.reference(case, rows=rows, magnitudes=False)
    a, b = _rejected(case, ref, mags, got)
    assert a & {'dTq', 'dTk', 'dTv'} and {'dTq', 'dTk', 'dTv'} <= b, (a, b)


def test_gate_rejects_one_token_dq_scaled_by_one_plus_2_to_minus_10(checked):
    case, ref, mags = checked
    got = {k: v.clone() for k, v in ref.items()}
    t = int(case.sort_idx[_window(case, 37)[5]])
    got['dq'][t] *= 1 + 2.0 ** -10
    a, b = _rejected(case, ref, mags, got)
    # The factor magnitudes cannot reject this one: their coefficient for dq is 2^-9 (set by the few elements where k + Tq
    # cancels), above 2^-10 times |dq| <= magnitude.  This corruption is why the gate has the term-wise line.
    assert a == set() and b == {'dq'}, (a, b)


@pytest.mark.parametrize('kind', ['dTq', 'dTk', 'dTv'])
def test_gate_rejects_one_table_row_gradient_zeroed(checked, kind):
    """(the row of axis 0 that the FEWEST pairs reach: the one a whole-tensor maximum would not see)"""
    case, ref, mags = checked
    counts = np.bincount(case.rows[:, 0], minlength=case.L)
    r = int(np.argmin(np.where(counts > 0, counts, counts.max() + 1)))
    got = {k: v.clone() for k, v in ref.items()}
    got[kind][r, 0] = 0
    a, b = _rejected(case, ref, mags, got)
    assert a == {kind} and b == {kind}, (a, b, r, counts[r])
