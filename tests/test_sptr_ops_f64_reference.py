"""The float64 statement of the `sptr_cuda` operator entries (tests/sptr_ops_f64_ref.py) checked on the CPU: against the oracle
and autograd, its magnitudes and term counts by hand, the gate against the fp32 evaluation of the same statement in two pair
orders, and the gate against five corruptions it must reject.  The cases of tests/test_gpu_sptr_ops_f64.py are pinned here."""
import os
import re

import pytest
import torch

import sptr_ops_f64_ref as R
from oracle import sptr_ops_ref as O

HIP_SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'u2mkd_amd', 'csrc', 'sptr_ops.hip')

_cache = {}


def _reference(name):
    """float64 results, magnitudes and term counts of a case, once per session; nobody writes to them"""
    if name not in _cache:
        _cache[name] = R.evaluate(R.get_case(name))
    return _cache[name]


def _close(a, b, mag):
    """|a - b| <= 1e-12 mag, equality where mag is 0"""
    return bool(((a - b).abs() <= 1e-12 * mag).all())


def _rejected(name, got):
    ref, mag, terms = _reference(name)
    return {k for k in R.KINDS if bool(R.violations(k, got[k], ref[k], mag[k], terms[k]).any())}


# ---- the statement ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', R.CASE_NAMES)
def test_equals_the_oracle_in_float64(name):
    c = R.get_case(name)
    ref, mag, _ = _reference(name)
    d = lambda x: x.double()
    q, k, v, go_n, go_m, attn, tq, tk, tv = (d(x) for x in (c.q, c.k, c.v, c.go_n, c.go_m, c.attn, c.tq, c.tk, c.tv))
    q_t, k_t, v_t, tq_t, tk_t, tv_t, r_t = R.t3(q), R.t3(k), R.t3(v), R.tt(tq), R.tt(tk), R.tt(tv), c.rel.t().contiguous()
    i0o, i1o, i0, i1 = O.precompute_all(c.N, c.n, c.n_max, c.counts, c.offsets, c.sq_offsets)
    for a, b in zip((i0o, i1o, i0, i1), (c.i0o, c.i1o, c.i0, c.i1)):
        assert a.dtype == b.dtype and torch.equal(a, b)
    want = {'s1': O.attention_step1_forward(q_t, k_t, i0, i1),
            'dp': O.dot_prod_with_idx_forward(q_t, i0, k_t, i1, tq_t, tk_t, r_t),
            'dpa': O.dot_prod_with_idx_all_forward(q_t, i0, k_t, i1, tq_t, tk_t, r_t),
            's2_out': O.attention_step2_forward(attn, v, i0, i1),
            'rv_out': O.attention_step2_with_rel_pos_value_forward(attn, v, i0, i1, tv, c.rel)}
    want['s1_gq'], want['s1_gk'] = O.attention_step1_backward(go_m, i0, i1, q, k)
    want['s2_ga'], want['s2_gv'] = O.attention_step2_backward(go_n, i0, i1, attn, v_t)
    want['dp_gq'], want['dp_gk'], want['dp_gtq'], want['dp_gtk'] = O.dot_prod_with_idx_backward(go_m, q, i0, k, i1, tq, tk, c.rel)
    want['rv_ga'], want['rv_gv'], want['rv_gt'] = O.attention_step2_with_rel_pos_value_backward(go_n, i0, i1, attn, v_t, tv_t, r_t)
    assert set(want) == set(R.KINDS)
    for kind in R.KINDS:
        assert want[kind].dtype == torch.float64 and want[kind].shape == ref[kind].shape, kind
        assert _close(ref[kind], want[kind], mag[kind]), kind


@pytest.mark.parametrize('name', R.CASE_NAMES)
def test_every_backward_is_the_autograd_derivative_of_its_forward(name):
    c = R.get_case(name)
    ref, mag, _ = _reference(name)
    kw = dict(magnitudes=False)
    q, k, v, attn, tq, tk, tv = (x.double().requires_grad_(True) for x in (c.q, c.k, c.v, c.attn, c.tq, c.tk, c.tv))
    go_m, go_n = c.go_m.double(), c.go_n.double()
    r_t = c.rel.t().contiguous()

    def grads(out, grad, leaves):
        return torch.autograd.grad(out, leaves, grad)

    # the launchers' layouts are permutations of the leaves, so autograd carries the gradient back through them
    gq, gk = grads(R.attention_step1_forward(R.t3(q), R.t3(k), c.i0, c.i1, **kw)['s1'], go_m.t(), (q, k))
    assert _close(ref['s1_gq'], gq, mag['s1_gq']) and _close(ref['s1_gk'], gk, mag['s1_gk'])
    got = grads(R.dot_prod_with_idx_forward(R.t3(q), c.i0, R.t3(k), c.i1, R.tt(tq), R.tt(tk), r_t, **kw)['dp'], go_m.t(),
                (q, k, tq, tk))
    for kind, g in zip(('dp_gq', 'dp_gk', 'dp_gtq', 'dp_gtk'), got):
        assert _close(ref[kind], g, mag[kind]), kind
    got = grads(R.attention_step2_forward(attn, v, c.i0, c.i1, **kw)['s2_out'], go_n, (attn, v))
    for kind, g in zip(('s2_ga', 's2_gv'), got):
        assert _close(ref[kind], g, mag[kind]), kind
    got = grads(R.attention_step2_with_rel_pos_value_forward(attn, v, c.i0, c.i1, tv, c.rel, **kw)['rv_out'], go_n, (attn, v, tv))
    for kind, g in zip(('rv_ga', 'rv_gv', 'rv_gt'), got):
        assert _close(ref[kind], g, mag[kind]), kind


@pytest.mark.parametrize('name', R.CASE_NAMES)
def test_the_decomposition_identity_holds(name):
    """the reference's own check: dot_prod_with_idx_all == dot_prod_with_idx + attention_step1"""
    ref, mag, _ = _reference(name)
    assert _close(ref['dpa'], ref['dp'] + ref['s1'], mag['dpa'])
    assert _close(mag['dpa'], mag['dp'] + mag['s1'], mag['dpa'])


def test_cross_case_equals_the_oracle_and_has_two_token_counts():
    x = R.cross_case()
    assert (x['Nq'], x['Nk'], x['M'], x['h'], x['d']) == (37, 53, 300, 3, 16)
    assert x['q_t'].shape == (3, 16, 37) and x['k_t'].shape == (3, 16, 53)
    assert int(x['index0'].max()) < 37 <= int(x['index1'].max()) < 53          # keys past the last query: N_k is really used
    res, mag, terms = R.attention_step1_forward(x['q_t'], x['k_t'], x['index0'], x['index1'])
    assert _close(res['s1'], O.attention_step1_forward(x['q_t'].double(), x['k_t'].double(), x['index0'], x['index1']), mag['s1'])
    assert bool((terms['s1'] == 16).all())


# ---- terms and mag by hand ----------------------------------------------------------------------------------------------------

def test_terms_and_magnitudes_by_hand_on_counts_3_2_6():
    h, d, L = 2, 2, 3
    c = R.Case('hand', [3, 2, 6], h, d, L)
    assert (c.N, c.M, c.n, c.n_max) == (11, 49, 3, 6)
    assert c.i0o.tolist() == [0, 3, 6, 9, 11, 13, 19, 25, 31, 37, 43] and c.i0o_closed.tolist()[-1] == 49
    assert c.i1o.tolist() == [0, 1, 2, 9, 10, 13, 14, 15, 16, 17, 18]
    assert c.i0.tolist() == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 2 + [4] * 2 + sum(([t] * 6 for t in range(5, 11)), [])
    assert c.i1.tolist() == [0, 1, 2] * 3 + [3, 4] * 2 + list(range(5, 11)) * 6
    full = lambda x, val: torch.full_like(x, val)
    c.q, c.k, c.v = full(c.q, -1.0), full(c.k, 2.0), full(c.v, -3.0)
    c.go_m, c.go_n, c.attn = full(c.go_m, -0.5), full(c.go_n, 4.0), full(c.attn, 0.25)
    c.tq, c.tk, c.tv = full(c.tq, 0.5), full(c.tk, -0.25), full(c.tv, 1.0)
    # axis 0: every pair hits row 0; axis 1: the 13 pairs of the first two windows hit row 1, the 36 of the last row 2;
    # axis 2: pair m hits row m % 3 (17, 16 and 16 pairs)
    m = torch.arange(49)
    c.rel = torch.stack([torch.zeros(49, dtype=torch.long), torch.where(m < 13, 1, 2), m % 3], 1).int()
    res, mag, terms = R.evaluate(c)
    win = torch.tensor([3] * 3 + [2] * 2 + [6] * 6, dtype=torch.float64)[:, None, None].expand(11, h, d)
    hits = torch.tensor([[49, 0, 17], [0, 13, 16], [0, 36, 16]], dtype=torch.float64)[:, :, None, None].expand(L, 3, h, d)

    def const(kind, value, magnitude, count):
        assert bool((res[kind] == value).all()), (kind, res[kind].flatten()[0])
        assert bool((mag[kind] == magnitude).all()), (kind, mag[kind].flatten()[0])
        assert bool((terms[kind] == count).all()), (kind, terms[kind].flatten()[0])

    const('s1', -4.0, 4.0, 2)                                       # d = 2 products of -1 * 2
    const('dp', -6.0, 6.0, 4)                                       # 2 (-1 * 1.5 + 2 * -0.75)
    const('dpa', -10.0, 10.0, 6)                                    # 2 (-1 * (2 + 1.5) + 2 * -0.75)
    const('s2_ga', -24.0, 24.0, 2)                                  # 2 (4 * -3)
    const('rv_ga', 0.0, 48.0, 4)                                    # 2 (4 * (3 - 3)): cancels, magnitude 2 * 4 * (3 + 3)
    for kind, per_pair, per_pair_mag in (('s1_gq', -1.0, 1.0), ('s1_gk', 0.5, 0.5), ('s2_out', -0.75, 0.75), ('s2_gv', 1.0, 1.0),
                                         ('dp_gq', -0.75, 0.75), ('dp_gk', 0.375, 0.375), ('rv_out', 0.0, 1.5), ('rv_gv', 1.0, 1.0)):
        const(kind, per_pair * win, per_pair_mag * win, win)        # L_w equal pairs per token
    for kind, per_hit in (('dp_gtq', 0.5), ('dp_gtk', -1.0), ('rv_gt', 1.0)):
        const(kind, per_hit * hits, abs(per_hit) * hits, hits)
    # the bound: zero where nothing is added, c = terms + r_kind elsewhere
    b = R.bound('dp_gtq', mag['dp_gtq'], terms['dp_gtq'])
    assert float(b[1, 0, 0, 0]) == 0.0 and float(b[0, 0, 0, 0]) == 50 * R.U / (1 - 50 * R.U) * 24.5
    assert float(R.bound('rv_out', mag['rv_out'], terms['rv_out'])[3, 0, 0]) == 6 * R.U / (1 - 6 * R.U) * 3.0
    assert float(R.bound('dpa', mag['dpa'], terms['dpa'])[0, 0]) == 10 * R.U / (1 - 10 * R.U) * 10.0
    assert R.U == 2.0 ** -24 and max(R.R_KIND.values()) <= 6 and set(R.R_KIND) == set(R.KINDS) and len(R.KINDS) == 16


def test_worst_and_violations_treat_a_zero_bound_as_equality():
    ref, mag, terms = torch.zeros(3, dtype=torch.float64), torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64), torch.ones(3)
    ok = torch.zeros(3)
    assert not bool(R.violations('s1', ok, ref, mag, terms).any()) and R.worst('s1', ok, ref, mag, terms) == 0.0
    bad = torch.tensor([0.0, 1e-30, 0.0])
    assert R.violations('s1', bad, ref, mag, terms).tolist() == [False, True, False]
    assert R.worst('s1', bad, ref, mag, terms) == float('inf')
    nan = torch.tensor([0.0, 0.0, float('nan')])
    assert R.violations('s1', nan, ref, mag, terms).tolist() == [False, False, True]
    assert R.worst('s1', nan, ref, mag, terms) == float('inf')
    edge = torch.tensor([0.0, 0.0, 2 * R.U / (1 - 2 * R.U)], dtype=torch.float64)
    assert not bool(R.violations('s1', edge, ref, mag, terms).any()) and R.worst('s1', edge, ref, mag, terms) == 1.0


# ---- the cases ----------------------------------------------------------------------------------------------------------------

def test_the_cases_are_those_of_the_issue():
    assert R.CASE_NAMES == ('tails', 'wide', 'straddle', 'one-entry', 'ceiling', 'under')
    tails = (1, 2, 63, 64, 65, 257, 3, 1, 30)
    want = {'tails': (tails, 3, 16, 7), 'wide': ((5, 90, 1, 33, 2, 17), 5, 64, 13), 'straddle': (tails, 7, 24, 31),
            'one-entry': (tails, 7, 24, 31), 'ceiling': ((3, 1, 40, 9), 2, 64, 50), 'under': ((3, 1, 40, 9), 2, 64, 42)}
    for name in R.CASE_NAMES:
        c = R.get_case(name)
        assert (tuple(c.counts.tolist()), c.h, c.d, c.L) == want[name], name
        assert c.N == sum(want[name][0]) and c.M == sum(x * x for x in want[name][0])
        assert c.d <= R.HDIM_MAX and c.L <= R.L_MAX
        assert int(c.rel.min()) >= 0 and int(c.rel.max()) < c.L and c.rel.shape == (c.M, 3)
        assert float(c.attn.min()) >= 0.0 and float(c.attn.max()) < 1.0
        assert bool((c.rel == 0).all()) == (name == 'one-entry')
    for name in ('tails', 'straddle', 'one-entry'):
        c = R.get_case(name)
        assert (c.N, c.M) == (486, 79254)
        assert c.N % R.K_GT_TOK != 0 and c.M % R.K_OP_THREADS != 0          # both tails run
        assert {1, 64, 65, 257} <= set(c.counts.tolist()) and c.n_max > R.K_OP_THREADS
        assert (c.n_max ** 2 + R.K_OP_THREADS * 8 - 1) // (R.K_OP_THREADS * 8) > 1     # precompute_all: gridDim.y > 1
    assert R.get_case('ceiling').N == 53 == R.get_case('under').N                  # no multiple of kGtTok either
    C = {name: R.get_case(name).h * R.get_case(name).d for name in R.CASE_NAMES}
    assert (C['tails'], C['wide'], C['straddle'], C['one-entry']) == (48, 320, 168, 168)
    assert C['tails'] < R.K_GT_CW                                            # a partial channel slice only
    assert C['wide'] > R.K_OP_THREADS and C['wide'] == 5 * R.K_GT_CW         # blockIdx.y = 1 of the token kernels; five slices
    assert C['straddle'] == 2 * R.K_GT_CW + 40 and R.K_GT_CW % 24 != 0       # slices 64, 64, 40; heads cross their borders
    # one-entry: the straddle case with every pair on row 0; all other rows are never hit
    s, o = R.get_case('straddle'), R.get_case('one-entry')
    assert torch.equal(s.counts, o.counts)
    _, _, terms = _reference('one-entry')
    for kind in R.TABLE_GRADS:
        assert bool((terms[kind][0] == 79254).all()) and bool((terms[kind][1:] == 0).all())
    # the fp32 operands are exactly representable inputs of the float64 statement: nothing is rounded on the way in
    assert all(getattr(s, x).dtype == torch.float32 for x in ('q', 'k', 'v', 'go_n', 'go_m', 'attn', 'tq', 'tk', 'tv'))


def test_the_lds_byte_counts_are_those_of_the_source():
    ceiling, under = R.get_case('ceiling'), R.get_case('under')
    assert R.scores_lds_bytes(ceiling.d, ceiling.L) == 76800 == 24 * 64 * 50
    assert R.dot_prod_backward_lds_bytes(ceiling.L) == 76800 == 1536 * 50
    assert R.scores_lds_bytes(under.d, under.L) == 64512 == R.dot_prod_backward_lds_bytes(under.L)
    assert R.dot_prod_backward_lds_bytes(42) <= 65536 < R.dot_prod_backward_lds_bytes(43)       # L = 42: the last under 64 KiB
    assert (ceiling.d, ceiling.L) == (R.HDIM_MAX, R.L_MAX)
    src = open(HIP_SOURCE).read()
    flat = re.sub(r'\s+', ' ', src)
    assert 'constexpr int kOpThreads = %d;' % R.K_OP_THREADS in flat
    assert 'constexpr int kGtTok = %d;' % R.K_GT_TOK in flat and 'constexpr int kGtCW = %d;' % R.K_GT_CW in flat
    assert 'hdim <= %d' % R.HDIM_MAX in flat and 'L <= %d' % R.L_MAX in flat
    # the launch sizes: both score forms, and the dot-prod backward
    assert flat.count('kOpThreads, 2 * hdim * 3 * L * sizeof(float)') == 2
    assert flat.count('kGtTok * kGtCW, 2 * 3 * L * kGtCW * sizeof(float)') == 1


# ---- the gate against the fp32 evaluation of the statement --------------------------------------------------------------------

def test_fp32_evaluation_sits_inside_the_gate_in_two_orders():
    """worst err / bound per kind over the six cases, pairs summed in ascending m and in a fixed random permutation of m; the
    figures printed here are the table in the helper's docstring"""
    worst = {'ascending': dict.fromkeys(R.KINDS, 0.0), 'permuted': dict.fromkeys(R.KINDS, 0.0)}
    for name in R.CASE_NAMES:
        c = R.get_case(name)
        ref, mag, terms = _reference(name)
        perm = torch.randperm(c.M, generator=torch.Generator().manual_seed(5))
        for order, pairs in (('ascending', None), ('permuted', perm)):
            got = R.evaluate(c, dtype=torch.float32, magnitudes=False, pairs=pairs)
            for kind in R.KINDS:
                assert got[kind].dtype == torch.float32
                w = R.worst(kind, got[kind], ref[kind], mag[kind], terms[kind])
                worst[order][kind] = max(worst[order][kind], w)
                assert not bool(R.violations(kind, got[kind], ref[kind], mag[kind], terms[kind]).any()), (name, order, kind, w)
    print()
    for kind in R.KINDS:
        print('%-7s ascending %.3f  permuted %.3f' % (kind, worst['ascending'][kind], worst['permuted'][kind]))
    for order in worst:
        assert all(0.0 < w <= 1.0 for w in worst[order].values()), worst[order]           # and fp32 is really what ran


# ---- corruptions the gate must reject, applied to the fp32 evaluation -----------------------------------------------------------

CORRUPTED = ('tails', 'straddle')


@pytest.mark.parametrize('name', CORRUPTED)
def test_gate_rejects_the_last_pair_of_every_window_dropped(name):
    c = R.get_case(name)
    keep = torch.ones(c.M, dtype=torch.bool)
    keep[c.sq_offsets[1:].long() - 1] = False
    assert int((~keep).sum()) == c.n
    got = R.evaluate(c, dtype=torch.float32, magnitudes=False, pairs=torch.nonzero(keep)[:, 0])
    # every plain-store output notices.  A table-gradient entry of `tails` sums ~11,000 products, and one product fewer is
    # inside the rounding bound of such a sum: no elementwise bound on an fp32 sum can see it there.
    assert set(R.PLAIN_STORES) <= _rejected(name, got)


@pytest.mark.parametrize('name', CORRUPTED)
def test_gate_rejects_a_key_side_walk_of_stride_one(name):
    """m = sk + i where m = sk + i n belongs: the pairs of the NEXT queries' first keys"""
    c = R.get_case(name)
    n_of = torch.repeat_interleave(c.counts.long(), c.counts.long())                       # window length of every token
    tok = torch.repeat_interleave(torch.arange(c.N), n_of)
    step = torch.arange(len(tok)) - torch.repeat_interleave(torch.cumsum(n_of, 0) - n_of, n_of)
    right = c.i1o.long()[tok] + step * n_of[tok]
    assert torch.equal(torch.sort(right)[0], torch.arange(c.M)) and torch.equal(c.i1.long()[right], tok)   # the right walk
    wrong = c.i1o.long()[tok] + step
    assert int(wrong.max()) < c.M
    got = R.evaluate(c, dtype=torch.float32, magnitudes=False, walk_k=(tok, wrong))
    key_side = {'s1_gk', 's2_gv', 'dp_gk', 'dp_gtk', 'rv_gv', 'rv_gt'}
    assert _rejected(name, got) == key_side
    same = R.evaluate(c, dtype=torch.float32, magnitudes=False, walk_k=(tok, right))       # the hook itself changes nothing
    assert _rejected(name, same) == set()


@pytest.mark.parametrize('name', CORRUPTED)
def test_gate_rejects_rel_axes_1_and_2_swapped(name):
    c = R.get_case(name)
    got = R.evaluate(c, dtype=torch.float32, magnitudes=False, rel=c.rel[:, [0, 2, 1]].contiguous())
    assert _rejected(name, got) == {'dp', 'dpa', 'dp_gq', 'dp_gk', 'dp_gtq', 'dp_gtk', 'rv_out', 'rv_ga', 'rv_gt'}


@pytest.mark.parametrize('name', CORRUPTED)
def test_gate_rejects_the_next_head_for_the_channels_of_one_slice(name):
    """hh = (c / d + 1) mod h for the channels of the last 64-wide slice (the only one of `tails`, the 40-wide one of `straddle`)"""
    c = R.get_case(name)
    C = c.h * c.d
    hc = torch.arange(C) // c.d
    first = (C - 1) // R.K_GT_CW * R.K_GT_CW
    hc[first:] = (hc[first:] + 1) % c.h
    got = R.evaluate(c, dtype=torch.float32, magnitudes=False, head_of_channel=hc)
    assert _rejected(name, got) == set(R.PER_TOKEN) | set(R.TABLE_GRADS)
    ref, mag, terms = _reference(name)
    for kind in R.PER_TOKEN:                                                # and only that slice's channels
        bad = R.violations(kind, got[kind], ref[kind], mag[kind], terms[kind]).view(c.N, C)
        assert not bool(bad[:, :first].any()) and bool(bad[:, first:].any()), kind


def test_gate_rejects_1e_minus_6_in_a_table_row_no_pair_hits():
    """(`tails` and `straddle` hit every row; `one-entry` is `straddle` with rows 1.. never hit)"""
    name = 'one-entry'
    c = R.get_case(name)
    got = R.evaluate(c, dtype=torch.float32, magnitudes=False)
    assert _rejected(name, got) == set()
    for kind in R.TABLE_GRADS:
        x = dict(got)
        x[kind] = got[kind].clone()
        assert float(x[kind][c.L - 1, 2, c.h - 1, c.d - 1]) == 0.0
        x[kind][c.L - 1, 2, c.h - 1, c.d - 1] = 1e-6
        assert _rejected(name, x) == {kind}
