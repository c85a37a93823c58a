"""The 'f32' bound of tests/conv_fwd_f64_ref.py on the CPU, on the inputs of tests/test_gpu_conv_lk_f64.py (every case of
conv_lk_tables.CASES): the tables reach the edges they claim; the honest fp32 evaluation with ONE RUNNING accumulator per element
through every offset and channel (the structure of conv_lk_kernel, which keeps conv_os2's registers), offsets ascending and
descending, stays at or below HALF the bound whose r is measured on the ascending one; and every wrong evaluation of a walk in
chunks of 32 offsets exceeds the bound on EVERY case it applies to -- no case is skipped:

    the last chunk dropped;  offset 32 dropped;  kflip mirrored inside each 32-offset chunk instead of over K ('flip' cases);
    the weights of chunk c taken from chunk c - 1;  the last live pair of the table skipped.

What does not apply, by construction: K = 32 has one chunk (no offset 32, no chunk before it, and mirroring inside the chunk is
mirroring over the volume); the in-chunk mirror differs from the true one on the 'flip' role only."""
import functools
import math

import pytest
import torch

import conv_fwd_f64_ref as R
import conv_lk_tables as T


def _lg(v):
    return math.log2(v) if v > 0 else float('-inf')


@functools.lru_cache(maxsize=None)
def _case(case):
    c = T.make_case(case)
    ref, mag, part = R.reference(c['x'], c['w'], c['nbr'], c['n_in'], c['role'])
    r = R.rel_err(R.honest_fp32(c['x'], c['w'], c['nbr'], c['n_in'], c['role'], running=True), ref, mag)
    return c, ref, mag, r


_IDS = ['%s-%s-%dx%d-%s' % c for c in T.CASES]


# ---- the tables --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(T.TABLES))
def test_tables_are_injective_in_range_and_placed_as_named(name):
    k_total, n_in, n_out, placement = T.TABLES[name]
    nbr, n_in_ = T.make_table(name)
    assert nbr.shape == (k_total, n_out) and nbr.dtype == torch.int32 and n_in_ == n_in
    assert int(nbr.min()) >= -1 and int(nbr.max()) < n_in
    assert torch.equal(nbr, T.make_table(name)[0])
    for k in range(k_total):
        live = nbr[k][nbr[k] >= 0]
        assert len(torch.unique(live)) == len(live), (name, k)
    per_offset = (nbr >= 0).sum(dim=1)
    chunks = [int(per_offset[c0:c0 + T.CHUNK].sum()) for c0 in range(0, k_total, T.CHUNK)]
    assert len(chunks) == T.n_chunks(k_total)
    assert int(per_offset[k_total - 1]) > 0 and chunks[-1] > 0
    if k_total > T.CHUNK:
        assert int(per_offset[T.CHUNK]) > 0                                   # offset 32 is there to be dropped
    if placement == 'last':
        assert len(chunks) > 1 and all(c == 0 for c in chunks[:-1])
    elif placement == 'gap':
        assert len(chunks) >= 4 and chunks[2] == 0 and all(c > 0 for i, c in enumerate(chunks) if i != 2)
    else:
        assert all(c > 0 for c in chunks)
    per_row = (nbr >= 0).sum(dim=0)
    if n_out > 3:
        assert int((per_row == 0).sum()) >= 1                                 # rows without a neighbour at all
    if placement == 'deadblock':
        assert int(per_row[16:32].sum()) == 0 and int(per_row[:16].sum()) > 0 and int(per_row[32:48].sum()) > 0
    inv = T.invert(nbr, n_in)
    assert inv.shape == (k_total, n_in) and int((inv >= 0).sum()) == int((nbr >= 0).sum())
    k, j = [int(v) for v in torch.nonzero(nbr >= 0)[-1]]
    assert int(inv[k, int(nbr[k, j])]) == j


def test_the_cases_cover_every_volume_tail_role_width_and_spread():
    ks = {T.TABLES[c[0]][0] for c in T.CASES}
    assert ks == {32, 33, 63, 64, 65, 125, 129, 343}
    assert {T.TABLES[c[0]][2] for c in T.CASES} == set(R.TAILS)
    assert {T.TABLES[c[0]][3] for c in T.CASES} == {'dense', 'last', 'gap', 'deadblock'}
    assert {c[1] for c in T.CASES} == set(R.ROLES)
    assert {c[2] for c in T.CASES} == {4, 20, 32, 96} and {c[3] for c in T.CASES} == {4, 24, 32, 48, 96}
    assert {c[4] for c in T.CASES} == set(R.SPREADS)
    assert {c[0] for c in T.CASES} == set(T.TABLES)
    for name, role, ca, cb, spread in T.CASES:
        assert role in ('fwd', 'fwdT') or (role == 'flip') == (name in T.SQUARE)       # the inverse roles: n_in != n_out
    assert any(T.TABLES[c[0]][1] != T.TABLES[c[0]][2] for c in T.CASES if c[1] in ('inv', 'invT'))


# ---- honest evaluations --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', T.CASES, ids=_IDS)
def test_running_fp32_ascending_and_descending_stay_at_half_the_bound(case):
    c, ref, mag, r = _case(case)
    args = (c['x'], c['w'], c['nbr'], c['n_in'], c['role'])
    bd = R.bound('f32', mag, r)
    for what, got in (('ascending', R.honest_fp32(*args, running=True)), ('descending', R.honest_fp32(*args, running=True, descending=True))):
        ok, over, rel = R.check(got, ref, bd, mag)
        print('[conv-lk host] %s %s: r 2^%.1f  err/mag 2^%.1f  err/bound %.3f' % (what, case, _lg(r), _lg(rel), over))
        assert ok and over <= 0.5, (what, over, rel)
        assert int(torch.count_nonzero(got[(mag == 0).all(dim=1)])) == 0       # a row without a neighbour is exactly zero
    if c['role'] in R.ON_OUTPUTS and ref.shape[0] > 3:                         # (the tables' dead rows are rows of the outputs)
        assert bool((mag == 0).all(dim=1).any())


# ---- degraded evaluations ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(T.DEGRADED))
def test_degraded_chunk_walks_exceed_the_bound_on_every_case_they_apply_to(name):
    applies, f = T.DEGRADED[name]
    seen = 0
    for case in T.CASES:
        c, ref, mag, r = _case(case)
        if not applies(c):
            continue
        ok, over, rel = R.check(f(c), ref, R.bound('f32', mag, r), mag)
        print('[conv-lk host] %s, %s: err/mag 2^%.1f  err/bound %.3g' % (name, case, _lg(rel), over))
        assert not ok and over > 1.0, (case, over, rel)
        seen += 1
    expect = sum(1 for case in T.CASES if (T.TABLES[case[0]][0] > T.CHUNK or name in ('the last chunk dropped', 'the last live pair skipped'))
                 and (case[1] == 'flip' or 'kflip' not in name))
    assert seen == expect and seen >= 6, (seen, expect)
