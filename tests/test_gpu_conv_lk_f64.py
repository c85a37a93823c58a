"""u2mkd_conv_forward_lk (csrc/conv_lk.hip: kernel volumes up to 343, the offsets walked in chunks of 32) against float64,
elementwise, through the C ABI on the synthetic tables of tests/conv_lk_tables.py: K = 32, 33, 63, 64, 65, 125, 129 and 343,
1 / 63 / 64 / 65 / 129 rows, a table whose live offsets are all in the last chunk, an empty middle chunk, a 16-row block and
single rows without any neighbour, n_in != n_out for the inverse roles (their table derived from nbr alone).

Reference and bound: ``reference`` and ``bound('f32', ...)`` of tests/conv_fwd_f64_ref.py, r measured per case by
``honest_fp32(running=True)`` -- the kernel keeps ONE running fp32 accumulator per element across offsets and channel steps, as
conv_os2 does.  Nothing is fitted to what the kernel returns; an element with mag = 0 must be exactly zero.  Every launch writes
into a NaN-prefilled output and is run three times: the same bits.  tests/test_host_conv_lk_bound.py shows on the same inputs
what the bound rejects."""
import math

import pytest
import torch

import conv_fwd_f64_ref as R
import conv_lk_tables as T

pytestmark = pytest.mark.gpu


def _lg(v):
    return math.log2(v) if v > 0 else float('-inf')


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a device fault: nothing else of this session may use the GPU
        pytest.exit('GPU fault in %s: %s' % (what, e), returncode=3)


def _launch(L, x, n_in, wt, tbl, kflip):
    """one u2mkd_conv_forward_lk into a NaN-prefilled output"""
    k, cb, ca = wt.shape
    n_rows = tbl.shape[1]
    assert x.shape[1] == ca and tbl.shape[0] == k and tbl.is_contiguous() and wt.is_contiguous() and x.is_contiguous()
    assert int(tbl.max()) < x.shape[0] and int(tbl.min()) >= -1                     # (checked before the kernel reads it)
    out = torch.full((n_rows, cb), float('nan'), device='cuda')
    L.call('u2mkd_conv_forward_lk', L.ptr(x), x.shape[0], ca, L.ptr(wt), cb, L.ptr(tbl), n_rows, n_rows, k, kflip, L.ptr(out), L.stream())
    _sync('u2mkd_conv_forward_lk K=%d %d -> %d' % (k, ca, cb))
    return out


@pytest.mark.parametrize('case', T.CASES, ids=['%s-%s-%dx%d-%s' % c for c in T.CASES])
def test_conv_forward_lk_against_float64(hip, case):
    L = hip
    c = T.make_case(case)
    name, role, ca, cb, spread = case
    assert L.load().u2mkd_conv_lk_supported(ca, cb, c['k']) == 1
    tbl, wt, kflip = T.launch(c)
    x, w, nbr = c['x'].cuda(), c['w'].cuda(), c['nbr'].cuda()
    ref, mag, part = R.reference(x, w, nbr, c['n_in'], role)
    r = R.rel_err(R.honest_fp32(x, w, nbr, c['n_in'], role, running=True), ref, mag)
    tbl, wt = tbl.cuda(), wt.cuda()
    got = _launch(L, x, x.shape[0], wt, tbl, kflip)
    assert got.shape == ref.shape
    ok, over, rel = R.check(got, ref, R.bound('f32', mag, r), mag)
    print('[conv-lk] %s: r 2^%.1f  err/mag 2^%.1f  err/bound %.3f' % (case, _lg(r), _lg(rel), over))
    assert bool(torch.isfinite(got).all())                                           # every element was written
    assert ok, (case, over, rel)
    assert int(torch.count_nonzero(got[mag == 0])) == 0                              # no neighbour: exact zeros
    if role in R.ON_OUTPUTS and ref.shape[0] > 3:
        assert bool((mag == 0).all(dim=1).any())
    for _ in range(2):
        assert torch.equal(_launch(L, x, x.shape[0], wt, tbl, kflip), got)


def test_a_wider_table_is_walked_by_its_leading_dimension(hip):
    """nbr [k, ld] with ld > n_rows: the first 70 rows of a 129-row table give the first 70 rows of the result"""
    L = hip
    c = T.make_case(('t125', 'fwd', 20, 24, 'unit'))
    tbl, wt, kflip = T.launch(c)
    x, wt, tbl = c['x'].cuda(), wt.cuda(), tbl.cuda()
    whole = _launch(L, x, x.shape[0], wt, tbl, kflip)
    part = torch.full((70, 24), float('nan'), device='cuda')
    L.call('u2mkd_conv_forward_lk', L.ptr(x), x.shape[0], 20, L.ptr(wt), 24, L.ptr(tbl), tbl.shape[1], 70, 125, kflip, L.ptr(part), L.stream())
    _sync('u2mkd_conv_forward_lk on 70 of 129 rows')
    assert torch.equal(part, whole[:70])


def test_arguments_are_checked_before_any_launch(hip):
    L = hip
    lib = L.load()
    assert lib.u2mkd_conv_lk_supported(4, 16, 125) == 1 and lib.u2mkd_conv_lk_supported(32, 32, 343) == 1
    assert lib.u2mkd_conv_lk_supported(5, 16, 125) == 0 and lib.u2mkd_conv_lk_supported(4, 0, 125) == 0
    assert lib.u2mkd_conv_lk_supported(4, 16, 344) == 0 and lib.u2mkd_conv_lk_supported(4, 16, 0) == 0
    x, wt = torch.zeros(8, 4, device='cuda'), torch.zeros(344, 4, 4, device='cuda')
    tbl = torch.full((344, 8), -1, dtype=torch.int32, device='cuda')
    out = torch.full((8, 4), 7.0, device='cuda')
    L.call('u2mkd_conv_forward_lk', L.ptr(x), 8, 4, L.ptr(wt), 4, L.ptr(tbl), 8, 0, 343, 0, L.ptr(out), L.stream())     # no rows: no launch
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(RuntimeError, match='kernel volume 344 not in 1..343'):
        L.call('u2mkd_conv_forward_lk', L.ptr(x), 8, 4, L.ptr(wt), 4, L.ptr(tbl), 8, 8, 344, 0, L.ptr(out), L.stream())
    with pytest.raises(RuntimeError, match='multiple of 4'):
        L.call('u2mkd_conv_forward_lk', L.ptr(x), 8, 6, L.ptr(wt), 4, L.ptr(tbl), 8, 8, 343, 0, L.ptr(out), L.stream())
    with pytest.raises(RuntimeError, match='kflip'):
        L.call('u2mkd_conv_forward_lk', L.ptr(x), 8, 4, L.ptr(wt), 4, L.ptr(tbl), 8, 8, 343, 2, L.ptr(out), L.stream())
    L.call('u2mkd_conv_forward_lk', L.ptr(x), 8, 4, L.ptr(wt), 4, L.ptr(tbl), 8, 8, 343, 1, L.ptr(out), L.stream())     # an empty table: zeros
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(out)) == 0
