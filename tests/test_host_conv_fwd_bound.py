"""The bounds of tests/conv_fwd_f64_ref.py on the CPU, on the inputs of tests/test_gpu_conv_fwd_f64.py (every pattern-and-spread
combination of ``COMBOS``): the synthetic tables reach the edges they claim, ``family`` restates the dispatch, the honest
evaluations -- plain fp32 with the offsets ascending and descending, in both accumulator structures of the kernels (per-offset
products, and on the roles the offset walkers serve their one running chain, each under the r measured on its own structure),
the bf16x3 form with exactly the six kept products, the one-plane 16-bit products with fp32 sums -- stay at or below HALF their
bound (measured: 0.25 / 0.25 per-offset ascending / descending, 0.25 / 0.45 running, 0.17 bf16x3), and every degraded evaluation
fails where it
should.  Half the bound is headroom for a summation order the CPU did not try; it makes a later GPU failure mean something.

The half is asked of what a summation order can change.  The 16-bit bounds and the epilogue's bound also hold the rounding of
a STORED value -- u |ref| of a bf16 / fp16 row, 2^-24 of the epilogue's fma and residual add -- which is the same in every order
and reaches its full size on single elements; there the evaluation has to pass the bound whose accumulation factor is halved
(``margin`` 2 instead of 4), and its ratio to the whole bound is printed.

No-ops, by construction (each of these forms fails on other patterns of the same test):
  * 'one neighbour index off by one row' on tails1 and ragged-one: one input row, there is no other row to point at;
  * 'mirrored offset not mirrored' on tails1: its one row is its own neighbour at offsets k and K-1-k alike, so the sum over the
    mirrored set of offsets is the same sum;
  * 'mirrored offset not mirrored' and 'weight not transposed' on the 'fwd' role: the forward neither mirrors nor transposes; they
    are judged on the 'flip' role (symmetric tables) and 'weight not transposed' also on the 'inv' role (ragged tables)."""
import functools
import math

import pytest
import torch

import conv_fwd_f64_ref as R

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
SHAPE = (64, 64)               # the degraded forms that swap weights need a square launch
HOST_COMBOS = R.COMBOS


def _lg(v):
    return math.log2(v) if v > 0 else float('-inf')


@functools.lru_cache(maxsize=None)
def _case(name, role, spread, dtype=F32, shape=SHAPE):
    c = R.make_case(name, role, shape[0], shape[1], spread, dtype)
    wr = c['w'].to(dtype).float() if dtype != F32 else c['w']          # 16-bit forms: the weights as the fragments hold them
    ref, mag, part = R.reference(c['x'], wr, c['nbr'], c['n_in'], role, nominal=dtype == F16)
    plain = R.reference(c['x'], wr, c['nbr'], c['n_in'], role)[1] if dtype == F16 else mag
    r = R.rel_err(R.honest_fp32(c['x'], wr, c['nbr'], c['n_in'], role), ref, plain)
    return c, ref, mag, part, r


@functools.lru_cache(maxsize=None)
def _r_running(name, role, spread):
    """r of the offset walkers: measured on the running chain (they serve the 'fwd' and 'flip' roles only)"""
    c, ref, mag, part, r = _case(name, role, spread)
    return R.rel_err(R.honest_fp32(c['x'], c['w'], c['nbr'], c['n_in'], role, running=True), ref, mag)


def _roles(name):
    return R.roles_of(name, inverse=name in R.RAGGED)


# ---- the tables ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(R.PATTERNS))
def test_every_offset_of_a_table_is_injective_and_in_range(name):
    nbr, n_in = R.table(name)
    gen, k, n_in_, n_out = R.PATTERNS[name]
    assert nbr.shape == (k, n_out) and nbr.dtype == torch.int32 and n_in == n_in_
    assert int(nbr.min()) >= -1 and int(nbr.max()) < n_in
    for kk in range(k):
        live = nbr[kk][nbr[kk] >= 0]
        assert len(torch.unique(live)) == len(live), (name, kk)
    # what u2mkd_pairs_capacity relies on: an offset holds at most min(n_in, n_out) pairs
    assert max(R.pair_counts(nbr)) <= min(n_in, n_out)
    assert torch.equal(nbr, R.table(name)[0])            # the generator is deterministic


@pytest.mark.parametrize('name', R.SYMMETRIC)
def test_tails_tables_are_symmetric_with_empty_and_centre_only_rows(name):
    nbr, n_in = R.table(name)
    k, n = nbr.shape
    assert n == n_in and n in R.TAILS
    for kk in range(k):
        j = torch.nonzero(nbr[kk] >= 0)[:, 0]
        assert torch.equal(nbr[k - 1 - kk][nbr[kk][j].long()].long(), j), kk
    c = k // 2
    live = nbr[c] >= 0
    assert torch.equal(nbr[c][live].long(), torch.nonzero(live)[:, 0])          # the centre is the identity on live rows
    per_row = (nbr >= 0).sum(dim=0)
    assert bool((per_row[~live] == 0).all())
    if n >= 63:
        assert int((per_row == 0).sum()) >= 2                                  # rows without a neighbour at any offset
        assert int(((per_row == 1) & live).sum()) >= 2                         # rows with the centre only
        assert abs(int((per_row == 0).sum()) - n / 10) <= n / 10
    else:
        assert int(per_row[0]) >= 1
    assert sorted(R.PATTERNS[p][3] for p in R.SYMMETRIC) == sorted(R.TAILS)


def test_ragged_tables_hold_the_listed_pair_counts():
    counts27 = R.pair_counts(R.table('ragged27')[0])
    assert counts27 == R.RAGGED_COUNTS[27]
    for c in (0, 1, 63, 64, 65, 127, 128, 129, 700):
        assert c in counts27
    assert R.pair_counts(R.table('ragged8')[0]) == R.RAGGED_COUNTS[8] and 700 in R.RAGGED_COUNTS[8] and 0 in R.RAGGED_COUNTS[8]
    one, n_in = R.table('ragged-one')
    assert n_in == 1 and set(R.pair_counts(one)) == {0, 1}
    (_, _, i27, o27), (_, _, i8, o8) = R.PATTERNS['ragged27'], R.PATTERNS['ragged8']
    assert i27 < o27 and i8 > o8                                               # n_in != n_out in both directions
    for name in R.RAGGED:                                                      # rows without a neighbour, on either side
        nbr, n_in = R.table(name)
        assert int(((nbr >= 0).sum(dim=0) == 0).sum()) > 0


def test_heavy_tiles_pass_both_split_thresholds_and_many_passes_the_grid_clamps():
    nbr, _ = R.table('heavy')
    has = (nbr >= 0).long()
    masks = (has << torch.arange(nbr.shape[0])[:, None]).sum(dim=0)
    assert len(torch.unique(masks)) == nbr.shape[1]                          # pairwise different masks
    blocks = R.tile_blocks(nbr)
    assert len(blocks) == 4
    assert any(30 < b <= 60 for b in blocks) and any(b > 60 for b in blocks), blocks     # U2MKD_TILE_SPLIT = 30, 60
    nbr, n_in = R.table('many')
    n = nbr.shape[1]
    padded = sum(-(-c // 128) * 128 for c in R.pair_counts(nbr))
    assert padded // 64 > 2048                                                 # the f32 pair kernel's workgroups walk runs of tiles
    cap = (27 * n + 127) // 128 * 128 + 128 * 27
    assert padded <= cap and cap // 64 > 2048
    # more WORK ITEMS (not just grid slots) than 256 CUs hold at 8 workgroups each -- the tile kernel's LDS allows no more, (64, 64)
    # and (32, 128) keep 4 and 3 -- so the clamped grid deals several items to a workgroup; the quarters alone are enough
    blocks = R.tile_blocks(nbr)
    assert R.work_items(nbr) > 2048 and 4 * (sum(b > 60 for b in blocks) - 1) > 2048
    assert R.work_items(R.table('heavy')[0]) == 2 + 2 + 4 + 4
    assert R.family(32, 256, F32, n, 27) == ('u2mkd_conv_forward_sorted', 'f32', ('conv_os3', 32, 'wide'))


# ---- the reference against itself ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['tails65', 'ragged27', 'ragged8', 'ragged-one'])
def test_the_float64_references_agree_and_the_inverse_role_is_the_adjoint(name):
    """conv_f64 (a dense gather per offset) and the pair loop give the same sums; conv_from_pairs_f64, built from nbr alone, is
    the adjoint of the forward: <conv(x), g> = <x, conv^T(g)>; on a symmetric table it equals the mirrored walk (flip)."""
    nbr, n_in = R.table(name)
    g_ = torch.Generator().manual_seed(5)
    x = torch.randn(n_in, 12, generator=g_, dtype=torch.float64)
    g = torch.randn(nbr.shape[1], 20, generator=g_, dtype=torch.float64)
    w = torch.randn(nbr.shape[0], 12, 20, generator=g_, dtype=torch.float64)
    y, mag = R.conv_f64(x, w, nbr, False)
    y2, mag2, part = R.reference(x, w, nbr, n_in, 'fwd')
    assert torch.allclose(y, y2, rtol=1e-13, atol=1e-13) and torch.allclose(mag, mag2, rtol=1e-13, atol=1e-13)
    assert bool((part <= mag * (1 + 1e-12)).all()) and bool((y.abs() <= part * (1 + 1e-12) + 1e-300).all())
    dx, dmag = R.conv_from_pairs_f64(g, w, nbr, n_in, True)
    assert dx.shape == x.shape
    lhs, rhs = float((y * g).sum()), float((x * dx).sum())
    assert abs(lhs - rhs) <= 1e-11 * float((mag * g.abs()).sum())
    up, _ = R.conv_from_pairs_f64(g[:, :12].contiguous(), w, nbr, n_in, False)          # the transposed convolution: 12 -> 20
    assert up.shape == (n_in, 20)
    assert abs(float((up * torch.ones_like(up)).sum()) - float((R.reference(torch.ones(n_in, 20, dtype=torch.float64), w, nbr, n_in, 'fwdT')[0]
                                                                * g[:, :12]).sum())) <= 1e-10 * float(up.abs().sum() + 1)
    if name in R.SYMMETRIC:
        flip, _ = R.conv_f64(g, w, nbr, True)
        assert torch.allclose(flip, dx, rtol=1e-12, atol=1e-12)


# ---- the dispatch ----------------------------------------------------------------------------------------------------------

def test_family_restates_the_dispatch_for_every_shape_of_the_gpu_test():
    fam = lambda ci, co, dt=F32, n=3000, k=27: R.family(ci, co, dt, n, k)
    # the tile kernel's 12 instantiations; f16x2 where cin is 32, 64 or 128, bf16x3 at cin 96; (64, 128) and (128, 64) sit on the
    # boundary of the two schedules: pairs below 24000 rows
    for co in (32, 64):
        for ci in (32, 64, 96, 128):
            want = ('u2mkd_conv_forward_tiles', 'x3' if ci == 96 else 'f16x2', None)
            if ci * co >= 8192:
                assert fam(ci, co, n=30000) == want and fam(ci, co)[0] == 'u2mkd_conv_forward_pairs_f16x2'
            else:
                assert fam(ci, co) == want, (ci, co)
    assert fam(32, 96) == ('u2mkd_conv_forward_tiles', 'f16x2', None) and fam(32, 128) == ('u2mkd_conv_forward_tiles', 'f16x2', None)
    assert fam(64, 96) == ('u2mkd_conv_forward_tiles', 'f16x2', None)
    assert fam(96, 64) == ('u2mkd_conv_forward_tiles', 'x3', None)             # the input gradient of 64 -> 96
    assert fam(64, 128, n=30000) == ('u2mkd_conv_forward_tiles', 'f16x2', None)
    assert fam(64, 128, n=23999) == ('u2mkd_conv_forward_pairs_f16x2', 'f16x2', (128, 1))
    assert fam(128, 128)[0] == 'u2mkd_conv_forward_pairs_f16x2' and not R.tiles_supported(128, 128)
    assert not R.tiles_supported(96, 96) and not R.tiles_supported(128, 96) and R.tiles_supported(128, 64)
    # u2mkd_conv_forward_sorted
    for (ci, co), form in {(4, 32): ('conv_os2', 32), (48, 16): ('conv_os2', 32), (20, 12): ('conv_os2', 32), (8, 20): ('conv_os2', 32),
                           (64, 48): ('conv_os2', 64), (16, 128): ('conv_os3', 32, 'narrow')}.items():
        assert fam(ci, co) == ('u2mkd_conv_forward_sorted', 'f32', form), (ci, co)
    assert fam(32, 256, n=R.MANY_ROWS)[2] == ('conv_os3', 32, 'wide') and fam(32, 256, n=32704)[2] == ('conv_os3', 32, 'narrow')
    assert fam(32, 256, n=800)[0] == 'u2mkd_conv_forward_pairs_f16x2'       # (below 24000 rows 32 x 256 is a pair-schedule layer)
    # the f32 pair kernel: channel counts the fragment kernels do not take
    for (ci, co), v in {(136, 96): 32, (96, 100): 32, (192, 48): 32, (128, 136): 64}.items():
        assert fam(ci, co) == ('u2mkd_conv_forward_pairs', 'f32', v), (ci, co)
    # the fragment pair kernels: every column tile of conv_px3.hip and both TL
    for (ci, co), form in {(32, 32): (128, 1), (96, 96): (96, 1), (128, 192): (192, 1), (64, 256): (256, 1), (256, 128): (128, 1),
                           (256, 512): (128, 2), (128, 128): (128, 1), (96, 192): (192, 1), (128, 136): None}.items():
        if form is not None and ci * co > 8192:
            assert fam(ci, co) == ('u2mkd_conv_forward_pairs_f16x2', 'f16x2', form), (ci, co)
    assert fam(512, 96, dt=BF16)[2] == (96, 2)
    # 16-bit rows: the tile kernel where it has the shape, the pair kernel everywhere else
    for dt, tag in ((BF16, '_bf16'), (F16, '_f16')):
        for ci, co in ((32, 32), (64, 64), (96, 64), (128, 32), (64, 128)):
            assert fam(ci, co, dt) == ('u2mkd_conv_forward_tiles' + tag, 'tile16', None)
        for (ci, co), form in {(96, 96): (96, 1), (160, 64): (128, 1), (256, 192): (192, 1)}.items():
            assert fam(ci, co, dt) == ('u2mkd_conv_forward_pairs' + tag, 'pair16', form)
    with pytest.raises(ValueError):
        fam(48, 16, BF16)


# ---- the split behind T_FWD ------------------------------------------------------------------------------------------------

def test_the_rounding_split_is_exact_and_its_planes_are_as_small_as_T_FWD_assumes():
    g = torch.Generator().manual_seed(2)
    w = torch.randn(200000, generator=g) * torch.pow(10.0, torch.randint(-20, 21, (200000,), generator=g).float())
    w[:4] = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -17, 2.0 - 2.0 ** -23, -(1.0 + 2.0 ** -7 - 2.0 ** -23)])
    h, m, l = R.split3_round(w)
    assert torch.equal(h.double() + m.double() + l.double(), w.double())
    for p in (h, m, l):
        assert int((p.view(torch.int32) & 0xffff).abs().max()) == 0            # each plane is a bf16
    assert bool((m.abs() <= 2.0 ** -8 * w.abs()).all()) and bool((l.abs() <= 2.0 ** -17 * w.abs()).all())
    x = w.flip(0).contiguous()
    xh, xm, xl = R.split3(x)
    dropped = m.double() * xl.double() + l.double() * xm.double() + l.double() * xl.double()
    assert bool((dropped.abs() <= R.T_FWD * (w.double() * x.double()).abs()).all())


# ---- honest evaluations ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,spread', HOST_COMBOS, ids=lambda v: str(v))
def test_honest_fp32_and_bf16x3_stay_at_half_their_bound(name, spread):
    for role in _roles(name):
        c, ref, mag, part, r = _case(name, role, spread)
        args = (c['x'], c['w'], c['nbr'], c['n_in'], role)
        forms = [('fp32 ascending', R.honest_fp32(*args), 'f32', r),
                 ('fp32 descending', R.honest_fp32(*args, descending=True), 'f32', r),
                 ('bf16x3, six products', R.x3_eval(*args), 'x3', r)]
        if role in ('fwd', 'flip'):          # the running chain of conv_os2 / conv_os3, under its own r
            rr = _r_running(name, role, spread)
            forms += [('fp32 running ascending', R.honest_fp32(*args, running=True), 'f32', rr),
                      ('fp32 running descending', R.honest_fp32(*args, running=True, descending=True), 'f32', rr)]
        for what, got, kind, rk in forms:
            ok, over, rel = R.check(got, ref, R.bound(kind, mag, rk), mag)
            print('[conv-f64 host] %s %s %s %s: r 2^%.1f  err/mag 2^%.1f  err/bound %.3f' % (what, name, role, spread, _lg(rk), _lg(rel), over))
            assert ok and over <= 0.5, (what, role, over, rel)
            # a row without a neighbour is exactly zero
            assert int(torch.count_nonzero(got[(mag == 0).all(dim=1)])) == 0
        # and both are far inside the f16x2 figure
        assert R.check(R.x3_eval(*args), ref, R.bound('f16x2', mag, r), mag)[1] <= 0.5


_COMBOS16 = [(n, s) for n, s in HOST_COMBOS if n != 'many']


@pytest.mark.parametrize('dtype', [BF16, F16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('name,spread', _COMBOS16, ids=lambda v: str(v))
def test_honest_16_bit_forms_pass_with_half_the_accumulation_margin(name, spread, dtype):
    for role in _roles(name):
        c, ref, mag, part, r = _case(name, role, spread, dtype)
        args = (c['x'], c['w'], c['nbr'], c['n_in'], role)
        k = c['k']
        forms = (('tile16', R.rows16_eval(*args, pair=False), 'tile16'), ('pair16', R.rows16_eval(*args, pair=True), 'pair16'),
                 ('pair16 with y kept in fp32', R.DEGRADED['pair16 with y kept in fp32'][2](c), 'pair16'))
        for what, got, kind in forms:
            half = R.bound(kind, mag, r, ref, part, dtype, k, margin=R.MARGIN / 2)
            ok, over, rel = R.check(got, ref, R.bound(kind, mag, r, ref, part, dtype, k), mag)
            print('[conv-f64 host] %s %s %s %s %s: r 2^%.1f  err/mag 2^%.1f  err/bound %.3f' % (what, str(dtype)[6:], name, role, spread, _lg(r), _lg(rel), over))
            assert bool(torch.isfinite(got.float()).all())
            assert ok and R.check(got, ref, half, mag)[0], (what, role, over)
        # the pair form's roundings of y are real: it does NOT fit the tile form's bound everywhere (ragged27: rows of many offsets)
        if name == 'ragged27' and role == 'fwd' and spread == 'rows':
            assert not R.check(forms[1][1], ref, R.bound('tile16', mag, r, ref, part, dtype, k), mag)[0]


@pytest.mark.parametrize('res,relu', [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize('name', ['tails65', 'ragged27'])
def test_epilogue_honest_passes_and_degraded_fails(name, res, relu):
    c, ref, mag, part, r = _case(name, 'fwd', 'rows')
    scale, shift, resid = R.make_affine(SHAPE[1], ref.shape[0])
    resid = resid if res else None
    assert bool((scale > 0).any()) and bool((scale < 0).any())
    want, emag = R.epilogue_f64(ref, mag, scale, shift, resid, relu)
    honest = R.honest_fp32(c['x'], c['w'], c['nbr'], c['n_in'], 'fwd')
    x3 = R.x3_eval(c['x'], c['w'], c['nbr'], c['n_in'], 'fwd')
    for kind in ('f32', 'x3', 'f16x2'):
        conv32 = honest if kind == 'f32' else x3           # (the bf16x3 emulation stands in under the f16x2 figure too)
        half = R.epilogue_bound(R.bound(kind, mag, r, margin=R.MARGIN / 2) if kind != 'f16x2' else R.bound(kind, mag, r) / 2, emag, scale, res)
        bd = R.epilogue_bound(R.bound(kind, mag, r), emag, scale, res)
        got = R.epilogue_fp32(conv32, scale, shift, resid, relu)
        ok, over, rel = R.check(got, want, bd, emag)
        print('[conv-f64 host] epilogue over %s %s res %d relu %d: err/emag 2^%.1f  err/bound %.3f' % (kind, name, res, relu, _lg(rel), over))
        assert ok and R.check(got, want, half, emag)[0], (kind, over)
        # a row without a neighbour: exactly the fp32 shift (+ res), ReLU applied
        dead = (mag == 0).all(dim=1)
        alone = shift.expand_as(got) + resid if res else shift.expand_as(got)
        assert bool(dead.any()) and torch.equal(got[dead], (alone.clamp(min=0) if relu else alone)[dead])
        for bad, kw in R.EPILOGUE_DEGRADED.items():
            if 'ReLU' in bad and not (res and relu):
                continue                                                       # (the same evaluation without both)
            ok, over, _ = R.check(R.epilogue_fp32(conv32, scale, shift, resid, relu, **kw), want, bd, emag)
            print('[conv-f64 host] %s over %s %s: err/bound %.3g' % (bad, kind, name, over))
            assert not ok and over > 1.0, (bad, kind, over)


# ---- degraded evaluations --------------------------------------------------------------------------------------------------

_ONE_ROW = ('tails1', 'ragged-one')
_REJECTED = sorted(n for n, (kinds, reject, f) in R.DEGRADED.items() if reject)


def _judged_roles(name, pattern):
    if name == 'mirrored offset not mirrored':
        return tuple(r for r in _roles(pattern) if r == 'flip')
    if name == 'weight not transposed':
        return tuple(r for r in _roles(pattern) if r in ('flip', 'inv'))
    return _roles(pattern)


@pytest.mark.parametrize('name', _REJECTED)
def test_degraded_evaluations_fail_the_widest_bound_on_the_rows_spread(name):
    """Judged against the elementwise LARGEST of the bounds the form applies to: what fails it fails each of them."""
    kinds = R.DEGRADED[name][0]
    seen = 0
    for pattern, spread in HOST_COMBOS:
        if spread != 'rows' or (pattern == 'many' and name.startswith('x3')):
            continue                                                           # (the bf16x3 emulation of 'many' is run once, above)
        for role in _judged_roles(name, pattern):
            if name == 'one neighbour index off by one row' and pattern in _ONE_ROW:
                continue                                                       # one input row: no other row to point at
            if name == 'mirrored offset not mirrored' and pattern == 'tails1':
                continue           # one row: offsets k and K-1-k both map it to itself, the sum over the mirrored set is the same sum
            c, ref, mag, part, r = _case(pattern, role, spread)
            got = R.DEGRADED[name][2](c)
            bd = functools.reduce(torch.maximum, [R.bound(kind, mag, r) for kind in kinds])
            ok, over, rel = R.check(got, ref, bd, mag)
            print('[conv-f64 host] %s, %s %s: err/mag 2^%.1f  err/bound %.3g' % (name, pattern, role, _lg(rel), over))
            assert not ok and over > 1.0, (pattern, role, over, rel)
            seen += 1
    assert seen >= 3, seen
