"""tests/point_voxel_f64_ref.py, the float64 reference and the bound of the point <-> voxel row movers (csrc/voxel.hip), checked on
the host: the float64 functions are oracle/ts_ref's operations (the caller's ``counts`` honoured), every honest fp32 evaluation
stays inside the bound on every input set and row type of the GPU test, the bound rejects every formulation it has to reject, and
no fp16 reference sits at the edge of the type's range."""
import pytest
import torch

import point_voxel_f64_ref as P
from oracle import ts_ref as R

DT = tuple(P.DTYPES)
ORDERS = ('asc', 'desc', 'pair')


def _close(got, want, scale):
    """|got - want| <= 1e-12 of the magnitude that was summed, elementwise"""
    return bool(((got - want).abs() <= 1e-12 * scale + 1e-300).all())


@pytest.mark.parametrize('kind', ('randn', 'mean1e3', 'wide'))
@pytest.mark.parametrize('lay,cmode', [(lay, 'hist') for lay in P.VOX_LAYOUTS] + [('V1r', 'twice'), ('V3', 'twice')])
def test_voxelize64_is_the_oracle_on_double_inputs(lay, cmode, kind):
    for c in (3, 12):
        case = P.vox_case(lay, c, kind, torch.float32, cmode)
        x, g, idx, counts = case['x'].double(), case['g'].double(), case['idx'], case['counts']
        assert _close(case['mean'], R.voxelize_forward(x, idx, counts), P.voxelize64(x.abs(), idx, counts))
        want = R.voxelize_backward(g, idx, counts, idx.numel())
        assert _close(case['bwd'], want, want.abs())
        assert _close(case['sum'], R.voxelize_forward(x, idx, (counts > -1).int()), P.segment64(x.abs(), case['order'], None, case['seg']))
        if cmode == 'twice':        # the voxel whose count was set to 0 has points and stays 0
            v = int(((counts == 0) & (case['seg'][1:] > case['seg'][:-1])).nonzero()[0])
            assert float(case['mean'][v].abs().max()) == 0.0 and float(case['sum'][v].abs().max()) > 0.0


@pytest.mark.parametrize('kind', ('randn', 'mean1e3', 'wide'))
@pytest.mark.parametrize('wkind', P.WKINDS)
def test_devoxelize64_is_the_oracle_on_double_inputs(wkind, kind):
    for c in (3, 12):
        case = P.devox_case(wkind, c, kind, torch.float32)
        f, g, idx8, w8 = case['f'].double(), case['g'].double(), case['idx8'], case['w8'].double()
        assert _close(case['fwd'], R.devoxelize_forward(f, idx8, w8), P.devoxelize64(f.abs(), idx8, w8.abs()))
        assert _close(case['bwd'], R.devoxelize_backward(g, idx8, w8, case['nv']), P.devoxelize_bwd64(g.abs(), idx8, w8.abs(), case['nv']))
        # the two entry lists are transposes of each other: <devoxelize(f), g> = <f, devoxelize_bwd(g)>
        lhs, rhs = float((case['fwd'] * g).sum()), float((f * case['bwd']).sum())
        assert abs(lhs - rhs) <= 1e-9 * (abs(lhs) + 1.0)


@pytest.mark.parametrize('scale', P.TI_SCALES)
def test_ti_weights64_is_the_oracle_on_double_inputs(scale):
    case = P.ti_case(scale)
    want = R.calc_ti_weights(case['coords'].double(), case['idx_kn'], scale).t()
    assert _close(case['ref'], want, want.abs() + 1e-9)
    miss = case['idx_kn'].t() == -1
    assert float(case['ref'][miss].abs().max()) == 0.0 and float(case['bound'][miss].abs().max()) == 0.0
    n_miss = miss.sum(1)
    assert all(int((n_miss == k).sum()) >= 20 for k in (0, 3, 8))
    assert bool((case['coords'][:, :3] < 0).any()) and float(case['ref'].min()) == 0.0


def _inside(got, ref, bound, dtype, what):
    ok, ratio, err = P.compare(got, ref, bound, dtype)
    assert ok, '%s: err / bound = %.3g (err %.3g)' % (what, ratio, err)
    return ratio


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('lay', P.VOX_LAYOUTS)
def test_honest_voxelize_evaluations_are_inside_the_bound(lay, dt):
    dtype = P.DTYPES[dt]
    for c in P.widths(dtype):
        for kind in P.kinds(dtype, c):
            case = P.vox_case(lay, c, kind, dtype)
            for order in ORDERS:
                what = (lay, c, kind, dt, order)
                got = P.segment_fp32(case['x'], case['order'], None, case['seg'], True, case['counts'], dtype, order)
                _inside(got, case['mean'], case['mean_b'], dtype, ('mean',) + what)
                got = P.segment_fp32(case['x'], case['order'], None, case['seg'], False, None, dtype, order)
                _inside(got, case['sum'], case['sum_b'], dtype, ('sum',) + what)
            i = case['idx'].long()
            ok = (i >= 0) & (i < case['nv'])
            cnt = torch.where(ok, case['counts'].long()[i.clamp(0, case['nv'] - 1)], torch.zeros_like(i)).float()[:, None]
            rows = case['g'].float()[i.clamp(0, case['nv'] - 1)]
            got = torch.where(cnt > 0, rows / cnt.clamp(min=1.0), torch.zeros_like(rows)).to(dtype)
            _inside(got, case['bwd'], case['bwd_b'], dtype, ('bwd', lay, c, kind, dt))


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('lay', ('V1s', 'V1r', 'V3'))
def test_honest_evaluations_with_counts_that_are_not_the_histogram(lay, dt):
    dtype = P.DTYPES[dt]
    for c in (4, 32):
        case = P.vox_case(lay, c, 'randn', dtype, 'twice')
        for order in ORDERS:
            got = P.segment_fp32(case['x'], case['order'], None, case['seg'], True, case['counts'], dtype, order)
            _inside(got, case['mean'], case['mean_b'], dtype, (lay, c, dt, order))
        # ... and dividing by the segment length instead is outside it
        got = P.segment_fp32(case['x'], case['order'], None, case['seg'], True, None, dtype)
        assert not P.compare(got, case['mean'], case['mean_b'], dtype)[0]


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('wkind', P.WKINDS)
def test_honest_devoxelize_evaluations_are_inside_the_bound(wkind, dt):
    dtype = P.DTYPES[dt]
    for c in P.widths(dtype):
        for kind in P.kinds(dtype, c):
            case = P.devox_case(wkind, c, kind, dtype)
            fwd = P.devoxelize_fwd_plan(case['idx8'], case['w8'])
            for order in ORDERS:
                what = (wkind, c, kind, dt, order)
                _inside(P.segment_fp32(case['f'], *fwd, False, None, dtype, order), case['fwd'], case['fwd_b'], dtype, ('fwd',) + what)
                _inside(P.segment_fp32(case['g'], *case['plan'], False, None, dtype, order), case['bwd'], case['bwd_b'], dtype,
                        ('bwd',) + what)


@pytest.mark.parametrize('scale', P.TI_SCALES)
def test_honest_ti_weights_are_inside_the_bound(scale):
    case = P.ti_case(scale)
    got = P.ti_weights_fp32(case['coords'], case['idx_kn'], scale)
    _inside(got, case['ref'], case['bound'], torch.float32, ('ti', scale))


@pytest.mark.parametrize('name', sorted(P.WRONG))
def test_the_bound_rejects(name):
    form, variant, where = P.WRONG[name]
    good, ref, bound, dtype = P.evaluate(form, where)
    assert P.compare(good, ref, bound, dtype)[0]
    bad = P.evaluate(form, where, variant=variant)[0]
    ok, ratio, _ = P.compare(bad, ref, bound, dtype)
    assert not ok and ratio > 1.0, (name, ratio)


def test_the_wrong_formulations_cover_the_required_ones():
    have = {(form, variant) for form, variant, _ in P.WRONG.values()}
    assert have >= {('vox', 'tail_dropped'), ('vox', 'round_each_add'), ('devox_bwd', 'weights_rounded'),
                    ('devox_bwd', 'neighbour_weight'), ('vox', 'div_m_plus_1'), ('vox', 'sum_not_mean'),
                    ('devox_fwd', 'missing_as_row0'), ('devox_fwd', 'w8_transposed'), ('ti', 'no_eps'), ('ti', 'truncf')}
    sixteen = {where[3] for form, variant, where in P.WRONG.values() if variant == 'round_each_add'}
    assert sixteen == {'bf16', 'f16'}
    for form, variant, where in P.WRONG.values():      # the rounded sums are judged on the layouts with the 130- and 1000-entry segments
        if variant == 'round_each_add':
            assert where[0] in ('V1s', 'V1r') and {130, 1000} <= set(P.V1_LENS)


def test_no_fp16_reference_sits_at_the_edge_of_the_range():
    dtype = torch.float16
    seen_inf = {'mean': 0, 'sum': 0, 'fwd': 0, 'bwd': 0}
    for c in P.widths(dtype):
        for kind in P.kinds(dtype, c):
            cases = [P.vox_case(lay, c, kind, dtype) for lay in P.VOX_LAYOUTS] + [P.devox_case(w, c, kind, dtype) for w in P.WKINDS]
            cases += [P.vox_case(lay, c, 'randn', dtype, 'twice') for lay in ('V1s', 'V1r', 'V3') if c in (4, 32)]
            for case in cases:
                for r, b in case['pairs']:
                    assert P.straddles(case[r], case[b], dtype) == 0, (c, kind, r)
                    if kind == 'overflow' and r in seen_inf and ('idx8' in case) == (r in ('fwd', 'bwd')):
                        seen_inf[r] += int((case[r].abs() - case[b] > P.F16_INF).sum())
    # the overflow sets do leave the range: the mean (halved counts), the plain sum, the weighted sums
    assert all(v > 0 for v in seen_inf.values()), seen_inf


def test_compare_by_class():
    ref = torch.tensor([[0.0, 1.0, float('nan'), 1e5, -1e5]], dtype=torch.float64)
    bound = torch.tensor([[0.0, 1e-3, 0.0, 60.0, 60.0]], dtype=torch.float64)
    inf, nan = float('inf'), float('nan')
    good = torch.tensor([[0.0, 1.0005, nan, inf, -inf]], dtype=torch.float16)
    assert P.compare(good, ref, bound, torch.float16)[0]
    for k, v in ((0, 6e-8), (1, 1.002), (1, nan), (2, 0.0), (3, 65504.0), (3, -inf), (4, inf), (4, nan)):
        bad = good.clone()
        bad[0, k] = v
        assert not P.compare(bad, ref, bound, torch.float16)[0], (k, v)
    # a reference within its bound of [65504, 65520] is not decided: it counts as a straddle and fails
    edge = torch.tensor([[65500.0]], dtype=torch.float64)
    assert P.straddles(edge, torch.tensor([[40.0]], dtype=torch.float64), torch.float16) == 1
    assert not P.compare(torch.tensor([[65504.0]], dtype=torch.float16), edge, torch.tensor([[40.0]], dtype=torch.float64), torch.float16)[0]
    assert P.straddles(edge, torch.tensor([[40.0]], dtype=torch.float64), torch.bfloat16) == 0
