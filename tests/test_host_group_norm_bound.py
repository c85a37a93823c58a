"""tests/scene_rows_f64_ref.py, the float64 reference and the bound of the scene GroupNorm kernels (csrc/gn.hip), checked on
the host: the reference IS the loop formulation (F.group_norm scene by scene), a straightforward two-pass fp32 evaluation
stays inside the bound on every input set of the GPU test, and the bound rejects the formulations it has to reject."""
import pytest
import torch

import scene_rows_f64_ref as R


def _loop64(x, bidx, groups, gamma, beta):
    """torchsparse v1.4.0's formulation in float64: a mask, feats[mask], F.group_norm, a masked write, per batch index"""
    n, c = x.shape
    out = torch.zeros(n, c, dtype=torch.float64)
    for k in range(int(bidx.max()) + 1):
        mask = bidx == k
        if not bool(mask.any()):
            continue
        # (torch.group_norm: the operator behind F.group_norm, whose Python wrapper refuses a scene of one row)
        yk = torch.group_norm(x[mask].t().reshape(1, c, -1), groups, gamma, beta, R.EPS, False)
        out = out.masked_scatter(mask.reshape(-1, 1).expand(n, c), yk.reshape(c, -1).t())
    return out


@pytest.mark.parametrize('lay', R.LAYOUTS)
@pytest.mark.parametrize('c,groups', [(32, 4), (48, 16), (64, 64), (96, 1)])
def test_reference_is_the_loop_formulation(lay, c, groups):
    case = R.make_case(lay, c, 'randn', torch.float32)
    x = case['x'].double().requires_grad_()
    gamma, beta = case['gamma'].double().requires_grad_(), case['beta'].double().requires_grad_()
    y = _loop64(x, case['bidx'], groups, gamma, beta)
    f = R.forward64(case['x'], case['bidx'], groups, case['gamma'], case['beta'])
    assert float((y.detach() - f['y']).abs().max()) < 1e-12
    dx, dg, db = torch.autograd.grad(y, (x, gamma, beta), case['dy'].double())
    b = R.backward64(case['dy'], case['x'], case['bidx'], groups, case['gamma'], f=f)
    scale = lambda t: float(t.abs().max()) + 1.0
    assert float((dx - b['dx']).abs().max()) < 1e-11 * scale(dx)
    assert float((dg - b['dgamma']).abs().max()) < 1e-11 * scale(dg)
    assert float((db - b['dbeta']).abs().max()) < 1e-11 * scale(db)
    # the per-scene statistics are those of the scene's rows, wherever they lie
    for k, idx in f['scenes']:
        xs = case['x'][idx].double().reshape(idx.numel(), groups, c // groups)
        assert torch.allclose(f['mean'][k], xs.mean((0, 2)), rtol=0, atol=1e-13)
        assert torch.allclose(f['rstd'][k], 1.0 / torch.sqrt(xs.var((0, 2), unbiased=False) + R.EPS), rtol=1e-13, atol=0)


def _cases16():
    return [('L2', c, g, kind, dt, True) for c, g in R.SHAPES16 for kind in R.KINDS for dt in (torch.bfloat16, torch.float16)]


def _cases32():
    return [(lay, c, g, kind, torch.float32, aff) for c, g in R.SHAPES for lay in R.LAYOUTS for kind in R.KINDS
            for aff in (True, False)]


@pytest.mark.parametrize('lay,c,groups,kind,dtype,affine', _cases32() + _cases16())
def test_two_pass_fp32_is_inside_the_bound(lay, c, groups, kind, dtype, affine):
    case, f, fb, b, bb = R.reference(lay, c, groups, kind, dtype, affine)
    gamma, beta = (case['gamma'], case['beta']) if affine else (None, None)
    y = R.two_pass_fp32(case['x'], case['bidx'], groups, gamma, beta, dtype)
    ok, ratio, err = R.worst(y, f['y'], fb['y'])
    assert ok, f'y: error / bound {ratio:.3g} (error {err:.3g})'
    g = R.two_pass_backward_fp32(case['dy'], case['x'], case['bidx'], groups, gamma, dtype)
    for name in ('dx', 'dgamma', 'dbeta'):
        ok, ratio, err = R.worst(g[name], b[name], bb[name])
        assert ok, f'{name}: error / bound {ratio:.3g} (error {err:.3g})'


# where each wrong formulation shows: (layout, c, groups, kind)
_SHOWS = {'statistics per channel instead of per group': ('L1', 32, 4, 'randn'),
          'statistics over the whole batch instead of per scene': ('L2', 32, 4, 'randn'),
          'the unbiased variance': ('L3', 32, 4, 'randn'),
          'variance as E[x^2] - mean^2': ('L1', 32, 4, 'mean1e3'),
          'a dropped slab': ('L2', 48, 16, 'randn')}


@pytest.mark.parametrize('name', sorted(R.WRONG))
def test_the_bound_rejects(name):
    lay, c, groups, kind = _SHOWS[name]
    case, f, fb, _, _ = R.reference(lay, c, groups, kind, torch.float32, True)
    y = R.two_pass_fp32(case['x'], case['bidx'], groups, case['gamma'], case['beta'], torch.float32, variant=R.WRONG[name])
    ok, ratio, _ = R.worst(y, f['y'], fb['y'])
    assert not ok and ratio > 2.0, f'{name}: error / bound {ratio:.3g} is not rejected'


def test_the_named_wrong_formulations_are_all_there():
    assert sorted(R.WRONG) == sorted(_SHOWS) and len(R.WRONG) == 5


def test_pool_reference():
    x = torch.tensor([[1.0, 5.0], [3.0, 5.0], [3.0, -1.0], [9.0, 9.0]])
    bidx = torch.tensor([0, 0, 0, 2], dtype=torch.int32)
    p = R.pool64(x, bidx)
    assert torch.equal(p['max'], torch.tensor([[3.0, 5.0], [float('-inf')] * 2, [9.0, 9.0]]))
    assert p['arg'].tolist() == [[1, 0], [-1, -1], [3, 3]]        # the smallest row index among the maxima
    assert bool(p['avg'][1].isnan().all()) and p['avg'][0].tolist() == [7.0 / 3.0, 3.0]
