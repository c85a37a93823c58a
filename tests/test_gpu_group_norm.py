"""spnn.GroupNorm on the scene kernels (csrc/gn.hip), through the C ABI and through the module, against the float64 reference
under the derived bound of tests/scene_rows_f64_ref.py -- y, dx, dgamma, dbeta and the mean / rstd the ABI entry returns, no
element and no case left out.  Scene layouts sit on the slab edges (1, 127, 128, 129, 257 rows), reach their rows through the
order (shuffled) and leave a batch index without rows.  Every test prints its largest error / bound before it asserts."""
import pytest
import torch

import scene_rows_f64_ref as R
from u2mkd_amd import _lib as L
from u2mkd_amd import torchsparse as ts
from u2mkd_amd.torchsparse import nn as spnn
from u2mkd_amd.torchsparse.nn import functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def _dev(t):
    return None if t is None else t.to(DEV)


def _abi(case, groups, affine, dtype, plan):
    """one forward + backward through u2mkd_gn_forward / u2mkd_gn_backward: y, mean, rstd, dx, dgamma, dbeta"""
    x, dy = case['x'].to(DEV), case['dy'].to(DEV)
    gamma, beta = (_dev(case['gamma']), _dev(case['beta'])) if affine else (None, None)
    n, c = x.shape
    f32 = dict(dtype=torch.float32, device=DEV)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(plan.nb, groups, **f32), torch.empty(plan.nb, groups, **f32)
    stats = torch.empty(plan.nslab * groups * 2, dtype=torch.float64, device=DEV)
    partial = torch.empty(plan.nslab * (2 * c + 2 * groups), **f32)
    sums = torch.empty(plan.nb * groups * 2, **f32)
    dgamma, dbeta = (torch.empty(c, **f32), torch.empty(c, **f32)) if affine else (None, None)
    scene = (L.ptr(plan.bidx), L.ptr(plan.order), L.ptr(plan.seg), L.ptr(plan.slab_seg), L.ptr(plan.slabs), plan.nslab, plan.nb)
    L.call('u2mkd_gn_forward', L.ptr(x), CODE[dtype], n, c, groups, *scene, L.ptr(gamma), L.ptr(beta), R.EPS, L.ptr(stats),
           L.ptr(mean), L.ptr(rstd), L.ptr(y), L.stream())
    L.call('u2mkd_gn_backward', L.ptr(dy), L.ptr(x), CODE[dtype], n, c, groups, *scene, L.ptr(mean), L.ptr(rstd), L.ptr(gamma),
           L.ptr(partial), L.ptr(sums), L.ptr(dgamma), L.ptr(dbeta), L.ptr(dx), L.stream())
    torch.cuda.synchronize()
    return {'y': y, 'mean': mean, 'rstd': rstd, 'dx': dx, 'dgamma': dgamma, 'dbeta': dbeta}


def _module(case, groups, affine, coords):
    """the same through spnn.GroupNorm on a SparseTensor and autograd"""
    c = case['x'].shape[1]
    gn = spnn.GroupNorm(groups, c, affine=affine).to(DEV)
    if affine:
        with torch.no_grad():
            gn.weight.copy_(case['gamma'])
            gn.bias.copy_(case['beta'])
    x = case['x'].to(DEV).requires_grad_()
    inp = ts.SparseTensor(x, coords, stride=2)
    out = gn(inp)
    out.feats.backward(case['dy'].to(DEV))
    return {'y': out.feats.detach(), 'dx': x.grad, 'dgamma': gn.weight.grad if affine else None,
            'dbeta': gn.bias.grad if affine else None}, inp, out


def _hold(tag, got, f, fb, b, bb, affine):
    names = ['y', 'mean', 'rstd', 'dx'] + (['dgamma', 'dbeta'] if affine else [])
    bad = []
    for name in names:
        ref, bound = (f[name], fb[name]) if name in ('y', 'mean', 'rstd') else (b[name], bb[name])
        ok, ratio, err = R.worst(got[name], ref, bound)
        print(f'GNRATIO {tag} {name} {ratio:.4f} {err:.3e}')
        if not ok:
            bad.append(f'{name}: error / bound {ratio:.3g} (error {err:.3g})')
    assert not bad, f'{tag}: ' + '; '.join(bad)


def _exact_rows(case, lay, c, groups, kind, affine, y):
    """rows whose y is beta EXACTLY: a scene of variance 0, and the one-row scene when every channel is its own group"""
    bidx = case['bidx']
    beta = case['beta'].to(y.dtype) if affine else torch.zeros(c, dtype=y.dtype)
    rows = []
    if kind == 'const':
        rows.append(bidx == R.CONST_SCENE[lay])
    if groups == c and lay in ('L1', 'L2'):
        rows.append(bidx == 0)
    for mask in rows:
        got = y.cpu()[mask]
        assert got.shape[0] > 0 and torch.equal(got, beta.expand_as(got)), 'a group of variance 0 must give y = beta exactly'


@pytest.mark.parametrize('affine', [True, False], ids=['affine', 'plain'])
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('lay', R.LAYOUTS)
@pytest.mark.parametrize('c,groups', R.SHAPES)
def test_group_norm_fp32(c, groups, lay, kind, affine):
    case, f, fb, b, bb = R.reference(lay, c, groups, kind, torch.float32, affine)
    coords = R.coords_of(case['bidx']).to(DEV)
    plan = F.scene_plan(coords)
    assert plan.nb == f['nb'] and plan.n == case['x'].shape[0]
    got = _abi(case, groups, affine, torch.float32, plan)
    _hold(f'f32 C{c} G{groups} {lay} {kind} {"affine" if affine else "plain"}', got, f, fb, b, bb, affine)
    _exact_rows(case, lay, c, groups, kind, affine, got['y'])
    if lay == 'L3':       # the batch index without rows: nothing to normalise, its statistics are written as 0
        assert float(got['mean'][1].abs().max()) == 0.0 and float(got['rstd'][1].abs().max()) == 0.0
    mod, _, _ = _module(case, groups, affine, coords)
    for name, t in mod.items():       # the module runs the same kernels: the same bits
        assert (t is None and got[name] is None) or torch.equal(t, got[name]), name


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('dname', ['bf16', 'f16'])
@pytest.mark.parametrize('c,groups', R.SHAPES16)
def test_group_norm_16_bit_rows(c, groups, dname, kind):
    dtype = R.DTYPES[dname]
    case, f, fb, b, bb = R.reference('L2', c, groups, kind, dtype, True)
    coords = R.coords_of(case['bidx']).to(DEV)
    got = _abi(case, groups, True, dtype, F.scene_plan(coords))
    assert got['y'].dtype == dtype and got['dx'].dtype == dtype and got['dgamma'].dtype == torch.float32
    _hold(f'{dname} C{c} G{groups} L2 {kind} affine', got, f, fb, b, bb, True)
    _exact_rows(case, 'L2', c, groups, kind, True, got['y'])
    mod, _, _ = _module(case, groups, True, coords)       # stored 16-bit rows go in, the same type comes out
    assert mod['y'].dtype == dtype and mod['dx'].dtype == dtype and mod['dgamma'].dtype == torch.float32
    for name, t in mod.items():
        assert torch.equal(t, got[name]), name


@pytest.mark.parametrize('c,groups,lay', [(48, 16, 'L2'), (128, 32, 'L3'), (96, 1, 'L1')])
def test_three_runs_give_the_same_bits(c, groups, lay):
    case = R.make_case(lay, c, 'randn', torch.float32)
    coords = R.coords_of(case['bidx']).to(DEV)
    runs = [_module(case, groups, True, coords)[0] for _ in range(3)]
    for r in runs[1:]:
        for name in ('y', 'dx', 'dgamma', 'dbeta'):
            assert torch.equal(r[name], runs[0][name]), name


def test_module_keeps_coords_stride_and_maps():
    case = R.make_case('L2', 32, 'randn', torch.float32)
    coords = R.coords_of(case['bidx']).to(DEV)
    inp = ts.SparseTensor(case['x'].to(DEV), coords, stride=(2, 2, 4))
    inp.cmaps[(2, 2, 4)] = coords
    inp.kmaps['k'] = 'map'
    out = spnn.GroupNorm(4, 32).to(DEV)(inp)
    assert out.coords is inp.coords and out.stride == (2, 2, 4) and out.cmaps is inp.cmaps and out.kmaps is inp.kmaps
    assert out.feats.shape == inp.feats.shape and out.feats is not inp.feats
    out2 = F.group_norm(inp, 4)       # the functional form, no affine parameters
    assert out2.coords is inp.coords and out2.cmaps is inp.cmaps and out2.kmaps is inp.kmaps


def _loop(feats, bidx, groups, weight, bias):
    """the loop formulation on torch's GPU operators: mask, feats[mask], group_norm, masked write"""
    out = torch.zeros_like(feats)
    c = feats.shape[1]
    for k in range(int(bidx.max()) + 1):
        mask = bidx == k
        if int(mask.sum()) == 0:
            continue
        yk = torch.group_norm(feats[mask].t().reshape(1, c, -1), groups, weight, bias, R.EPS, False)
        out = out.masked_scatter(mask.reshape(-1, 1).expand_as(out), yk.reshape(c, -1).t())
    return out


@pytest.mark.parametrize('lay', R.LAYOUTS)
def test_width_the_kernels_do_not_serve_takes_the_loop(lay):
    bidx = R.layout(lay)
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(bidx.numel(), 6, generator=g).to(DEV)
    dy = torch.randn(bidx.numel(), 6, generator=g).to(DEV)
    gn = spnn.GroupNorm(3, 6).to(DEV)
    with torch.no_grad():
        gn.weight.normal_()
        gn.bias.normal_()
    x = x0.clone().requires_grad_()
    out = gn(ts.SparseTensor(x, R.coords_of(bidx).to(DEV)))
    out.feats.backward(dy)
    xr = x0.clone().requires_grad_()
    w, b = gn.weight.detach().clone().requires_grad_(), gn.bias.detach().clone().requires_grad_()
    ref = _loop(xr, bidx.to(DEV), 3, w, b)
    ref.backward(dy)
    assert torch.equal(out.feats, ref) and torch.equal(x.grad, xr.grad)
    # the parameter gradients are sums of at most 5 per-scene terms, which autograd may add in another order: each evaluation is
    # within 4 u of the exact sum of its terms' magnitudes
    xhat = ((ref - b) / w).detach().abs()
    assert bool(((gn.weight.grad - w.grad).abs() <= 8 * R.U32 * (dy.abs() * xhat).sum(0)).all())
    assert bool(((gn.bias.grad - b.grad).abs() <= 8 * R.U32 * dy.abs().sum(0)).all())


def test_second_layer_reads_nothing_from_the_device(monkeypatch):
    calls = []
    real = F.read_counts

    def counting(tensors):
        calls.append(len(tensors))
        return real(tensors)
    monkeypatch.setattr(F, 'read_counts', counting)
    case = R.make_case('L2', 32, 'randn', torch.float32)
    coords = R.coords_of(case['bidx']).to(DEV)       # a fresh coordinate tensor: no plan on it yet
    x = case['x'].to(DEV).requires_grad_()
    a, b = spnn.GroupNorm(4, 32).to(DEV), spnn.GroupNorm(8, 32).to(DEV)
    h = a(ts.SparseTensor(x, coords))
    assert calls == [1], 'the scene plan reads B once'
    out = b(h)
    pooled = F.global_avg_pool(out)
    (out.feats.sum() + pooled.sum()).backward()
    torch.cuda.synchronize()
    assert calls == [1], 'a second layer, a pooling and the backward over the same coordinates read nothing'
