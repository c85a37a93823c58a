"""spnn.GlobalAvgPool / GlobalMaxPool on the scene kernels (csrc/gn.hip) and F.spcrop, on the scene layouts of
tests/scene_rows_f64_ref.py: the max equals torch.max per scene, the mean is within ONE fp32 ulp of the float64 mean (the
column sums are carried in double up to the one division), a batch index without rows gives -inf / NaN, the max's gradient
goes to the smallest row index among the maxima, three runs give the same bits."""
import pytest
import torch

import scene_rows_f64_ref as R
from u2mkd_amd import torchsparse as ts
from u2mkd_amd.torchsparse import nn as spnn
from u2mkd_amd.torchsparse.nn import functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
WIDTHS = (4, 32, 100, 6)       # 6: not a multiple of 4, the loop formulation


def _case(lay, c):
    bidx = R.layout(lay)
    g = torch.Generator().manual_seed(977 * c + R.LAYOUTS.index(lay))
    n = bidx.numel()
    return bidx, torch.randn(n, c, generator=g), torch.randn(int(bidx.max()) + 1, c, generator=g)


def _run(module, x0, bidx, dy):
    x = x0.to(DEV).requires_grad_()
    out = module(ts.SparseTensor(x, R.coords_of(bidx).to(DEV)))
    out.backward(dy.to(DEV))
    return out.detach(), x.grad


def _same_bits(a, b):
    """torch.equal with the NaNs of a batch index without rows in the same places"""
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))


def _loop_grad(x0, bidx, dy, fn):
    """autograd through the loop formulation on the CPU (absent batch indices take no gradient)"""
    x = x0.clone().requires_grad_()
    nb, sc = R.scenes(bidx)
    out = torch.stack([fn(x[idx]) for _, idx in sc])
    out.backward(dy[[k for k, _ in sc]])
    return x.grad


@pytest.mark.parametrize('lay', R.LAYOUTS)
@pytest.mark.parametrize('c', WIDTHS)
def test_global_max_pool(c, lay):
    bidx, x, dy = _case(lay, c)
    ref = R.pool64(x, bidx)
    out, dx = _run(spnn.GlobalMaxPool(), x, bidx, dy)
    assert out.shape == (int(bidx.max()) + 1, c) and out.dtype == torch.float32
    assert torch.equal(out.cpu(), ref['max'])
    if lay == 'L3':
        assert bool((out[1] == float('-inf')).all()), 'a batch index without rows gives the identity of max'
    assert torch.equal(dx.cpu(), _loop_grad(x, bidx, dy, lambda t: t.max(0).values))      # (randn: no ties)
    again = [_run(spnn.GlobalMaxPool(), x, bidx, dy) for _ in range(2)]
    assert all(torch.equal(o, out) and torch.equal(g, dx) for o, g in again)


@pytest.mark.parametrize('lay', R.LAYOUTS)
@pytest.mark.parametrize('c', WIDTHS)
def test_global_avg_pool(c, lay):
    bidx, x, dy = _case(lay, c)
    ref = R.pool64(x, bidx)
    out, dx = _run(spnn.GlobalAvgPool(), x, bidx, dy)
    assert out.shape == ref['avg'].shape and out.dtype == torch.float32
    have = ref['count'] > 0
    err = (out.cpu().double() - ref['avg'])[have].abs()
    if c % 4 == 0:
        ulps = float((err / R.ulp32(ref['avg'][have])).max())
        print(f'POOLULP avg C{c} {lay} forward {ulps:.3f}')
        assert ulps <= 1.0
    else:       # the loop formulation: torch's fp32 mean; N_k additions in any order are within N_k u mean|x|, plus the division
        amean = torch.stack([x[idx].double().abs().mean(0) for _, idx in R.scenes(bidx)[1]])
        cnt = ref['count'][have].double().reshape(-1, 1)
        assert bool((err <= (cnt + 2) * R.U32 * amean).all())
    if lay == 'L3':
        assert bool(out[1].isnan().all()), 'a batch index without rows gives NaN, as torch.mean of nothing does'
    dref = torch.zeros(x.shape, dtype=torch.float64)
    for k, idx in R.scenes(bidx)[1]:
        dref[idx] = dy[k].double() / idx.numel()
    gerr = (dx.cpu().double() - dref).abs()
    gulps = float((gerr / R.ulp32(dref)).max())
    print(f'POOLULP avg C{c} {lay} backward {gulps:.3f}')
    assert gulps <= 1.0
    again = [_run(spnn.GlobalAvgPool(), x, bidx, dy) for _ in range(2)]
    assert all(_same_bits(o, out) and torch.equal(g, dx) for o, g in again)


def test_max_ties_and_nans():
    """equal maxima: the value is theirs, the gradient goes to the smallest row index; a NaN propagates"""
    bidx = R.layout('L2')       # shuffled: the smallest ROW index, not the first position in some other order
    n, c = bidx.numel(), 8
    x = torch.randn(n, c, generator=torch.Generator().manual_seed(3)).clamp(max=2.0)
    rows4 = (bidx == 4).nonzero().reshape(-1)
    rows3 = (bidx == 3).nonzero().reshape(-1)
    tied = rows4[[256, 3, 130, 77]]       # four equal maxima in three different slabs of scene 4
    x[tied, 0] = 5.0
    x[rows3[[100, 5]], 1] = 6.0
    x[rows3[50], 2] = float('nan')
    dy = torch.randn(5, c, generator=torch.Generator().manual_seed(4))
    out, dx = _run(spnn.GlobalMaxPool(), x, bidx, dy)
    out, dx = out.cpu(), dx.cpu()
    assert float(out[4, 0]) == 5.0 and float(out[3, 1]) == 6.0
    assert bool(out[3, 2].isnan()) and int(out.isnan().sum()) == 1
    first4, first3 = int(tied.min()), int(rows3[[100, 5]].min())
    assert float(dx[first4, 0]) == float(dy[4, 0]) and int((dx[:, 0] != 0).sum()) == 5
    assert float(dx[first3, 1]) == float(dy[3, 1]) and int((dx[:, 1] != 0).sum()) == 5
    assert float(dx[int(rows3[50]), 2]) == float(dy[3, 2])
    ref = R.pool64(x, bidx)
    keep = [0, 1, 3, 4, 5, 6, 7]
    assert torch.equal(out[:, keep], ref['max'][:, keep])


def test_functional_forms_and_16_bit_rows():
    bidx, x, _ = _case('L2', 32)
    coords = R.coords_of(bidx).to(DEV)
    xb = x.to(torch.bfloat16)
    inp = ts.SparseTensor(xb.to(DEV), coords)
    mx, av = F.global_max_pool(inp), F.global_avg_pool(inp)
    assert mx.dtype == torch.bfloat16 and av.dtype == torch.bfloat16
    ref = R.pool64(xb, bidx)
    assert torch.equal(mx.cpu(), ref['max'])
    assert torch.equal(av.cpu(), ref['avg'].float().to(torch.bfloat16))      # one rounding to fp32, one to the row type


def test_spcrop_is_the_boolean_mask():
    bidx = R.layout('L2')
    coords = R.coords_of(bidx).to(DEV)
    g = torch.Generator().manual_seed(9)
    x0 = torch.randn(bidx.numel(), 16, generator=g).to(DEV)
    lo, hi = (3, 2, 0), (30, 12, 0)
    x = x0.clone().requires_grad_()
    inp = ts.SparseTensor(x, coords, stride=2)
    inp.kmaps['k'] = 'map'
    out = spnn.SparseCrop(lo, hi)(inp)
    xyz = coords[:, :3]
    mask = ((xyz >= torch.tensor(lo, device=DEV)) & (xyz <= torch.tensor(hi, device=DEV))).all(1)
    assert 0 < int(mask.sum()) < bidx.numel()
    assert torch.equal(out.coords, coords[mask]) and torch.equal(out.feats, x0[mask])
    assert out.stride == inp.stride and out.kmaps == {} and out.cmaps == {} and out.kmaps is not inp.kmaps
    dy = torch.randn(out.feats.shape, generator=g).to(DEV)
    out.feats.backward(dy)
    xr = x0.clone().requires_grad_()
    xr[mask].backward(dy)
    assert torch.equal(x.grad, xr.grad)
    # both ends inclusive, one-sided forms
    only_min = F.spcrop(inp, coords_min=lo)
    assert torch.equal(only_min.coords, coords[(xyz >= torch.tensor(lo, device=DEV)).all(1)])
    only_max = F.spcrop(inp, coords_max=hi)
    assert torch.equal(only_max.coords, coords[(xyz <= torch.tensor(hi, device=DEV)).all(1)])
    assert F.spcrop(inp).coords.shape == coords.shape


def test_relu_and_leaky_relu_on_sparse_tensors():
    bidx = R.layout('L3')
    coords = R.coords_of(bidx).to(DEV)
    x = torch.randn(bidx.numel(), 8, generator=torch.Generator().manual_seed(1)).to(DEV)
    inp = ts.SparseTensor(x.clone(), coords, stride=4)
    out = F.relu(inp, inplace=False)
    assert torch.equal(out.feats, x.clamp(min=0)) and out.coords is inp.coords and out.kmaps is inp.kmaps and out.stride == (4, 4, 4)
    out = F.leaky_relu(inp, 0.2, inplace=False)
    assert torch.equal(out.feats, torch.nn.functional.leaky_relu(x, 0.2)) and out.cmaps is inp.cmaps
