"""The weight gradient of kernel volumes above 64: ConvolutionFunction.backward hands u2mkd_conv_wgrad_pairs the offsets in blocks
of at most 64 (KernelMap.pairs_blocks: u2mkd_wgrad_plan is one wave of 64 lanes) and writes block b into grad_weight[b0:b1].
On the synthetic tables of tests/conv_lk_tables.py at K = 64 (one block), 65 (a second block of one offset), 128, 129 and 343,
with (cin, cout) in (4, 32), (32, 32), (64, 64): grad_weight against ``wgrad_f64`` of tests/wgrad_f64_ref.py under its ``bound``
with the ``family`` of the shape (r measured per offset by its ``honest_fp32``), block by block -- a block stitched to the wrong
slice fails every element of two slices; an offset without pairs gets exact zeros; three runs give the same bits; kmap[0] /
kmap[1] are the rulebook computed from nbr on the CPU."""
import math

import pytest
import torch

import conv_lk_tables as T
import wgrad_f64_ref as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def F(hip):
    from u2mkd_amd.torchsparse.nn import functional as F
    return F


def _lg(v):
    return math.log2(v) if v > 0 else float('-inf')


def _backward(F, c, kmap):
    x = c['x'].cuda().requires_grad_(True)
    w = torch.nn.Parameter(c['w'].cuda())
    out = F.ConvolutionFunction.apply(x, w, kmap, False)
    out.backward(c['dy'].cuda())
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a device fault: nothing else of this session may use the GPU
        pytest.exit('GPU fault in the backward of K=%d: %s' % (c['k'], e), returncode=3)
    return w.grad.detach().clone()


@pytest.mark.parametrize('case', T.WGRAD_CASES, ids=['%s-%dx%d' % c for c in T.WGRAD_CASES])
def test_grad_weight_by_offset_blocks_against_float64(F, case):
    name, cin, cout = case
    c = T.make_wgrad_case(case)
    nbr, n_in, k = c['nbr'], c['n_in'], c['k']
    n_out = nbr.shape[1]
    kmap = F.KernelMap(nbr.cuda(), T.invert(nbr, n_in).cuda(), n_in, n_out, False, None)
    blocks = kmap.pairs_blocks()
    assert [(b[0], b[1]) for b in blocks] == [(b0, min(b0 + T.WGRAD_BLOCK, k)) for b0 in range(0, k, T.WGRAD_BLOCK)]
    got = _backward(F, c, kmap)
    assert got.shape == (k, cin, cout) and bool(torch.isfinite(got).all())

    pairs, counts = T.rulebook(nbr)
    a, b = c['x'].cuda(), c['dy'].cuda()
    dw, mag = W.wgrad_f64(a, b, pairs.cuda(), counts.tolist(), 0)
    r = W.rel_err(W.honest_fp32(a, b, pairs.cuda(), counts.tolist(), 0), dw, mag)
    fam = W.family(cin, cout, torch.float32)
    t = W.T_X3 if fam[0] == 'x3' else W.T_EXACT
    for b0, b1, *_ in blocks:                                   # the stitching: block by block
        ok, over, rel = W.check(got[b0:b1], dw[b0:b1], mag[b0:b1], t, r[b0:b1])
        print('[conv-lk wgrad] %s %s offsets %d..%d: err/mag 2^%.1f  err/bound %.3f' % (case, fam[0], b0, b1, _lg(rel), over))
        assert ok, (case, b0, b1, over, rel)
    empty = counts == 0
    if name == 't343':
        assert int(empty.sum()) >= 32                           # its empty middle chunk
    assert int(torch.count_nonzero(got[empty.cuda()])) == 0     # an offset without pairs: exact zeros
    for _ in range(2):
        assert torch.equal(_backward(F, c, kmap), got)

    # kmap[0], kmap[1], kmap[2]: torchsparse's rulebook, the blocks one after the other
    assert torch.equal(kmap[0].cpu(), pairs) and torch.equal(kmap[1].cpu(), counts) and kmap[2] == (n_in, n_out)
    assert kmap[0].dtype == torch.int32 and kmap[1].dtype == torch.int32


def test_prebuild_builds_the_blocks(F):
    nbr, n_in = T.make_table('t129')
    kmap = F.KernelMap(nbr.cuda(), T.invert(nbr, n_in).cuda(), n_in, nbr.shape[1], False, None)
    assert kmap._pair_blocks is None
    kmap.prebuild({'pairs_plan'})
    assert kmap._pair_blocks is not None and len(kmap.pairs_blocks()) == 3
    with pytest.raises(RuntimeError, match='pairs_blocks'):
        kmap.pairs_plan()
