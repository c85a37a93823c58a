"""spnn.Conv3d with kernel volumes above 32, end to end: kernel_size 5 (K = 125), (3, 3, 5) (45), 7 (343), 4 at stride 1 (64, an
even volume: not symmetric), 4 at stride 4 with its transposed inverse, and 5 at stride 2 (the general down-sampling branch).
Two scenes of about 150 voxels with negative coordinates, one with a gap wider than any of the kernels.

Output coordinates against the rule of INTEGRATION.md, computed here from the coordinates alone; forward, dfeats and dkernel
against float64 built from a coordinate dictionary and get_kernel_offsets (nothing of the library's map code), under the bounds
of tests/conv_fwd_f64_ref.py ('f32', r of the running chain: these layers run on u2mkd_conv_forward_lk) and
tests/wgrad_f64_ref.py.  Under bf16 autocast a K = 125 layer returns the fp32 result rounded once; K = 729 raises."""
import math

import numpy as np
import pytest
import torch

import conv_fwd_f64_ref as R
import wgrad_f64_ref as W
from oracle import ts_ref as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ts(hip):
    import u2mkd_amd.torchsparse as ts
    return ts


def _lg(v):
    return math.log2(v) if v > 0 else float('-inf')


def _scenes():
    """int32 [n, 4] (x, y, z, batch), rows permuted: scene 0 = two clusters 20 voxels apart along x (a gap wider than 7), scene 1
    one cluster; both reach below zero"""
    rng = np.random.default_rng(11)

    def cluster(n, lo, hi, shift=(0, 0, 0)):
        box = hi - lo
        flat = rng.choice(box ** 3, n, replace=False)
        return np.stack(np.unravel_index(flat, (box,) * 3), 1) + lo + np.asarray(shift)

    s0 = np.concatenate([cluster(80, -3, 3), cluster(70, -2, 4, (20, 0, 1))])
    s1 = cluster(150, -4, 4)
    c = np.concatenate([np.concatenate([s0, np.zeros((len(s0), 1), int)], 1), np.concatenate([s1, np.ones((len(s1), 1), int)], 1)])
    c = c[rng.permutation(len(c))].astype(np.int32)
    assert len(np.unique(c, axis=0)) == len(c) == 300 and c[:, :3].min() < 0
    xs = np.sort(np.unique(c[c[:, 3] == 0][:, 0]))
    assert int(np.diff(xs).max()) > 7
    return np.ascontiguousarray(c)


def _sorted_bxyz(c):
    return np.ascontiguousarray(np.unique(c[:, [3, 0, 1, 2]], axis=0)[:, [1, 2, 3, 0]]).astype(np.int32)


def _out_coords(c, ks, st):
    """the rule of INTEGRATION.md (tensor stride 1)"""
    if all(s == 1 for s in st):
        return c
    if all(s in (1, k) for s, k in zip(st, ks)):
        f = c.copy()
        f[:, :3] = np.floor_divide(c[:, :3], np.asarray(st)) * np.asarray(st)
        return _sorted_bxyz(f)
    lo = c[:, :3].min(0)                                             # one minimum for all batches together
    cand = (c[None, :, :3] + O.get_kernel_offsets(ks, 1)[:, None, :]).reshape(-1, 3)
    cand = np.concatenate([cand, np.tile(c[:, 3:], (int(np.prod(ks)), 1))], 1)
    keep = ((cand[:, :3] % np.asarray(st) == 0) & (cand[:, :3] >= lo)).all(1)
    return _sorted_bxyz(cand[keep])


def _table(c, oc, ks):
    """nbr int32 [K, n_out] from a coordinate dictionary: the input row at out + offset"""
    index = {tuple(row): i for i, row in enumerate(c.tolist())}
    offs = O.get_kernel_offsets(ks, 1).tolist()
    nbr = torch.full((len(offs), len(oc)), -1, dtype=torch.int32)
    for k, (dx, dy, dz) in enumerate(offs):
        for j, (x, y, z, b) in enumerate(oc.tolist()):
            nbr[k, j] = index.get((x + dx, y + dy, z + dz, b), -1)
    return nbr


def _check_rows(what, got, x, w, nbr, n_in, role):
    ref, mag, part = R.reference(x, w, nbr, n_in, role)
    r = R.rel_err(R.honest_fp32(x, w, nbr, n_in, role, running=True), ref, mag)
    ok, over, rel = R.check(got.cpu(), ref, R.bound('f32', mag, r), mag)
    print('[large-kernel] %s: r 2^%.1f  err/mag 2^%.1f  err/bound %.3f' % (what, _lg(r), _lg(rel), over))
    assert got.shape == ref.shape and ok, (what, over, rel)
    assert int(torch.count_nonzero(got.cpu()[mag == 0])) == 0


def _check_dkernel(what, got, a, b, nbr, swap):
    kk, jj = torch.nonzero(nbr >= 0, as_tuple=True)
    pairs = torch.stack([nbr[kk, jj].long(), jj], dim=1).int()
    counts = (nbr >= 0).sum(dim=1).tolist()
    dw, mag = W.wgrad_f64(a, b, pairs, counts, swap)
    r = W.rel_err(W.honest_fp32(a, b, pairs, counts, swap), dw, mag)
    fam = W.family(a.shape[1], b.shape[1], torch.float32)
    ok, over, rel = W.check(got.cpu(), dw, mag, W.T_X3 if fam[0] == 'x3' else W.T_EXACT, r)
    print('[large-kernel] %s dkernel: err/mag 2^%.1f  err/bound %.3f' % (what, _lg(rel), over))
    assert ok, (what, over, rel)


LAYERS = [  # (kernel_size, stride, cin, cout)
    (5, 1, 4, 16), (5, 1, 5, 16), ((3, 3, 5), 1, 8, 16), (7, 1, 4, 8), (4, 1, 8, 16), (4, 4, 4, 16), (5, 2, 4, 16),
]


@pytest.mark.parametrize('ks,st,cin,cout', LAYERS, ids=lambda v: str(v).replace(' ', ''))
def test_conv3d_large_kernel_against_float64(ts, ks, st, cin, cout):
    spnn = ts.nn
    ks3, st3 = O.make_ntuple(ks), O.make_ntuple(st)
    k_total = int(np.prod(ks3))
    c = _scenes()
    torch.manual_seed(k_total + cin)
    x = torch.randn(len(c), cin)
    conv = spnn.Conv3d(cin, cout, kernel_size=ks, stride=st).cuda()
    assert tuple(conv.kernel.shape) == (k_total, cin, cout)
    w = conv.kernel.detach().cpu().clone()
    xin = x.cuda().requires_grad_(True)
    inp = ts.SparseTensor(xin, torch.from_numpy(c).cuda())
    inp.cmaps[inp.stride] = inp.coords          # (as v1.4.0: the transposed layer looks its output coordinates up by stride)
    y = conv(inp)
    oc = _out_coords(c, ks3, st3)
    assert y.coords.dtype == torch.int32 and (y.coords.cpu().numpy() == oc).all()
    assert y.stride == st3
    nbr = _table(c, oc, ks3)
    what = 'k%s s%s %d -> %d' % (ks3, st3, cin, cout)
    _check_rows(what + ' forward', y.F.detach(), x, w, nbr, len(c), 'fwd')
    g = torch.randn(len(oc), cout)
    y.F.backward(g.cuda())
    torch.cuda.synchronize()
    symmetric = st3 == (1, 1, 1) and k_total % 2 == 1
    _check_rows(what + ' dfeats', xin.grad, g, w, nbr, len(c), 'inv')
    if symmetric:       # the same sums on the forward table with mirrored offsets
        assert torch.allclose(R.reference(g, w, nbr, len(c), 'flip')[0], R.reference(g, w, nbr, len(c), 'inv')[0], rtol=1e-12, atol=1e-300)
    _check_dkernel(what, conv.kernel.grad, x, g, nbr, 0)
    assert tuple(y.kmaps)[0][1] == ks3 and len(y.kmaps[tuple(y.kmaps)[0]][0]) == int((nbr >= 0).sum())

    if st3 == (4, 4, 4):      # the transposed inverse on the same map: back to the input coordinates
        up = spnn.Conv3d(cout, cin, kernel_size=ks, stride=st, transposed=True).cuda()
        wu = up.kernel.detach().cpu().clone()
        yin = y.F.detach().clone().requires_grad_(True)
        yt = ts.SparseTensor(yin, y.coords, stride=y.stride)
        yt.cmaps, yt.kmaps = y.cmaps, y.kmaps
        z = up(yt)
        assert (z.coords.cpu().numpy() == c).all() and z.stride == (1, 1, 1)
        yc = yin.detach().cpu()
        _check_rows(what + ' transposed forward', z.F.detach(), yc, wu, nbr, len(c), 'invT')
        gz = torch.randn(len(c), cin)
        z.F.backward(gz.cuda())
        torch.cuda.synchronize()
        _check_rows(what + ' transposed dfeats', yin.grad, gz, wu, nbr, len(c), 'fwdT')
        _check_dkernel(what + ' transposed', up.kernel.grad, yc, gz, nbr, 1)


def test_bf16_autocast_rounds_the_fp32_result_once(ts):
    c = _scenes()
    torch.manual_seed(3)
    x = torch.randn(len(c), 32).cuda()
    conv = ts.nn.Conv3d(32, 32, kernel_size=5).cuda()
    coords = torch.from_numpy(c).cuda()
    with torch.no_grad():
        want = conv(ts.SparseTensor(x, coords)).F
        with torch.autocast('cuda', dtype=torch.bfloat16):
            got = conv(ts.SparseTensor(x, coords)).F
    assert want.dtype == torch.float32 and got.dtype == torch.bfloat16
    assert torch.equal(got, want.bfloat16())


def test_kernel_volume_above_343_raises_before_any_launch(ts):
    c = _scenes()
    conv = ts.nn.Conv3d(4, 8, kernel_size=9).cuda()
    with pytest.raises(ValueError, match=r'conv3d: kernel volume 729 .*above 343'):
        conv(ts.SparseTensor(torch.randn(len(c), 4).cuda(), torch.from_numpy(c).cuda()))
