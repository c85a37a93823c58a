"""FP16 STORAGE end to end: the reference's own mixed-precision mode (amp.autocast + amp.GradScaler,
core/nusc_trainers.py:157-158,285; torchsparse keeps conv / voxelize / devoxelize rows in half there --
custom_fwd(cast_inputs=torch.half)).

Per operator, under ``torch.autocast('cuda', float16)``: outputs and row gradients are fp16, and against the FP32 ORACLE
(oracle.ts_ref / torch CPU) evaluated on the same fp16-ROUNDED inputs the error stays within TOL = 2^-10 of the tensor's
magnitude.  That is tests/test_gpu_bf16_rows.py's 2^-7 scaled by the ratio of the unit roundoffs (2^-12 against 2^-9): the
kernels round at the same places.  A CPU emulation of the worst case -- 27 per-offset partials each rounded to fp16, summed
in fp32 and rounded once more -- reads 0.29-0.41 x 2^-10 of the tensor maximum at (64,64), (128,128) and (512,256), the
bf16 analogue 0.38-0.45 x 2^-7: the same 2.2-2.6 x margin.  Weight / parameter gradients are fp32.

What bf16 never needed: RANGE.  An fp32 result beyond +-65504 is stored as +-inf (never saturated), and inf / NaN in rows
reach dX and dW, because GradScaler finds an overflowed step by its non-finite gradients.

Then the model (rows really travel in fp16, U2MKD_F16_ROWS=0 gives the fp32-row formulation back), the trainer with its
GradScaler, and the weight-fragment caches of a module used under bf16 and fp16 autocast in turn."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from downsample_general_ref import ref_spdownsample_general
import point_voxel_f64_ref as P
from oracle import ts_ref as R
from u2mkd_amd.synth import synth_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2.0 ** -10
F16_MAX = 65504.0


@pytest.fixture(scope='module')
def F(hip):
    from u2mkd_amd.torchsparse.nn import functional as F
    return F


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _err(got, want):
    """max |got - want| relative to the magnitude of want"""
    want = want.double() if isinstance(want, torch.Tensor) else torch.from_numpy(want).double()
    return float((got.double().cpu() - want).abs().max() / (want.abs().max() + 1e-12))


def _held(got, ref_err):
    """inside the derived elementwise bound of tests/point_voxel_f64_ref.py for rows of got's type (no element excluded)"""
    ref, err = ref_err
    ok, ratio, worst = P.compare(got.detach(), ref, P.stored(err, ref, got.dtype), got.dtype)
    assert ok, 'err / bound = %.4g (err %.4g)' % (ratio, worst)


def _r(t):
    """fp16-rounded copy (fp32 values that are exactly representable in fp16)"""
    return t.half().float()


def _amp():
    return torch.autocast('cuda', dtype=torch.float16)


_MAPS = {}


def _scene(kind):
    """(coords, oracle nbmaps, nbsizes, (n_in, n_out) of the forward map, kernel size, stride) of synth_batch(2500, 2, 7);
    computed once and shared"""
    hit = _MAPS.get(kind)
    if hit is None:
        coords = synth_batch(2500, 2, 7)['coords']
        ks, st = (3, 1) if kind == 'subm' else (2, 2)
        nbmaps, nbsizes, oc, _ = R.build_kmap(coords, 1, ks, st)
        hit = _MAPS[kind] = (coords, nbmaps, nbsizes, (len(coords), len(oc)), ks, st)
    return hit


# ------------------------------------------------------------------ 1. conv
# (64,64) (96,128): the tile kernel; (256,192): the pair schedule, 64-channel steps; (96,96) (160,64): its 32-channel-step tail
@pytest.mark.parametrize('cin,cout', [(64, 64), (96, 128), (256, 192), (96, 96), (160, 64)])
@pytest.mark.parametrize('kind', ['subm', 'down', 'up'])
def test_conv_f16_rows_against_the_fp32_oracle(F, cin, cout, kind):
    coords, nbmaps, nbsizes, sizes, ks, st_ = _scene('subm' if kind == 'subm' else 'down')
    torch.manual_seed(cin + cout)
    km = F.build_kmap(_dev(coords), (1,) * 3, (ks,) * 3, (st_,) * 3)
    transposed = kind == 'up'
    n_in, n_out = (sizes[1], sizes[0]) if transposed else sizes
    x = _r(torch.randn(n_in, cin))
    w = _r(torch.randn(ks ** 3, cin, cout) / (ks ** 3 * cin) ** 0.5)
    g = _r(torch.randn(n_out, cout))
    want = R.conv_forward(x, w, nbmaps, nbsizes, sizes, transposed=transposed)
    wgi, wgw = R.conv_backward(x, w, g, nbmaps, nbsizes, transposed=transposed)
    xd, wd = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    with _amp():
        assert F.row_dtype() == torch.float16
        out = F.ConvolutionFunction.apply(xd, wd, km, transposed)
    assert out.dtype == torch.float16 and bool(torch.isfinite(out.float()).all())
    e_out = _err(out, want)
    out.backward(g.cuda().half())
    assert xd.grad.dtype == torch.float32 and wd.grad.dtype == torch.float32      # the dtypes of the leaves
    e_dx, e_dw = _err(xd.grad, wgi), _err(wd.grad, wgw)
    print('conv %s %d->%d: out %.3f dx %.3f dw %.3f (x TOL)' % (kind, cin, cout, e_out / TOL, e_dx / TOL, e_dw / TOL))
    assert e_out < TOL and e_dx < TOL and e_dw < TOL
    # deterministic
    with _amp():
        again = F.ConvolutionFunction.apply(xd, wd, km, transposed)
    assert torch.equal(out, again)


def test_strided_k27_conv_f16_rows_through_conv3d(F):
    """(64, 64) on the k = 3, s = 2 map (the general down-sample) through ``conv3d`` under fp16 autocast"""
    from u2mkd_amd import torchsparse as ts
    c = synth_batch(3000, 2, 7)['coords']
    oc = ref_spdownsample_general(c, 2, 3, 1)
    nbmaps, nbsizes, _, _ = R.build_kmap(c, 1, 3, 2, out_coords=oc)
    sizes = (len(c), len(oc))
    torch.manual_seed(128)
    x = _r(torch.randn(sizes[0], 64))
    w = _r(torch.randn(27, 64, 64) / (27 * 64) ** 0.5)
    g = _r(torch.randn(sizes[1], 64))
    want = R.conv_forward(x, w, nbmaps, nbsizes, sizes, transposed=False)
    wgi, wgw = R.conv_backward(x, w, g, nbmaps, nbsizes, transposed=False)
    xd, wd = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    with _amp():
        out = F.conv3d(ts.SparseTensor(xd, _dev(c)), wd, 3, stride=2)
    assert (out.coords.cpu().numpy() == oc).all()
    assert out.feats.dtype == torch.float16 and bool(torch.isfinite(out.feats.float()).all())
    assert _err(out.feats, want) < TOL
    out.feats.backward(g.cuda().half())
    assert xd.grad.dtype == torch.float32 and wd.grad.dtype == torch.float32
    assert _err(xd.grad, wgi) < TOL and _err(wd.grad, wgw) < TOL


# ------------------------------------------------------------------ 2. the 4-channel stem
def test_conv_small_channel_counts_round_the_fp32_result(F):
    """the 4-channel stem has no 16-bit kernel: fp32 rows in, fp32 kernel, ONE rounding of the result"""
    coords = synth_batch(2000, 1, 3)['coords']
    km = F.build_kmap(_dev(coords), (1,) * 3, (3,) * 3, (1,) * 3)
    torch.manual_seed(0)
    x, w = torch.randn(len(coords), 4, device='cuda'), torch.randn(27, 4, 32, device='cuda') * 0.1
    ref = F.ConvolutionFunction.apply(x, w, km, False)
    with _amp():
        out = F.ConvolutionFunction.apply(x, w, km, False)
    assert out.dtype == torch.float16 and torch.equal(out, ref.half())


# ------------------------------------------------------------------ 3. Linear
@pytest.mark.parametrize('n,cin,cout,bias', [(777, 128, 96, False), (64, 96, 32, True), (5000, 32, 256, True)])
def test_linear_f16_rows(F, n, cin, cout, bias):
    torch.manual_seed(n)
    x, w = _r(torch.randn(n, cin)), _r(torch.randn(cout, cin) / cin ** 0.5)
    b = torch.randn(cout) if bias else None
    g = _r(torch.randn(n, cout))
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if bias else None
    yr = torch.nn.functional.linear(xr, wr, br)
    yr.backward(g)
    xd, wd = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    bd = b.cuda().requires_grad_(True) if bias else None
    with _amp():
        y = F.linear(xd, wd, bd)
    assert y.dtype == torch.float16 and _err(y, yr.detach()) < TOL
    y.backward(g.cuda().half())
    assert wd.grad.dtype == torch.float32
    assert _err(xd.grad, xr.grad) < TOL and _err(wd.grad, wr.grad) < TOL
    if bias:
        assert bd.grad.dtype == torch.float32 and _err(bd.grad, br.grad) < 1e-4


# ------------------------------------------------------------------ 4. BatchNorm
@pytest.mark.parametrize('n,c', [(5000, 32), (777, 256)])
@pytest.mark.parametrize('mode', ['plain', 'relu', 'res'])
def test_batch_norm_f16_rows(F, n, c, mode):
    torch.manual_seed(c)
    x = _r(torch.randn(n, c) * 2 + 0.5)
    res = _r(torch.randn(n, c)) if mode == 'res' else None
    g = _r(torch.randn(n, c))
    bn_r = torch.nn.BatchNorm1d(c).double()
    with torch.no_grad():
        bn_r.weight.uniform_(0.5, 1.5)
        bn_r.bias.uniform_(-0.5, 0.5)
    bn_d = torch.nn.BatchNorm1d(c)
    bn_d.load_state_dict({k: v.float() for k, v in bn_r.state_dict().items()})
    bn_d.cuda()
    xr = x.double().requires_grad_(True)
    rr = res.double().requires_grad_(True) if res is not None else None
    yr = bn_r(xr)
    if mode == 'res':
        yr = torch.relu(yr + rr)
    elif mode == 'relu':
        yr = torch.relu(yr)
    yr.backward(g.double())
    xd = x.cuda().half().requires_grad_(True)
    rd = res.cuda().half().requires_grad_(True) if res is not None else None
    with _amp():
        y = F.batch_norm(xd, bn_d, mode != 'plain', rd)
    assert y.dtype == torch.float16 and _err(y, yr.detach()) < TOL
    y.backward(g.cuda().half())
    assert xd.grad.dtype == torch.float16
    # the ReLU mask flips only where |pre-activation| is below the fp16 rounding of y: the masked gradient rows differ
    # there by one element of g; a relative bound over the tensor holds them (4 x TOL, as the bf16 suite)
    assert _err(xd.grad, xr.grad) < 4 * TOL
    if rd is not None:
        assert rd.grad.dtype == torch.float16 and _err(rd.grad, rr.grad) < 4 * TOL
    assert bn_d.weight.grad.dtype == torch.float32 and bn_d.bias.grad.dtype == torch.float32
    assert _err(bn_d.weight.grad, bn_r.weight.grad) < TOL and _err(bn_d.bias.grad, bn_r.bias.grad) < TOL
    # running statistics from the fp16-rounded rows, in fp32
    assert bn_d.running_mean.dtype == torch.float32
    assert _err(bn_d.running_mean, bn_r.running_mean) < 1e-5 and _err(bn_d.running_var, bn_r.running_var) < 1e-5
    # eval mode
    bn_d.eval(); bn_r.eval()
    with _amp():
        ye = F.batch_norm(x.cuda().half(), bn_d, mode != 'plain', rd.detach() if rd is not None else None)
    yre = bn_r(x.double())
    yre = torch.relu(yre + res.double()) if mode == 'res' else (torch.relu(yre) if mode == 'relu' else yre)
    assert ye.dtype == torch.float16 and _err(ye, yre) < TOL


@pytest.mark.parametrize('with_res', [False, True])
def test_sync_batch_norm_pieces_reproduce_the_one_entry_passes_on_f16_rows(F, with_res):
    """u2mkd_bn_local_stats -> u2mkd_bn_merge_stats (one rank) -> u2mkd_bn_apply and u2mkd_bn_backward_local ->
    u2mkd_bn_backward_apply with row dtype 2 against u2mkd_bn_train_forward / u2mkd_bn_backward with row dtype 2: the
    same kernels over the same fp16 rows, bit for bit."""
    L = F.L
    n, c, eps, relu = 3001, 96, 1e-5, 1
    torch.manual_seed(7)
    x = (torch.randn(n, c, device='cuda') * 2 + 0.5).half()
    res = torch.randn(n, c, device='cuda').half() if with_res else None
    dy = torch.randn(n, c, device='cuda').half()
    gamma, beta = torch.rand(c, device='cuda') + 0.5, torch.randn(c, device='cuda')
    st = L.stream()
    slabs = L.load().u2mkd_bn_num_slabs(n)
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device='cuda')
    # one entry per pass
    partial, mean, invstd, y = f32(slabs * 2 * c), f32(c), f32(c), torch.empty_like(x)
    L.call('u2mkd_bn_train_forward', L.ptr(x), L.ptr(res), 2, n, c, L.ptr(gamma), L.ptr(beta), eps, 0.1, None, None, None, relu,
           L.ptr(partial), L.ptr(mean), L.ptr(invstd), L.ptr(y), st)
    dgamma, dbeta, dx = f32(c), f32(c), torch.empty_like(x)
    dres = torch.empty_like(x) if with_res else None
    L.call('u2mkd_bn_backward', L.ptr(dy), L.ptr(x), L.ptr(res), 2, n, c, L.ptr(mean), L.ptr(invstd), L.ptr(gamma), L.ptr(beta),
           relu, 1, L.ptr(partial), L.ptr(dgamma), L.ptr(dbeta), L.ptr(dx), L.ptr(dres), st)
    # the pieces
    stats, mit, y2 = f32(1, 2 * c + 1), f32(2 * c + 1), torch.empty_like(x)
    L.call('u2mkd_bn_local_stats', L.ptr(x), 2, n, c, L.ptr(partial), L.ptr(stats), st)
    mean2, invstd2, total = mit[:c], mit[c:2 * c], mit[2 * c:]
    L.call('u2mkd_bn_merge_stats', L.ptr(stats), 1, c, eps, 0.1, None, None, L.ptr(mean2), L.ptr(invstd2), L.ptr(total), None, st)
    L.call('u2mkd_bn_apply', L.ptr(x), L.ptr(res), 2, n, c, L.ptr(mean2), L.ptr(invstd2), L.ptr(gamma), L.ptr(beta), relu,
           L.ptr(y2), st)
    sums, dx2 = f32(2 * c), torch.empty_like(x)
    dres2 = torch.empty_like(x) if with_res else None
    L.call('u2mkd_bn_backward_local', L.ptr(dy), L.ptr(x), L.ptr(res), 2, n, c, L.ptr(mean2), L.ptr(invstd2), L.ptr(gamma),
           L.ptr(beta), relu, L.ptr(partial), L.ptr(sums), None, st)
    L.call('u2mkd_bn_backward_apply', L.ptr(dy), L.ptr(x), L.ptr(res), 2, n, c, L.ptr(total), L.ptr(mean2), L.ptr(invstd2),
           L.ptr(gamma), L.ptr(beta), relu, L.ptr(sums), L.ptr(dx2), L.ptr(dres2), st)
    assert bool(torch.isfinite(y.float()).all()) and float(y.float().abs().max()) > 0
    print('pieces: |mean - mean2| %.3g |invstd - invstd2| %.3g y %d dx %d differing elements' % (
        float((mean - mean2).abs().max()), float((invstd - invstd2).abs().max()), int((y != y2).sum()), int((dx != dx2).sum())))
    assert torch.equal(y, y2) and torch.equal(dx, dx2)
    assert torch.equal(dbeta, sums[:c]) and torch.equal(dgamma, sums[c:])
    if with_res:
        assert torch.equal(dres, dres2)


def test_every_row_batch_norm_entry_refuses_row_dtype_3(F):
    """each of the seven entries checks its row-dtype argument before anything else (no launch: the buffers are never read)"""
    L = F.L
    n, c, eps = 64, 32, 1e-5
    x = torch.zeros(n, c, device='cuda')
    v = torch.zeros(2 * c + 1, device='cuda')
    X, V, st = L.ptr(x), L.ptr(v), L.stream()
    entries = {
        'u2mkd_bn_train_forward': (X, None, 3, n, c, V, V, eps, 0.1, None, None, None, 0, V, V, V, X, st),
        'u2mkd_bn_eval_forward': (X, None, 3, n, c, V, V, eps, V, V, 0, V, X, st),
        'u2mkd_bn_backward': (X, X, None, 3, n, c, V, V, V, V, 0, 1, V, V, V, X, None, st),
        'u2mkd_bn_local_stats': (X, 3, n, c, V, V, st),
        'u2mkd_bn_apply': (X, None, 3, n, c, V, V, V, V, 0, X, st),
        'u2mkd_bn_backward_local': (X, X, None, 3, n, c, V, V, V, V, 0, V, V, None, st),
        'u2mkd_bn_backward_apply': (X, X, None, 3, n, c, V, V, V, V, V, 0, V, X, None, st),
    }
    assert len(entries) == 7
    for name, args in entries.items():
        with pytest.raises(RuntimeError, match=name + ': row dtype 3'):
            L.call(name, *args)
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0 and float(v.abs().max()) == 0.0


# ------------------------------------------------------------------ 5. voxelize / devoxelize
def test_point_voxel_transfers_f16_rows(F):
    b = synth_batch(6000, 2, 11)
    coords = b['coords']
    c = 64
    torch.manual_seed(1)
    # voxelize: points -> stride-2 voxels
    fl = np.concatenate([coords[:, :3] // 2 * 2, coords[:, 3:]], 1).astype(np.int32)
    uniq, inv = np.unique(fl, axis=0, return_inverse=True)
    idx = torch.from_numpy(inv.astype(np.int32))
    counts = torch.bincount(idx.long(), minlength=len(uniq)).int()
    feats = _r(torch.randn(len(coords), c))
    g = _r(torch.randn(len(uniq), c))
    fd = feats.cuda().requires_grad_(True)
    with _amp():
        out = F.spvoxelize(fd, idx.cuda(), counts.cuda())
    assert out.dtype == torch.float16
    _held(out, P.voxelize_full(feats, idx, counts))
    out.backward(g.cuda().half())
    _held(fd.grad.to(out.dtype), P.voxelize_bwd_full(g, idx, counts))
    # the 4-channel coordinate means stay fp32 (SphereFormer quantises them into windows)
    with _amp():
        xyz = F.spvoxelize(torch.randn(len(coords), 4, device='cuda'), idx.cuda(), counts.cuda())
    assert xyz.dtype == torch.float32
    # devoxelize: 8-corner gather with random weights, some corners missing
    nv = len(uniq)
    i8 = torch.randint(-1, nv, (len(coords), 8), dtype=torch.int32)
    w8 = torch.rand(len(coords), 8) * (i8 >= 0)
    vf = _r(torch.randn(nv, c))
    gp = _r(torch.randn(len(coords), c))
    vd = vf.cuda().requires_grad_(True)
    with _amp():
        y = F.spdevoxelize(vd, i8.cuda(), w8.cuda())
    assert y.dtype == torch.float16
    _held(y, P.devoxelize_full(vf, i8, w8))
    y.backward(gp.cuda().half())
    _held(vd.grad.to(y.dtype), P.devoxelize_bwd_full(gp, i8, w8, nv))


# ------------------------------------------------------------------ 6. range
def _range_case(cin, cout):
    """(x, w, want, half) of the range test: the second half of the rows (the second scene of the batch: no neighbour in the
    first) scaled by 2^12, the weights by 2^11 -- both still inside fp16 -- so that the fp32 result of those rows is ~2^23 z."""
    coords, nbmaps, nbsizes, sizes, ks, _ = _scene('subm')
    torch.manual_seed(1000 + cin + cout)
    n = sizes[0]
    half = n // 2
    x = torch.randn(n, cin)
    x[half:] *= 2.0 ** 12
    x = _r(x)
    # (unit variance per neighbour, w ~ N(0, 1 / cin): |want| ~ 2^23 |z| with z ~ N(0, neighbours) on the second half)
    w = _r(torch.randn(ks ** 3, cin, cout) / cin ** 0.5 * 2.0 ** 11)
    assert float(x.abs().max()) < F16_MAX and float(w.abs().max()) < F16_MAX
    want = R.conv_forward(x, w, nbmaps, nbsizes, sizes, transposed=False)
    want = want if isinstance(want, torch.Tensor) else torch.from_numpy(want)
    return x, w, want.float(), half


@pytest.mark.parametrize('cin,cout', [(64, 64), (256, 192)])      # the tile kernel; the pair schedule (fp16 scratch rows)
def test_values_beyond_the_fp16_range_become_inf_and_never_a_finite_number(F, cin, cout):
    coords = _scene('subm')[0]
    x, w, want, half = _range_case(cin, cout)
    km = F.build_kmap(_dev(coords), (1,) * 3, (3,) * 3, (1,) * 3)
    with _amp(), torch.no_grad():
        out = F.ConvolutionFunction.apply(x.cuda(), w.cuda(), km, False).cpu()
    assert out.dtype == torch.float16
    lo, lo_want = out[:half].float(), want[:half]
    assert bool(torch.isfinite(lo).all()) and float(lo_want.abs().max()) < F16_MAX
    assert float((lo - lo_want).abs().max() / lo_want.abs().max()) < TOL
    checked = want[half:].abs() > 1.1 * F16_MAX
    # (elements below the threshold are not checked: per-offset fp16 partials of the pair schedule may already have overflowed)
    share = float(checked.float().mean())
    assert share >= 0.98, share
    assert not bool(torch.isfinite(out[half:].float())[checked].any())


def test_an_inf_in_the_output_gradient_reaches_both_gradients(F):
    coords, _, _, sizes, _, _ = _scene('subm')
    km = F.build_kmap(_dev(coords), (1,) * 3, (3,) * 3, (1,) * 3)
    torch.manual_seed(5)
    for cin, cout in ((64, 64), (256, 192)):
        xd = _r(torch.randn(sizes[0], cin)).cuda().requires_grad_(True)
        wd = _r(torch.randn(27, cin, cout) / (27 * cin) ** 0.5).cuda().requires_grad_(True)
        with _amp():
            out = F.ConvolutionFunction.apply(xd, wd, km, False)
        g = torch.randn(sizes[0], cout, device='cuda').half()
        g[1234, 7] = float('inf')
        out.backward(g)
        assert not bool(torch.isfinite(wd.grad).all()), (cin, cout)
        assert not bool(torch.isfinite(xd.grad[1234]).all()), (cin, cout)      # (the centre offset: row 1234 reads dY[1234])


# ------------------------------------------------------------------ 7. model
def _spvcnn(cr, seed=0):
    from u2mkd_amd import lidar
    torch.manual_seed(seed)
    m = lidar.SPVCNN(cr=cr, in_channel=4, num_classes=17, pres=0.05, vres=0.05).cuda().train()
    m.dropout.p = 0.0
    return m


def _spy_model_step(F):
    """SPVCNN cr = 1.0, one forward + backward under fp16 autocast with every F.L.call counted.  Returns (counts, model,
    fp32 logits, fp16-autocast logits)."""
    from u2mkd_amd import torchsparse as ts
    from u2mkd_amd.losses import MixLovaszCrossEntropy
    b = synth_batch(6000, 1, seed=5)
    feats, coords, labels = (torch.from_numpy(b[k]).cuda() for k in ('feats', 'coords', 'labels'))
    m = _spvcnn(1.0)
    ref = m({'lidar': ts.SparseTensor(feats, coords)})['x_vox'].detach()
    seen = {'conv_f16': 0, 'conv_other': 0, 'bn_rows': [], 'f16': 0, 'bf16': 0}
    real_call = F.L.call

    def spy(name, *a):
        if name.startswith('u2mkd_conv_forward_tiles') or name.startswith('u2mkd_conv_forward_pairs'):
            seen['conv_f16' if name.endswith('_f16') else 'conv_other'] += 1
        if name == 'u2mkd_bn_train_forward':          # (x, res, row dtype, ...)
            seen['bn_rows'].append(a[2])
        seen['f16'] += name.endswith('_f16')
        seen['bf16'] += name.endswith('_bf16')
        return real_call(name, *a)
    F.L.call = spy
    try:
        with _amp():
            out = m({'lidar': ts.SparseTensor(feats, coords)})['x_vox']
            loss = MixLovaszCrossEntropy(ignore_index=0)(out, labels)
        loss.backward()
    finally:
        F.L.call = real_call
    return seen, m, ref, out.detach()


def test_spvcnn_rows_travel_in_f16_and_logits_stay_close_to_fp32(F):
    seen, m, ref, out = _spy_model_step(F)
    # every conv but the 4-channel stem and every BatchNorm ran on fp16 rows, nothing on bf16 rows
    assert seen['conv_f16'] >= 30 and seen['conv_other'] <= 1, seen
    assert len(seen['bn_rows']) >= 40 and set(seen['bn_rows']) == {2}, seen
    assert seen['bf16'] == 0, seen
    assert bool(torch.isfinite(out.float()).all())
    # the bf16 suite's bounds, which fp16's three extra bits can only meet more easily
    d = (out.float() - ref).abs()
    print('logits: max %.4f median %.5f of |ref|.max()' % (float(d.max() / ref.abs().max()), float(d.median() / ref.abs().max())))
    assert float(d.max()) < 0.15 * float(ref.abs().max()) and float(d.median()) < 0.02 * float(ref.abs().max()), \
        (float(d.max()), float(d.median()), float(ref.abs().max()))
    for n, p in m.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), n


def test_the_switch_gives_fp32_rows_back():
    """U2MKD_F16_ROWS=0 (read at import: a fresh process): the same step calls no _f16 entry (and no BatchNorm entry with a
    16-bit row dtype: fp32 rows take the C++ host path or row dtype 0)"""
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n'
            'import torch\n'
            'from u2mkd_amd.torchsparse.nn import functional as F\n'
            'import test_gpu_f16_rows as T\n'
            'seen, m, ref, out = T._spy_model_step(F)\n'
            'assert seen["f16"] == 0 and seen["bf16"] == 0 and seen["conv_other"] >= 30 and set(seen["bn_rows"]) <= {0}, seen\n'
            'assert bool(torch.isfinite(out.float()).all())\n'
            'print("ok")\n') % (ROOT, os.path.join(ROOT, 'tests'))
    env = dict(os.environ, U2MKD_F16_ROWS='0')
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


# ------------------------------------------------------------------ 8. trainer
@pytest.mark.parametrize('amp', ['fp16', True])
def test_lidar_step_trains_under_fp16_amp(hip, amp):
    from u2mkd_amd import lidar, train as T
    b = synth_batch(3000, 1, 9)
    feats, coords, labels = (torch.from_numpy(b[k]).cuda() for k in ('feats', 'coords', 'labels'))
    torch.manual_seed(0)
    model = lidar.SPVCNN(cr=0.5, in_channel=4, num_classes=17, pres=0.05, vres=0.05).cuda().train()
    run = T.LidarStep(model, amp=amp)
    assert run.amp.dtype == torch.float16 and run.amp.scaler.is_enabled()
    before = [p.detach().clone() for p in model.parameters()]
    losses, moved = [], 0
    for _ in range(4):
        losses.append(float(run(feats, coords, labels)))
        now = [p.detach().clone() for p in model.parameters()]
        moved += any(not torch.equal(a, b_) for a, b_ in zip(before, now))
        before = now
    assert all(np.isfinite(v) for v in losses), losses
    scale = float(run.amp.scaler.get_scale())
    assert np.isfinite(scale) and scale > 0, scale
    assert moved >= 1, (moved, scale)      # (a step whose gradients overflowed is skipped and halves the scale: not all four)
    for n, p in model.named_parameters():
        assert bool(torch.isfinite(p).all()), n


# ------------------------------------------------------------------ 9. coherence
def test_one_module_under_bf16_then_fp16_then_bf16_autocast(F):
    """The weight-fragment cache keys on the arith: the fp16 pass neither reads the bf16 plane nor spoils it, and a raw write
    to the kernel (tests/test_gpu_state_coherence.py's kind) invalidates both."""
    from u2mkd_amd import torchsparse as ts
    from u2mkd_amd.torchsparse import nn as spnn
    coords, nbmaps, nbsizes, sizes, _, _ = _scene('subm')
    torch.manual_seed(3)
    conv = spnn.Conv3d(64, 64, 3).cuda()
    x = _r(torch.randn(sizes[0], 64))
    with torch.no_grad():
        first = _under(torch.bfloat16, conv, x, coords, ts)
        second = _under(torch.float16, conv, x, coords, ts)
        third = _under(torch.bfloat16, conv, x, coords, ts)
        assert first.dtype == torch.bfloat16 and second.dtype == torch.float16
        assert torch.equal(third, first)
        # the fp32 result on fp16-rounded rows (the kernel is the module's fp32 parameter as it is)
        want = R.conv_forward(x, conv.kernel.detach().cpu(), nbmaps, nbsizes, sizes, transposed=False)
        print('coherence: fp16 pass %.3f x TOL' % (_err(second, want) / TOL))
        assert _err(second, want) < TOL
        # a raw write, then the announcement the library asks for: both planes are rebuilt.  (x 2 is exact on the bf16 plane;
        # on the fp16 plane it is not where a weight is an fp16 subnormal, |w| < 2^-14: that pass is held to the oracle again)
        conv.kernel.data.mul_(2.0)
        F.invalidate_weight_caches()
        assert _err(_under(torch.float16, conv, x, coords, ts), 2 * want) < TOL
        assert torch.equal(_under(torch.bfloat16, conv, x, coords, ts).float(), 2 * first.float())


def _under(dt, conv, x, coords, ts):
    with torch.autocast('cuda', dtype=dt):
        return conv(ts.SparseTensor(x.cuda(), _dev(coords))).feats


def test_f16_batched_fragments_equal_the_per_weight_launch(F):
    """u2mkd_weight_fragments_batch with fp16 one-plane jobs (planes = 1, column 7 = 1): the same bytes as
    u2mkd_weight_fragments(arith = 5), next to bf16 one-plane (column 7 = 0), bf16x3 and f16x2 jobs in one table -- the
    one-launch refresh behind the optimizer step (tests/test_gpu_conv_f16x2.py has the f16x2 twin)."""
    L = F.L
    lib = L.load()
    st = L.stream()
    torch.manual_seed(12)
    shapes = [(27, 64, 64, 5), (27, 32, 96, 3), (8, 64, 128, 5), (27, 64, 64, 3), (1, 96, 32, 5), (27, 32, 32, 4), (27, 128, 128, 5),
              (8, 32, 64, 2)]
    ref, bufs, rows, first = [], [], [], 0
    for i, (k, r, c, arith) in enumerate(shapes):
        # (magnitudes from 1e-3 to 1e3: fp16 subnormal weights and weights of both signs included, all inside fp16's range)
        w = torch.randn(k, r, c, device='cuda') * 10.0 ** (i - 3 if arith == 5 else 0)
        nbytes = lib.u2mkd_weight_fragments_bytes(k, r, c, arith)
        a = torch.empty(2, nbytes, dtype=torch.uint8, device='cuda')
        L.call('u2mkd_weight_fragments', L.ptr(w), k, r, c, 2, arith, L.ptr(a), st)
        b = torch.full((2, nbytes), 0xA5, dtype=torch.uint8, device='cuda')
        rows.append([w.data_ptr(), b.data_ptr(), first, k, r, c, {2: 3, 3: 1, 4: 2, 5: 1}[arith], int(arith == 5)])
        first += 2 * (k * r * c // 512)
        ref.append((a, w)); bufs.append(b)
    table = torch.tensor(rows, dtype=torch.int64).cuda()
    L.call('u2mkd_weight_fragments_batch', L.ptr(table), len(rows), first, st)
    for (a, w), b, sh in zip(ref, bufs, shapes):
        assert torch.equal(a, b), sh
    # and the arith-5 image is the fp16 plane, not the bf16 one: the same weight laid out as arith 3 differs from it
    k, r, c, _ = shapes[0]
    as3 = torch.empty_like(ref[0][0])
    L.call('u2mkd_weight_fragments', L.ptr(ref[0][1]), k, r, c, 2, 3, L.ptr(as3), st)
    assert as3.shape == ref[0][0].shape and not torch.equal(as3, ref[0][0])


def test_conv3d_f16_rows_follow_an_optimizer_step(F):
    """spnn.Conv3d(64, 64, 3) under fp16 autocast: forward + backward, one SGD step -- whose post hook re-lays the fp16
    fragments of both orientations in ONE u2mkd_weight_fragments_batch launch -- and the next forward and input gradient,
    served by those fragments with no per-weight launch, are held to the fp32 oracle on the UPDATED kernel."""
    from u2mkd_amd import torchsparse as ts
    from u2mkd_amd.torchsparse import nn as spnn
    coords, nbmaps, nbsizes, sizes, _, _ = _scene('subm')
    torch.manual_seed(5)
    conv = spnn.Conv3d(64, 64, 3).cuda()
    opt = torch.optim.SGD(conv.parameters(), lr=0.05)
    x, g = _r(torch.randn(sizes[0], 64)), _r(torch.randn(sizes[0], 64))
    calls = []
    real = F.L.call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)

    def step():
        xd = x.cuda().requires_grad_(True)
        with _amp():
            y = conv(ts.SparseTensor(xd, _dev(coords))).feats
        y.backward(g.cuda().half())
        return y.detach(), xd.grad

    F.L.call = spy
    try:
        w0 = conv.kernel.detach().clone()
        step()
        opt.step()
        after_step = len(calls)
        y, dx = step()
    finally:
        F.L.call = real
    assert calls[:after_step].count('u2mkd_weight_fragments_batch') == 1
    assert 'u2mkd_weight_fragments' in calls[:after_step] and 'u2mkd_weight_fragments' not in calls[after_step:], calls
    assert any(c.endswith('_f16') for c in calls[after_step:])
    w1 = conv.kernel.detach().cpu()
    assert float((w1 - w0.cpu()).abs().max()) > 2.0 ** -6 * float(w1.abs().max())       # the step moved the kernel visibly
    want = R.conv_forward(x, w1, nbmaps, nbsizes, sizes, transposed=False)
    wgi, _ = R.conv_backward(x, w1, g, nbmaps, nbsizes, transposed=False)
    stale = R.conv_forward(x, w0.cpu(), nbmaps, nbsizes, sizes, transposed=False)
    print('after the step: out %.3f dx %.3f x TOL (the kernel before the step: %.1f x TOL)' % (
        _err(y, want) / TOL, _err(dx, wgi) / TOL, _err(y, stale) / TOL))
    assert y.dtype == torch.float16 and _err(y, want) < TOL and _err(dx, wgi) < TOL
