"""torchsparse.nn's BEV modules through the drop-in, on the GPU, against float64 (tests/bev_f64_ref.py): ToBEVReduction,
ToBEVConvolution, ToDenseBEVConvolution and ToBEVHeightCompression on every case of ``bev_f64_ref.CASES`` -- N of 1, 63, 64, 65,
129 and 1500, C of 4, 20 and 64 (and 6: padded), Cout of 4 and 32, 1 / 3 / 31 heights on the conv engine, 32 and 33 on torch
operators, every height axis, a 5 x 7 grid, tensor strides (1, 1, 1) and (2, 2, 1) with offsets, module stride 2, B = 3 with batch
index 1 empty, a full column and a column of one row, clamped heights, negative BEV coordinates, three row types.  Forward,
dfeats, dkernel and dbias under the derived bounds, the torch.equal claims as such, three runs bit for bit, one host read per
plan, out-of-range inputs raise before any store kernel, empty inputs.  tests/test_host_bev_ref.py shows on the same inputs
what the bounds reject.  (16-bit convolution cases run under autocast, where the conv engine keeps 16-bit rows.)"""
import contextlib
import math

import pytest
import torch

import bev_f64_ref as R
import conv_fwd_f64_ref as CR
import wgrad_f64_ref as WR

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DEV = 'cuda'


@pytest.fixture(scope='module')
def env(hip):
    from u2mkd_amd import torchsparse as ts
    import u2mkd_amd.torchsparse.nn as spnn
    from u2mkd_amd.torchsparse.nn import functional as F
    return ts, spnn, F, hip


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a device fault: nothing else of this session may use the GPU
        pytest.exit('GPU fault in %s: %s' % (what, e), returncode=3)


def _judge(what, got, ref, bd):
    ok, worst = R.check(got.detach().cpu(), ref, bd)
    print('\n[bev] %s: largest err / bound %.3f' % (what, worst))
    assert bool(torch.isfinite(got).all()), what
    assert ok, '%s: largest err / bound %.3f' % (what, worst)


def _module(spnn, b):
    m = b['module']
    if m == 'reduction':
        return spnn.ToBEVReduction(dim=b['dim'])
    if m == 'height':
        return spnn.ToBEVHeightCompression(b['c'], b['shape'], offset=b['offset'], dim=b['dim'])
    if m == 'convolution':
        mod = spnn.ToBEVConvolution(b['c'], b['cout'], b['nk'], stride=b['stride'], dim=b['dim'], bias=b['bias'])
    else:
        mod = spnn.ToDenseBEVConvolution(b['c'], b['cout'], b['shape'], offset=b['offset'], dim=b['dim'], bias=b['bias'])
    with torch.no_grad():
        mod.kernel.copy_(b['kernel'])
        if b['bias']:
            mod.bias.copy_(b['bias_t'])
    return mod


def _run(env, b, mod, coords, g=None):
    """one forward (+ backward with ``g``) on the device: (output rows / dense tensor, out coords or None, dfeats, dkernel, dbias)"""
    ts, spnn, F, L = env
    dtype = b['dtype']
    x = b['feats'].to(DEV)
    if b['n'] in (64, 129):                                 # non-contiguous rows: the left half of a wider tensor
        x = torch.cat([x, x], 1)[:, :b['c']]
        assert not x.is_contiguous() or b['n'] == 1
    x = x.detach().requires_grad_(True)
    conv16 = dtype != F32 and b['module'] in ('convolution', 'dense')
    with (torch.autocast('cuda', dtype=dtype) if conv16 else contextlib.nullcontext()):
        out = mod(ts.SparseTensor(x, coords, stride=b['s']))
    oc = None
    if b['module'] in ('reduction', 'convolution'):
        assert out.stride == tuple(b['s'][k] * b['stride'] for k in range(3)) and not out.cmaps and not out.kmaps
        out, oc = out.feats, out.coords
    _sync('%s forward' % b['name'])
    assert out.dtype == dtype, (out.dtype, dtype)
    grads = (None, None, None)
    if g is not None:
        for p in mod.parameters():
            p.grad = None
        out.backward(g.to(DEV))
        _sync('%s backward' % b['name'])
        assert x.grad.dtype == dtype
        grads = (x.grad, getattr(mod, 'kernel', None) is not None and mod.kernel.grad,
                 b['bias'] and mod.bias.grad)
    return out.detach(), oc, grads


def _f64(b, x, k, bias):
    m = b['module']
    if m == 'reduction':
        oc, out, mag, cnt = R.reduction64(x, b['coords'], b['dim'])
        return dict(oc=oc, out=out, mag=mag, cnt=cnt)
    if m == 'convolution':
        oc, out, mag, cnt, inv, z = R.convolution64(x, b['coords'], b['s'], k, bias, b['stride'], b['dim'])
        return dict(oc=oc, out=out, mag=mag, cnt=cnt, group=inv, z=z)
    if m == 'dense':
        out, mag, cnt, cell, z = R.dense_convolution64(x, b['coords'], b['s'], k, bias, b['shape'], b['offset'], b['dim'])
        return dict(out=out, mag=mag, cnt=cnt, group=cell, z=z)
    out, mag, cnt = R.height_compression64(x, b['coords'], b['s'], b['shape'], b['offset'], b['dim'])
    return dict(out=out, mag=mag, cnt=cnt)


def _rows_of(t, dense):
    """[n_out, Cout] rows of a result (dense: NCHW -> cells)"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) if dense else t


def _unit_like(t, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(t.shape, generator=g).to(dtype)


def _check_conv(b, f, x, kr, g_rows, out_rows, dx, dk, db, engine, plan):
    """the convolution part of ToBEVConvolution / ToDenseBEVConvolution against float64 under the bounds of the kernel family"""
    dtype, nk, n = b['dtype'], b['nk'], b['n']
    n_out = f['cnt'].shape[0]
    group, z = f['group'], f['z']
    ref_rows = _rows_of(f['out'].detach(), b['module'] == 'dense')
    bias_mag = f['cnt'][:, None] * b['bias_t'].double().abs() if b['bias'] else None
    if engine:
        nbr = R.neighbour_table(group, z, nk, n_out)
        assert torch.equal(plan.kmap.nbr.cpu(), nbr), 'the plan\'s neighbour table'
        inv_tbl = plan.kmap.nbr_inv.cpu()
        assert torch.equal(inv_tbl[z, torch.arange(n)], group.int()) and int((inv_tbl >= 0).sum()) == n
        for what, cin, cout, src, role, n_rows, got, bm in (('forward', b['c'], b['cout'], x, 'fwd', n_out, out_rows, bias_mag),
                                                            ('dfeats', b['cout'], b['c'], g_rows, 'inv', n, dx, None)):
            fam = R.conv_family(cin, cout, dtype, n_rows, nk)
            ref, mag, part = CR.reference(src, kr, nbr, n, role, nominal=dtype == F16)
            plain = CR.reference(src, kr, nbr, n, role)[1] if dtype == F16 else mag
            r = CR.rel_err(CR.honest_fp32(src, kr, nbr, n, role, running=fam[0] == 'u2mkd_conv_forward_sorted'), ref, plain)
            bd = R.conv_bound(fam[1], mag, r, ref, part, dtype, nk, bm)
            if what == 'forward':      # the two float64 statements agree: the table's and the module's
                want = ref + (f['cnt'][:, None] * b['bias_t'].double() if b['bias'] else 0)
                assert torch.allclose(want, ref_rows, rtol=1e-12, atol=0)
                ref = ref_rows
            _judge('%s %s %s' % (b['name'], what, fam[0][6:]), got, ref, bd)
            assert int(torch.count_nonzero(got.cpu()[(mag == 0).all(1) & ((bm is None) or (bm == 0).all(1))])) == 0
    else:
        total = f['mag'] if b['module'] == 'convolution' else _rows_of(f['mag'], True)
        honest = R.honest_rows_fp32(x, kr, b['bias_t'] if b['bias'] else 0, z, group, n_out)
        r = CR.rel_err(honest, ref_rows, total)
        _judge('%s forward (torch operators) r 2^%.1f' % (b['name'], math.log2(max(r, 1e-300))), out_rows, ref_rows,
               R.store_rounding(CR.bound('f32', total, r), ref_rows, dtype))
        # dfeats_r = g[group_r] @ kernel[z_r]^T: one chain per row
        gr = g_rows.double()[group]
        kz = kr.double()[z]
        ref = torch.bmm(gr[:, None, :], kz.transpose(1, 2))[:, 0, :]
        mag = torch.bmm(gr.abs()[:, None, :], kz.abs().transpose(1, 2))[:, 0, :]
        hon = torch.zeros(n, b['c'])
        for kk in range(nk):
            rows = torch.nonzero(z == kk)[:, 0]
            if len(rows):
                hon[rows] = CR._chain(torch.zeros(len(rows), b['c']), g_rows.float()[group][rows], kr.float()[kk].t())
        _judge('%s dfeats (torch operators)' % b['name'], dx, ref,
               R.store_rounding(CR.bound('f32', mag, CR.rel_err(hon, ref, mag)), ref, dtype))
    # dkernel over the (input row, output row) pairs of every height
    pairs, counts = R.pair_list(group, z, nk)
    dw, wmag = WR.wgrad_f64(x, g_rows, pairs, counts, 0)
    fam_w = WR.family(R.pad4(b['c']), R.pad4(b['cout']), dtype if engine else F32)
    T = WR.T_X3 if (engine and fam_w[0] == 'x3' and dtype == F32) else WR.T_EXACT
    if fam_w[0] == 'x3' and dtype == F16:
        wmag = WR.wgrad_f64(WR.nominal_fp16(x), WR.nominal_fp16(g_rows), pairs, counts, 0)[0]
    r = WR.rel_err(WR.honest_fp32(x, g_rows, pairs, counts, 0), dw, WR.wgrad_f64(x, g_rows, pairs, counts, 0)[1])
    ok, worst, _ = WR.check(dk.cpu(), dw, wmag, T, r)
    print('\n[bev] %s dkernel %s: largest err / bound %.3f' % (b['name'], fam_w[0], worst))
    assert ok and dk.dtype == F32, '%s dkernel: largest err / bound %.3f' % (b['name'], worst)
    if b['bias']:
        # dbias = sum over the input rows of g[group_r] = sum over the cells of m g: exact products, one sum
        gd = g_rows.double()
        ref = (f['cnt'][:, None] * gd).sum(0, keepdim=True)
        mag = (f['cnt'][:, None] * gd.abs()).sum(0, keepdim=True)
        if engine:
            bd = R.U32 * mag                               # summed in double, rounded once
        else:
            seq = torch.zeros(1, b['cout'])
            for row in g_rows.float()[group]:
                seq += row
            bd = CR.bound('f32', mag, CR.rel_err(seq, ref, mag))
        _judge('%s dbias' % b['name'], db, ref, bd)


@pytest.mark.parametrize('name', [c['name'] for c in R.CASES])
def test_case_against_float64(env, name):
    ts, spnn, F, L = env
    b = R.build(R.CASE[name])
    dtype, m = b['dtype'], b['module']
    dense = m in ('dense', 'height')
    mod = _module(spnn, b).to(DEV)
    coords = b['coords'].to(DEV)                              # a fresh coordinate tensor: no plan on it yet
    x = b['feats']
    kr = b['kernel'].to(dtype).float() if (m in ('convolution', 'dense') and dtype != F32) else b.get('kernel')
    engine = m in ('convolution', 'dense') and b['nk'] <= R.ENGINE_MAX_K and b['stride'] == 1
    if m in ('convolution', 'dense') and dtype != F32 and not engine:
        kr = b['kernel']
    # float64: forward, and autograd through it for the gradients
    x64 = x.double().requires_grad_(True)
    f = _f64(b, x64, kr, b.get('bias_t', 0))
    g = _unit_like(f['out'], dtype, 5)
    f['out'].backward(g.double())
    out, oc, (dx, dk, db) = _run(env, b, mod, coords, g)
    assert out.shape == f['out'].shape
    if oc is not None:
        assert torch.equal(oc.cpu(), f['oc']) and oc.dtype == torch.int32      # rows sorted by (b, x, y, z)
    if dense:
        assert out.shape[0] == 3 and int(torch.count_nonzero(out[1])) == 0 or b['n'] == 1       # batch index 1 has no rows
    ref = f['out'].detach()
    if m == 'reduction':
        _judge(name + ' forward', out, ref, R.mean_bound(ref, dtype))
        _judge(name + ' dfeats', dx, x64.grad, R.mean_bound(x64.grad, dtype))
    elif m == 'height':
        bd = R.dense_store_bound(ref, f['mag'], f['cnt'], dtype)
        _judge(name + ' forward', out, ref, bd)
        one = f['cnt'] == 1
        assert bool(one.any()) and torch.equal(out.cpu()[one].double(), ref[one])          # a slot fed by one row IS that row
        assert int(torch.count_nonzero(out.cpu()[f['cnt'] == 0])) == 0
        if b['beyond'] and b['n'] > 3:
            assert int(f['cnt'].max()) > 1, 'the clamp puts several rows on one (cell, w)'
        assert torch.equal(dx.cpu().double(), x64.grad)                                   # the gather is a copy
    else:
        plan_name = [k for k in coords.__dict__['_u2mkd_plans'] if k.startswith('bev_')]
        assert len(plan_name) == 1
        plan = coords.__dict__['_u2mkd_plans'][plan_name[0]][1]
        assert (plan.kmap is not None) == engine
        g_rows = _rows_of(g, m == 'dense')
        _check_conv(b, f, x, kr, g_rows, _rows_of(out, m == 'dense'), dx, dk, db, engine, plan)
    # three runs, the same bits
    for _ in range(2):
        out2, oc2, (dx2, dk2, db2) = _run(env, b, mod, coords, g)
        assert torch.equal(out, out2) and torch.equal(dx, dx2)
        if dk is not False and dk is not None:
            assert torch.equal(dk, dk2)
        if b['bias']:
            assert torch.equal(db, db2)


@pytest.mark.parametrize('dtype', [F32, BF16, F16], ids=['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('c', [4, 20, 64, 132])
@pytest.mark.parametrize('grid', [(5, 7), (9, 15)], ids=lambda v: '%dx%d' % v)
def test_dense_store_and_gather_are_copies(env, dtype, c, grid):
    """u2mkd_bev_dense_store / _gather with the rows as the cells: NHWC <-> NCHW, bit for bit (35 cells: less than a tile; 135:
    two tiles and a tail; 132 channels: two channel chunks, the second a partial one)"""
    ts, spnn, F, L = env
    h, w = grid
    rows = CR.make_rows('rows', 3 * h * w, c, dtype, seed=2).to(DEV).requires_grad_(True)
    out = F.BevDenseFunction.apply(rows, None, None, 3, 1, h, w, dtype)
    _sync('dense store')
    assert torch.equal(out, rows.detach().view(3, h, w, c).permute(0, 3, 1, 2))
    g = torch.randn(3, c, h, w, device=DEV).to(dtype)
    out.backward(g)
    _sync('dense gather')
    assert torch.equal(rows.grad, g.permute(0, 2, 3, 1).reshape(-1, c))


def _counting(monkeypatch, F):
    calls = []
    real = F.read_counts

    def counting(tensors):
        calls.append(len(tensors))
        return real(tensors)
    monkeypatch.setattr(F, 'read_counts', counting)
    return calls


@pytest.mark.parametrize('name', ['red-n129', 'conv-n65', 'dense-n65', 'height-n129'])
def test_second_module_reads_nothing_from_the_device(env, monkeypatch, name):
    ts, spnn, F, L = env
    calls = _counting(monkeypatch, F)
    b = R.build(R.CASE[name])
    coords = b['coords'].to(DEV)
    a, c = _module(spnn, b).to(DEV), _module(spnn, b).to(DEV)
    g = _unit_like(_f64(b, b['feats'], b.get('kernel'), b.get('bias_t', 0))['out'], b['dtype'], 1)
    _run(env, b, a, coords, g)
    assert len(calls) == 1, 'the plan reads its flag / count block once'
    _run(env, b, c, coords, g)
    _run(env, b, a, coords, g)
    assert len(calls) == 1, 'a second module, a second step and the backward over the same coordinates read nothing'


class _Spy:
    def __init__(self, L):
        self.L, self.names = L, []

    def __enter__(self):
        self.orig = self.L.call
        self.L.call = lambda name, *a: (self.names.append(name), self.orig(name, *a))[1]
        return self

    def __exit__(self, *exc):
        self.L.call = self.orig


def _broken(b, how):
    c = b['coords'].clone()
    b0, b1 = R.bev_axes(b['dim'])
    if how == 'u':
        c[-1, b0] = b['offset'][b0] + 5 * b['s'][b0]                # u = H
    elif how == 'v-negative':
        c[-1, b1] = b['offset'][b1] - b['s'][b1]                    # v = -1
    elif how == 'height':
        c[-1, b['dim']] = b['nk'] * b['s'][b['dim']]                # z = n_kernels
    elif how == 'height-negative':
        c[-1, b['dim']] = -b['s'][b['dim']]
    elif how == 'batch':
        c[-1, 3] = -1
    return c


@pytest.mark.parametrize('name,how', [('dense-n65', 'u'), ('dense-n64', 'v-negative'), ('dense-n65', 'height'), ('dense-n65', 'batch'),
                                      ('height-n129', 'u'), ('height-n63', 'v-negative'), ('conv-n65', 'height'),
                                      ('conv-n64', 'height-negative'), ('conv-stride2', 'height')])
def test_out_of_range_raises_before_any_store(env, name, how):
    ts, spnn, F, L = env
    b = R.build(R.CASE[name])
    mod = _module(spnn, b).to(DEV)
    coords = _broken(b, how).to(DEV)
    with _Spy(L) as spy:
        with pytest.raises(ValueError, match='out of range'):
            mod(ts.SparseTensor(b['feats'].to(DEV), coords, stride=b['s']))
    _sync('out of range')
    assert 'u2mkd_bev_plan' in spy.names
    assert not [n for n in spy.names if 'dense_store' in n or n.startswith('u2mkd_conv') or 'segment' in n], spy.names


def test_height_compression_clamps_and_does_not_check_the_height(env):
    ts, spnn, F, L = env
    b = R.build(R.CASE['height-n129'])
    c = b['coords'].clone()
    c[0, b['dim']] = -7 * b['s'][b['dim']]
    c[1, b['dim']] = 1000
    b['coords'] = c
    out, _, _ = _run(env, b, _module(spnn, b).to(DEV), c.to(DEV))
    f = _f64(b, b['feats'], None, 0)
    _judge('clamped heights', out, f['out'], R.dense_store_bound(f['out'], f['mag'], f['cnt'], F32))


@pytest.mark.parametrize('name', ['red-n63', 'conv-n65', 'dense-n65', 'height-n63'])
def test_empty_input(env, name):
    ts, spnn, F, L = env
    b = R.build(R.CASE[name])
    mod = _module(spnn, b).to(DEV)
    x = torch.zeros(0, b['c'], device=DEV, requires_grad=True)
    out = mod(ts.SparseTensor(x, torch.zeros(0, 4, dtype=torch.int32, device=DEV), stride=b['s']))
    if b['module'] in ('reduction', 'convolution'):
        assert out.feats.shape == (0, b['cout'] or b['c']) and out.coords.shape == (0, 4) and out.coords.dtype == torch.int32
    else:
        ch = b['cout'] if b['module'] == 'dense' else b['c'] * b['nk']
        assert out.shape == (0, ch, 5, 7)
    _sync('empty input')


def test_functional_forms_take_the_modules_tensors(env):
    ts, spnn, F, L = env
    b = R.build(R.CASE['dense-n65'])
    mod = _module(spnn, b).to(DEV)
    x = ts.SparseTensor(b['feats'].to(DEV), b['coords'].to(DEV), stride=b['s'])
    assert torch.equal(mod(x), F.to_dense_bev_convolution(x, mod.kernel, mod.bias, b['shape'], mod.offset, b['dim']))
    hc = spnn.ToBEVHeightCompression(b['c'], b['shape'], b['offset'], b['dim'])
    assert torch.equal(hc(x), F.to_bev_height_compression(x, b['c'], b['shape'], b['offset'], b['dim']))
    cv = spnn.ToBEVConvolution(b['c'], b['cout'], b['nk'], bias=True).to(DEV)
    assert torch.equal(cv(x).feats, F.to_bev_convolution(x, cv.kernel, cv.bias, 1, 1).feats)
    assert torch.equal(spnn.ToBEVReduction(2)(x).feats, F.to_bev_reduction(x, 2).feats)
    _sync('functional forms')
