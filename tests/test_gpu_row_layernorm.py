"""Row LayerNorm on the device (csrc/ln.hip; u2mkd_ln_forward, u2mkd_ln_add_forward, u2mkd_ln_backward; RowLayerNorm and
SphereFormer over them).

  1  every output of every lane-group form, for the three row types, inside the derived float64 bound of
     tests/row_ln_f64_ref.py with no element excluded, and the largest error at most twice that of torch's own formulation
     (F.layer_norm on the upcast rows, rounded to the row type; torch's backward) or one unit in the last place.
  2  n = 0 launches nothing; an unsupported width is refused by the entry and runs torch's route in the module.
  3  the add form: the stream row is the fp32 sum rounded once, normed is the plain form on the stored stream bit for bit, the
     fused backward is the float64 gradient with both consumers present, d_branch = w_row d_shortcut.
  4  the same bits run after run, on another stream and in fresh tensors.
  5  the SphereFormer block: 16-bit rows out of norm1 / norm2 under autocast, as close to a float64 evaluation of the block as
     the formulation over torch's layer_norm, DropPath's mask unchanged, a frozen teacher that repeats itself."""
import contextlib

import numpy as np
import pytest
import torch

import row_ln_f64_ref as R
from oracle import sptr_ref as S

pytestmark = pytest.mark.gpu

F = torch.nn.functional
CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
SENTINEL = 12288.0                                     # (exact in bf16 and fp16)


@pytest.fixture(autouse=True)
def _row_kernels_on(monkeypatch):
    """every test here runs with the row kernels switched on for the three row types (U2MKD_ROW_LN=1), whatever the defaults are;
    the block tests switch them off again for the formulation they compare against"""
    from u2mkd_amd.torchsparse.nn import functional as spf
    monkeypatch.setattr(spf, '_ROW_LN_ON', {k: True for k in spf._ROW_LN_ON})


def _f32(n, dev='cuda'):
    return torch.empty(n, dtype=torch.float32, device=dev)


def _forward(L, x, gamma, beta, stats=True):
    n, c = x.shape
    y = torch.empty_like(x)
    mean, rstd = (_f32(n), _f32(n)) if stats else (None, None)
    L.call('u2mkd_ln_forward', L.ptr(x), CODE[x.dtype], n, c, L.ptr(gamma), L.ptr(beta), R.EPS, L.ptr(mean), L.ptr(rstd), L.ptr(y),
           L.stream())
    return y, mean, rstd


def _add_forward(L, a, b, w, gamma, beta, stats=True):
    n, c = a.shape
    s, y = torch.empty_like(a), torch.empty_like(a)
    mean, rstd = (_f32(n), _f32(n)) if stats else (None, None)
    L.call('u2mkd_ln_add_forward', L.ptr(a), L.ptr(b), L.ptr(w), CODE[a.dtype], n, c, L.ptr(gamma), L.ptr(beta), R.EPS, L.ptr(mean),
           L.ptr(rstd), L.ptr(s), L.ptr(y), L.stream())
    return s, y, mean, rstd


def _backward(L, dy, x, mean, rstd, gamma, ds=None, w=None):
    n, c = x.shape
    slabs = L.load().u2mkd_ln_num_slabs(n, c)
    assert slabs == -(-n // R.SLAB_ROWS)
    partial = _f32(max(slabs, 1) * 2 * c)
    out = {'dx': torch.empty_like(x), 'dgamma': _f32(c), 'dbeta': _f32(c)}
    if w is not None:
        out['db'] = torch.empty_like(x)
    L.call('u2mkd_ln_backward', L.ptr(dy), L.ptr(x), L.ptr(ds), L.ptr(w), CODE[x.dtype], n, c, L.ptr(mean), L.ptr(rstd), L.ptr(gamma),
           L.ptr(partial), L.ptr(out['dgamma']), L.ptr(out['dbeta']), L.ptr(out['dx']), L.ptr(out.get('db')), L.stream())
    return out


def _torch_formulation(x, dy, gamma, beta):
    """torch's own: F.layer_norm on the upcast rows, the result rounded to the row type; torch's backward"""
    xt = x.float().requires_grad_(True)
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.layer_norm(xt, (x.shape[1],), gm, bt, R.EPS).to(x.dtype)
    y.backward(dy)
    return {'y': y.detach(), 'dx': xt.grad.to(x.dtype), 'dgamma': gm.grad, 'dbeta': bt.grad}


def _cuda(case):
    return {k: v.cuda() for k, v in case.items()}


# ------------------------------------------------------------------ 1. every output against float64
@pytest.mark.parametrize('tag', list(R.DTYPES))
@pytest.mark.parametrize('c', R.CS)
def test_every_output_inside_the_float64_bound_and_within_twice_torchs_error(hip, c, tag):
    """Every element of every output of every (n, kind) inside the derived bound, and per case -- (n, c, kind, row type, output) --
    the kernel's largest error at most twice that of torch's formulation on the same inputs, or one floor (one unit in the last
    place of the output's type at the case's largest reference magnitude), whichever is larger.  Figures of this test on the
    MI355X: NOTES N17.2."""
    L, dt = hip, R.DTYPES[tag]
    lines, failed = [], []
    for n in R.NS:
        for kind in R.KINDS:
            case = _cuda(R.make_case(n, c, kind, dt))
            x, dy, gm, bt = case['x'], case['dy'], case['gamma'], case['beta']
            y, mean, rstd = _forward(L, x, gm, bt)
            y_nostats, _, _ = _forward(L, x, gm, bt, stats=False)
            f = R.forward64(x, gm, bt)
            got = dict(_backward(L, dy, x, mean, rstd, gm), y=y)
            b = R.backward64(dy, x, gm)
            ref = dict({k: b[k] for k in ('dx', 'dgamma', 'dbeta')}, y=f['y'])
            bound = dict(R.backward_bound(dy, x, gm, dt, b=b), y=R.forward_bound(x, gm, bt, dt, f=f))
            tch = _torch_formulation(x, dy, gm, bt)
            torch.cuda.synchronize()
            assert torch.equal(y, y_nostats), (n, kind)              # NULL mean / rstd: the same rows
            # the saved statistics themselves: steps 1 and 4 of the bound
            dm, _, dr, _ = R._stat_errors(x, f, R.EPS)
            assert bool(((mean.double()[:, None] - f['mu']).abs() <= dm).all()), (n, kind)
            assert bool(((rstd.double()[:, None] - f['r']).abs() <= dr).all()), (n, kind)
            for name in ('y', 'dx', 'dgamma', 'dbeta'):
                ok, over, e_k = R.worst(got[name], ref[name], bound[name])
                e_t = float((tch[name].double() - ref[name]).abs().max())
                floor = R.floor_ulp(ref[name], got[name].dtype)
                lines.append('n=%-5d %-8s %-7s err/bound %.3f  kernel %.3e  torch %.3e  floor %.3e  ratio %.2f'
                             % (n, kind, name, over, e_k, e_t, floor, e_k / max(e_t, floor, 1e-300)))
                if not ok or not e_k <= max(2.0 * e_t, floor):
                    failed.append(lines[-1])
            # the fused form of the backward: + ds, db = w dx
            got = _backward(L, dy, x, mean, rstd, gm, ds=case['ds'], w=case['w'])
            b = R.backward64(dy, x, gm, ds=case['ds'], w=case['w'])
            bound = R.backward_bound(dy, x, gm, dt, ds=case['ds'], w=case['w'], b=b)
            for name in ('dx', 'db', 'dgamma', 'dbeta'):
                ok, over, e_k = R.worst(got[name], b[name], bound[name])
                lines.append('n=%-5d %-8s %-7s err/bound %.3f  kernel %.3e  (fused: + ds, w)' % (n, kind, name, over, e_k))
                if not ok:
                    failed.append(lines[-1])
    print('\nc=%d %s\n%s' % (c, tag, '\n'.join(lines)))
    assert not failed, failed


# ------------------------------------------------------------------ 2. nothing to do, and widths the kernels do not take
@pytest.mark.parametrize('tag', list(R.DTYPES))
def test_an_empty_batch_launches_nothing(hip, tag):
    L, dt = hip, R.DTYPES[tag]
    x = torch.empty(0, 64, dtype=dt, device='cuda')
    gm, bt = torch.ones(64, device='cuda'), torch.zeros(64, device='cuda')
    assert L.load().u2mkd_ln_num_slabs(0, 64) == 0
    y, mean, rstd = _forward(L, x, gm, bt)
    s, y2, _, _ = _add_forward(L, x, x, None, gm, bt)
    out = {'dgamma': torch.full((64,), SENTINEL, device='cuda'), 'dbeta': torch.full((64,), SENTINEL, device='cuda')}
    L.call('u2mkd_ln_backward', None, None, None, None, CODE[dt], 0, 64, None, None, L.ptr(gm), None, L.ptr(out['dgamma']),
           L.ptr(out['dbeta']), None, None, L.stream())
    torch.cuda.synchronize()
    assert y.shape == (0, 64) and bool((out['dgamma'] == SENTINEL).all()) and bool((out['dbeta'] == SENTINEL).all())
    # the module: empty rows out, zero parameter gradients
    from u2mkd_amd.lidar.blocks import RowLayerNorm
    m = RowLayerNorm(64).cuda()
    xin = torch.empty(0, 64, dtype=dt, device='cuda', requires_grad=True)
    with (torch.autocast('cuda', dt) if dt != torch.float32 else contextlib.nullcontext()):
        stream, normed = m.add_norm(xin, xin)
        out = m(xin)
    (out.sum() + normed.sum() + stream.sum()).backward()
    assert out.shape == (0, 64) and out.dtype == dt and xin.grad.shape == (0, 64)
    assert float(m.weight.grad.abs().max()) == 0.0 and float(m.bias.grad.abs().max()) == 0.0


def test_an_unsupported_width_is_refused_by_the_entries_and_runs_torchs_route_in_the_module(hip, monkeypatch):
    L = hip
    from u2mkd_amd.lidar.blocks import RowLayerNorm
    lib = L.load()
    for c in (36, 24, 1032):
        x = torch.randn(5, c, device='cuda')
        y = torch.full_like(x, SENTINEL)
        gm, bt = torch.ones(c, device='cuda'), torch.zeros(c, device='cuda')
        rc = lib.u2mkd_ln_forward(L.ptr(x), 0, 5, c, L.ptr(gm), L.ptr(bt), R.EPS, None, None, L.ptr(y), L.stream())
        msg = lib.u2mkd_last_error().decode()
        rc2 = lib.u2mkd_ln_add_forward(L.ptr(x), L.ptr(x), None, 0, 5, c, L.ptr(gm), L.ptr(bt), R.EPS, None, None, L.ptr(y), L.ptr(y),
                                       L.stream())
        rc3 = lib.u2mkd_ln_backward(L.ptr(x), L.ptr(x), None, None, 0, 5, c, L.ptr(gm), L.ptr(gm), L.ptr(gm), L.ptr(y), L.ptr(y),
                                    L.ptr(y), L.ptr(y), None, L.stream())
        torch.cuda.synchronize()
        assert (rc, rc2, rc3) == (3, 3, 3) and 'not supported' in msg, (rc, rc2, rc3, msg)
        assert bool((y == SENTINEL).all())
    calls, real = [], L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    torch.manual_seed(36)
    ours, ref = RowLayerNorm(36).cuda(), torch.nn.LayerNorm(36).cuda()
    with torch.no_grad():
        ours.weight.normal_(1.0, 0.5)
        ours.bias.normal_()
    ref.load_state_dict(ours.state_dict())
    x = torch.randn(257, 36, device='cuda')
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = ours(xa), ref(xb)
    g = torch.randn_like(ya)
    ya.backward(g)
    yb.backward(g)
    assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
    assert torch.equal(ours.weight.grad, ref.weight.grad) and torch.equal(ours.bias.grad, ref.bias.grad)
    assert not calls, calls
    # ... and so do rows that are not contiguous
    wide = torch.randn(64, 128, device='cuda')
    ours64, ref64 = RowLayerNorm(64).cuda(), torch.nn.LayerNorm(64).cuda()
    assert torch.equal(ours64(wide[:, :64]), ref64(wide[:, :64])) and not calls, calls
    ours64(wide[:, :64].contiguous())
    assert calls == ['u2mkd_ln_forward'], calls


# ------------------------------------------------------------------ 3. the add form
def _amp(dt):
    return torch.autocast('cuda', dt) if dt != torch.float32 else contextlib.nullcontext()


@pytest.mark.parametrize('with_w', [False, True], ids=['plain', 'row_scale'])
@pytest.mark.parametrize('tag', list(R.DTYPES))
def test_add_form_stream_normed_and_the_fused_backward(hip, monkeypatch, tag, with_w):
    L, dt = hip, R.DTYPES[tag]
    from u2mkd_amd.lidar.blocks import RowLayerNorm
    calls, real = [], L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    lines, failed = [], []
    for n, c in ((7, 40), (257, 64), (4099, 256), (64, 1024)):
        case = _cuda(R.make_case(n, c, 'randn', dt, seed=3))
        a, b, gm, bt = case['a'], case['b'], case['gamma'], case['beta']
        w = case['w'] if with_w else None
        # the entries: the stream row and LN of the STORED stream row
        s, y, mean, rstd = _add_forward(L, a, b, w, gm, bt)
        y_plain, mean_plain, rstd_plain = _forward(L, s, gm, bt)
        if w is None:
            want = (a.float() + b.float()).to(dt)
        else:
            want = R.stream64(a, b, w, dt)
            # (torch.addcmul on the upcast rows is the same fp32 expression; it may or may not be contracted to one fma)
            lines.append('n=%d c=%d: stream rows that differ from torch.addcmul in fp32, rounded: %d' % (
                n, c, int((torch.addcmul(a.float(), b.float(), w[:, None]).to(dt) != s).sum())))
        assert torch.equal(s, want), (n, c)
        assert torch.equal(y, y_plain) and torch.equal(mean, mean_plain) and torch.equal(rstd, rstd_plain), (n, c)
        # the module: two outputs, both consumed; one fused pass back
        m = RowLayerNorm(c).cuda()
        with torch.no_grad():
            m.weight.copy_(gm)
            m.bias.copy_(bt)
        ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        row_scale = None if w is None else w[:, None].to(dt)
        wk = None if w is None else row_scale.float().reshape(-1)      # (mask / keep as the module is handed it: in the row type)
        del calls[:]
        with _amp(dt):
            stream, normed = m.add_norm(ar, br, row_scale)
        assert stream.dtype == dt and normed.dtype == dt
        s_ref = s if w is None else _add_forward(L, a, b, wk, gm, bt)[0]
        assert torch.equal(stream, s_ref) and torch.equal(normed, _forward(L, s_ref, gm, bt)[0])
        g1, g2 = case['ds'], case['dy']
        del calls[:]
        ((stream.float() * g1.float()).sum() + (normed.float() * g2.float()).sum()).backward()
        torch.cuda.synchronize()
        assert calls == ['u2mkd_ln_backward'], calls
        ref = R.backward64(g2, s_ref, gm, ds=g1, w=wk)
        bound = R.backward_bound(g2, s_ref, gm, dt, ds=g1, w=wk, b=ref)
        got = {'dx': ar.grad, 'dgamma': m.weight.grad, 'dbeta': m.bias.grad, 'db': br.grad}
        for name in ('dx', 'dgamma', 'dbeta') + (('db',) if with_w else ()):
            ok, over, e_k = R.worst(got[name], ref[name], bound[name])
            lines.append('n=%d c=%d %-7s err/bound %.3f  kernel %.3e' % (n, c, name, over, e_k))
            if not ok:
                failed.append(lines[-1])
        if with_w:
            # d_branch = w_row d_shortcut: both are one rounding of the row type away from fp32 values that differ by one fp32
            # rounding (fp32 rows: the same product, exactly)
            prod = wk[:, None].double() * ar.grad.double()
            if dt == torch.float32:
                assert torch.equal(br.grad, wk[:, None] * ar.grad), (n, c)
            else:
                tol = (2 * R.ROW_UNIT[dt] + 2 * R.U32) * prod.abs() + 2 * R.TINY[dt]
                assert bool(((br.grad.double() - prod).abs() <= tol).all()), (n, c)
            assert float(br.grad[wk == 0].abs().sum()) == 0.0      # a dropped row's branch gets no gradient
        else:
            assert torch.equal(ar.grad, br.grad)
    print('\n%s %s\n%s' % (tag, 'row_scale' if with_w else 'plain', '\n'.join(lines)))
    assert not failed, failed


def test_double_backward_takes_torchs_route(hip):
    """create_graph: the backward is torch's differentiable formulation, so a gradient of a gradient exists and agrees with
    nn.LayerNorm's -- two fp32 evaluations of one expression three derivatives deep, held to 2^-24 x 2^10 of its largest value"""
    from u2mkd_amd.lidar.blocks import RowLayerNorm
    torch.manual_seed(5)
    ours, ref = RowLayerNorm(64).cuda(), torch.nn.LayerNorm(64).cuda()
    with torch.no_grad():
        ours.weight.normal_(1.0, 0.5)
        ours.bias.normal_()
    ref.load_state_dict(ours.state_dict())
    x, a = torch.randn(33, 64, device='cuda'), torch.randn(33, 64, device='cuda')
    res = []
    for m in (ours, ref):
        xi = x.clone().requires_grad_(True)
        (gx,) = torch.autograd.grad((m(xi) * a).sum(), xi, create_graph=True)
        (ggx,) = torch.autograd.grad((gx ** 2).sum(), xi)
        res.append(ggx)
    scale = float(res[1].abs().max())
    assert scale > 1e-2 and float((res[0] - res[1]).abs().max()) <= 2.0 ** -14 * scale


# ------------------------------------------------------------------ 4. the same bits every time
def test_the_same_bits_run_after_run_on_another_stream_and_in_fresh_tensors(hip):
    L = hip
    for tag in R.DTYPES:
        dt = R.DTYPES[tag]
        case = _cuda(R.make_case(4099, 256, 'randn', dt, seed=9))
        a, b, w, gm, bt = case['a'], case['b'], case['w'], case['gamma'], case['beta']

        def run(copy=False):
            a_, b_, w_, gm_, bt_, dy_, ds_ = [t.clone() if copy else t for t in (a, b, w, gm, bt, case['dy'], case['ds'])]
            s, y, mean, rstd = _add_forward(L, a_, b_, w_, gm_, bt_)
            out = _backward(L, dy_, s, mean, rstd, gm_, ds=ds_, w=w_)
            return dict(out, s=s, y=y, mean=mean, rstd=rstd)

        first = run()
        for _ in range(2):
            again = run()
            assert all(torch.equal(first[k], again[k]) for k in first), tag
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            other = run(copy=True)
        side.synchronize()
        assert all(torch.equal(first[k], other[k]) for k in first), tag


# ------------------------------------------------------------------ 5. the block
WINDOW, WINDOW_SPHERE, A = np.array([0.3, 0.3, 0.3], dtype=np.float32), np.array([2.0, 2.0, 120.0]), 0.0125


def _scene():
    g = torch.Generator().manual_seed(11)
    n = 3000
    xyz = torch.rand(n, 3, generator=g) * torch.tensor([3.0, 3.0, 1.0]) + torch.tensor([2.0, -1.5, -0.5])
    b = torch.sort(torch.randint(0, 2, (n,), generator=g))[0].int()
    return n, xyz, b, torch.randn(n, 64, generator=g), torch.randn(n, 64, generator=g)


def _make_block(drop_path=0.0):
    from u2mkd_amd.lidar import sphereformer as SF
    torch.manual_seed(64)
    block = SF.SphereFormer(64, 4, WINDOW.copy(), WINDOW_SPHERE.copy(), WINDOW / 24, WINDOW_SPHERE / 24, drop_path=drop_path, a=A).cuda()
    with torch.no_grad():
        for name, p in block.named_parameters():
            if 'table' in name:
                torch.nn.init.normal_(p, std=0.2)
            elif name.startswith('norm'):
                p.add_(0.3 * torch.randn_like(p))
    return block


def _block_float64(block, x, g, xyz, b, w1=None, w2=None):
    """float64 autograd evaluation of the block (spherical_transformer.py:192-229, 316-348 over oracle.sptr_ref, CPU) on the rows
    ``x`` and the output gradient ``g``; w1 / w2: DropPath's mask / keep of its two uses.  (output, {name: gradient}).
    oracle.spformer_ref.SphereFormer itself cannot serve as the float64 evaluation: its attention casts q, k, v and the tables to
    fp32 (``.float()``, as the reference does under amp) whatever the module's dtype, and its DropPath draws its own masks; so this
    is the arrangement tests/test_gpu_sptr_rows16.py uses for the attention layer, extended by the two LayerNorms, the MLP and
    the two residual sums, over the same oracle.sptr_ref functions spformer_ref is built on."""
    P = {n: p.detach().double().cpu().requires_grad_(True) for n, p in block.named_parameters()}
    x = x.detach().double().cpu().requires_grad_(True)
    n = x.shape[0]
    h = F.layer_norm(x, (64,), P['norm1.weight'], P['norm1.bias'], block.norm1.eps)
    qkv = (h @ P['attn.qkv.weight'].t() + P['attn.qkv.bias']).reshape(n, 3, 4, 16)
    q, k, v = qkv[:, 0] * block.attn.scale, qkv[:, 1], qkv[:, 2]
    xyz = xyz.float().cpu()
    b = b.cpu().long()
    outs = []
    for h0, pts, window, quant, sfx, a in ((0, xyz, WINDOW, WINDOW / 24, '', None),
                                           (2, S.cart2sphere(xyz), WINDOW_SPHERE, WINDOW_SPHERE / 24, '_sphere', A)):
        i0, i0o, n_max, i1, i1o, sort_idx = S.get_indices_params(pts, b, np.asarray(window))
        tabs = [P['attn.relative_pos_%s_table%s' % (t, sfx)] for t in ('query', 'key', 'value')]
        outs.append(S.sparse_self_attention(q[:, h0:h0 + 2], k[:, h0:h0 + 2], v[:, h0:h0 + 2], pts, i0, i0o, n_max, i1, i1o,
                                            sort_idx, np.asarray(window), np.asarray(quant), 24, *tabs, a))
    att = torch.cat(outs, 1).reshape(n, 64) @ P['attn.proj.weight'].t() + P['attn.proj.bias']
    s = x + (att if w1 is None else w1.double().cpu() * att)
    h2 = F.layer_norm(s, (64,), P['norm2.weight'], P['norm2.bias'], block.norm2.eps)
    m = F.gelu(h2 @ P['mlp.fc1.weight'].t() + P['mlp.fc1.bias']) @ P['mlp.fc2.weight'].t() + P['mlp.fc2.bias']
    y = s + (m if w2 is None else w2.double().cpu() * m)
    y.backward(g.detach().double().cpu())
    return y.detach(), dict({'rows': x.grad}, **{n_: p.grad for n_, p in P.items()})


def _run_block(block, rows, g, xyz, b, dt, monkeypatch, on, seed=None):
    """one forward / backward of the block with the row LayerNorm kernels on or off: outputs, gradients, what the hooks saw"""
    from u2mkd_amd import _lib as L
    from u2mkd_amd.torchsparse.nn import functional as spf
    monkeypatch.setattr(spf, '_ROW_LN_ON', {k: on for k in spf._ROW_LN_ON})
    seen, calls, masks, real_call, real_bernoulli = {}, [], [], L.call, torch.Tensor.bernoulli_
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), real_call(name, *a))[1])

    def bernoulli_(self, *a, **kw):
        out = real_bernoulli(self, *a, **kw)
        masks.append(out.clone())
        return out

    monkeypatch.setattr(torch.Tensor, 'bernoulli_', bernoulli_)
    dtype_of = lambda o: (o[1] if isinstance(o, tuple) else o).dtype      # (norm2 runs its add form: (stream, normed))
    hooks = [block.norm1.register_forward_hook(lambda m, i, o: seen.__setitem__('norm1', dtype_of(o))),
             block.norm2.register_forward_hook(lambda m, i, o: seen.__setitem__('norm2', dtype_of(o)))]
    x = rows.clone().requires_grad_(True)
    block.zero_grad(set_to_none=True)
    if seed is not None:
        torch.manual_seed(seed)
    with _amp(dt):
        y = block(x, xyz, b)
    y.backward(g.to(y.dtype))
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    monkeypatch.setattr(L, 'call', real_call)
    monkeypatch.setattr(torch.Tensor, 'bernoulli_', real_bernoulli)
    res = dict({'out': y.detach(), 'rows': x.grad.float()}, **{n_: p.grad.clone() for n_, p in block.named_parameters()})
    return res, seen, [c for c in calls if c.startswith('u2mkd_ln_')], masks


def _compare_with_float64(res_on, res_off, out64, ref, label):
    lines, failed = [], []
    for name, want in dict(ref, out=out64).items():
        scale = float(want.abs().max())
        e_on = float((res_on[name].double().cpu() - want).abs().max()) / scale
        e_off = float((res_off[name].double().cpu() - want).abs().max()) / scale
        lines.append('%-44s %.3e %.3e  ratio %.2f' % (name, e_on, e_off, e_on / max(e_off, 1e-300)))
        if not e_on <= 2.0 * e_off:
            failed.append(lines[-1])
    print('\n%s: max error / max|float64|, row LayerNorm kernels | torch layer_norm\n%s' % (label, '\n'.join(lines)))
    return failed


@pytest.mark.parametrize('tag', ['bf16', 'f16'])
def test_block_under_autocast_hands_16_bit_rows_to_qkv_and_fc1(hip, monkeypatch, tag):
    """Both formulations run the same block on the same 16-bit rows.  Output and gradients: the largest error of each, relative to
    max |float64|, against the float64 evaluation of the block -- the kernels' is at most twice that of the formulation over
    torch's layer_norm (the N16 layer criterion).  The measured columns are printed, and recorded in NOTES N17.2."""
    from u2mkd_amd.lidar import sphereformer as SF
    dt = R.DTYPES[tag]
    n, xyz, b, x0, g0 = _scene()
    xyz, b = xyz.cuda(), b.cuda()
    monkeypatch.setattr(SF, 'cart2sphere', lambda p: S.cart2sphere(p.cpu()).to(p.device))      # the float64 evaluation's atan2
    block = _make_block()
    rows, g = x0.cuda().to(dt), g0.cuda().to(dt)
    res_on, seen_on, ln_on, _ = _run_block(block, rows, g, xyz, b, dt, monkeypatch, True)
    res_off, seen_off, ln_off, _ = _run_block(block, rows, g, xyz, b, dt, monkeypatch, False)
    assert seen_on == {'norm1': dt, 'norm2': dt}, seen_on
    assert seen_off == {'norm1': torch.float32, 'norm2': torch.float32}, seen_off          # (what torch's autocast layer_norm returns)
    assert ln_on == ['u2mkd_ln_forward', 'u2mkd_ln_add_forward', 'u2mkd_ln_backward', 'u2mkd_ln_backward'], ln_on
    assert not ln_off, ln_off
    assert res_on['out'].dtype == dt and bool(torch.isfinite(res_on['out'].float()).all())
    out64, ref = _block_float64(block, rows, g, xyz, b)
    assert len(ref) == 1 + len(list(block.named_parameters())) == 19
    failed = _compare_with_float64(res_on, res_off, out64, ref, tag)
    assert not failed, failed


def test_block_in_fp32_with_drop_path_draws_the_same_mask(hip, monkeypatch):
    from u2mkd_amd.lidar import sphereformer as SF
    n, xyz, b, x0, g0 = _scene()
    xyz, b = xyz.cuda(), b.cuda()
    monkeypatch.setattr(SF, 'cart2sphere', lambda p: S.cart2sphere(p.cpu()).to(p.device))
    block = _make_block(drop_path=0.3).train()
    rows, g = x0.cuda(), g0.cuda()
    res_on, _, ln_on, masks_on = _run_block(block, rows, g, xyz, b, torch.float32, monkeypatch, True, seed=1234)
    res_off, _, ln_off, masks_off = _run_block(block, rows, g, xyz, b, torch.float32, monkeypatch, False, seed=1234)
    assert ln_on == ['u2mkd_ln_forward', 'u2mkd_ln_add_forward', 'u2mkd_ln_backward', 'u2mkd_ln_backward'] and not ln_off
    assert len(masks_on) == len(masks_off) == 2 and all(torch.equal(p, q) for p, q in zip(masks_on, masks_off))
    assert 0 < int((masks_on[0] == 0).sum()) < n and not torch.equal(masks_on[0], masks_on[1])
    keep = 1 - 0.3
    out64, ref = _block_float64(block, rows, g, xyz, b, masks_on[0] / keep, masks_on[1] / keep)
    failed = _compare_with_float64(res_on, res_off, out64, ref, 'fp32, drop_path 0.3')
    assert not failed, failed


@pytest.mark.parametrize('tag', list(R.DTYPES))
def test_frozen_teacher_block_repeats_itself_and_stores_no_statistics(hip, monkeypatch, tag):
    from u2mkd_amd import _lib as L
    dt = R.DTYPES[tag]
    n, xyz, b, x0, _ = _scene()
    xyz, b = xyz.cuda(), b.cuda()
    block = _make_block(drop_path=0.3).eval()
    rows = x0.cuda().to(dt)
    stats, real = [], L.call

    def spy(name, *a):
        if name == 'u2mkd_ln_forward':
            stats.append((a[7], a[8]))
        elif name == 'u2mkd_ln_add_forward':
            stats.append((a[9], a[10]))
        return real(name, *a)

    monkeypatch.setattr(L, 'call', spy)
    with torch.no_grad(), _amp(dt):
        outs = [block(rows, xyz, b) for _ in range(10)]
    torch.cuda.synchronize()
    assert outs[0].dtype == dt and all(torch.equal(outs[0], o) for o in outs[1:])
    assert len(stats) == 20 and all(s == (None, None) for s in stats), stats[:4]
