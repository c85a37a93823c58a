"""Window attention on 16-bit rows (csrc/sptr.hip with the row type T = bf16 / fp16; u2mkd_sptr_attention_{forward,backward}
_strided_bf16 / _f16; sptr/functional.py under U2MKD_SPTR_ROWS16): the arithmetic is the fp32 kernels', only loads and stores
change, so everything is compared with the fp32 entries on the same values -- for equality.

  1  per kernel form (S = 1, 4, 16 lanes per token, one or two backward launches, both branches), packed operands as the layer
     packs them: out16 == round(out32), lse16 == lse32, dqkv16 == round(dqkv32), the table gradients equal bit for bit.  The
     fp32 backward is given the 16-bit out upcast -- the tensor the 16-bit backward reads -- so delta is the same number.
  2  the forward against the float64 reference of tests/sptr_f64_ref.py on the rounded inputs: the fp32 kernels' bound plus
     one rounding of the stored value.
  3  fp16's range: a result beyond 65504 is stored as inf (never the largest finite number), and an inf in dout reaches dq of
     its token and dk, dv of every token of its window.
  4  strides that are no multiple of 8 elements and rows that are not 16-byte aligned are refused before anything is launched.
  5  the attention layer under bf16 / fp16 autocast: 16-bit entries only, 16-bit saved tensors, the forward equal to the
     upcast formulation's, the gradients as close to a float64 evaluation of the layer as the upcast formulation's.
  6  SPVCNN + SphereFormer: equal logits with the switch on and off, and a training step under both amp modes."""
import contextlib
import copy
import functools
import os

import numpy as np
import pytest
import torch

import sptr_f64_ref as R
from oracle import sptr_ref as S
from u2mkd_amd.synth import synth_batch

pytestmark = pytest.mark.gpu

SENTINEL = 12288.0                                     # (exact in bf16 and fp16)
DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16}
UNIT = {'bf16': 2.0 ** -8, 'f16': 2.0 ** -11}          # unit roundoff of the stored type
TINY = {'bf16': 1e-30, 'f16': 2.0 ** -25}              # half the smallest fp16 subnormal: what a store can lose near zero
FORMS = [(1, True), (4, True), (4, False), (16, True)]                       # (lanes per token, one backward launch)


@contextlib.contextmanager
def _form(S_, merge):
    """U2MKD_SPTR_SPLIT / U2MKD_SPTR_BWD_MERGE (read by the library on every call) for the calls inside"""
    keys = ('U2MKD_SPTR_SPLIT', 'U2MKD_SPTR_BWD_MERGE')
    was = {k: os.environ.get(k) for k in keys}
    os.environ['U2MKD_SPTR_SPLIT'] = str(S_)
    if merge:
        os.environ.pop('U2MKD_SPTR_BWD_MERGE', None)
    else:
        os.environ['U2MKD_SPTR_BWD_MERGE'] = '0'
    try:
        yield
    finally:
        for k, v in was.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _entry(base, tag):
    return base + ('_' + tag if tag else '')


def _plan_args(L, case, dev):
    i32 = lambda x: torch.as_tensor(x, dtype=torch.int32, device=dev).contiguous()
    keep = [i32(case.sort_idx), i32(case.wstart), i32(case.wlen), i32(case.qc),
            torch.as_tensor(case.radial, device=dev) if case.sphere else None] + \
           [t.to(dev).contiguous() for t in (case.tq, case.tk, case.tv)]
    return keep, tuple(L.ptr(t) for t in keep) + (case.L, case.qgl, case.a)


def _packed(case, tag, dev, v_fill=None):
    """(qkv [n, 3, H, 16], dout [n, H, 16]) in the row type ``tag``: the branch at head 1, head 0 another branch's"""
    n, H = case.n, case.h + 1
    g = torch.Generator().manual_seed(case.n)
    qkv = torch.randn(n, 3, H, 16, generator=g)
    for c, x in enumerate((case.q, case.k, case.v)):
        qkv[:, c, 1:] = x
    if v_fill is not None:
        qkv[:, 2, 1:] = v_fill
    dout = torch.randn(n, H, 16, generator=g)
    dout[:, 1:] = case.dout
    return qkv.to(dev).to(DTYPES[tag]), dout.to(dev).to(DTYPES[tag])


def _forward(L, case, plan, qkv, tag):
    n, h, H = case.n, case.h, case.h + 1
    out = torch.full((n, H, 16), float('nan'), device=qkv.device, dtype=qkv.dtype)
    lse = torch.full((n, h), float('nan'), device=qkv.device)
    L.call(_entry('u2mkd_sptr_attention_forward_strided', tag), L.ptr(qkv[:, 0, 1:]), L.ptr(qkv[:, 1, 1:]), L.ptr(qkv[:, 2, 1:]),
           3 * H * 16, case.q_scale, *plan, n, h, 16, L.ptr(out[:, 1:]), H * 16, L.ptr(lse), L.stream())
    return out, lse


def _backward(L, case, plan, qkv, out, dout, lse, tag):
    n, h, H = case.n, case.h, case.h + 1
    dev = qkv.device
    dqkv = torch.full((n, 3, H, 16), SENTINEL, device=dev, dtype=qkv.dtype)
    shape = (case.L, 3, h, 16)
    dtq, dtk, dtv = (torch.full(shape, float('nan'), device=dev) for _ in range(3))
    delta = torch.empty(n, h, device=dev)
    nbytes = L.load().u2mkd_sptr_backward_workspace_bytes(n, h, case.L)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    ld = 3 * H * 16
    L.call(_entry('u2mkd_sptr_attention_backward_strided', tag), L.ptr(qkv[:, 0, 1:]), L.ptr(qkv[:, 1, 1:]), L.ptr(qkv[:, 2, 1:]), ld,
           case.q_scale, L.ptr(out[:, 1:]), L.ptr(dout[:, 1:]), H * 16, L.ptr(lse), *plan, case.qc_span, n, h, 16, L.ptr(delta),
           L.ptr(ws), nbytes, L.ptr(dqkv[:, 0, 1:]), L.ptr(dqkv[:, 1, 1:]), L.ptr(dqkv[:, 2, 1:]), ld, None, None, None, L.stream())
    L.call('u2mkd_sptr_table_reduce', L.ptr(ws), n, h, case.L, case.a, L.ptr(dtq), L.ptr(dtk), L.ptr(dtv), L.stream())
    return dqkv, dtq, dtk, dtv


@functools.lru_cache(maxsize=None)
def _both(tag, sphere, S_, merge):
    """The 16-bit entries and the fp32 entries on the same (rounded) values, one kernel form; computed once per case."""
    from u2mkd_amd import _lib as L
    dev = torch.device('cuda')
    case = R.get_case(S_, sphere, 3 if S_ == 4 else 2, False)
    keep, plan = _plan_args(L, case, dev)
    qkv16, dout16 = _packed(case, tag, dev)
    with _form(S_, merge):
        out16, lse16 = _forward(L, case, plan, qkv16, tag)
        g16 = _backward(L, case, plan, qkv16, out16, dout16, lse16, tag)
        qkv32, dout32 = qkv16.float(), dout16.float()
        out32, lse32 = _forward(L, case, plan, qkv32, '')
        g32 = _backward(L, case, plan, qkv32, out16.float(), dout32, lse32, '')      # (out: what the 16-bit backward read)
        torch.cuda.synchronize()
    return case, {'qkv': qkv16, 'dout': dout16, 'out': out16, 'lse': lse16, 'grads': g16}, {'out': out32, 'lse': lse32, 'grads': g32}


def _form_id(f):
    return 'S%d%s' % (f[0], '' if f[1] else '-twolaunch')


# ------------------------------------------------------------------ 1. bit equality with the fp32 entries
@pytest.mark.parametrize('form', FORMS, ids=_form_id)
@pytest.mark.parametrize('sphere', [False, True], ids=['cubic', 'sphere'])
@pytest.mark.parametrize('tag', ['bf16', 'f16'])
def test_rows16_entries_equal_the_fp32_entries_rounded_once(hip, tag, sphere, form):
    S_, merge = form
    dt = DTYPES[tag]
    case, r16, r32 = _both(tag, sphere, S_, merge)
    tpb = 128 // S_
    assert case.n % tpb != 0 and 1000 < case.n < 4300 and case.h == (3 if S_ == 4 else 2)
    assert {1, S_, S_ + 1, 385} <= set(int(w) for w in case.window_lengths)
    assert r16['out'].dtype == dt and r16['grads'][0].dtype == dt and r16['lse'].dtype == torch.float32
    # the other branch's columns: untouched by both
    for r in (r16, r32):
        assert bool(torch.isnan(r['out'][:, 0]).all()) and bool((r['grads'][0][:, :, 0] == SENTINEL).all())
    assert bool(torch.isfinite(r16['out'][:, 1:].float()).all()) and bool(torch.isfinite(r16['grads'][0].float()).all())
    assert torch.equal(r16['out'][:, 1:], r32['out'][:, 1:].to(dt))
    assert torch.equal(r16['lse'], r32['lse'])
    for c, name in enumerate(('dq', 'dk', 'dv')):
        a, b = r16['grads'][0][:, c, 1:], r32['grads'][0][:, c, 1:].to(dt)
        assert torch.equal(a, b), (name, int((a != b).sum()), float((a.float() - b.float()).abs().max()))
    for name, a, b in zip(('dTq', 'dTk', 'dTv'), r16['grads'][1:], r32['grads'][1:]):
        assert a.dtype == torch.float32 and bool(torch.isfinite(a).all())
        assert torch.equal(a, b), (name, int((a != b).sum()), float((a - b).abs().max()))


# ------------------------------------------------------------------ 2. the forward against float64
@functools.lru_cache(maxsize=None)
def _reference64(tag, sphere, S_):
    case, r16, _ = _both(tag, sphere, S_, True)
    rounded = copy.copy(case)                          # the same plan and tables, q, k, v, dout as the kernels saw them
    rounded.q, rounded.k, rounded.v = (r16['qkv'][:, c, 1:].float().cpu() for c in range(3))
    rounded.dout = r16['dout'][:, 1:].float().cpu()
    return R.reference(rounded, device='cuda')


@pytest.mark.parametrize('S_', [1, 16])
@pytest.mark.parametrize('sphere', [False, True], ids=['cubic', 'sphere'])
@pytest.mark.parametrize('tag', ['bf16', 'f16'])
def test_rows16_forward_within_the_fp32_bound_plus_one_rounding_of_float64(hip, tag, sphere, S_):
    """|out16 - out64| <= kappa mag + u (|out64| + kappa mag) + t, elementwise, with kappa and mag of tests/sptr_f64_ref.py
    (the fp32 kernels' bound, twice: factor-wise and term-wise), u the unit roundoff of the stored type and t what a store
    can lose next to zero; lse (fp32) under its fp32 bound."""
    case, r16, _ = _both(tag, sphere, S_, True)
    assert case.edge_slack() > 1.0
    ref, mag, mag_abs = _reference64(tag, sphere, S_)
    out = r16['out'][:, 1:].to(torch.float64)
    err = (out - ref['out']).abs()
    u, t = UNIT[tag], TINY[tag]
    figures = []
    for kappa, m in ((R.KAPPA['out'], mag['out']), (R.KAPPA_ABS['out'], mag_abs['out'])):
        bound = kappa * m + u * (ref['out'].abs() + kappa * m) + t
        figures.append(float((err / bound).max()))
    lse_bad = int(R.violations('lse', r16['lse'], ref['lse'], mag['lse']).sum())
    print('\n%s %s S%d: max err / bound %.3f (factor-wise) %.3f (term-wise), lse violations %d'
          % (tag, 'sphere' if sphere else 'cubic', S_, figures[0], figures[1], lse_bad))
    assert bool(torch.isfinite(out).all())
    assert figures[0] <= 1.0 and figures[1] <= 1.0, figures
    assert lse_bad == 0


# ------------------------------------------------------------------ 3. the fp16 range
@pytest.mark.parametrize('tag', ['bf16', 'f16'])
def test_rows16_values_beyond_the_fp16_range_are_stored_as_inf(hip, tag):
    """v = 7e4 (a bf16 number; inf once rounded to fp16): out is inf everywhere under fp16, finite under bf16.  And the case
    a store decides: v = 65504 -- fp16's largest finite number -- with value tables of +64 per axis makes every out 65696 in
    fp32, beyond the rounding threshold 65520: stored as inf, not saturated to 65504 (bf16: the finite 65536 + ...)."""
    L = hip
    dev = torch.device('cuda')
    for S_, sphere in ((1, False), (16, True)):
        case = copy.copy(R.get_case(S_, sphere, 2, False))
        keep, plan = _plan_args(L, case, dev)
        with _form(S_, True):
            qkv, _ = _packed(case, tag, dev, v_fill=7e4)
            out, lse = _forward(L, case, plan, qkv, tag)
            case.tv = torch.full_like(case.tv, 64.0)
            keep2, plan2 = _plan_args(L, case, dev)
            qkv2, _ = _packed(case, tag, dev, v_fill=65504.0)
            out2, _ = _forward(L, case, plan2, qkv2, tag)
            torch.cuda.synchronize()
        assert bool(torch.isfinite(lse).all())
        for o in (out, out2):
            o = o[:, 1:].float()
            if tag == 'f16':
                assert bool(torch.isinf(o).all()) and bool((o > 0).all())
            else:
                assert bool(torch.isfinite(o).all()) and float(o.min()) > 6.5e4


@pytest.mark.parametrize('merge', [True, False], ids=['merged', 'twolaunch'])
@pytest.mark.parametrize('tag', ['bf16', 'f16'])
def test_rows16_an_inf_in_dout_reaches_the_gradients_of_its_window(hip, tag, merge):
    """One inf in dout of token t (what an overflowed fp16 step hands down): dq of t, and dk and dv of EVERY token of t's window,
    are non-finite -- the GradScaler finds the step -- and no token outside the window is touched.  (dq of the window's other
    tokens does not depend on dout of t: ds_ij = p_ij (dout_i . (v_j + Tv) - delta_i).)"""
    L = hip
    dev = torch.device('cuda')
    S_ = 4
    case = R.get_case(S_, False, 3, False)
    keep, plan = _plan_args(L, case, dev)
    qkv, dout = _packed(case, tag, dev)
    p = int(np.nonzero(case.wlen == S_ + 1)[0][0])                 # a sorted position in a window of S + 1 tokens
    members = case.sort_idx[case.wstart[p]:case.wstart[p] + case.wlen[p]].astype(np.int64)
    t = int(case.sort_idx[p])
    dout[t, 2, 5] = float('inf')                                   # (head 1 of the branch)
    with _form(S_, merge):
        out, lse = _forward(L, case, plan, qkv, tag)
        dqkv, dtq, dtk, dtv = _backward(L, case, plan, qkv, out, dout, lse, tag)
        torch.cuda.synchronize()
    bad = ~torch.isfinite(dqkv[:, :, 1:].float()).all(-1).all(-1)       # [n, 3]: token has a non-finite element in dq | dk | dv
    inside = torch.zeros(case.n, dtype=torch.bool, device=dev)
    inside[torch.as_tensor(members, device=dev)] = True
    assert bool(bad[t, 0])
    assert bool(bad[inside, 1].all()) and bool(bad[inside, 2].all())
    assert not bool(bad[~inside].any())
    only_t = torch.zeros_like(inside)
    only_t[t] = True
    assert not bool(bad[~only_t, 0].any())


# ------------------------------------------------------------------ 4. refusals
@pytest.mark.parametrize('tag', ['bf16', 'f16'])
def test_rows16_entries_refuse_odd_strides_and_misaligned_rows(hip, tag):
    L = hip
    lib = L.load()
    dev = torch.device('cuda')
    case = R.get_case(1, False, 2, False)
    n, h, H = case.n, case.h, case.h + 1
    keep, plan = _plan_args(L, case, dev)
    qkv, dout = _packed(case, tag, dev)
    out = torch.full((n * H * 16 + 64,), float('nan'), device=dev, dtype=qkv.dtype)
    lse = torch.full((n, h), float('nan'), device=dev)
    dq = torch.full((n * 3 * H * 16 + 64,), SENTINEL, device=dev, dtype=qkv.dtype)
    delta = torch.full((n, h), float('nan'), device=dev)
    nbytes = lib.u2mkd_sptr_backward_workspace_bytes(n, h, case.L)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    ld, ldo = 3 * H * 16, H * 16
    q, k, v = (L.ptr(qkv[:, c, 1:]) for c in range(3))
    fwd = getattr(lib, 'u2mkd_sptr_attention_forward_strided_' + tag)
    bwd = getattr(lib, 'u2mkd_sptr_attention_backward_strided_' + tag)

    def forward(q=q, k=k, v=v, ld=ld, o=L.ptr(out), ldo=ldo):
        return fwd(q, k, v, ld, case.q_scale, *plan, n, h, 16, o, ldo, L.ptr(lse), L.stream())

    def backward(q=q, ld=ld, o=L.ptr(out), do=L.ptr(dout[:, 1:]), ldo=ldo, g=L.ptr(dq), ldg=ld):
        return bwd(q, k, v, ld, case.q_scale, o, do, ldo, L.ptr(lse), *plan, case.qc_span, n, h, 16, L.ptr(delta), L.ptr(ws), nbytes,
                   g, g + 32 * H, g + 64 * H, ldg, None, None, None, L.stream())

    refused = [forward(ld=ld + 4), forward(ldo=ldo + 4), forward(q=q + 2), forward(v=v + 2), forward(o=L.ptr(out) + 2),
               backward(ld=ld + 4), backward(ldo=ldo + 4), backward(ldg=ld + 4), backward(q=q + 2), backward(o=L.ptr(out) + 2),
               backward(do=L.ptr(dout[:, 1:]) + 2), backward(g=L.ptr(dq) + 2)]
    messages = lib.u2mkd_last_error().decode()
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in refused), refused
    assert '16-byte aligned' in messages or 'multiples of 8' in messages, messages
    # nothing was launched: every output still holds what it was filled with
    assert bool(torch.isnan(out.float()).all()) and bool(torch.isnan(lse).all()) and bool(torch.isnan(delta).all())
    assert bool((dq == SENTINEL).all())
    assert forward() == 0                                          # the same call with what it asks for is accepted
    torch.cuda.synchronize()
    assert bool(torch.isfinite(lse).all())


# ------------------------------------------------------------------ 5. the layer
def _layer_scene():
    g = torch.Generator().manual_seed(11)
    n = 3000
    xyz = torch.rand(n, 3, generator=g) * torch.tensor([3.0, 3.0, 1.0]) + torch.tensor([2.0, -1.5, -0.5])
    b = torch.sort(torch.randint(0, 2, (n,), generator=g))[0].int()
    return n, xyz, b, torch.randn(n, 64, generator=g), torch.randn(n, 64, generator=g)


WINDOW, WINDOW_SPHERE, A = np.array([0.3, 0.3, 0.3], dtype=np.float32), np.array([2.0, 2.0, 120.0]), 0.0125


def _make_layer():
    from u2mkd_amd.lidar import sphereformer as SF
    torch.manual_seed(64)
    layer = SF.SparseMultiheadSASphereConcat(64, 4, WINDOW.copy(), WINDOW_SPHERE.copy(), WINDOW / 24, WINDOW_SPHERE / 24, A).cuda()
    for name, p in layer.named_parameters():
        if 'table' in name:
            torch.nn.init.normal_(p, std=0.2)
    return layer


def _layer_float64(layer, x, g, xyz, b):
    """float64 autograd evaluation of the layer (spherical_transformer.py:192-229 over oracle.sptr_ref, CPU) on the rows ``x`` and
    the output gradient ``g``: {name: gradient} for the input rows and every parameter"""
    P = {n: p.detach().double().cpu().requires_grad_(True) for n, p in layer.named_parameters()}
    x = x.detach().double().cpu().requires_grad_(True)
    n = x.shape[0]
    qkv = (x @ P['qkv.weight'].t() + P['qkv.bias']).reshape(n, 3, 4, 16)
    q, k, v = qkv[:, 0] * layer.scale, qkv[:, 1], qkv[:, 2]
    xyz = xyz.float().cpu()
    b = b.cpu().long()
    outs = []
    for h0, pts, window, quant, sfx, a in ((0, xyz, WINDOW, WINDOW / 24, '', None),
                                           (2, S.cart2sphere(xyz), WINDOW_SPHERE, WINDOW_SPHERE / 24, '_sphere', A)):
        i0, i0o, n_max, i1, i1o, sort_idx = S.get_indices_params(pts, b, np.asarray(window))
        tabs = [P['relative_pos_%s_table%s' % (w, sfx)] for w in ('query', 'key', 'value')]
        outs.append(S.sparse_self_attention(q[:, h0:h0 + 2], k[:, h0:h0 + 2], v[:, h0:h0 + 2], pts, i0, i0o, n_max, i1, i1o,
                                            sort_idx, np.asarray(window), np.asarray(quant), 24, *tabs, a))
    y = torch.cat(outs, 1).reshape(n, 64) @ P['proj.weight'].t() + P['proj.bias']
    y.backward(g.detach().double().cpu())
    return dict({'rows': x.grad}, **{n_: p.grad for n_, p in P.items()})


@pytest.mark.parametrize('tag', ['bf16', 'f16'])
def test_rows16_attention_layer_under_autocast(hip, monkeypatch, tag):
    """Both formulations run the same layer on the same 16-bit rows.  Gradients: the largest error of each, relative to
    max |grad64|, against the float64 evaluation -- the 16-bit path's is at most twice the upcast path's (one more 16-bit
    rounding, of out on its way into delta, next to those both share).  The two measured columns are printed, and recorded
    in NOTES N16.2 (largest ratio there: 1.37)."""
    from u2mkd_amd import _lib as L
    from u2mkd_amd.lidar import sphereformer as SF
    from u2mkd_amd.sptr import functional as SFn
    dt = DTYPES[tag]
    n, xyz, b, x0, g0 = _layer_scene()
    xyz, b = xyz.cuda(), b.cuda()
    # the spherical coordinates of the float64 evaluation: the CPU's atan2, not the device's (a token on a window edge)
    monkeypatch.setattr(SF, 'cart2sphere', lambda p: S.cart2sphere(p.cpu()).to(p.device))
    layer = _make_layer()
    rows, g = x0.cuda().to(dt), g0.cuda().to(dt)
    seen, calls, real_call, real_attention = {}, [], L.call, SF.sptr.packed_window_attention

    def spy_call(name, *a):
        calls.append(name)
        return real_call(name, *a)

    def spy_attention(*a, **kw):
        y = real_attention(*a, **kw)
        seen['attention'] = y
        return y

    monkeypatch.setattr(L, 'call', spy_call)
    monkeypatch.setattr(SF.sptr, 'packed_window_attention', spy_attention)
    hook = layer.proj.register_forward_pre_hook(lambda m, inp: seen.__setitem__('proj_in', inp[0].dtype))
    res = {}
    for on in (True, False):
        monkeypatch.setattr(SFn, '_ROWS16', on)
        del calls[:]
        x = rows.clone().requires_grad_(True)
        layer.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dt):
            y = layer(x, xyz, b)
        att = seen['attention']
        saved = att.grad_fn.saved_tensors
        y.backward(g.to(y.dtype))
        torch.cuda.synchronize()
        attention_calls = [c for c in calls if c.startswith('u2mkd_sptr_attention')]
        assert len(attention_calls) == 4, attention_calls                               # two branches, forward and backward
        if on:
            assert all(c.endswith('_' + tag) for c in attention_calls), attention_calls
            assert att.dtype == dt and saved[0].dtype == dt and saved[1].dtype == dt
            assert saved[0].shape == (n, 3, 4, 16) and saved[1].shape == (n, 4, 16)
            assert seen['proj_in'] == dt
        else:
            assert not any(c.endswith('_bf16') or c.endswith('_f16') for c in attention_calls), attention_calls
            assert att.dtype == torch.float32 and saved[0].dtype == torch.float32
        assert x.grad.dtype == dt
        res[on] = dict({'out': y.detach(), 'rows': x.grad.float()}, **{n_: p.grad.clone() for n_, p in layer.named_parameters()})
    hook.remove()
    assert res[True]['out'].dtype == dt and torch.equal(res[True]['out'], res[False]['out'])
    assert bool(torch.isfinite(res[True]['out'].float()).all())
    ref = _layer_float64(layer, rows, g, xyz, b)
    lines, failed = [], []
    for name, want in ref.items():
        scale = float(want.abs().max())
        e_on = float((res[True][name].double().cpu() - want).abs().max()) / scale
        e_off = float((res[False][name].double().cpu() - want).abs().max()) / scale
        lines.append('%-40s %.3e %.3e' % (name, e_on, e_off))
        if not e_on <= 2.0 * e_off:
            failed.append(name)
    print('\n%s: max error / max|grad64|, 16-bit path | upcast path\n%s' % (tag, '\n'.join(lines)))
    assert len(ref) == 11                                                              # rows, qkv and proj (weight, bias), six tables
    assert not failed, (failed, lines)


def test_rows16_one_module_under_bf16_then_fp16_then_no_autocast(hip):
    n, xyz, b, x0, _ = _layer_scene()
    xyz, b, x0 = xyz.cuda(), b.cuda(), x0.cuda()
    layer = _make_layer()
    with torch.no_grad():
        fresh = layer(x0, xyz, b)
        for dt in (torch.bfloat16, torch.float16):
            with torch.autocast('cuda', dt):
                y = layer(x0.to(dt), xyz, b)
            assert y.dtype == dt and bool(torch.isfinite(y.float()).all())
        third = layer(x0, xyz, b)
    assert third.dtype == torch.float32 and torch.equal(third, fresh)


# ------------------------------------------------------------------ 6. SPVCNN + SphereFormer
@pytest.mark.parametrize('amp', ['bf16', 'fp16'])
def test_rows16_spvcnn_spformer_logits_and_a_training_step(hip, monkeypatch, amp):
    from u2mkd_amd import lidar, torchsparse as ts, train as T
    from u2mkd_amd.sptr import functional as SFn
    dt = {'bf16': torch.bfloat16, 'fp16': torch.float16}[amp]
    batch = synth_batch(4000, 1, seed=3)
    feats, coords, labels = (torch.from_numpy(batch[k]).cuda() for k in ('feats', 'coords', 'labels'))
    torch.manual_seed(0)
    model = lidar.SPVCNN_SPFORMER(**lidar.spformer_kwargs(cr=1.0, drop_path_rate=0.0)).cuda().train()
    model.dropout.p = 0.0
    logits = {}
    for on in (True, False):
        monkeypatch.setattr(SFn, '_ROWS16', on)
        with torch.no_grad(), torch.autocast('cuda', dt):
            logits[on] = model({'lidar': ts.SparseTensor(feats, coords)})['x_vox']
    assert bool(torch.isfinite(logits[True].float()).all())
    assert torch.equal(logits[True], logits[False])
    monkeypatch.setattr(SFn, '_ROWS16', True)
    run = T.LidarStep(model, amp=amp)
    before = [p.detach().clone() for p in model.parameters()]
    scale = float(run.amp.scaler.get_scale())
    loss = float(run(feats, coords, labels))
    assert np.isfinite(loss), loss
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    if amp == 'fp16':                                              # the scaler found nothing to skip: the step was applied
        assert float(run.amp.scaler.get_scale()) == scale
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
