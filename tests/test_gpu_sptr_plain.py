"""The table-free window attention (csrc/sptr_plain.hip: sptr_plain_fwd_kernel<S>, sptr_delta_kernel, sptr_plain_bwd_kernel<S>
with S = 1, 2, 4, 8, 16 lanes per (token, head)) through the C ABI against the float64 reference of
tests/sptr_plain_f64_ref.py, elementwise, on the plans of tests/sptr_f64_ref.py's small cubic cases.

U2MKD_SPTR_SPLIT is read by the library on every call, so monkeypatch.setenv selects the form.  Every case runs twice:
contiguous [n, h, 16] operands, and operands packed the way an attention layer packs them -- qkv [n, 3, H, 16] with H = h + 1
and the heads of the call starting at head 1, out / dout [n, H, 16], the gradient [n, 3, H, 16]; head 0 belongs to somebody
else and must come back untouched."""
import functools

import pytest
import torch

import sptr_plain_f64_ref as P

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


@functools.lru_cache(maxsize=None)
def _reference(S, h, q_scale):
    """float64 reference and magnitudes, on the device, once per case (both layouts share it)"""
    case = P.get_case(S, h)
    ref, mag, mag_abs = P.reference(case, q_scale, device='cuda')
    return case, ref, mag, mag_abs


def _operands(case, dev, packed):
    """(q, k, v, dout views [n, h, 16]), ld_qkv, ld_out, heads of the packed buffers or None"""
    n, h = case.n, case.h
    if not packed:
        q, k, v, dout = (x.to(dev).contiguous() for x in (case.q, case.k, case.v, case.dout))
        return (q, k, v, dout), h * 16, h * 16, None
    H = h + 1
    g = torch.Generator().manual_seed(case.n)
    qkv = torch.randn(n, 3, H, 16, generator=g).to(dev)
    for c, x in enumerate((case.q, case.k, case.v)):
        qkv[:, c, 1:] = x.to(dev)
    dout = torch.randn(n, H, 16, generator=g).to(dev)
    dout[:, 1:] = case.dout.to(dev)
    return (qkv[:, 0, 1:], qkv[:, 1, 1:], qkv[:, 2, 1:], dout[:, 1:]), 3 * H * 16, H * 16, H


def _run(L, case, dev, q_scale, packed, repeats=3):
    n, h = case.n, case.h
    (q, k, v, dout), ld_qkv, ld_out, H = _operands(case, dev, packed)
    i32 = lambda x: torch.as_tensor(x, dtype=torch.int32, device=dev).contiguous()
    sort_idx, wstart, wlen = i32(case.sort_idx), i32(case.wstart), i32(case.wlen)
    plan = (L.ptr(sort_idx), L.ptr(wstart), L.ptr(wlen), n, h, 16)
    st = L.stream()
    lse = torch.full((n, h), float('nan'), device=dev)
    if packed:
        out_full = torch.full((n, H, 16), float('nan'), device=dev)
        out = out_full[:, 1:]
    else:
        out_full = out = torch.full((n, h, 16), float('nan'), device=dev)
    L.call('u2mkd_sptr_plain_forward_strided', L.ptr(q), L.ptr(k), L.ptr(v), ld_qkv, q_scale, *plan, L.ptr(out), ld_out, L.ptr(lse), st)
    runs = []
    for _ in range(repeats):
        delta = torch.empty(n, h, device=dev)
        if packed:
            full = torch.full((n, 3, H, 16), SENTINEL, device=dev)
            dq, dk, dv = full[:, 0, 1:], full[:, 1, 1:], full[:, 2, 1:]
            ld_grad = 3 * H * 16
        else:
            full = torch.full((3, n, h, 16), SENTINEL, device=dev)
            dq, dk, dv = full[0], full[1], full[2]
            ld_grad = h * 16
        L.call('u2mkd_sptr_plain_backward_strided', L.ptr(q), L.ptr(k), L.ptr(v), ld_qkv, q_scale, L.ptr(out), L.ptr(dout), ld_out,
               L.ptr(lse), *plan, L.ptr(delta), L.ptr(dq), L.ptr(dk), L.ptr(dv), ld_grad, st)
        runs.append({'dq': dq, 'dk': dk, 'dv': dv, 'full': full})
    torch.cuda.synchronize()
    return {'out': out, 'lse': lse, 'out_full': out_full}, runs


@pytest.mark.parametrize('packed', [False, True], ids=['contiguous', 'packed'])
@pytest.mark.parametrize('S,h,q_scale', P.gpu_cases(), ids=[P.case_id(c) for c in P.gpu_cases()])
def test_plain_attention_equals_the_float64_reference_elementwise(hip, monkeypatch, S, h, q_scale, packed):
    monkeypatch.setenv('U2MKD_SPTR_SPLIT', str(S))
    dev = torch.device('cuda')
    case, ref, mag, mag_abs = _reference(S, h, q_scale)
    assert case.n % (128 // S) != 0
    fwd, runs = _run(hip, case, dev, q_scale, packed)
    got = dict(fwd, **runs[0])
    if packed:                                           # the other head's columns: untouched
        assert bool(torch.isnan(fwd['out_full'][:, 0]).all())
        for r in runs:
            assert bool((r['full'][:, :, 0] == SENTINEL).all())
    figures, failed = [], []
    for kind in P.KINDS:
        x = got[kind]
        assert bool(torch.isfinite(x).all()), kind                              # (every element written: no NaN / sentinel left
        assert not bool((x == SENTINEL).any()), kind                            # would also miss the gate below)
        w, w_abs = P.worst(kind, x, ref[kind], mag[kind]), P.worst(kind, x, ref[kind], mag_abs[kind])
        figures.append('%s %.2e/%.1e %.2e/%.1e' % (kind, w, P.KAPPA[kind], w_abs, P.KAPPA_ABS[kind]))
        bad = int(P.violations(kind, x, ref[kind], mag[kind]).sum())
        bad_abs = int(P.violations(kind, x, ref[kind], mag_abs[kind], kappa=P.KAPPA_ABS[kind]).sum())
        if bad or bad_abs:
            failed.append((kind, bad, bad_abs))
    print('\n%s %s n=%d  max err/magnitude vs kappa (factor | term-wise): %s' % (
        P.case_id((S, h, q_scale)), 'packed' if packed else 'contiguous', case.n, '; '.join(figures)))
    assert not failed, (failed, figures)
    for r in runs[1:]:                                   # no atomics: the same bits on every run
        assert torch.equal(r['full'], runs[0]['full'])


def test_empty_token_and_head_counts_do_nothing_and_give_zeros(hip):
    from u2mkd_amd.sptr import functional as SF
    dev = torch.device('cuda')
    st = hip.stream()
    keep = torch.full((4, 2, 16), SENTINEL, device=dev)
    i = torch.zeros(4, dtype=torch.int32, device=dev)
    for n, h in ((0, 2), (4, 0)):
        hip.call('u2mkd_sptr_plain_forward_strided', hip.ptr(keep), hip.ptr(keep), hip.ptr(keep), 32, 1.0, hip.ptr(i), hip.ptr(i),
                 hip.ptr(i), n, h, 16, hip.ptr(keep), 32, hip.ptr(keep), st)
        hip.call('u2mkd_sptr_plain_backward_strided', hip.ptr(keep), hip.ptr(keep), hip.ptr(keep), 32, 1.0, hip.ptr(keep), hip.ptr(keep),
                 32, hip.ptr(keep), hip.ptr(i), hip.ptr(i), hip.ptr(i), n, h, 16, hip.ptr(keep), hip.ptr(keep), hip.ptr(keep),
                 hip.ptr(keep), 32, st)
        torch.cuda.synchronize()
        assert bool((keep == SENTINEL).all())
        plan = SF.WindowPlan(torch.rand(n, 3, device=dev), torch.zeros(n, dtype=torch.long, device=dev), [0.5, 0.5, 0.5]) if n else None
        q, k, v = (torch.randn(n, h, 16, device=dev, requires_grad=True) for _ in range(3))
        out = SF.plain_window_attention(q, k, v, plan)
        assert out.shape == (n, h, 16) and float(out.detach().abs().sum()) == 0.0
        out.sum().backward()
        for t in (q, k, v):
            assert t.grad.shape == t.shape and float(t.grad.abs().sum()) == 0.0


def test_bad_head_dim_and_bad_strides_are_refused_with_nothing_written(hip):
    dev = torch.device('cuda')
    st = hip.stream()
    n, h = 8, 2
    rows = torch.randn(n, 3, 40, device=dev)
    outs = torch.full((5, n, 40), SENTINEL, device=dev)
    lse = torch.full((n, h), SENTINEL, device=dev)
    idx = torch.arange(n, dtype=torch.int32, device=dev)
    one = torch.ones(n, dtype=torch.int32, device=dev)
    q, k, v = rows[:, 0], rows[:, 1], rows[:, 2]

    def fwd(ld_qkv, ld_out, hdim):
        hip.call('u2mkd_sptr_plain_forward_strided', hip.ptr(q), hip.ptr(k), hip.ptr(v), ld_qkv, 1.0, hip.ptr(idx), hip.ptr(idx),
                 hip.ptr(one), n, h, hdim, hip.ptr(outs[0]), ld_out, hip.ptr(lse), st)

    def bwd(ld_qkv, ld_out, ld_grad, hdim):
        hip.call('u2mkd_sptr_plain_backward_strided', hip.ptr(q), hip.ptr(k), hip.ptr(v), ld_qkv, 1.0, hip.ptr(outs[0]), hip.ptr(outs[1]),
                 ld_out, hip.ptr(lse), hip.ptr(idx), hip.ptr(idx), hip.ptr(one), n, h, hdim, hip.ptr(lse), hip.ptr(outs[2]),
                 hip.ptr(outs[3]), hip.ptr(outs[4]), ld_grad, st)

    with pytest.raises(RuntimeError, match='head dim'):
        fwd(120, 40, 8)
    with pytest.raises(RuntimeError, match='head dim'):
        bwd(120, 40, 40, 32)
    with pytest.raises(RuntimeError, match='stride'):
        fwd(122, 40, 16)                                   # not a multiple of 4 floats
    with pytest.raises(RuntimeError, match='stride'):
        fwd(120, 38, 16)
    with pytest.raises(RuntimeError, match='stride'):
        fwd(120, 28, 16)                                   # a multiple of 4 that cannot hold two heads
    with pytest.raises(RuntimeError, match='stride'):
        bwd(120, 40, 42, 16)
    with pytest.raises(RuntimeError, match='stride'):
        bwd(121, 40, 40, 16)
    q_real = q
    q = rows.view(-1)[1:].as_strided((n, 40), (120, 1))    # a row pointer 4 bytes off a 16-byte boundary
    with pytest.raises(RuntimeError, match='aligned'):
        fwd(120, 40, 16)
    with pytest.raises(RuntimeError, match='aligned'):
        bwd(120, 40, 40, 16)
    q = q_real
    torch.cuda.synchronize()
    assert bool((outs == SENTINEL).all()) and bool((lse == SENTINEL).all())
