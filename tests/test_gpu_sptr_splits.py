"""Every key-split form of the fused window attention (csrc/sptr.hip: S = 1, 2, 4, 8, 16 lanes per (token, head), forward
and backward, one or two backward launches) against the float64 reference of tests/sptr_f64_ref.py, elementwise.

U2MKD_SPTR_SPLIT / U2MKD_SPTR_BWD_MERGE are read by the library on every call, so monkeypatch.setenv selects the form;
they stay fixed from the backward call to u2mkd_sptr_table_reduce, which recomputes the grid from them.  Kernels per case:

    forward    S = 1: sptr_attn_fwd_kernel             S > 1: sptr_attn_fwd_split_kernel<S>
    backward   S > 1:              sptr_bwd_both_kernel<S>
               S > 1 '-twolaunch': sptr_bwd_query_kernel<S> + sptr_bwd_key_kernel<S>
               S = 1:              sptr_bwd_query_kernel<1> + sptr_bwd_key_kernel<1>   ('-66k': the persistent grid of 512
                                   workgroups takes a second pass; S > 1 takes one in every small case, grid of 128)
    always     sptr_delta_kernel, sptr_table_reduce_kernel (through u2mkd_sptr_table_reduce)

Operands are packed the way the attention layer packs them: qkv [n, 3, H, 16] with H = h + 1 and the branch's heads
starting at head 1, out / dout [n, H, 16], the gradient [n, 3, H, 16]; head 0 belongs to another branch and must come
back untouched."""
import functools

import pytest
import torch

import sptr_f64_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


@functools.lru_cache(maxsize=None)
def _reference(S, sphere, h, big):
    """float64 reference and magnitudes, on the device, once per distinct input (the two-launch cases share theirs)."""
    case = R.get_case(S, sphere, h, big)
    ref, mag, mag_abs = R.reference(case, device='cuda')
    return case, ref, mag, mag_abs


def _run(L, case, dev):
    n, h, H = case.n, case.h, case.h + 1
    g = torch.Generator().manual_seed(case.n)
    qkv = torch.randn(n, 3, H, 16, generator=g).to(dev)                      # (head 0: another branch's operands)
    for c, x in enumerate((case.q, case.k, case.v)):
        qkv[:, c, 1:] = x.to(dev)
    dout = torch.randn(n, H, 16, generator=g).to(dev)
    dout[:, 1:] = case.dout.to(dev)
    i32 = lambda x: torch.as_tensor(x, dtype=torch.int32, device=dev).contiguous()
    sort_idx, wstart, wlen, qc = i32(case.sort_idx), i32(case.wstart), i32(case.wlen), i32(case.qc)
    radial = torch.as_tensor(case.radial, device=dev) if case.sphere else None
    tq, tk, tv = (t.to(dev).contiguous() for t in (case.tq, case.tk, case.tv))
    nan = lambda *s: torch.full(s, float('nan'), device=dev)
    out, lse = nan(n, H, 16), nan(n, h)
    dqkv = torch.full((n, 3, H, 16), SENTINEL, device=dev)
    dtq, dtk, dtv = nan(*tq.shape), nan(*tq.shape), nan(*tq.shape)
    delta = torch.empty(n, h, device=dev)
    nbytes = L.load().u2mkd_sptr_backward_workspace_bytes(n, h, case.L)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    st = L.stream()
    ld = 3 * H * 16
    plan = (L.ptr(sort_idx), L.ptr(wstart), L.ptr(wlen), L.ptr(qc), L.ptr(radial), L.ptr(tq), L.ptr(tk), L.ptr(tv), case.L,
            case.qgl, case.a)
    L.call('u2mkd_sptr_attention_forward_strided', L.ptr(qkv[:, 0, 1:]), L.ptr(qkv[:, 1, 1:]), L.ptr(qkv[:, 2, 1:]), ld,
           case.q_scale, *plan, n, h, 16, L.ptr(out[:, 1:]), H * 16, L.ptr(lse), st)
    L.call('u2mkd_sptr_attention_backward_strided', L.ptr(qkv[:, 0, 1:]), L.ptr(qkv[:, 1, 1:]), L.ptr(qkv[:, 2, 1:]), ld,
           case.q_scale, L.ptr(out[:, 1:]), L.ptr(dout[:, 1:]), H * 16, L.ptr(lse), *plan, case.qc_span, n, h, 16, L.ptr(delta),
           L.ptr(ws), nbytes, L.ptr(dqkv[:, 0, 1:]), L.ptr(dqkv[:, 1, 1:]), L.ptr(dqkv[:, 2, 1:]), ld, None, None, None, st)
    L.call('u2mkd_sptr_table_reduce', L.ptr(ws), n, h, case.L, case.a, L.ptr(dtq), L.ptr(dtk), L.ptr(dtv), st)
    torch.cuda.synchronize()
    return {'out': out, 'lse': lse, 'dqkv': dqkv, 'dTq': dtq, 'dTk': dtk, 'dTv': dtv}


@pytest.mark.parametrize('S,sphere,merge,h,big', R.gpu_cases(), ids=[R.case_id(c) for c in R.gpu_cases()])
def test_split_form_equals_the_float64_reference_elementwise(hip, monkeypatch, S, sphere, merge, h, big):
    monkeypatch.setenv('U2MKD_SPTR_SPLIT', str(S))
    if merge:
        monkeypatch.delenv('U2MKD_SPTR_BWD_MERGE', raising=False)
    else:
        monkeypatch.setenv('U2MKD_SPTR_BWD_MERGE', '0')
    dev = torch.device('cuda')
    case, ref, mag, mag_abs = _reference(S, sphere, h, big)
    assert case.edge_slack() > 1.0                                             # no pair near a radial bin edge, none dropped
    tpb = 128 // S                                                             # tokens per workgroup pass
    assert case.n % tpb != 0
    if S > 1 or big:
        assert -(-case.n // tpb) > (512 if S == 1 else 128)                    # the persistent backward grid takes a second pass

    def views(r):
        return {'out': r['out'][:, 1:], 'lse': r['lse'], 'dq': r['dqkv'][:, 0, 1:], 'dk': r['dqkv'][:, 1, 1:],
                'dv': r['dqkv'][:, 2, 1:], 'dTq': r['dTq'], 'dTk': r['dTk'], 'dTv': r['dTv']}
    first = _run(hip, case, dev)
    got = views(first)
    # the other branch's columns: untouched
    assert bool((first['dqkv'][:, :, 0] == SENTINEL).all())
    assert bool(torch.isnan(first['out'][:, 0]).all())
    figures, failed = [], []
    for kind in R.KINDS:
        x = got[kind]
        assert bool(torch.isfinite(x).all()), kind
        w, w_abs = R.worst(kind, x, ref[kind], mag[kind]), R.worst(kind, x, ref[kind], mag_abs[kind])
        figures.append('%s %.2e/%.1e %.2e/%.1e' % (kind, w, R.KAPPA[kind], w_abs, R.KAPPA_ABS[kind]))
        bad = int(R.violations(kind, x, ref[kind], mag[kind]).sum())
        bad_abs = int(R.violations(kind, x, ref[kind], mag_abs[kind], kappa=R.KAPPA_ABS[kind]).sum())
        if bad or bad_abs:
            failed.append((kind, bad, bad_abs))
    print('\n%s n=%d  max err/magnitude vs kappa (factor | term-wise): %s' % (R.case_id((S, sphere, merge, h, big)), case.n,
                                                                           '; '.join(figures)))
    assert not failed, (failed, figures)
    again = views(_run(hip, case, dev))
    for kind in R.KINDS:
        assert torch.equal(got[kind], again[kind]), kind
