"""sptr.VarLengthMultiheadSA on the GPU, forward and backward, for the four pe_types and both shift_win values against a
restatement of the reference module's forward (sptr/modules.py:122-199) on the CPU: torch's linear layers with the module's
weights, the position embedding per scene added in place to query and key, and the oracle's Python layer
(oracle.sptr_layer_ref.layer(CpuBackend())) on pair lists built from the oracle's clusters.  Gates of tests/test_gpu_sptr.py:
forward <= 1e-5, every gradient (input features, linears, tables) <= 1e-4, relative to the largest reference element.

One deliberate difference from the reference copy this project was modelled on: its module never hands ``pe_type`` to
sparse_self_attention (sptr/modules.py:166-189), so its 'contextual' module computes table-free attention and its three
tables never receive a gradient.  The module here passes it -- the tables it constructs are used -- and so does this
restatement.

The key bias of the table-free forms: softmax_j((q_i . (k_j + b)) = softmax_j(q_i . k_j), so d(k.bias) = sum_j dk_j is
ANALYTICALLY ZERO there ('none', 'sine', 'fourier'; with tables k_j . Tk(r_ij) makes it a real gradient) and both sides hold
nothing but the rounding of that cancelling sum (~1e-7 against terms of ~1): relative to the largest reference element the
gate would compare noise with noise.  For this one gradient the 1e-4 is therefore taken relative to what the sum is made
of -- the largest column sum of |dk_j| of the restatement -- which is the same relative bound on the same sum and the one
that can fail (a kernel that drops one dk row moves the sum by a whole term, far above 1e-4 of the column sum of 600)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sptr_layer_ref as LR
from oracle import sptr_ref as S

pytestmark = pytest.mark.gpu

N, C, HEADS = 600, 32, 2
WINDOW = [0.6, 0.6, 0.6]
QUANT = [0.025, 0.025, 0.025]
PE_TYPES = ('none', 'sine', 'fourier', 'contextual')


@functools.lru_cache(maxsize=None)
def _scene():
    g = torch.Generator().manual_seed(31)
    xyz = torch.rand(N, 3, generator=g) * torch.tensor([2.4, 2.4, 1.2]) - torch.tensor([1.0, 1.3, 0.2])
    batch = torch.cat([torch.zeros(330), torch.ones(N - 330)])
    feats = torch.randn(N, C, generator=g)
    gout = torch.randn(N, C, generator=g)
    return torch.cat([batch[:, None], xyz], 1), feats, gout


def _build(pe_type, shift):
    from u2mkd_amd import sptr
    torch.manual_seed(5)
    kw = dict(rel_query=True, rel_key=True, rel_value=True, quant_size=QUANT) if pe_type == 'contextual' else {}
    m = sptr.VarLengthMultiheadSA(C, HEADS, 'win', WINDOW, shift_win=shift, pe_type=pe_type, **kw)
    for n, p in m.named_parameters():
        if 'table' in n:
            torch.nn.init.normal_(p, std=0.2)
    return m


def _pairs(xyz, batch, shift):
    w = torch.tensor(WINDOW)
    cluster = S.grid_cluster(xyz + 1 / 2 * w, batch, w, start=xyz.min(0)[0]) if shift else S.grid_cluster(xyz, batch, w, None)
    _, v2p, counts = torch.unique(cluster, sorted=True, return_inverse=True, return_counts=True)
    _, sort_idx = v2p.sort(stable=True)
    lay = LR.layer(LR.CpuBackend())
    n_max = int(counts.max())
    i0o, i1o, i0, i1 = lay.precompute_all(N, counts.shape[0], n_max, counts)
    return lay, (i0.long(), i0o, n_max, i1.long(), i1o, sort_idx)


def _restatement(m, pe_type, shift):
    """(out, query_feats after the call, {name: gradient}) of the reference's forward over the oracle layer, weights of ``m``"""
    indices, feats, gout = _scene()
    sd = {k: v.detach().clone().requires_grad_(v.dtype.is_floating_point and 'gauss' not in k) for k, v in m.state_dict().items()}
    x0 = feats.clone().requires_grad_(True)
    query = x0 * 1.0
    key, value = query.clone(), query.clone()
    xyz, batch = indices[:, 1:], indices[:, 0]
    if pe_type in ('sine', 'fourier'):
        rows = []
        for b in (0, 1):
            p = xyz[batch == b]
            rows.append(m.pos_enc(p[None], input_range=[p.min(0)[0][None], p.max(0)[0][None]])[0].permute(1, 0))
        pos_emb = torch.cat(rows, 0)
        query += pos_emb
        key += pos_emb
    after = query.detach().clone()
    q = F.linear(query, sd['q.weight'], sd['q.bias']).reshape(N, HEADS, C // HEADS) * m.scale
    k = F.linear(key, sd['k.weight'], sd['k.bias']).reshape(N, HEADS, C // HEADS)
    v = F.linear(value, sd['v.weight'], sd['v.bias']).reshape(N, HEADS, C // HEADS)
    k.retain_grad()
    lay, (i0, i0o, n_max, i1, i1o, sort_idx) = _pairs(xyz, batch, shift)
    kw = {}
    if pe_type == 'contextual':
        kw = dict(pe_type='contextual', rel_query=True, rel_key=True, rel_value=True, quant_size=np.array(QUANT),
                  quant_grid_length=m.quant_grid_length, relative_pos_query_table=sd['relative_pos_query_table'],
                  relative_pos_key_table=sd['relative_pos_key_table'], relative_pos_value_table=sd['relative_pos_value_table'])
    x = lay.sparse_self_attention(q.float(), k.float(), v.float(), xyz.float(), i0, i0o, n_max, i1, i1o, sort_idx, np.array(WINDOW),
                                  shift, **kw)
    out = F.linear(x.view(N, C), sd['proj.weight'], sd['proj.bias'])
    out.backward(gout)
    grads = {k: v.grad for k, v in sd.items() if v.requires_grad}
    grads['input'] = x0.grad
    return out.detach(), after, grads, float(k.grad.abs().sum(0).max())


def _rel(a, b):
    a, b = a.double().cpu(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


@pytest.mark.parametrize('shift', [False, True], ids=['plain', 'shifted'])
@pytest.mark.parametrize('pe_type', PE_TYPES)
def test_module_forward_backward_equal_the_restatement(hip, pe_type, shift):
    from u2mkd_amd import sptr
    indices, feats, gout = _scene()
    m = _build(pe_type, shift)
    want, want_after, want_grads, dk_terms = _restatement(m, pe_type, shift)
    m = m.cuda()
    x0 = feats.clone().cuda().requires_grad_(True)
    query = x0 * 1.0
    t = sptr.SparseTrTensor(query, indices.cuda(), None, 2)
    out = m(t)
    assert isinstance(out, sptr.SparseTrTensor) and out.query_indices is t.query_indices and out.batch_size == 2
    # the position embedding went into the caller's query_feats in place (sptr/modules.py:146); nothing else does
    assert t.query_feats is query and torch.allclose(query.detach().cpu(), want_after, rtol=0, atol=2e-5)
    assert (pe_type in ('sine', 'fourier')) == (not torch.equal(query.detach(), x0.detach()))
    out.query_feats.backward(gout.cuda())
    got = {n: p.grad for n, p in m.named_parameters()}
    got['input'] = x0.grad
    assert set(got) == set(want_grads)

    def rel(n):
        if n == 'k.bias' and pe_type != 'contextual':          # analytically zero: relative to the terms of the sum (docstring)
            return float((got[n].double().cpu() - want_grads[n].double()).abs().max() / dk_terms)
        return _rel(got[n], want_grads[n])
    figures = ['out %.2e' % _rel(out.query_feats.detach(), want)] + ['%s %.2e' % (n, rel(n)) for n in sorted(got)]
    print('\n%s %s: %s' % (pe_type, 'shifted' if shift else 'plain', '; '.join(figures)))
    assert _rel(out.query_feats.detach(), want) < 1e-5
    if pe_type != 'contextual':
        assert float(want_grads['k.bias'].abs().max()) < 1e-5 * dk_terms          # (zero up to rounding in the restatement too)
    for n in sorted(got):
        assert rel(n) < 1e-4, n


@pytest.mark.parametrize('pe_type', ['none', 'contextual'])
def test_second_call_on_the_same_tensor_takes_the_cached_plan(hip, monkeypatch, pe_type):
    from u2mkd_amd import sptr
    from u2mkd_amd.sptr import modules as M
    indices, feats, _ = _scene()
    m = _build(pe_type, True).cuda()
    t = sptr.SparseTrTensor(feats.clone().cuda(), indices.cuda(), None, 2)
    assert t.find_indice_params('win') is None
    with torch.no_grad():
        first = m(t).query_feats
        cached = t.indice_dict['win']
        assert isinstance(cached[0], sptr.WindowPlan) and cached[0].shift_win is True and cached[7] is True
        assert np.array_equal(cached[6], m.window_size)

        def refuse(*a, **k):
            raise AssertionError('the cached plan must be used')
        monkeypatch.setattr(M, 'get_indices_params', refuse)
        second = m(t).query_feats
        assert t.indice_dict['win'] is cached and torch.equal(first, second)
        other = _build(pe_type, False).cuda()                     # same key, another shift_win: the reference's assertion
        with pytest.raises(AssertionError, match='same indice_key'):
            other(t)
