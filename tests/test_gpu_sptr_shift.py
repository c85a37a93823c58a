"""Shifted window plans (sptr/utils.py:63-64), the shifted quantiser (sptr/modules.py:42-44) and sparse_self_attention in its
four served forms -- {contextual, none} x {shift_win, no shift} -- against the CPU oracle: the window decisions are integer
decisions on fp32 inputs and must be EQUAL (tokens on the shifted window / quantiser edges and one ulp either side
included), the attention is held to the gates of tests/test_gpu_sptr.py (forward <= 1e-5, every gradient <= 1e-4, relative
to the largest reference element) against oracle.sptr_layer_ref.layer(CpuBackend()) on pair lists built from the oracle's
clusters."""
import functools

import numpy as np
import pytest
import torch

from oracle import sptr_layer_ref as LR
from oracle import sptr_ref as S

pytestmark = pytest.mark.gpu

WINDOW = np.array([0.6, 0.6, 0.6])
QUANT = WINDOW / 24
QGL = 24
N, H = 3000, 2


@functools.lru_cache(maxsize=None)
def _scene():
    """~3000 tokens in two scenes; the second half sits on shifted-window edges (lo + k w - w / 2) and shifted quantiser edges
    (+ j quant), moved by -1 / 0 / +1 ulp: the construction of tests/test_gpu_sptr.py:160-165 moved by the shift."""
    g = torch.Generator().manual_seed(7)
    w, qz = torch.tensor(WINDOW).float(), torch.tensor(QUANT).float()
    xyz = torch.rand(N, 3, generator=g) * w * 7.3
    lo = xyz.min(0)[0]
    k = torch.randint(1, 7, (N // 2, 3), generator=g).float()
    j = torch.randint(0, 24, (N // 2, 3), generator=g).float()
    edge = lo + torch.where(torch.rand(N // 2, 3, generator=g) < 0.5, k * w - 0.5 * w, k * w - 0.5 * w + j * qz)
    ulp = torch.randint(-1, 2, (N // 2, 3), generator=g)
    edge = torch.where(ulp > 0, torch.nextafter(edge, edge + 1), torch.where(ulp < 0, torch.nextafter(edge, edge - 1), edge))
    xyz[N // 2:] = edge
    xyz[0] = lo                                                     # keep the minimum where it was
    batch = torch.sort(torch.randint(0, 2, (N,), generator=g))[0]
    assert torch.equal(xyz.min(0)[0], lo)
    return xyz, batch


@functools.lru_cache(maxsize=None)
def _oracle_plan(shift):
    """the reference's get_indices_params (sptr/utils.py:49-78) on the CPU, shift_win included: (cluster, sort_idx, counts of
    the sorted unique clusters, window index of every sorted position, pair lists of the oracle layer)"""
    xyz, batch = _scene()
    w = torch.from_numpy(WINDOW).type_as(xyz)
    if shift:
        cluster = S.grid_cluster(xyz + 1 / 2 * w, batch, w, start=xyz.min(0)[0])
    else:
        cluster = S.grid_cluster(xyz, batch, w, None)
    _, v2p, counts = torch.unique(cluster, sorted=True, return_inverse=True, return_counts=True)
    v2p_sorted, sort_idx = v2p.sort(stable=True)
    lay = LR.layer(LR.CpuBackend())
    n_max = int(counts.max())
    i0o, i1o, i0, i1 = lay.precompute_all(v2p.shape[0], counts.shape[0], n_max, counts)
    return cluster, sort_idx, counts, v2p_sorted, (i0.long(), i0o, n_max, i1.long(), i1o, sort_idx)


def _rel(a, b):
    a, b = a.double().cpu(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


@pytest.mark.parametrize('shift', [False, True], ids=['plain', 'shifted'])
def test_window_plan_and_quantiser_decisions_equal_the_oracle(hip, shift):
    from u2mkd_amd import sptr
    xyz, batch = _scene()
    cluster, sort_idx, counts, v2p_sorted, _ = _oracle_plan(shift)
    plan = sptr.WindowPlan(xyz.cuda(), batch.cuda(), WINDOW, shift_win=shift)
    assert plan.shift_win is shift
    assert torch.equal(plan.lo.cpu()[:3], xyz.min(0)[0])                               # the UNSHIFTED minimum, shifted or not
    assert torch.equal(plan.sort_idx.cpu().long(), sort_idx)                           # the window order and the order inside
    starts = torch.cat([counts.new_zeros(1), counts.cumsum(0)[:-1]])
    assert torch.equal(plan.wstart.cpu().long(), starts[v2p_sorted])                   # the window of every token
    assert torch.equal(plan.wlen.cpu().long(), counts[v2p_sorted])
    if shift:                                                                          # (the shift does move tokens)
        assert not torch.equal(_oracle_plan(False)[1], sort_idx)
    # in-window quantised coordinates (sptr/modules.py:41-44), sorted order
    qc, _, span = plan.quant_coords(xyz.cuda(), QUANT, False)
    w = torch.from_numpy(WINDOW).float()
    xyz_ctg = xyz[sort_idx]
    shift_size = 1 / 2 * w if shift else 0.0
    want = torch.div((xyz_ctg - xyz_ctg.min(0)[0] + shift_size) % w, torch.from_numpy(QUANT).float(), rounding_mode='floor')
    assert torch.equal(qc.cpu(), want.int())
    assert int(want.max()) < span and int(want.min()) == 0
    assert len(torch.unique(want)) >= 24


@functools.lru_cache(maxsize=None)
def _operands():
    g = torch.Generator().manual_seed(9)
    q, k, v, go = (torch.randn(N, H, 16, generator=g) for _ in range(4))
    tabs = tuple(0.3 * torch.randn(2 * QGL - 1, 3, H, 16, generator=g) for _ in range(3))
    return q, k, v, go, tabs


@functools.lru_cache(maxsize=None)
def _oracle_attention(contextual, shift):
    """(out, gradients of q, k, v and -- contextual -- the three tables) of the oracle layer, once per form"""
    xyz, _ = _scene()
    q, k, v, go, tabs = _operands()
    lay = LR.layer(LR.CpuBackend())
    i0, i0o, n_max, i1, i1o, sort_idx = _oracle_plan(shift)[4]
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v) + (tabs if contextual else ())]
    kw = dict(pe_type='contextual', rel_query=True, rel_key=True, rel_value=True, quant_size=QUANT, quant_grid_length=QGL,
              relative_pos_query_table=leaves[3], relative_pos_key_table=leaves[4],
              relative_pos_value_table=leaves[5]) if contextual else {}
    out = lay.sparse_self_attention(leaves[0], leaves[1], leaves[2], xyz, i0, i0o, n_max, i1, i1o, sort_idx, WINDOW, shift, **kw)
    out.backward(go)
    return out.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize('shift', [False, True], ids=['plain', 'shifted'])
@pytest.mark.parametrize('contextual', [True, False], ids=['contextual', 'none'])
def test_sparse_self_attention_equals_the_oracle_layer(hip, contextual, shift):
    from u2mkd_amd import sptr
    xyz, batch = _scene()
    q, k, v, go, tabs = _operands()
    want, want_grads = _oracle_attention(contextual, shift)
    leaves = [t.clone().cuda().requires_grad_(True) for t in (q, k, v) + (tabs if contextual else ())]
    i0, i0o, n_max, i1, i1o, sort_idx = sptr.get_indices_params(xyz.cuda(), batch.cuda(), WINDOW, shift)
    kw = dict(pe_type='contextual', rel_query=True, rel_key=True, rel_value=True, quant_size=QUANT, quant_grid_length=QGL,
              relative_pos_query_table=leaves[3], relative_pos_key_table=leaves[4],
              relative_pos_value_table=leaves[5]) if contextual else {}
    out = sptr.sparse_self_attention(leaves[0], leaves[1], leaves[2], xyz.cuda(), i0.int(), i0o.int(), n_max, i1.int(), i1o.int(),
                                     sort_idx, WINDOW, shift, **kw)
    out.backward(go.cuda())
    figures = ['out %.2e' % _rel(out.detach(), want)]
    names = ('dq', 'dk', 'dv', 'dTq', 'dTk', 'dTv')
    figures += ['%s %.2e' % (n, _rel(t.grad, g)) for n, t, g in zip(names, leaves, want_grads)]
    print('\n%s %s: %s' % ('contextual' if contextual else 'none', 'shifted' if shift else 'plain', '; '.join(figures)))
    assert _rel(out.detach(), want) < 1e-5
    for n, t, g in zip(names, leaves, want_grads):
        assert _rel(t.grad, g) < 1e-4, n


def test_shift_win_that_differs_from_the_plan_raises(hip):
    from u2mkd_amd import sptr
    xyz, batch = _scene()
    q = torch.randn(N, H, 16).cuda()
    for built, asked in ((False, True), (True, False)):
        r = sptr.get_indices_params(xyz.cuda(), batch.cuda(), WINDOW, built)
        with pytest.raises(ValueError, match='shift_win'):
            sptr.sparse_self_attention(q, q, q, xyz.cuda(), r[0], r[1], r[2], r[3], r[4], r[5], WINDOW, asked)
    # a subset of the relative-position terms stays unimplemented
    r = sptr.get_indices_params(xyz.cuda(), batch.cuda(), WINDOW, False)
    t = torch.zeros(47, 3, H, 16).cuda()
    with pytest.raises(NotImplementedError):
        sptr.sparse_self_attention(q, q, q, xyz.cuda(), r[0], r[1], r[2], r[3], r[4], r[5], WINDOW, False, pe_type='contextual',
                                   rel_query=True, rel_key=True, rel_value=False, quant_size=QUANT, quant_grid_length=QGL,
                                   relative_pos_query_table=t, relative_pos_key_table=t)
