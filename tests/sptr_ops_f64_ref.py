"""float64 statement of the nine float `sptr_cuda` operator entries (csrc/sptr_ops.hip, u2mkd_sptr_<name>), with the
magnitude and the term count of every output element (test helper; imports nothing from oracle/).

Each entry is written as explicit index sums over the pair list (index0[m] = query token, index1[m] = key token of pair m),
in the LAUNCHER's layouts, in the dtype asked for (float64 by default).  With T(m) = T[r1(m), 0] + T[r2(m), 1] + T[r3(m), 2]
the rows of a table selected by rel_idx of pair m, hh = c / d the head of channel c = hh d + j:

    entry (kernel)                                  output       element                                          terms  r_kind
    attention_step1_forward   (ops_scores<1>)       s1   [h,M]   sum_j q[hh,j,i0] k[hh,j,i1]                      d      1
    dot_prod_with_idx_forward (ops_scores<2>)       dp   [h,M]   sum_j q Tq(m)[j] + k Tk(m)[j]                    2d     3
    dot_prod_with_idx_all_forward (ops_scores<3>)   dpa  [h,M]   sum_j q (k + Tq(m)[j]) + k Tk(m)[j]              3d     4
    attention_step1_backward  (ops_step1_backward)  s1_gq [N,h,d] sum_{m: i0[m]=t} go[m,hh] k[i1[m],c]            L_w    1
                                                    s1_gk        sum_{m: i1[m]=t} go[m,hh] q[i0[m],c]             L_w    1
    attention_step2_forward   (ops_step2_forward<0>) s2_out      sum_{m: i0[m]=t} attn[m,hh] v[i1[m],c]           L_w    1
    attention_step2_backward  (ops_step2_grad_attn<0>) s2_ga [M,h] sum_j go[i0,hh,j] v[hh,j,i1]                   d      1
                              (ops_step2_grad_v<0>) s2_gv        sum_{m: i1[m]=t} attn[m,hh] go[i0[m],c]          L_w    1
    dot_prod_with_idx_backward (ops_dot_prod_backward) dp_gq     sum_{m: i0[m]=t} Tq(m)[c] go[m,hh]               L_w    3
                                                    dp_gk        sum_{m: i1[m]=t} Tk(m)[c] go[m,hh]               L_w    3
                                                    dp_gtq [L,3,h,d] sum_{m: rel[m,ax]=row} q[i0[m],c] go[m,hh]   hits   1
                                                    dp_gtk       sum_{m: rel[m,ax]=row} k[i1[m],c] go[m,hh]       hits   1
    attention_step2_with_rel_pos_value_forward (ops_step2_forward<1>)
                                                    rv_out       sum_{m: i0[m]=t} attn[m,hh] (v[i1[m],c] + Tv(m)[c])  L_w  4
    attention_step2_with_rel_pos_value_backward (ops_step2_grad_attn<1>)
                                                    rv_ga [M,h]  sum_j go[i0,hh,j] (Tv(m)[j] + v[hh,j,i1])        2d     4
                              (ops_step2_grad_v<1>) rv_gv        sum_{m: i1[m]=t} attn[m,hh] go[i0[m],c]          L_w    1
                                                    rv_gt [L,3,h,d] sum_{m: rel[ax,m]=row} attn[m,hh] go[i0[m],c] hits   1

``terms`` is the number of products added into the element: the scalar products of the written-out sum per pair (d, 2d, 3d) for
the per-pair outputs, the window length L_w for the per-token outputs, the number of pairs whose rel_idx hits (row, axis) for a
table gradient.  ``mag`` is the same sum with every factor (q, k, v, attn, grad_out, each of the three table entries) replaced by
its absolute value, so a sum of table entries plus v or k becomes a sum of absolute values.

THE GATE, elementwise, no element excluded, u = 2^-24:

    |kernel - float64| <= c u / (1 - c u) * mag,     c = terms + r_kind

the textbook bound (Higham, Accuracy and Stability, Lemma 3.1 / eq. 3.4) of an fp32 sum of ``terms`` products in ANY order --
sequential, the LDS atomics of the table gradients, the one global atomic per entry and workgroup -- whose every term carries
at most r_kind roundings before it enters the sum; fused multiply-add only removes roundings.  Where mag is 0 the bound is 0
and asks for equality (a table row no pair hits).  r_kind, counted from the kernel's expression:

    r = 1   `s += qs * ks`, `gq += go * k`, `sum += attn * v`, `g = attn * go`, `g = qv * go`: the product.
    r = 3   `(t1 + t2 + t3) * go` (dp_gq, dp_gk) and `qs * a`, `ks * b` with a, b = t1 + t2 + t3 (dp): two table additions, the
            product.
    r = 4   `qs * (ks + a)` (dpa): two table additions, the add of k, the product (the `ks * b` terms carry 3);
            `attn * (v + t1 + t2 + t3)` (rv_out) and `go * (t1 + t2 + t3 + v)` (rv_ga): three additions, the product.

No kind needs more than 4.  A sum of n terms adds at most n - 1 roundings to any term (the first add, to 0, is exact), so
c = terms + r_kind has one rounding to spare.

THE fp32 SELF-CHECK (tests/test_sptr_ops_f64_reference.py::test_fp32_evaluation_sits_inside_the_gate_in_two_orders): this
statement evaluated in fp32 on the CPU, pairs in ascending m and in a fixed random permutation of m, against float64, worst
err / bound per kind over the six cases (torch 2.x CPU):

    kind     ascending  permuted      kind     ascending  permuted
    s1       0.226      0.226         dp_gq    0.600      0.600
    dp       0.053      0.053         dp_gk    0.621      0.621
    dpa      0.032      0.032         dp_gtq   0.107      0.124
    s1_gq    0.572      0.572         dp_gtk   0.108      0.104
    s1_gk    0.517      0.517         rv_out   0.394      0.394
    s2_out   0.577      0.577         rv_ga    0.072      0.072
    s2_ga    0.208      0.208         rv_gv    0.610      0.610
    s2_gv    0.610      0.610         rv_gt    0.137      0.119

(The per-pair kinds sum over j only and do not see the pair order.  The per-token maxima sit in the windows of one to three
tokens, where c is 2 to 7 and every rounding counts; in the 257-token window and in the table gradients the worst-case bound
has room, as a worst-case bound of a long sum must.)
"""
import functools

import torch

U = 2.0 ** -24

# constants of csrc/sptr_ops.hip (pinned against the source by the host tests)
K_OP_THREADS = 256          # kOpThreads: pairs per workgroup of the per-pair kernels, channels per blockIdx.y of the token kernels
K_GT_TOK = 4                # kGtTok: token slots per workgroup of the two table-gradient kernels
K_GT_CW = 64                # kGtCW: channels per workgroup of the two table-gradient kernels
HDIM_MAX, L_MAX = 64, 50    # check_hd

R_KIND = {'s1': 1, 'dp': 3, 'dpa': 4, 's1_gq': 1, 's1_gk': 1, 's2_out': 1, 's2_ga': 1, 's2_gv': 1, 'dp_gq': 3, 'dp_gk': 3,
          'dp_gtq': 1, 'dp_gtk': 1, 'rv_out': 4, 'rv_ga': 4, 'rv_gv': 1, 'rv_gt': 1}
KINDS = tuple(R_KIND)
ENTRIES = {'attention_step1_forward': ('s1',), 'dot_prod_with_idx_forward': ('dp',), 'dot_prod_with_idx_all_forward': ('dpa',),
           'attention_step1_backward': ('s1_gq', 's1_gk'), 'attention_step2_forward': ('s2_out',),
           'attention_step2_backward': ('s2_ga', 's2_gv'), 'dot_prod_with_idx_backward': ('dp_gq', 'dp_gk', 'dp_gtq', 'dp_gtk'),
           'attention_step2_with_rel_pos_value_forward': ('rv_out',),
           'attention_step2_with_rel_pos_value_backward': ('rv_ga', 'rv_gv', 'rv_gt')}
PER_PAIR = ('s1', 'dp', 'dpa', 's2_ga', 'rv_ga')                         # [h,M] or [M,h]
PER_TOKEN = ('s1_gq', 's1_gk', 's2_out', 's2_gv', 'dp_gq', 'dp_gk', 'rv_out', 'rv_gv')
TABLE_GRADS = ('dp_gtq', 'dp_gtk', 'rv_gt')                              # atomics: the caller zeroes them
PLAIN_STORES = PER_PAIR + PER_TOKEN
ORDER_FREE = PER_PAIR                                                    # sums over j only


def scores_lds_bytes(hdim, L):
    """dynamic LDS of ops_scores_kernel<2/3>: both tables of one head, [2][hdim][3][L] floats"""
    return 2 * hdim * 3 * L * 4


def dot_prod_backward_lds_bytes(L):
    """dynamic LDS of ops_dot_prod_backward_kernel: both table gradients of a channel slice, [2][3L][kGtCW] floats"""
    return 2 * 3 * L * K_GT_CW * 4


# ---- layouts ------------------------------------------------------------------------------------------------------------------

def t3(x):
    """[N,h,d] -> [h,d,N] (the caller's transpose of q, k, v)"""
    return x.permute(1, 2, 0).contiguous()


def tt(x):
    """[L,3,h,d] -> [h,d,3,L] (the caller's transpose of a table)"""
    return x.permute(2, 3, 1, 0).contiguous()


def _nhd(x_t):
    return x_t.permute(2, 0, 1)


def _l3hd(t_t):
    return t_t.permute(3, 2, 0, 1)


def _ident(x):
    return x


def _tsum(table, rel, first=None, last=None):
    """table [L,3,...], rel [M,3] -> [M,...]: the three selected rows in the kernels' association, v or k added first or last"""
    x = table[rel[:, 0], 0] if first is None else first + table[rel[:, 0], 0]
    x = x + table[rel[:, 1], 1] + table[rel[:, 2], 2]
    return x if last is None else x + last


def _scatter(rows, index, src):
    if src.is_cuda and rows <= L_MAX and src.dtype == torch.float64:
        # a table gradient on the device: index_add would serialise M float64 atomics on one address when every pair hits one
        # row (13 s for `one-entry`); the same sum as a one-hot product.  Rows no pair hits are sums of +-0 products: zero.
        onehot = (torch.arange(rows, device=src.device)[:, None] == index[None, :]).to(src.dtype)
        return onehot @ src
    return torch.zeros((rows,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device).index_add(0, index, src)


def _count(index, rows):
    return torch.bincount(index, minlength=rows)


def _head_of_channel(h, d, head_of_channel, device):
    if head_of_channel is None:
        return torch.arange(h * d, device=device) // d
    return torch.as_tensor(head_of_channel, dtype=torch.int64, device=device)


def _pack(names, ev, magnitudes, terms):
    res = dict(zip(names, ev(_ident)))
    if not magnitudes:
        return res
    with torch.no_grad():
        mag = dict(zip(names, ev(torch.abs)))
        trm = {n: t.expand(res[n].shape) for n, t in zip(names, terms())}
    return res, mag, trm


# ---- the per-pair entries -----------------------------------------------------------------------------------------------------

def _scores(mode, name, q_t, k_t, index_q, index_k, table_q_t, table_k_t, rel_t, dtype, magnitudes):
    q, k = _nhd(q_t.to(dtype)), _nhd(k_t.to(dtype))
    iq, ik = index_q.long(), index_k.long()
    d = q.shape[2]
    if mode != 1:
        tq, tk, rel = _l3hd(table_q_t.to(dtype)), _l3hd(table_k_t.to(dtype)), rel_t.long().t()

    def ev(a):
        qs, ks = a(q)[iq], a(k)[ik]                                         # [M,h,d]
        if mode == 1:
            e = qs * ks
        elif mode == 2:
            e = qs * _tsum(a(tq), rel) + ks * _tsum(a(tk), rel)
        else:
            e = qs * (ks + _tsum(a(tq), rel)) + ks * _tsum(a(tk), rel)
        return (e.sum(-1).t(),)                                             # [h,M]

    return _pack((name,), ev, magnitudes, lambda: (torch.full((1, 1), mode * d, device=q.device),))   # d, 2d, 3d products


def attention_step1_forward(q_t, k_t, index0, index1, dtype=torch.float64, magnitudes=True):
    """q_t [h,d,N_q], k_t [h,d,N_k] -> s1 [h,M]"""
    return _scores(1, 's1', q_t, k_t, index0, index1, None, None, None, dtype, magnitudes)


def dot_prod_with_idx_forward(q_t, index_q, k_t, index_k, table_q_t, table_k_t, rel_t, dtype=torch.float64, magnitudes=True):
    """q_t, k_t [h,d,N]; tables [h,d,3,L]; rel_t [3,M] -> dp [h,M]"""
    return _scores(2, 'dp', q_t, k_t, index_q, index_k, table_q_t, table_k_t, rel_t, dtype, magnitudes)


def dot_prod_with_idx_all_forward(q_t, index_q, k_t, index_k, table_q_t, table_k_t, rel_t, dtype=torch.float64,
                                  magnitudes=True):
    """q_t, k_t [h,d,N]; tables [h,d,3,L]; rel_t [3,M] -> dpa [h,M]"""
    return _scores(3, 'dpa', q_t, k_t, index_q, index_k, table_q_t, table_k_t, rel_t, dtype, magnitudes)


# ---- the per-token entries.  ``walk_k = (token, pair)`` replaces the key-side walk {(index1[m], m)} and ``head_of_channel`` the
# map c -> c / d: the corruptions of tests/test_sptr_ops_f64_reference.py, nothing else passes them. -----------------------------

def _key_walk(index1, walk_k):
    if walk_k is None:
        return index1, None
    return walk_k[0].long(), walk_k[1].long()


def _at(x, m):
    return x if m is None else x[m]


def attention_step1_backward(grad_out, index0, index1, q, k, dtype=torch.float64, magnitudes=True, walk_k=None,
                             head_of_channel=None):
    """grad_out [M,h]; q, k [N,h,d] -> s1_gq, s1_gk [N,h,d]"""
    N, h, d = q.shape
    go, q2, k2 = grad_out.to(dtype), q.to(dtype).reshape(N, h * d), k.to(dtype).reshape(N, h * d)
    i0, i1 = index0.long(), index1.long()
    kt, km = _key_walk(i1, walk_k)
    hc = _head_of_channel(h, d, head_of_channel, go.device)

    def ev(a):
        g = a(go)[:, hc]                                                    # [M,C]
        gq = _scatter(N, i0, g * a(k2)[i1])
        gk = _scatter(N, kt, _at(g, km) * a(q2)[_at(i0, km)])
        return gq.view(N, h, d), gk.view(N, h, d)

    return _pack(('s1_gq', 's1_gk'), ev, magnitudes, lambda: (_count(i0, N)[:, None, None], _count(kt, N)[:, None, None]))


def _step2_forward(name, attn, v, index0, index1, table, rel, dtype, magnitudes, head_of_channel):
    N, h, d = v.shape
    at, v2 = attn.to(dtype), v.to(dtype).reshape(N, h * d)
    i0, i1 = index0.long(), index1.long()
    hc = _head_of_channel(h, d, head_of_channel, at.device)
    if table is not None:
        tb, r = table.to(dtype).reshape(table.shape[0], 3, h * d), rel.long()

    def ev(a):
        val = a(v2)[i1]
        if table is not None:
            val = _tsum(a(tb), r, first=val)
        return (_scatter(N, i0, a(at)[:, hc] * val).view(N, h, d),)

    return _pack((name,), ev, magnitudes, lambda: (_count(i0, N)[:, None, None],))


def attention_step2_forward(attn, v, index0, index1, dtype=torch.float64, magnitudes=True, head_of_channel=None):
    """attn [M,h]; v [N,h,d] -> s2_out [N,h,d]"""
    return _step2_forward('s2_out', attn, v, index0, index1, None, None, dtype, magnitudes, head_of_channel)


def attention_step2_with_rel_pos_value_forward(attn, v, index0, index1, table, rel, dtype=torch.float64, magnitudes=True,
                                               head_of_channel=None):
    """attn [M,h]; v [N,h,d]; table [L,3,h,d]; rel [M,3] -> rv_out [N,h,d]"""
    return _step2_forward('rv_out', attn, v, index0, index1, table, rel, dtype, magnitudes, head_of_channel)


def _step2_backward(names, grad_out, index0, index1, attn, v_t, table_t, rel_t, dtype, magnitudes, walk_k, head_of_channel):
    N, h, d = grad_out.shape
    go, at, v = grad_out.to(dtype), attn.to(dtype), _nhd(v_t.to(dtype))
    i0, i1 = index0.long(), index1.long()
    kt, km = _key_walk(i1, walk_k)
    hc = _head_of_channel(h, d, head_of_channel, go.device)
    rpe = table_t is not None
    if rpe:
        tb, r = _l3hd(table_t.to(dtype)), rel_t.long().t()
        L = tb.shape[0]
        rk = _at(r, km)

    def ev(a):
        val = a(v)[i1]                                                      # [M,h,d]
        if rpe:
            val = _tsum(a(tb), r, last=val)
        ga = (a(go)[i0] * val).sum(-1)                                      # [M,h]
        g = _at(a(at)[:, hc], km) * a(go).reshape(N, h * d)[_at(i0, km)]    # [M,C], the key-side walk
        out = [ga, _scatter(N, kt, g).view(N, h, d)]
        if rpe:
            out.append(torch.stack([_scatter(L, rk[:, ax], g) for ax in range(3)], 1).view(L, 3, h, d))
        return out

    def terms():
        out = [torch.full((1, 1), (2 if rpe else 1) * d, device=go.device), _count(kt, N)[:, None, None]]
        if rpe:
            out.append(torch.stack([_count(rk[:, ax], L) for ax in range(3)], 1)[:, :, None, None])
        return out

    return _pack(names, ev, magnitudes, terms)


def attention_step2_backward(grad_out, index0, index1, attn, v_t, dtype=torch.float64, magnitudes=True, walk_k=None,
                             head_of_channel=None):
    """grad_out [N,h,d]; attn [M,h]; v_t [h,d,N] -> s2_ga [M,h], s2_gv [N,h,d]"""
    return _step2_backward(('s2_ga', 's2_gv'), grad_out, index0, index1, attn, v_t, None, None, dtype, magnitudes, walk_k,
                           head_of_channel)


def attention_step2_with_rel_pos_value_backward(grad_out, index0, index1, attn, v_t, table_t, rel_t, dtype=torch.float64,
                                                magnitudes=True, walk_k=None, head_of_channel=None):
    """grad_out [N,h,d]; attn [M,h]; v_t [h,d,N]; table_t [h,d,3,L]; rel_t [3,M] -> rv_ga [M,h], rv_gv [N,h,d], rv_gt [L,3,h,d]"""
    return _step2_backward(('rv_ga', 'rv_gv', 'rv_gt'), grad_out, index0, index1, attn, v_t, table_t, rel_t, dtype, magnitudes,
                           walk_k, head_of_channel)


def dot_prod_with_idx_backward(grad_out, q, index_q, k, index_k, table_q, table_k, rel, dtype=torch.float64, magnitudes=True,
                               walk_k=None, head_of_channel=None):
    """grad_out [M,h]; q, k [N,h,d]; tables [L,3,h,d]; rel [M,3] -> dp_gq, dp_gk [N,h,d], dp_gtq, dp_gtk [L,3,h,d]"""
    N, h, d = q.shape
    C, L = h * d, table_q.shape[0]
    go, q2, k2 = grad_out.to(dtype), q.to(dtype).reshape(N, C), k.to(dtype).reshape(N, C)
    tq, tk = table_q.to(dtype).reshape(L, 3, C), table_k.to(dtype).reshape(L, 3, C)
    i0, i1, r = index_q.long(), index_k.long(), rel.long()
    kt, km = _key_walk(i1, walk_k)
    rk = _at(r, km)
    hc = _head_of_channel(h, d, head_of_channel, go.device)

    def ev(a):
        g = a(go)[:, hc]                                                    # [M,C]
        gk_side = _at(g, km)
        gq = _scatter(N, i0, _tsum(a(tq), r) * g)
        gk = _scatter(N, kt, _tsum(a(tk), rk) * gk_side)
        eq = a(q2)[i0] * g                                                  # the query of the pair: the token of the query walk
        ek = a(k2)[kt] * gk_side                                            # the token of the key walk
        gtq = torch.stack([_scatter(L, r[:, ax], eq) for ax in range(3)], 1)
        gtk = torch.stack([_scatter(L, rk[:, ax], ek) for ax in range(3)], 1)
        return gq.view(N, h, d), gk.view(N, h, d), gtq.view(L, 3, h, d), gtk.view(L, 3, h, d)

    def terms():
        hq = torch.stack([_count(r[:, ax], L) for ax in range(3)], 1)[:, :, None, None]
        hk = torch.stack([_count(rk[:, ax], L) for ax in range(3)], 1)[:, :, None, None]
        return _count(i0, N)[:, None, None], _count(kt, N)[:, None, None], hq, hk

    return _pack(('dp_gq', 'dp_gk', 'dp_gtq', 'dp_gtk'), ev, magnitudes, terms)


# ---- the gate -----------------------------------------------------------------------------------------------------------------

def bound(kind, mag, terms):
    c = terms.to(torch.float64) + R_KIND[kind]
    return c * U / (1.0 - c * U) * mag.to(torch.float64)


def violations(kind, got, ref, mag, terms):
    """elementwise mask of the elements OUTSIDE the gate (a NaN is outside)"""
    return ~((got.to(torch.float64) - ref).abs() <= bound(kind, mag, terms))


def worst(kind, got, ref, mag, terms):
    """max err / bound; an error against a zero bound is inf, no error against a zero bound is 0"""
    err, b = (got.to(torch.float64) - ref).abs(), bound(kind, mag, terms)
    ratio = torch.where(b > 0, err / b, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float('inf'))))
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float('inf')), ratio)
    return float(ratio.max()) if ratio.numel() else 0.0


# ---- the cases ----------------------------------------------------------------------------------------------------------------

_TAILS = (1, 2, 63, 64, 65, 257, 3, 1, 30)
_SMALL = (3, 1, 40, 9)
#          name         window lengths          h  hdim  L  rel_idx all zero
CASES = {'tails': (_TAILS, 3, 16, 7, False),
         'wide': ((5, 90, 1, 33, 2, 17), 5, 64, 13, False),
         'straddle': (_TAILS, 7, 24, 31, False),
         'one-entry': (_TAILS, 7, 24, 31, True),
         'ceiling': (_SMALL, 2, 64, 50, False),
         'under': (_SMALL, 2, 64, 42, False)}
CASE_NAMES = tuple(CASES)


def precompute_all(counts):
    """counts [n] -> index_0_offsets [N], index_1_offsets [N], index_0 [M], index_1 [M] (int32): pair m = sq_w + i L_w + t is
    (query start_w + i, key start_w + t); index_0_offsets[start_w + t] = sq_w + L_w t; index_1_offsets[start_w + t] = sq_w + t."""
    counts = torch.as_tensor(counts, dtype=torch.int64)
    start = torch.cumsum(counts, 0) - counts
    sq = torch.cumsum(counts * counts, 0) - counts * counts
    win = torch.repeat_interleave(torch.arange(len(counts)), counts)          # window of every token
    rank = torch.arange(int(counts.sum())) - start[win]                        # position of the token in its window
    i0o, i1o = sq[win] + counts[win] * rank, sq[win] + rank
    pw = torch.repeat_interleave(torch.arange(len(counts)), counts * counts)   # window of every pair
    pm = torch.arange(int((counts * counts).sum())) - sq[pw]
    i0 = start[pw] + torch.div(pm, counts[pw], rounding_mode='floor')
    i1 = start[pw] + pm % counts[pw]
    return i0o.int(), i1o.int(), i0.int(), i1.int()


class Case:
    """fp32 operands in the [N,h,d] / [L,3,h,d] / [M,3] / [M,h] layouts (t3, tt and .t() give the launchers' others)"""

    def __init__(self, name, counts, h, d, L, rel_zero=False, seed=0):
        self.name, self.h, self.d, self.L = name, h, d, L
        c = torch.as_tensor(counts, dtype=torch.int64)
        self.counts = c.int()
        self.offsets = torch.cat([c.new_zeros(1), c.cumsum(0)]).int()
        self.sq_offsets = torch.cat([c.new_zeros(1), (c * c).cumsum(0)]).int()
        self.n, self.n_max = len(c), int(c.max())
        self.N, self.M = int(c.sum()), int((c * c).sum())
        self.i0o, self.i1o, self.i0, self.i1 = precompute_all(c)
        g = torch.Generator().manual_seed(seed)
        N, M = self.N, self.M
        self.q, self.k, self.v, self.go_n = (torch.randn(N, h, d, generator=g) + 0.3 for _ in range(4))
        self.tq, self.tk, self.tv = (torch.randn(L, 3, h, d, generator=g) + 0.3 for _ in range(3))
        self.go_m = torch.randn(M, h, generator=g) + 0.3
        self.attn = torch.rand(M, h, generator=g)
        self.rel = torch.zeros(M, 3, dtype=torch.int32) if rel_zero else torch.randint(0, L, (M, 3), generator=g).int()

    @property
    def i0o_closed(self):
        """index_0_offsets with M appended, as sptr/functional.py:165 passes it (the kernels read entry t + 1)"""
        return torch.cat([self.i0o, torch.tensor([self.M], dtype=torch.int32)])


@functools.lru_cache(maxsize=None)
def get_case(name):
    """the case, built once and shared: nobody writes to it"""
    counts, h, d, L, rel_zero = CASES[name]
    return Case(name, counts, h, d, L, rel_zero, seed=1000 + CASE_NAMES.index(name))


@functools.lru_cache(maxsize=None)
def cross_case():
    """attention_step1_forward with N_q != N_k: q_t [h,d,37], k_t [h,d,53], 300 pairs drawn at random in range"""
    g = torch.Generator().manual_seed(77)
    h, d, Nq, Nk, M = 3, 16, 37, 53, 300
    q, k = torch.randn(Nq, h, d, generator=g) + 0.3, torch.randn(Nk, h, d, generator=g) + 0.3
    return dict(h=h, d=d, Nq=Nq, Nk=Nk, M=M, q_t=t3(q), k_t=t3(k), index0=torch.randint(0, Nq, (M,), generator=g).int(),
                index1=torch.randint(0, Nk, (M,), generator=g).int())


def evaluate(case, dtype=torch.float64, device='cpu', magnitudes=True, pairs=None, walk_k=None, rel=None, head_of_channel=None):
    """All sixteen outputs of the nine entries on ``case``: {kind: tensor} and, with ``magnitudes``, {kind: mag}, {kind: terms}.

    ``pairs`` (int64 [M']) lists the pairs that are summed, in the order they are summed (default: all, ascending m); the per-pair
    outputs of pairs left out stay 0, as in a zeroed buffer.  ``walk_k``, ``rel`` and ``head_of_channel`` replace the key-side walk,
    the relative indices and the head of a channel for the corruptions of the host tests."""
    dev = torch.device(device)
    mv = lambda x: x.to(dev)
    sel = (lambda x: mv(x)) if pairs is None else (lambda x: mv(x)[mv(pairs)])
    q, k, v, go_n, tq, tk, tv = (mv(x) for x in (case.q, case.k, case.v, case.go_n, case.tq, case.tk, case.tv))
    i0, i1, attn, go_m = sel(case.i0), sel(case.i1), sel(case.attn), sel(case.go_m)
    r = sel(case.rel if rel is None else rel)
    q_t, k_t, v_t, tq_t, tk_t, tv_t, r_t = t3(q), t3(k), t3(v), tt(tq), tt(tk), tt(tv), r.t().contiguous()
    kw = dict(dtype=dtype, magnitudes=magnitudes)
    tok = dict(kw, head_of_channel=head_of_channel)
    key = dict(tok, walk_k=None if walk_k is None else tuple(mv(x) for x in walk_k))
    parts = [attention_step1_forward(q_t, k_t, i0, i1, **kw),
             dot_prod_with_idx_forward(q_t, i0, k_t, i1, tq_t, tk_t, r_t, **kw),
             dot_prod_with_idx_all_forward(q_t, i0, k_t, i1, tq_t, tk_t, r_t, **kw),
             attention_step1_backward(go_m, i0, i1, q, k, **key),
             attention_step2_forward(attn, v, i0, i1, **tok),
             attention_step2_backward(go_n, i0, i1, attn, v_t, **key),
             dot_prod_with_idx_backward(go_m, q, i0, k, i1, tq, tk, r, **key),
             attention_step2_with_rel_pos_value_forward(attn, v, i0, i1, tv, r, **tok),
             attention_step2_with_rel_pos_value_backward(go_n, i0, i1, attn, v_t, tv_t, r_t, **key)]
    merged = [{}, {}, {}] if magnitudes else [{}]
    for p in parts:
        for dst, src in zip(merged, p if magnitudes else (p,)):
            dst.update(src)
    if pairs is not None:                                   # per-pair outputs back at their pair's place
        pr = mv(pairs)
        for dct in merged:
            for kind in PER_PAIR:
                x = dct[kind]
                if kind in ('s2_ga', 'rv_ga'):
                    dct[kind] = torch.zeros((case.M, case.h), dtype=x.dtype, device=dev).index_copy(0, pr, x.contiguous())
                else:
                    dct[kind] = torch.zeros((case.h, case.M), dtype=x.dtype, device=dev).index_copy(1, pr, x.contiguous())
    return merged if magnitudes else merged[0]
