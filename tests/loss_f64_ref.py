"""float64 reference of the loss kernels (csrc/lovasz.hip behind u2mkd_amd/losses.py: _LovaszFunction, _CrossEntropyFunction,
_KLDivFunction), and the elementwise bound the kernels are held to (test helper; plain torch on CPU tensors, no import of the
package's kernels).

WHAT IS COMPUTED, on the fp32 inputs AS STORED:

  Lovasz (classes='present')   probabilities p [P, C], int64 labels, ignore_index, upstream gradient g.  Per class c over the valid
      rows (label != ignore_index): fg = [label == c], e = |fg - p_c|, the entries sorted by e descending, cs(i) the number of
      foreground entries among the first i + 1, gts their total,
          jac(i) = 1 - (gts - cs(i)) / (gts + (i + 1) - cs(i))      grad(i) = jac(i) - jac(i - 1), grad(0) = jac(0)
          loss = 1 / max(#present, 1)  sum_{c present} sum_i e_i grad(i)             present: gts > 0
          d loss / d p[row, c] = -sgn(fg - p) grad(rank of the row in class c) g present_c / max(#present, 1);  0 on ignored rows
  Cross entropy   x [P, C], labels, ignore_index, g:  lse = log sum_c exp(x_c), loss = mean over the valid rows of lse - x[label]
      (0 / 0 = nan without a valid row), dx = g / count (softmax(x) - onehot) on the valid rows, 0 elsewhere.
  KL 'batchmean'   s [P, C], t [T, C], index [P] or None (row p of the teacher is t[index[p]]; T may be smaller or larger than P):
      p_t = softmax(t_row), loss = 1 / P sum_p sum_c p_t (log p_t - log_softmax(s)_c), a term with p_t = 0 counts 0;
      ds = g / P (softmax(s) - p_t).

THE BOUND is that of an evaluation in fp32 arithmetic in the kernels' order of operations, read from csrc/lovasz.hip and written
down below.  u = 2^-24 is fp32's unit roundoff, g(k) = k u / (1 - k u) bounds k roundings in a row.  Every term is u times a
magnitude THAT IS ACTUALLY SUMMED.  No constant is fitted to a measured error of the loss kernels.  The upstream gradient is
taken at its fp32 value (the kernels read a float).

 L1  e = fl(|fg - p|) is ONE IEEE operation (the subtraction; |.| is exact).  The reference computes it bit for bit in fp32 and
     takes the SORT ORDER from these fp32 values: the kernel's key c 2^32 + (0x7F800000 - bits(e)) is an integer, exact in double,
     that orders like (c, -e), so the device sort sees the same order.  The value of e that enters the float64 loss is the exact |fg - p|; its rounding is counted in L3.
 L2  jac(i) = fl(1 - fl(a / b)), a = gts - cs and b = gts + (i + 1) - cs integers below 2^24, exact in fp32: ONE division and ONE
     subtraction.  With q = a / b in [0, 1] and jac = 1 - q:  |jac^ - jac| <= u q + u jac + u^2 q <= u (1 + u) =: J.
     grad(i) = fl(jac^(i) - jac^(i - 1)) CANCELS down to about 1 / P, so its error does not scale with it:
         Eg(i) = 2 J + u (|grad(i)| + 2 J)   (i > 0),      Eg(0) = J
     an ABSOLUTE 2 u, not a relative one -- which is still 1e-4 of the 1 / P a rank off by one moves an entry by (P = 1500).
 L3  a term fl(e^ grad^) carries e's rounding and the product's.  The class sum is a 256-thread tree in LDS (8 additions on any
     path), then the nblk = ceil(P / 256) partials added one after the other, then lane c mod 64 adds its ceil(C / 64) classes
     (an addition to the initial 0 is exact), then the min(C, 64) lanes that hold something one after the other; the loss is the
     sum times fl(1 / #present): two more roundings.  D = 2 + 8 + nblk + (ceil(C / 64) - 1) + (min(C, 64) - 1) + 2 (``lovasz_depth``):
         bound(loss) = 1 / #present  sum_{c present} sum_i [ e_i Eg(i) + g(D) e_i (|grad(i)| + Eg(i)) ]
 L4  backward, fl(fl(-sgn grad^) fl(fl(g fl(1 / #present)) present_c)): the sign and present_c are exact, three roundings:
         bound(d) = |g| / #present (Eg + g(3) (|grad| + Eg))     on the entries of a present class with e > 0
     An entry with e == 0 (fg == p exactly: sgn = 0), an entry of an absent class and every entry of an ignored row have
     gradient EXACTLY 0: bound 0, which asks for equality.
 L5  TIES.  The sort is free to order entries of one class whose e are bit-equal.  A run of such entries that are all foreground
     has grad = 1 / b for every rank (b does not change along the run): decided.  A run with e > 0 that holds a background entry
     while foreground entries are still to come (a > 0) is UNDECIDED -- a mixed run, and a background-only run too, whose ranks
     carry a / (b (b - 1)) with b growing along the run: which entry gets which rank is the sort's choice, in the reference
     project as well.  For an undecided run that starts at rank i0 after k0 foreground and m0 = i0 - k0 background entries and
     holds nf foreground and nb background entries,
         a foreground entry has grad = 1 / (gts + m), m in [m0, m0 + nb]
         a background entry has grad = (gts - k) / ((gts + m)(gts + m - 1)), k in [k0, k0 + nf], m in [m0 + 1, m0 + nb]
     and an undecided entry's gradient must lie inside that ENVELOPE widened by bound(d) at its upper end.  The run's SUM of grad
     telescopes to jac(end) - jac(before) whatever the order: sum_run -sgn d is held to the sum of the run's bound(d) with no
     exclusion, and so are the loss (e is the same for the whole run) and every decided entry.  Condition on the inputs: at most
     UNDECIDED_CAP of a case's entries are undecided unless the case is built to tie (``TIE_CASES`` states their share).
 C1  cross entropy and KL, per row: m = max (exact), d_c = fl(x_c - m) (u |d_c|), expf of it (argument error e^{u |d|} - 1, then
     EXPF_ULP units in the last place, 2 u each, and one fp32 minimum normal TINY for results that underflow):
         ee_c = exp(d_c) (expm1(u |d_c|) + 2 u EXPF_ULP) + TINY
     s = the C terms added one after the other:  ds = sum ee + g(C - 1) (s + sum ee), s in [1, C];
     logf(s^):  El = r / (1 - r) + 2 u LOGF_ULP (|log s| + r / (1 - r)), r = ds / s;   lse^ = fl(m + logf): Ese = El + u (|lse| + El).
 C2  CE row loss fl(lse^ - x[label]): Er = Ese + u (|lse - x[label]| + Ese); rows >= 0.  The wave-64 butterfly is 6 additions, the 4
     wave partials 2 more; the finish adds the workgroup partials and divides by the (exact) count in DOUBLE and rounds once:
         bound(loss) = B + u (|loss| + B),   B = [ sum Er + g(8) sum (row + Er) ] / count
     CE backward fl(fl(g fl(1 / count)) fl(expf(fl(x - lse^)) - onehot)), p = softmax(x):
         Ep = p (expm1(Ese + u |x - lse|) + 2 u EXPF_ULP) + TINY      bound(dx) = |g| / count (Ep + g(4) (|p - onehot| + Ep))
 C3  KL forward: lse_s, lse_t as C1 (Es, Et).  lpt = fl(t_c - lt^): Elp = Et + u (|t_c - lt| + Et); pt = expf(lpt^):
         Ept = pt (expm1(Elp) + 2 u EXPF_ULP) + TINY;    sp = sum_c pt^ (C additions): Esp = sum Ept + g(C - 1) sum (pt + Ept)
     a = fl(s_c - ls^): Ea = Es + u (|s_c - ls| + Es);  b = fl(lpt^ - a^): Eb = Elp + Ea + u (|b| + Elp + Ea);
     term = fl(pt^ b^): Et_ = Ept (|b| + Eb) + pt Eb + u (pt + Ept)(|b| + Eb).  The terms have either sign; a row adds its C terms
     one after the other, then the butterfly and the partials (8), the finish in double times fl(1 / P) and one rounding:
         bound(loss) = B + 2 u (|loss| + B),   B = [ sum Et_ + g(C + 8) sum (|term| + Et_) ] / P
     KL backward fl(fl(g fl(1 / P)) fl(fl(expf(fl(s - ls^)) sp^) - pt^)), ps = softmax(s), sum p_t = 1:
         Eps = ps (expm1(Es + u |s - ls|) + 2 u EXPF_ULP) + TINY       Epr = Eps (1 + Esp) + ps Esp + u (ps + Eps)(1 + Esp)
         bound(ds) = |g| / P (Epr + Ept + g(4) (|ps - pt| + Epr + Ept))
     Note what C1 says about logits of large common magnitude: lse is stored in fp32, so Ese carries u |lse| (6e-4 at logits
     near 1e4) and every probability of the backward inherits it as a relative error.  That is the kernels' order of operations.

 EXPF_ULP / LOGF_ULP: the largest error of the device library's expf / logf in units in the last place.  The ROCm installation
 states it nowhere (no header, no document under share/doc), so they are MEASURED against float64 by tools/libm_ulp.py, which
 calls the two functions compiled with the library's flags on EVERY fp32 argument the kernels can pass (expf: [-104, -2^-30];
 logf: [1, 256]), and carry a factor 2 over the measured maximum.  They are not calibrated on the loss kernels.

WHAT THE BOUND CAN SEE.  ``WRONG`` names the formulations it has to reject (tests/test_host_loss_bound.py); ``honest_fp32`` is
the fp32 evaluation in the kernels' order that has to stay inside on every case of ``CASES``."""
import math

import torch

U32 = 2.0 ** -24
TINY = 2.0 ** -126
# measured by tools/libm_ulp.py on the MI355X (the device library's expf / logf at the library's flags, against float64):
#   expf  [-104, -2^-30]  307 232 769 values  max error 0.8567 ulp at x = -5.285436153411865   (subnormal results: 1 unit of 2^-149)
#   logf  [1, 256]         67 108 865 values  max error 2.3086 ulp at x = 7.308056354522705
# twice the measured maximum:
EXPF_ULP = 2 * 0.8567
LOGF_ULP = 2 * 2.3086
UNDECIDED_CAP = 0.01
LV_THREADS = 256
CE_THREADS = 256
FIN_LANES = 64


def g_(k):
    """k roundings in a row"""
    return k * U32 / (1.0 - k * U32)


def f32(v):
    """the fp32 value of a Python float (what a float argument receives)"""
    return float(torch.tensor(v, dtype=torch.float32))


def lovasz_depth(P, C):
    """L3: roundings on the way of one term into the loss"""
    nblk = -(-P // LV_THREADS)
    return 2 + 8 + nblk + (-(-C // FIN_LANES) - 1) + (min(C, FIN_LANES) - 1) + 2


# ---- Lovasz -------------------------------------------------------------------------------------------------------------------

def _lovasz_sorted(probas, labels, ignore):
    """the class-major sorted view of one input: everything [C, P], rank along dim 1, the ignored rows behind the valid ones"""
    p32 = probas.float()
    P, C = p32.shape
    valid = labels != ignore
    fg = (labels[None, :] == torch.arange(C)[:, None]) & valid[None, :]
    e32 = (fg.float() - p32.t()).abs()                                     # L1: bit for bit
    diff = fg.double() - p32.t().double()
    key = torch.where(valid[None, :], e32, torch.full_like(e32, -1.0))
    order = torch.sort(key, dim=1, descending=True, stable=True)[1]
    nv = int(valid.sum())
    live = (torch.arange(P)[None, :] < nv).expand(C, P)
    return {'P': P, 'C': C, 'order': order, 'nv': nv, 'live': live, 'fg': torch.gather(fg, 1, order),
            'e32': torch.gather(e32, 1, order), 'e': torch.gather(diff.abs(), 1, order), 'sgn': torch.gather(torch.sign(diff), 1, order)}


def lovasz64(probas, labels, ignore, g=1.0, depth=None):
    """reference, bounds and the tie structure of one Lovasz input (a dict; [P, C] tensors in the layout of ``probas``)"""
    s = _lovasz_sorted(probas, labels, ignore)
    P, C, live = s['P'], s['C'], s['live']
    fgs = s['fg'].double()
    cs = fgs.cumsum(1)
    gts = cs[:, -1:]
    rank = torch.arange(P, dtype=torch.float64)[None, :].expand(C, P)
    a, b = gts - cs, gts + (rank + 1) - cs
    jac = 1.0 - a / b
    grad = jac - torch.cat([jac.new_zeros(C, 1), jac[:, :-1]], 1)
    J = U32 * (1 + U32)
    eg = torch.where(rank == 0, torch.full_like(grad, J), 2 * J + U32 * (grad.abs() + 2 * J))                      # L2
    present = (gts > 0).double()
    npres = max(float(present.sum()), 1.0)
    gv = f32(g)
    e = s['e'] * live
    D = lovasz_depth(P, C) if depth is None else depth
    loss = float((present * e * grad).sum() / npres)
    b_loss = float((present * (e * eg + g_(D) * e * (grad.abs() + eg))).sum() / npres)                             # L3
    moves = live & (s['sgn'] != 0) & (present > 0)
    k = abs(gv) / npres
    d_sorted = torch.where(moves, -s['sgn'] * grad * (gv / npres), torch.zeros_like(grad))
    b_sorted = torch.where(moves, k * (eg + g_(3) * (grad.abs() + eg)), torch.zeros_like(grad))                    # L4
    # L5: runs of bit-equal e32 among the live entries of a class
    e32 = s['e32']
    start = torch.ones(C, P, dtype=torch.bool)
    start[:, 1:] = (e32[:, 1:] != e32[:, :-1]) | ~live[:, 1:]
    gid = (start.reshape(-1).long().cumsum(0) - 1).view(C, P)
    ng = int(gid.max()) + 1
    size = torch.bincount(gid.reshape(-1), minlength=ng).double()
    nf = torch.bincount(gid.reshape(-1), weights=fgs.reshape(-1), minlength=ng)
    i0 = torch.cummax(torch.where(start, rank, torch.zeros_like(rank)), 1)[0]
    k0 = torch.gather(cs - fgs, 1, i0.long())
    size_e, nf_e = size[gid], nf[gid]
    nb_e = size_e - nf_e
    und = live & (e32 > 0) & (size_e >= 2) & (nb_e > 0) & (gts - k0 > 0) & (present > 0)
    m0 = i0 - k0
    one = torch.ones_like(grad)
    lo_f, hi_f = 1.0 / (gts + m0 + nb_e).clamp(min=1.0), 1.0 / (gts + m0).clamp(min=1.0)
    hi_b = (gts - k0) / ((gts + m0 + 1) * (gts + m0).clamp(min=1.0))
    lo_b = (gts - k0 - nf_e).clamp(min=0.0) / ((gts + m0 + nb_e) * (gts + m0 + nb_e - 1).clamp(min=1.0)).clamp(min=1.0)
    lo = torch.where(s['fg'], lo_f, lo_b) * k
    hi = torch.where(s['fg'], hi_f, hi_b) * k
    b_env = k * (2 * J + U32 * (hi / max(k, 1e-300) + 2 * J) + g_(3) * (hi / max(k, 1e-300) + 3 * J)) * one
    # run sums (every run of live entries with e > 0 of a present class, undecided or not)
    flip = torch.where(moves, -s['sgn'] * (1.0 if gv >= 0 else -1.0), torch.zeros_like(grad))     # flip * d = |d| of the reference
    in_run = moves
    out = {'P': P, 'C': C, 'loss': loss, 'b_loss': b_loss, 'npresent': npres, 'order': s['order'], 'gid': gid, 'ngroups': ng,
           'in_run': in_run, 'flip': flip, 'share': float(und.double().mean()) if und.numel() else 0.0}
    out['run_ref'] = torch.bincount(gid.reshape(-1), weights=(flip * d_sorted * in_run).reshape(-1), minlength=ng)
    out['run_bound'] = torch.bincount(gid.reshape(-1), weights=(b_sorted * in_run).reshape(-1), minlength=ng)
    for name, t in (('d', d_sorted), ('b_d', b_sorted), ('lo', lo), ('hi', hi), ('b_env', b_env)):
        out[name] = _unsort(t, s['order'])
    out['und'] = _unsort(und, s['order'])
    out['flip_pc'] = _unsort(flip, s['order'])
    return out


def _unsort(t_sorted, order):
    """[C, P] in sorted order -> [P, C] in the layout of the input"""
    out = torch.empty_like(t_sorted)
    out.scatter_(1, order, t_sorted)
    return out.t().contiguous()


def _ratio(err, bound):
    """err / bound per element; a zero bound asks for equality; nan counts as outside"""
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, float('inf'), 0.0).to(err.dtype))
    return torch.where(torch.isnan(r), torch.full_like(r, float('inf')), r)


def _scalar(got, ref, bound):
    got = float(got)
    if math.isnan(ref):
        return (math.isnan(got), 0.0 if math.isnan(got) else float('inf'))
    err = abs(got - ref)
    if math.isnan(err):
        return (False, float('inf'))
    over = err / bound if bound > 0 else (0.0 if err == 0 else float('inf'))
    return (over <= 1.0, over)


def _tensor(got, ref, bound, mask=None):
    r = _ratio((got.double() - ref).abs(), bound)
    if mask is not None:
        r = r[mask]
    over = float(r.max()) if r.numel() else 0.0
    return (over <= 1.0, over)


def check_lovasz(ref, loss, d):
    """{output: (passes, largest error / bound)}: the loss, every decided entry of the gradient, the undecided entries against
    their envelope, every run's sum"""
    out = {'loss': _scalar(loss, ref['loss'], ref['b_loss']), 'd': _tensor(d, ref['d'], ref['b_d'], ~ref['und'])}
    v = ref['flip_pc'] * d.double()
    outside = torch.maximum(ref['lo'] - v, v - ref['hi']).clamp(min=0.0)
    out['d_undecided'] = _tensor(outside, torch.zeros_like(outside), ref['b_env'], ref['und'])
    d_sorted = torch.gather(d.double().t(), 1, ref['order'])
    runs = torch.bincount(ref['gid'].reshape(-1), weights=(ref['flip'] * d_sorted * ref['in_run']).reshape(-1), minlength=ref['ngroups'])
    out['d_run_sum'] = _tensor(runs, ref['run_ref'], ref['run_bound'])
    return out


# ---- cross entropy ------------------------------------------------------------------------------------------------------------

def _lse64(x):
    """C1 for the rows of x (fp32 values): (lse, its bound Ese) in float64"""
    xd = x.double()
    C = xd.shape[1]
    m = xd.max(1, keepdim=True)[0]
    d = xd - m
    ex = torch.exp(d)
    ee = ex * (torch.expm1(U32 * d.abs()) + 2 * U32 * EXPF_ULP) + TINY
    s = ex.sum(1, keepdim=True)
    ds = ee.sum(1, keepdim=True) + g_(C - 1) * (s + ee.sum(1, keepdim=True))
    r = ds / s
    rr = r / (1 - r)
    el = rr + 2 * U32 * LOGF_ULP * (torch.log(s).abs() + rr)
    lse = m + torch.log(s)
    return lse, el + U32 * (lse.abs() + el)


def ce64(x, labels, ignore, g=1.0):
    xd = x.double()
    P, C = xd.shape
    valid = (labels != ignore) & (labels >= 0) & (labels < C)
    count = float(valid.sum())
    gv = f32(g)
    lse, ese = _lse64(x)
    onehot = torch.zeros_like(xd)
    onehot[valid, labels[valid]] = 1.0
    xl = (xd * onehot).sum(1, keepdim=True)
    row = (lse - xl) * valid[:, None]
    er = (ese + U32 * ((lse - xl).abs() + ese)) * valid[:, None]
    if count == 0:
        return {'loss': float('nan'), 'b_loss': 0.0, 'dx': torch.zeros_like(xd), 'b_dx': torch.zeros_like(xd)}
    loss = float(row.sum() / count)
    B = float((er.sum() + g_(8) * (row.abs() + er).sum()) / count)
    p = torch.exp(xd - lse)
    ep = p * (torch.expm1(ese + U32 * (xd - lse).abs()) + 2 * U32 * EXPF_ULP) + TINY
    k = abs(gv) / count
    dx = torch.where(valid[:, None], (gv / count) * (p - onehot), torch.zeros_like(xd))
    b_dx = torch.where(valid[:, None], k * (ep + g_(4) * ((p - onehot).abs() + ep)), torch.zeros_like(xd))
    return {'loss': loss, 'b_loss': B + U32 * (abs(loss) + B), 'dx': dx, 'b_dx': b_dx}


def check_ce(ref, loss, dx):
    return {'loss': _scalar(loss, ref['loss'], ref['b_loss']), 'dx': _tensor(dx, ref['dx'], ref['b_dx'])}


# ---- KL -----------------------------------------------------------------------------------------------------------------------

def kl64(s, t, index, g=1.0):
    sd = s.double()
    P, C = sd.shape
    tr = t if index is None else t.index_select(0, index)
    td = tr.double()
    gv = f32(g)
    ls, es = _lse64(s)
    lt, et = _lse64(tr)
    lpt = td - lt
    elp = et + U32 * (lpt.abs() + et)
    pt = torch.exp(lpt)
    ept = pt * (torch.expm1(elp) + 2 * U32 * EXPF_ULP) + TINY
    esp = ept.sum(1, keepdim=True) + g_(C - 1) * (pt + ept).sum(1, keepdim=True)
    a = sd - ls
    ea = es + U32 * (a.abs() + es)
    b = lpt - a
    eb = elp + ea + U32 * (b.abs() + elp + ea)
    term = torch.where(pt > 0, pt * b, torch.zeros_like(pt))
    eterm = ept * (b.abs() + eb) + pt * eb + U32 * (pt + ept) * (b.abs() + eb)
    loss = float(term.sum() / P)
    B = float((eterm.sum() + g_(C + 8) * (term.abs() + eterm).sum()) / P)
    ps = torch.exp(a)
    eps_ = ps * (torch.expm1(ea) + 2 * U32 * EXPF_ULP) + TINY
    epr = eps_ * (1 + esp) + ps * esp + U32 * (ps + eps_) * (1 + esp)
    k = abs(gv) / P
    return {'loss': loss, 'b_loss': B + 2 * U32 * (abs(loss) + B), 'ds': (gv / P) * (ps - pt),
            'b_ds': k * (epr + ept + g_(4) * ((ps - pt).abs() + epr + ept))}


def check_kl(ref, loss, ds):
    return {'loss': _scalar(loss, ref['loss'], ref['b_loss']), 'ds': _tensor(ds, ref['ds'], ref['b_ds'])}


# ---- fp32 evaluations in the kernels' order: the honest one, and the wrong ones as switches of it --------------------------------

def _f(v):
    return torch.tensor(v, dtype=torch.float32)


def _tree256(terms):
    """[R, n] fp32 -> [R, nblk]: the 256-thread LDS tree of lovasz_terms_kernel per workgroup"""
    R, n = terms.shape
    nblk = -(-n // LV_THREADS)
    red = torch.zeros(R, nblk * LV_THREADS, dtype=torch.float32)
    red[:, :n] = terms
    red = red.view(R, nblk, LV_THREADS).clone()
    st = LV_THREADS // 2
    while st > 0:
        red[:, :, :st] = red[:, :, :st] + red[:, :, st:2 * st]
        st //= 2
    return red[:, :, 0]


def lovasz_fp32(probas, labels, ignore, g=1.0, wrong=None, reverse_ties=False):
    """(loss, d [P, C]) in fp32, the kernels' order; ``wrong`` switches one of the wrong formulations on; ``reverse_ties`` orders
    the entries of equal error the other way round (the sort's freedom of L5)"""
    if reverse_ties:
        loss, d = lovasz_fp32(probas.flip(0), labels.flip(0), ignore, g, wrong)
        return loss, d.flip(0)
    p32 = probas.float()
    P, C = p32.shape
    valid = labels != ignore
    cls = torch.arange(C)[:, None]
    fg = (labels[None, :] == cls) & valid[None, :]
    diff = fg.float() - p32.t()
    e = diff.abs()
    if wrong == 'ascending sort':
        order = torch.sort(torch.where(valid[None, :], e, torch.full_like(e, float('inf'))), dim=1, stable=True)[1]
    else:
        order = torch.sort(torch.where(valid[None, :], e, torch.full_like(e, -1.0)), dim=1, descending=True, stable=True)[1]
    es = torch.gather(torch.where(valid[None, :], e, torch.full_like(e, -1.0)), 1, order)
    fgs = torch.gather(fg, 1, order)
    csi = fgs.long().cumsum(1)
    gts, cs, fgf = csi[:, -1:].float(), csi.float(), fgs.float()
    i1 = torch.arange(1, P + 1, dtype=torch.float32)[None, :]
    off = 1.0 if wrong == 'union with i for i + 1' else 0.0
    one = _f(1.0)
    jac = one - (gts - cs) / (gts + ((i1 - off) - cs))
    cs1 = cs - fgf
    prev = one - (gts - cs1) / (gts + ((i1 - 1.0 - off) - cs1))
    grad = torch.cat([jac[:, :1], (jac - prev)[:, 1:]], 1)
    if wrong == 'grad(0) = 0':
        grad[:, 0] = 0.0
    term = es.clamp(min=0.0) * grad
    part = _tree256(term)
    tsum = torch.zeros(C, dtype=torch.float32)
    for bi in range(part.shape[1]):
        tsum = tsum + part[:, bi]
    if wrong == 'presence counted over the ignored rows':
        pr = ((labels[None, :] == cls).sum(1) > 0).float()
    else:
        pr = (csi[:, -1] > 0).float()
    lane_l, lane_n = torch.zeros(FIN_LANES), torch.zeros(FIN_LANES)
    for c0 in range(0, C, FIN_LANES):
        w = min(FIN_LANES, C - c0)
        lane_l[:w] = lane_l[:w] + tsum[c0:c0 + w] * pr[c0:c0 + w]
        lane_n[:w] = lane_n[:w] + pr[c0:c0 + w]
    l, n = _f(0.0), _f(0.0)
    for k in range(FIN_LANES):
        l, n = l + lane_l[k], n + lane_n[k]
    inv = one / (_f(float(C)) if wrong == 'mean over C' else torch.clamp(n, min=1.0))
    loss = l * inv
    gv = _f(1.0 if wrong == 'g_out ignored' else g)
    sgn = torch.sign(torch.gather(diff, 1, order))
    d_sorted = torch.where(torch.gather(valid[None, :].expand(C, P), 1, order), -sgn * grad * ((gv * inv) * pr[:, None]),
                           torch.zeros_like(grad))
    return loss, _unsort(d_sorted, order)


def _rows_lse_fp32(x, no_max=False):
    """m + logf(sum expf(x - m)), the C terms added one after the other"""
    m = torch.zeros(x.shape[0]) if no_max else x.max(1)[0]
    s = torch.zeros(x.shape[0])
    for c in range(x.shape[1]):
        s = s + torch.exp(x[:, c] - m)
    return m + torch.log(s)


def _block_partials_fp32(rows):
    """[P] fp32 -> per workgroup of 256 rows: the wave-64 butterfly, then (w0 + w1) + (w2 + w3)"""
    P = rows.shape[0]
    nblk = -(-P // CE_THREADS)
    v = torch.zeros(nblk * CE_THREADS)
    v[:P] = rows
    v = v.view(nblk, CE_THREADS // 64, 64)
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ off]
    w = v[:, :, 0]
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def _finish_double(partials):
    """ce_finish_kernel / kl_finish_kernel: lane i mod 256 adds its partials in double, then a 256-wide tree in double"""
    n = partials.shape[0]
    k = -(-n // 256)
    v = torch.zeros(k * 256, dtype=torch.float64)
    v[:n] = partials.double()
    v = v.view(k, 256)
    acc = torch.zeros(256, dtype=torch.float64)
    for i in range(k):
        acc = acc + v[i]
    st = 128
    while st >= 1:
        acc[:st] = acc[:st] + acc[st:2 * st]
        st //= 2
    return acc[0]


def ce_fp32(x, labels, ignore, g=1.0, wrong=None):
    x = x.float()
    P, C = x.shape
    valid = (labels != ignore) & (labels >= 0) & (labels < C)
    lse = _rows_lse_fp32(x, no_max=wrong == 'lse without the max subtraction')
    safe = labels.clamp(0, C - 1)
    row = torch.where(valid, lse - x[torch.arange(P), safe], torch.zeros(P))
    sl, sc = _finish_double(_block_partials_fp32(row)), _finish_double(_block_partials_fp32(valid.float()))
    if wrong == 'mean over all P rows':
        sc = torch.tensor(float(P), dtype=torch.float64)
    loss = (sl / sc).float()
    inv = (1.0 / sc).float() if float(sc) > 0 else _f(0.0)
    onehot = torch.zeros_like(x)
    onehot[torch.arange(P), safe] = 1.0
    if wrong == 'gradient without the -onehot':
        onehot = torch.zeros_like(x)
    dx = torch.where(valid[:, None], (_f(g) * inv) * (torch.exp(x - lse[:, None]) - onehot), torch.zeros_like(x))
    return loss, dx


def kl_fp32(s, t, index, g=1.0, wrong=None):
    s, t = s.float(), t.float()
    P, C = s.shape
    tr = t[:P] if (index is None or wrong == "the teacher's rows not re-indexed") else t.index_select(0, index)
    ls, lt = _rows_lse_fp32(s), _rows_lse_fp32(tr)
    sp, loss = torch.zeros(P), torch.zeros(P)
    for c in range(C):
        lpt = tr[:, c] - lt
        pt = torch.exp(lpt)
        sp = sp + pt
        if wrong == 'no guard for p_t = 0':
            loss = loss + pt * (torch.log(pt) - (s[:, c] - ls))
        else:
            loss = loss + torch.where(pt > 0, pt * (lpt - (s[:, c] - ls)), torch.zeros(P))
    inv_rows = _f(1.0) / _f(float(P * C if wrong == 'divided by P C' else P))
    total = (_finish_double(_block_partials_fp32(loss)) * inv_rows.double()).float()
    pt = torch.exp(tr - lt[:, None])
    ds = (_f(g) * inv_rows) * (torch.exp(s - ls[:, None]) * sp[:, None] - pt)
    return total, ds


# the formulations the bound has to reject: name -> (kernel, the case it is shown on, the outputs it has to break)
WRONG = {
    'union with i for i + 1': ('lovasz', 'lv-1500x17-i255-lastabsent-g65536', ('loss', 'd')),
    'grad(0) = 0': ('lovasz', 'lv-1500x17-i255-lastabsent-g65536', ('loss', 'd')),
    'mean over C': ('lovasz', 'lv-1500x17-i255-lastabsent-g65536', ('loss', 'd')),
    'presence counted over the ignored rows': ('lovasz', 'lv-255x17-i0', ('loss', 'd')),
    'g_out ignored': ('lovasz', 'lv-1500x17-i255-lastabsent-g65536', ('d',)),
    'ascending sort': ('lovasz', 'lv-1500x17-i255-lastabsent-g65536', ('loss', 'd')),
    'mean over all P rows': ('ce', 'ce-1500x17-i255', ('loss', 'dx')),
    'lse without the max subtraction': ('ce', 'ce-513x17-1e4', ('loss', 'dx')),
    'gradient without the -onehot': ('ce', 'ce-1500x17-i255', ('dx',)),
    'divided by P C': ('kl', 'kl-1500x17-perm', ('loss', 'ds')),
    "the teacher's rows not re-indexed": ('kl', 'kl-1500x17-perm', ('loss', 'ds')),
    'no guard for p_t = 0': ('kl', 'kl-257x17-peak80-longer', ('loss',)),
}


def honest_fp32(case, wrong=None, reverse_ties=False):
    """{output: value} of one case, evaluated in fp32 on the CPU in the kernels' order"""
    k = case['kernel']
    if k == 'lovasz':
        loss, d = lovasz_fp32(case['probas'], case['labels'], case['ignore'], case['g'], wrong, reverse_ties)
        return {'loss': loss, 'd': d}
    if k == 'ce':
        loss, dx = ce_fp32(case['x'], case['labels'], case['ignore'], case['g'], wrong)
        return {'loss': loss, 'dx': dx}
    loss, ds = kl_fp32(case['s'], case['t'], case['index'], case['g'], wrong)
    return {'loss': loss, 'ds': ds}


def evaluate64(case):
    k = case['kernel']
    if k == 'lovasz':
        return lovasz64(case['probas'], case['labels'], case['ignore'], case['g'])
    if k == 'ce':
        return ce64(case['x'], case['labels'], case['ignore'], case['g'])
    return kl64(case['s'], case['t'], case['index'], case['g'])


def check(case, ref, got):
    """{output: (passes, largest error / bound)} of the outputs of one case"""
    k = case['kernel']
    if k == 'lovasz':
        return check_lovasz(ref, got['loss'], got['d'])
    if k == 'ce':
        return check_ce(ref, got['loss'], got['dx'])
    return check_kl(ref, got['loss'], got['ds'])


# ---- the input sets (shared by the host test and the GPU test) ----------------------------------------------------------------
# name -> spec.  Lovasz / CE: P, C, ignore, logits kind, label pattern, share of ignored rows, g.  KL: P, C, T (teacher rows),
# index kind, logits kind, g.  'wide': the input is a column slice of a tensor of C + 3 columns (non-contiguous).
def _lv(P, C, ignore, kind='randn2', pattern='uniform', ignored=0.2, g=1.0, wide=False):
    return dict(kernel='lovasz', P=P, C=C, ignore=ignore, kind=kind, pattern=pattern, ignored=ignored, g=g, wide=wide)


def _ce(P, C, ignore, kind='randn2', pattern='uniform', ignored=0.2, g=1.0, wide=False):
    return dict(kernel='ce', P=P, C=C, ignore=ignore, kind=kind, pattern=pattern, ignored=ignored, g=g, wide=wide)


def _kl(P, C, T, index, kind='randn2', g=1.0, wide=False, peak=False):
    return dict(kernel='kl', P=P, C=C, T=T, index=index, kind=kind, g=g, wide=wide, peak=peak)


SPECS = {
    # Lovasz: rows at both sides of a workgroup of 256, classes into the second and third trip of the finish loop
    'lv-1x5-i0': _lv(1, 5, 0, ignored=0.0),
    'lv-2x2-i255-g-0.37': _lv(2, 2, 255, ignored=0.0, g=-0.37),
    'lv-255x17-i0': _lv(255, 17, 0),
    'lv-256x5-i255-g65536': _lv(256, 5, 255, g=65536.0),
    'lv-257x17-i-100-onefg-g-0.37': _lv(257, 17, -100, pattern='onefg', g=-0.37),
    'lv-512x65-i255': _lv(512, 65, 255),
    'lv-513x17-i255-oneclass': _lv(513, 17, 255, pattern='oneclass'),
    'lv-512x17-i0-ignored95': _lv(512, 17, 0, ignored=0.95),
    'lv-257x5-i-100-allbutone': _lv(257, 5, -100, pattern='allbutone'),
    'lv-256x17-i255-allignored': _lv(256, 17, 255, pattern='allignored'),
    'lv-255x130-i0-noneignored': _lv(255, 130, 0, ignored=0.0),
    'lv-1500x17-i255-lastabsent-g65536': _lv(1500, 17, 255, pattern='lastabsent', g=65536.0),
    'lv-1500x130-i-100': _lv(1500, 130, -100),
    'lv-1500x2-i255-g-0.37': _lv(1500, 2, 255, g=-0.37),
    'lv-513x17-i255-wide': _lv(513, 17, 255, wide=True),
    'lv-513x5-i0-saturated': _lv(513, 5, 0, kind='randn30'),
    'lv-512x2-i255-tied': _lv(512, 2, 255, kind='tied', ignored=0.0),
    # cross entropy
    'ce-1x17-i0': _ce(1, 17, 0, ignored=0.0),
    'ce-2x2-i255-g-0.37': _ce(2, 2, 255, ignored=0.0, g=-0.37),
    'ce-255x33-i0': _ce(255, 33, 0),
    'ce-256x17-i-100-g65536': _ce(256, 17, -100, g=65536.0),
    'ce-257x2-i255': _ce(257, 2, 255),
    'ce-512x17-i0-ignored95': _ce(512, 17, 0, ignored=0.95),
    'ce-513x17-1e4': _ce(513, 17, 255, kind='1e4'),
    'ce-513x33-i255-saturated': _ce(513, 33, 255, kind='randn30'),
    'ce-1500x17-i255': _ce(1500, 17, 255, g=-0.37),
    'ce-257x17-i-100-allbutone': _ce(257, 17, -100, pattern='allbutone'),
    'ce-256x17-i255-allignored': _ce(256, 17, 255, pattern='allignored'),
    'ce-513x17-i255-wide': _ce(513, 17, 255, wide=True),
    'ce-66000x17-i255': _ce(66000, 17, 255),
    # KL
    'kl-1x2-none': _kl(1, 2, 1, 'none'),
    'kl-2x17-none-g-0.37': _kl(2, 17, 2, 'none', g=-0.37),
    'kl-255x33-none': _kl(255, 33, 255, 'none'),
    'kl-256x17-perm-g65536': _kl(256, 17, 256, 'perm', g=65536.0),
    'kl-257x17-peak80-longer': _kl(257, 17, 300, 'random', peak=True),
    'kl-512x2-repeats-shorter': _kl(512, 2, 100, 'random'),
    'kl-513x17-1e4-none': _kl(513, 17, 513, 'none', kind='1e4'),
    'kl-513x33-saturated-longer': _kl(513, 33, 600, 'random', kind='randn30'),
    'kl-1500x17-perm': _kl(1500, 17, 1500, 'perm', g=-0.37),
    'kl-513x17-wide-repeats-shorter': _kl(513, 17, 64, 'random', wide=True),
    'kl-66000x17-longer': _kl(66000, 17, 66013, 'random'),
}
CASES = list(SPECS)
# the cases built to tie, with the share of undecided entries they have (measured on the CPU; every other case stays at or below
# UNDECIDED_CAP): the per-entry check is the envelope there, the run sums and the loss carry the test
TIE_CASES = {'lv-513x5-i0-saturated': 0.154, 'lv-512x2-i255-tied': 0.25}


def _logits(kind, n, c, gen):
    x = torch.randn(n, c, generator=gen)
    if kind == 'randn2':
        return x * 2
    if kind == 'randn30':
        return x * 30
    if kind == '1e4':
        return x + 1e4
    raise ValueError(kind)


def _labels(spec, gen):
    P, C, ignore = spec['P'], spec['C'], spec['ignore']
    lo = 1 if ignore == 0 else 0                       # with ignore_index 0 the class 0 is the ignored one
    y = torch.randint(lo, C, (P,), generator=gen)
    pattern = spec['pattern']
    if pattern == 'onefg':                             # class 3 has exactly one foreground point
        y[y == 3] = 4
        y[P // 2] = 3
    elif pattern == 'oneclass':                        # all valid points in one class
        y[:] = C - 2
    elif pattern == 'lastabsent':
        y[y == C - 1] = lo
    drop = torch.rand(P, generator=gen) < spec['ignored']
    if pattern == 'allbutone':
        drop[:] = True
        drop[P // 3] = False
    elif pattern == 'allignored':
        drop[:] = True
    elif pattern == 'onefg':
        drop[P // 2] = False
    y[drop] = ignore
    return y


def make_case(name):
    """CPU tensors of one case, the same on every machine"""
    spec = SPECS[name]
    gen = torch.Generator().manual_seed(7919 * CASES.index(name) + 13)
    k, P, C = spec['kernel'], spec['P'], spec['C']
    case = {'name': name, 'kernel': k, 'g': spec['g'], 'wide': spec['wide']}
    if k in ('lovasz', 'ce'):
        if spec['kind'] == 'tied':                     # C = 2, a quarter of the rows with equal logits (p = 0.5 for both) and mixed labels
            x = torch.randn(P, C, generator=gen) * 2
            x[::4, 1] = x[::4, 0]
        else:
            x = _logits(spec['kind'], P, C, gen)
        case.update(labels=_labels(spec, gen), ignore=spec['ignore'])
        if k == 'lovasz':
            case['probas'] = torch.softmax(x, 1)
        else:
            case['x'] = x
    else:
        T = spec['T']
        case['s'] = _logits(spec['kind'], P, C, gen)
        case['t'] = _logits(spec['kind'], T, C, gen)
        if spec['peak']:
            # a logit 80 above the rest (the other probabilities near fp32's smallest normal), and 120 above (they are exactly 0)
            case['t'][:, 0] = case['t'][:, 0] + 80.0 * (torch.arange(T) % 3 == 0) + 120.0 * (torch.arange(T) % 3 == 1)
        case['index'] = {'none': None, 'perm': torch.randperm(T, generator=gen)[:P],
                         'random': torch.randint(0, T, (P,), generator=gen)}[spec['index']]
    return case
