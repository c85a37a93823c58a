"""float64 reference of the row BatchNorm kernels (csrc/bn.hip: u2mkd_bn_train_forward, u2mkd_bn_eval_forward, u2mkd_bn_backward,
u2mkd_bn_train_forward_from_partial and the SyncBatchNorm pieces), and the elementwise bound the kernels are held to (test
helper; plain torch, CPU or GPU tensors).

WHAT IS COMPUTED.  Rows ``x [n, c]`` of the row type T (fp32, bf16, fp16), ``gamma``, ``beta`` fp32 [c] (None: 1 / 0), an optional
residual ``res [n, c]`` of the row type, per CHANNEL and on the STORED values,

    mu = mean_n(x)   M2 = sum_n (x - mu)^2   var = M2 / n   unbiased = M2 / (n - 1)   r = 1 / sqrt(var + eps)
    xhat = (x - mu) r   pre = xhat gamma + beta [+ res]   y = pre or max(pre, 0)
    running' = (1 - momentum) running + momentum (mu | unbiased)                       (momentum: the fp32 value that is passed)
    dy' = dy where pre > 0 (ReLU form), else dy      dres = dy'      dbeta = sum_n dy'      dgamma = sum_n dy' xhat
    dx = gamma r (dy' - dbeta / n - xhat dgamma / n)      eval form (mu, var given): dx = dy' gamma r

``forward64`` / ``backward64`` / ``running64`` evaluate this in float64; ``ranks64`` does so over the concatenation of several
ranks' rows (SyncBatchNorm).

THE BOUND is that of an evaluation in fp32 arithmetic throughout, in the order of operations written down below: slab sums, Chan's
update over the slabs, the file's formulas.  The kernels carry every sum over rows and the arithmetic between a load and a store
in double and round once (csrc/bn.hip, ARITHMETIC), and merge the slabs around a pivot without a division, which makes every
term below smaller and none larger; the bound is kept at the fp32 sequence so that an honest fp32 evaluation
(``slab_chan_fp32``) is inside it as well, and a rewrite of the statistics pass in fp32 is held to it.  u = 2^-24 is fp32's unit roundoff, g(k) = k u / (1 - k u)
bounds k roundings in a row, uT is the row type's unit roundoff (0 for fp32 rows, whose last rounding is an fp32 one and is counted
there; 2^-8 for bf16, 2^-11 for fp16).  Every term is u times a magnitude THAT IS ACTUALLY SUMMED, to first order in u with the
second-order parts kept where they are cheap to keep.  No constant is fitted to a measured error.

 The kernels' shape (``row_lanes``, ``register_form``, ``thread_rows``, ``num_slabs``).  A workgroup of 256 threads owns a slab of
 128 rows: c / 4 float4 columns x rl = 256 // (c / 4) row lanes (1 for c = 1024).  A thread adds its ceil(rows / rl) rows one after
 the other (at most 16 in the register form, c <= 128), the rl lanes' sums are then added one after the other out of LDS, of
 which at most ``rows`` are not zero.  An addition to the initial zero, or of a zero, is exact: no value passes through more
 than Ds = ceil(rows / rl) - 1 + min(rl, rows) - 1 additions that round (``slab_depth``; rows = 128 but for the last slab).

 1  a slab's mean, sum * fl(1 / n_b), two more roundings unless n_b is a power of two (the reciprocal and the product are then
    exact):  e_b = g(Ds + 2 | 0) mean_b|x|.
 2  a slab's centred second moment around the COMPUTED mean: sum_b (x - m_b^)^2 = M2_b + n_b (m_b^ - m_b)^2, every term carries
    the rounding of the difference twice and that of the square, the sum Ds more:  q_b = n_b e_b^2 + g(Ds + 3)(M2_b + n_b e_b^2).
 3  Chan's update over the slabs: lane l of 64 takes slabs l, l + 64, ... one after the other (ceil(nslab / 64) - 1 updates; an
    update into an empty accumulator is exact), the 64 lanes are merged by a 6-level tree: Dm = min(nslab - 1,
    ceil(nslab / 64) + 5) updates on any path (``merge_depth``).  One update, mean' = mean + (m_b - mean) (n_b / tot), rounds the
    difference, the quotient, the product and the sum: 3 u |m_b - mean| + u |mean'|, and passes the errors of its operands on
    with weights n_a / tot and n_b / tot that add up to 1.  Every partial mean lies between the smallest and the largest slab
    mean, so with A = max_b |m_b| + max_b e_b and S = max_b m_b - min_b m_b + 2 max_b e_b
        E = max_b e_b + Dm u (A + 3 S)                         bounds the error of EVERY partial mean, the final one included.
    The second moment is M2 = sum_b M2_b + sum_updates d^2 n_a n_b / tot for any order of updates (d: the difference of the two
    exact partial means; the second sum is the between-slab moment B = sum_b n_b (m_b - mu)^2).  A computed d is off by at most
    2 E, so the second sum is off by at most sum (4 E |d| + 4 E^2) n_a n_b / tot <= 4 E sqrt(W B) + 4 W E^2 (Cauchy-Schwarz),
    where W = sum n_a n_b / tot <= (rows that are the smaller side of an update) <= 7 n: once in a lane's chain, once per tree
    level.  All terms are positive, each passes through at most 2 additions per update and the cross term carries 6 roundings:
        dM2 = Q + g(2 Dm + 6)(M2 + Q),      Q = sum_b q_b + 4 E sqrt(7 n B) + 28 n E^2
    SyncBatchNorm's rank-order merge is the same update over the ranks' (mean, M2, count) rows with Dm = world - 1, W <= n, the
    ranks' own E and dM2 in the place of e_b and q_b (``stat_errors`` takes a list of ranks); the partials of
    u2mkd_bn_train_forward_from_partial, computed in float64 and rounded to fp32 by the test, have e_b = u |m_b|, q_b = u M2_b.
 4  var = fl(M2 / n):  dv = dM2 / n + u (var + dM2 / n);  unbiased likewise over n - 1.
    r = 1 / sqrt(v + eps): 3 u covers the three roundings and eps's own (the fp32 value of 1e-5), the change of 1 / sqrt over
    [var - dv, var + dv] is taken at the ends of the interval (var = 0 is a case):
        dr = max(r(var - dv) - r, r - r(var + dv)) + 3 u r(var - dv).       Eval form: E = 0, dr = 3 u r.
    running' = fl(fl(fl(1 - momentum) running) + fl(momentum s)), s off by ds:  momentum ds + g(3)((1 - momentum)|running| +
    momentum (|s| + ds)) + one fp32 floor.
 5  xhat in registers, fl(fl(x - m^) r^):  ed = E + u (|x - mu| + E),   eh = ed (r + dr) + |x - mu| dr + u (|x - mu| + ed)(r + dr).
 6  pre = fl(fl(xhat^ gamma) + beta) [+ res, one more rounding]:
        Ep = |gamma| eh + 2 u |gamma| (|xhat| + eh) + u |beta|  [+ u (|pre64| + Ep)]
    bound(y) = Ep + max(uT (|y64| + Ep), tinyT) + floor(y64).  ReLU is 1-Lipschitz: nothing is excluded from y.

 ``floor`` is one unit in the last place of the stored type at the largest reference magnitude of the output, which every
 evaluation that returns the type may have; tinyT = 2^-25 is half the distance of fp16's subnormals, 0 for the other types.

 THE FUSED RELU in the backward.  The kernels take the mask from fp32 arithmetic on the stored x (Ep above, of fp32 size for
 16-bit rows too).  An element is UNDECIDED when |pre64| <= Ep: it may take either branch, and its dres / dx must be inside the
 bound of one of the two.  Every decided element is held with no exclusion; dres of a decided element is dy or 0 exactly.
 U1 = sum_undecided |dy| and U2 = sum_undecided |dy| (|xhat| + eh) are added to the bounds of dbeta and dgamma and reach every dx
 through them.  Condition: at most 1 % of a case's elements are undecided (``UNDECIDED_CAP``; tests/test_host_row_bn_bound.py
 asserts it for every case of the GPU test).

 7  sums over the rows.  A channel's sum passes, per slab, through the Ds additions of a full slab (of the n rows, if fewer),
    then ceil(nslab / 64) additions in one of 64 lanes and 63 across the lanes, [world - 1 across the ranks]:
    Dn = Ds + ceil(nslab / 64) + 63 [+ world - 1] (``sum_depth``).  With |dy'| taken over every element that may be live,
        bound(dbeta)  = g(Dn) sum |dy'| + U1 + floor32(dbeta64)
        bound(dgamma) = sum |dy'| eh + g(Dn + 1) sum |dy'| (|xhat| + eh) + U2 + floor32(dgamma64)
 8  dx = fl(fl(gamma r^) fl(fl(dy' - fl(db^ i)) - fl(fl(xhat^ dg^) i))), i = fl(1 / n); s1 = dbeta / n, s2 = dgamma / n, e1, e2
    the bounds of step 7 over n:
        d1 = e1 + 2 u (|s1| + e1)        d2 = eh (|s2| + e2) + |xhat| e2 + 3 u (|xhat| + eh)(|s2| + e2)
        et = d1 + d2 + u (2 |dy'| + 2 |s1| + 2 d1 + |xhat s2| + d2)           eg = |gamma| dr + u |gamma| (r + dr)
        Edx = (|gamma| r + eg) et + eg |t64| + u (|gamma| r + eg)(|t64| + et)
    eval form, fl(fl(dy' gamma) r^):  Edx = |dy' gamma| dr + 2 u |dy' gamma| (r + dr).
    bound(dx) = Edx + max(uT (|dx64| + Edx), tinyT) + floor(dx64)

WHAT THE BOUND CAN SEE.  ``WRONG`` names the formulations it has to reject (tests/test_host_row_bn_bound.py): the variance as
E[x^2] - mean^2, one fp32 accumulator per channel over all rows, slab means merged with equal weights, statistics accumulated
in the 16-bit row type, parameter gradients summed from the unmasked dy.  ``slab_chan_fp32`` is the honest evaluation -- per-slab
mean and centred M2 in fp32, Chan's update in fp32, the file's formulas, one rounding to the row type -- that has to stay
inside on every input set of the GPU test."""
import math

import torch

U32 = 2.0 ** -24
ROW_UNIT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}       # uT (fp32: counted with u)
ULP_REL = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}   # one ulp of a value in [1, 2)
TINY = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
THREADS = 256
SLAB_ROWS = 128
REG_ROWS = 16
FIN_LANES = 64
EPS = 1e-5
MOMENTUM = 0.1
UNDECIDED_CAP = 0.01


def g_(k):
    """k roundings in a row"""
    return k * U32 / (1.0 - k * U32)


# ---- the kernels' shape, restated ---------------------------------------------------------------------------------------------

def supported(c):
    return c % 4 == 0 and 4 <= c <= 1024


def row_lanes(c):
    """rl of bn_layout / the partial kernels"""
    c4 = c // 4
    return 1 if c4 >= THREADS else THREADS // c4


def register_form(c):
    """the dispatch condition of bn_launch_stats_partial (without the U2MKD_BN_STATS_SERIAL switch)"""
    c4 = c // 4
    return c4 <= 32 and SLAB_ROWS // (THREADS // c4) <= REG_ROWS


def thread_rows(c):
    """rows one thread adds one after the other (at most REG_ROWS in the register form)"""
    return -(-SLAB_ROWS // row_lanes(c))


def num_slabs(n, slab_rows=SLAB_ROWS):
    return -(-n // slab_rows) if n > 0 else 0


def slab_depth(c, rows=SLAB_ROWS):
    """additions that round on the way of one value into the sum of a slab of ``rows`` rows (an int or a tensor of counts)"""
    rl = row_lanes(c)
    if torch.is_tensor(rows):
        return torch.ceil(rows / rl) - 1 + rows.clamp(max=rl) - 1
    return -(-rows // rl) - 1 + min(rl, rows) - 1


def merge_depth(nslab):
    return max(0, min(nslab - 1, -(-nslab // FIN_LANES) + 5))


def sum_depth(n, c, world=1):
    return slab_depth(c, min(n, SLAB_ROWS)) + -(-num_slabs(n) // FIN_LANES) + FIN_LANES - 1 + world - 1


def floor_ulp(ref, dtype):
    """one unit in the last place of ``dtype`` at the largest magnitude of ``ref`` (0 for an all-zero reference)"""
    m = float(ref.detach().abs().max()) if ref.numel() else 0.0
    if m == 0.0 or not math.isfinite(m):
        return 0.0
    return 2.0 ** math.floor(math.log2(m)) * ULP_REL[dtype]


def f32(v):
    """the fp32 value of a Python float (what a C float argument receives)"""
    return float(torch.tensor(v, dtype=torch.float32))


# ---- float64 evaluations ------------------------------------------------------------------------------------------------------

def _affine(gamma, beta, like):
    c = like.shape[-1]
    gd = gamma.double() if gamma is not None else torch.ones(c, dtype=torch.float64, device=like.device)
    bd = beta.double() if beta is not None else torch.zeros(c, dtype=torch.float64, device=like.device)
    return gd, bd


def forward64(x, gamma, beta, eps=EPS, res=None, relu=False, stats=None):
    """train form, or the eval form on ``stats`` = (running_mean, running_var)"""
    xd = x.double()
    n = xd.shape[0]
    gd, bd = _affine(gamma, beta, xd)
    if stats is None:
        mu = xd.mean(0)
        dev = xd - mu
        m2 = (dev * dev).sum(0)
        var = m2 / n
        unbiased = m2 / (n - 1) if n > 1 else var
    else:
        mu, var = stats[0].double(), stats[1].double()
        dev = xd - mu
        m2, unbiased = var * n, var
    r = 1.0 / torch.sqrt(var + eps)
    xhat = dev * r
    pre = xhat * gd + bd
    if res is not None:
        pre = pre + res.double()
    return {'mu': mu, 'var': var, 'unbiased': unbiased, 'M2': m2, 'r': r, 'dev': dev, 'xhat': xhat, 'pre': pre,
            'y': pre.clamp(min=0.0) if relu else pre, 'n': n, 'training': stats is None, 'relu': bool(relu)}


def running64(running_mean, running_var, f, momentum=MOMENTUM):
    """the momentum update; ``momentum`` is taken at its fp32 value, as the entry receives it (cumulative average: 1 / step)"""
    m = f32(momentum)
    return ((1.0 - m) * running_mean.double() + m * f['mu'], (1.0 - m) * running_var.double() + m * f['unbiased'])


def backward64(dy, f, gamma, undecided=None):
    """dx, dres, dgamma, dbeta, the masked dy' ('dym'); with ``undecided`` also the other branch of those elements
    ('dx_alt', 'dres_alt', 'dym_alt'), the sums staying those of the float64 mask"""
    dyd = dy.double()
    gd, _ = _affine(gamma, None, dyd)
    n = f['n']
    live = (f['pre'] > 0) if f['relu'] else torch.ones_like(dyd, dtype=torch.bool)
    dym = torch.where(live, dyd, torch.zeros_like(dyd))
    out = {'dym': dym, 'dres': dym, 'dbeta': dym.sum(0), 'dgamma': (dym * f['xhat']).sum(0), 'live': live}

    def dx_of(d):
        if f['training']:
            return gd * f['r'] * (d - out['dbeta'] / n - f['xhat'] * (out['dgamma'] / n))
        return d * gd * f['r']

    out['dx'] = dx_of(dym)
    if undecided is not None:
        out['dym_alt'] = torch.where(live ^ undecided, dyd, torch.zeros_like(dyd))
        out['dres_alt'] = out['dym_alt']
        out['dx_alt'] = dx_of(out['dym_alt'])
    return out


def ranks64(cases, mode, eps=EPS):
    """the ranks' rows as ONE batch: ({x, dy, res, gamma, beta} concatenated over the rows, the rank sizes)"""
    keys = ('x', 'dy') + (('res',) if mode == 'res' else ())
    cat = {k: torch.cat([cs[k] for cs in cases], 0) for k in keys}
    cat['gamma'], cat['beta'] = cases[0]['gamma'], cases[0]['beta']
    return cat, [cs['x'].shape[0] for cs in cases]


# ---- the bound ----------------------------------------------------------------------------------------------------------------

def _slab_moments(xd, slab_rows):
    """per slab: count [k], mean [k, c], centred M2 [k, c], mean |x| [k, c] in float64"""
    n, c = xd.shape
    k = num_slabs(n, slab_rows)
    pad = k * slab_rows - n
    xp = torch.cat([xd, xd.new_zeros(pad, c)], 0).reshape(k, slab_rows, c) if pad else xd.reshape(k, slab_rows, c)
    nb = torch.full((k,), float(slab_rows), dtype=torch.float64, device=xd.device)
    nb[-1] = slab_rows - pad
    valid = (torch.arange(slab_rows, device=xd.device)[None, :] < nb[:, None]).to(xd.dtype)[:, :, None]
    mean = xp.sum(1) / nb[:, None]
    dev = (xp - mean[:, None, :]) * valid
    return nb, mean, (dev * dev).sum(1), xp.abs().sum(1) / nb[:, None]


def _chan_errors(nb, mean_b, e_b, q_sum, m2_parts, depth, levels):
    """step 3: (mu, M2, E, dM2) of Chan's update over parts of ``nb`` rows with means ``mean_b`` known to ``e_b``"""
    u = U32
    n = nb.sum()
    mu = (nb[:, None] * mean_b).sum(0) / n
    between = (nb[:, None] * (mean_b - mu) ** 2).sum(0)
    emax = e_b.max(0).values
    a = mean_b.abs().max(0).values + emax
    spread = mean_b.max(0).values - mean_b.min(0).values + 2 * emax
    e = emax + depth * u * (a + 3 * spread)
    m2 = m2_parts + between
    q = q_sum + 4 * e * torch.sqrt(levels * n * between) + 4 * levels * n * e * e
    return mu, m2, e, q + g_(2 * depth + 6) * (m2 + q)


def stat_errors(ranks, eps=EPS, slab_rows=SLAB_ROWS, rounded_partials=False):
    """steps 1-4 for the rows of one rank (a tensor) or of several (a list, merged in rank order; empty ranks are skipped):
    {'E', 'dM2', 'dv', 'dr', 'dunb', 'n'} next to the float64 statistics of the whole batch"""
    u = U32
    ranks = [r for r in (ranks if isinstance(ranks, (list, tuple)) else [ranks]) if r.shape[0] > 0]
    c = ranks[0].shape[1]
    per = []
    for x in ranks:
        nb, mean_b, m2_b, mabs_b = _slab_moments(x.double(), slab_rows)
        if rounded_partials:
            e_b, q_b = u * mean_b.abs(), u * m2_b
        else:
            ds = slab_depth(c, nb)
            pow2 = torch.log2(nb) == torch.floor(torch.log2(nb))
            e_b = g_(ds + torch.where(pow2, 0.0, 2.0))[:, None] * mabs_b
            q_b = nb[:, None] * e_b * e_b + g_(ds + 3)[:, None] * (m2_b + nb[:, None] * e_b * e_b)
        mu, m2, e, dm2 = _chan_errors(nb, mean_b, e_b, q_b.sum(0), m2_b.sum(0), merge_depth(len(nb)), 7)
        per.append((nb.sum(), mu, m2, e, dm2))
    if len(per) > 1:
        nr = torch.stack([p[0] for p in per])
        mu, m2, e, dm2 = _chan_errors(nr, torch.stack([p[1] for p in per]), torch.stack([p[3] for p in per]),
                                      sum(p[4] for p in per), sum(p[2] for p in per), len(per) - 1, 1)
        n = float(nr.sum())
    else:
        n, mu, m2, e, dm2 = per[0]
        n = float(n)
    var = m2 / n
    dv = dm2 / n + u * (var + dm2 / n)
    r = 1.0 / torch.sqrt(var + eps)
    r_lo = 1.0 / torch.sqrt((var - dv).clamp(min=0.0) + eps)
    r_hi = 1.0 / torch.sqrt(var + dv + eps)
    dr = torch.maximum(r_lo - r, r - r_hi) + 3 * u * r_lo
    dunb = (dm2 / (n - 1) + u * (m2 + dm2) / (n - 1)) if n > 1 else dv
    return {'E': e, 'dM2': dm2, 'dv': dv, 'dr': dr, 'dunb': dunb, 'n': n}


def eval_errors(f):
    """the eval form: the mean is an input, r^ = 1 / sqrtf(var + eps) of an input"""
    z = torch.zeros_like(f['r'])
    return {'E': z, 'dM2': z, 'dv': z, 'dr': 3 * U32 * f['r'], 'dunb': z, 'n': float(f['n'])}


def _stored(err, ref, dtype):
    """an fp32 result of error ``err`` stored in ``dtype``: + one rounding of the row type + the floor"""
    store = (ROW_UNIT[dtype] * (ref.abs() + err)).clamp(min=TINY[dtype]) if ROW_UNIT[dtype] else torch.zeros_like(err)
    return err + store + floor_ulp(ref, dtype)


def _xhat_errors(f, se):
    u = U32
    adev = f['dev'].abs()
    ed = se['E'] + u * (adev + se['E'])
    rr = f['r'] + se['dr']
    return ed * rr + adev * se['dr'] + u * (adev + ed) * rr


def forward_bound(f, se, gamma, beta, dtype, res=None, running=None, momentum=MOMENTUM):
    """{'y', 'mean', 'invstd' [, 'running_mean', 'running_var'], 'pre_err', 'undecided'} next to forward64's values ``f``;
    ``running`` = the (running_mean, running_var) BEFORE the update"""
    u = U32
    gd, bd = _affine(gamma, beta, f['pre'])
    eh = _xhat_errors(f, se)
    ep = gd.abs() * eh + 2 * u * gd.abs() * (f['xhat'].abs() + eh) + u * bd.abs()
    if res is not None:
        ep = ep + u * (f['pre'].abs() + ep)
    out = {'y': _stored(ep, f['y'], dtype), 'mean': se['E'] + floor_ulp(f['mu'], torch.float32),
           'invstd': se['dr'] + floor_ulp(f['r'], torch.float32), 'pre_err': ep, 'eh': eh,
           'undecided': (f['pre'].abs() <= ep) if f['relu'] else torch.zeros_like(f['pre'], dtype=torch.bool)}
    if running is not None:
        m = f32(momentum)
        want = running64(running[0], running[1], f, momentum)
        for name, old, s, ds, new in (('running_mean', running[0], f['mu'], se['E'], want[0]),
                                      ('running_var', running[1], f['unbiased'], se['dunb'], want[1])):
            out[name] = m * ds + g_(3) * ((1.0 - m) * old.double().abs() + m * (s.abs() + ds)) + floor_ulp(new, torch.float32)
    return out


def backward_bound(dy, f, b, fb, se, gamma, dtype, world=1, n_slab_rows=None, depth=None):
    """{'dx', 'dres', 'dgamma', 'dbeta' [, 'dx_alt', 'dres_alt']} next to backward64's values ``b`` (computed with
    ``undecided`` = fb['undecided'] in the ReLU form); fb = forward_bound's result; ``n_slab_rows``: the largest rank's rows;
    ``depth``: Dn of step 7 for kernels of another shape than the row kernels' (tests/bn2d_f64_ref.py)"""
    u = U32
    n, c = f['n'], dy.shape[1]
    gd, _ = _affine(gamma, None, f['pre'])
    ag, eh, axh, und = gd.abs(), fb['eh'], f['xhat'].abs(), fb['undecided']
    ady_all = dy.double().abs()
    ady = ady_all * (b['live'] | und)
    dn = sum_depth(n_slab_rows or n, c, world) if depth is None else depth
    u1, u2 = (ady_all * und).sum(0), (ady_all * (axh + eh) * und).sum(0)
    bdb = g_(dn) * ady.sum(0) + u1 + floor_ulp(b['dbeta'], torch.float32)
    bdg = (ady * eh).sum(0) + g_(dn + 1) * (ady * (axh + eh)).sum(0) + u2 + floor_ulp(b['dgamma'], torch.float32)
    out = {'dbeta': bdb, 'dgamma': bdg, 'dres': torch.zeros_like(ady), 'dres_alt': torch.zeros_like(ady)}
    rr = f['r'] + se['dr']

    def edx(dym, dx64):
        if not f['training']:
            return _stored((dym * gd).abs() * se['dr'] + 2 * u * (dym * gd).abs() * rr, dx64, dtype)
        s1, s2, e1, e2 = b['dbeta'] / n, b['dgamma'] / n, bdb / n, bdg / n
        d1 = e1 + 2 * u * (s1.abs() + e1)
        d2 = eh * (s2.abs() + e2) + axh * e2 + 3 * u * (axh + eh) * (s2.abs() + e2)
        t64 = dym - s1 - f['xhat'] * s2
        et = d1 + d2 + u * (2 * dym.abs() + 2 * s1.abs() + 2 * d1 + (f['xhat'] * s2).abs() + d2)
        eg = ag * se['dr'] + u * ag * rr
        gr = ag * f['r'] + eg
        return _stored(gr * et + eg * t64.abs() + u * gr * (t64.abs() + et), dx64, dtype)

    out['dx'] = edx(b['dym'], b['dx'])
    # what the undecided elements alone may move: the sums by U1 / U2, a dx through them
    und_dx = (ag * f['r'] * (u1 + axh * u2) / n) if f['training'] else torch.zeros_like(ady)
    out['allow'] = {'dbeta': float(u1.max()), 'dgamma': float(u2.max()), 'dx': float(und_dx.max()) if und_dx.numel() else 0.0}
    if 'dx_alt' in b:
        out['dx_alt'] = edx(b['dym_alt'], b['dx_alt'])
    return out


def worst(got, ref, bound, ref_alt=None, bound_alt=None, undecided=None):
    """(passes, largest |got - ref| / bound, largest |got - ref|): no element excluded; a zero bound asks for equality.  With
    ``undecided``: those elements may be inside the bound of the other branch instead (error and ratio are then the smaller)."""
    err = (got.double() - ref).abs()
    if err.numel() == 0:
        return True, 0.0, 0.0

    def ratio(e, bd):
        return torch.where(bd > 0, e / bd.clamp(min=1e-300), torch.where(e > 0, float('inf'), 0.0).to(e.dtype))

    over = ratio(err, bound)
    if undecided is not None and ref_alt is not None and bool(undecided.any()):
        err_alt = (got.double() - ref_alt).abs()
        over_alt = ratio(err_alt, bound_alt)
        take = undecided & (over_alt < over)
        over = torch.where(take, over_alt, over)
        err = torch.where(take, err_alt, err)
    return bool((over <= 1.0).all()), float(over.max()), float(err.max())


# ---- fp32 evaluations: the honest one and the wrong ones ----------------------------------------------------------------------

def _finish_fp32(case, mode, dtype, mean, m2, n, eps=EPS, momentum=MOMENTUM, unmasked_sums=False, training=True):
    """the file's forward and backward formulas in fp32 from the statistics (mean, M2), rounded once to the row type"""
    xf, dyf = case['x'].float(), case['dy'].float()
    c = xf.shape[1]
    gm = case['gamma'] if case['gamma'] is not None else torch.ones(c)
    bt = case['beta'] if case['beta'] is not None else torch.zeros(c)
    var = m2 / n
    invstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    unbiased = m2 / (n - 1) if n > 1 else var
    m = torch.tensor(momentum, dtype=torch.float32)
    xhat = (xf - mean) * invstd
    pre = xhat * gm + bt
    if mode == 'res':
        pre = pre + case['res'].float()
    relu = mode in ('relu', 'res')
    dym = torch.where(pre > 0, dyf, torch.zeros_like(dyf)) if relu else dyf
    dsum = dyf if unmasked_sums else dym
    dbeta, dgamma = dsum.sum(0), (dsum * xhat).sum(0)
    inv_n = torch.tensor(1.0, dtype=torch.float32) / n
    dx = gm * invstd * (dym - dbeta * inv_n - xhat * dgamma * inv_n) if training else dym * gm * invstd
    return {'y': (pre.clamp(min=0.0) if relu else pre).to(dtype), 'mean': mean, 'invstd': invstd,
            'running_mean': (1 - m) * case['rm'] + m * mean, 'running_var': (1 - m) * case['rv'] + m * unbiased,
            'dx': dx.to(dtype), 'dres': dym.to(dtype), 'dgamma': dgamma, 'dbeta': dbeta}


def _slab_stats_fp32(xf, slab_rows=SLAB_ROWS, acc=torch.float32):
    """per slab (count, mean, centred M2), accumulated in ``acc``"""
    out = []
    for r0 in range(0, xf.shape[0], slab_rows):
        s = xf[r0:r0 + slab_rows].to(acc)
        nb = s.shape[0]
        mean = (s.sum(0, dtype=acc) / nb).to(acc)
        dev = (s - mean).to(acc)
        out.append((float(nb), mean.float(), (dev * dev).to(acc).sum(0, dtype=acc).float()))
    return out


def _chan_merge_fp32(parts, equal_weights=False):
    na, mean, m2 = 0.0, torch.zeros_like(parts[0][1]), torch.zeros_like(parts[0][1])
    for k, (nb, mb, qb) in enumerate(parts):
        tot = na + nb
        delta = mb - mean
        w = torch.tensor(1.0 / (k + 1) if equal_weights else nb / tot, dtype=torch.float32)
        mean = mean + delta * w
        m2 = m2 + (qb + delta * delta * torch.tensor(na * nb / tot, dtype=torch.float32))
        na = tot
    return mean, m2


def slab_chan_fp32(case, mode, dtype, eps=EPS, momentum=MOMENTUM):
    """the honest evaluation: per-slab mean and centred M2 in fp32, Chan's update over the slabs in fp32"""
    xf = case['x'].float()
    mean, m2 = _chan_merge_fp32(_slab_stats_fp32(xf))
    return _finish_fp32(case, mode, dtype, mean, m2, xf.shape[0], eps, momentum)


def eval_fp32(case, mode, dtype, eps=EPS):
    """the eval form in fp32 on the case's running statistics (the running outputs it returns mean nothing)"""
    n = case['x'].shape[0]
    return _finish_fp32(case, mode, dtype, case['rm'], case['rv'] * n, n, eps, training=False)


def _wrong_e_x2(case, mode, dtype):
    xf = case['x'].float()
    n = xf.shape[0]
    mean = xf.mean(0)
    var = ((xf * xf).mean(0) - mean * mean).clamp(min=0.0)
    return _finish_fp32(case, mode, dtype, mean, var * n, n)


def _serial_sum(t, acc=torch.float32):
    """sum over the rows, ONE accumulator of type ``acc`` per channel (one rounding per addition)"""
    s = torch.zeros(t.shape[1], dtype=acc)
    for row in t.to(acc):
        s = s + row
    return s


def _wrong_one_accumulator(case, mode, dtype):
    xf = case['x'].float()
    n = xf.shape[0]
    mean = _serial_sum(xf) / n
    dev = xf - mean
    return _finish_fp32(case, mode, dtype, mean, _serial_sum(dev * dev), n)


def _wrong_equal_weights(case, mode, dtype):
    xf = case['x'].float()
    mean, m2 = _chan_merge_fp32(_slab_stats_fp32(xf), equal_weights=True)
    return _finish_fp32(case, mode, dtype, mean, m2, xf.shape[0])


def _wrong_row_type_stats(case, mode, dtype):
    x = case['x']
    n = x.shape[0]
    mean = (_serial_sum(x, dtype).float() / n).to(dtype)
    dev = (x - mean).to(dtype)
    m2 = _serial_sum((dev * dev).to(dtype), dtype).float()
    return _finish_fp32(case, mode, dtype, mean.float(), m2, n)


def _wrong_unmasked_sums(case, mode, dtype):
    xf = case['x'].float()
    mean, m2 = _chan_merge_fp32(_slab_stats_fp32(xf))
    return _finish_fp32(case, mode, dtype, mean, m2, xf.shape[0], unmasked_sums=True)


# the formulations the bound has to reject: name -> f(case, mode, dtype) -> the outputs of slab_chan_fp32
WRONG = {'variance as E[x^2] - mean^2': _wrong_e_x2,
         'one fp32 accumulator per channel': _wrong_one_accumulator,
         'slab means merged with equal weights': _wrong_equal_weights,
         'statistics accumulated in the row type': _wrong_row_type_stats,
         'parameter gradients from the unmasked dy': _wrong_unmasked_sums}


# ---- the input sets (shared by the host test and the GPU test) ----------------------------------------------------------------

PAIRS = ((2, 4), (2, 1024), (127, 12), (128, 48), (129, 48), (129, 132), (257, 128), (257, 1020), (8193, 96), (8193, 256),
         (32769, 32))
KINDS = ('randn', 'mean1e3', 'constch', 'scales')
MODES = ('plain', 'relu', 'res')
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
AFFINE_FALSE_PAIR = (129, 48)
OUTPUTS = ('y', 'mean', 'invstd', 'running_mean', 'running_var', 'dx', 'dres', 'dgamma', 'dbeta')


# (n, c, kind) -> the seed of a case whose seed-0 draw has more than UNDECIDED_CAP of its elements undecided in some mode or row type
# (2 rows of mean 1e3 that round to the same 16-bit value leave a channel of variance 0 next to a mean known to 1e3 u)
SEEDS = {(2, 4, 'mean1e3'): 1, (2, 1024, 'mean1e3'): 7, (32769, 32, 'mean1e3'): 1}


def make_case(n, c, kind, dtype, seed=None, affine=True):
    """CPU tensors of one case, the same on every machine: rows x, dy, res of ``dtype`` (rounded to it), gamma = 1 + 0.5 randn and
    beta = randn fp32 (None with affine=False), running statistics rm / rv fp32 that are not the initial 0 / 1."""
    seed = SEEDS.get((n, c, kind), 0) if seed is None else seed
    g = torch.Generator().manual_seed(100003 * seed + 131 * n + c + 7 * KINDS.index(kind))
    x = torch.randn(n, c, generator=g)
    gamma = 1.0 + 0.5 * torch.randn(c, generator=g)
    if kind == 'mean1e3':        # mean 1e3, spread 1: where E[x^2] - mean^2 and a single accumulator lose the variance
        x = x + 1e3
    elif kind == 'constch':      # every fourth channel holds one value in all rows: variance 0, invstd = 1 / sqrt(eps)
        x[:, ::4] = torch.randn(1, c, generator=g)[:, ::4]
    elif kind == 'scales':       # channel j scaled by 2^(j mod 13 - 6), gamma by its inverse: small and large channels together
        s = 2.0 ** (torch.arange(c) % 13 - 6).float()
        x, gamma = x * s, gamma / s
    elif kind != 'randn':
        raise ValueError(kind)
    x = x.to(dtype)
    rm = x.float().mean(0) + 0.1 * torch.randn(c, generator=g)
    rv = x.float().var(0, unbiased=False) * (0.5 + torch.rand(c, generator=g)) + 0.1
    return {'x': x, 'dy': torch.randn(n, c, generator=g).to(dtype), 'res': torch.randn(n, c, generator=g).to(dtype),
            'gamma': gamma if affine else None, 'beta': torch.randn(c, generator=g) if affine else None, 'rm': rm, 'rv': rv}


def cases(n, c):
    """(kind, mode, affine) of every case of the pair (n, c)"""
    out = [(kind, mode, True) for kind in KINDS for mode in MODES]
    if (n, c) == AFFINE_FALSE_PAIR:
        out += [('randn', mode, False) for mode in MODES]
    return out


def evaluate64(case, mode, dtype, training=True, eps=EPS, momentum=MOMENTUM, se=None):
    """references and bounds of one case: ({output: float64 value}, {output: bound}, the undecided mask, its share)"""
    res = case['res'] if mode == 'res' else None
    relu = mode in ('relu', 'res')
    stats = None if training else (case['rm'], case['rv'])
    f = forward64(case['x'], case['gamma'], case['beta'], eps, res, relu, stats)
    if se is None:
        se = stat_errors(case['x'], eps) if training else eval_errors(f)
    fb = forward_bound(f, se, case['gamma'], case['beta'], dtype, res, (case['rm'], case['rv']) if training else None, momentum)
    b = backward64(case['dy'], f, case['gamma'], fb['undecided'] if relu else None)
    bb = backward_bound(case['dy'], f, b, fb, se, case['gamma'], dtype)
    ref = {'y': f['y'], 'mean': f['mu'], 'invstd': f['r'], 'dx': b['dx'], 'dres': b['dres'], 'dgamma': b['dgamma'], 'dbeta': b['dbeta']}
    bound = {'y': fb['y'], 'mean': fb['mean'], 'invstd': fb['invstd'], 'dx': bb['dx'], 'dres': bb['dres'], 'dgamma': bb['dgamma'],
             'dbeta': bb['dbeta']}
    if training:
        ref['running_mean'], ref['running_var'] = running64(case['rm'], case['rv'], f, momentum)
        bound['running_mean'], bound['running_var'] = fb['running_mean'], fb['running_var']
    bound['allow'] = bb['allow']
    if relu:
        for k in ('dx', 'dres'):
            ref[k + '_alt'], bound[k + '_alt'] = b[k + '_alt'], bb[k + '_alt']
    und = fb['undecided']
    return ref, bound, und, float(und.double().mean()) if und.numel() else 0.0


def check(got, ref, bound, und, names=None):
    """{output: (passes, largest error / bound, largest error)} of the outputs ``got`` has"""
    out = {}
    for name in names or [k for k in OUTPUTS if k in got and k in ref]:
        if name in ('dx', 'dres') and name + '_alt' in ref:
            out[name] = worst(got[name], ref[name], bound[name], ref[name + '_alt'], bound[name + '_alt'], und)
        else:
            out[name] = worst(got[name], ref[name], bound[name])
    return out
