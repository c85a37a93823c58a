"""float64 reference of the row LayerNorm kernels (csrc/ln.hip: u2mkd_ln_forward, u2mkd_ln_add_forward, u2mkd_ln_backward), and
the elementwise bound the kernels are held to (test helper; plain torch, CPU or GPU tensors).

WHAT IS COMPUTED.  Rows ``x [n, c]`` of the row type T (fp32, bf16, fp16), ``gamma``, ``beta`` fp32 [c]; on the STORED values,

    mu = mean_c(x)   var = mean_c((x - mu)^2)   r = 1 / sqrt(var + eps)   xhat = (x - mu) r   y = xhat gamma + beta
    g = dy gamma     s1 = mean_c(g)   s2 = mean_c(g xhat)   dx = r (g - s1 - xhat s2) [+ ds]   [db = w_row dx]
    dgamma = sum_rows dy xhat          dbeta = sum_rows dy

``forward64`` / ``backward64`` evaluate this in float64.  In the add form x is the stored stream row ``s = round_T(a + w b)``
(``stream64``): the kernel takes its statistics from the rounded s, so nothing else changes.

THE BOUND is that of an evaluation in fp32 arithmetic throughout, in the kernels' order of operations.  The kernels carry the
arithmetic between a load and a store in double and round once (csrc/ln.hip, ARITHMETIC), which makes every term below smaller
and none larger; the bound is kept at the fp32 sequence so that a straightforward fp32 evaluation is inside it as well.
u = 2^-24 is fp32's unit roundoff, uT the row type's (0 for fp32 rows -- their last rounding is an fp32 one and is
counted there --, 2^-8 for bf16, 2^-11 for fp16).  Every term below is u times a magnitude THAT IS ACTUALLY SUMMED, read off the
kernel's operation sequence, to first order in u with the second-order parts kept where they are cheap to keep.

 Sums over the channels of a row.  A lane adds its 8 V values one after the other (8 V - 1 additions), the G lanes of the row's
 group are then added by a butterfly of log2 G steps: no value passes through more than D = 8 V - 1 + log2 G additions, so the
 computed sum of terms t_j is off by at most D u sum |t_j|.  (G, V) as the kernel picks them from c (``lane_form``).
 Times 1 / c (one rounding of the constant, one of the product): (D + 2) u mean |t_j| for a mean.

 1  the mean.  dm0 = (D + 2) u mean|x| bounds a plain fp32 mean; a mean refined once, m = m0 + mean_c(x - m0), has
    |m - mu| <= u |mu| + (D + 3) u (mean|x - mu| + dm0).  dm is the LARGER of the two.
 2  a deviation in registers, fl(x_j - m):  ed_j = dm + u (|x_j - mu| + dm).
 3  the variance, mean_c of the squared deviations from m: sum_j (x_j - m)^2 = c var + c (m - mu)^2, every square carries
    2 u (its operand) + u (the product), the sum D u, the division by c 2 u:  dv = dm^2 + (D + 5) u (var + dm^2).
 4  r = 1 / sqrt(v + eps): 3 u covers an fp32 evaluation's three roundings (eps itself is the fp32 value of 1e-5, 2^-25.3 away), and the change of 1 / sqrt over [var - dv, var + dv] taken at the ends
    of that interval (no linearisation: var = 0 is a case):  dr = max(r(var - dv) - r, r - r(var + dv)) + 3 u r(var - dv).
 5  xhat in registers, fl(fl(x_j - m) r^):  eh_j = ed_j (r + dr) + |x_j - mu| dr + u (|x_j - mu| + ed_j)(r + dr).
 6  y = fl(fl(xhat^ gamma) + beta) (a fused multiply-add has one rounding fewer):
        Ey_j = |gamma_j| eh_j + 2 u |gamma_j| (|xhat_j| + eh_j) + u |beta_j|
    bound(y) = Ey + max(uT (|y64| + Ey), tinyT) + floor(y64)

 ``floor`` is one unit in the last place of the stored type at the largest reference magnitude of the output,
 2^floor(log2 max|ref|) * 2 uT (fp32 outputs: 2 u), which every evaluation that returns the type may have.  tinyT = 2^-25 is
 half the distance of fp16's subnormals (a store below 2^-14 loses up to that whatever its size); 0 for the other types.

 Backward.  The kernel reads the forward's m and r^ (errors dm, dr) and recomputes xhat^ (error eh_j).
 7  g_j = fl(dy_j gamma_j): u |g_j|.   s1: d1 = (D + 3) u mean|g|.
    s2 = mean_c(g xhat^): d2 = mean_c(|g| eh) + (D + 4) u mean_c(|g| (|xhat| + eh)).
 8  t_j = g_j - s1 - xhat^_j s2, the three terms subtracted in fp32:
        et_j = u |g_j| + d1 + eh_j (|s2| + d2) + |xhat_j| d2                     (errors of the operands)
             + u (|g_j| + |s1| + d1) + 2 u (|xhat_j| + eh_j)(|s2| + d2) + u (|g_j| + |s1| + |xhat_j s2|)   (roundings)
 9  dx_j = fl(r^ t_j) [+ ds_j, one more fp32 rounding of the sum]:
        Edx_j = (r + dr) et_j + dr |t64_j| + u (r + dr)(|t64_j| + et_j)  [+ u (|dx64_j + ds_j| + Edx_j)]
    bound(dx) = Edx + max(uT (|dx64| + Edx), tinyT) + floor(dx64)
    db = round_T(fl(w dx^)) from the unrounded dx^:  Edb = |w| Edx + u |db64|, bound(db) as for dx.
 10 sums over the rows.  A channel's sum passes, per row slab of 128, through G / 2 additions in a lane's registers, log2(64 / G)
    butterfly steps across the lane groups of a wave and 3 additions across the waves; the slab sum kernel adds the slabs'
    partials in double and rounds once: Dn fp32 roundings at most for an fp32 evaluation of that shape (``row_depth``).
        bound(dgamma) = sum_rows |dy| eh + (Dn + 1) u sum_rows |dy| (|xhat| + eh) + floor32(dgamma64)
        bound(dbeta)  = Dn u sum_rows |dy| + floor32(dbeta64)

WHAT THE BOUND CAN SEE.  ``WRONG`` names the formulations it has to reject (tests/test_host_row_layernorm.py): the variance as
E[x^2] - mean^2 in fp32 on rows of mean 1e3 and spread 1, statistics accumulated in bf16, and -- for the add form's own property,
y == LN(stored s) -- statistics taken from the unrounded s.  ``two_pass_fp32`` is the straightforward evaluation that has to stay
inside on every input set of the GPU test."""
import math

import torch

U32 = 2.0 ** -24
ROW_UNIT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}       # uT (fp32: counted with u)
ULP_REL = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}   # one ulp of a value in [1, 2)
TINY = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
SLAB_ROWS = 128
EPS = 1e-5


# ---- the kernel's shape, restated ---------------------------------------------------------------------------------------------

def supported(c):
    return c % 8 == 0 and 32 <= c <= 1024


def lane_form(c):
    """(G lanes per row, V chunks of 8 channels per lane) -- U2_LN_DISPATCH of csrc/ln.hip"""
    c8 = c // 8
    for g in (8, 16, 32, 64):
        if c8 <= g:
            return g, 1
    return 64, 2


def channel_depth(c):
    g, v = lane_form(c)
    return 8 * v - 1 + int(math.log2(g))


def row_depth(n, c):
    g, _ = lane_form(c)
    return g // 2 + int(math.log2(64 // g)) + 3 + 1


def floor_ulp(ref, dtype):
    """one unit in the last place of ``dtype`` at the largest magnitude of ``ref`` (0 for an all-zero reference)"""
    m = float(ref.detach().abs().max()) if ref.numel() else 0.0
    if m == 0.0 or not math.isfinite(m):
        return 0.0
    return 2.0 ** math.floor(math.log2(m)) * ULP_REL[dtype]


# ---- float64 evaluations ------------------------------------------------------------------------------------------------------

def stream64(a, b, w, dtype):
    """the add form's stream row: a + w_row b, exact (float64 holds the 48-bit product and, for these magnitudes, the sum),
    rounded ONCE to fp32 and from there to the row type -- what one fp32 fused multiply-add followed by the store leaves"""
    s = a.double() + (b.double() if w is None else w.double().reshape(-1, 1) * b.double())
    return s.float().to(dtype)


def forward64(x, gamma, beta, eps=EPS):
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    dev = xd - mu
    var = (dev * dev).mean(1, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    xhat = dev * r
    return {'y': xhat * gamma.double() + beta.double(), 'mu': mu, 'var': var, 'r': r, 'dev': dev, 'xhat': xhat}


def backward64(dy, x, gamma, eps=EPS, ds=None, w=None):
    f = forward64(x, gamma, torch.zeros_like(gamma), eps)
    dyd = dy.double()
    g = dyd * gamma.double()
    s1 = g.mean(1, keepdim=True)
    s2 = (g * f['xhat']).mean(1, keepdim=True)
    t = g - s1 - f['xhat'] * s2
    dx = f['r'] * t
    if ds is not None:
        dx = dx + ds.double()
    out = {'dx': dx, 'dgamma': (dyd * f['xhat']).sum(0), 'dbeta': dyd.sum(0), 'g': g, 's1': s1, 's2': s2, 't': t, 'f': f}
    if w is not None:
        out['db'] = w.double().reshape(-1, 1) * dx
    return out


# ---- the bound ----------------------------------------------------------------------------------------------------------------

def _stat_errors(x, f, eps):
    """(dm, ed, dr, eh) of steps 1-5 for the rows x and their float64 statistics f"""
    u, c = U32, x.shape[1]
    D = channel_depth(c)
    xd = x.double()
    adev = f['dev'].abs()
    dm0 = (D + 2) * u * xd.abs().mean(1, keepdim=True)
    dm = torch.maximum(dm0, u * f['mu'].abs() + (D + 3) * u * (adev.mean(1, keepdim=True) + dm0))
    ed = dm + u * (adev + dm)
    dv = dm * dm + (D + 5) * u * (f['var'] + dm * dm)
    r_lo = 1.0 / torch.sqrt((f['var'] - dv).clamp(min=0.0) + eps)
    r_hi = 1.0 / torch.sqrt(f['var'] + dv + eps)
    dr = torch.maximum(r_lo - f['r'], f['r'] - r_hi) + 3 * u * r_lo
    eh = ed * (f['r'] + dr) + adev * dr + u * (adev + ed) * (f['r'] + dr)
    return dm, ed, dr, eh


def _stored(err, ref, dtype):
    """an fp32 result of error ``err`` stored in ``dtype``: + one rounding of the row type + the floor"""
    store = (ROW_UNIT[dtype] * (ref.abs() + err)).clamp(min=TINY[dtype]) if ROW_UNIT[dtype] else torch.zeros_like(err)
    return err + store + floor_ulp(ref, dtype)


def forward_bound(x, gamma, beta, dtype, eps=EPS, f=None):
    """elementwise bound on |y - y64| for rows x stored in ``dtype``"""
    f = f or forward64(x, gamma, beta, eps)
    u = U32
    _, _, _, eh = _stat_errors(x, f, eps)
    ag, ab = gamma.double().abs(), beta.double().abs()
    ey = ag * eh + 2 * u * ag * (f['xhat'].abs() + eh) + u * ab
    return _stored(ey, f['y'], dtype)


def backward_bound(dy, x, gamma, dtype, eps=EPS, ds=None, w=None, b=None):
    """{'dx', 'dgamma', 'dbeta' [, 'db']}: elementwise bounds next to backward64's values ``b``"""
    b = b or backward64(dy, x, gamma, eps, ds, w)
    f = b['f']
    u, (n, c) = U32, x.shape
    D, Dn = channel_depth(c), row_depth(n, c)
    _, _, dr, eh = _stat_errors(x, f, eps)
    ag, axh, ady = b['g'].abs(), f['xhat'].abs(), dy.double().abs()
    as1, as2 = b['s1'].abs(), b['s2'].abs()
    d1 = (D + 3) * u * ag.mean(1, keepdim=True)
    d2 = (ag * eh).mean(1, keepdim=True) + (D + 4) * u * (ag * (axh + eh)).mean(1, keepdim=True)
    et = (u * ag + d1 + eh * (as2 + d2) + axh * d2
          + u * (ag + as1 + d1) + 2 * u * (axh + eh) * (as2 + d2) + u * (ag + as1 + axh * as2))
    rr = f['r'] + dr
    edx = rr * et + dr * b['t'].abs() + u * rr * (b['t'].abs() + et)
    if ds is not None:
        edx = edx + u * (b['dx'].abs() + edx)
    out = {'dx': _stored(edx, b['dx'], dtype),
           'dgamma': (ady * eh).sum(0) + (Dn + 1) * u * (ady * (axh + eh)).sum(0) + floor_ulp(b['dgamma'], torch.float32),
           'dbeta': Dn * u * ady.sum(0) + floor_ulp(b['dbeta'], torch.float32)}
    if w is not None:
        edb = w.double().abs().reshape(-1, 1) * edx + u * b['db'].abs()
        out['db'] = _stored(edb, b['db'], dtype)
    return out


def worst(got, ref, bound):
    """(passes, largest |got - ref| / bound, largest |got - ref|): no element excluded; a zero bound asks for equality"""
    err = (got.double() - ref).abs()
    if err.numel() == 0:
        return True, 0.0, 0.0
    over = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, float('inf'), 0.0).to(err.dtype))
    return bool((err <= bound).all()), float(over.max()), float(err.max())


# ---- fp32 evaluations: the honest one and the wrong ones ----------------------------------------------------------------------

def two_pass_fp32(x, gamma, beta, dtype, eps=EPS):
    """the straightforward evaluation: fp32 mean, fp32 mean of the squared deviations, one rounding to the row type"""
    xf = x.float()
    mean = xf.mean(1, keepdim=True)
    dev = xf - mean
    rstd = 1.0 / torch.sqrt((dev * dev).mean(1, keepdim=True) + eps)
    return (dev * rstd * gamma + beta).to(dtype)


def two_pass_backward_fp32(dy, x, gamma, dtype, eps=EPS, ds=None, w=None):
    xf, dyf = x.float(), dy.float()
    mean = xf.mean(1, keepdim=True)
    dev = xf - mean
    rstd = 1.0 / torch.sqrt((dev * dev).mean(1, keepdim=True) + eps)
    xhat = dev * rstd
    g = dyf * gamma
    dx = rstd * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    if ds is not None:
        dx = dx + ds.float()
    out = {'dx': dx.to(dtype), 'dgamma': (dyf * xhat).sum(0), 'dbeta': dyf.sum(0)}
    if w is not None:
        out['db'] = (w.float().reshape(-1, 1) * dx).to(dtype)
    return out


def _wrong_e_x2(x, gamma, beta, dtype, eps=EPS):
    xf = x.float()
    mean = xf.mean(1, keepdim=True)
    var = ((xf * xf).mean(1, keepdim=True) - mean * mean).clamp(min=0.0)
    return ((xf - mean) / torch.sqrt(var + eps) * gamma + beta).to(dtype)


def _serial_sum_in(t, dtype):
    """sum over dim 1, the accumulator kept in ``dtype`` (one rounding per addition)"""
    acc = torch.zeros(t.shape[0], dtype=dtype)
    for j in range(t.shape[1]):
        acc = (acc.float() + t[:, j].float()).to(dtype)
    return acc.float().reshape(-1, 1)


def _wrong_bf16_stats(x, gamma, beta, dtype, eps=EPS):
    xf, c = x.float(), x.shape[1]
    mean = _serial_sum_in(xf, torch.bfloat16) / c
    dev = xf - mean
    var = _serial_sum_in(dev * dev, torch.bfloat16) / c
    return (dev / torch.sqrt(var + eps) * gamma + beta).to(dtype)


# the formulations the bound has to reject: name -> f(x, gamma, beta, dtype) -> y of the row type
WRONG = {'variance as E[x^2] - mean^2': _wrong_e_x2, 'statistics accumulated in bf16': _wrong_bf16_stats}


def add_form_unrounded_stats(a, b, w, gamma, beta, dtype, eps=EPS):
    """the add form done WRONG: the stream row is stored rounded, the statistics (and y) are taken from the unrounded fp32 sum"""
    s = (a.double() + (b.double() if w is None else w.double().reshape(-1, 1) * b.double())).float()      # (the fp32 fma's value)
    return s.to(dtype), two_pass_fp32(s, gamma, beta, dtype, eps)


# ---- the input sets (shared by the host test and the GPU test) ----------------------------------------------------------------

NS = (1, 7, 64, 257, 4099)
CS = (32, 40, 64, 128, 256, 512, 1024)
KINDS = ('randn', 'mean1e3', 'const')
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}


def make_case(n, c, kind, dtype, seed=0):
    """CPU tensors of one case, the same on every machine: rows x, dy, ds, a, b of ``dtype`` (rounded to it), gamma / beta fp32
    (random, not the initial 1 / 0), w fp32 [n] = DropPath's mask / keep at rate 0.3."""
    g = torch.Generator().manual_seed(100003 * seed + 131 * n + c + 7 * KINDS.index(kind))
    x = torch.randn(n, c, generator=g)
    if kind == 'mean1e3':       # mean 1e3, spread 1: where E[x^2] - mean^2 cancels
        x = x + 1e3
    elif kind == 'const':       # one repeated value per row: variance 0, rstd = 1 / sqrt(eps)
        x = torch.randn(n, 1, generator=g).expand(n, c).contiguous()
    elif kind != 'randn':
        raise ValueError(kind)
    a = torch.randn(n, c, generator=g)
    w = (torch.rand(n, generator=g) < 0.7).float() / 0.7
    return {'x': x.to(dtype), 'dy': torch.randn(n, c, generator=g).to(dtype), 'ds': torch.randn(n, c, generator=g).to(dtype),
            'a': a.to(dtype), 'b': (x - a).to(dtype), 'w': w,
            'gamma': 1.0 + 0.5 * torch.randn(c, generator=g), 'beta': torch.randn(c, generator=g)}
