"""float64 reference of the scene kernels (csrc/gn.hip: u2mkd_gn_forward, u2mkd_gn_backward, u2mkd_scene_pool_forward,
u2mkd_scene_pool_backward), and the elementwise bound the GroupNorm kernels are held to (test helper; plain torch).

WHAT IS COMPUTED.  Rows ``x [n, c]`` of the row type T (fp32, bf16, fp16), a batch index ``bidx [n]`` per row, ``gamma``, ``beta``
fp32 [c] (None: 1 / 0).  A SCENE k is the set of rows with bidx == k (they need not be contiguous), a GROUP g of G the channels
[g c / G, (g + 1) c / G).  Per (scene, group), over its m = (c / G) N_k STORED values,

    mu = mean(x)   var = mean((x - mu)^2) (biased)   r = 1 / sqrt(var + eps)   xhat = (x - mu) r   y = xhat gamma + beta
    g = dy gamma   s1 = mean(g)   s2 = mean(g xhat)   dx = r (g - s1 - xhat s2)
    dgamma = sum over ALL rows of dy xhat            dbeta = sum over all rows of dy

which is ``torch.nn.functional.group_norm(x[bidx == k].T.reshape(1, c, -1), G, gamma, beta, eps)`` transposed back, scene by
scene (the loop formulation torchsparse v1.4.0 runs; tests/test_host_group_norm_bound.py holds this file to it, through
``torch.group_norm``, the operator behind that wrapper, which also takes a scene of one row).  A batch index
without rows contributes nothing.  ``forward64`` / ``backward64`` evaluate this in float64.

THE BOUND is that of a two-pass evaluation in fp32 arithmetic throughout: the mean, then the mean of the squared deviations from
the computed mean, every sum a PAIRWISE fp32 sum (``two_pass_fp32``: halves added level by level, D = ceil(log2 m) additions on
any path).  The kernels carry every sum in double and round once per stored value (slab partials, mean, rstd, the results), which
makes every term below smaller; the bound is kept at the fp32 sequence so that the straightforward evaluation is inside it as
well.  u = 2^-24 is fp32's unit roundoff, uT the row type's (0 for fp32 rows -- their last rounding is an fp32 one and is counted
there --, 2^-8 for bf16, 2^-11 for fp16).  Every term is u times a magnitude THAT IS ACTUALLY SUMMED, to first order in u with
the second-order parts kept where they are cheap to keep.  No constant is fitted to a measured error.

 A pairwise sum of terms t_j is off by at most D u sum |t_j|; times 1 / m (the product or quotient rounds once, the constant
 once): (D + 2) u mean |t_j| for a mean.

 1  the mean:  dm = (D + 2) u mean|x|.
 2  a deviation in registers, fl(x_j - m^):  ed_j = dm + u (|x_j - mu| + dm).
 3  the variance, the mean of the squared deviations from m^: sum_j (x_j - m^)^2 = m var + m (m^ - mu)^2, every square carries
    2 u (its operand) + u (the product), the sum D u, the division 2 u:  dv = dm^2 + (D + 5) u (var + dm^2).
 4  r = 1 / sqrt(v + eps): 3 u covers an fp32 evaluation's three roundings and eps's own (the fp32 value of 1e-5); the change of
    1 / sqrt over [var - dv, var + dv] is taken at the ends of the interval (var = 0 is a case):
        dr = max(r(var - dv) - r, r - r(var + dv)) + 3 u r(var - dv).
    mean and rstd as stored:  bound(mean) = dm + floor32(mean),  bound(rstd) = dr + floor32(rstd).
 5  xhat in registers, fl(fl(x_j - m^) r^):  eh_j = ed_j (r + dr) + |x_j - mu| dr + u (|x_j - mu| + ed_j)(r + dr).
 6  y = fl(fl(xhat^ gamma) + beta):  Ey_j = |gamma_j| eh_j + 2 u |gamma_j| (|xhat_j| + eh_j) + u |beta_j|
        bound(y) = Ey + max(uT (|y64| + Ey), tinyT) + floor(y64)

 ``floor`` is one unit in the last place of the stored type at the largest reference magnitude of the output, which every
 evaluation that returns the type may have; tinyT = 2^-25 is half the distance of fp16's subnormals (a store below 2^-14 loses up
 to that whatever its size), 0 for the other types.

 Backward, from the forward's m^ and r^ (errors dm, dr) and the recomputed xhat^ (error eh_j):
 7  g_j = fl(dy_j gamma_j): u |g_j|.   s1: d1 = (D + 3) u mean|g|.
    s2 = mean(g xhat^):  d2 = mean(|g| eh) + (D + 4) u mean(|g| (|xhat| + eh)).
 8  t_j = g_j - s1 - xhat^_j s2, the three terms subtracted in fp32:
        et_j = u |g_j| + d1 + eh_j (|s2| + d2) + |xhat_j| d2                                          (errors of the operands)
             + u (|g_j| + |s1| + d1) + 2 u (|xhat_j| + eh_j)(|s2| + d2) + u (|g_j| + |s1| + |xhat_j s2|)      (roundings)
 9  dx_j = fl(r^ t_j):  Edx_j = (r + dr) et_j + dr |t64_j| + u (r + dr)(|t64_j| + et_j)
        bound(dx) = Edx + max(uT (|dx64| + Edx), tinyT) + floor(dx64)
 10 sums over all n rows, pairwise, Dn = ceil(log2 n):
        bound(dgamma) = sum_rows |dy| eh + (Dn + 1) u sum_rows |dy| (|xhat| + eh) + floor32(dgamma64)
        bound(dbeta)  = Dn u sum_rows |dy| + floor32(dbeta64)

WHAT THE BOUND CAN SEE.  ``WRONG`` names the formulations it has to reject (tests/test_host_group_norm_bound.py): statistics per
channel instead of per group, statistics over the whole batch instead of per scene, the unbiased variance, the variance as
E[x^2] - mean^2 in fp32 on rows of mean 1e3 and spread 1, and a dropped slab (the first 128 rows of a scene left out of its
statistics).  ``two_pass_fp32`` is the straightforward evaluation that has to stay inside on every input set of the GPU test.

POOLING.  ``pool64``: per scene the column mean in float64 (NaN for a batch index without rows) and the column max with the
smallest row index among the maxima (-inf / -1 without rows).  The kernels carry the column sums in double up to the one
division, so the mean is held to ONE fp32 ulp of the float64 mean (``ulp32``), the max to equality."""
import functools
import math

import torch

U32 = 2.0 ** -24
ROW_UNIT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}       # uT (fp32: counted with u)
ULP_REL = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}   # one ulp of a value in [1, 2)
TINY = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
SLAB_ROWS = 128
EPS = 1e-5


def depth(m):
    """additions on any path of a pairwise sum of m terms"""
    return int(math.ceil(math.log2(m))) if m > 1 else 0


def floor_ulp(ref, dtype):
    """one unit in the last place of ``dtype`` at the largest magnitude of ``ref`` (0 for an all-zero reference)"""
    m = float(ref.detach().abs().max()) if ref.numel() else 0.0
    if m == 0.0 or not math.isfinite(m):
        return 0.0
    return 2.0 ** math.floor(math.log2(m)) * ULP_REL[dtype]


def scenes(bidx):
    """(nb, [(k, ascending row ids of scene k)] for every batch index that has rows)"""
    b = bidx.long()
    nb = int(b.max()) + 1 if b.numel() else 0
    out = []
    for k in range(nb):
        idx = (b == k).nonzero().reshape(-1)
        if idx.numel():
            out.append((k, idx))
    return nb, out


# ---- float64 evaluations ------------------------------------------------------------------------------------------------------

def _g3(t, groups):
    """[nk, c] -> [nk, G, c / G]"""
    return t.reshape(t.shape[0], groups, t.shape[1] // groups)


def forward64(x, bidx, groups, gamma=None, beta=None, eps=EPS):
    """{'y' [n, c], 'mean' / 'rstd' [nb, G] (0 for a batch index without rows), and per element 'mu', 'var', 'r', 'dev', 'xhat'
    [n, c], 'm' [n, 1] = the number of values its statistics were taken over}"""
    n, c = x.shape
    xd = x.double()
    gd = torch.ones(c, dtype=torch.float64) if gamma is None else gamma.double()
    bd = torch.zeros(c, dtype=torch.float64) if beta is None else beta.double()
    nb, sc = scenes(bidx)
    out = {k: torch.zeros(n, c, dtype=torch.float64) for k in ('mu', 'var', 'r', 'dev', 'xhat')}
    out['m'] = torch.ones(n, 1, dtype=torch.float64)
    out['mean'] = torch.zeros(nb, groups, dtype=torch.float64)
    out['rstd'] = torch.zeros(nb, groups, dtype=torch.float64)
    for k, idx in sc:
        xs = _g3(xd[idx], groups)
        mu = xs.mean((0, 2), keepdim=True)
        dev = xs - mu
        var = (dev * dev).mean((0, 2), keepdim=True)
        r = 1.0 / torch.sqrt(var + eps)
        out['mean'][k], out['rstd'][k] = mu.reshape(-1), r.reshape(-1)
        for name, v in (('mu', mu), ('var', var), ('r', r), ('dev', dev), ('xhat', dev * r)):
            out[name][idx] = v.expand_as(xs).reshape(idx.numel(), c)
        out['m'][idx] = float(idx.numel() * (c // groups))
    out['y'] = out['xhat'] * gd + bd
    out['gamma'], out['beta'], out['scenes'], out['nb'] = gd, bd, sc, nb
    return out


def backward64(dy, x, bidx, groups, gamma=None, eps=EPS, f=None):
    f = f or forward64(x, bidx, groups, gamma, None, eps)
    n, c = x.shape
    dyd = dy.double()
    g = dyd * f['gamma']
    s1, s2 = torch.zeros(n, c, dtype=torch.float64), torch.zeros(n, c, dtype=torch.float64)
    for k, idx in f['scenes']:
        gs, hs = _g3(g[idx], groups), _g3(f['xhat'][idx], groups)
        s1[idx] = gs.mean((0, 2), keepdim=True).expand_as(gs).reshape(idx.numel(), c)
        s2[idx] = (gs * hs).mean((0, 2), keepdim=True).expand_as(gs).reshape(idx.numel(), c)
    t = g - s1 - f['xhat'] * s2
    return {'dx': f['r'] * t, 'dgamma': (dyd * f['xhat']).sum(0), 'dbeta': dyd.sum(0), 'g': g, 's1': s1, 's2': s2, 't': t, 'f': f}


# ---- the bound ----------------------------------------------------------------------------------------------------------------

def _group_mean(t, f, groups):
    """per element: the mean of ``t`` over the element's (scene, group)"""
    out = torch.zeros_like(t)
    for _, idx in f['scenes']:
        ts = _g3(t[idx], groups)
        out[idx] = ts.mean((0, 2), keepdim=True).expand_as(ts).reshape(idx.numel(), t.shape[1])
    return out


def _stat_errors(x, f, groups, eps):
    """(dm, ed, dr, eh) of steps 1-5, per element"""
    u = U32
    D = torch.ceil(torch.log2(f['m'])).clamp(min=0.0)
    adev = f['dev'].abs()
    dm = (D + 2) * u * _group_mean(x.double().abs(), f, groups)
    ed = dm + u * (adev + dm)
    dv = dm * dm + (D + 5) * u * (f['var'] + dm * dm)
    r_lo = 1.0 / torch.sqrt((f['var'] - dv).clamp(min=0.0) + eps)
    r_hi = 1.0 / torch.sqrt(f['var'] + dv + eps)
    dr = torch.maximum(r_lo - f['r'], f['r'] - r_hi) + 3 * u * r_lo
    eh = ed * (f['r'] + dr) + adev * dr + u * (adev + ed) * (f['r'] + dr)
    return D, dm, ed, dr, eh


def _stored(err, ref, dtype):
    """an fp32 result of error ``err`` stored in ``dtype``: + one rounding of the row type + the floor"""
    store = (ROW_UNIT[dtype] * (ref.abs() + err)).clamp(min=TINY[dtype]) if ROW_UNIT[dtype] else torch.zeros_like(err)
    return err + store + floor_ulp(ref, dtype)


def _per_group(t, f, groups):
    """a per-element quantity that is constant over a (scene, group), as [nb, G] (0 for a batch index without rows)"""
    out = torch.zeros(f['nb'], groups, dtype=torch.float64)
    for k, idx in f['scenes']:
        out[k] = _g3(t[idx[:1]], groups)[0, :, 0]
    return out


def forward_bound(x, bidx, groups, gamma, beta, dtype, eps=EPS, f=None):
    """{'y' [n, c], 'mean', 'rstd' [nb, G]}: elementwise bounds next to forward64's values"""
    f = f or forward64(x, bidx, groups, gamma, beta, eps)
    u = U32
    _, dm, _, dr, eh = _stat_errors(x, f, groups, eps)
    ag, ab = f['gamma'].abs(), f['beta'].abs()
    ey = ag * eh + 2 * u * ag * (f['xhat'].abs() + eh) + u * ab
    return {'y': _stored(ey, f['y'], dtype),
            'mean': _per_group(dm, f, groups) + floor_ulp(f['mean'], torch.float32),
            'rstd': _per_group(dr, f, groups) + floor_ulp(f['rstd'], torch.float32)}


def backward_bound(dy, x, bidx, groups, gamma, dtype, eps=EPS, b=None):
    """{'dx', 'dgamma', 'dbeta'}: elementwise bounds next to backward64's values ``b``"""
    b = b or backward64(dy, x, bidx, groups, gamma, eps)
    f = b['f']
    u, n = U32, x.shape[0]
    D, _, _, dr, eh = _stat_errors(x, f, groups, eps)
    Dn = depth(n)
    ag, axh, ady = b['g'].abs(), f['xhat'].abs(), dy.double().abs()
    as1, as2 = b['s1'].abs(), b['s2'].abs()
    d1 = (D + 3) * u * _group_mean(ag, f, groups)
    d2 = _group_mean(ag * eh, f, groups) + (D + 4) * u * _group_mean(ag * (axh + eh), f, groups)
    et = (u * ag + d1 + eh * (as2 + d2) + axh * d2
          + u * (ag + as1 + d1) + 2 * u * (axh + eh) * (as2 + d2) + u * (ag + as1 + axh * as2))
    rr = f['r'] + dr
    edx = rr * et + dr * b['t'].abs() + u * rr * (b['t'].abs() + et)
    return {'dx': _stored(edx, b['dx'], dtype),
            'dgamma': (ady * eh).sum(0) + (Dn + 1) * u * (ady * (axh + eh)).sum(0) + floor_ulp(b['dgamma'], torch.float32),
            'dbeta': Dn * u * ady.sum(0) + floor_ulp(b['dbeta'], torch.float32)}


def worst(got, ref, bound):
    """(passes, largest |got - ref| / bound, largest |got - ref|): no element excluded; a zero bound asks for equality"""
    err = (got.double().cpu() - ref).abs()
    if err.numel() == 0:
        return True, 0.0, 0.0
    over = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, float('inf'), 0.0).to(err.dtype))
    return bool((err <= bound).all()), float(over.max()), float(err.max())


# ---- fp32 evaluations: the honest one and the wrong ones ----------------------------------------------------------------------

def pairwise_sum(t):
    """sum over dim 0 in t's dtype, halves added level by level (a padding zero adds exactly): depth(m) additions on any path"""
    while t.shape[0] > 1:
        if t.shape[0] % 2:
            t = torch.cat([t, torch.zeros_like(t[:1])])
        t = t[0::2] + t[1::2]
    return t[0]


def _flat(ts):
    """[nk, G, cg] -> [nk * cg, G]: a (scene, group)'s values along dim 0"""
    return ts.permute(0, 2, 1).reshape(-1, ts.shape[1])


def _fp32_stats(xs, eps, variant=''):
    """(mean, rstd) [1, G, 1] of one scene's values xs [nk, G, cg] fp32"""
    m = xs.shape[0] * xs.shape[2]
    mean = (pairwise_sum(_flat(xs)) / m).reshape(1, -1, 1)
    if variant == 'e_x2':
        var = (pairwise_sum(_flat(xs * xs)) / m).reshape(1, -1, 1) - mean * mean
        var = var.clamp(min=0.0)
    else:
        dev = xs - mean
        var = (pairwise_sum(_flat(dev * dev)) / (m - 1 if variant == 'unbiased' and m > 1 else m)).reshape(1, -1, 1)
    return mean, 1.0 / torch.sqrt(var + eps)


def two_pass_fp32(x, bidx, groups, gamma, beta, dtype, eps=EPS, variant=''):
    """the straightforward evaluation: per (scene, group) the fp32 mean, the fp32 mean of the squared deviations, one rounding
    to the row type.  ``variant`` names a WRONG formulation."""
    n, c = x.shape
    xf = x.float()
    g = torch.ones(c) if gamma is None else gamma.float()
    b = torch.zeros(c) if beta is None else beta.float()
    y = torch.zeros(n, c)
    _, sc = scenes(bidx)
    if variant == 'whole_batch':
        sc = [(0, torch.arange(n))]
    for _, idx in sc:
        xs = _g3(xf[idx], c if variant == 'per_channel' else groups)
        if variant == 'dropped_slab' and idx.numel() > SLAB_ROWS:
            mean, rstd = _fp32_stats(xs[SLAB_ROWS:], eps)
        else:
            mean, rstd = _fp32_stats(xs, eps, variant)
        y[idx] = ((xs - mean) * rstd).reshape(idx.numel(), c)
    return (y * g + b).to(dtype)


def two_pass_backward_fp32(dy, x, bidx, groups, gamma, dtype, eps=EPS):
    n, c = x.shape
    xf, dyf = x.float(), dy.float()
    g = torch.ones(c) if gamma is None else gamma.float()
    gr = dyf * g
    dx, xhat = torch.zeros(n, c), torch.zeros(n, c)
    for _, idx in scenes(bidx)[1]:
        xs, gs = _g3(xf[idx], groups), _g3(gr[idx], groups)
        m = xs.shape[0] * xs.shape[2]
        mean, rstd = _fp32_stats(xs, eps)
        hs = (xs - mean) * rstd
        s1 = (pairwise_sum(_flat(gs)) / m).reshape(1, -1, 1)
        s2 = (pairwise_sum(_flat(gs * hs)) / m).reshape(1, -1, 1)
        dx[idx] = (rstd * (gs - s1 - hs * s2)).reshape(idx.numel(), c)
        xhat[idx] = hs.reshape(idx.numel(), c)
    return {'dx': dx.to(dtype), 'dgamma': pairwise_sum(dyf * xhat), 'dbeta': pairwise_sum(dyf)}


# the formulations the bound has to reject: name -> variant of two_pass_fp32
WRONG = {'statistics per channel instead of per group': 'per_channel',
         'statistics over the whole batch instead of per scene': 'whole_batch',
         'the unbiased variance': 'unbiased',
         'variance as E[x^2] - mean^2': 'e_x2',
         'a dropped slab': 'dropped_slab'}


# ---- pooling ------------------------------------------------------------------------------------------------------------------

def pool64(x, bidx):
    """{'avg' [nb, c] float64, 'max' [nb, c] in x's dtype, 'arg' [nb, c] int64, 'count' [nb]}"""
    n, c = x.shape
    nb, sc = scenes(bidx)
    avg = torch.full((nb, c), float('nan'), dtype=torch.float64)
    mx = torch.full((nb, c), float('-inf'), dtype=x.dtype)
    arg = torch.full((nb, c), -1, dtype=torch.int64)
    cnt = torch.zeros(nb, dtype=torch.int64)
    for k, idx in sc:
        xs = x[idx]
        avg[k] = xs.double().mean(0)
        mx[k] = xs.max(0).values
        first = (xs == mx[k]).int().argmax(0)          # the first row among the maxima (ascending row ids)
        arg[k] = idx[first]
        cnt[k] = idx.numel()
    return {'avg': avg, 'max': mx, 'arg': arg, 'count': cnt}


def ulp32(ref):
    """one fp32 unit in the last place at every element of the float64 reference (the smallest normal's for anything below)"""
    a = ref.abs().clamp(min=2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(a))) * 2.0 ** -23


# ---- the input sets (shared by the host test and the GPU tests) ---------------------------------------------------------------

SHAPES = ((32, 4), (48, 16), (64, 64), (96, 1), (128, 32))
SHAPES16 = ((32, 4), (48, 16))
KINDS = ('randn', 'mean1e3', 'const')
LAYOUTS = ('L1', 'L2', 'L3')
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
CONST_SCENE = {'L1': 4, 'L2': 4, 'L3': 3}       # the scene that holds one value in the 'const' kind: it spans three slabs


@functools.lru_cache(maxsize=None)
def layout(name):
    """the batch index of every row, int32 [n]:
    L1 contiguous scenes of 1, 127, 128, 129, 257 rows; L2 the same rows shuffled with a fixed seed; L3 batch indices 0, 2, 3 of
    40, 5, 300 rows, index 1 absent"""
    if name in ('L1', 'L2'):
        b = torch.cat([torch.full((k,), i, dtype=torch.int32) for i, k in enumerate((1, 127, 128, 129, 257))])
        if name == 'L2':
            b = b[torch.randperm(b.numel(), generator=torch.Generator().manual_seed(20))]
        return b
    if name == 'L3':
        return torch.cat([torch.full((k,), i, dtype=torch.int32) for i, k in ((0, 40), (2, 5), (3, 300))])
    raise ValueError(name)


def coords_of(bidx):
    """int32 [n, 4] = (x, y, z, b): distinct voxels, the batch index last"""
    n = bidx.numel()
    i = torch.arange(n, dtype=torch.int32)
    return torch.stack([i % 37, (i // 37) % 41, i // (37 * 41), bidx.int()], 1).contiguous()


@functools.lru_cache(maxsize=None)
def make_case(lay, c, kind, dtype, seed=0):
    """CPU tensors of one case, the same on every machine: bidx, rows x and dy of ``dtype`` (rounded to it), gamma / beta fp32
    (random, not the initial 1 / 0).  Treat as read-only: the cases are shared."""
    bidx = layout(lay)
    n = bidx.numel()
    g = torch.Generator().manual_seed(100003 * seed + 131 * n + c + 7 * KINDS.index(kind) + 1009 * LAYOUTS.index(lay))
    x = torch.randn(n, c, generator=g)
    if kind == 'mean1e3':       # mean 1e3, spread 1: where E[x^2] - mean^2 cancels
        x = x + 1e3
    elif kind == 'const':       # one scene holds one value: variance 0, rstd = 1 / sqrt(eps), y = beta
        x[bidx == CONST_SCENE[lay]] = 0.7310585975646973
    elif kind != 'randn':
        raise ValueError(kind)
    return {'bidx': bidx, 'x': x.to(dtype), 'dy': torch.randn(n, c, generator=g).to(dtype),
            'gamma': 1.0 + 0.5 * torch.randn(c, generator=g), 'beta': torch.randn(c, generator=g)}


@functools.lru_cache(maxsize=None)
def reference(lay, c, groups, kind, dtype, affine):
    """(case, forward64, forward bounds, backward64, backward bounds) of one case, computed once and shared"""
    case = make_case(lay, c, kind, dtype)
    gamma, beta = (case['gamma'], case['beta']) if affine else (None, None)
    f = forward64(case['x'], case['bidx'], groups, gamma, beta)
    fb = forward_bound(case['x'], case['bidx'], groups, gamma, beta, dtype, f=f)
    b = backward64(case['dy'], case['x'], case['bidx'], groups, gamma, f=f)
    bb = backward_bound(case['dy'], case['x'], case['bidx'], groups, gamma, dtype, b=b)
    return case, f, fb, b, bb
