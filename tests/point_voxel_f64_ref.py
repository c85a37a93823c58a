"""float64 reference of the point <-> voxel row movers (csrc/voxel.hip: u2mkd_voxelize_forward / _backward, u2mkd_devoxelize_forward /
_backward, u2mkd_segment_sum, u2mkd_segment_mean, their _bf16 / _f16 entries, u2mkd_ti_weights), and the elementwise bound they
are held to (test helper; plain torch on the CPU).

WHAT IS COMPUTED.  Rows of the row type T (fp32, bf16, fp16) are moved between points and voxels:

    voxelize        out[v] = sum over {i: idx[i] = v, 0 <= v < nv, counts[v] > 0} of x[i] / counts[v]      (0 where counts[v] = 0)
    its backward    gx[i] = g[idx[i]] / counts[idx[i]]     (0 for idx[i] outside [0, nv) or counts = 0)
    devoxelize      out[i] = sum over the corners k of 8 with idx8[i, k] >= 0 of w8[i, k] f[idx8[i, k]]
    its backward    gf[v] = sum over {(i, k): idx8[i, k] = v, w8[i, k] != 0} of w8[i, k] g[i]
    segment sum     out[v] = sum over the entries e of segment v (seg[v] <= e < seg[v + 1]) of ew[e] src[erow[e]]  (ew None: 1);
                    mean: every term divided by the segment length, or by counts[v] (u2mkd_segment_mean: 0 where counts[v] <= 0)
    ti_weights      the 8 trilinear weights of a point in its cell of edge ``scale``, zeroed at a missing corner (index -1),
                    divided by (their sum + 1e-8)

All of them are ONE form -- a list of entries (destination, source row, weight) grouped by destination and a divisor per
destination -- and ``segment_full`` evaluates that form in float64 on the STORED inputs (the values the row type holds).  The
named functions (``voxelize64``, ``voxelize_bwd64``, ``devoxelize64``, ``devoxelize_bwd64``, ``segment64``, ``ti_weights64``) build
the entry list of their operation and call it; tests/test_host_point_voxel_bound.py holds them to oracle/ts_ref on double inputs.

Zero-weight corners: the backward of devoxelize drops them (u2mkd_devoxelize_plan and the atomic kernel alike), so a NaN gradient
row does not reach a voxel through a zero weight; the forward multiplies (0 * NaN = NaN).  The reference follows both.
PRECONDITION of u2mkd_devoxelize_forward: every index is < nv -- the entry has no nv argument and reads feats[idx]; an index
>= nv is undefined in torchsparse too.  No input set here has one.

THE BOUND.  u = 2^-24 (fp32), gamma_k = k u / (1 - k u) (k roundings compounded), uT the row type's unit roundoff (2^-8 bf16,
2^-11 fp16; fp32 rows: the last rounding is an fp32 one and is counted in E), tinyT = 2^-25 for fp16 (a store below 2^-14 loses up
to half a subnormal step), 0 otherwise.  16-bit inputs widen exactly.  The bound holds for ANY order of the additions, so one bound
serves the CSR forms (fixed order), the atomic forms (any order) and an fma contraction (fewer roundings).  Roundings counted from
the kernels:

  scatter-mean, m terms      fl(x_j / c): 1 per term; the sum: m - 1 additions on the longest path (the first addition is to 0 and is
                             exact); a term passes at most 1 + (m - 1) roundings:          E = gamma_m sum|x_j| / c
                             (c = counts[v]; the segment length m where no counts are given)
  weighted sum, m terms      fl(w_e s_e): 1 per term, m - 1 additions (0 + t exact):        E = gamma_m sum|w_e s_e|
                             devoxelize forward: m = 8 (the corners present are <= 8); its backward and the segment sums: m = the
                             segment's length.  Without weights the product is exact; gamma_m is kept.
  voxelize backward          one division:                                                  E = u |ref|
  ti_weights (scale a power of two: p / scale, floor, * scale, + scale, scale^3 and the division by it are exact)
                             a weight: 3 differences + 2 products + the division by s3 = 6 roundings; the sum of the 8 (all >= 0):
                             7 additions (the first is to 0) + the constant = 8 more on the longest path, 14 in the denominator;
                             1 / (1 + theta_14) = 1 + theta_15; the quotient 1:   6 + 15 + 1 = 22:        E_k = gamma_22 w_k
                             (the constant is the fp32 value of 1e-8, as the kernel holds it)

  stored:  bound = E                                    fp32 rows
           bound = E + max(uT (|ref| + E), tinyT)       16-bit rows

A ZERO BOUND ASKS FOR EQUALITY (``compare``): empty voxels, points outside [0, nv) in the backward, points without a corner, the
weight of a missing corner.  No element is excluded and no constant is fitted.  Non-finite values are compared by class: where the
reference is NaN the result must be NaN, and nowhere else; an fp16 element whose reference lies beyond 65520 (the value from which
rounding to nearest gives inf) by more than its bound must be inf of that sign.  A finite reference within its bound of
[65504, 65520] could be either; ``straddles`` counts them, the inputs are chosen so that there are none (the host test asserts it),
and ``compare`` fails on one.

WHAT THE BOUND CAN SEE.  ``segment_fp32`` / ``ti_weights_fp32`` evaluate in fp32 with one rounding to the row type at the end: the
sums in ascending entry order (the kernels' order: for fp32 rows and the mean it IS torchsparse's in-order loop
``out[idx[i]] += x[i] / counts[idx[i]]``, which the GPU test holds u2mkd_segment_sum / u2mkd_segment_mean to bit for bit), descending
and pairwise: all inside the bound.  ``WRONG`` names the formulations it has to reject, each on a named input set."""
import functools

import torch

U32 = 2.0 ** -24
ROW_UNIT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
F16_MAX, F16_INF = 65504.0, 65520.0
TI_ROUNDINGS = 22
EPS32 = float(torch.tensor(1e-8, dtype=torch.float32))


def gamma(k):
    k = torch.as_tensor(k, dtype=torch.float64)
    return k * U32 / (1.0 - k * U32)


def stored(err, ref, dtype):
    """the bound of a result of computation error ``err`` stored in ``dtype``"""
    if not ROW_UNIT[dtype]:
        return err
    return err + (ROW_UNIT[dtype] * (ref.abs() + err)).clamp(min=TINY[dtype])


def straddles(ref, bound, dtype):
    """number of finite references whose interval [|ref| - bound, |ref| + bound] meets [65504, 65520] (fp16 rows)"""
    if dtype != torch.float16:
        return 0
    a = ref.abs()
    return int((ref.isfinite() & bound.isfinite() & (a + bound >= F16_MAX) & (a - bound <= F16_INF)).sum())


def worst(got, ref, bound):
    """(passes, largest |got - ref| / bound, largest |got - ref|): no element excluded; a zero bound asks for equality"""
    return _worst((got.double().cpu() - ref).abs(), bound)


def _worst(err, bound):
    if err.numel() == 0:
        return True, 0.0, 0.0
    over = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, float('inf'), 0.0).to(err.dtype))
    fin = err[err.isfinite()]
    return bool((err <= bound).all()), float(over.max()), float(fin.max()) if fin.numel() else float('inf')


def compare(got, ref, bound, dtype):
    """``worst`` with the non-finite classes: NaN exactly where the reference is NaN; inf of the reference's sign where it lies
    beyond fp16's range by more than the bound; everything else finite and within the bound; a straddling element fails"""
    assert got.dtype == dtype and tuple(got.shape) == tuple(ref.shape), (got.dtype, got.shape, ref.shape)
    g = got.double().cpu()
    inf = torch.full_like(ref, float('inf'))
    zero = torch.zeros_like(ref)
    nan = ref.isnan()
    b = torch.where(nan, zero, bound)
    err = torch.where(nan, torch.where(g.isnan(), zero, inf), torch.nan_to_num((g - ref).abs(), nan=float('inf'), posinf=float('inf')))
    if dtype == torch.float16:
        a = ref.abs()
        over = ~nan & (a - b > F16_INF)
        err = torch.where(over, torch.where(g == torch.sign(ref) * inf, zero, inf), err)
        edge = ~nan & ~over & (a + b >= F16_MAX)
        err = torch.where(edge, inf, err)
        b = torch.where(over | edge, zero, b)
    return _worst(err, b)


# ---- entry lists --------------------------------------------------------------------------------------------------------------

def csr(keys, nv):
    """(order int32 [E], seg int32 [nv + 1]): the entries with 0 <= key < nv grouped by key, ascending entry id inside a group --
    what u2mkd_csr_build leaves in order[:seg[nv]]"""
    k = keys.long().reshape(-1)
    ids = ((k >= 0) & (k < nv)).nonzero().reshape(-1)
    order = ids[torch.argsort(k[ids], stable=True)]
    seg = torch.zeros(nv + 1, dtype=torch.int64)
    seg[1:] = torch.cumsum(torch.bincount(k[ids], minlength=nv), 0)
    return order.int(), seg.int()


def devoxelize_plan(idx8, w8, nv):
    """(entry_row = point, entry_w, seg) of devoxelize's backward, as u2mkd_devoxelize_plan: zero-weight corners dropped"""
    keys = torch.where(w8 != 0, idx8.long(), torch.full_like(idx8.long(), -1)).reshape(-1)
    order, seg = csr(keys, nv)
    return (order.long() // 8).int(), w8.reshape(-1)[order.long()].contiguous(), seg


def devoxelize_fwd_plan(idx8, w8, variant=''):
    """devoxelize's forward as an entry list: destination = the point, source row = the voxel, corners ascending"""
    i = idx8.long()
    n = i.shape[0]
    w = w8.reshape(-1).reshape(8, n).t() if variant == 'w8_transposed' else w8
    ok = torch.ones_like(i, dtype=torch.bool) if variant == 'missing_as_row0' else i >= 0
    seg = torch.zeros(n + 1, dtype=torch.int64)
    seg[1:] = torch.cumsum(ok.sum(1), 0)
    return i.clamp(min=0)[ok].int(), w[ok].contiguous(), seg.int()


def _segments(seg):
    """(destination of every entry [E], length of every segment [nv], position of every entry inside its segment [E])"""
    s = seg.long()
    lens = s[1:] - s[:-1]
    dest = torch.repeat_interleave(torch.arange(lens.numel()), lens)
    return dest, lens, torch.arange(int(s[-1])) - s[:-1][dest]


# ---- float64 ------------------------------------------------------------------------------------------------------------------

def segment_full(src, erow, ew, seg, mean=False, counts=None):
    """(reference, computation error E) float64 [nv, c] of the segment form"""
    dest, lens, _ = _segments(seg)
    e = dest.numel()
    t = src.double()[erow[:e].long()]
    if ew is not None:
        t = t * ew[:e].double()[:, None]
    nv, c = lens.numel(), src.shape[1]
    s = torch.zeros(nv, c, dtype=torch.float64).index_add_(0, dest, t)
    a = torch.zeros(nv, c, dtype=torch.float64).index_add_(0, dest, t.abs())
    if mean:
        d = (lens if counts is None else counts.long()).double()[:, None]
        s = torch.where(d > 0, s / d.clamp(min=1.0), torch.zeros_like(s))
        a = torch.where(d > 0, a / d.clamp(min=1.0), torch.zeros_like(a))
    return s, gamma(lens)[:, None] * a


def segment64(src, erow, ew, seg, mean=False, counts=None):
    return segment_full(src, erow, ew, seg, mean, counts)[0]


def voxelize_full(x, idx, counts):
    order, seg = csr(idx, counts.numel())
    return segment_full(x, order, None, seg, True, counts)


def voxelize64(x, idx, counts):
    return voxelize_full(x, idx, counts)[0]


def voxelize_bwd_full(g, idx, counts):
    nv = counts.numel()
    i = idx.long().reshape(-1)
    ok = (i >= 0) & (i < nv)
    cnt = torch.where(ok, counts.long()[i.clamp(0, max(nv - 1, 0))], torch.zeros_like(i)).double()[:, None]
    rows = g.double()[i.clamp(0, max(nv - 1, 0))]
    ref = torch.where(cnt > 0, rows / cnt.clamp(min=1.0), torch.zeros_like(rows))
    return ref, U32 * ref.abs()


def voxelize_bwd64(g, idx, counts):
    return voxelize_bwd_full(g, idx, counts)[0]


def devoxelize_full(f, idx8, w8):
    i = idx8.long()
    t = f.double()[i.clamp(min=0)] * w8.double()[:, :, None]
    t = torch.where((i >= 0)[:, :, None], t, torch.zeros_like(t))
    return t.sum(1), gamma(8) * t.abs().sum(1)


def devoxelize64(f, idx8, w8):
    return devoxelize_full(f, idx8, w8)[0]


def devoxelize_bwd_full(g, idx8, w8, nv):
    return segment_full(g, *devoxelize_plan(idx8, w8, nv))


def devoxelize_bwd64(g, idx8, w8, nv):
    return devoxelize_bwd_full(g, idx8, w8, nv)[0]


def _ti(p, idx_kn, s, eps, floor):
    """ti_weights_kernel's formula in p's dtype: [n, 8]"""
    pf = floor(p / s) * s if s != 1 else floor(p)
    lo, hi = p - pf, (pf + s) - p
    w = torch.stack([(lo[:, 0] if k & 4 else hi[:, 0]) * (lo[:, 1] if k & 2 else hi[:, 1]) * (lo[:, 2] if k & 1 else hi[:, 2])
                     for k in range(8)], 1)
    if s != 1:
        w = w / (s * s * s)
    w = torch.where(idx_kn.t() == -1, torch.zeros_like(w), w)
    tot = torch.zeros_like(w[:, 0])
    for k in range(8):
        tot = tot + w[:, k]
    return w / (tot + eps)[:, None]


def ti_weights_full(coords, idx_kn, scale):
    assert coords.dtype == torch.float32
    ref = _ti(coords[:, :3].double(), idx_kn, float(scale), EPS32, torch.floor)
    return ref, gamma(TI_ROUNDINGS) * ref


def ti_weights64(coords, idx_kn, scale):
    return ti_weights_full(coords, idx_kn, scale)[0]


# ---- fp32 evaluations: the honest ones and the wrong ones -----------------------------------------------------------------------

def pairwise_sum1(t):
    """sum over dim 1 in t's dtype, halves added level by level (a padding zero adds exactly)"""
    while t.shape[1] > 1:
        if t.shape[1] % 2:
            t = torch.cat([t, torch.zeros_like(t[:, :1])], 1)
        t = t[:, 0::2] + t[:, 1::2]
    return t[:, 0]


def segment_fp32(src, erow, ew, seg, mean, counts, dtype, order='asc', variant=''):
    """the segment form in fp32 arithmetic, the sum in ``order`` (asc / desc / pair), one rounding to ``dtype`` at the end.
    ``variant`` names a WRONG formulation."""
    dest, lens, pos = _segments(seg)
    e, nv, c = dest.numel(), lens.numel(), src.shape[1]
    x = src.float()[erow[:e].long()]
    w = None if ew is None else ew.float()[:e]
    if w is not None and variant == 'weights_rounded':
        w = w.to(dtype).float()
    if w is not None and variant == 'neighbour_weight':
        w = torch.roll(w, -1)
    d = (lens if counts is None else counts.long()).float()
    if variant == 'div_m_plus_1':
        d = d + 1
    if mean and variant != 'sum_not_mean':
        t = x / d[dest][:, None]
    else:
        t = x if w is None else x * w[:, None]
    if variant == 'tail_dropped':
        t = torch.where((pos < lens[dest] // 4 * 4)[:, None], t, torch.zeros_like(t))
    m = max(int(lens.max()) if nv else 0, 1)
    pad = torch.zeros(nv, m, c, dtype=torch.float32)
    pad[dest, (lens[dest] - 1 - pos) if order == 'desc' else pos] = t
    if order == 'pair':
        out = pairwise_sum1(pad)
    else:
        # one entry of every segment per step; the segments by descending length, so that step j touches only those longer than j
        # (the others would add a padding zero, which changes nothing)
        by_len = torch.argsort(lens, descending=True, stable=True)
        pad, sorted_lens = pad[by_len], lens[by_len]
        acc = torch.zeros(nv, c, dtype=torch.float32)
        for j in range(m):
            k = int((sorted_lens > j).sum())
            acc[:k] = acc[:k] + pad[:k, j]
            if variant == 'round_each_add':
                acc[:k] = acc[:k].to(dtype).float()
        out = torch.empty_like(acc)
        out[by_len] = acc
    if mean:
        out = torch.where((d > 0)[:, None], out, torch.zeros_like(out))
    return out.to(dtype)


def ti_weights_fp32(coords, idx_kn, scale, variant=''):
    return _ti(coords[:, :3].float(), idx_kn, float(scale), 0.0 if variant == 'no_eps' else torch.tensor(1e-8),
               torch.trunc if variant == 'truncf' else torch.floor)


# ---- the input sets (shared by the host test and the GPU test; fixed seeds) -----------------------------------------------------

V1_LENS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 0, 63, 64, 65, 130, 1000, 0)
VOX_LAYOUTS = ('V1s', 'V1r', 'V2', 'V3')
DEVOX_N, DEVOX_NV, HUB = 257, 50, 7
WKINDS = ('tri', 'signed')
KINDS = ('randn', 'mean1e3', 'wide', 'nan_row')
WIDTHS32 = (1, 3, 4, 6, 12, 17, 20, 32, 96, 256)
WIDTHS16 = (4, 12, 16, 20, 48, 128)
CMODES = ('twice',)            # counts that are NOT the histogram (part of the counts cases); 'hist' is the default, 'half' the
#                                overflow case's
TI_SCALES = (1, 2, 16)


def widths(dtype, vec4_only=False):
    ws = WIDTHS32 if dtype == torch.float32 else WIDTHS16
    return tuple(c for c in ws if c % 4 == 0) if vec4_only else ws


@functools.lru_cache(maxsize=None)
def vox_layout(name):
    """(idx int32 [n], nv).  V1: segments of V1_LENS points (first, last and one middle voxel empty) + 40 points with idx -1 + 10
    with idx in {nv, nv + 5}, sorted by voxel (V1s) or shuffled (V1r); V2: one voxel of 37 points; V3: 900 random points, 300 voxels"""
    if name in ('V1s', 'V1r'):
        nv = len(V1_LENS)
        idx = torch.cat([torch.full((40,), -1)] + [torch.full((m,), v) for v, m in enumerate(V1_LENS)]
                        + [torch.tensor([nv, nv + 5] * 5).sort().values]).int()
        if name == 'V1r':
            idx = idx[torch.randperm(idx.numel(), generator=torch.Generator().manual_seed(31))]
        return idx.contiguous(), nv
    if name == 'V2':
        return torch.zeros(37, dtype=torch.int32), 1
    if name == 'V3':
        return torch.randint(0, 300, (900,), generator=torch.Generator().manual_seed(32)).int(), 300
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def vox_counts(name, cmode='hist'):
    """int32 [nv]: 'hist' the histogram of the index; 'twice' twice it, and 0 at the first voxel that has at least two points;
    'half' max(1, hist // 2) (the overflow case: the mean of rows of 6e4 leaves fp16's range)"""
    idx, nv = vox_layout(name)
    i = idx.long()
    hist = torch.bincount(i[(i >= 0) & (i < nv)], minlength=nv)
    if cmode == 'twice':
        hist = hist * 2
        hist[int((hist >= 4).nonzero()[0])] = 0
    elif cmode == 'half':
        hist = (hist // 2).clamp(min=1)
    elif cmode != 'hist':
        raise ValueError(cmode)
    return hist.int()


@functools.lru_cache(maxsize=None)
def devox_layout(wkind):
    """(idx8 int32 [257, 8], w8 fp32 [257, 8]), nv = 50.  Rows 0-4: no corner; 5-9: exactly one (the hub); 10-14: voxel 3 at
    corners 0 and 1; corner 7 of every other row is the hub voxel 7 (a segment of ~250 entries in the backward); ~30 % of the
    other corners missing.  Weights: 'tri' trilinear (>= 0, sum 1), 'signed' rand - 0.3; 20 % of them exactly 0."""
    g = torch.Generator().manual_seed(4100)
    n = DEVOX_N
    idx = torch.randint(0, DEVOX_NV, (n, 8), generator=g)
    idx[torch.rand(n, 8, generator=g) < 0.3] = -1
    idx[:, 7] = HUB
    idx[:5] = -1
    idx[5:10, :7] = -1
    idx[10:15, :2] = 3
    g = torch.Generator().manual_seed(4200 + WKINDS.index(wkind))
    if wkind == 'tri':
        fr = torch.rand(n, 3, generator=g)
        w = torch.stack([(fr[:, 0] if k & 4 else 1 - fr[:, 0]) * (fr[:, 1] if k & 2 else 1 - fr[:, 1])
                         * (fr[:, 2] if k & 1 else 1 - fr[:, 2]) for k in range(8)], 1)
    else:
        w = torch.rand(n, 8, generator=g) - 0.3
    w[torch.rand(n, 8, generator=g) < 0.2] = 0.0
    return idx.int().contiguous(), w.float().contiguous()


def rows(kind, n, c, dtype, seed):
    """[n, c] of ``dtype`` (rounded to it): randn; mean1e3 (+1000); wide (per-row scale 10^U(-6, 4): where a max-relative norm is
    blind); nan_row (rows n // 2 and n - 1 NaN); overflow (uniform in +-6e4: weighted sums leave fp16's range); overflow_mean (6e4
    (0.6 + 0.4 rand), one sign per column: the mean with halved counts leaves it)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, generator=g)
    if kind == 'mean1e3':
        x = x + 1e3
    elif kind == 'wide':
        x = x * 10.0 ** (torch.rand(n, 1, generator=g) * 10.0 - 6.0)
    elif kind == 'nan_row':
        x[n // 2] = float('nan')
        x[n - 1] = float('nan')
    elif kind == 'overflow':
        x = (torch.rand(n, c, generator=g) * 2 - 1) * 6e4
    elif kind == 'overflow_mean':
        x = 6e4 * (0.6 + 0.4 * torch.rand(n, c, generator=g)) * torch.sign(torch.randn(1, c, generator=g))
    elif kind != 'randn':
        raise ValueError(kind)
    return x.to(dtype)


OVERFLOW_MAX_WIDTH = 20


def kinds(dtype, c):
    """the row values a case of width c runs on: 'overflow' for fp16 rows only, and up to 20 channels (its weighted sums are spread
    evenly over +-1e5, so about one result in 2500 lies within its bound of fp16's edge: a few thousand results leave seeds
    without such an element to choose from, 257 x 128 do not)"""
    return KINDS + (('overflow',) if dtype == torch.float16 and c <= OVERFLOW_MAX_WIDTH else ())


def _seed(*parts):
    s = 0
    for p in parts:
        for ch in str(p):
            s = (s * 131 + ord(ch)) % 1000003
    return s


def _pick(build, dtype):
    """the first of the seeds 0, 1, ... whose case has no straddling reference"""
    for k in range(64):
        case = build(k)
        if not any(straddles(case[r], case[b], dtype) for r, b in case['pairs']):
            return case
    raise RuntimeError('no seed without a reference at the edge of fp16')


@functools.lru_cache(maxsize=None)
def vox_case(lay, c, kind, dtype, cmode='hist'):
    """one voxelize case, computed once and shared (read-only): inputs, the entry list, and (reference, bound) of the scatter-mean
    ('mean'), its backward ('bwd') and the plain segment sum over the same entries ('sum')"""
    idx, nv = vox_layout(lay)
    counts = vox_counts(lay, 'half' if kind == 'overflow' else cmode)
    order, seg = csr(idx, nv)
    n = idx.numel()
    xkind = 'overflow_mean' if kind == 'overflow' else kind

    def build(k):
        s = _seed(lay, c, kind, cmode) + 7919 * k
        case = {'idx': idx, 'nv': nv, 'counts': counts, 'order': order, 'seg': seg, 'x': rows(xkind, n, c, dtype, s),
                'g': rows('randn' if kind == 'overflow' else kind, nv, c, dtype, s + 1)}
        for name, (ref, err) in (('mean', segment_full(case['x'], order, None, seg, True, counts)),
                                 ('bwd', voxelize_bwd_full(case['g'], idx, counts)),
                                 ('sum', segment_full(case['x'], order, None, seg))):
            case[name], case[name + '_b'] = ref, stored(err, ref, dtype)
        case['pairs'] = (('mean', 'mean_b'), ('bwd', 'bwd_b'), ('sum', 'sum_b'))
        return case
    return _pick(build, dtype)


@functools.lru_cache(maxsize=None)
def devox_case(wkind, c, kind, dtype):
    """one devoxelize case: inputs, the backward's entry list, (reference, bound) of the forward ('fwd') and the backward ('bwd')"""
    idx8, w8 = devox_layout(wkind)
    plan = devoxelize_plan(idx8, w8, DEVOX_NV)

    def build(k):
        s = _seed(wkind, c, kind) + 7919 * k
        case = {'idx8': idx8, 'w8': w8, 'nv': DEVOX_NV, 'plan': plan, 'f': rows(kind, DEVOX_NV, c, dtype, s),
                'g': rows(kind, DEVOX_N, c, dtype, s + 1)}
        for name, (ref, err) in (('fwd', devoxelize_full(case['f'], idx8, w8)), ('bwd', segment_full(case['g'], *plan))):
            case[name], case[name + '_b'] = ref, stored(err, ref, dtype)
        case['pairs'] = (('fwd', 'fwd_b'), ('bwd', 'bwd_b'))
        return case
    return _pick(build, dtype)


@functools.lru_cache(maxsize=None)
def ti_case(scale):
    """300 points in cells of edge ``scale`` (a power of two), negative coordinates included: 0-29 exactly on cell corners, 30-59 on
    a face; rows 0-99 all corners present, 100-199 corners 1, 4, 6 missing, 200-219 all 8 missing, the rest ~30 % missing"""
    g = torch.Generator().manual_seed(5100 + scale)
    n = 300
    p = (torch.rand(n, 3, generator=g) * 40 - 20) * scale
    p[:30] = torch.floor(p[:30] / scale) * scale
    p[30:60, 0] = torch.floor(p[30:60, 0] / scale) * scale
    coords = torch.cat([p, torch.randint(0, 2, (n, 1), generator=g).float()], 1).float().contiguous()
    idx = torch.randint(0, 1000, (8, n), generator=g)
    idx[:, 220:][torch.rand(8, n - 220, generator=g) < 0.3] = -1
    idx[:, 100:200][[1, 4, 6]] = -1
    idx[:, 200:220] = -1
    ref, err = ti_weights_full(coords, idx, scale)
    return {'coords': coords, 'idx_kn': idx.contiguous(), 'scale': scale, 'ref': ref, 'bound': err}


# the formulations the bound has to reject: name -> (form, variant, the input set it is rejected on)
#   form 'vox': the scatter-mean of vox_case(lay, c, kind, dtype); 'devox_bwd' / 'devox_fwd': of devox_case(wkind, c, kind, dtype);
#   'ti': ti_case(scale)
WRONG = {
    'the tail after the last multiple of 4 entries dropped': ('vox', 'tail_dropped', ('V1s', 4, 'randn', 'f32')),
    'the sum rounded to bf16 after every addition': ('vox', 'round_each_add', ('V1s', 16, 'mean1e3', 'bf16')),
    'the sum rounded to fp16 after every addition': ('vox', 'round_each_add', ('V1r', 16, 'mean1e3', 'f16')),
    'weights rounded to the row type': ('devox_bwd', 'weights_rounded', ('tri', 16, 'randn', 'f16')),
    "the neighbouring entry's weight": ('devox_bwd', 'neighbour_weight', ('signed', 4, 'randn', 'f32')),
    'division by m + 1': ('vox', 'div_m_plus_1', ('V1s', 4, 'mean1e3', 'f32')),
    'the sum instead of the mean': ('vox', 'sum_not_mean', ('V3', 12, 'randn', 'f32')),
    'a corner with idx = -1 read as row 0': ('devox_fwd', 'missing_as_row0', ('signed', 4, 'randn', 'f32')),
    'w8 read as [8, n]': ('devox_fwd', 'w8_transposed', ('tri', 12, 'randn', 'f32')),
    'ti_weights without the + 1e-8': ('ti', 'no_eps', (1,)),
    'ti_weights with truncf instead of floorf': ('ti', 'truncf', (2,)),
}


def evaluate(form, where, order='asc', variant=''):
    """(result of the fp32 evaluation, reference, bound, dtype) of one form on one named input set"""
    if form == 'ti':
        case = ti_case(*where)
        return ti_weights_fp32(case['coords'], case['idx_kn'], case['scale'], variant), case['ref'], case['bound'], torch.float32
    a, c, kind, dt = where
    dtype = DTYPES[dt]
    if form == 'vox':
        case = vox_case(a, c, kind, dtype)
        return (segment_fp32(case['x'], case['order'], None, case['seg'], True, case['counts'], dtype, order, variant),
                case['mean'], case['mean_b'], dtype)
    case = devox_case(a, c, kind, dtype)
    if form == 'devox_bwd':
        return segment_fp32(case['g'], *case['plan'], False, None, dtype, order, variant), case['bwd'], case['bwd_b'], dtype
    if form == 'devox_fwd':
        erow, ew, seg = devoxelize_fwd_plan(case['idx8'], case['w8'], variant)
        return segment_fp32(case['f'], erow, ew, seg, False, None, dtype, order), case['fwd'], case['fwd_b'], dtype
    raise ValueError(form)
