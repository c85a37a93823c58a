"""float64 reference of the pair-list weight gradient (u2mkd_conv_wgrad_pairs and its _bf16 / _f16 forms) on SYNTHETIC
PAIR LISTS, and the bound the kernels are held to (test helper; plain torch, CPU or GPU tensors).

The kernels take a pool of rows ``a [n, ca]``, ``b [n, cb]``, a pair list ``pairs`` int32 [P, 2] grouped by offset with
``counts[k]`` pairs in offset k, and ``swap``: operand a is gathered through pair column 0 and b through column 1, the other
way round when ``swap`` is set (ConvolutionFunction passes it for transposed convolutions).  They return

    dW[k] = sum over the pairs (i, j) of offset k of a[i]^T b[j]                [K, ca, cb]

``wgrad_f64`` evaluates that sum in float64 and, next to it, ``mag`` = the same sum over |a|, |b|: the scale every rounding
error of the sum is relative to, however the terms cancel.

THE BOUND.  Elementwise, per offset k,

    |kernel - dW64| <= bound(mag, T, r) = mag * (T + 4 * max(r[k], 2^-24))

``r[k]`` is not a constant.  It is MEASURED on the inputs of the case at hand by ``honest_fp32``: the same sum in plain fp32,
32 pairs multiplied at a time (one rounding per product), the products added in pair order (one rounding per addition); r[k]
is its largest |error| / mag over the elements of offset k.  That is what fp32 accumulation alone costs on these inputs: an
offset of one pair has r = 2^-25 or less (one product rounding), an offset of 9000 pairs of rows whose magnitudes differ by
1e20 has r around 2^-22.  The factor 4 covers a summation order other than the honest one -- the kernels cut an offset into
chunks of plan[1] pairs, keep one fp32 slab per chunk (or per run of merged chunks) and add the slabs 16 lanes wide; two
honest orders were seen to differ by 4.1x on one input, and tests/test_gpu_conv_f16x2.py uses the same factor between two
accuracy classes.  The floor 2^-24 is one fp32 rounding of the result, which every evaluation that returns fp32 may have.

``T`` is the part of the error that does not come from accumulating in fp32 but from the arithmetic of the products:

  T = 0 (``T_EXACT``)   the f32-MFMA kernel (conv_wgrad_pairs_kernel, v_mfma_f32_16x16x4_f32: fp32 products, fp32 sums --
                        the honest evaluation with fewer roundings), and bf16 / fp16 rows in every kernel: the product of two
                        values of 8 (11) significant bits has 16 (22) and is exact in fp32, the rows are widened exactly, and
                        only sums remain.
  T = 2^-21 (1 + 2^-9)  (``T_X3``) fp32 rows in conv_wgrad_x3_kernel.  Every fp32 x is split by TRUNCATION into three bf16,
                        x = h + m + l exactly: h holds the leading 8 significant bits of x (binary exponent e), so
                        |x - h| < 2^(e-7); m holds the next 8 bits that are present, so |m| < 2^(e-7) <= 2^-7 |x| and
                        |x - h - m| < 2^-7 * 2^(e-8) = 2^(e-15); l is that rest, at most 8 significant bits, exact in a bf16:
                        |l| < 2^-15 |x|.  Of the nine partial products of (ha + ma + la)(hb + mb + lb) the kernel adds six and
                        DROPS ma lb, la mb and la lb:
                            |dropped| < (2^-7 * 2^-15 + 2^-15 * 2^-7 + 2^-15 * 2^-15) |a||b| = 2^-21 (1 + 2^-9) |a||b|.
                        Truncation gives h, m and l the sign of x, so every dropped product has the sign of a b: over terms
                        of one sign the dropped parts add up and do not average out against mag, hence a term of its own
                        and not a share of the factor 4.  The six products kept are exact in fp32 (8 x 8 bits); their sums
                        are accumulation and belong to r.
                        (The issue that asked for this helper proposed T = 2^-20 (1 + 2^-8) from |l| < 2^-14 |x|.  The split
                        leaves 24 - 16 = 8 bits to l, which start 16 binary places below the leading bit of x, so
                        |l| < 2^-15 |x| and the dropped part is half of that; the tighter figure is used.  conv_wgrad_x3.hip
                        records a largest error of 2^-20.1 * mag for this kernel on a real scene with rows of 1e-10..1e10: T
                        plus the accumulation of some 10^4 pairs per offset, for which r is near 2^-22 -- not T alone.)

FP16 SUBNORMALS ON THE FP16 MATRIX INSTRUCTION (``nominal_fp16``).  fp16 rows in conv_wgrad_x3_kernel are multiplied by
v_mfma_f32_16x16x32_f16, and T = 0 holds there with ONE correction that the MI355X forced: the instruction aligns the
products of a block to the largest NOMINAL exponent -- the exponent FIELDS of the operands added, and a subnormal fp16 has the
field of the smallest normal, 2^-14, whatever its leading bit -- and keeps 24 bits below it.  Seen on the first run of the GPU
test (fp16, 64 x 64, pattern heavy, spread rows, an offset of two pairs): the terms (427 * 2^-24) * (1352 * 2^-17) and
(137 * 2^-5) * (5 * 2^-24) sum to 3383064 * 2^-41; the kernel returned 3383040 * 2^-41, the first product cut off below 2^-36 =
2^(2 - 14 - 24): 24 bits below the second product's nominal exponent 2 + (-14), although that product is only 2^-19.6.  The
error, 2^-17.1 of mag, is 2^-24.5 of the nominal magnitude.  One subnormal operand times a normal one alone is exact, and so
are two normal products 23 binary places apart (both measured).  So for fp16 rows on that kernel the bound is taken relative
to ``mag`` of the NOMINAL rows, every nonzero |x| < 2^-14 raised to 2^-14: the same mag wherever no operand is subnormal, and
nowhere a wider coefficient.  In absolute terms this costs 2^-24 * 2^-14 |a| per term: what fp16 storage loses on such a value
anyway.  The f32-MFMA kernel widens fp16 rows exactly to normal fp32 and keeps the plain mag; bf16 has fp32's exponent range and
no case of the tests reaches its subnormals.

WHAT THE BOUND CAN SEE.  ``x3_eval`` restates the bf16x3 product (the planes by the same bit operations, the six products in
the kernel's order, an exact sum per 32 pairs rounded into an fp32 accumulator) and takes a list of products to leave out;
``DEGRADED`` names five wrong evaluations.  tests/test_host_wgrad_bound.py requires on the inputs of the GPU test that the
honest evaluations pass the bound and every degraded one fails it on the ``rows`` spread, and on the ``unit`` spread in the
offsets of at most 64 pairs.  On ``randn`` data in an offset of thousands of pairs a lost m * m product (2^-16 of single
terms whose signs vary) sits below the fp32 accumulation of the sum itself, and no bound that an honest fp32 sum passes can
see it there; that is why every GPU case has small offsets and the ``rows`` spread."""
import torch

T_EXACT = 0.0
T_X3 = 2.0 ** -21 * (1.0 + 2.0 ** -9)
FLOOR = 2.0 ** -24
MARGIN = 4.0
POOL = 4096

# the six partial products conv_wgrad_x3_kernel adds, in its order (low order first); 0 = h, 1 = m, 2 = l; (plane of a, of b)
X3_PRODUCTS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))


# ---- the pair list ---------------------------------------------------------------------------------------------------------

def columns(pairs, swap):
    """(indices into a, indices into b) of every pair, int64"""
    p = pairs.long()
    return (p[:, 1], p[:, 0]) if swap else (p[:, 0], p[:, 1])


def ranges(counts):
    out, lo = [], 0
    for c in counts:
        out.append((lo, lo + int(c)))
        lo += int(c)
    return out


# ---- evaluations -----------------------------------------------------------------------------------------------------------

def wgrad_f64(a, b, pairs, counts, swap):
    """(dW, mag) float64 [K, ca, cb]: dW[k] = sum over offset k's pairs of a[pa]^T b[pb]; mag the same over |a|, |b|"""
    ia, ib = columns(pairs, swap)
    ad, bd = a.double(), b.double()
    k, ca, cb = len(counts), a.shape[1], b.shape[1]
    dw = torch.zeros(k, ca, cb, dtype=torch.float64, device=a.device)
    mag = torch.zeros_like(dw)
    for kk, (lo, hi) in enumerate(ranges(counts)):
        if hi > lo:
            ra, rb = ad[ia[lo:hi]], bd[ib[lo:hi]]
            dw[kk] = ra.t() @ rb
            mag[kk] = ra.abs().t() @ rb.abs()
    return dw, mag


def nominal_fp16(x):
    """|x| as v_mfma_f32_16x16x32_f16 aligns it: a nonzero fp16 below the smallest normal counts as 2^-14 (docstring above)"""
    m = x.double().abs()
    return torch.where((m > 0) & (m < 2.0 ** -14), torch.full_like(m, 2.0 ** -14), m)


def honest_fp32(a, b, pairs, counts, swap, skip_last=False):
    """The sum in plain fp32: 32 pairs multiplied at a time, their products added in pair order.  fp32 [K, ca, cb].
    (skip_last: a degraded form -- the last pair of every offset is left out)"""
    ia, ib = columns(pairs, swap)
    af, bf = a.float(), b.float()
    k, ca, cb = len(counts), a.shape[1], b.shape[1]
    dw = torch.zeros(k, ca, cb, dtype=torch.float32, device=a.device)
    for kk, (lo, hi) in enumerate(ranges(counts)):
        if skip_last:
            hi = max(hi - 1, lo)
        acc = dw[kk]
        for p0 in range(lo, hi, 32):
            p1 = min(p0 + 32, hi)
            prod = af[ia[p0:p1]][:, :, None] * bf[ib[p0:p1]][:, None, :]
            for i in range(p1 - p0):
                acc += prod[i]
    return dw


def slab_order_fp32(a, b, pairs, counts, swap, chunk=128):
    """Another honest fp32 order, the one of the kernels at merge 1: one honest partial sum (a slab) per ``chunk`` pairs, lane g
    of 16 adds slabs g, g + 16, ... in order, the 16 lanes are added in order.  fp32 [K, ca, cb]."""
    k = len(counts)
    dw = torch.zeros(k, a.shape[1], b.shape[1], dtype=torch.float32, device=a.device)
    for kk, (lo, hi) in enumerate(ranges(counts)):
        cuts = list(range(lo, hi, chunk))
        if not cuts:
            continue
        slabs = honest_fp32(a, b, pairs[lo:hi], [min(chunk, hi - c) for c in cuts], swap)
        lanes = torch.zeros(16, *dw.shape[1:], dtype=torch.float32, device=a.device)
        for j in range(len(cuts)):
            lanes[j % 16] += slabs[j]
        for g in range(16):
            dw[kk] += lanes[g]
    return dw


def split3(x):
    """fp32 x -> (h, m, l), each a bf16 held in an fp32: wx_split4 of conv_wgrad_x3.hip, bit operation for bit operation.
    x = h + m + l exactly for |x| >= 2^-110 (below that the last bits of l lie under the smallest bf16 denormal, 2^-133, and
    are cut off; no case of the tests goes there)."""
    x = x.float().contiguous()
    keep = -65536       # 0xffff0000
    h = (x.view(torch.int32) & keep).view(torch.float32)
    r1 = x - h
    m = (r1.view(torch.int32) & keep).view(torch.float32)
    l = ((r1 - m).view(torch.int32) & keep).view(torch.float32)
    return h, m, l


def x3_eval(a, b, pairs, counts, swap, drop=()):
    """The bf16x3 product of conv_wgrad_x3_kernel: per 32 pairs the partial products of X3_PRODUCTS in order, each the exact
    sum of its 32 terms (float64: a term has 16 significant bits) rounded into the fp32 accumulator.  ``drop``: products to
    leave out (degraded forms).  fp32 [K, ca, cb]."""
    ia, ib = columns(pairs, swap)
    pa = [p.double() for p in split3(a)]
    pb = [p.double() for p in split3(b)]
    k, ca, cb = len(counts), a.shape[1], b.shape[1]
    dw = torch.zeros(k, ca, cb, dtype=torch.float32, device=a.device)
    todo = [pq for pq in X3_PRODUCTS if pq not in drop]
    for kk, (lo, hi) in enumerate(ranges(counts)):
        acc = dw[kk]
        for p0 in range(lo, hi, 32):
            xa, xb = ia[p0:min(p0 + 32, hi)], ib[p0:min(p0 + 32, hi)]
            for p, q in todo:
                acc.copy_((acc.double() + pa[p][xa].t() @ pb[q][xb]).float())
    return dw


# the wrong evaluations the bound has to reject: name -> f(a, b, pairs, counts, swap) -> fp32 [K, ca, cb]
DEGRADED = {
    'x3 without m*m': lambda a, b, p, c, s: x3_eval(a, b, p, c, s, drop=((1, 1),)),
    'x3 without m*m and l*h': lambda a, b, p, c, s: x3_eval(a, b, p, c, s, drop=((1, 1), (2, 0))),
    'one operand rounded to bf16': lambda a, b, p, c, s: honest_fp32(a.bfloat16().float(), b, p, c, s),
    'last pair of every offset skipped': lambda a, b, p, c, s: honest_fp32(a, b, p, c, s, skip_last=True),
    'pair columns not swapped': lambda a, b, p, c, s: honest_fp32(a, b, p, c, 0),       # (differs from the truth when s = 1)
}


# ---- the bound -------------------------------------------------------------------------------------------------------------

def rel_err(got, dw, mag):
    """largest |got - dw| / mag per offset, float64 [K] (0 for an offset without pairs; inf where mag = 0 and got != dw)"""
    err = (got.double() - dw).abs()
    ratio = torch.where(mag > 0, err / mag.clamp(min=1e-300), torch.where(err > 0, float('inf'), 0.0).to(err.dtype))
    return ratio.flatten(1).amax(dim=1)


def bound(mag, T, r):
    """mag * (T + 4 * max(r, 2^-24)); r per offset ([K]) or one number"""
    r = torch.as_tensor(r, dtype=torch.float64, device=mag.device)
    coef = T + MARGIN * r.clamp(min=FLOOR)
    return mag * (coef[:, None, None] if coef.dim() else coef)


def check(got, dw, mag, T, r):
    """(passes, largest err / bound, largest err / mag) of ``got`` against the bound; an element with mag = 0 must be exact"""
    err = (got.double() - dw).abs()
    bd = bound(mag, T, r)
    over = torch.where(bd > 0, err / bd.clamp(min=1e-300), torch.where(err > 0, float('inf'), 0.0).to(err.dtype))
    return bool((err <= bd).all()), float(over.max()), float(rel_err(got, dw, mag).max())


# ---- the cases (shared by the host test and the GPU test) ------------------------------------------------------------------

_RAGGED = [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257, 0, 0, 1000, 5, 3, 7, 11, 13, 17, 19, 23, 29, 37]
_HEAVY = [(i * 7) % 4 for i in range(27)]

# pattern -> (counts per offset, n_rows handed to the plan, swap)
PATTERNS = {
    # with n_rows = 4096 the plan's chunk is 128 pairs: offsets of 0, 1, one step, a step +- 1, a chunk +- 1, chunk tails
    'ragged': (_RAGGED, 4096, 0),
    'ragged8': ([0, 1, 33, 130, 64, 0, 700, 17], 4096, 0),
    'ragged8-swap': ([0, 1, 33, 130, 64, 0, 700, 17], 4096, 1),
    # one offset of more than 64 chunks (9000 / 128 = 71 slabs at merge 1), the others at most 3 pairs
    'heavy': (_HEAVY[:13] + [9000] + _HEAVY[14:], 9000, 0),
    # ... of more than 2 * 64 chunks: more than 64 LIVE slabs at merge 2
    'heavy-merged': (_HEAVY[:13] + [17000] + _HEAVY[14:], 9000, 0),
    'dense1': ([5000], 5000, 0),          # nn.Linear: identity pairs
    'empty': ([0] * 27, 4096, 0),
}
SPREADS = ('unit', 'rows', 'tiny')


def make_case(pattern, ca, cb, spread, dtype=torch.float32, seed=0):
    """CPU tensors of one case: a [n, ca], b [n, cb] of ``dtype`` (rounded to it), pairs int32 [max(P, 1), 2], counts, n_rows,
    swap.  The same generator on every machine: the host test calibrates on exactly what the GPU test runs."""
    counts, n_rows, swap = PATTERNS[pattern]
    g = torch.Generator().manual_seed(1000 * seed + 7 * ca + cb)
    n = max(POOL, n_rows if pattern == 'dense1' else 0)
    a, b = torch.randn(n, ca, generator=g), torch.randn(n, cb, generator=g)
    if spread == 'rows':        # every row its own power of ten, on both operands; a tenth of the rows all zero
        lo, hi = (-3, 4) if dtype == torch.float16 else (-10, 11)       # (fp16: inside its range)
        a = a * torch.pow(10.0, torch.randint(lo, hi, (n, 1), generator=g).float())
        b = b * torch.pow(10.0, torch.randint(lo, hi, (n, 1), generator=g).float())
        a[torch.rand(n, generator=g) < 0.1] = 0.0
        b[torch.rand(n, generator=g) < 0.1] = 0.0
    elif spread == 'tiny':      # gradients late in training
        a, b = a * 1e-20, b * 1e-10
    elif spread != 'unit':
        raise ValueError(spread)
    p = sum(counts)
    if pattern == 'dense1':
        pairs = torch.arange(p, dtype=torch.int32)[:, None].repeat(1, 2)
    else:
        pairs = torch.randint(0, n, (max(p, 1), 2), generator=g, dtype=torch.int32)
    return {'a': a.to(dtype), 'b': b.to(dtype), 'pairs': pairs.contiguous(), 'counts': list(counts), 'n_rows': n_rows,
            'swap': swap, 'k': len(counts)}


# ---- the dispatch of wgrad_pairs_impl (csrc/conv.hip), restated --------------------------------------------------------------

def family(ca, cb, dtype, f32_arith=False):
    """('x3', merge) or ('mfma', (wm, wn, pairs per step)): the kernel a shape and row type is launched on"""
    if ca % 64 == 0 and cb % 64 == 0 and (dtype != torch.float32 or not f32_arith):
        tiles = (ca // 64) * (cb // 64)
        return 'x3', (6 if tiles >= 9 else 4 if tiles >= 4 else 2 if tiles >= 2 else 1)
    pick = lambda c: 1 if c <= 32 else 2 if c <= 64 else 3 if c <= 96 else 4
    wm, wn = pick(ca), pick(cb)
    return 'mfma', (wm, wn, 16 if max(wm, wn) >= 3 else 32)


def live_slabs(plan, k, merge):
    """per offset, the workgroup slots whose slab the kernel writes and wgrad_pairs_reduce_kernel reads: the offset's first
    slot and every later slot of it that is a multiple of ``merge`` (plan = the int32 list of u2mkd_wgrad_plan)"""
    wg = plan[3 + k:4 + 2 * k]
    return [[w for w in range(wg[i], wg[i + 1]) if w == wg[i] or w % merge == 0] for i in range(k)]
