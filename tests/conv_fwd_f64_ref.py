"""float64 reference of the sparse convolution's forward and input gradient on SYNTHETIC NEIGHBOUR TABLES, and the bounds
every kernel form is held to (test helper; plain torch, CPU or GPU tensors).

THE OPERATION.  A neighbour table ``nbr`` int32 [K, n_out] names, per offset k and output row j, the input row that feeds it
(-1: none).  A launch multiplies rows ``x`` [n_src, ca] by one [ca, cb] matrix per offset and sums per destination row.  Five
ROLES say which side of a pair is the destination and which matrix an offset takes, ``w`` = the layer's kernel [K, ., .]:

    'fwd'    out[j] = sum_k x[nbr[k][j]] @ w[k]                 the forward (tile kernels kflip 0, pair kernels swap 0)
    'flip'   out[j] = sum_k x[nbr[k][j]] @ w[K-1-k]^T           input gradient of a SYMMETRIC map on the forward table (kflip 1)
    'inv'    out[i] = sum_k sum_{j: nbr[k][j] = i} x[j] @ w[k]^T    input gradient of a strided map (pair kernels swap 1)
    'invT'   out[i] = sum_k sum_{j: nbr[k][j] = i} x[j] @ w[k]      the transposed convolution (pair kernels swap 1)
    'fwdT'   out[j] = sum_k x[nbr[k][j]] @ w[k]^T               input gradient of the transposed convolution (swap 0)

``conv_f64`` is the float64 evaluation of 'fwd' / 'flip' (moved here from tests/test_gpu_conv_f16x2.py, which imports it);
``conv_from_pairs_f64`` evaluates the two inverse roles from ``nbr`` ALONE -- never from nbr_inv, pos_in or anything else the
library built.  Both return ``mag``, the same sum over |x|, |w|: the scale every rounding error is relative to however the
terms cancel.  ``evaluate`` is the one loop under all of them and under every fp32 / emulated evaluation below.

THE BOUNDS (``bound``, ``check``), elementwise; an element with mag = 0 (a row without a neighbour) must be EXACT.
``A = mag * 4 * max(r, 2^-24)`` is the accumulation term of tests/wgrad_f64_ref.py (its MARGIN and FLOOR): ``r`` is MEASURED
per case as the largest err / mag of ``honest_fp32`` -- the same contraction in plain fp32, offset by offset in ascending order,
product by product, WITH THE ACCUMULATOR STRUCTURE OF THE FORM under test (``running``, see there) -- against float64 on the
same inputs; 4 covers another summation order (a second honest order, offsets descending, is held to the same bound by the host
test), 2^-24 is one rounding of the result.
(NOTES N22 records how r came to be measured this way.)

  'f16x2'  mag * 2^-20: the project's figure for the f16x2 arithmetic (tests/test_gpu_conv_f16x2.py), tile arith 4 and
           u2mkd_conv_forward_pairs_f16x2.
  'f32'    A: the f32-MFMA forms -- tile arith 1, conv_os2 / conv_os3 behind u2mkd_conv_forward_sorted, launch_conv_pairs<32|64>
           behind u2mkd_conv_forward_pairs -- and u2mkd_pairs_gather_sum over their rows: fp32 products, fp32 sums, the honest
           evaluation in another order.
  'x3'     mag * T_FWD + A: bf16x3, tile arith 2 (conv_tp.hip) and u2mkd_conv_forward_pairs_x3 (conv_px3.hip).
           T_FWD = 2^-23 (1.5 + 2^-9).  Both kernels add, per 32-channel step, the six partial products (weight plane x row
           plane) l h, h l, m m, m h, h m, h h and DROP m l, l m and l l: the SAME product list as the weight gradient
           (wgrad_f64_ref.X3_PRODUCTS drops ma lb, la mb, la lb).  T_X3 is not copied all the same, because the WEIGHT operand
           is split differently here: the gathered rows are split by truncation as there (x & 0xffff0000 twice: |m_x| < 2^-7
           |x|, |l_x| < 2^-15 |x|), but the weight fragments (weight_fragments_x3_kernel, split3 / px_split3) are split by
           ROUNDING to nearest: for w in [2^e, 2^(e+1)) h = bf16(w) is within half a unit of its 8-bit significand, |w - h| <=
           2^(e-8), so |m_w| <= 2^-8 |w|; unless w - h is exactly 2^(e-8) (then l = 0) its exponent is at most e - 9, and m =
           bf16(w - h) is within half a unit of ITS last place, 2^(e-17), so |l_w| <= 2^-17 |w| (the rest has at most 7
           significant bits and is exact in a bf16).  Hence
               |dropped| <= (2^-8 * 2^-15 + 2^-17 * 2^-7 + 2^-17 * 2^-15) |w||x| = 2^-23 (1 + 1/2 + 2^-9) |w||x|,
           three eighths of T_X3.  The six kept products are exact in fp32 (8 x 8 bits); their sums belong to A.  Rounded planes
           may differ in sign from w, so the dropped parts do not all add up as under truncation; the bound takes them as if
           they did.
  16-bit rows (bf16 / fp16 storage): the reference is float64 of the rows and weights AS ROUNDED to the row type (the weight
           fragments of arith 3 / 5 hold w rounded to nearest).  A product of two such values has 16 (22) significant bits and
           is exact in fp32, so only sums and the roundings of stored rows remain; u = 2^-8 (bf16: 8 significant bits) or 2^-11
           (fp16: 11) is the rounding unit to nearest, half a unit in the last place of a value at the bottom of its binade; s =
           half the smallest subnormal of the type (what a result below the normal range loses).
             'tile16'  (u2mkd_conv_forward_tiles_bf16 / _f16: the fp32 sum of the LDS tile is rounded ONCE at the store)
                       A + u (|ref| + A) + s
             'pair16'  (u2mkd_conv_forward_pairs_bf16 / _f16 + u2mkd_pairs_gather_sum_bf16 / _f16: every live offset's scratch
                       row y_k is the fp32 sum of that offset rounded to the row type, the gather-sum adds the y_k in fp32 and
                       rounds the sum):  E = A + u (part + A) + K s,  bound = E + u (|ref| + E) + s,
                       ``part`` = sum_k |ref_k|, the magnitudes of the per-offset partial results that are rounded.
           The bound is ONE-SIDED: an evaluation that keeps y in fp32 (the tile form's arithmetic) passes 'pair16' as well.
           fp16 operands below the smallest normal count at their NOMINAL exponent 2^-14 in ``mag``, as wgrad_f64_ref.nominal_fp16
           explains (the fp16 matrix instruction aligns products by exponent fields).
  epilogue (u2mkd_conv_forward_tiles_ep, u2mkd_pairs_gather_sum_ep: relu?(fma(conv, scale, shift) (+ res))): with ``emag`` =
           |scale| mag + |shift| + |res| of ``epilogue_f64`` and B the bound of the convolution under it,
               |scale| B + ops * 2^-24 * (emag + |scale| B),   ops = 1 (the fma) + 1 (the residual add, where there is one).
           ReLU adds nothing: max(., 0) is exact and moves a value no further from the truth than it was.

WHAT THE BOUNDS CAN SEE.  ``DEGRADED`` names wrong CPU evaluations; tests/test_host_conv_fwd_bound.py requires on the inputs
of the GPU test that every honest evaluation stays at or below HALF its bound and every degraded one that should fail does.
No figure here is fitted to what a kernel returns."""
import torch

from wgrad_f64_ref import FLOOR, MARGIN, nominal_fp16, split3

T_FWD = 2.0 ** -23 * (1.5 + 2.0 ** -9)
T_F16X2 = 2.0 ** -20
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SUBNORMAL = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}

# the six partial products conv_tp_kernel / conv_px3_kernel add per 32-channel step, in their order (low order first);
# 0 = h, 1 = m, 2 = l; (plane of the weight, plane of the row)
X3_PRODUCTS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))

ROLES = ('fwd', 'flip', 'inv', 'invT', 'fwdT')
ON_OUTPUTS, TRANSPOSED = ('fwd', 'flip', 'fwdT'), ('flip', 'inv', 'fwdT')          # destination = the map's outputs; B_k = a transposed weight


# ---- the contraction -------------------------------------------------------------------------------------------------------

def n_dst(nbr, n_in, role):
    return nbr.shape[1] if role in ON_OUTPUTS else n_in


def shape_of(w, role):
    """(ca, cb) of the launch: channels of x, channels of out"""
    return (w.shape[2], w.shape[1]) if role in TRANSPOSED else (w.shape[1], w.shape[2])


def offsets(nbr, role, order=None):
    """per offset, in ``order`` (default ascending): (k, dst rows, src rows, index of the weight, weight transposed)"""
    k_total = nbr.shape[0]
    for k in (range(k_total) if order is None else order):
        idx = nbr[k].long()
        j = torch.nonzero(idx >= 0)[:, 0]
        i = idx[j]
        if role == 'fwd':
            yield k, j, i, k, False
        elif role == 'flip':
            yield k, j, i, k_total - 1 - k, True
        elif role == 'inv':
            yield k, i, j, k, True
        elif role == 'invT':
            yield k, i, j, k, False
        elif role == 'fwdT':
            yield k, j, i, k, True
        else:
            raise ValueError(role)


def evaluate(x, w, nbr, n_in, role, mul, dtype, order=None, post=None):
    """out[dst] (+)= post(mul(x[src], B_k)) per offset, accumulated in ``dtype``.  Every offset's map is injective, so a
    destination row takes at most one term per offset and index_add_ is one addition per element: the order is the offsets'."""
    out = torch.zeros(n_dst(nbr, n_in, role), shape_of(w, role)[1], dtype=dtype, device=x.device)
    for k, dst, src, kw, tr in offsets(nbr, role, order):
        if len(dst):
            t = mul(x[src], w[kw].t() if tr else w[kw], k)
            out.index_add_(0, dst, (post(t) if post else t).to(dtype))
    return out


def _f64(x, w, nbr, n_in, role, nominal=False, parts=False):
    xd, wd = x.double(), w.double()
    out = evaluate(xd, wd, nbr, n_in, role, lambda a, b, k: a @ b, torch.float64)
    xa, wa = (nominal_fp16(x), nominal_fp16(w)) if nominal else (xd.abs(), wd.abs())
    mag = evaluate(xa, wa, nbr, n_in, role, lambda a, b, k: a @ b, torch.float64)
    if parts:
        return out, mag, evaluate(xd, wd, nbr, n_in, role, lambda a, b, k: (a @ b).abs(), torch.float64)
    return out, mag


def conv_f64(x, w, nbr, flip):
    """out[j] = sum_k x[nbr[k][j]] @ B_k in float64; forward: B_k = w[k] ([cin, cout]); input gradient (flip): the transposed
    weights of the mirrored offset.  Also returns sum_k |x| @ |B_k| (the scale an error bound is relative to)."""
    k, n = nbr.shape
    xd, wd = x.double(), w.double()
    cols = w.shape[1] if flip else w.shape[2]
    out = torch.zeros(n, cols, dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(out)
    for kk in range(k):
        idx = nbr[kk].long()
        ok = idx >= 0
        rows = xd[idx.clamp(min=0)] * ok[:, None]
        b = wd[k - 1 - kk].t() if flip else wd[kk]
        out += rows @ b
        mag += rows.abs() @ b.abs()
    return out, mag


def conv_from_pairs_f64(x, w, nbr, n_in, transpose_w):
    """The INVERSE role in float64, from ``nbr`` alone: out[i] = sum over the pairs (i = nbr[k][j], j) of x[j] @ (w[k]^T if
    transpose_w else w[k]) -- rows of the map's inputs, summed over the outputs they feed.  transpose_w: the input gradient of a
    strided map; else the transposed convolution.  (out, mag) float64 [n_in, .]"""
    return _f64(x, w, nbr, n_in, 'inv' if transpose_w else 'invT')


def reference(x, w, nbr, n_in, role, nominal=False):
    """(out, mag, part) float64 of any role; part = sum_k |per-offset partial result| (the 'pair16' bound).  nominal: mag over
    the nominal fp16 magnitudes."""
    return _f64(x, w, nbr, n_in, role, nominal=nominal, parts=True)


def _chain(acc, a, b):
    """acc + a @ b in plain fp32, one channel at a time: one rounding per product, one per addition"""
    for c in range(a.shape[1]):
        acc = acc + a[:, c:c + 1] * b[c]
    return acc


def honest_fp32(x, w, nbr, n_in, role, descending=False, skip=None, post=None, mat=None, running=False):
    """The contraction in plain fp32, the offsets ascending (descending: the second honest order), within an offset the channels
    ascending, every product rounded and added on its own; no library matmul, so the same arithmetic on every machine.  Two
    accumulator structures, as the kernels have them:
      running=False  every offset's product is summed from zero and added to the row once -- the tile kernel (a block's MFMA
                     accumulators start at zero, ``o += acc0 + acc1``), the pair kernels (a scratch row y per pair, summed by the
                     gather-sum);
      running=True   ONE running sum per row through every offset and channel -- conv_os2 / conv_os3, whose ``acc`` registers
                     live from the first offset to the store: ca / 4 additions per offset at the magnitude of the running sum.
    ``skip``: an offset left out (a degraded form); ``mat(k)``: another matrix for offset k (degraded forms); ``post``: applied to
    every offset's product before it is added (the 16-bit pair form's rounded scratch rows).  fp32."""
    xf, wf = x.float(), w.float()
    order = [k for k in range(nbr.shape[0]) if k != skip]
    out = torch.zeros(n_dst(nbr, n_in, role), shape_of(w, role)[1], dtype=torch.float32, device=x.device)
    for k, dst, src, kw, tr in offsets(nbr, role, order[::-1] if descending else order):
        if len(dst):
            b = mat(k) if mat is not None else (wf[kw].t() if tr else wf[kw])
            if running:
                out[dst] = _chain(out[dst], xf[src], b)
            else:
                t = _chain(torch.zeros(len(dst), out.shape[1], device=x.device), xf[src], b)
                out[dst] = out[dst] + (post(t) if post else t)
    return out


def split3_round(w):
    """fp32 w -> (h, m, l) by ROUNDING to nearest, each a bf16 held in an fp32: split3 of conv_tp.hip / px_split3"""
    w = w.float()
    h = w.bfloat16().float()
    r1 = w - h
    m = r1.bfloat16().float()
    return h, m, (r1 - m).bfloat16().float()


def x3_eval(x, w, nbr, n_in, role, drop=()):
    """The bf16x3 product of conv_tp_kernel / conv_px3_kernel: rows split by truncation, weights by rounding; per offset an fp32
    accumulator takes, per 32-channel step, the partial products of X3_PRODUCTS in order, each the exact sum of its 32 terms
    (float64: a term has 16 significant bits); the offset's accumulator is then added to the row.  ``drop``: products left out."""
    px = [p.double() for p in split3(x)]
    pw = [p.double() for p in split3_round(w)]
    todo = [pq for pq in X3_PRODUCTS if pq not in drop]
    rows = torch.arange(x.shape[0], device=x.device)

    def mul(src, b, k):        # src = row indices, b = (weight index, transposed)
        kw, tr = b
        acc = None
        for c0 in range(0, px[0].shape[1], 32):
            for p, q in todo:
                wk = pw[p][kw].t() if tr else pw[p][kw]
                t = px[q][src][:, c0:c0 + 32] @ wk[c0:c0 + 32]
                acc = t.float() if acc is None else (acc.double() + t).float()
        return acc

    out = torch.zeros(n_dst(nbr, n_in, role), shape_of(w, role)[1], dtype=torch.float32, device=x.device)
    for k, dst, src, kw, tr in offsets(nbr, role):
        if len(dst):
            out.index_add_(0, dst, mul(rows[src], (kw, tr), k))
    return out


def rows16_eval(x, w, nbr, n_in, role, pair, y_fp32=False):
    """One-plane 16-bit products with fp32 sums on rows / weights of a 16-bit type: the tile form rounds the fp32 sum once;
    the pair form (``pair``) rounds every live offset's row y and then the sum (y_fp32: y kept in fp32 -- the tile form's
    arithmetic under the pair form's name).  Returns a tensor of x's dtype."""
    dt = x.dtype
    post = (lambda t: t.to(dt).float()) if pair and not y_fp32 else None
    return honest_fp32(x, w.to(dt), nbr, n_in, role, post=post).to(dt)


# ---- the folded eval-mode epilogue ---------------------------------------------------------------------------------------------

def epilogue_f64(conv64, mag, scale, shift, res, relu):
    """(relu?(conv * scale + shift (+ res)), |scale| * mag + |shift| + |res|) in float64"""
    v = conv64 * scale.double() + shift.double()
    m = mag * scale.double().abs() + shift.double().abs()
    if res is not None:
        v = v + res.double()
        m = m + res.double().abs()
    return (v.clamp(min=0) if relu else v), m


def epilogue_fp32(conv32, scale, shift, res, relu, no_shift=False, relu_first=False):
    """The epilogue as the kernels compute it, in fp32: fma, residual add, ReLU (no_shift / relu_first: degraded forms)"""
    v = conv32.double() * scale.double()          # (the product of two fp32 is exact in float64: the sum below rounds like an fma)
    v = (v if no_shift else v + shift.double()).float()
    if relu and relu_first:
        v = v.clamp(min=0)
    if res is not None:
        v = v + res
    return v.clamp(min=0) if relu and not relu_first else v


# ---- the bounds ------------------------------------------------------------------------------------------------------------

def rel_err(got, ref, mag):
    """largest |got - ref| / mag (inf where mag = 0 and got != ref)"""
    err = (got.double() - ref).abs()
    ratio = torch.where(mag > 0, err / mag.clamp(min=1e-300), torch.where(err > 0, float('inf'), 0.0).to(err.dtype))
    return float(ratio.max()) if ratio.numel() else 0.0


def bound(kind, mag, r, ref=None, part=None, dtype=None, k=0, margin=MARGIN):
    """The elementwise bound of the docstring; kind in 'f16x2', 'f32', 'x3', 'tile16', 'pair16'.  (margin: the host test
    halves the factor of the accumulation term where a bound also holds the rounding of a stored value, which no summation
    order changes)"""
    acc = mag * (margin * max(float(r), FLOOR))
    if kind == 'f16x2':
        return mag * T_F16X2
    if kind == 'f32':
        return acc
    if kind == 'x3':
        return mag * T_FWD + acc
    u, s = UNIT[dtype], SUBNORMAL[dtype]
    live = (mag > 0).double()
    if kind == 'tile16':
        return acc + u * (ref.abs() + acc) + s * live
    if kind == 'pair16':
        e = acc + u * (part + acc) + k * s * live
        return e + u * (ref.abs() + e) + s * live
    raise ValueError(kind)


def epilogue_bound(conv_bound, emag, scale, has_res):
    sb = conv_bound * scale.double().abs()
    return sb + (2 if has_res else 1) * 2.0 ** -24 * (emag + sb)


def check(got, ref, bd, mag=None):
    """(passes, largest err / bound, largest err / mag) -- an element whose bound is 0 must be exact"""
    err = (got.double() - ref).abs()
    over = torch.where(bd > 0, err / bd.clamp(min=1e-300), torch.where(err > 0, float('inf'), 0.0).to(err.dtype))
    worst = float(over.max()) if over.numel() else 0.0
    return bool((err <= bd).all()), worst, rel_err(got, ref, ref.abs() if mag is None else mag)


# ---- the dispatch of _conv_os (functional.py) and of the C side (conv.hip, conv_tp.hip), restated --------------------------

def tiles_supported(cin, cout):
    nbw = {32: 1, 64: 1, 96: 2, 128: 2}.get(cout)
    return nbw is not None and cin in (32, 64, 96, 128) and cin * nbw <= 128


def pairs_mode(cin, cout, n_rows):
    return cout % 4 == 0 and (cin * cout > 8192 or (cin * cout == 8192 and n_rows < 24000))


def px3_tile(cin, cout):
    """(column tile, TL) of conv_px3.hip's px3_shape, restated"""
    w3 = cout % 96 == 0 and cout % 128 != 0
    tl = 2 if (cin >= 512 or cout >= 384) else 1
    nbw = 2 if tl == 2 else (4 if (cout % 192 == 0 if w3 else cout % 256 == 0) else 2)
    return 16 * (3 if w3 else 4) * nbw, tl


def family(cin, cout, dtype, n_rows, k):
    """(entry, arithmetic, form) a cin -> cout LAUNCH of ``dtype`` rows over ``n_rows`` destination rows is run on under default
    settings.  arithmetic: 'f16x2', 'x3', 'f32', 'tile16', 'pair16'.  form: the instantiation where the entry has several --
    u2mkd_conv_forward_sorted: ('conv_os2', kc) or ('conv_os3', kc, 'narrow' | 'wide'); u2mkd_conv_forward_pairs: its variant
    (32 | 64 channels per stage); the bf16x3 / f16x2 pair kernels: (column tile, TL) of conv_px3.hip."""
    px3 = cin >= 32 and cin % 32 == 0 and cout >= 32 and cout % 32 == 0
    if dtype != torch.float32:
        tag = '_bf16' if dtype == torch.bfloat16 else '_f16'
        if tiles_supported(cin, cout):
            return 'u2mkd_conv_forward_tiles' + tag, 'tile16', None
        if not px3:
            raise ValueError('no 16-bit kernel for %d -> %d' % (cin, cout))
        return 'u2mkd_conv_forward_pairs' + tag, 'pair16', px3_tile(cin, cout)
    if pairs_mode(cin, cout, n_rows):
        if px3:
            return 'u2mkd_conv_forward_pairs_f16x2', 'f16x2', px3_tile(cin, cout)
        return 'u2mkd_conv_forward_pairs', 'f32', 64 if (cin * cout >= 16384 and cin % 64 == 0) else 32
    if tiles_supported(cin, cout):
        return 'u2mkd_conv_forward_tiles', ('f16x2' if cin in (32, 64, 128) else 'x3'), None
    kc = 64 if cin % 64 == 0 else 32
    if cout % 128 == 0 and cin >= 16:
        tiles = -(-n_rows // 64) * (cout // 128)
        return 'u2mkd_conv_forward_sorted', 'f32', ('conv_os3', kc, 'narrow' if tiles < 1024 else 'wide')
    return 'u2mkd_conv_forward_sorted', 'f32', ('conv_os2', kc)


# ---- synthetic neighbour tables ----------------------------------------------------------------------------------------------

_RAGGED27 = [0, 1, 63, 64, 65, 127, 128, 129, 700, 2, 0, 31, 33, 5, 3, 7, 11, 13, 17, 19, 23, 29, 37, 255, 257, 1, 0]
_RAGGED8 = [0, 1, 33, 130, 64, 0, 700, 17]
RAGGED_COUNTS = {27: _RAGGED27, 8: _RAGGED8}
TAILS = (1, 63, 64, 65, 129)
MANY_ROWS = 36000
# pattern name -> (generator, K, n_in, n_out); the sizes are the smallest at which the edge exists
PATTERNS = {
    'tails1': ('tails', 27, 1, 1), 'tails63': ('tails', 27, 63, 63), 'tails64': ('tails', 27, 64, 64),
    'tails65': ('tails', 27, 65, 65), 'tails129': ('tails', 27, 129, 129),
    'ragged27': ('ragged', 27, 750, 800),          # n_in < n_out
    'ragged8': ('ragged', 8, 900, 720),            # n_in > n_out
    'ragged-one': ('ragged', 27, 1, 65),           # one input row: every offset has 0 or 1 pairs
    'heavy': ('heavy', 27, 256, 256),
    'many': ('many', 27, MANY_ROWS, MANY_ROWS),
}
SYMMETRIC = ('tails1', 'tails63', 'tails64', 'tails65', 'tails129')
SMALL = SYMMETRIC + ('ragged27', 'ragged8', 'ragged-one')
RAGGED = ('ragged27', 'ragged8', 'ragged-one')
# every (pattern, spread) the GPU test runs; the host test runs the CPU evaluations on exactly these
COMBOS = [(p, 'rows') for p in SMALL] + [('ragged27', 'unit'), ('ragged27', 'tiny'), ('heavy', 'rows'), ('many', 'rows')]


def roles_of(name, inverse=False):
    """the roles a pattern serves: 'flip' needs a symmetric table; inverse: the pair kernels' swapped walk"""
    return ('fwd',) + (('flip',) if name in SYMMETRIC else ()) + (('inv', 'invT') if inverse else ())


def make_table(pattern, k_total, n_in, n_out, seed=0):
    """A synthetic neighbour table int32 [K, n_out] (CPU).  EVERY OFFSET'S MAP IS INJECTIVE: no input row appears twice in one
    offset, as in a real kernel map (u2mkd_pairs_build writes pos_in[i][k] once, and the pair capacity K * min(n_in, n_out) +
    padding relies on it).  Entries lie in [-1, n_in).  The same generator on every machine.
      'tails'   symmetric (n_in = n_out, nbr[K-1-k][nbr[k][j]] = j, the centre offset the identity on live rows); about a tenth
                of the rows without a neighbour at any offset, a tenth with the centre only
      'ragged'  per-offset pair counts RAGGED_COUNTS[K] (0, 1, 63, 64, 65, 127, 128, 129, 700 ...), each capped by
                min(n_in, n_out); n_in != n_out
      'heavy'   four 64-row tiles of rows with pairwise different masks: rows that have the last offset carry ~75 % of the
                others (a sorted tile of them counts 3 - 4 blocks per offset: beyond both split thresholds), rows that have not
                carry ~30 % (~2 blocks per offset: between the thresholds)
      'many'    MANY_ROWS rows, every offset a cyclic shift on 55 % of the rows: a sorted 64-row tile then holds ~35 rows per
                offset, 3 blocks each, ~70 blocks -- past the second split threshold, so that nearly every tile is FOUR work items
                and the item count (``work_items``) exceeds 2048 = 256 CUs x 8 workgroups, more than any instantiation of the tile
                kernel keeps resident: the clamped grid deals several items to a workgroup.  (Sparser rows cannot do this: 61
                blocks in 64 rows take at least 571 pairs, 9 per row.)"""
    g = torch.Generator().manual_seed(7919 * seed + 31 * k_total + 1000003 * n_out + n_in)
    nbr = torch.full((k_total, n_out), -1, dtype=torch.int64)
    if pattern == 'tails':
        assert n_in == n_out and k_total % 2 == 1
        n, c = n_out, k_total // 2
        kind = torch.rand(n, generator=g)
        kind[0] = 1.0                                          # (row 0 always takes part: n = 1 is not an empty case)
        live = torch.nonzero(kind >= 0.1)[:, 0]               # the others: no neighbour at any offset
        active = torch.nonzero(kind >= 0.2)[:, 0]             # live but not active: the centre only
        nbr[c, live] = live
        for k in range(c):
            perm = active[torch.randperm(len(active), generator=g)]
            take = torch.rand(len(active), generator=g) < 0.35
            nbr[k, active[take]] = perm[take]
            nbr[k_total - 1 - k, perm[take]] = active[take]
    elif pattern == 'ragged':
        for k, cnt in enumerate(RAGGED_COUNTS[k_total]):
            cnt = min(cnt, n_in, n_out)
            rows = torch.randperm(n_out, generator=g)[:cnt]
            nbr[k, rows] = torch.randperm(n_in, generator=g)[:cnt]
    elif pattern == 'heavy':
        dense = torch.arange(n_out) % 2 == 1
        for k in range(k_total):
            p = torch.where(dense, 0.75, 0.3)
            has = torch.rand(n_out, generator=g) < p if k < k_total - 1 else dense
            perm = torch.randperm(n_in, generator=g)[:n_out]
            nbr[k, has] = perm[has]
    elif pattern == 'many':
        assert n_in == n_out
        j = torch.arange(n_out)
        for k in range(k_total):
            has = torch.rand(n_out, generator=g) < 0.55
            nbr[k, has] = ((j + 1 + 997 * k) % n_in)[has]
    else:
        raise ValueError(pattern)
    assert int(nbr.max()) < n_in and int(nbr.min()) >= -1
    return nbr.int().contiguous()


def table(name, seed=0):
    """(nbr, n_in) of a named pattern"""
    gen, k, n_in, n_out = PATTERNS[name]
    return make_table(gen, k, n_in, n_out, seed), n_in


def pair_counts(nbr):
    return [int(c) for c in (nbr >= 0).sum(dim=1)]


def tile_blocks(nbr, rows=64):
    """per 64-row tile of the mask-sorted table (TileSchedule's order): sum over offsets of ceil(pairs / 16)"""
    k_total, n = nbr.shape
    has = (nbr >= 0).long()
    mask = (has << torch.arange(k_total)[:, None]).sum(dim=0)
    order = torch.argsort(mask, stable=True)
    has = has[:, order]
    return [int(((has[:, t:t + rows].sum(dim=1) + 15) // 16).sum()) for t in range(0, n, rows)]


def work_items(nbr, split=(30, 60)):
    """the number of work items u2mkd_tile_schedule makes of the table: a tile of b blocks is 1 << ((b > split[0]) + (b > split[1]))
    parts of 64, 32 or 16 rows, of which those that hold a row count"""
    n, total = nbr.shape[1], 0
    for t, b in enumerate(tile_blocks(nbr)):
        lg = (b > split[0]) + (b > split[1])
        rows_left = min(64, n - 64 * t)
        total += sum(1 for sub in range(1 << lg) if sub * (64 >> lg) < rows_left)
    return total


# ---- rows and weights ------------------------------------------------------------------------------------------------------

SPREADS = ('unit', 'rows', 'tiny')


def make_rows(spread, n, c, dtype=torch.float32, seed=0):
    """[n, c] rows of ``dtype`` (CPU).  'unit': randn.  'rows': a magnitude per row, 1e-18 .. 1e18 for fp32 (16-bit rows: a
    range that stays finite in the type after the convolution: 1e-10 .. 1e10 bf16, 1e-3 .. 1e3 fp16), a tenth of the rows zero,
    a twentieth with one nonzero channel.  'tiny': gradients late in training, 1e-20 (fp16: 1e-4).  Seeded per case."""
    g = torch.Generator().manual_seed(104729 * seed + 613 * n + c)
    x = torch.randn(n, c, generator=g)
    if spread == 'rows':
        lo, hi = {torch.float32: (-18, 19), torch.bfloat16: (-10, 11), torch.float16: (-3, 4)}[dtype]
        x = x * torch.pow(10.0, torch.randint(lo, hi, (n, 1), generator=g).float())
        zero, one = torch.rand(n, generator=g) < 0.1, torch.rand(n, generator=g) < 0.05
        zero[0] = one[0] = False                               # (row 0 stays a full row: a table of one row is not all zeros)
        x[zero] = 0.0
        keep = torch.zeros(c)
        keep[3 % c] = 1.0
        x[one] = x[one] * keep
    elif spread == 'tiny':
        x = x * (1e-4 if dtype == torch.float16 else 1e-20)
    elif spread != 'unit':
        raise ValueError(spread)
    return x.to(dtype)


def make_weights(k_total, rows, cols, spread='unit', seed=0):
    """kernel [K, rows, cols] fp32 at the scale of a trained layer ('tiny': after heavy decay, x 1e-6)"""
    g = torch.Generator().manual_seed(15485863 * seed + 101 * rows + cols + 7 * k_total)
    w = torch.randn(k_total, rows, cols, generator=g) / (k_total * rows) ** 0.5
    return w * 1e-6 if spread == 'tiny' else w


def make_affine(c, n, seed=0):
    """(scale of mixed sign, shift, residual [n, c]) of a folded eval-mode BatchNorm"""
    g = torch.Generator().manual_seed(32452843 * seed + 17 * c + n)
    scale = torch.randn(c, generator=g) * torch.pow(10.0, torch.randint(-2, 3, (c,), generator=g).float())
    return scale, torch.randn(c, generator=g), torch.randn(n, c, generator=g) * 3.0


def make_case(name, role, ca, cb, spread, dtype=torch.float32, seed=0):
    """CPU tensors of one case: the table, x [n_src, ca] of ``dtype``, the kernel w fp32 shaped so that the launch is ca -> cb"""
    nbr, n_in = table(name, seed)
    n_src = n_in if role in ON_OUTPUTS else nbr.shape[1]
    w = make_weights(nbr.shape[0], cb if role in TRANSPOSED else ca, ca if role in TRANSPOSED else cb, spread, seed)
    return {'nbr': nbr, 'n_in': n_in, 'x': make_rows(spread, n_src, ca, dtype, seed), 'w': w, 'role': role, 'k': nbr.shape[0]}


# ---- wrong evaluations the bounds have to reject (or, where said, to accept) ---------------------------------------------------

def _off_by_one(c):
    """one neighbour index off by one row, at the first pair that gathers the largest row of x which the table uses at all: an
    error in a row that is tiny next to the other terms of its sum is invisible to ANY bound relative to mag, so the wrong index
    sits where the term weighs most.  (The CPU evaluation does not need the changed offset to stay injective.)"""
    nbr, n_in = c['nbr'].clone(), c['n_in']
    forward = c['role'] in ON_OUTPUTS
    for row in torch.argsort(c['x'].float().abs().amax(dim=1), descending=True).tolist():
        hit = torch.nonzero(nbr == row) if forward else torch.nonzero(nbr[:, row] >= 0)
        if len(hit):
            k, j = (int(hit[0, 0]), int(hit[0, 1])) if forward else (int(hit[0, 0]), row)
            nbr[k, j] = (int(nbr[k, j]) + 1) % n_in
            return nbr
    return nbr


def _skip_last_pair(nbr):
    nbr = nbr.clone()
    for k in range(nbr.shape[0]):
        j = torch.nonzero(nbr[k] >= 0)[:, 0]
        if len(j):
            nbr[k, j[-1]] = -1
    return nbr


def _largest_offset(nbr):
    return int((nbr >= 0).sum(dim=1).argmax())


def _flip_as(c, mirror, transpose):
    """the 'flip' role (square shapes) with the mirroring of the offset or the transposition of the weight left out"""
    w, kt = c['w'].float(), c['k']
    pick = lambda k: w[kt - 1 - k if mirror else k]
    return honest_fp32(c['x'], w, c['nbr'], c['n_in'], 'fwd', mat=lambda k: pick(k).t() if transpose else pick(k))


# name -> (kinds it applies to, must the bound reject it, f(case) -> result)
DEGRADED = {
    'one offset left out': (('f32', 'x3', 'f16x2'), True,
                            lambda c: honest_fp32(c['x'], c['w'], c['nbr'], c['n_in'], c['role'], skip=_largest_offset(c['nbr']))),
    # (the next two: square shapes, and only the roles that mirror / transpose differ from them)
    'mirrored offset not mirrored': (('f32', 'x3', 'f16x2'), True, lambda c: _flip_as(c, mirror=False, transpose=True)),
    'weight not transposed': (('f32', 'x3', 'f16x2'), True,
                              lambda c: _flip_as(c, mirror=True, transpose=False) if c['role'] == 'flip' else
                              honest_fp32(c['x'], c['w'], c['nbr'], c['n_in'], 'invT' if c['role'] == 'inv' else c['role'])),
    'one neighbour index off by one row': (('f32', 'x3', 'f16x2'), True,
                                           lambda c: honest_fp32(c['x'], c['w'], _off_by_one(c), c['n_in'], c['role'])),
    'an operand rounded to bf16': (('f32', 'x3', 'f16x2'), True,
                                   lambda c: honest_fp32(c['x'].bfloat16().float(), c['w'], c['nbr'], c['n_in'], c['role'])),
    'x3 with one more product dropped': (('x3',), True,
                                         lambda c: x3_eval(c['x'], c['w'], c['nbr'], c['n_in'], c['role'], drop=((1, 1),))),
    'last pair of every offset skipped': (('f32', 'x3', 'f16x2'), True,
                                          lambda c: honest_fp32(c['x'], c['w'], _skip_last_pair(c['nbr']), c['n_in'], c['role'])),
    'pair16 with y kept in fp32': (('pair16',), False,
                                   lambda c: rows16_eval(c['x'], c['w'], c['nbr'], c['n_in'], c['role'], pair=True, y_fp32=True)),
}
EPILOGUE_DEGRADED = {
    'epilogue without shift': dict(no_shift=True),
    'epilogue with ReLU before the residual add': dict(relu_first=True),
}
