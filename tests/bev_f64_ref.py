"""float64 statement of torchsparse.nn's four BEV modules and the bounds the drop-in is held to (test helper; plain torch, CPU or
GPU tensors).  The torchsparse source is not at hand; the semantics are RECALLED from v1.4.0 and this file is their normative
statement.

THE OPERATIONS.  coords int32 [N, 4] = (x, y, z, b), feats [N, C], tensor stride s; ``dim`` is the height axis, the two other
axes in ascending order are the BEV axes; ``trunc`` rounds toward zero; B = the largest batch index + 1.  Every forward here
is an ``index_add_`` of float64 rows into a dense float64 buffer, so autograd through it is the backward reference, and every
forward returns next to its result ``mag``: the same sum over absolute values, the scale every rounding error is relative to.

  reduction64          key = coords with axis dim set to 0; out = the MEAN of the rows that share a key (rows sorted by (b, x, y, z)).
  convolution64        z_r = trunc(c[dim] / s[dim]); y_r = feats_r @ kernel[z_r] + bias (per input row, BEFORE the sum: a cell fed
                       by m rows carries m * bias); ratio = s * stride; key: axis dim 0, the BEV axes trunc(c / ratio) * ratio
                       (unchanged for stride 1); out = the SUM of y_r per key.
  dense_convolution64  y_r as above (the offset is NOT subtracted for the kernel index); u = trunc((c[bev0] - offset[bev0]) /
                       s[bev0]), v likewise; out [B, Cout, H, W], out[b, :, u, v] = the sum of y_r.
  height_compression64 u, v as above, w = clamp(trunc((c[dim] - offset[dim]) / s[dim]), 0, Z - 1); out [B, C * Z, H, W],
                       out[b, c * Z + w, u, v] = the sum of feats_r[c].

``variant`` names ONE deliberate mistake (``DEGRADED``): the host test requires the bounds to reject each.

THE BOUNDS, all derived, none fitted to what a kernel returns.
  convolution part     ``reference`` / ``bound`` / ``check`` / ``family`` of tests/conv_fwd_f64_ref.py on the neighbour table
                       ``neighbour_table`` builds from (cell, height) alone -- roles 'fwd' (forward) and 'inv' (input gradient) --
                       and tests/wgrad_f64_ref.py on ``pair_list`` for dkernel; the kernel family that serves a shape decides the
                       bound, as in the conv tests.  ``conv_bound`` adds
  per-row bias         the cell's m * bias is added exactly and the sum rounded once: m |bias| joins the magnitude, and the bound
                       grows by one rounding of the row type at that magnitude, 2^-24 (fp32) or u (16-bit rows, + s) times
                       (mag + m |bias| + the convolution's bound).
  reduction mean       the kernel sums in double and rounds once: ONE fp32 ulp of the float64 mean (scene_rows_f64_ref.ulp32); for
                       16-bit rows one rounding unit u of the type at |mean| plus its subnormal floor s.
  dense store          a (cell, w) slot fed by one row is that row, bit for bit (bound 0 = torch.equal); a slot fed by m rows is
                       summed in fp32 in ascending row order: (m - 1) * 2^-24 * sum |terms|, plus for 16-bit rows the store's
                       rounding u * (|ref| + that) + s.
  dense gather         a copy: torch.equal.
The formulation on torch operators (more than 31 heights, stride > 1) is an fp32 evaluation in another order: the 'f32' bound
with r measured on ``honest_rows_fp32``."""
import torch

import conv_fwd_f64_ref as CR
from scene_rows_f64_ref import ulp32

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
UNIT, SUBNORMAL = CR.UNIT, CR.SUBNORMAL
U32 = 2.0 ** -24

DEGRADED = {
    'bias added once per cell': 'bias_once',
    'reduction as a sum': 'sum',
    'height index not divided by the stride': 'no_stride_div',
    'offset subtracted for the kernel index': 'offset_in_kernel_index',
    'channel index w * C + c': 'wc_channel',
    'u and v swapped': 'uv_swapped',
    'floor instead of trunc on a negative coordinate': 'floor',
    'a dropped last row': 'drop_last',
}


def bev_axes(dim):
    return tuple(k for k in range(3) if k != dim)


def _div(a, b, variant=''):
    return torch.div(a, b, rounding_mode='floor' if variant == 'floor' else 'trunc')


def _rows(feats, coords, variant):
    if variant == 'drop_last':
        return feats[:-1], coords[:-1]
    return feats, coords


def batch_size(coords):
    return int(coords[:, 3].max()) + 1 if coords.shape[0] else 0


def sorted_keys(key):
    """(out coords int32 [n_out, 4] sorted by (b, x, y, z), inverse int64 [N]) of the rows ``key`` [N, 4] = (x, y, z, b)"""
    if key.shape[0] == 0:
        return key.int(), torch.zeros(0, dtype=torch.int64)
    uniq, inv = torch.unique(key[:, [3, 0, 1, 2]].long(), dim=0, return_inverse=True)
    return uniq[:, [1, 2, 3, 0]].int(), inv


def reduction64(feats, coords, dim=1, variant=''):
    """(out coords, mean float64 [n_out, C], mag, rows per output row)"""
    feats, coords = _rows(feats, coords, variant)
    key = coords.clone()
    key[:, dim] = 0
    oc, inv = sorted_keys(key)
    x = feats.double()
    cnt = torch.zeros(oc.shape[0], dtype=torch.float64).index_add_(0, inv, torch.ones(inv.shape[0], dtype=torch.float64))
    tot = torch.zeros(oc.shape[0], x.shape[1], dtype=torch.float64).index_add_(0, inv, x)
    mag = torch.zeros(oc.shape[0], x.shape[1], dtype=torch.float64).index_add_(0, inv, x.detach().abs())
    if variant == 'sum':
        return oc, tot, mag, cnt
    return oc, tot / cnt[:, None], mag / cnt[:, None], cnt


def height_index(coords, s, dim, offset=(0, 0, 0), variant=''):
    c = coords[:, dim].long()
    if variant == 'offset_in_kernel_index':
        c = c - offset[dim]
    return c if variant == 'no_stride_div' else _div(c, s[dim], variant)


def _rows64(feats, kernel, bias, z):
    """(y_r without the bias, sum |x| |k|) per input row"""
    x, k = feats.double(), kernel.double()
    kz = k[z]
    y = torch.bmm(x[:, None, :], kz)[:, 0, :]
    mag = torch.bmm(x.detach().abs()[:, None, :], kz.detach().abs())[:, 0, :]
    return y, mag


def _with_bias(out, mag, cnt, bias, variant):
    if not isinstance(bias, torch.Tensor):
        return out, mag
    b = bias.double().reshape(1, -1)
    m = (cnt > 0).double()[:, None] if variant == 'bias_once' else cnt[:, None]
    return out + m * b, mag + m * b.detach().abs()


def convolution64(feats, coords, s, kernel, bias=0, stride=1, dim=1, variant=''):
    """(out coords, out float64 [n_out, Cout], mag, rows per output row, inverse, height index)"""
    feats, coords = _rows(feats, coords, variant)
    z = height_index(coords, s, dim, variant=variant)
    z = z.clamp(0, kernel.shape[0] - 1) if variant else z          # (a degraded form may leave the range: it is still evaluated)
    assert int(z.min()) >= 0 and int(z.max()) < kernel.shape[0], 'kernel index out of range'
    key = coords.clone()
    key[:, dim] = 0
    if stride > 1:
        for a in bev_axes(dim):
            ratio = s[a] * stride
            key[:, a] = (_div(coords[:, a].long(), ratio, variant) * ratio).int()
    oc, inv = sorted_keys(key)
    y, ym = _rows64(feats, kernel, bias, z)
    n_out = oc.shape[0]
    cnt = torch.zeros(n_out, dtype=torch.float64).index_add_(0, inv, torch.ones(inv.shape[0], dtype=torch.float64))
    out = torch.zeros(n_out, y.shape[1], dtype=torch.float64).index_add_(0, inv, y)
    mag = torch.zeros(n_out, y.shape[1], dtype=torch.float64).index_add_(0, inv, ym)
    out, mag = _with_bias(out, mag, cnt, bias, variant)
    return oc, out, mag, cnt, inv, z


def cells(coords, s, shape, offset, dim, variant=''):
    """(cell index (b * H + u) * W + v int64 [N], B, H, W); u, v must be in range"""
    b0, b1 = bev_axes(dim)
    h, w = shape[b0], shape[b1]
    u = _div(coords[:, b0].long() - offset[b0], s[b0], variant)
    v = _div(coords[:, b1].long() - offset[b1], s[b1], variant)
    if variant == 'uv_swapped':
        u, v = v.clamp(max=h - 1), u.clamp(max=w - 1)
    assert int(u.min()) >= 0 and int(u.max()) < h and int(v.min()) >= 0 and int(v.max()) < w, 'BEV cell out of range'
    return (coords[:, 3].long() * h + u) * w + v, h, w


def dense_convolution64(feats, coords, s, kernel, bias, shape, offset=(0, 0, 0), dim=1, variant='', nb=None):
    """(out float64 [B, Cout, H, W], mag, rows per cell [B * H * W], cell, height index)"""
    nb = batch_size(coords) if nb is None else nb
    feats, coords = _rows(feats, coords, variant)
    z = height_index(coords, s, dim, offset, variant)
    z = z.clamp(0, kernel.shape[0] - 1) if variant else z
    assert int(z.min()) >= 0 and int(z.max()) < kernel.shape[0], 'kernel index out of range'
    cell, h, w = cells(coords, s, shape, offset, dim, variant)
    y, ym = _rows64(feats, kernel, bias, z)
    n_out = nb * h * w
    cnt = torch.zeros(n_out, dtype=torch.float64).index_add_(0, cell, torch.ones(cell.shape[0], dtype=torch.float64))
    out = torch.zeros(n_out, y.shape[1], dtype=torch.float64).index_add_(0, cell, y)
    mag = torch.zeros(n_out, y.shape[1], dtype=torch.float64).index_add_(0, cell, ym)
    out, mag = _with_bias(out, mag, cnt, bias, variant)
    to_nchw = lambda t: t.view(nb, h, w, -1).permute(0, 3, 1, 2)
    return to_nchw(out), to_nchw(mag), cnt, cell, z


def height_compression64(feats, coords, s, shape, offset=(0, 0, 0), dim=1, variant='', nb=None):
    """(out float64 [B, C * Z, H, W], mag, rows per (cell, w) slot as [B, C * Z, H, W])"""
    nb = batch_size(coords) if nb is None else nb
    feats, coords = _rows(feats, coords, variant)
    zz = shape[dim]
    wq = _div(coords[:, dim].long() - offset[dim], s[dim], variant).clamp(0, zz - 1)
    cell, h, w = cells(coords, s, shape, offset, dim, variant)
    x = feats.double()
    c = x.shape[1]
    slot = cell * zz + wq
    n_slot = nb * h * w * zz
    out = torch.zeros(n_slot, c, dtype=torch.float64).index_add_(0, slot, x)
    mag = torch.zeros(n_slot, c, dtype=torch.float64).index_add_(0, slot, x.detach().abs())
    cnt = torch.zeros(n_slot, dtype=torch.float64).index_add_(0, slot, torch.ones(slot.shape[0], dtype=torch.float64))

    def to_nchw(t):
        t = t.view(nb, h, w, zz, -1)
        if variant == 'wc_channel':
            return t.permute(0, 3, 4, 1, 2).reshape(nb, -1, h, w)
        return t.permute(0, 4, 3, 1, 2).reshape(nb, -1, h, w)
    return to_nchw(out), to_nchw(mag), to_nchw(cnt[:, None].expand(-1, c).contiguous())


# ---- the convolution as a neighbour table ----------------------------------------------------------------------------------

def neighbour_table(group, z, nk, n_out):
    """nbr int32 [nk, n_out]: the input row of output row g at height k (-1: none), from (group, height) alone; a (group,
    height) pair must hold at most one row"""
    slot = z.long() * n_out + group.long()
    assert len(torch.unique(slot)) == len(slot), 'a (cell, height) pair holds several rows'
    nbr = torch.full((nk * n_out,), -1, dtype=torch.int32)
    nbr[slot] = torch.arange(len(slot), dtype=torch.int32)
    return nbr.view(nk, n_out)


def pair_list(group, z, nk):
    """(pairs int32 [N, 2] (in, out) grouped by height, counts per height): what the weight gradient sums over"""
    order = torch.sort(z.long(), stable=True).indices
    pairs = torch.stack([order, group.long()[order]], 1).int()
    return pairs, torch.bincount(z.long(), minlength=nk).tolist()


def honest_rows_fp32(feats, kernel, bias, z, group, n_out):
    """The formulation on torch operators in plain fp32: y_r = chain over the channels of feats_r * kernel[z_r] (one rounding per
    product and per addition), + bias, then the rows of an output row added in ascending row order."""
    x, k = feats.float(), kernel.float()
    y = torch.zeros(x.shape[0], k.shape[2])
    for kk in range(k.shape[0]):
        rows = torch.nonzero(z == kk)[:, 0]
        if len(rows):
            y[rows] = CR._chain(torch.zeros(len(rows), k.shape[2]), x[rows], k[kk])
    if isinstance(bias, torch.Tensor):
        y = y + bias.float().reshape(1, -1)
    out = torch.zeros(n_out, k.shape[2])
    for r in range(x.shape[0]):
        out[group[r]] += y[r]
    return out


def pad4(c):
    return c + (-c) % 4


def conv_family(cin, cout, dtype, n_rows, nk):
    """(entry, arithmetic, form) of conv_fwd_f64_ref.family for the PADDED launch (channel counts are padded to multiples of 4)"""
    return CR.family(pad4(cin), pad4(cout), dtype, n_rows, nk)


def store_rounding(err, ref, dtype):
    """the bound after the value is stored in ``dtype``: fp32 unchanged; 16-bit u * (|ref| + err) + s on top"""
    if dtype == F32:
        return err
    return err + UNIT[dtype] * (ref.abs() + err) + SUBNORMAL[dtype]


def conv_bound(kind, mag, r, ref, part, dtype, nk, bias_mag=None, margin=CR.MARGIN):
    """the convolution's bound (conv_fwd_f64_ref.bound) on the magnitude WITHOUT the bias, then the per-row bias: ``bias_mag`` =
    m |bias| per output element, one more rounding of the row type at mag + bias_mag"""
    bd = CR.bound(kind, mag, r, ref, part, dtype if dtype != F32 else None, nk, margin=margin)
    if bias_mag is None:
        return bd
    total = mag + bias_mag + bd
    if dtype == F32:
        return bd + U32 * total
    return bd + UNIT[dtype] * total + SUBNORMAL[dtype]


def mean_bound(ref, dtype):
    if dtype == F32:
        return ulp32(ref)
    return UNIT[dtype] * ref.abs() + SUBNORMAL[dtype]


def dense_store_bound(ref, mag, cnt, dtype):
    """0 for a slot fed by one row (or none); (m - 1) * 2^-24 * sum |terms| for m rows, + the 16-bit store's rounding"""
    acc = (cnt - 1).clamp(min=0) * U32 * mag
    return torch.where(cnt > 1, store_rounding(acc, ref, dtype), torch.zeros_like(acc))


def check(got, ref, bd):
    """(passes, largest err / bound) -- an element whose bound is 0 must be exact"""
    ok, worst, _ = CR.check(got, ref, bd)
    return ok, worst


# ---- the input sets (shared by the host test and the GPU test) -----------------------------------------------------------------

ENGINE_MAX_K = 31        # the conv engine's neighbour tables hold at most 31 offsets (a row's offsets are one int32 mask)
GRID = (5, 7)            # (H, W): not square, so that swapped axes show
BATCHES = (0, 2)         # B = 3, batch index 1 without rows
SIZES = (1, 63, 64, 65, 129, 1500)


def shape_of(dim, nz, grid=GRID):
    b0, b1 = bev_axes(dim)
    shape = [0, 0, 0]
    shape[dim], shape[b0], shape[b1] = nz, grid[0], grid[1]
    return tuple(shape)


def make_coords(n, dim, s, nz, offset=(0, 0, 0), unique=True, beyond=0, shift=(0, 0), seed=0, grid=GRID, offset_height=False):
    """int32 [n, 4]: rows on the H x W x (nz + beyond) slots of batches 0 and 2, at tensor stride ``s`` and ``offset`` on the BEV
    axes (and on the height axis with ``offset_height``).  The first rows are a column with EVERY height (batch 0, cell (0, 0))
    and a column with ONE (batch 2, cell (H-1, W-1)); the rest is drawn from the other slots -- without replacement (``unique``:
    a (cell, height) pair holds one row), else with.  ``beyond``: heights past nz - 1 (the clamp).  ``shift``: cells added to
    (u, v) -- negative values give negative BEV coordinates (sparse modules only)."""
    g = torch.Generator().manual_seed(seed * 7919 + n * 31 + dim)
    h, w = grid
    nh = nz + beyond
    first = [(0, 0, 0, k) for k in range(nh)] + [(2, h - 1, w - 1, nh // 2)]
    pool = [(b, u, v, k) for b in BATCHES for u in range(h) for v in range(w) for k in range(nh)
            if (b, u, v) not in ((0, 0, 0), (2, h - 1, w - 1))]
    if unique:
        assert n <= len(first) + len(pool), (n, len(first) + len(pool))
        pick = [pool[i] for i in torch.randperm(len(pool), generator=g).tolist()]
    else:
        pick = [pool[i] for i in torch.randint(0, len(pool), (n,), generator=g).tolist()]
    slots = (first + pick)[:n]
    if n > 1:       # no particular row order
        slots = [slots[i] for i in torch.randperm(len(slots), generator=g).tolist()]
    b0, b1 = bev_axes(dim)
    c = torch.zeros(n, 4, dtype=torch.int32)
    for i, (b, u, v, k) in enumerate(slots):
        c[i, 3] = b
        c[i, b0] = (u + shift[0]) * s[b0] + offset[b0]
        c[i, b1] = (v + shift[1]) * s[b1] + offset[b1]
        c[i, dim] = k * s[dim] + (offset[dim] if offset_height else 0)
    return c


def make_feats(n, c, dtype=F32, seed=0, spread='rows'):
    """rows of a magnitude each (conv_fwd_f64_ref.make_rows)"""
    return CR.make_rows(spread, n, c, dtype, seed)


def make_kernel(nk, cin, cout, seed=0):
    g = torch.Generator().manual_seed(seed + 17 * nk + cin)
    return (torch.rand(nk, cin, cout, generator=g) * 2 - 1) / cin ** 0.5


def make_bias(cout, seed=0):
    g = torch.Generator().manual_seed(seed + 5 * cout)
    return torch.randn(1, cout, generator=g)


def _case(name, module, n, c, cout=0, nk=3, dim=1, s=(1, 1, 1), offset=(0, 0, 0), stride=1, bias=False, dtype=F32, shift=(0, 0),
          unique=True, beyond=0):
    return dict(name=name, module=module, n=n, c=c, cout=cout, nk=nk, dim=dim, s=s, offset=offset, stride=stride, bias=bias,
                dtype=dtype, shift=shift, unique=unique, beyond=beyond)


# every size, width, height count, axis, stride and row type the GPU test runs (tests/test_gpu_bev.py); the host test takes its
# inputs from the same list
CASES = [
    # ToBEVReduction: columns of several rows; negative BEV coordinates; widths 4 / 20 / 64 and one that is no multiple of 4
    _case('red-n1', 'reduction', 1, 4, nk=5),
    _case('red-n63', 'reduction', 63, 20, nk=5, dim=0, s=(2, 2, 1), shift=(-2, -3)),
    _case('red-n64', 'reduction', 64, 64, nk=5, dim=2),
    _case('red-n65', 'reduction', 65, 6, nk=5, shift=(-2, 0)),
    _case('red-n129', 'reduction', 129, 4, nk=5, unique=False),
    _case('red-n1500', 'reduction', 1500, 64, nk=32, s=(2, 2, 1), shift=(-1, -1), unique=False),
    _case('red-bf16', 'reduction', 129, 64, nk=5, dtype=BF16, unique=False),
    _case('red-f16', 'reduction', 129, 64, nk=5, dtype=F16, unique=False),
    # ToBEVConvolution: one offset per row, n_kernels 1 / 3 / 31 on the engine (ENGINE_MAX_K), 32, 33 and stride 2 on torch operators
    _case('conv-n1', 'convolution', 1, 4, 4, nk=1),
    _case('conv-n63-k1', 'convolution', 63, 4, 4, nk=1, dim=0, bias=True),
    _case('conv-n64', 'convolution', 64, 20, 4, nk=3, dim=2, s=(2, 2, 1), bias=True, shift=(-2, -3)),
    _case('conv-n65', 'convolution', 65, 64, 32, nk=3, bias=True),
    _case('conv-n129', 'convolution', 129, 4, 32, nk=3, dim=1, s=(2, 2, 1), shift=(-1, 0)),
    _case('conv-n1500-k32', 'convolution', 1500, 64, 32, nk=32, bias=True),
    _case('conv-n1500-k31', 'convolution', 1500, 64, 32, nk=31, bias=True),
    _case('conv-k33', 'convolution', 129, 4, 4, nk=33, bias=True),
    _case('conv-stride2', 'convolution', 129, 20, 4, nk=3, stride=2, bias=True, shift=(-3, -2)),
    _case('conv-stride2-s2', 'convolution', 65, 4, 32, nk=3, dim=0, s=(2, 2, 1), stride=2, shift=(-3, -2)),
    _case('conv-bf16', 'convolution', 65, 64, 32, nk=3, bias=True, dtype=BF16),
    _case('conv-f16', 'convolution', 65, 64, 32, nk=3, bias=True, dtype=F16),
    # ToDenseBEVConvolution: offsets that are multiples of the stride, on the height axis too (NOT subtracted for the kernel index)
    _case('dense-n1', 'dense', 1, 4, 4, nk=1),
    _case('dense-n63-k1', 'dense', 63, 4, 4, nk=1, dim=2, offset=(3, 5, 0), bias=True),
    _case('dense-n64', 'dense', 64, 20, 4, nk=3, dim=0, s=(2, 2, 1), offset=(2, 4, 2), bias=True),
    _case('dense-n65', 'dense', 65, 64, 32, nk=3, offset=(2, 1, 1), bias=True),
    _case('dense-n129', 'dense', 129, 4, 32, nk=3, s=(2, 2, 1), offset=(4, 2, 3)),
    _case('dense-n1500-k32', 'dense', 1500, 64, 32, nk=32, offset=(1, 1, 2), bias=True),
    _case('dense-n1500-k31', 'dense', 1500, 64, 32, nk=31, offset=(1, 1, 2), bias=True),
    _case('dense-k33', 'dense', 129, 4, 4, nk=33, bias=True),
    _case('dense-cout6', 'dense', 65, 4, 6, nk=3, bias=True),
    _case('dense-bf16', 'dense', 65, 64, 32, nk=3, bias=True, dtype=BF16),
    _case('dense-f16', 'dense', 65, 64, 32, nk=3, bias=True, dtype=F16),
    # ToBEVHeightCompression: heights beyond Z - 1 (several rows on one (cell, w)), widths 4 / 20 / 64 and 6 (padded)
    _case('height-n1', 'height', 1, 4, nk=3),
    _case('height-n63', 'height', 63, 20, nk=3, dim=0, s=(2, 2, 1), offset=(2, 4, 3), beyond=2),
    _case('height-n64', 'height', 64, 64, nk=2, dim=2, offset=(1, 2, 3), beyond=3),
    _case('height-n65', 'height', 65, 6, nk=3, beyond=1),
    _case('height-n129', 'height', 129, 4, nk=5, s=(2, 2, 1), offset=(2, 1, 0), beyond=2),
    _case('height-n1500', 'height', 1500, 64, nk=5, unique=False, beyond=2),
    _case('height-z33', 'height', 129, 4, nk=33),
    _case('height-bf16', 'height', 129, 64, nk=3, dtype=BF16, beyond=2),
    _case('height-f16', 'height', 129, 64, nk=3, dtype=F16, beyond=2),
]
CASE = {c['name']: c for c in CASES}


def build(case):
    """CPU tensors of a case: coords, feats (rounded to the row type), kernel, bias (tensor or 0), shape"""
    dense = case['module'] in ('dense', 'height')
    coords = make_coords(case['n'], case['dim'], case['s'], case['nk'], case['offset'], case['unique'], case['beyond'],
                         case['shift'], offset_height=case['module'] == 'height')
    out = dict(case, coords=coords, feats=make_feats(case['n'], case['c'], case['dtype'], seed=3),
               shape=shape_of(case['dim'], case['nk']) if dense else None)
    if case['cout']:
        out['kernel'] = make_kernel(case['nk'], case['c'], case['cout'])
        out['bias_t'] = make_bias(case['cout']) if case['bias'] else 0
    return out
