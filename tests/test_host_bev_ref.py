"""tests/bev_f64_ref.py on the CPU, on the inputs of tests/test_gpu_bev.py (``bev_f64_ref.CASES``).

INDEPENDENCE.  The float64 forwards equal the upstream text -- ``torch.sparse_coo_tensor(...).coalesce()`` / ``.to_dense()``,
``index_select`` of the kernel, ``permute(0, 4, 3, 1, 2)`` + ``view`` -- run on the CPU in float64 on the same inputs (sparse
results after sorting the rows; coalesce() takes no negative index, so the coordinates are shifted to be non-negative around it).

DEGRADED VARIANTS.  Each mistake of ``bev_f64_ref.DEGRADED`` is rejected by the bound of the module it belongs to, by name.

HEADROOM.  An honest fp32 evaluation stays at or below HALF of each bound where a summation order can change the result (the
convolution's accumulation term: the rule of tests/test_host_conv_fwd_bound.py).  A bound that holds roundings no order changes
-- the one rounding of the mean, the m - 1 additions of the store in their fixed ascending order, the rounding of the bias sum, a
16-bit store -- reaches its full size on single elements; there the evaluation has to pass the bound with the accumulation
factor halved (``margin`` 2), and its ratio to the whole bound is printed."""
import functools

import pytest
import torch

import bev_f64_ref as R
import conv_fwd_f64_ref as CR

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


@functools.lru_cache(maxsize=None)
def _built(name):
    return R.build(R.CASE[name])


def _names(module):
    return [c['name'] for c in R.CASES if c['module'] == module]


# ---- the upstream text ---------------------------------------------------------------------------------------------------------

def _coalesce(coords_t, feats):
    """rows of equal coordinates summed by coalesce(); coords_t int64 [4, N] (any sign)"""
    lo = coords_t.min(dim=1, keepdim=True).values
    t = torch.sparse_coo_tensor(coords_t - lo, feats).coalesce()
    return (t.indices() + lo).t().contiguous(), t.values()


def _sorted_rows(coords, feats):
    """rows sorted by (b, x, y, z)"""
    c = coords.long()
    key = ((c[:, 3] * 4096 + c[:, 0] + 2048) * 4096 + c[:, 1] + 2048) * 4096 + c[:, 2] + 2048
    order = torch.argsort(key)
    return coords[order].int(), feats[order]


def upstream_reduction(feats, coords, dim):
    coords = coords.clone()
    coords[:, dim] = 0
    feats = torch.cat([torch.ones_like(feats[:, :1]), feats], dim=1)
    c, f = _coalesce(coords.t().long(), feats)
    return c, f[:, 1:] / f[:, :1]


def upstream_convolution(feats, coords, s, kernel, bias, stride, dim):
    ratio = torch.tensor(s) * stride
    stride_t = torch.tensor(s)
    kernels = torch.index_select(kernel, 0, torch.div(coords[:, dim], stride_t[dim]).trunc().long())
    feats = (feats.unsqueeze(dim=-1) * kernels).sum(1) + bias
    coords = coords.t().long().clone()
    coords[dim, :] = 0
    if stride > 1:
        coords[:3] = (torch.div(coords[:3], ratio[:, None]).trunc() * ratio[:, None]).long()
    return _coalesce(coords, feats)


def upstream_dense_convolution(feats, coords, s, kernel, bias, shape, offset, dim):
    bev_dims = list(R.bev_axes(dim))
    stride_t, shape_t = torch.tensor(s), torch.tensor(shape)
    offset_t = torch.tensor(list(offset) + [0])
    bev_shape = shape_t[bev_dims]
    kernels = torch.index_select(kernel, 0, torch.div(coords[:, dim], stride_t[dim]).trunc().long())
    sparse_features = (feats.unsqueeze(dim=-1) * kernels).sum(1) + bias
    sparse_coords = (coords - offset_t).t()[[3] + bev_dims].long()
    sparse_coords[1:] = torch.div(sparse_coords[1:], stride_t[bev_dims].unsqueeze(dim=-1)).trunc().long()
    batch_size = int(sparse_coords[0].max()) + 1
    flat = sparse_coords[0] * int(bev_shape.prod()) + sparse_coords[1] * int(bev_shape[1]) + sparse_coords[2]
    bev = torch.sparse_coo_tensor(flat[None], sparse_features, torch.Size([batch_size * int(bev_shape.prod()), sparse_features.size(-1)])).to_dense()
    return bev.view(batch_size, *bev_shape.tolist(), -1).permute(0, 3, 1, 2).contiguous()


def upstream_height_compression(feats, coords, s, shape, offset, dim):
    bev_dims = list(R.bev_axes(dim))
    stride_t, shape_t = torch.tensor(s), torch.tensor(shape)
    offset_t = torch.tensor(list(offset) + [0])
    bev_shape = shape_t[bev_dims + [dim]]
    c = (coords - offset_t).t()[[3] + bev_dims + [dim]].long()
    c[1:] = torch.div(c[1:], stride_t[bev_dims + [dim]].unsqueeze(dim=-1)).trunc().long()
    c[-1] = torch.clamp(c[-1], 0, int(bev_shape[-1]) - 1)
    flat = c[0] * int(bev_shape.prod()) + c[1] * int(bev_shape[1:].prod()) + c[2] * int(bev_shape[2]) + c[3]
    batch_size = int(c[0].max()) + 1
    bev = torch.sparse_coo_tensor(flat[None], feats, torch.Size([batch_size * int(bev_shape.prod()), feats.size(-1)])).to_dense()
    bev = bev.view(batch_size, *bev_shape.tolist(), -1)          # B, H, W, Z, C
    return bev.permute(0, 4, 3, 1, 2).contiguous().view(batch_size, -1, *bev_shape[:2].tolist())


def _same(a, b):
    assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-12, atol=0), float((a - b).abs().max())


@pytest.mark.parametrize('name', _names('reduction'))
def test_reduction_is_the_upstream_text(name):
    b = _built(name)
    oc, out, _, _ = R.reduction64(b['feats'], b['coords'], b['dim'])
    uc, uf = _sorted_rows(*upstream_reduction(b['feats'].double(), b['coords'], b['dim']))
    assert torch.equal(oc, uc)
    _same(out, uf)


@pytest.mark.parametrize('name', _names('convolution'))
def test_convolution_is_the_upstream_text(name):
    b = _built(name)
    bias = b['bias_t'].double() if b['bias'] else 0
    oc, out, _, cnt, _, _ = R.convolution64(b['feats'], b['coords'], b['s'], b['kernel'], b['bias_t'], b['stride'], b['dim'])
    uc, uf = _sorted_rows(*upstream_convolution(b['feats'].double(), b['coords'], b['s'], b['kernel'].double(), bias, b['stride'], b['dim']))
    assert torch.equal(oc, uc)
    _same(out, uf)
    if b['bias'] and b['nk'] > 1:
        assert int(cnt.max()) > 1, 'a cell fed by several rows carries several biases'


@pytest.mark.parametrize('name', _names('dense'))
def test_dense_convolution_is_the_upstream_text(name):
    b = _built(name)
    bias = b['bias_t'].double() if b['bias'] else 0
    out = R.dense_convolution64(b['feats'], b['coords'], b['s'], b['kernel'], b['bias_t'], b['shape'], b['offset'], b['dim'])[0]
    _same(out, upstream_dense_convolution(b['feats'].double(), b['coords'], b['s'], b['kernel'].double(), bias, b['shape'],
                                          b['offset'], b['dim']))


@pytest.mark.parametrize('name', _names('height'))
def test_height_compression_is_the_upstream_text(name):
    b = _built(name)
    out = R.height_compression64(b['feats'], b['coords'], b['s'], b['shape'], b['offset'], b['dim'])[0]
    _same(out, upstream_height_compression(b['feats'].double(), b['coords'], b['s'], b['shape'], b['offset'], b['dim']))


def test_the_cases_reach_their_edges():
    sizes = {c['n'] for c in R.CASES}
    assert set(R.SIZES) <= sizes
    for module in ('reduction', 'convolution', 'dense', 'height'):
        cs = [c for c in R.CASES if c['module'] == module]
        assert {c['dim'] for c in cs} == {0, 1, 2} and {(1, 1, 1), (2, 2, 1)} <= {c['s'] for c in cs}
        assert {F32, BF16, F16} == {c['dtype'] for c in cs} and {4, 20, 64} <= {c['c'] for c in cs}
        if module in ('convolution', 'dense'):
            assert {1, 3, 32, 33} <= {c['nk'] for c in cs} and {4, 32} <= {c['cout'] for c in cs}
        if module in ('reduction', 'convolution'):
            assert any(int(_built(c['name'])['coords'][:, :3].min()) < 0 for c in cs)
        if module in ('dense', 'height'):
            assert any(any(c['offset']) for c in cs)
    assert {1, 2} == {c['stride'] for c in R.CASES if c['module'] == 'convolution'}
    b = _built('dense-n65')
    cnt = R.dense_convolution64(b['feats'], b['coords'], b['s'], b['kernel'], 0, b['shape'], b['offset'], b['dim'])[2]
    cnt = cnt.view(3, 5, 7)
    assert int(cnt[0, 0, 0]) == 3 and int(cnt[2, 4, 6]) == 1 and int(cnt[1].sum()) == 0      # a full column, a column of one, no batch 1
    b = _built('height-n129')
    assert int(R.height_compression64(b['feats'], b['coords'], b['s'], b['shape'], b['offset'], b['dim'])[2].max()) > 1


# ---- degraded variants ---------------------------------------------------------------------------------------------------------

def _densify(oc, vals, lo=-64, size=128):
    """sparse rows on a dense [B, size, size, size, C] grid (so that two results with different row sets compare)"""
    out = torch.zeros(3, size, size, size, vals.shape[1], dtype=vals.dtype)
    c = oc.long()
    out[c[:, 3], c[:, 0] - lo, c[:, 1] - lo, c[:, 2] - lo] = vals
    return out


def _rejects(name, variant):
    """True if the bound of the case's module, taken at the honest reference, rejects the degraded float64 evaluation"""
    b = _built(name)
    m, v = b['module'], R.DEGRADED[variant]
    if m == 'reduction':
        oc, ref, mag, cnt = R.reduction64(b['feats'], b['coords'], b['dim'])
        oc2, bad, _, _ = R.reduction64(b['feats'], b['coords'], b['dim'], variant=v)
        bd = R.mean_bound(ref, b['dtype'])
        return not R.check(_densify(oc2, bad, size=64, lo=-32), _densify(oc, ref, size=64, lo=-32), _densify(oc, bd, size=64, lo=-32))[0]
    if m == 'convolution':
        oc, ref, mag, cnt, inv, z = R.convolution64(b['feats'], b['coords'], b['s'], b['kernel'], b['bias_t'], b['stride'], b['dim'])
        oc2, bad = R.convolution64(b['feats'], b['coords'], b['s'], b['kernel'], b['bias_t'], b['stride'], b['dim'], variant=v)[:2]
        r = CR.rel_err(R.honest_rows_fp32(b['feats'], b['kernel'], b['bias_t'], z, inv, len(cnt)), ref, mag)
        bd = R.store_rounding(CR.bound('f32', mag, r), ref, b['dtype'])
        return not R.check(_densify(oc2, bad, size=64, lo=-32), _densify(oc, ref, size=64, lo=-32), _densify(oc, bd, size=64, lo=-32))[0]
    if m == 'dense':
        ref, mag, cnt, cell, z = R.dense_convolution64(b['feats'], b['coords'], b['s'], b['kernel'], b['bias_t'], b['shape'],
                                                       b['offset'], b['dim'])
        bad = R.dense_convolution64(b['feats'], b['coords'], b['s'], b['kernel'], b['bias_t'], b['shape'], b['offset'], b['dim'],
                                    variant=v, nb=3)[0]
        rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
        r = CR.rel_err(R.honest_rows_fp32(b['feats'], b['kernel'], b['bias_t'], z, cell, len(cnt)), rows(ref), rows(mag))
        return not R.check(bad, ref, R.store_rounding(CR.bound('f32', mag, r), ref, b['dtype']))[0]
    ref, mag, cnt = R.height_compression64(b['feats'], b['coords'], b['s'], b['shape'], b['offset'], b['dim'])
    bad = R.height_compression64(b['feats'], b['coords'], b['s'], b['shape'], b['offset'], b['dim'], variant=v, nb=3)[0]
    return not R.check(bad, ref, R.dense_store_bound(ref, mag, cnt, b['dtype']))[0]


_REJECTED = [
    ('bias added once per cell', 'conv-n65'), ('bias added once per cell', 'dense-n65'), ('bias added once per cell', 'conv-stride2'),
    ('reduction as a sum', 'red-n63'), ('reduction as a sum', 'red-n1500'),
    ('height index not divided by the stride', 'conv-n129'), ('height index not divided by the stride', 'dense-n129'),
    ('offset subtracted for the kernel index', 'dense-n65'), ('offset subtracted for the kernel index', 'dense-n129'),
    ('channel index w * C + c', 'height-n63'), ('channel index w * C + c', 'height-n129'),
    ('u and v swapped', 'dense-n65'), ('u and v swapped', 'height-n129'),
    ('floor instead of trunc on a negative coordinate', 'conv-stride2'), ('floor instead of trunc on a negative coordinate', 'conv-stride2-s2'),
    ('a dropped last row', 'red-n63'), ('a dropped last row', 'conv-n65'), ('a dropped last row', 'dense-n65'),
    ('a dropped last row', 'height-n63'),
]


@pytest.mark.parametrize('variant,name', _REJECTED)
def test_the_bounds_reject_the_degraded_variant(variant, name):
    assert _rejects(name, variant), '%s passes the bound of %s' % (variant, name)


def test_every_degraded_variant_is_judged():
    assert {v for v, _ in _REJECTED} == set(R.DEGRADED)


# ---- headroom --------------------------------------------------------------------------------------------------------------------

def _engine(c):
    return c['module'] in ('convolution', 'dense') and c['nk'] <= R.ENGINE_MAX_K and c['stride'] == 1


@pytest.mark.parametrize('name', [c['name'] for c in R.CASES if _engine(c)])
def test_honest_fp32_convolution_keeps_half_the_bound(name):
    b = _built(name)
    dtype, nk, n = b['dtype'], b['nk'], b['n']
    if b['module'] == 'convolution':
        _, out, _, cnt, group, z = R.convolution64(b['feats'], b['coords'], b['s'], b['kernel'], b['bias_t'], 1, b['dim'])
    else:
        out, _, cnt, group, z = R.dense_convolution64(b['feats'], b['coords'], b['s'], b['kernel'], b['bias_t'], b['shape'], b['offset'], b['dim'])
    n_out = len(cnt)
    nbr = R.neighbour_table(group, z, nk, n_out)
    kr = b['kernel'].to(dtype).float()
    g = torch.randn(n_out, b['cout'], generator=torch.Generator().manual_seed(5)).to(dtype)
    for cin, cout, src, role, n_rows in ((b['c'], b['cout'], b['feats'], 'fwd', n_out), (b['cout'], b['c'], g, 'inv', n)):
        fam = R.conv_family(cin, cout, dtype, n_rows, nk)
        running = fam[0] == 'u2mkd_conv_forward_sorted'
        ref, mag, part = CR.reference(src, kr, nbr, n, role, nominal=dtype == F16)
        plain = CR.reference(src, kr, nbr, n, role)[1] if dtype == F16 else mag
        r = CR.rel_err(CR.honest_fp32(src, kr, nbr, n, role, running=running), ref, plain)
        other = CR.honest_fp32(src, kr, nbr, n, role, descending=True, running=running)
        bias = role == 'fwd' and b['bias']
        stored = bias or dtype != F32
        if bias:      # the cell's m * bias added exactly, one rounding
            m = cnt[:, None] * b['bias_t'].double()
            other = (other.double() + m).float()
            ref = ref + m
        if dtype != F32:
            other = other.to(dtype)
        bm = cnt[:, None] * b['bias_t'].double().abs() if bias else None
        if fam[1] in ('f16x2', 'x3'):      # the arithmetic's own term is no matter of order: judged on the accumulation term alone
            kind = 'f32'
        else:
            kind = fam[1]
        whole = R.conv_bound(kind, mag, r, ref, part, dtype, nk, bm)
        ok, worst = R.check(other, ref, R.conv_bound(kind, mag, r, ref, part, dtype, nk, bm, margin=2.0) if stored else whole)
        print('\n[bev-host] %s %s %s: honest / bound %.3f' % (name, role, fam[1], R.check(other, ref, whole)[1]))
        assert ok and (stored or worst <= 0.5), (name, role, worst)


@pytest.mark.parametrize('name', _names('reduction'))
def test_honest_mean_keeps_its_bound(name):
    b = _built(name)
    _, ref, _, cnt = R.reduction64(b['feats'], b['coords'], b['dim'])
    honest = ref.to(b['dtype'])                          # summed wider, rounded once
    ok, worst = R.check(honest, ref, R.mean_bound(ref, b['dtype']))
    print('\n[bev-host] %s: honest / bound %.3f' % (name, worst))
    assert ok and (b['dtype'] != F32 or worst <= 0.5)


@pytest.mark.parametrize('name', _names('height'))
def test_honest_fp32_store_keeps_its_bound(name):
    b = _built(name)
    zz, dim = b['shape'][b['dim']], b['dim']
    ref, mag, cnt = R.height_compression64(b['feats'], b['coords'], b['s'], b['shape'], b['offset'], dim)
    wq = torch.div(b['coords'][:, dim].long() - b['offset'][dim], b['s'][dim], rounding_mode='trunc').clamp(0, zz - 1)
    cell, h, w = R.cells(b['coords'], b['s'], b['shape'], b['offset'], dim)
    acc = torch.zeros(3 * h * w * zz if b['n'] > 1 else h * w * zz, b['c'])
    x = b['feats'].float()
    for r in range(b['n']):                               # ascending row order, fp32
        acc[cell[r] * zz + wq[r]] += x[r]
    nb = ref.shape[0]
    honest = acc.view(nb, h, w, zz, -1).permute(0, 4, 3, 1, 2).reshape(nb, -1, h, w).to(b['dtype'])
    ok, worst = R.check(honest, ref, R.dense_store_bound(ref, mag, cnt, b['dtype']))
    print('\n[bev-host] %s: honest / bound %.3f' % (name, worst))
    assert ok
