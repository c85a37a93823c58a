"""Every kernel form of the sparse convolution's forward and input gradient against float64, elementwise, under the derived
bounds of tests/conv_fwd_f64_ref.py: the tile kernel in its three fp32-row arithmetics (f16x2, bf16x3, f32 MFMA) on all 12
instantiations, its folded eval-mode epilogue and its 16-bit forms; the offset walkers conv_os2 / conv_os3 behind
u2mkd_conv_forward_sorted; the f32, bf16x3, f16x2 and 16-bit pair kernels with their gather-sums and the gather-sum epilogue;
and the dispatch itself through ConvolutionFunction and conv_eval_affine.

The first part runs SYNTHETIC neighbour tables through the C ABI (TileSchedule / PairSchedule built from them), so that the
schedules reach what real scenes do not: 64-row tile tails (n_out of 1, 63, 64, 65, 129), offsets of 0, 1, 63 .. 129 and 700
pairs (the padding to 128), n_in != n_out down to one input row, tiles cut into halves and quarters, a grid clamped to the
resident slots, more than 2048 pair tiles.  Each case asserts FROM WHAT IT READ BACK (sch.items, ps.meta, ps.tile_k) that it
reached its edge.  Every launch writes into NaN-prefilled outputs over a NaN-prefilled pair scratch, is repeated bitwise, and
rows without a neighbour must be exactly zero (exactly shift (+ res) under the epilogue).
tests/test_host_conv_fwd_bound.py shows on the same inputs what the bounds reject."""
import math
import os
import types

import pytest
import torch

import conv_fwd_f64_ref as R

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
TAG = {BF16: '_bf16', F16: '_f16'}
ARITH = {'f32': 1, 'x3': 2, 'f16x2': 4, BF16: 3, F16: 5}       # u2mkd_weight_fragments' codes
TILE_SHAPES = [(ci, co) for co in (32, 64) for ci in (32, 64, 96, 128)] + [(ci, co) for co in (96, 128) for ci in (32, 64)]


def _lg(v):
    return math.log2(v) if v > 0 else float('-inf')


@pytest.fixture(scope='module')
def L(hip):
    if os.environ.get('U2MKD_CONV_ARITH') or os.environ.get('U2MKD_CONV_SCHEDULE'):
        pytest.skip('U2MKD_CONV_ARITH / U2MKD_CONV_SCHEDULE override the default dispatch')
    return hip


@pytest.fixture(scope='module')
def F(L):
    from u2mkd_amd.torchsparse.nn import functional as F
    return F


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a device fault: nothing else of this session may use the GPU
        pytest.exit('GPU fault in %s: %s' % (what, e), returncode=3)


# ---- tables, schedules and references, built once per module -------------------------------------------------------------------

_TABLES, _CASES = {}, {}


def _table(F, name):
    """(nbr on the device, n_in, TileSchedule, PairSchedule) of a named synthetic pattern"""
    hit = _TABLES.get(name)
    if hit is None:
        nbr, n_in = R.table(name)
        assert int(nbr.max()) < n_in and int(nbr.min()) >= -1                     # (checked before any kernel reads it)
        dev = nbr.cuda()
        hit = _TABLES[name] = (dev, n_in, F.TileSchedule(dev), F.PairSchedule(dev, n_in))
        _sync('the schedules of ' + name)
    return hit


def _case(name, role, ca, cb, spread, dtype=F32, running=False):
    """device tensors of a case and its float64 reference: (x, w, ref, mag, part, r); 16-bit: float64 of the ROUNDED rows, weights.
    running: r on the running chain of the offset walkers (conv_fwd_f64_ref.honest_fp32)"""
    key = (name, role, ca, cb, spread, dtype, running)
    hit = _CASES.get(key)
    if hit is None:
        c = R.make_case(name, role, ca, cb, spread, dtype)
        x, w, nbr = c['x'].cuda(), c['w'].cuda(), c['nbr'].cuda()
        hit = (x, w) + _reference(x, w, nbr, c['n_in'], role, dtype, running)
        if len(_CASES) > 64:
            _CASES.clear()
        _CASES[key] = hit
    return hit


def _reference(x, w, nbr, n_in, role, dtype, running=False):
    wr = w.to(dtype).float() if dtype != F32 else w
    ref, mag, part = R.reference(x, wr, nbr, n_in, role, nominal=dtype == F16)
    plain = R.reference(x, wr, nbr, n_in, role)[1] if dtype == F16 else mag
    r = R.rel_err(R.honest_fp32(x, wr, nbr, n_in, role, running=running), ref, plain)
    return ref, mag, part, r


def _fragments(L, w, arith):
    """both orientations of the MFMA-fragment image of kernel w [K, cin, cout]: [0] the forward's, [1] the input gradient's"""
    k, cin, cout = w.shape
    buf = torch.empty(2, L.load().u2mkd_weight_fragments_bytes(k, cin, cout, arith), dtype=torch.uint8, device='cuda')
    L.call('u2mkd_weight_fragments', L.ptr(w), k, cin, cout, 2, arith, L.ptr(buf), L.stream())
    return buf


def _row_major(w, role):
    """[K, cb, ca] fp32: the layout the f32 kernels read (rows = output columns, the reduction contiguous)"""
    return (w if role in R.TRANSPOSED else w.transpose(1, 2)).contiguous()


# ---- launches through the C ABI ----------------------------------------------------------------------------------------------

def _run_tiles(L, sch, x, w, role, arith, ep=None):
    """u2mkd_conv_forward_tiles (fp32 rows, arith explicit), _tiles_ep (ep = (scale, shift, res, relu)) or _tiles_bf16 / _f16"""
    assert role in ('fwd', 'flip')
    ca, cb = R.shape_of(w, role)
    k, flip = w.shape[0], int(role == 'flip')
    wf = _fragments(L, w, arith)[flip]
    out = torch.full((sch.n, cb), float('nan'), dtype=x.dtype, device='cuda')
    head = (L.ptr(x), x.shape[0], ca, L.ptr(wf), cb, L.ptr(sch.nbr_s), L.ptr(sch.order), L.ptr(sch.items), L.ptr(sch.n_items), sch.n, k, flip)
    if x.dtype != F32:
        name = 'u2mkd_conv_forward_tiles' + TAG[x.dtype]
        L.call(name, *head, L.ptr(out), L.stream())
    elif ep is not None:
        name = 'u2mkd_conv_forward_tiles_ep'
        L.call(name, *head, arith, L.ptr(ep[0]), L.ptr(ep[1]), L.ptr(ep[2]), int(ep[3]), L.ptr(out), L.stream())
    else:
        name = 'u2mkd_conv_forward_tiles'
        L.call(name, *head, arith, L.ptr(out), L.stream())
    _sync('%s %d -> %d' % (name, ca, cb))
    return out


def _run_sorted(L, sch, x, w, role):
    assert role in ('fwd', 'flip')
    ca, cb = R.shape_of(w, role)
    out = torch.full((sch.n, cb), float('nan'), device='cuda')
    L.call('u2mkd_conv_forward_sorted', L.ptr(x), x.shape[0], ca, L.ptr(_row_major(w, role)), cb, L.ptr(sch.nbr_s), L.ptr(sch.order),
           L.ptr(sch.tile_order), sch.n, w.shape[0], int(role == 'flip'), L.ptr(out), L.stream())
    _sync('u2mkd_conv_forward_sorted %d -> %d' % (ca, cb))
    return out


def _run_pairs(L, F, ps, x, w, role, form, variant=0, ep=None):
    """PairSchedule.run: form 'f32' (u2mkd_conv_forward_pairs, variant 32 | 64), 'x3', 'f16x2' or 'pair16' (by x's dtype), then the
    gather-sum (ep: u2mkd_pairs_gather_sum_ep).  The scratch rows y are prefilled with NaN of every row type (all bits set)."""
    assert role in ('fwd', 'inv', 'invT')
    ca, cb = R.shape_of(w, role)
    swap = role != 'fwd'
    n_rows = ps.n_in if swap else ps.n_out
    assert x.shape == ((ps.n_out if swap else ps.n_in), ca)
    F._scratch(ps.cap * cb * 4, x.device).fill_(255)
    out = torch.full((n_rows, cb), float('nan'), dtype=x.dtype, device='cuda')
    if form == 'f32':
        wt, frag = _row_major(w, role), False
    else:
        wt = _fragments(L, w, ARITH[x.dtype] if form == 'pair16' else ARITH[form])[1 if role in R.TRANSPOSED else 0]
        frag = {'x3': True, 'f16x2': 2, 'pair16': True}[form]
    ps.run(x, wt, cb, swap, out, variant=variant, fragments=frag, epilogue=ep)
    _sync('the pair kernels (%s) %d -> %d' % (form, ca, cb))
    return out


# ---- what a case reached -------------------------------------------------------------------------------------------------------

def _check_tile_edge(name, sch, nbr):
    n_items = int(sch.n_items)
    items = sch.items[:n_items].tolist()
    tiles = -(-sch.n // 64)
    lgs = {it & 3 for it in items}
    assert n_items >= tiles and {it >> 4 for it in items} == set(range(tiles))         # every tile has its work items
    if name == 'heavy':
        assert {1, 2} <= lgs, lgs                                                       # tiles cut into halves AND into quarters
        assert n_items == sum(1 << (it & 3) for it in items if (it >> 2) & 3 == 0)
    if name == 'many':
        # more work items than 256 CUs x 8 workgroups, beyond what any instantiation keeps resident: launch_tp clamps the grid
        # below the item count and the workgroups deal themselves several items each
        assert n_items > 2048, n_items
        assert sum(1 for it in items if it & 3 == 2) > 2048                             # (the quarters alone)
    if name.startswith('tails'):
        assert sch.n in R.TAILS and int(((nbr >= 0).sum(dim=0) == 0).sum()) > (0 if sch.n > 1 else -1)


def _check_pair_edge(name, ps, nbr):
    counts = R.pair_counts(nbr)
    padded = [-(-c // 128) * 128 for c in counts]
    meta = ps.meta.tolist()
    assert ps.nbsizes.tolist() == counts
    assert meta == [sum(padded), sum(padded) // 64] and meta[0] <= ps.cap
    tile_k = ps.tile_k[:meta[1]].tolist()
    assert [tile_k.count(k) for k in range(ps.k)] == [p // 64 for p in padded]           # the padded counts, per offset
    if name in ('ragged27', 'ragged8'):
        for c in ((0, 1, 63, 64, 65, 127, 128, 129, 700) if ps.k == 27 else (0, 1, 700)):
            assert c in counts
        assert ps.n_in != ps.n_out
    if name == 'ragged-one':
        assert ps.n_in == 1 and set(counts) == {0, 1}
    if name == 'many':
        assert meta[1] > 2048 and ps.cap // 64 > 2048, meta                              # a workgroup walks a run of tiles


def _judge(form, shape, name, role, spread, got, ref, bd, mag, r, dead_value=None, emag=None):
    """print the case's line, then: finite, inside the bound, rows without a neighbour exact (mag = the convolution's; emag =
    the magnitude the printed ratio is relative to under the epilogue)"""
    ok, over, rel = R.check(got, ref, bd, mag if emag is None else emag)
    print('\n[conv-f64] %s, %dx%d, %s %s, %s: r 2^%.1f  err/mag 2^%.1f  err/bound %.3f'
          % (form, shape[0], shape[1], name, role, spread, _lg(r), _lg(rel), over))
    assert bool(torch.isfinite(got).all()), (form, name, role)
    assert ok, '%s %s %s %s: largest err / bound %.3f (err / mag 2^%.1f, r 2^%.1f)' % (form, name, role, spread, over, _lg(rel), _lg(r))
    dead = (mag == 0).all(dim=1)
    if dead_value is None:
        assert int(torch.count_nonzero(got[dead])) == 0
    else:
        assert torch.equal(got[dead], dead_value[dead])
    return over


_SMALL_RUNS = [(n, 'rows') for n in R.SMALL] + [('ragged27', 'unit'), ('ragged27', 'tiny')]


def _tile_runs(F, L, ca, cb, kind, arith, dtype, runs, form):
    worst = 0.0
    for name, spread in runs:
        nbr, n_in, sch, ps = _table(F, name)
        _check_tile_edge(name, sch, nbr)
        for role in R.roles_of(name):
            x, w, ref, mag, part, r = _case(name, role, ca, cb, spread, dtype)
            got = _run_tiles(L, sch, x, w, role, arith)
            bd = R.bound(kind, mag, r, ref, part, dtype if dtype != F32 else None, nbr.shape[0])
            worst = max(worst, _judge(form, (ca, cb), name, role, spread, got, ref, bd, mag, r))
            assert torch.equal(got, _run_tiles(L, sch, x, w, role, arith))
    return worst


# ---- the tile kernel -----------------------------------------------------------------------------------------------------------

# (no f16x2 instantiation at cin 96: the default there is bf16x3)
_TILE_CASES = [(ca, cb, kind) for kind in ('f16x2', 'x3', 'f32') for ca, cb in TILE_SHAPES if not (kind == 'f16x2' and ca == 96)]


@pytest.mark.parametrize('ca,cb,kind', _TILE_CASES)
def test_tile_kernel_every_instantiation_and_arithmetic(L, F, ca, cb, kind):
    """u2mkd_conv_forward_tiles with arith 4, 2 and 1 passed explicitly, kflip 0 on every table and 1 on the symmetric ones"""
    lib = L.load()
    assert lib.u2mkd_conv_tiles_supported(ca, cb, 27) == 1 and R.tiles_supported(ca, cb)
    assert lib.u2mkd_conv_tiles_arith(ca, cb, 27) == (4 if ca != 96 else 2)
    assert R.family(ca, cb, F32, 30000, 27)[1] == ('f16x2' if ca != 96 else 'x3')
    _tile_runs(F, L, ca, cb, kind, ARITH[kind], F32, _SMALL_RUNS, 'tiles ' + kind)


@pytest.mark.parametrize('kind', ['f16x2', 'x3', 'f32'])
@pytest.mark.parametrize('ca,cb', [(64, 64), (32, 128)], ids=lambda v: str(v))
@pytest.mark.parametrize('name', ['heavy', 'many'])
def test_tile_kernel_split_tiles_and_clamped_grid(L, F, name, ca, cb, kind):
    _tile_runs(F, L, ca, cb, kind, ARITH[kind], F32, [(name, 'rows')], 'tiles ' + kind)


@pytest.mark.parametrize('dtype', [BF16, F16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('ca,cb', [(32, 32), (64, 64), (96, 64), (128, 32), (64, 128)], ids=lambda v: str(v))
def test_tile_kernel_16_bit_rows(L, F, ca, cb, dtype):
    runs = _SMALL_RUNS + ([('heavy', 'rows')] if (ca, cb) == (64, 64) else [])
    assert R.family(ca, cb, dtype, 30000, 27) == ('u2mkd_conv_forward_tiles' + TAG[dtype], 'tile16', None)
    _tile_runs(F, L, ca, cb, 'tile16', ARITH[dtype], dtype, runs, 'tiles' + TAG[dtype])


def _affine(cb, n, res, dev='cuda'):
    scale, shift, resid = (t.to(dev) for t in R.make_affine(cb, n))
    assert bool((scale > 0).any()) and bool((scale < 0).any())                          # a scale of mixed sign
    return scale, shift, (resid if res else None)


def _dead_value(shift, resid, relu, n):
    v = shift.expand(n, -1) + resid if resid is not None else shift.expand(n, -1).clone()
    return v.clamp(min=0) if relu else v


@pytest.mark.parametrize('res,relu', [(False, False), (False, True), (True, False), (True, True)], ids=lambda v: str(int(v)))
@pytest.mark.parametrize('ca,cb', [(64, 64), (96, 64), (32, 128)], ids=lambda v: str(v))
def test_tile_kernel_folded_epilogue(L, F, ca, cb, res, relu):
    """u2mkd_conv_forward_tiles_ep in the arithmetic the dispatch gives the shape (f16x2; bf16x3 at cin 96)"""
    kind = R.family(ca, cb, F32, 30000, 27)[1]
    for name, spread in [(n, 'rows') for n in R.SMALL]:
        nbr, n_in, sch, ps = _table(F, name)
        x, w, ref, mag, part, r = _case(name, 'fwd', ca, cb, spread)
        scale, shift, resid = _affine(cb, sch.n, res)
        got = _run_tiles(L, sch, x, w, 'fwd', ARITH[kind], ep=(scale, shift, resid, relu))
        want, emag = R.epilogue_f64(ref, mag, scale, shift, resid, relu)
        bd = R.epilogue_bound(R.bound(kind, mag, r), emag, scale, res)
        _judge('tiles_ep ' + kind, (ca, cb), name, 'res %d relu %d' % (res, relu), spread, got, want, bd, mag, r,
               dead_value=_dead_value(shift, resid, relu, sch.n), emag=emag)
        assert torch.equal(got, _run_tiles(L, sch, x, w, 'fwd', ARITH[kind], ep=(scale, shift, resid, relu)))


# ---- the offset walkers --------------------------------------------------------------------------------------------------------

_SORTED = [((4, 32), ('conv_os2', 32)), ((48, 16), ('conv_os2', 32)), ((20, 12), ('conv_os2', 32)), ((8, 20), ('conv_os2', 32)),
           ((64, 48), ('conv_os2', 64)), ((16, 128), ('conv_os3', 32, 'narrow'))]


@pytest.mark.parametrize('shape,form', _SORTED, ids=lambda v: str(v))
def test_sorted_walkers_conv_os2_and_narrow_conv_os3(L, F, shape, form):
    ca, cb = shape
    for name, spread in _SMALL_RUNS:
        nbr, n_in, sch, ps = _table(F, name)
        assert R.family(ca, cb, F32, sch.n, nbr.shape[0]) == ('u2mkd_conv_forward_sorted', 'f32', form)
        for role in R.roles_of(name):
            x, w, ref, mag, part, r = _case(name, role, ca, cb, spread, running=True)
            got = _run_sorted(L, sch, x, w, role)
            _judge('sorted %s' % (form,), shape, name, role, spread, got, ref, R.bound('f32', mag, r), mag, r)
            assert torch.equal(got, _run_sorted(L, sch, x, w, role))


def test_sorted_walker_wide_conv_os3_on_many_rows(L, F):
    nbr, n_in, sch, ps = _table(F, 'many')
    assert R.family(32, 256, F32, sch.n, 27) == ('u2mkd_conv_forward_sorted', 'f32', ('conv_os3', 32, 'wide'))
    x, w, ref, mag, part, r = _case('many', 'fwd', 32, 256, 'rows', running=True)
    got = _run_sorted(L, sch, x, w, 'fwd')
    _judge('sorted conv_os3 wide', (32, 256), 'many', 'fwd', 'rows', got, ref, R.bound('f32', mag, r), mag, r)
    assert torch.equal(got, _run_sorted(L, sch, x, w, 'fwd'))


# ---- the pair kernels ----------------------------------------------------------------------------------------------------------

_PAIR_RUNS = [(n, 'rows') for n in R.RAGGED + R.SYMMETRIC] + [('ragged27', 'unit')]


def _pair_runs(F, L, ca, cb, form, kind, dtype, runs, variant=0, label=None):
    for name, spread in runs:
        nbr, n_in, sch, ps = _table(F, name)
        _check_pair_edge(name, ps, nbr)
        for role in ('fwd', 'inv', 'invT'):
            x, w, ref, mag, part, r = _case(name, role, ca, cb, spread, dtype)
            got = _run_pairs(L, F, ps, x, w, role, form, variant)
            bd = R.bound(kind, mag, r, ref, part, dtype if dtype != F32 else None, nbr.shape[0])
            _judge(label or form, (ca, cb), name, role, spread, got, ref, bd, mag, r)
            assert torch.equal(got, _run_pairs(L, F, ps, x, w, role, form, variant))


@pytest.mark.parametrize('ca,cb,variant', [(136, 96, 32), (96, 100, 32), (192, 48, 32), (128, 136, 64)])
def test_f32_pair_kernel_and_gather_sum(L, F, ca, cb, variant):
    """u2mkd_conv_forward_pairs (launch_conv_pairs<32|64>) + u2mkd_pairs_gather_sum, both roles of the pair list"""
    assert R.family(ca, cb, F32, 3000, 27) == ('u2mkd_conv_forward_pairs', 'f32', variant)
    _pair_runs(F, L, ca, cb, 'f32', 'f32', F32, _PAIR_RUNS, variant, 'pairs f32<%d>' % variant)


_PX3 = [((32, 32), (128, 1)), ((96, 96), (96, 1)), ((128, 192), (192, 1)), ((64, 256), (256, 1)), ((256, 128), (128, 1)), ((256, 512), (128, 2))]


@pytest.mark.parametrize('form', ['f16x2', 'x3'])
@pytest.mark.parametrize('shape,tile', _PX3, ids=lambda v: str(v))
def test_fragment_pair_kernels_every_column_tile(L, F, shape, tile, form):
    """u2mkd_conv_forward_pairs_f16x2 / _x3 + the gather-sum: the 128-, 96-, 192- and 256-column tiles of conv_px3.hip, TL 1 and 2.
    ``tile`` says which instantiation a shape is in the list for, by the restatement of px3_shape in the reference module (the
    host test holds it to hand-written expectations); the library's ABI reports no instantiation, so nothing observed confirms it."""
    ca, cb = shape
    lib = L.load()
    assert lib.u2mkd_conv_pairs_x3_supported(ca, cb) == 1 and lib.u2mkd_conv_pairs_f16x2_supported(ca, cb) == 1
    assert R.px3_tile(ca, cb) == tile
    if ca * cb > 8192:
        assert R.family(ca, cb, F32, 3000, 27) == ('u2mkd_conv_forward_pairs_f16x2', 'f16x2', tile)
    _pair_runs(F, L, ca, cb, form, form, F32, _PAIR_RUNS, label='pairs ' + form)


@pytest.mark.parametrize('form', ['f16x2', 'x3', 'f32'])
def test_pair_kernels_beyond_2048_tiles(L, F, form):
    ca, cb = (128, 128) if form != 'f32' else (96, 100)
    nbr, n_in, sch, ps = _table(F, 'many')
    _check_pair_edge('many', ps, nbr)
    for role in ('fwd', 'inv'):
        x, w, ref, mag, part, r = _case('many', role, ca, cb, 'rows')
        got = _run_pairs(L, F, ps, x, w, role, form)
        _judge('pairs ' + form, (ca, cb), 'many', role, 'rows', got, ref, R.bound(form, mag, r), mag, r)
        assert torch.equal(got, _run_pairs(L, F, ps, x, w, role, form))


@pytest.mark.parametrize('res,relu', [(False, False), (False, True), (True, False), (True, True)], ids=lambda v: str(int(v)))
@pytest.mark.parametrize('ca,cb', [(128, 128), (96, 192)], ids=lambda v: str(v))
def test_gather_sum_folded_epilogue(L, F, ca, cb, res, relu):
    """u2mkd_pairs_gather_sum_ep over the f16x2 pair kernel's rows (what conv_eval_affine runs for a wide layer), both roles"""
    for name in R.RAGGED:
        nbr, n_in, sch, ps = _table(F, name)
        for role in ('fwd', 'invT'):
            x, w, ref, mag, part, r = _case(name, role, ca, cb, 'rows')
            scale, shift, resid = _affine(cb, ref.shape[0], res)
            got = _run_pairs(L, F, ps, x, w, role, 'f16x2', ep=(scale, shift, resid, relu))
            want, emag = R.epilogue_f64(ref, mag, scale, shift, resid, relu)
            bd = R.epilogue_bound(R.bound('f16x2', mag, r), emag, scale, res)
            _judge('gather_sum_ep f16x2', (ca, cb), name, '%s res %d relu %d' % (role, res, relu), 'rows', got, want, bd, mag, r,
                   dead_value=_dead_value(shift, resid, relu, ref.shape[0]), emag=emag)
            assert torch.equal(got, _run_pairs(L, F, ps, x, w, role, 'f16x2', ep=(scale, shift, resid, relu)))


@pytest.mark.parametrize('dtype', [BF16, F16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('shape,tile', [((96, 96), (96, 1)), ((160, 64), (128, 1)), ((256, 192), (192, 1))], ids=lambda v: str(v))
def test_pair_kernels_16_bit_rows(L, F, shape, tile, dtype):
    """u2mkd_conv_forward_pairs_bf16 / _f16 + u2mkd_pairs_gather_sum_bf16 / _f16"""
    ca, cb = shape
    assert R.family(ca, cb, dtype, 3000, 27) == ('u2mkd_conv_forward_pairs' + TAG[dtype], 'pair16', tile)
    _pair_runs(F, L, ca, cb, 'pair16', 'pair16', dtype, [(n, 'rows') for n in R.RAGGED], label='pairs' + TAG[dtype])


# ---- the dispatch: ConvolutionFunction and conv_eval_affine ----------------------------------------------------------------------

_KINDS = {'subm': (3, 1, False), 'down': (2, 2, False), 'up': (2, 2, True), 'k3s2': (3, 2, False)}
_SCENE = {}


def _scene(F, kind):
    """(coords, kernel map) of the 3000-voxel scene for one kind of layer"""
    hit = _SCENE.get(kind)
    if hit is None:
        from u2mkd_amd.synth import synth_batch
        coords = torch.from_numpy(synth_batch(3000, 1, seed=7)['coords']).cuda()
        ks, st, _ = _KINDS[kind]
        hit = _SCENE[kind] = (coords, F.build_kmap(coords, (1,) * 3, (ks,) * 3, (st,) * 3))
    return hit


class _Spy:
    """records the names of the C entries called while it is open"""

    def __init__(self, L):
        self.L, self.names = L, []

    def __enter__(self):
        self.orig = self.L.call
        self.L.call = lambda name, *a: (self.names.append(name), self.orig(name, *a))[1]
        return self

    def __exit__(self, *exc):
        self.L.call = self.orig

    def conv_entries(self):
        return [n for n in self.names if n.startswith('u2mkd_conv_forward')]


def _scene_rows(n, c, seed, dtype=F32):
    return R.make_rows('rows', n, c, dtype, seed).cuda()


_FN_CASES = [(kind, shape, F32) for kind in _KINDS for shape in [(64, 64), (64, 96), (128, 128), (48, 16), (128, 136)]] + \
            [(kind, shape, dt) for dt in (BF16, F16) for kind in _KINDS for shape in [(64, 64), (96, 96)]]


@pytest.mark.parametrize('kind,shape,dtype', _FN_CASES, ids=lambda v: str(v).replace('torch.', ''))
def test_convolution_function_forward_and_input_gradient(L, F, kind, shape, dtype):
    """ConvolutionFunction on a 3000-voxel scene, rows of a magnitude each: the forward and x.grad against float64 taken from
    km.nbr alone, under the bound of the arithmetic that conv_fwd_f64_ref.family predicts -- and the entries it predicts are the
    entries that ran (64 -> 96: f16x2 tiles forward, bf16x3 tiles for the input gradient; 48 -> 16: the sorted walkers ...)."""
    cin, cout = shape
    ks, st, transposed = _KINDS[kind]
    coords, km = _scene(F, kind)
    k = ks ** 3
    n_x, n_y = (km.n_out, km.n_in) if transposed else (km.n_in, km.n_out)
    w = R.make_weights(k, cin, cout, 'unit', seed=3).cuda()
    x = _scene_rows(n_x, cin, 11, dtype).float().requires_grad_(True)
    g = _scene_rows(n_y, cout, 12, dtype).float()
    wp = w.clone().requires_grad_(True)
    with _Spy(L) as spy:
        if dtype == F32:
            y = F.ConvolutionFunction.apply(x, wp, km, transposed)
        else:
            with torch.autocast('cuda', dtype=dtype):
                y = F.ConvolutionFunction.apply(x, wp, km, transposed)
        _sync('ConvolutionFunction.forward %s' % kind)
        fwd_entries, spy.names = spy.conv_entries(), []
        y.backward(g.to(y.dtype))
        _sync('ConvolutionFunction.backward %s' % kind)
        bwd_entries = spy.conv_entries()
    assert y.dtype == dtype and x.grad.dtype == F32
    fam_f = R.family(cin, cout, dtype, n_y, k)
    fam_b = R.family(cout, cin, dtype, n_x, k)
    assert fwd_entries == [fam_f[0]], (fwd_entries, fam_f)
    assert bwd_entries == [fam_b[0]], (bwd_entries, fam_b)
    nbr = km.nbr
    xs, gs = x.detach().to(dtype), g.to(dtype)
    for what, fam, got, src, role in (('forward', fam_f, y.detach(), xs, 'invT' if transposed else 'fwd'),
                                      ('x.grad', fam_b, x.grad.to(dtype), gs, 'fwdT' if transposed else 'inv')):
        ref, mag, part, r = _reference(src, w, nbr, km.n_in, role, dtype, running=fam[0] == 'u2mkd_conv_forward_sorted')
        bd = R.bound(fam[1], mag, r, ref, part, dtype if dtype != F32 else None, k)
        _judge('ConvolutionFunction %s %s %s' % (kind, what, fam[0][6:]), shape, 'scene', role, 'rows', got, ref, bd, mag, r)


@pytest.mark.parametrize('res', [False, True], ids=['nores', 'res'])
@pytest.mark.parametrize('kind', ['subm', 'down', 'up'])
@pytest.mark.parametrize('c', [64, 128])
def test_conv_eval_affine_matches_the_float64_epilogue(L, F, c, kind, res):
    """conv_eval_affine on a Conv3d + eval BatchNorm pair: the tile kernel's folded store (64 x 64) and the gather-sum's
    (128 x 128), plain, strided and transposed, with and without the residual"""
    from u2mkd_amd import torchsparse
    import u2mkd_amd.torchsparse.nn as spnn
    ks, st, transposed = _KINDS[kind]
    coords, km = _scene(F, kind)
    k = ks ** 3
    n_x, n_y = (km.n_out, km.n_in) if transposed else (km.n_in, km.n_out)
    conv = types.SimpleNamespace(kernel_size=ks, stride=st, dilation=1, bias=None, transposed=transposed,
                                 kernel=R.make_weights(k, c, c, 'unit', seed=5).cuda())
    bn = spnn.BatchNorm(c).cuda().eval()
    gen = torch.Generator().manual_seed(77)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(c, generator=gen))                     # mixed sign
        bn.bias.copy_(torch.randn(c, generator=gen))
        bn.running_mean.copy_(torch.randn(c, generator=gen))
        bn.running_var.copy_(torch.rand(c, generator=gen) * 4 + 0.05)
    scale, shift = F.eval_bn_affine(bn)
    x = _scene_rows(n_x, c, 21)
    resid = _scene_rows(n_y, c, 22) if res else None
    key_stride = (1, 1, 1)
    if transposed:
        t = torchsparse.SparseTensor(x, km.out_coords, stride=st)
        t.cmaps[key_stride] = coords
    else:
        t = torchsparse.SparseTensor(x, coords, stride=1)
    t.kmaps[(key_stride, (ks,) * 3, (st,) * 3, (1,) * 3)] = km
    with _Spy(L) as spy:
        out = F.conv_eval_affine(t, conv, scale, shift, True, resid)
        _sync('conv_eval_affine %s' % kind)
    assert out is not None, 'no folded form for %d x %d %s' % (c, c, kind)
    fam = R.family(c, c, F32, n_y, k)
    want_entries = ['u2mkd_conv_forward_tiles_ep'] if fam[0].endswith('tiles') else [fam[0], 'u2mkd_pairs_gather_sum_ep']
    ran = [n for n in spy.names if n.startswith('u2mkd_conv_forward') or 'gather_sum' in n]
    assert ran == want_entries, (ran, fam)
    role = 'invT' if transposed else 'fwd'
    ref, mag, part, r = _reference(x, conv.kernel, km.nbr, km.n_in, role, F32)
    want, emag = R.epilogue_f64(ref, mag, scale, shift, resid, True)
    bd = R.epilogue_bound(R.bound(fam[1], mag, r), emag, scale, res)
    _judge('conv_eval_affine %s %s' % (kind, fam[0][6:]), (c, c), 'scene', role, 'rows', out.F, want, bd, mag, r,
           dead_value=_dead_value(shift, resid, True, n_y), emag=emag)


# ---- the dense route: LinearFunction and PointwiseConvFunction -------------------------------------------------------------------

_DENSE_KIND = {'u2mkd_linear_forward': 'f32', 'u2mkd_linear_forward_x3': 'x3', 'u2mkd_linear_forward_f16x2': 'f16x2',
               'u2mkd_linear_forward_bf16': 'tile16', 'u2mkd_linear_forward_f16': 'tile16'}      # (16-bit: ONE rounding, at the store)
_DENSE_ROWS = 65                  # the smallest size that crosses a 64-row tile and leaves a one-row tail
_DENSE_CASES = [(fn, (64, 64), dt) for fn in ('linear', 'pointwise') for dt in (F32, BF16, F16)] + [('linear', (36, 20), F32)]


@pytest.mark.parametrize('fn,shape,dtype', _DENSE_CASES, ids=lambda v: str(v).replace('torch.', ''))
def test_linear_and_pointwise_conv_launch_the_dense_route(L, F, fn, shape, dtype):
    """LinearFunction / PointwiseConvFunction at 65 rows: the forward launches the entry _dense_route names, the backward ONE
    u2mkd_conv_wgrad_pairs[_bf16|_f16] and then the input gradient's entry (36 -> 20, no fragment shape: u2mkd_transpose_weights,
    then u2mkd_linear_forward); y and x.grad against float64 x @ W under the bound of the arithmetic the route names (a linear
    layer is the one-offset identity table), w.grad under wgrad_f64_ref's."""
    import wgrad_f64_ref as W
    cin, cout = shape
    n = _DENSE_ROWS
    nbr = torch.arange(n, dtype=torch.int32, device='cuda')[None]
    w = R.make_weights(1, cin, cout, 'unit', seed=9).cuda()                     # kernel layout [1, cin, cout]
    x = R.make_rows('unit', n, cin, dtype, 31).cuda().float().requires_grad_(True)
    g = R.make_rows('unit', n, cout, dtype, 32).cuda().float()
    wp = (w[0].t().contiguous() if fn == 'linear' else w[0].clone()).requires_grad_(True)       # nn.Linear: [out, in]
    apply = (lambda: F.LinearFunction.apply(x, wp, None)) if fn == 'linear' else (lambda: F.PointwiseConvFunction.apply(x, wp, None))
    with _Spy(L) as spy:
        if dtype == F32:
            y = apply()
        else:
            with torch.autocast('cuda', dtype=dtype):
                y = apply()
        _sync('%s forward' % fn)
        fwd, spy.names = [e for e in spy.names if 'weight_fragments' not in e], []
        y.backward(g.to(y.dtype))
        _sync('%s backward' % fn)
        bwd = [e for e in spy.names if 'weight_fragments' not in e and 'wgrad_plan' not in e]
    assert y.dtype == dtype and x.grad.dtype == F32
    rf, rb = F._dense_route(dtype, cin, cout), F._dense_route(dtype, cout, cin)
    assert fwd == [rf.entry], (fwd, rf)
    assert bwd == ['u2mkd_conv_wgrad_pairs' + TAG.get(dtype, '')] + ([] if rb.fragments else ['u2mkd_transpose_weights']) + [rb.entry], (bwd, rb)
    if shape == (36, 20):
        assert (rf.entry, rb.entry) == ('u2mkd_linear_forward', 'u2mkd_linear_forward') and not rf.fragments
    xs, gs = x.detach().to(dtype), g.to(dtype)
    for what, route, got, src, role in (('forward', rf, y.detach(), xs, 'fwd'), ('x.grad', rb, x.grad.to(dtype), gs, 'fwdT')):
        ref, mag, part, r = _reference(src, w, nbr, n, role, dtype)
        bd = R.bound(_DENSE_KIND[route.entry], mag, r, ref, part, dtype if dtype != F32 else None, 1)
        _judge('%s %s %s' % (fn, what, route.entry[6:]), shape, 'identity', role, 'unit', got, ref, bd, mag, r)
    # w.grad: dW = X^T dY in the kernel layout (nn.Linear: its transpose), fp32 whatever the rows
    pairs = torch.stack([nbr[0], nbr[0]], 1).contiguous()
    dw, mag = W.wgrad_f64(xs, gs, pairs, [n], 0)
    r = W.rel_err(W.honest_fp32(xs, gs, pairs, [n], 0), dw, mag)
    got = (wp.grad.t() if fn == 'linear' else wp.grad)[None]
    t = W.T_X3 if (dtype == F32 and W.family(cin, cout, dtype)[0] == 'x3') else W.T_EXACT
    ok, over, rel = W.check(got, dw, mag, t, r)
    print('[conv-f64] %s w.grad %dx%d: err/mag 2^%.1f  err/bound %.3f' % (fn, cin, cout, _lg(rel), over))
    assert wp.grad.dtype == F32 and ok, (fn, shape, dtype, over, rel)


@pytest.mark.parametrize('shape,dtype', [((64, 64), F32), ((96, 96), BF16)], ids=lambda v: str(v).replace('torch.', ''))
def test_convolution_function_at_64_offsets_launches_the_route(L, F, shape, dtype):
    """k = 64 (tests/conv_lk_tables.py 't64'), beyond the row mask of the tile schedule: 64 -> 64 on fp32 rows runs the offset-chunk
    kernel, 96 -> 96 under bf16 autocast keeps bf16 rows on the pair schedule -- forward and input gradient on the entry
    _conv_route names, the results finite and of the types of the k <= 31 test"""
    import conv_lk_tables as T
    cin, cout = shape
    nbr, n_in = T.make_table('t64')
    k, n_out = nbr.shape
    assert int(nbr.max()) < n_in and int(nbr.min()) >= -1
    km = F.KernelMap(nbr.cuda(), T.invert(nbr, n_in).cuda(), n_in, n_out, False, None)
    wp = R.make_weights(k, cin, cout, 'unit', seed=4).cuda().requires_grad_(True)
    x = R.make_rows('unit', n_in, cin, dtype, 41).cuda().float().requires_grad_(True)
    g = R.make_rows('unit', n_out, cout, dtype, 42).cuda().float()
    with _Spy(L) as spy:
        with torch.autocast('cuda', dtype=dtype, enabled=dtype != F32):
            y = F.ConvolutionFunction.apply(x, wp, km, False)
        _sync('ConvolutionFunction.forward k=64')
        fwd, spy.names = spy.conv_entries(), []
        y.backward(g.to(y.dtype))
        _sync('ConvolutionFunction.backward k=64')
        bwd = spy.conv_entries()
    rf, rb = F._conv_route(dtype, cin, cout, k, n_out), F._conv_route(dtype, cout, cin, k, n_in)
    assert fwd == [rf.entry] and bwd == [rb.entry], (fwd, bwd, rf, rb)
    assert rf.entry == ('u2mkd_conv_forward_lk' if dtype == F32 else 'u2mkd_conv_forward_pairs_bf16')
    assert y.dtype == dtype and x.grad.dtype == F32 and wp.grad.shape == (k, cin, cout)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(wp.grad).all())
