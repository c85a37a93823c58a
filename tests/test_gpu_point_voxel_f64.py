"""Every form of the point <-> voxel row movers (csrc/voxel.hip) against float64, element by element, inside the bound derived in
tests/point_voxel_f64_ref.py (no fitted constant, no element excluded, a zero bound asks for equality, NaN and fp16's inf compared by
class): through the C ABI u2mkd_segment_sum / u2mkd_segment_mean and their _bf16 / _f16 entries on the entry lists of
u2mkd_csr_build and u2mkd_devoxelize_plan, the atomic u2mkd_voxelize_forward / u2mkd_devoxelize_backward at both vector widths,
u2mkd_voxelize_backward and u2mkd_devoxelize_forward on the three row types, u2mkd_ti_weights; through the public API
F.spvoxelize / F.spdevoxelize (fp32, and 16-bit rows under autocast) and fusion._SegmentMap, outputs and gradients.
tests/test_host_point_voxel_bound.py shows on the host what that bound rejects.  Every figure is printed before it is asserted
(``pytest -s``); the largest err / bound per form and row type of a run is in NOTES N23."""
import contextlib

import pytest
import torch

import point_voxel_f64_ref as P

pytestmark = pytest.mark.gpu

SFX = {'f32': '', 'bf16': '_bf16', 'f16': '_f16'}
DT = tuple(P.DTYPES)
RATIOS = {}


@pytest.fixture(scope='module')
def F(hip):
    from u2mkd_amd.torchsparse.nn import functional as F
    yield F
    for (form, dt), r in sorted(RATIOS.items()):
        print('[N23 worst] %-34s %-4s err/bound %.3f' % (form, dt, r))


def _hold(form, dt, got, ref, bound, what):
    ok, ratio, err = P.compare(got, ref, bound, P.DTYPES[dt])
    print('[N23] %-34s %-4s %-40s err/bound %.3f err %.3g' % (form, dt, what, ratio, err))
    RATIOS[(form, dt)] = max(RATIOS.get((form, dt), 0.0), ratio)
    assert ok, '%s %s %s: err / bound = %.4g (err %.4g)' % (form, dt, what, ratio, err)


def _same(a, b):
    """bit-identical values (NaN in the same places)"""
    a, b = a.cpu(), b.cpu()
    return a.dtype == b.dtype and torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0))


def _garbage(n, c, dtype):
    """an output buffer that a CSR form has to overwrite completely"""
    return torch.full((n, c), 7.0, dtype=dtype, device='cuda')


def _csr_on_device(L, keys, nv):
    """u2mkd_csr_build; its live entries are the stable grouping (P.csr)"""
    k = keys.cuda().contiguous()
    e = k.numel()
    order = torch.empty(e, dtype=torch.int32, device='cuda')
    seg = torch.empty(nv + 1, dtype=torch.int32, device='cuda')
    ws = torch.empty(max(L.load().u2mkd_csr_workspace_bytes(e, nv), 16), dtype=torch.uint8, device='cuda')
    L.call('u2mkd_csr_build', L.ptr(k), e, nv, L.ptr(ws), L.ptr(order), L.ptr(seg), L.stream())
    want_order, want_seg = P.csr(keys, nv)
    assert torch.equal(seg.cpu(), want_seg) and torch.equal(order.cpu()[:want_order.numel()], want_order)
    return order, seg


def _devox_plan_on_device(L, idx8, w8, nv):
    """u2mkd_devoxelize_plan; its live entries are P.devoxelize_plan's"""
    i, w = idx8.cuda().contiguous(), w8.cuda().contiguous()
    n = i.shape[0]
    erow = torch.empty(8 * n, dtype=torch.int32, device='cuda')
    ew = torch.empty(8 * n, dtype=torch.float32, device='cuda')
    seg = torch.empty(nv + 1, dtype=torch.int32, device='cuda')
    ws = torch.empty(max(L.load().u2mkd_devoxelize_plan_workspace_bytes(n, nv), 16), dtype=torch.uint8, device='cuda')
    L.call('u2mkd_devoxelize_plan', L.ptr(i), L.ptr(w), n, nv, L.ptr(ws), L.ptr(erow), L.ptr(ew), L.ptr(seg), L.stream())
    want_row, want_w, want_seg = P.devoxelize_plan(idx8, w8, nv)
    e = want_row.numel()
    assert torch.equal(seg.cpu(), want_seg) and torch.equal(erow.cpu()[:e], want_row) and torch.equal(ew.cpu()[:e], want_w)
    return erow, ew, seg


def _segment(L, dt, src, erow, ew, seg, nv, mean, counts=None):
    """one CSR form, run twice into overwritten buffers: the two runs are equal"""
    outs = []
    for _ in range(2):
        out = _garbage(nv, src.shape[1], src.dtype)
        if counts is not None:
            L.call('u2mkd_segment_mean' + SFX[dt], L.ptr(src), src.shape[1], L.ptr(erow), L.ptr(seg), L.ptr(counts), nv, L.ptr(out),
                   L.stream())
        else:
            L.call('u2mkd_segment_sum' + SFX[dt], L.ptr(src), src.shape[1], L.ptr(erow), L.ptr(ew), L.ptr(seg), nv, int(mean),
                   L.ptr(out), L.stream())
        outs.append(out)
    assert _same(outs[0], outs[1])
    return outs[0]


# ---- the CSR forms through the C ABI ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('entry', ['segment_sum mean=1', 'segment_mean counts=histogram', 'segment_sum mean=0'])
def test_segment_forms_on_the_voxelize_layouts(F, hip, entry, dt):
    L, dtype = hip, P.DTYPES[dt]
    for lay in P.VOX_LAYOUTS:
        idx, nv = P.vox_layout(lay)
        order, seg = _csr_on_device(L, idx, nv)
        for c in P.widths(dtype, vec4_only=True):
            for kind in P.kinds(dtype, c):
                if kind == 'overflow' and entry == 'segment_sum mean=1':
                    continue        # (the overflowing mean divides by halved counts: the form below)
                case = P.vox_case(lay, c, kind, dtype)
                x = case['x'].cuda()
                what = '%s c=%d %s%s' % (lay, c, kind, ' (halved counts)' if kind == 'overflow' and entry.startswith('segment_mean') else '')
                if entry == 'segment_sum mean=0':
                    _hold(entry, dt, _segment(L, dt, x, order, None, seg, nv, 0), case['sum'], case['sum_b'], what)
                    continue
                counts = case['counts'].cuda() if entry.startswith('segment_mean') else None
                got = _segment(L, dt, x, order, None, seg, nv, 1, counts)
                _hold(entry, dt, got, case['mean'], case['mean_b'], what)
                if kind != 'overflow':
                    # counts = the histogram: the divisor is the segment length, and the two entries agree bit for bit
                    assert _same(got, _segment(L, dt, x, order, None, seg, nv, 1, None if counts is not None else case['counts'].cuda()))
                if dt == 'f32':
                    # the claim in segment_sum_kernel: bit-identical to the in-order out[idx[i]] += x[i] / counts[idx[i]] in fp32
                    loop = P.segment_fp32(case['x'], case['order'], None, case['seg'], True, case['counts'], dtype, 'asc')
                    assert _same(got, loop), what


@pytest.mark.parametrize('dt', DT)
def test_segment_mean_with_counts_that_are_not_the_histogram(F, hip, dt):
    """twice the histogram, and one voxel that has points but counts = 0: the mean divides by counts[v] and that voxel stays 0"""
    L, dtype = hip, P.DTYPES[dt]
    for lay in ('V1s', 'V1r', 'V3'):
        idx, nv = P.vox_layout(lay)
        order, seg = _csr_on_device(L, idx, nv)
        for c in (4, 32):
            case = P.vox_case(lay, c, 'randn', dtype, 'twice')
            got = _segment(L, dt, case['x'].cuda(), order, None, seg, nv, 1, case['counts'].cuda())
            _hold('segment_mean counts=2 x histogram', dt, got, case['mean'], case['mean_b'], '%s c=%d' % (lay, c))
            dead = (case['counts'] == 0) & (case['seg'][1:] > case['seg'][:-1])
            assert int(dead.sum()) == 1 and float(got.cpu()[dead].float().abs().max()) == 0.0


@pytest.mark.parametrize('dt', DT)
def test_segment_sum_with_entry_weights(F, hip, dt):
    """mean = 0 with entry_w, on the entry lists of u2mkd_devoxelize_plan (devoxelize's backward as the models run it)"""
    L, dtype = hip, P.DTYPES[dt]
    for wkind in P.WKINDS:
        idx8, w8 = P.devox_layout(wkind)
        erow, ew, seg = _devox_plan_on_device(L, idx8, w8, P.DEVOX_NV)
        for c in P.widths(dtype, vec4_only=True):
            for kind in P.kinds(dtype, c):
                case = P.devox_case(wkind, c, kind, dtype)
                got = _segment(L, dt, case['g'].cuda(), erow, ew, seg, P.DEVOX_NV, 0)
                _hold('segment_sum mean=0 entry_w', dt, got, case['bwd'], case['bwd_b'], '%s c=%d %s' % (wkind, c, kind))


# ---- the atomic forms (fp32; VEC = 4 at c % 4 == 0, VEC = 1 otherwise) ----------------------------------------------------------

@pytest.mark.parametrize('vec', [1, 4])
def test_voxelize_forward_atomic(F, hip, vec):
    L = hip
    for lay, cmode in [(lay, 'hist') for lay in P.VOX_LAYOUTS] + [('V1r', 'twice'), ('V3', 'twice')]:
        for c in [c for c in P.WIDTHS32 if (c % 4 == 0) == (vec == 4)]:
            for kind in P.KINDS if cmode == 'hist' else ('randn',):
                case = P.vox_case(lay, c, kind, torch.float32, cmode)
                out = torch.zeros(case['nv'], c, device='cuda')
                x, idx, counts = case['x'].cuda(), case['idx'].cuda(), case['counts'].cuda()
                L.call('u2mkd_voxelize_forward', L.ptr(x), L.ptr(idx), L.ptr(counts), idx.numel(), case['nv'], c, L.ptr(out), L.stream())
                _hold('voxelize_forward atomic VEC=%d' % vec, 'f32', out, case['mean'], case['mean_b'], '%s %s c=%d %s' % (lay, cmode, c, kind))


@pytest.mark.parametrize('vec', [1, 4])
def test_devoxelize_backward_atomic(F, hip, vec):
    L = hip
    for wkind in P.WKINDS:
        for c in [c for c in P.WIDTHS32 if (c % 4 == 0) == (vec == 4)]:
            for kind in P.KINDS:
                case = P.devox_case(wkind, c, kind, torch.float32)
                out = torch.zeros(case['nv'], c, device='cuda')
                g, idx8, w8 = case['g'].cuda(), case['idx8'].cuda(), case['w8'].cuda()
                L.call('u2mkd_devoxelize_backward', L.ptr(g), L.ptr(idx8), L.ptr(w8), idx8.shape[0], case['nv'], c, L.ptr(out), L.stream())
                _hold('devoxelize_backward atomic VEC=%d' % vec, 'f32', out, case['bwd'], case['bwd_b'], '%s c=%d %s' % (wkind, c, kind))


# ---- the gathers through the C ABI --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dt', DT)
def test_voxelize_backward(F, hip, dt):
    L, dtype = hip, P.DTYPES[dt]
    for lay, cmode in [(lay, 'hist') for lay in P.VOX_LAYOUTS] + [('V1r', 'twice'), ('V3', 'twice')]:
        for c in P.widths(dtype):
            for kind in P.KINDS if cmode == 'hist' else ('randn',):
                case = P.vox_case(lay, c, kind, dtype, cmode)
                n = case['idx'].numel()
                out = _garbage(n, c, dtype)
                g, idx, counts = case['g'].cuda(), case['idx'].cuda(), case['counts'].cuda()
                L.call('u2mkd_voxelize_backward' + SFX[dt], L.ptr(g), L.ptr(idx), L.ptr(counts), n, case['nv'], c, L.ptr(out), L.stream())
                _hold('voxelize_backward', dt, out, case['bwd'], case['bwd_b'], '%s %s c=%d %s' % (lay, cmode, c, kind))


@pytest.mark.parametrize('dt', DT)
def test_devoxelize_forward(F, hip, dt):
    """(every index < nv: u2mkd_devoxelize_forward has no nv argument -- the precondition recorded in NOTES N23)"""
    L, dtype = hip, P.DTYPES[dt]
    for wkind in P.WKINDS:
        for c in P.widths(dtype):
            for kind in P.kinds(dtype, c):
                case = P.devox_case(wkind, c, kind, dtype)
                assert int(case['idx8'].max()) < case['nv']
                out = _garbage(P.DEVOX_N, c, dtype)
                f, idx8, w8 = case['f'].cuda(), case['idx8'].cuda(), case['w8'].cuda()
                L.call('u2mkd_devoxelize_forward' + SFX[dt], L.ptr(f), L.ptr(idx8), L.ptr(w8), P.DEVOX_N, c, L.ptr(out), L.stream())
                _hold('devoxelize_forward', dt, out, case['fwd'], case['fwd_b'], '%s c=%d %s' % (wkind, c, kind))


@pytest.mark.parametrize('scale', P.TI_SCALES)
def test_ti_weights(F, hip, scale):
    L = hip
    case = P.ti_case(scale)
    n = case['coords'].shape[0]
    w = _garbage(n, 8, torch.float32)
    i8 = torch.full((n, 8), 77, dtype=torch.int32, device='cuda')
    coords, idx = case['coords'].cuda(), case['idx_kn'].cuda()
    L.call('u2mkd_ti_weights', L.ptr(coords), L.ptr(idx), n, float(scale), L.ptr(w), L.ptr(i8), L.stream())
    _hold('ti_weights', 'f32', w, case['ref'], case['bound'], 'scale=%d' % scale)
    assert torch.equal(i8.cpu(), case['idx_kn'].t().int())
    w2, i2 = F.ti_weights_n8(coords, idx, scale)
    assert _same(w2, w) and torch.equal(i2, i8)
    assert _same(F.calc_ti_weights(coords, idx, scale), w.t())


# ---- the public API: outputs and gradients ------------------------------------------------------------------------------------

def _amp(dtype):
    return contextlib.nullcontext() if dtype == torch.float32 else torch.autocast('cuda', dtype=dtype)


def _spvoxelize(F, case, dt, out_dtype, what):
    """F.spvoxelize forward and .backward on one case whose values the row type ``dt`` holds: fp32 tensors in, as the models pass
    them; the output in ``out_dtype``"""
    dtype = P.DTYPES[dt]
    x = case['x'].float().cuda().requires_grad_(True)
    with _amp(dtype):
        out = F.spvoxelize(x, case['idx'].cuda(), case['counts'].cuda())
    assert out.dtype == out_dtype, (what, out.dtype)
    odt = {v: k for k, v in P.DTYPES.items()}[out_dtype]
    if out_dtype == dtype:
        ref, bound, gref, gbound = case['mean'], case['mean_b'], case['bwd'], case['bwd_b']
    else:       # fp32 rows from values a 16-bit type holds: the fp32 bound of the same references
        (ref, e), (gref, ge) = P.voxelize_full(case['x'], case['idx'], case['counts']), P.voxelize_bwd_full(case['g'], case['idx'], case['counts'])
        bound, gbound = P.stored(e, ref, out_dtype), P.stored(ge, gref, out_dtype)
    _hold('F.spvoxelize', odt, out.detach(), ref, bound, what)
    out.backward(case['g'].to(out_dtype).cuda())
    assert x.grad.dtype == torch.float32
    _hold('F.spvoxelize backward', odt, x.grad.to(out_dtype), gref, gbound, what)


def test_spvoxelize_fp32(F):
    for lay in P.VOX_LAYOUTS:
        for c in P.WIDTHS32:
            for kind in P.KINDS:
                _spvoxelize(F, P.vox_case(lay, c, kind, torch.float32), 'f32', torch.float32, '%s c=%d %s' % (lay, c, kind))


@pytest.mark.parametrize('dt', ['bf16', 'f16'])
def test_spvoxelize_under_autocast(F, dt):
    dtype = P.DTYPES[dt]
    for lay in P.VOX_LAYOUTS:
        for c in (16, 48):
            for kind in P.kinds(dtype, c):
                _spvoxelize(F, P.vox_case(lay, c, kind, dtype), dt, dtype, '%s c=%d %s' % (lay, c, kind))
        # the 4-channel coordinate means stay fp32 under autocast (SphereFormer quantises them into windows)
        _spvoxelize(F, P.vox_case(lay, 4, 'randn', dtype), dt, torch.float32, '%s c=4 stays fp32' % lay)


@pytest.mark.parametrize('dt', DT)
def test_spvoxelize_with_counts_that_are_not_the_histogram(F, dt):
    """F.spvoxelize divides by the counts it is given, at c % 4 == 0 as at c % 4 != 0, and its backward is the gradient of that"""
    dtype = P.DTYPES[dt]
    for lay in ('V1s', 'V1r', 'V3'):
        for c in (4, 32):
            out_dtype = dtype if c >= 16 else torch.float32
            _spvoxelize(F, P.vox_case(lay, c, 'randn', dtype, 'twice'), dt, out_dtype, '%s c=%d counts=2 x histogram' % (lay, c))


def _spdevoxelize(F, case, dt, out_dtype, what, i64=False):
    dtype = P.DTYPES[dt]
    f = case['f'].float().cuda().requires_grad_(True)
    idx8 = case['idx8'].long().cuda() if i64 else case['idx8'].cuda()
    with _amp(dtype):
        out = F.spdevoxelize(f, idx8, case['w8'].cuda())
    assert out.dtype == out_dtype, (what, out.dtype)
    odt = {v: k for k, v in P.DTYPES.items()}[out_dtype]
    if out_dtype == dtype:
        ref, bound, gref, gbound = case['fwd'], case['fwd_b'], case['bwd'], case['bwd_b']
    else:
        (ref, e), (gref, ge) = P.devoxelize_full(case['f'], case['idx8'], case['w8']), P.segment_full(case['g'], *case['plan'])
        bound, gbound = P.stored(e, ref, out_dtype), P.stored(ge, gref, out_dtype)
    _hold('F.spdevoxelize', odt, out.detach(), ref, bound, what)
    out.backward(case['g'].to(out_dtype).cuda())
    assert f.grad.dtype == torch.float32
    _hold('F.spdevoxelize backward', odt, f.grad.to(out_dtype), gref, gbound, what)


@pytest.mark.parametrize('i64', [False, True])
def test_spdevoxelize_fp32(F, i64):
    for wkind in P.WKINDS:
        for c in P.WIDTHS32:
            for kind in P.KINDS:
                _spdevoxelize(F, P.devox_case(wkind, c, kind, torch.float32), 'f32', torch.float32,
                              '%s c=%d %s %s' % (wkind, c, kind, 'int64' if i64 else 'int32'), i64)


@pytest.mark.parametrize('dt', ['bf16', 'f16'])
def test_spdevoxelize_under_autocast(F, dt):
    dtype = P.DTYPES[dt]
    for wkind in P.WKINDS:
        for c in (16, 48):
            for kind in P.kinds(dtype, c):
                _spdevoxelize(F, P.devox_case(wkind, c, kind, dtype), dt, dtype, '%s c=%d %s' % (wkind, c, kind), i64=(c == 48))
        _spdevoxelize(F, P.devox_case(wkind, 4, 'randn', dtype), dt, torch.float32, '%s c=4 stays fp32' % wkind)


@pytest.mark.parametrize('dt', DT)
def test_segment_map(F, hip, dt):
    """fusion._SegmentMap: the forward over one entry list, the gradient over its transpose; rows that arrive in bf16 / fp16 are
    moved in that type (``_moved16``), anything else as fp32, and the gradient has the source's type"""
    from u2mkd_amd import fusion
    dtype = P.DTYPES[dt]
    assert F._moved16(dtype) == (None if dt == 'f32' else dtype)
    for wkind in P.WKINDS:
        idx8, w8 = P.devox_layout(wkind)
        fwd = tuple(t.cuda() for t in P.devoxelize_fwd_plan(idx8, w8))
        bwd = _devox_plan_on_device(hip, idx8, w8, P.DEVOX_NV)
        for c in P.widths(dtype, vec4_only=True):
            for kind in P.kinds(dtype, c):
                case = P.devox_case(wkind, c, kind, dtype)
                src = case['f'].cuda().requires_grad_(True)
                out = fusion._SegmentMap.apply(src, fwd, bwd, P.DEVOX_N)
                assert out.dtype == dtype
                what = '%s c=%d %s' % (wkind, c, kind)
                _hold('_SegmentMap', dt, out.detach(), case['fwd'], case['fwd_b'], what)
                out.backward(case['g'].cuda())
                assert src.grad.dtype == dtype
                _hold('_SegmentMap backward', dt, src.grad, case['bwd'], case['bwd_b'], what)
    if dt == 'f32':     # a source that is neither: moved as fp32, the gradient returned in the source's type
        case = P.devox_case('tri', 4, 'randn', torch.float32)
        idx8, w8 = P.devox_layout('tri')
        src = case['f'].double().cuda().requires_grad_(True)
        out = fusion._SegmentMap.apply(src, tuple(t.cuda() for t in P.devoxelize_fwd_plan(idx8, w8)),
                                       _devox_plan_on_device(hip, idx8, w8, P.DEVOX_NV), P.DEVOX_N)
        assert out.dtype == torch.float32
        out.backward(case['g'].cuda())
        assert src.grad.dtype == torch.float64
        _hold('_SegmentMap backward', 'f32', src.grad.float(), case['bwd'], case['bwd_b'], 'float64 source')
