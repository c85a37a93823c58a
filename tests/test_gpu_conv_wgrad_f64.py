"""Every form of the pair-list weight gradient (u2mkd_conv_wgrad_pairs, _bf16, _f16: csrc/conv.hip wgrad_pairs_impl) against
float64, elementwise, under the bound of tests/wgrad_f64_ref.py -- mag * (T + 4 max(r, 2^-24)), r measured per case and offset
on an honest fp32 evaluation of the same inputs, T = 0 or the bf16x3 split's dropped products.

The inputs are SYNTHETIC pair lists through the C ABI, so that the plan reaches what real scenes do not: offsets of no pairs
and of one pair, chunk tails that are no multiple of the step, merged runs that start off a multiple of ``merge`` and cross an
offset boundary, offsets of more than 64 live slabs (the reduce's trip length).  Each case asserts FROM THE PLAN it read back
and from the dispatch rule (wgrad_f64_ref.family) that it reached the form it is there for.  tests/test_host_wgrad_bound.py
shows on the same inputs that the bound rejects a lost partial product, a rounded operand, a skipped pair and unswapped
columns."""
import math
import os
import subprocess
import sys

import pytest
import torch

import wgrad_f64_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
ENTRY = {F32: 'u2mkd_conv_wgrad_pairs', BF16: 'u2mkd_conv_wgrad_pairs_bf16', F16: 'u2mkd_conv_wgrad_pairs_f16'}

# fp32 rows on the f32-MFMA kernel (a channel count that is no multiple of 64): every tile class (<= 32, <= 64, <= 96, > 96) once
# per operand, with and without a channel tail, both step sizes
MFMA_SHAPES = [(4, 32), (32, 64), (48, 16), (64, 96), (96, 96), (96, 128), (128, 96), (192, 32), (160, 64), (20, 12), (8, 20)]
X3_SHAPES = [(64, 64), (64, 128), (128, 128), (192, 192)]                   # merge 1, 2, 4, 6
ROWS16_SHAPES = [(64, 64), (128, 128), (192, 192), (32, 64), (96, 96), (20, 12)]


def _cases():
    out = []
    add = lambda dt, shapes, pattern, spreads: out.extend((dt, ca, cb, pattern, s) for ca, cb in shapes for s in spreads)
    add(F32, MFMA_SHAPES, 'ragged', ('unit', 'rows'))
    add(F32, [(32, 64), (160, 64)], 'ragged', ('tiny',))
    add(F32, [(32, 64), (96, 96), (20, 12)], 'heavy', ('rows',))            # 32 and 16 pairs per step, a channel tail
    add(F32, [(64, 96), (20, 12), (192, 32)], 'ragged8', ('rows',))
    add(F32, [(64, 96), (20, 12), (192, 32)], 'ragged8-swap', ('rows',))
    add(F32, [(32, 64), (128, 96)], 'dense1', ('unit',))
    add(F32, [(20, 12), (96, 128)], 'empty', ('unit',))
    add(F32, X3_SHAPES, 'ragged', ('unit', 'rows', 'tiny'))
    add(F32, [(64, 128), (128, 128)], 'ragged8', ('rows',))
    add(F32, [(64, 128), (128, 128)], 'ragged8-swap', ('rows',))
    add(F32, [(64, 64)], 'heavy', ('unit', 'rows'))
    add(F32, [(64, 128)], 'heavy-merged', ('rows',))
    add(F32, [(64, 64), (192, 192)], 'dense1', ('unit', 'rows'))
    add(F32, [(64, 64), (128, 128)], 'empty', ('unit',))
    for dt in (BF16, F16):
        add(dt, ROWS16_SHAPES, 'ragged', ('unit', 'rows'))
        add(dt, [(64, 64), (96, 96)], 'heavy', ('rows',))
        add(dt, [(32, 64), (192, 192)], 'ragged8-swap', ('rows',))
        add(dt, [(64, 64), (32, 64)], 'dense1', ('unit',))
        add(dt, [(128, 128)], 'empty', ('unit',))
    add(BF16, [(64, 64), (20, 12)], 'ragged', ('tiny',))                     # (1e-20 is below fp16's range)
    return out


def _lg(v):
    return math.log2(v) if v > 0 else float('-inf')


def _id(c):
    return '%s-%dx%d-%s-%s' % (str(c[0]).split('.')[-1], c[1], c[2], c[3], c[4])


@pytest.fixture(scope='module')
def L(hip):
    if os.environ.get('U2MKD_CONV_ARITH'):
        pytest.skip('U2MKD_CONV_ARITH overrides the default')
    return hip


def _launch(L, a, b, pairs, counts, n_rows, swap):
    """One call of the entry of a's dtype: plan, NaN-filled workspace and dw.  Returns (dw, plan as a list)."""
    lib = L.load()
    k, ca, cb = len(counts), a.shape[1], b.shape[1]
    st = L.stream()
    nbsizes = torch.tensor(counts, dtype=torch.int32, device='cuda')
    plan = torch.full((lib.u2mkd_wgrad_plan_ints(k),), -1, dtype=torch.int32, device='cuda')
    L.call('u2mkd_wgrad_plan', L.ptr(nbsizes), k, n_rows, L.ptr(plan), st)
    nbytes = lib.u2mkd_conv_wgrad_pairs_workspace_bytes(n_rows, ca, cb, k)
    ws = torch.full((nbytes // 4,), float('nan'), device='cuda')
    dw = torch.full((k, ca, cb), float('nan'), device='cuda')
    L.call(ENTRY[a.dtype], L.ptr(a), ca, L.ptr(b), cb, L.ptr(pairs), L.ptr(plan), n_rows, k, swap, L.ptr(ws), nbytes, L.ptr(dw), st)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a device fault: nothing else of this session may use the GPU
        pytest.exit('GPU fault in %s [%d, %d, %d]: %s' % (ENTRY[a.dtype], k, ca, cb, e), returncode=3)
    return dw, plan.tolist()


def _check_plan(plan, counts, n_rows, pattern, fam, dtype):
    """The plan is the one the counts ask for, every slab lies inside the workspace, and the pattern reached its edge."""
    k, (kind, form) = len(counts), fam
    ch, kofs, wg = plan[1], plan[2:3 + k], plan[3 + k:4 + 2 * k]
    assert plan[0] == sum(counts) and kofs == [sum(counts[:i]) for i in range(k + 1)]
    assert wg == [sum(-(-c // ch) for c in counts[:i]) for i in range(k + 1)]
    g = min(max((n_rows * min(k, 8) * 2 + 511) // 512, 32), 1024)            # wgrad_g_target
    assert wg[k] <= g + k                                                      # the workspace holds g + k slabs
    merge = form if kind == 'x3' else 1
    step = 32 if kind == 'x3' else form[2]
    live = R.live_slabs(plan, k, merge)
    if pattern.startswith('ragged'):
        assert ch == 128
        assert 0 in counts and 1 in counts                                     # an offset without pairs, one of a single pair
        assert any(c % ch % step for c in counts)                              # a chunk tail that is no multiple of the step
        assert any(c > ch for c in counts)                                     # more than one slab
        if merge > 1:
            # a segment that starts off a multiple of merge (its slab is the `w0` of the reduce) ...
            assert any(wg[i] % merge and wg[i + 1] > wg[i] for i in range(k))
            # ... and a workgroup's run of `merge` slots with an offset boundary inside it
            assert any(wg[i] % merge and 0 < wg[i] < wg[k] and wg[i] > wg[i - 1] for i in range(1, k))
    if pattern in ('heavy', 'heavy-merged'):
        assert ch == 128 and max(len(s) for s in live) > 64, (ch, max(len(s) for s in live))      # a second trip of the reduce
        if pattern == 'heavy-merged':
            assert merge == 2
    if pattern == 'dense1':
        assert k == 1 and wg[1] > 1
    if pattern == 'empty':
        assert wg[k] == 0


def _expect_family(ca, cb, dtype):
    fam = R.family(ca, cb, dtype)
    if dtype == F32 and (ca, cb) in MFMA_SHAPES:
        pick = lambda c: 1 if c <= 32 else 2 if c <= 64 else 3 if c <= 96 else 4
        assert fam == ('mfma', (pick(ca), pick(cb), 16 if max(ca, cb) > 64 else 32))
    if (ca, cb) in X3_SHAPES:
        assert fam == ('x3', {(64, 64): 1, (64, 128): 2, (128, 128): 4, (192, 192): 6}[(ca, cb)])
    elif dtype != F32:
        assert fam[0] == 'mfma'
    return fam


def _run_case(L, dtype, ca, cb, pattern, spread, f32_arith=False):
    c = R.make_case(pattern, ca, cb, spread, dtype)
    a, b, pairs = c['a'].cuda(), c['b'].cuda(), c['pairs'].cuda()
    counts, n_rows, swap = c['counts'], c['n_rows'], c['swap']
    fam = R.family(ca, cb, dtype, f32_arith) if f32_arith else _expect_family(ca, cb, dtype)
    T = R.T_X3 if (fam[0] == 'x3' and dtype == F32) else R.T_EXACT
    got, plan = _launch(L, a, b, pairs, counts, n_rows, swap)
    _check_plan(plan, counts, n_rows, pattern, fam, dtype)
    # the reference: float64 of the rows as the kernel sees them (16-bit rows: of the rounded rows)
    dw, mag = R.wgrad_f64(a, b, pairs, counts, swap)
    r = R.rel_err(R.honest_fp32(a, b, pairs, counts, swap), dw, mag)
    if dtype == F16 and fam[0] == 'x3':      # the fp16 matrix instruction aligns to NOMINAL exponents: subnormals count as 2^-14
        mag = R.wgrad_f64(R.nominal_fp16(a), R.nominal_fp16(b), pairs, counts, swap)[1]
    ok, over, rel = R.check(got, dw, mag, T, r)
    print('\n[wgrad-f64] %s %s merge/tile %s %dx%d %s %s: r 2^%.1f  err/mag 2^%.1f  err/bound %.3f'
          % (str(dtype).split('.')[-1], fam[0], fam[1], ca, cb, pattern, spread, _lg(float(r.max())), _lg(rel), over))
    assert bool(torch.isfinite(got).all())
    assert ok, 'largest err / bound %.3f (err / mag 2^%.1f, r 2^%.1f)' % (over, _lg(rel), _lg(float(r.max())))
    if pattern == 'empty':
        assert int(torch.count_nonzero(got)) == 0
    again, _ = _launch(L, a, b, pairs, counts, n_rows, swap)
    assert torch.equal(got, again)
    # a 16-bit form against the fp32 entry on the widened rows, where both run the same arithmetic: the f32-MFMA kernel (rows
    # widened in registers), and bf16 rows on the bf16x3 kernel (a widened bf16 has m = l = 0: five products of zeros and h * h).
    # (fp16 rows on that kernel multiply in fp16; the fp32 entry splits a widened fp16 into h and m: not the same sums.)
    if dtype != F32 and (fam[0] == 'mfma' or dtype == BF16):
        wide, _ = _launch(L, a.float(), b.float(), pairs, counts, n_rows, swap)
        assert torch.equal(got, wide)
    return over


@pytest.mark.parametrize('case', _cases(), ids=_id)
def test_wgrad_pairs_within_the_float64_bound(L, case):
    _run_case(L, *case)


@pytest.mark.parametrize('kind,cin,cout', [('subm', 64, 64), ('down', 32, 64), ('up', 32, 64)])
def test_convolution_function_weight_gradient_within_the_float64_bound(L, kind, cin, cout):
    """The same bound through ConvolutionFunction.backward on a 3000-voxel scene; float64 from km.nbr (the neighbour table), not
    from the compacted pair list, so u2mkd_kmap_compact and the plan of KernelMap.pairs_plan are under test too."""
    from u2mkd_amd.synth import synth_batch
    from u2mkd_amd.torchsparse.nn import functional as F
    coords = torch.from_numpy(synth_batch(3000, 1, seed=7)['coords']).cuda()
    ks, st_ = (3, 1) if kind == 'subm' else (2, 2)
    km = F.build_kmap(coords, (1,) * 3, (ks,) * 3, (st_,) * 3)
    transposed = kind == 'up'
    n_x, n_g = (km.n_out, km.n_in) if transposed else (km.n_in, km.n_out)
    gen = torch.Generator().manual_seed(31)
    scale = lambda n: torch.pow(10.0, torch.randint(-10, 11, (n, 1), generator=gen).float())
    x = (torch.randn(n_x, cin, generator=gen) * scale(n_x)).cuda().requires_grad_(True)
    g = (torch.randn(n_g, cout, generator=gen) * scale(n_g)).cuda()
    w = (torch.randn(ks ** 3, cin, cout, generator=gen) / (ks ** 3 * cin) ** 0.5).cuda().requires_grad_(True)
    F.ConvolutionFunction.apply(x, w, km, transposed).backward(g)
    torch.cuda.synchronize()
    # pairs (input row, output row) of every offset from the table: nbr[k][j] = the input row of output j, or -1
    nbr = km.nbr.long()
    pairs, counts = [], []
    for kk in range(nbr.shape[0]):
        j = torch.nonzero(nbr[kk] >= 0)[:, 0]
        pairs.append(torch.stack([nbr[kk][j], j], dim=1))
        counts.append(len(j))
    pairs = torch.cat(pairs).int()
    assert sum(counts) > 0
    swap = 1 if transposed else 0        # transposed: x lives on the OUTPUT rows of the map
    xd = x.detach()
    dw, mag = R.wgrad_f64(xd, g, pairs, counts, swap)
    r = R.rel_err(R.honest_fp32(xd, g, pairs, counts, swap), dw, mag)
    fam = R.family(cin, cout, F32)
    assert fam[0] == ('x3' if kind == 'subm' else 'mfma')
    ok, over, rel = R.check(w.grad, dw, mag, R.T_X3 if fam[0] == 'x3' else R.T_EXACT, r)
    print('\n[wgrad-f64] ConvolutionFunction %s %dx%d: r 2^%.1f  err/mag 2^%.1f  err/bound %.3f'
          % (kind, cin, cout, _lg(float(r.max())), _lg(rel), over))
    assert bool(torch.isfinite(w.grad).all())
    assert ok, 'largest err / bound %.3f' % over


def _f32_switch_child():
    """(runs in the child process of the test below: U2MKD_CONV_ARITH=f32 is read once per process)"""
    from u2mkd_amd import _lib
    assert _lib.load().u2mkd_conv_tiles_arith(64, 64, 27) == 1          # the library read the switch
    for ca, cb in ((64, 64), (128, 128)):
        fam = R.family(ca, cb, F32, f32_arith=True)
        assert fam == ('mfma', (2, 2, 32) if ca == 64 else (4, 4, 16))
        for pattern, spread in (('ragged', 'unit'), ('ragged', 'rows'), ('heavy', 'rows'), ('ragged8-swap', 'rows')):
            _run_case(_lib, F32, ca, cb, pattern, spread, f32_arith=True)
    print('ok')


def test_f32_switch_runs_the_64_and_128_wide_instantiations_of_the_f32_mfma_kernel(L):
    """conv_wgrad_pairs_kernel<2, 2, 32> and <4, 4, 16> take fp32 rows only under U2MKD_CONV_ARITH=f32 (every other 64-multiple
    shape goes to the bf16x3 kernel): (64, 64) and (128, 128) with T = 0, in a fresh process."""
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n'
            'import test_gpu_conv_wgrad_f64 as T\n'
            'T._f32_switch_child()\n') % (ROOT, os.path.join(ROOT, 'tests'))
    env = dict(os.environ, U2MKD_CONV_ARITH='f32')
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
