"""Camera BatchNorm2d on the device (csrc/bn2d.hip through the C ABI; camera.BatchNorm2d / SyncBatchNorm2d / bn_act over it)
against the float64 evaluation and the derived elementwise bound of tests/bn2d_f64_ref.py.

  1  the single-process passes: u2mkd_bn2d_train_forward / u2mkd_bn2d_backward(batch_stats=1) and u2mkd_bn2d_eval_forward /
     u2mkd_bn2d_backward(batch_stats=0) at every piece, chunk and form boundary: every element of every output inside the bound
     (an undecided element of the ReLU forms inside that of either branch), the step counter bumped once in training and not
     at all in eval, the elements behind every output and behind the workspace untouched;
  2  per case the largest error next to that of torch's own formulation (F.batch_norm in fp32, add, ReLU; torch's backward):
     printed, not asserted (NOTES N29.3);
  3  the SyncBatchNorm2d pieces over three emulated ranks in this process against the float64 evaluation of all images as one batch;
  4  the ReLU mask of the forward and of the backward pass, bit for bit, on residuals that put every pre-activation on the edge;
  5  the modules: the three modes, affine=False, track_running_stats=False, momentum=None, what the entries refuse, bf16 autocast;
  6  the same bits run after run and on a second stream."""
import math

import pytest
import torch

import bn2d_f64_ref as R2

pytestmark = pytest.mark.gpu

TF = torch.nn.functional
F32 = torch.float32
SENTINEL = 12288.0
GUARD = 64                                             # elements behind every output that have to stay untouched


class _Out:
    """an fp32 output of ``shape`` filled with SENTINEL, GUARD elements of SENTINEL behind it"""

    def __init__(self, shape, dtype=F32):
        self.n = math.prod(shape)
        self.buf = torch.full((self.n + GUARD,), SENTINEL, dtype=dtype, device='cuda')
        self.t = self.buf[:self.n].view(shape)

    def intact(self):
        return bool((self.buf[self.n:] == SENTINEL).all())


def _outs(spec):
    return {k: _Out(shape) for k, shape in spec.items()}


def _finish(outs, extra=None):
    torch.cuda.synchronize()
    broken = [k for k, o in outs.items() if not o.intact()]
    assert not broken, 'written behind the output: %s' % broken
    return dict({k: o.t for k, o in outs.items() if k != 'ws'}, **(extra or {}))


def _cuda(case):
    return {k: (v.cuda() if v is not None else None) for k, v in case.items()}


def _geometry(L, x):
    b, c = x.shape[:2]
    hw = x[0, 0].numel()
    nbytes = L.load().u2mkd_bn2d_workspace_bytes(b, c, hw)
    assert nbytes == R2.workspace_bytes(b, c, hw)
    return b, c, hw, (nbytes // 4,)                     # the workspace: exactly what the library asks for, guarded like an output


def _train_forward(L, case, mode, momentum=R2.MOMENTUM):
    x = case['x']
    b, c, hw, ws = _geometry(L, x)
    outs = _outs({'y': tuple(x.shape), 'mean': (c,), 'invstd': (c,), 'ws': ws})
    rm, rv = case['rm'].clone(), case['rv'].clone()
    counter = torch.full((1,), 41, dtype=torch.int64, device='cuda')
    res = case['res'] if mode == 'res' else None
    L.call('u2mkd_bn2d_train_forward', L.ptr(x), L.ptr(res), b, c, hw, L.ptr(case['gamma']), L.ptr(case['beta']), R2.EPS, momentum,
           int(mode != 'plain'), L.ptr(rm), L.ptr(rv), L.ptr(counter), L.ptr(outs['ws'].t), L.ptr(outs['mean'].t),
           L.ptr(outs['invstd'].t), L.ptr(outs['y'].t), L.stream())
    return _finish(outs, {'running_mean': rm, 'running_var': rv, 'counter': counter})


def _eval_invstd(rv):
    """what the caller of u2mkd_bn2d_backward(batch_stats=0) has to hand over: the expression of the eval forward, in fp32"""
    return 1.0 / torch.sqrt(rv + torch.tensor(R2.EPS, dtype=F32, device=rv.device))


def _eval_forward(L, case, mode):
    x = case['x']
    b, c, hw, _ = _geometry(L, x)
    outs = _outs({'y': tuple(x.shape)})
    rm, rv = case['rm'].clone(), case['rv'].clone()
    res = case['res'] if mode == 'res' else None
    L.call('u2mkd_bn2d_eval_forward', L.ptr(x), L.ptr(res), b, c, hw, L.ptr(case['gamma']), L.ptr(case['beta']), R2.EPS,
           int(mode != 'plain'), L.ptr(rm), L.ptr(rv), L.ptr(outs['y'].t), L.stream())
    got = _finish(outs, {'mean': case['rm'], 'invstd': _eval_invstd(case['rv'])})
    assert torch.equal(rm, case['rm']) and torch.equal(rv, case['rv'])              # the running statistics are read only
    return got


def _backward(L, case, mode, mean, invstd, batch_stats):
    x = case['x']
    b, c, hw, ws = _geometry(L, x)
    spec = {'dx': tuple(x.shape), 'dgamma': (c,), 'dbeta': (c,), 'ws': ws}
    if mode == 'res':
        spec['dres'] = tuple(x.shape)
    outs = _outs(spec)
    res = case['res'] if mode == 'res' else None
    L.call('u2mkd_bn2d_backward', L.ptr(case['dy']), L.ptr(x), L.ptr(res), b, c, hw, L.ptr(mean), L.ptr(invstd), L.ptr(case['gamma']),
           L.ptr(case['beta']), int(mode != 'plain'), int(batch_stats), L.ptr(outs['ws'].t), L.ptr(outs['dgamma'].t),
           L.ptr(outs['dbeta'].t), L.ptr(outs['dx'].t), L.ptr(outs['dres'].t if mode == 'res' else None), L.stream())
    return _finish(outs)


def _torch_formulation(case, mode, training):
    """torch's own: F.batch_norm in fp32, + residual, ReLU; torch's backward"""
    xt = case['x'].clone().requires_grad_(True)
    rt = case['res'].clone().requires_grad_(True)
    gm = case['gamma'].clone().requires_grad_(True) if case['gamma'] is not None else None
    bt = case['beta'].clone().requires_grad_(True) if case['beta'] is not None else None
    rm, rv = case['rm'].clone(), case['rv'].clone()
    y = TF.batch_norm(xt, rm, rv, gm, bt, training, R2.MOMENTUM, R2.EPS)
    if mode == 'res':
        y = y + rt
    if mode != 'plain':
        y = torch.relu(y)
    y.backward(case['dy'])
    out = {'y': y.detach(), 'dx': xt.grad, 'running_mean': rm, 'running_var': rv}
    if mode == 'res':
        out['dres'] = rt.grad
    if gm is not None:
        out['dgamma'], out['dbeta'] = gm.grad, bt.grad
    return out


def _error(got, ref, name, und):
    """the largest error of an output; an undecided element of dx / dres is measured against the nearer of its two branches"""
    err = (R2.rows(got).double() - ref[name]).abs()
    if name + '_alt' in ref:
        err = torch.where(und, torch.minimum(err, (R2.rows(got).double() - ref[name + '_alt']).abs()), err)
    return float(err.max()) if err.numel() else 0.0


# ------------------------------------------------------------------ 1, 2. the single-process passes against float64 and next to torch
_MEASURED = {}
SHAPE_IDS = ['x'.join(map(str, s)) for s in R2.SHAPES]


def _measure(L, shape):
    """every case of one shape, run ONCE for the two tests below: one record per (kind, mode, affine, form, output)"""
    if shape in _MEASURED:
        return _MEASURED[shape]
    records, se = [], {}
    for kind, mode, affine in R2.cases(shape):
        case = _cuda(R2.make_case(shape, kind, affine=affine))
        if kind not in se:
            se[kind] = R2.stat_errors(case['x'])
        for training in (True, False):
            if training:
                fw = _train_forward(L, case, mode)
                assert int(fw['counter']) == 42, (kind, mode)                 # bumped exactly once
                assert float(fw['invstd'].min()) > 0.0
            else:
                fw = _eval_forward(L, case, mode)
            got = dict(fw, **_backward(L, case, mode, fw['mean'], fw['invstd'], training))
            ref, bound, und, share = R2.evaluate64(case, mode, training=training, se=se[kind] if training else None)
            assert share <= R2.UNDECIDED_CAP, (kind, mode, affine, training, share)
            names = [k for k in R2.OUTPUTS if k in got and k in ref and (training or k not in ('mean', 'invstd'))]
            tch = _torch_formulation(case, mode, training)
            for name, (ok, over, _) in R2.check(got, ref, bound, und, names).items():
                rec = {'case': '%-8s %-5s %-6s %-5s %-12s' % (kind, mode, 'affine' if affine else 'plain', 'train' if training else 'eval', name),
                       'inside': ok, 'over': over, 'kernel': _error(got[name], ref, name, und), 'share': share}
                if name in tch:
                    rec.update(torch=_error(tch[name], ref, name, und), floor=R2.floor_ulp(ref[name], F32))
                records.append(rec)
    _MEASURED[shape] = records
    return records


@pytest.mark.parametrize('shape', R2.SHAPES, ids=SHAPE_IDS)
def test_single_process_passes_inside_the_float64_bound(hip, shape):
    """Every element of every output of every (kind, mode) and of both forms -- train: u2mkd_bn2d_train_forward,
    u2mkd_bn2d_backward(batch_stats=1); eval: u2mkd_bn2d_eval_forward on running statistics that are not 0 / 1,
    u2mkd_bn2d_backward(batch_stats=0) on the invstd of the same expression -- inside the derived bound, mean, invstd and both
    running statistics inside theirs, no element excluded (an undecided element of the ReLU forms inside the bound of either
    branch).  Figures on the MI355X: NOTES N29."""
    records = _measure(hip, shape)
    print('\n%s\n%s' % (shape, '\n'.join('BOUND %s %s err/bound %.4f  kernel %.3e  share %.5f' % (
        'x'.join(map(str, shape)), r['case'], r['over'], r['kernel'], r['share']) for r in records)))
    failed = [(r['case'], r['over']) for r in records if not r['inside']]
    assert not failed, failed


@pytest.mark.parametrize('shape', R2.SHAPES, ids=SHAPE_IDS)
def test_largest_error_next_to_that_of_torchs_formulation(hip, shape):
    """Recorded, not asserted: per case -- (kind, mode, form, output) -- the kernels' largest error, that of torch's own
    formulation on the same device tensors and their ratio (to the larger of torch's error and one floor, one unit in the last
    place at the case's largest reference magnitude).  The kernels are fp32 throughout; the largest ratio per output on the
    MI355X is in NOTES N29.3."""
    records = [r for r in _measure(hip, shape) if 'torch' in r]
    assert records and all(math.isfinite(r['kernel']) and math.isfinite(r['torch']) for r in records)
    print('\n%s\n%s' % (shape, '\n'.join('TORCH %s %s kernel %.3e  torch %.3e  floor %.3e  ratio %.2f' % (
        'x'.join(map(str, shape)), r['case'], r['kernel'], r['torch'], r['floor'], r['kernel'] / max(r['torch'], r['floor'], 1e-300))
        for r in records)))


# ------------------------------------------------------------------ 3. the SyncBatchNorm2d pieces
@pytest.mark.parametrize('images,h,w', [((3, 2, 1), 4, 2049), ((2, 1, 1), 7, 9)], ids=['3+2+1x8196', '2+1+1x63'])
def test_sync_batch_norm_2d_pieces_over_three_ranks(hip, images, h, w):
    """u2mkd_bn2d_local_stats | stacked [world, 2c+1] rows | u2mkd_bn_merge_stats | u2mkd_bn2d_apply, then
    u2mkd_bn2d_backward_local | the sums added in rank order | u2mkd_bn2d_backward_apply, against the float64 evaluation of all
    images as ONE batch; the ranks' means differ by 0.5 rank"""
    L, c, world, hw = hip, 8, len(images), h * w
    whole = R2.make_case((sum(images), c, h, w), 'randn', seed=5)
    for r, xr in enumerate(torch.split(whole['x'], list(images))):
        xr += 0.5 * r
    whole = _cuda(whole)
    gm, bt = whole['gamma'], whole['beta']
    ranks = [{k: v.contiguous() for k, v in zip(('x', 'dy', 'res'), t)}
             for t in zip(*(torch.split(whole[k], list(images)) for k in ('x', 'dy', 'res')))]
    failed, lines = [], []
    for mode in ('plain', 'res'):
        relu = int(mode != 'plain')
        gathered = _Out((world, 2 * c + 1))
        for r, cs in enumerate(ranks):
            ws = _Out(_geometry(L, cs['x'])[3])
            L.call('u2mkd_bn2d_local_stats', L.ptr(cs['x']), images[r], c, hw, L.ptr(ws.t), L.ptr(gathered.t[r]), L.stream())
            torch.cuda.synchronize()
            assert ws.intact()
        st = _outs({'mean': (c,), 'invstd': (c,), 'total': (1,)})
        rm, rv = whole['rm'].clone(), whole['rv'].clone()
        counter = torch.full((1,), 7, dtype=torch.int64, device='cuda')
        L.call('u2mkd_bn_merge_stats', L.ptr(gathered.t), world, c, R2.EPS, R2.MOMENTUM, L.ptr(rm), L.ptr(rv), L.ptr(st['mean'].t),
               L.ptr(st['invstd'].t), L.ptr(st['total'].t), L.ptr(counter), L.stream())
        stats = _finish(dict(st, gathered=gathered))
        assert [float(stats['gathered'][r, 2 * c]) for r in range(world)] == [float(b * hw) for b in images]   # each row's count
        assert float(stats['total']) == float(sum(images) * hw) and int(counter) == 8
        ys, sums = [], []
        for r, cs in enumerate(ranks):
            o = _outs({'y': tuple(cs['x'].shape), 'sums': (2 * c,), 'keep': (2 * c,), 'ws': _geometry(L, cs['x'])[3]})
            res = cs['res'] if mode == 'res' else None
            L.call('u2mkd_bn2d_apply', L.ptr(cs['x']), L.ptr(res), images[r], c, hw, L.ptr(stats['mean']), L.ptr(stats['invstd']),
                   L.ptr(gm), L.ptr(bt), relu, L.ptr(o['y'].t), L.stream())
            L.call('u2mkd_bn2d_backward_local', L.ptr(cs['dy']), L.ptr(cs['x']), L.ptr(res), images[r], c, hw, L.ptr(stats['mean']),
                   L.ptr(stats['invstd']), L.ptr(gm), L.ptr(bt), relu, L.ptr(o['ws'].t), L.ptr(o['sums'].t), L.ptr(o['keep'].t),
                   L.stream())
            got_r = _finish(o)
            assert torch.equal(got_r['keep'], got_r['sums']), r                 # keep: the rank's own sums, bit for bit
            ys.append(got_r['y']), sums.append(got_r['sums'])
        total_sums = sums[0].clone()
        for s in sums[1:]:
            total_sums = total_sums + s                                          # (the all_reduce, in rank order)
        dxs, dress = [], []
        for r, cs in enumerate(ranks):
            o = _outs(dict({'dx': tuple(cs['x'].shape)}, **({'dres': tuple(cs['x'].shape)} if mode == 'res' else {})))
            res = cs['res'] if mode == 'res' else None
            L.call('u2mkd_bn2d_backward_apply', L.ptr(cs['dy']), L.ptr(cs['x']), L.ptr(res), images[r], c, hw, L.ptr(stats['total']),
                   L.ptr(stats['mean']), L.ptr(stats['invstd']), L.ptr(gm), L.ptr(bt), relu, L.ptr(total_sums), L.ptr(o['dx'].t),
                   L.ptr(o['dres'].t if mode == 'res' else None), L.stream())
            got_r = _finish(o)
            dxs.append(got_r['dx'])
            if mode == 'res':
                dress.append(got_r['dres'])
        got = {'y': torch.cat(ys), 'mean': stats['mean'], 'invstd': stats['invstd'], 'running_mean': rm, 'running_var': rv,
               'dx': torch.cat(dxs), 'dbeta': total_sums[:c], 'dgamma': total_sums[c:]}
        if mode == 'res':
            got['dres'] = torch.cat(dress)
        ref, bound, und, share = R2.evaluate64(whole, mode, ranks=images)
        assert share <= R2.UNDECIDED_CAP
        for name, (ok, over, e_k) in R2.check(got, ref, bound, und).items():
            lines.append('SYNC %s hw=%d %-5s %-12s err/bound %.4f  kernel %.3e' % (images, hw, mode, name, over, e_k))
            if not ok:
                failed.append(lines[-1])
    print('\n' + '\n'.join(lines))
    assert not failed, failed


# ------------------------------------------------------------------ 4. one ReLU mask in both passes
def _module(cls, case, **kw):
    bn = cls(case['x'].shape[1], **kw).cuda()
    with torch.no_grad():
        if bn.weight is not None:
            bn.weight.copy_(case['gamma'])
            bn.bias.copy_(case['beta'])
        if bn.running_mean is not None:
            bn.running_mean.copy_(case['rm'])
            bn.running_var.copy_(case['rv'])
    return bn


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('shape', [(2, 4, 17, 241), (6, 64, 45, 80)], ids=['2x4x17x241', '6x64x45x80'])
def test_forward_and_backward_take_the_same_relu_mask_bit_for_bit(hip, shape, training):
    """camera.BatchNorm2d with a residual that is the NEGATED output of the plain form, a third of it one fp32 step above and a
    third one below: every pre-activation of the fused form is 0 or one rounding off it, where the two passes agree only if
    they evaluate one expression on one (mean, invstd).  At every element with dy != 0: y > 0 exactly when dres == dy, and
    y == 0 exactly when dres == 0."""
    from u2mkd_amd import camera
    case = _cuda(R2.make_case(shape, 'scales', seed=3))
    bn = _module(camera.BatchNorm2d, case).train(training)
    x = case['x']
    with torch.no_grad():
        y0 = bn(x, False, None)
        bn.running_mean.copy_(case['rm'])
        bn.running_var.copy_(case['rv'])
    which = torch.arange(y0.numel(), device='cuda').view_as(y0) % 3
    res = torch.where(which == 0, -y0, torch.nextafter(-y0, torch.where(which == 1, 1.0, -1.0) * torch.full_like(y0, float('inf'))))
    res.requires_grad_(True)
    dy = torch.where(case['dy'] == 0, torch.ones_like(case['dy']), case['dy'])
    y = bn(x.clone().requires_grad_(True), True, res)
    y.backward(dy)
    torch.cuda.synchronize()
    dres, y = res.grad, y.detach()
    live, dead = y > 0, y == 0
    assert bool((live | dead).all()) and bool(((dres == dy) | (dres == 0)).all())
    share = float(live.double().mean())
    print('\nMASK %s %s: y > 0 at %.4f of the elements; y > 0 with dres == 0 at %d, y == 0 with dres == dy at %d' % (
        shape, 'train' if training else 'eval', share, int((live & (dres == 0)).sum()), int((dead & (dres == dy)).sum())))
    assert 0.2 < share < 0.5                            # the third that is one step above, and nothing else
    assert torch.equal(live, dres == dy) and torch.equal(dead, dres == 0)


# ------------------------------------------------------------------ 5. the module level
MODULE_SHAPE = R2.AFFINE_FALSE_SHAPE


def _module_pass(bn, case, mode, through):
    x = case['x'].clone().requires_grad_(True)
    res = case['res'].clone().requires_grad_(True) if mode == 'res' else None
    y = through(bn, x, mode != 'plain', res)
    y.backward(case['dy'])
    torch.cuda.synchronize()
    got = {'y': y.detach(), 'dx': x.grad}
    if res is not None:
        got['dres'] = res.grad
    if bn.weight is not None:
        got['dgamma'], got['dbeta'] = bn.weight.grad, bn.bias.grad
    if bn.running_mean is not None and bn.training:
        got['running_mean'], got['running_var'] = bn.running_mean, bn.running_var
    return got


@pytest.mark.parametrize('kw', [{}, {'affine': False}, {'track_running_stats': False}, {'affine': False, 'track_running_stats': False}],
                         ids=['default', 'no_affine', 'no_running', 'neither'])
@pytest.mark.parametrize('flavour', ['BatchNorm2d', 'SyncBatchNorm2d', 'bn_act'])
def test_modules_inside_the_bound(hip, monkeypatch, flavour, kw):
    """camera.BatchNorm2d, SyncBatchNorm2d without a process group (its one-rank route) and bn_act, the three modes, in training
    and in eval mode (batch statistics there too without running statistics): outputs and buffers inside the bound, on the
    kernels of csrc/bn2d.hip.  The eval form's invstd is torch.rsqrt(running_var + eps) for both passes: one rounding of the
    sum and a reciprocal square root good to one unit in the last place, inside the 3 u of the bound's dr."""
    from u2mkd_amd import camera
    cls = camera.SyncBatchNorm2d if flavour == 'SyncBatchNorm2d' else camera.BatchNorm2d
    through = (lambda bn, x, relu, res: camera.bn_act(bn, x, relu=relu, residual=res)) if flavour == 'bn_act' else \
        (lambda bn, x, relu, res: bn(x, relu, res))
    calls, real = [], hip.call
    monkeypatch.setattr(hip, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    for mode in R2.MODES:
        case = _cuda(R2.make_case(MODULE_SHAPE, 'randn', affine=kw.get('affine', True)))
        for training in (True, False):
            bn = _module(cls, case, **kw).train(training)
            del calls[:]
            got = _module_pass(bn, case, mode, through)
            batch_stats = training or bn.running_mean is None
            # (the eval forward applies the invstd tensor that is saved for the backward: test 4)
            assert calls == ['u2mkd_bn2d_train_forward' if batch_stats else 'u2mkd_bn2d_apply', 'u2mkd_bn2d_backward'], calls
            if bn.running_mean is not None:
                assert int(bn.num_batches_tracked) == (1 if training else 0)
                if not training:
                    assert torch.equal(bn.running_mean, case['rm']) and torch.equal(bn.running_var, case['rv'])
            ref, bound, und, _ = R2.evaluate64(case, mode, training=batch_stats)
            out = R2.check(got, ref, bound, und)
            assert sorted(out) == sorted(got) and all(v[0] for v in out.values()), (mode, training, out)


def test_momentum_none_takes_torchs_path(hip, monkeypatch):
    from u2mkd_amd import camera
    case = _cuda(R2.make_case(MODULE_SHAPE, 'randn'))
    calls, real = [], hip.call
    monkeypatch.setattr(hip, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    bn = _module(camera.BatchNorm2d, case, momentum=None).train()
    theirs = _module(torch.nn.BatchNorm2d, case, momentum=None).train()
    y = bn(case['x'], True, case['res'])
    assert not calls, calls
    want = torch.relu(theirs(case['x']) + case['res'])
    # torch's path IS torch.nn.BatchNorm2d on the same state: the same bits in the output and in the buffers
    assert torch.equal(y, want) and int(bn.num_batches_tracked) == int(theirs.num_batches_tracked) == 1
    assert torch.equal(bn.running_mean, theirs.running_mean) and torch.equal(bn.running_var, theirs.running_var)
    assert not torch.equal(bn.running_mean, case['rm'])


def test_the_entries_refuse_what_they_cannot_compute_and_the_modules_never_pass_it_down(hip, monkeypatch):
    """one value per channel in training, and b = 0: an error code from the entry, nothing launched, nothing written"""
    from u2mkd_amd import camera
    L = hip
    case = _cuda(R2.make_case((1, 4, 1, 2), 'randn'))
    one = {k: (v[:, :, :, :1].contiguous() if v is not None and v.dim() == 4 else v) for k, v in case.items()}
    for x, b, match in ((one['x'], 1, 'more than one value per channel'), (case['x'], 0, 'out of range')):
        c = x.shape[1]
        outs = _outs({'y': tuple(x.shape), 'mean': (c,), 'invstd': (c,), 'ws': (16,)})
        rm, rv = case['rm'].clone(), case['rv'].clone()
        counter = torch.full((1,), 41, dtype=torch.int64, device='cuda')
        with pytest.raises(RuntimeError, match=match):
            L.call('u2mkd_bn2d_train_forward', L.ptr(x), None, b, c, x[0, 0].numel(), L.ptr(case['gamma']), L.ptr(case['beta']), R2.EPS,
                   R2.MOMENTUM, 0, L.ptr(rm), L.ptr(rv), L.ptr(counter), L.ptr(outs['ws'].t), L.ptr(outs['mean'].t),
                   L.ptr(outs['invstd'].t), L.ptr(outs['y'].t), L.stream())
        torch.cuda.synchronize()
        assert all(bool((o.buf == SENTINEL).all()) for o in outs.values()) and int(counter) == 41
        assert torch.equal(rm, case['rm']) and torch.equal(rv, case['rv'])
    assert L.load().u2mkd_bn2d_workspace_bytes(0, 4, 2) == 0
    # eval mode takes one value per channel; an empty batch goes to torch
    bn = _module(camera.BatchNorm2d, case).eval()
    ref, bound, und, _ = R2.evaluate64(one, 'plain', training=False)
    assert R2.check({'y': bn(one['x']).detach()}, ref, bound, und, ['y'])['y'][0]
    calls, real = [], hip.call
    monkeypatch.setattr(hip, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    y = bn(case['x'][:0])
    assert y.shape == (0, 4, 1, 2) and not calls, calls


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
def test_bf16_autocast_fallback_is_within_one_bf16_ulp_of_float64(hip, monkeypatch, training):
    """under autocast the module takes torch's path on the bf16 map: y within one bf16 unit in the last place at the largest
    reference magnitude, plus the fp32 bound, of the float64 evaluation of the bf16 values"""
    from u2mkd_amd import camera
    case = _cuda(R2.make_case((3, 8, 32, 32), 'randn'))
    case['x'] = case['x'].bfloat16()
    calls, real = [], hip.call
    monkeypatch.setattr(hip, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    bn = _module(camera.BatchNorm2d, case).train(training)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        y = bn(case['x'], True)
    assert not [n for n in calls if 'bn2d' in n], calls
    assert y.shape == case['x'].shape and y.dtype == torch.bfloat16
    as_f32 = dict(case, x=case['x'].float())
    ref, bound, _, _ = R2.evaluate64(as_f32, 'relu', training=training)
    ok, over, err = R2.worst(R2.rows(y.detach()), ref['y'], bound['y'] + R2.floor_ulp(ref['y'], torch.bfloat16))
    print('\nBF16 %s: largest error %.3e, error / allowance %.3f' % ('train' if training else 'eval', err, over))
    assert ok, (over, err)


# ------------------------------------------------------------------ 6. the same bits every time
def test_the_same_bits_run_after_run_and_on_a_second_stream(hip):
    L = hip
    case = _cuda(R2.make_case((5, 4, 282, 378), 'randn', seed=9))

    def run(copy=False):
        cs = {k: (v.clone() if copy and v is not None else v) for k, v in case.items()}
        fw = _train_forward(L, cs, 'res')
        return dict(fw, **_backward(L, cs, 'res', fw['mean'], fw['invstd'], True))

    first = run()
    for _ in range(2):
        again = run()
        assert all(torch.equal(first[k], again[k]) for k in first)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = run(copy=True)
    side.synchronize()
    assert all(torch.equal(first[k], other[k]) for k in first)
