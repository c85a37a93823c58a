"""float64 reference of the camera BatchNorm2d kernels (csrc/bn2d.hip: u2mkd_bn2d_train_forward, u2mkd_bn2d_eval_forward,
u2mkd_bn2d_backward and the SyncBatchNorm2d pieces), and the elementwise bound the kernels are held to (test helper; plain
torch, CPU or GPU tensors).

WHAT IS COMPUTED is what tests/row_bn_f64_ref.py writes down, with n = B hw, on the NCHW map seen as [B hw, C] rows (``rows``),
in fp32 only; ``forward64``, ``backward64``, ``running64``, ``forward_bound``, ``backward_bound`` and ``worst`` are that file's.
Steps 4-6 and 8 of its bound, the undecided elements of the fused ReLU, U1 / U2 and ``UNDECIDED_CAP`` hold as they stand there:
csrc/bn2d.hip evaluates the same expressions in fp32, operation for operation (xhat = fl(fl(x - m) r), pre = xhat gamma + beta
[+ res], dx = fl(gamma r) fl(fl(dy' - fl(db i)) - fl(xhat fl(dg i))), eval form fl(fl(gamma r) dy')).  What depends on the
kernels' shape is restated here.  u = 2^-24, g(k) = k u / (1 - k u).  Every term is u times a magnitude THAT IS ACTUALLY SUMMED;
no constant is fitted to a measured error.

 The kernels' shape (``float4_form``, ``splits``, ``piece_counts``, ``piece_depth``, ``bwd_piece_depth``, ``merge_depth``,
 ``sum_depth``).  256 threads.  The statistics and the gradient sums cut every plane (b, c) into pieces of 8192 elements,
 ordered (b, split), the last one of hw - 8192 (splits - 1) elements; the elementwise kernels into chunks of 4096.  hw % 4 == 0:
 the float4 form, thread t takes the float4 at 4 t + 1024 k; the statistics kernel combines its four values as (d0 + d1) +
 (d2 + d3) before they reach the thread's accumulator (2 additions on a value's path), the gradient kernel adds them one after
 the other.  Otherwise the scalar form, thread t takes element t + 256 k.  The threads' sums pass a 6-level shuffle tree per
 wave, the 4 waves are added in order.  An addition to the initial zero, or of a dead lane's zero, is exact:
     Dp = [2] + trips - 1 + ceil(log2(min(64, live))) + ceil(live / 64) - 1      (``piece_depth``; live threads, trips of thread 0)
 = 18 for a full float4 piece, 40 for a full scalar one and for both forms of the gradient kernel, 0 for a piece of one element.

 1  a piece's mean from SHIFTED sums, shift = the piece's first element: d = fl(x - shift), s1 = sum d, mean_b = fl(shift +
    fl(s1 / n_b)).  With A1 = sum |x - shift|, S1 = sum (x - shift) = n_b (m_b - shift):
        e1 = g(Dp + 1) A1                                        (the error of s1: one rounding per d, Dp in the sum)
        e_b = e1 / n_b + u (|m_b - shift| + e1 / n_b) + u (|m_b| + 2 e1 / n_b)
 2  M2_b = max(fl(s2 - fl(fl(s1 s1) / n_b)), 0), s2 = sum fl(d d).  The sum that is carried is NOT M2_b but
        S2 = sum (x - shift)^2 = M2_b + n_b (m_b - shift)^2,
    and the term that is subtracted is S1^2 / n_b = n_b (m_b - shift)^2: both carry their roundings at THAT size, so the error of
    M2_b has a term in u n_b (m_b - shift)^2 that is not small against M2_b when the first element is not a typical one
    (input kind ``first8``: the first element of every piece 8 spreads off; n_b (m_b - shift)^2 = 64 M2_b):
        e2 = g(Dp + 3)(M2_b + n_b (m_b - shift)^2)                                   (d twice, the square, Dp in the sum)
        ec = (2 |S1| e1 + e1^2) / n_b + g(2)(|S1| + e1)^2 / n_b                    (the square and the quotient round)
        q_b = e2 + ec + u (M2_b + e2 + ec)                                          (the difference rounds; max(., 0) only helps)
 3  Chan's update over the np = B splits pieces in the order of bn2d_stats_finalize_kernel: lane l of 64 takes pieces l, l + 64,
    ... one after the other, the 64 lanes are merged by a 6-level tree (``merge_depth``: Dm = min(np - 1, ceil(np / 64) + 5)
    updates on any path).  The update is the row file's (difference, quotient, product, sum; the cross term of M2 with 6
    roundings), the piece counts are min(8192, hw - 8192 s) with s = i % splits, and so is the algebra (row file, step 3):
        E = max_b e_b + Dm u (A + 3 S)        dM2 = Q + g(2 Dm + 6)(M2 + Q),   Q = sum_b q_b + 4 E sqrt(7 n B) + 28 n E^2
    SyncBatchNorm2d: u2mkd_bn_merge_stats over the ranks' (mean, M2, count) rows in rank order, world - 1 updates, W <= n, the
    ranks' own E and dM2 in the place of e_b and q_b (``stat_errors`` takes a list of ranks' maps).
 4-6  as in the row file (var, invstd with 3 u, the running statistics, xhat, pre, y).  Eval form: the mean is an input and
    invstd is fl(1 / fl(sqrt(fl(var + eps)))) of an input, dr = 3 u r -- u2mkd_bn2d_eval_forward evaluates that expression in
    the kernel, and the invstd handed to u2mkd_bn2d_backward(batch_stats = 0) has to be that expression as well.
 7  a channel's gradient sums pass the ``bwd_piece_depth`` additions of its largest piece, then ceil(np / 64) - 1 in one of 64
    lanes and 6 tree levels of bn2d_bwd_finalize_kernel [, world - 1 across the ranks]: Dn = ``sum_depth``; bound(dbeta) and
    bound(dgamma) are the row file's with this Dn, U1 and U2 included.
 8  as in the row file; i = fl(1 / (B hw)) (on the host), or fl(1 / total) of the merged count.

WHAT THE BOUND CAN SEE.  ``WRONG`` names the formulations it has to reject (tests/test_host_bn2d_bound.py).
``piece_chan_fp32`` is the honest evaluation -- the shifted sums in the threads', the tree's and the waves' order, the
lane-strided Chan update and its tree, the file's formulas, all in fp32 -- that has to stay inside on every input set of the
GPU test (tests/test_gpu_bn2d_f64.py)."""
import math

import numpy as np
import torch

import row_bn_f64_ref as R
from row_bn_f64_ref import (EPS, MOMENTUM, U32, UNDECIDED_CAP, backward64, backward_bound, f32, floor_ulp, forward64,  # noqa: F401
                            forward_bound, g_, running64, worst)

THREADS = 256
WAVE = 64
CHUNK = 8192             # kB2Chunk: elements of one plane per statistics piece
APPLY_CHUNK = 4096       # kB2ApplyChunk: elements of one plane per elementwise workgroup
FIN_LANES = 64
F32 = torch.float32


def rows(t):
    """an NCHW map as [B hw, C] rows (row = b hw + pixel: the order of the pieces); anything else as it is"""
    if t is None or t.dim() != 4:
        return t
    b, c = t.shape[:2]
    return t.reshape(b, c, -1).permute(0, 2, 1).reshape(-1, c)


# ---- the kernels' shape, restated ---------------------------------------------------------------------------------------------

def float4_form(hw):
    return hw % 4 == 0


def splits(hw, chunk=CHUNK):
    """b2_splits"""
    return -(-hw // chunk)


def piece_counts(hw, chunk=CHUNK):
    return [min(chunk, hw - s * chunk) for s in range(splits(hw, chunk))]


def num_pieces(b, hw):
    return b * splits(hw)


def workspace_bytes(b, c, hw):
    return c * num_pieces(b, hw) * 2 * 4 if min(b, c, hw) > 0 else 0


def _block_depth(live):
    """the shuffle tree over the live lanes of a wave, then the live waves in order"""
    return math.ceil(math.log2(min(WAVE, live))) + -(-live // WAVE) - 1


def piece_depth(cnt, hw):
    """additions that round on the way of one value into s1 / s2 of a statistics piece of ``cnt`` elements"""
    items = cnt // 4 if float4_form(hw) else cnt
    return (2 if float4_form(hw) else 0) + -(-items // THREADS) - 1 + _block_depth(min(THREADS, items))


def bwd_piece_depth(cnt, hw):
    """the same for the sums of bn2d_bwd_partial_kernel, which adds the four values of a float4 one after the other"""
    items = cnt // 4 if float4_form(hw) else cnt
    per_thread = -(-items // THREADS) * (4 if float4_form(hw) else 1)
    return per_thread - 1 + _block_depth(min(THREADS, items))


def merge_depth(npieces):
    return max(0, min(npieces - 1, -(-npieces // FIN_LANES) + 5))


def sum_depth(b, hw, world=1):
    """Dn of step 7; ``b``: the images of the rank that has most"""
    return max(bwd_piece_depth(cnt, hw) for cnt in set(piece_counts(hw))) + merge_depth(num_pieces(b, hw)) + world - 1


# ---- the bound: steps 1-3 -----------------------------------------------------------------------------------------------------

def _piece_moments(x):
    """per piece, in the order (b, split), in float64: count [np]; shift, mean, centred M2, S1 = sum (x - shift),
    A1 = sum |x - shift| [np, C]"""
    b, c = x.shape[:2]
    xd = x.double().reshape(b, c, -1)
    hw = xd.shape[2]
    s = splits(hw)
    xp = torch.nn.functional.pad(xd, (0, s * CHUNK - hw)).reshape(b, c, s, CHUNK)
    cnt = torch.tensor(piece_counts(hw), dtype=torch.float64, device=x.device)
    valid = (torch.arange(CHUNK, device=x.device)[None, :] < cnt[:, None]).to(torch.float64)
    shift = xp[..., 0]
    d = (xp - shift[..., None]) * valid
    s1, a1 = d.sum(-1), d.abs().sum(-1)
    mean = shift + s1 / cnt
    dev = (xp - mean[..., None]) * valid
    m2 = (dev * dev).sum(-1)

    def flat(t):
        return t.permute(0, 2, 1).reshape(b * s, c)
    return cnt.repeat(b), flat(shift), flat(mean), flat(m2), flat(s1), flat(a1)


def _rank_errors(x, shift_terms=True):
    """steps 1-3 for one rank's map: (n, mu, M2, E, dM2).  ``shift_terms=False``: q_b as if the sums carried M2_b alone, which
    the honest evaluation does NOT meet on ``first8`` (tests/test_host_bn2d_bound.py)"""
    u = U32
    b, hw = x.shape[0], x[0, 0].numel()
    nb, shift, mean_b, m2_b, s1, a1 = _piece_moments(x)
    dp = torch.tensor([float(piece_depth(cnt, hw)) for cnt in piece_counts(hw)], dtype=torch.float64, device=x.device).repeat(b)
    n_ = nb[:, None]
    e1 = g_(dp + 1)[:, None] * a1
    e_b = e1 / n_ + u * ((mean_b - shift).abs() + e1 / n_) + u * (mean_b.abs() + 2 * e1 / n_)
    shifted = n_ * (mean_b - shift) ** 2                  # n_b (m_b - shift)^2: what the shifted sums carry on top of M2_b
    e2 = g_(dp + 3)[:, None] * (m2_b + shifted)
    ec = (2 * s1.abs() * e1 + e1 * e1) / n_ + g_(2) * (s1.abs() + e1) ** 2 / n_
    q_b = e2 + ec + u * (m2_b + e2 + ec) if shift_terms else (g_(dp + 3)[:, None] + u) * m2_b
    mu, m2, e, dm2 = R._chan_errors(nb, mean_b, e_b, q_b.sum(0), m2_b.sum(0), merge_depth(len(nb)), 7)
    return nb.sum(), mu, m2, e, dm2


def stat_errors(ranks, eps=EPS, shift_terms=True):
    """steps 1-4 for one rank's NCHW map (a tensor) or for several (a list, merged in rank order):
    {'E', 'dM2', 'dv', 'dr', 'dunb', 'n'}"""
    u = U32
    per = [_rank_errors(x, shift_terms) for x in (ranks if isinstance(ranks, (list, tuple)) else [ranks])]
    if len(per) > 1:
        nr = torch.stack([p[0] for p in per])
        mu, m2, e, dm2 = R._chan_errors(nr, torch.stack([p[1] for p in per]), torch.stack([p[3] for p in per]),
                                        sum(p[4] for p in per), sum(p[2] for p in per), len(per) - 1, 1)
        n = float(nr.sum())
    else:
        n, mu, m2, e, dm2 = per[0]
        n = float(n)
    var = m2 / n
    dv = dm2 / n + u * (var + dm2 / n)
    r = 1.0 / torch.sqrt(var + eps)
    r_lo = 1.0 / torch.sqrt((var - dv).clamp(min=0.0) + eps)
    r_hi = 1.0 / torch.sqrt(var + dv + eps)
    dr = torch.maximum(r_lo - r, r - r_hi) + 3 * u * r_lo
    dunb = (dm2 / (n - 1) + u * (m2 + dm2) / (n - 1)) if n > 1 else dv
    return {'E': e, 'dM2': dm2, 'dv': dv, 'dr': dr, 'dunb': dunb, 'n': n}


eval_errors = R.eval_errors           # the mean is an input, invstd = 1 / sqrtf(var + eps) of an input: dr = 3 u r


# ---- the input sets (shared by the host test and the GPU test) ----------------------------------------------------------------

SHAPES = ((1, 4, 1, 2), (2, 4, 7, 9), (4, 1, 9, 16), (3, 8, 32, 32), (2, 4, 64, 64), (2, 4, 17, 241), (2, 4, 64, 128),
          (2, 4, 3, 2731), (2, 4, 4, 2049), (33, 4, 3, 2731), (5, 4, 282, 378), (2, 130, 5, 5), (6, 64, 45, 80))
KINDS = ('randn', 'mean1e3', 'constch', 'scales', 'first8')
MODES = ('plain', 'relu', 'res')
AFFINE_FALSE_SHAPE = (2, 4, 17, 241)
OUTPUTS = R.OUTPUTS

# (shape, kind) -> the seed of a case whose seed-0 draw has more than UNDECIDED_CAP of its elements undecided in some mode
SEEDS = {}


def make_case(shape, kind, seed=None, affine=True):
    """CPU tensors of one case, the same on every machine: fp32 NCHW maps x, dy, res, gamma = 1 + 0.5 randn and beta = randn
    (None with affine=False), running statistics rm / rv that are not the initial 0 / 1."""
    b, c, h, w = shape
    seed = SEEDS.get((tuple(shape), kind), 0) if seed is None else seed
    g = torch.Generator().manual_seed(100003 * seed + 131 * b + 17 * c + 7 * h + w + 1009 * KINDS.index(kind))
    x = torch.randn(b, c, h * w, generator=g)
    gamma = 1.0 + 0.5 * torch.randn(c, generator=g)
    if kind == 'mean1e3':        # mean 1e3, spread 1: where E[x^2] - mean^2 and a single accumulator lose the variance
        x = x + 1e3
    elif kind == 'constch':      # every fourth channel holds one value everywhere: variance 0, invstd = 1 / sqrt(eps)
        x[:, ::4] = torch.randn(1, c, 1, generator=g)[:, ::4]
    elif kind == 'scales':       # channel j scaled by 2^(j mod 13 - 6), gamma by its inverse
        s = 2.0 ** (torch.arange(c) % 13 - 6).float()
        x, gamma = x * s[None, :, None], gamma / s
    elif kind == 'first8':       # the first element of every statistics piece of every plane 8 spreads off: the shift is not typical
        x[:, :, ::CHUNK] += 8.0
    elif kind != 'randn':
        raise ValueError(kind)
    x = x.reshape(b, c, h, w)
    flat = rows(x)
    rm = flat.mean(0) + 0.1 * torch.randn(c, generator=g)
    rv = flat.var(0, unbiased=False) * (0.5 + torch.rand(c, generator=g)) + 0.1
    return {'x': x, 'dy': torch.randn(b, c, h, w, generator=g), 'res': torch.randn(b, c, h, w, generator=g),
            'gamma': gamma if affine else None, 'beta': torch.randn(c, generator=g) if affine else None, 'rm': rm, 'rv': rv}


def cases(shape):
    """(kind, mode, affine) of every case of one shape"""
    out = [(kind, mode, True) for kind in KINDS for mode in MODES]
    if tuple(shape) == AFFINE_FALSE_SHAPE:
        out += [('randn', mode, False) for mode in MODES]
    return out


def evaluate64(case, mode, training=True, eps=EPS, momentum=MOMENTUM, se=None, ranks=None):
    """references and bounds of one case in the layout of ``rows``: ({output: float64 value}, {output: bound}, the undecided
    mask, its share).  ``se``: stat_errors of the case's x where the caller has them; ``ranks``: the images per rank of a
    SyncBatchNorm2d evaluation (x, dy, res are then all ranks' images as one batch)."""
    x, dy = rows(case['x']), rows(case['dy'])
    res = rows(case['res']) if mode == 'res' else None
    relu = mode in ('relu', 'res')
    hw = case['x'][0, 0].numel()
    f = forward64(x, case['gamma'], case['beta'], eps, res, relu, None if training else (case['rm'], case['rv']))
    if se is None:
        if not training:
            se = eval_errors(f)
        elif ranks:
            se = stat_errors(list(torch.split(case['x'], list(ranks))), eps)
        else:
            se = stat_errors(case['x'], eps)
    fb = forward_bound(f, se, case['gamma'], case['beta'], F32, res, (case['rm'], case['rv']) if training else None, momentum)
    b = backward64(dy, f, case['gamma'], fb['undecided'] if relu else None)
    depth = sum_depth(max(ranks) if ranks else case['x'].shape[0], hw, len(ranks) if ranks else 1)
    bb = backward_bound(dy, f, b, fb, se, case['gamma'], F32, depth=depth)
    ref = {'y': f['y'], 'mean': f['mu'], 'invstd': f['r'], 'dx': b['dx'], 'dres': b['dres'], 'dgamma': b['dgamma'], 'dbeta': b['dbeta']}
    bound = {'y': fb['y'], 'mean': fb['mean'], 'invstd': fb['invstd'], 'dx': bb['dx'], 'dres': bb['dres'], 'dgamma': bb['dgamma'],
             'dbeta': bb['dbeta'], 'allow': bb['allow'], 'pre_err': fb['pre_err']}
    if training:
        ref['running_mean'], ref['running_var'] = running64(case['rm'], case['rv'], f, momentum)
        bound['running_mean'], bound['running_var'] = fb['running_mean'], fb['running_var']
    if relu:
        for k in ('dx', 'dres'):
            ref[k + '_alt'], bound[k + '_alt'] = b[k + '_alt'], bb[k + '_alt']
    und = fb['undecided']
    return ref, bound, und, float(und.double().mean()) if und.numel() else 0.0


def check(got, ref, bound, und, names=None):
    """{output: (passes, largest error / bound, largest error)}; NCHW outputs are compared as rows"""
    return R.check({k: rows(v) for k, v in got.items() if torch.is_tensor(v)}, ref, bound, und, names)


# ---- fp32 evaluations: the honest one and the wrong ones ----------------------------------------------------------------------

def _block_sum_fp32(v):
    """[..., 256] the threads' values -> the workgroup's sum in the order of b2_block_sum2"""
    w = v.reshape(*v.shape[:-1], THREADS // WAVE, WAVE)
    for off in (32, 16, 8, 4, 2, 1):
        other = torch.zeros_like(w)
        other[..., :WAVE - off] = w[..., off:]            # (lanes past 64 - off never reach lane 0)
        w = w + other
    out = w[..., 0, 0]
    for k in range(1, THREADS // WAVE):
        out = out + w[..., k, 0]
    return out


def piece_stats_fp32(x):
    """bn2d_stats_partial_kernel in fp32, in its order: (count [np], mean [np, C], M2 [np, C]) in the order (b, split)"""
    b, c = x.shape[:2]
    xf = x.float().reshape(b, c, -1)
    hw = xf.shape[2]
    s = splits(hw)
    xp = torch.nn.functional.pad(xf, (0, s * CHUNK - hw)).reshape(b, c, s, CHUNK)
    cnt = torch.tensor(piece_counts(hw), dtype=F32)
    valid = (torch.arange(CHUNK)[None, :] < cnt[:, None]).to(F32)
    d = (xp - xp[..., :1]) * valid                          # (an element past the piece: d = 0, and adding it is exact)
    if float4_form(hw):
        d = d.reshape(b, c, s, CHUNK // (4 * THREADS), THREADS, 4)
        t1 = (d[..., 0] + d[..., 1]) + (d[..., 2] + d[..., 3])
        t2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + (d[..., 2] * d[..., 2] + d[..., 3] * d[..., 3])
    else:
        t1 = d.reshape(b, c, s, CHUNK // THREADS, THREADS)
        t2 = t1 * t1
    a1, a2 = t1[..., 0, :], t2[..., 0, :]
    for k in range(1, t1.shape[-2]):
        a1, a2 = a1 + t1[..., k, :], a2 + t2[..., k, :]
    s1, s2 = _block_sum_fp32(a1), _block_sum_fp32(a2)
    mean = xp[..., 0] + s1 / cnt
    m2 = (s2 - s1 * s1 / cnt).clamp(min=0.0)
    return cnt.repeat(b), mean.permute(0, 2, 1).reshape(b * s, c), m2.permute(0, 2, 1).reshape(b * s, c)


def finalize_fp32(nb, mean_b, m2_b, first_trip_only=False, equal_weights=False):
    """bn2d_stats_finalize_kernel in fp32: lane l takes pieces l, l + 64, ..., then the 6-level tree -> (count, mean [C],
    M2 [C]).  ``first_trip_only``, ``equal_weights``: two of the wrong forms"""
    npieces, c = mean_b.shape
    trips = -(-npieces // FIN_LANES)
    pad = trips * FIN_LANES - npieces
    nbp = torch.cat([nb, nb.new_zeros(pad)]).reshape(trips, FIN_LANES)
    mbp = torch.cat([mean_b, mean_b.new_zeros(pad, c)]).reshape(trips, FIN_LANES, c)
    qbp = torch.cat([m2_b, m2_b.new_zeros(pad, c)]).reshape(trips, FIN_LANES, c)
    na, ka = torch.zeros(FIN_LANES), torch.zeros(FIN_LANES)          # ka: pieces merged so far (the equal-weights form)
    mean, m2 = torch.zeros(FIN_LANES, c), torch.zeros(FIN_LANES, c)

    def update(na, ka, mean, m2, nb_, kb_, mb_, qb_):
        live = nb_ != 0
        tot = na + nb_
        safe = torch.where(live, tot, torch.ones_like(tot))
        delta = mb_ - mean
        w = kb_ / torch.where(live, ka + kb_, torch.ones_like(ka)) if equal_weights else nb_ / safe
        mean_new = mean + delta * w[:, None]
        m2_new = m2 + (qb_ + delta * delta * (na * nb_ / safe)[:, None])
        return (torch.where(live, tot, na), torch.where(live, ka + kb_, ka), torch.where(live[:, None], mean_new, mean),
                torch.where(live[:, None], m2_new, m2))

    for t in range(1 if first_trip_only else trips):
        na, ka, mean, m2 = update(na, ka, mean, m2, nbp[t], (nbp[t] != 0).float(), mbp[t], qbp[t])
    for off in (32, 16, 8, 4, 2, 1):
        def down(v):
            o = torch.zeros_like(v)
            o[:FIN_LANES - off] = v[off:]
            return o
        na, ka, mean, m2 = update(na, ka, mean, m2, down(na), down(ka), down(mean), down(m2))
    return float(na[0]), mean[0], m2[0]


def _finish_fp32(case, mode, mean, invstd, unbiased=None, inv_n=None, unmasked_sums=False, momentum=MOMENTUM):
    """the file's forward and backward formulas in fp32 from (mean, invstd); ``unbiased`` given: the training form"""
    xf, dyf = rows(case['x']), rows(case['dy'])
    n, c = xf.shape
    gm = case['gamma'] if case['gamma'] is not None else torch.ones(c)
    bt = case['beta'] if case['beta'] is not None else torch.zeros(c)
    xhat = (xf - mean) * invstd
    pre = xhat * gm + bt
    if mode == 'res':
        pre = pre + rows(case['res'])
    relu = mode in ('relu', 'res')
    dym = torch.where(pre > 0, dyf, torch.zeros_like(dyf)) if relu else dyf
    dsum = dyf if unmasked_sums else dym
    dbeta, dgamma = dsum.sum(0), (dsum * xhat).sum(0)
    out = {'y': pre.clamp(min=0.0) if relu else pre, 'mean': mean, 'invstd': invstd, 'dres': dym, 'dgamma': dgamma, 'dbeta': dbeta}
    if unbiased is not None:
        i = torch.tensor(1.0, dtype=F32) / n if inv_n is None else torch.tensor(inv_n, dtype=F32)
        m = torch.tensor(momentum, dtype=F32)
        out['dx'] = (gm * invstd) * (dym - dbeta * i - xhat * (dgamma * i))
        out['running_mean'], out['running_var'] = (1 - m) * case['rm'] + m * mean, (1 - m) * case['rv'] + m * unbiased
    else:
        out['dx'] = (gm * invstd) * dym
    return out


def _from_stats(case, mode, na, mean, m2, eps=EPS, **kw):
    var = m2 / na
    invstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))
    return _finish_fp32(case, mode, mean, invstd, m2 / (na - 1.0) if na > 1 else var, **kw)


def piece_chan_fp32(case, mode, training=True, eps=EPS):
    """the honest evaluation, fp32 throughout, in the kernels' order"""
    if not training:
        return _finish_fp32(case, mode, case['rm'], 1.0 / torch.sqrt(case['rv'] + torch.tensor(eps, dtype=F32)))
    return _from_stats(case, mode, *finalize_fp32(*piece_stats_fp32(case['x'])), eps=eps)


def _wrong_e_x2(case, mode):
    xf = rows(case['x'])
    n = xf.shape[0]
    mean = xf.mean(0)
    var = ((xf * xf).mean(0) - mean * mean).clamp(min=0.0)
    return _from_stats(case, mode, float(n), mean, var * n)


def _serial_sum(t):
    """sum over the rows, ONE fp32 accumulator per channel (one rounding per addition)"""
    return torch.from_numpy(np.add.accumulate(t.contiguous().numpy(), axis=0, dtype=np.float32)[-1].copy())


def _wrong_one_accumulator(case, mode):
    xf = rows(case['x'])
    n = xf.shape[0]
    mean = _serial_sum(xf) / n
    dev = xf - mean
    return _from_stats(case, mode, float(n), mean, _serial_sum(dev * dev))


def _wrong_equal_weights(case, mode):
    return _from_stats(case, mode, *finalize_fp32(*piece_stats_fp32(case['x']), equal_weights=True))


def _wrong_full_pieces(case, mode):
    nb, mean_b, m2_b = piece_stats_fp32(case['x'])
    return _from_stats(case, mode, *finalize_fp32(torch.full_like(nb, float(CHUNK)), mean_b, m2_b))


def _wrong_first_64_pieces(case, mode):
    return _from_stats(case, mode, *finalize_fp32(*piece_stats_fp32(case['x']), first_trip_only=True))


def _wrong_inv_n(case, mode):
    return _from_stats(case, mode, *finalize_fp32(*piece_stats_fp32(case['x'])), inv_n=1.0 / case['x'][0, 0].numel())


def _wrong_unmasked_sums(case, mode):
    return _from_stats(case, mode, *finalize_fp32(*piece_stats_fp32(case['x'])), unmasked_sums=True)


# the formulations the bound has to reject: name -> f(case, mode) -> the outputs of piece_chan_fp32
WRONG = {'variance as E[x^2] - mean^2': _wrong_e_x2,
         'one fp32 accumulator per channel': _wrong_one_accumulator,
         'pieces merged with equal weights': _wrong_equal_weights,
         'every piece counted as 8192 elements': _wrong_full_pieces,
         'pieces beyond the 64th dropped': _wrong_first_64_pieces,
         'inv_n = 1 / hw': _wrong_inv_n,
         'parameter gradients from the unmasked dy': _wrong_unmasked_sums}
