"""float64 reference of the fused window attention (csrc/sptr.hip) on a SYNTHETIC PLAN (test helper).

The kernels take a plan, not coordinates: a permutation ``sort_idx`` (sorted position -> token), the window of every
sorted position (``wstart``, ``wlen``), quantised in-window coordinates ``qc`` int32 [n, 3] and, on the spherical
branch, the fp32 radial coordinate ``radial`` [n] -- both per SORTED POSITION -- next to q, k, v [n, h, 16] and dout
[n, h, 16] per TOKEN and the three tables [L, 3, h, 16].  This module restates the operation on exactly those inputs:

  pairs    every (query, key) of a window, from ``wstart`` / ``wlen`` (the order of oracle.sptr_ref.precompute_all);
  rows     integer arithmetic: r = qc_i - qc_j + qgl - 1 per axis; spherical branch: axis 2 is the exponential split of
           spherical_transformer.py:39-64 (as oracle/sptr_ref.py:88-103 restates it) evaluated in float64 on the fp32
           radial values, then all three rows are clamped to [0, 2 * qgl - 1];
  outputs  out, lse, dq, dk, dv, dTq, dTk, dTv by explicit index sums (no autograd), in the dtype asked for, and for
           each of them the MAGNITUDE SUM its rounding error is relative to: the same sum with every factor replaced by
           its absolute value and ds = p (dp - delta) by p (|dp| + |delta|) -- the subtraction cancels, so the error of
           a gradient does not scale with |ds|.

The gate of tests/test_gpu_sptr_splits.py is elementwise, twice:

    |kernel - float64| <= KAPPA[kind]     * magnitude     + 1e-30       (the sums above)
    |kernel - float64| <= KAPPA_ABS[kind] * magnitude_abs + 1e-30       (every TERM by its absolute value)
    |lse - lse64|      <= KAPPA['lse'] * (1 + |lse64|)

The second line exists because a FACTOR can itself cancel: a window of one token has out = v + Tv(r0) + Tv(r1) + Tv(r2)
and magnitude |out|, so an element where the four terms cancel to 2e-4 carries their fp32 rounding (1e-7) as a relative
error of 5e-4 -- and the maximum over all elements, which is what a coefficient has to cover, is set by those few
elements (k + Tq and q + Tk cancel the same way in dq and dk).  magnitude_abs replaces k + Tq, q + Tk, v + Tv, dp and
delta by the sums of the absolute values of their terms; no element is ill-conditioned against it, its coefficient is
a few fp32 roundings, and it is the bound that holds the typical element tightly.

Neither coefficient is taken from a kernel.  tests/test_sptr_f64_reference.py evaluates THIS formulation in fp32 on the
CPU on every case of the GPU file, takes rho[kind] = max(err / magnitude) against float64 and requires
KAPPA[kind] = 8 * rho rounded up to a power of two (8: __expf, the online softmax and another summation order).
Measured (torch 2.x CPU; its vector width moves the last digits of an fp32 evaluation, so the test pins the recorded
figure within a factor of two and the power of two exactly):

    kind   rho       KAPPA    rho_abs   KAPPA_ABS
    out    4.84e-4   2^-8     2.36e-6   2^-15
    lse    6.49e-7   2^-17    (the same: relative to 1 + |lse64|)
    dq     1.53e-4   2^-9     2.42e-7   2^-18
    dk     1.70e-5   2^-12    2.66e-7   2^-18
    dv     1.55e-6   2^-16    1.55e-6   2^-16
    dTq    1.14e-6   2^-16    1.23e-7   2^-19
    dTk    7.68e-7   2^-17    8.81e-8   2^-20
    dTv    1.31e-6   2^-16    1.31e-6   2^-16

No pair of a case sits near a radial bin edge: the exponential split floors a logarithm, where fp32 and float64 may
legitimately disagree.  ``Case`` redraws (same generator) the radial value of every token that has a pair with
x = (|dr| + 2a) / a within ``edge_margin(x)`` of a bin edge: a power of two (the floor of log2) or 3 * 2^m (the
half-bin test |dr| >= (3 * 2^m - 2) a, i.e. x >= 3 * 2^m).  The diagonal pair dr = 0 is exempt (x = 2 exactly: both
precisions give log(2) / log(2) = 1).  The margin is max(1e-3, 16 fp32 ulps of the binade ABOVE x): logf, the division
by ln 2 and the three roundings before them move x by about 1.4e-6 x, i.e. 12 ulps just below a power of two, where the
ulp is half of what it is above."""
import numpy as np
import torch

QGL = 24
SPLIT_A = float(np.float32(0.0125))          # the value the kernels see (a float argument of the C ABI)
Q_SCALE = 0.25
SPLITS = (1, 2, 4, 8, 16)
KINDS = ('out', 'lse', 'dq', 'dk', 'dv', 'dTq', 'dTk', 'dTv')

# measured by tests/test_sptr_f64_reference.py::test_kappa_is_eight_rho_of_the_fp32_evaluation over all cases of
# gpu_cases(): fp32 evaluation of this formulation against float64, max over elements and cases of err / magnitude
RHO = {'out': 4.84e-4, 'lse': 6.49e-7, 'dq': 1.53e-4, 'dk': 1.70e-5, 'dv': 1.55e-6, 'dTq': 1.14e-6, 'dTk': 7.68e-7,
       'dTv': 1.31e-6}
RHO_ABS = {'out': 2.36e-6, 'lse': 6.49e-7, 'dq': 2.42e-7, 'dk': 2.66e-7, 'dv': 1.55e-6, 'dTq': 1.23e-7, 'dTk': 8.81e-8,
           'dTv': 1.31e-6}


def pow2_ceil(x):
    return float(2.0 ** np.ceil(np.log2(x)))


KAPPA = {k: pow2_ceil(8 * r) for k, r in RHO.items()}
KAPPA_ABS = {k: pow2_ceil(8 * r) for k, r in RHO_ABS.items()}


# ---- plan ----------------------------------------------------------------------------------------------------------

def pair_lists(wstart, wlen):
    """(i0, i1): sorted positions of the query and the key of every pair, queries ascending, keys ascending."""
    wl = np.asarray(wlen, dtype=np.int64)
    ws = np.asarray(wstart, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(wl)])
    i0 = np.repeat(np.arange(len(wl), dtype=np.int64), wl)
    i1 = ws[i0] + (np.arange(off[-1], dtype=np.int64) - off[i0])
    return i0, i1


def exp_split_x(radial, i0, i1, a):
    """float64 (dr, x = (|dr| + 2a) / a) of every pair, on the fp32 radial values."""
    r = np.asarray(radial).astype(np.float64)
    d = r[i0] - r[i1]
    return d, (np.abs(d) + 2 * a) / a


def edge_margin(x):
    """max(1e-3, 16 fp32 ulps) in units of x; the ulp is that of the binade above x (see the module docstring)."""
    k = np.floor(np.log2(x))
    return np.maximum(1e-3, 16.0 * 2.0 ** (k + 1 - 23))


def edge_distance(x):
    """distance of x >= 2 to the nearest bin edge of the exponential split: 2^k, 3 * 2^(k-1), 2^(k+1)."""
    k = np.floor(np.log2(x))
    lo = 2.0 ** k
    return np.minimum(np.minimum(np.abs(x - lo), np.abs(x - 2 * lo)), np.abs(x - 1.5 * lo))


def near_edge(radial, i0, i1, a):
    """bool per pair: off the diagonal and within the margin of a bin edge."""
    _, x = exp_split_x(radial, i0, i1, a)
    return (i0 != i1) & (edge_distance(x) <= edge_margin(x))


def rel_rows(qc, radial, i0, i1, qgl, a):
    """int64 [M, 3] table rows of every pair (sptr/modules.py:40-51, spherical_transformer.py:39-64)."""
    qc = np.asarray(qc, dtype=np.int64)
    r = qc[i0] - qc[i1] + qgl - 1
    if a > 0:
        d, x = exp_split_x(radial, i0, i1, a)
        flag = (d >= 0).astype(np.float64)
        idx = 2 * np.floor(np.log(x) / np.log(2.0)) - 2
        idx = idx + ((3 * 2.0 ** np.floor(idx / 2) - 2) * a <= np.abs(d))
        idx = idx * (2 * flag - 1) + (flag - 1)
        r[:, 2] = idx.astype(np.int64) + 24
        r = np.clip(r, 0, 2 * qgl - 1)
    return r


# ---- cases ---------------------------------------------------------------------------------------------------------

def window_lengths(S, big, rng):
    """Window lengths of a case, shuffled.  Small cases: every length at which S lanes per token change what a lane
    does (1, S - 1, S, S + 1, 2S + 1, 3S - 1), lengths around the 64-lane wave and a few large windows, then filler
    windows of 1..9 tokens until n is ~100 past 128 workgroups of 128 / S tokens (S > 1: the persistent backward grid
    of 128 workgroups takes a second pass) and no multiple of 128 / S.  Big cases (S = 1, grid of 512 workgroups of 128
    tokens): 66 000 tokens in windows of 1..9 and one of 129."""
    if big:
        total, lens = 66000, [129]
    else:
        lens = [1] + ([S - 1] if S > 1 else []) + [S, S + 1, 2 * S + 1, 3 * S - 1, 37, 64, 65, 129, 385]
        total = (128 * (128 // S) if S > 1 else 1024) + 100
    have = sum(lens)
    while have < total:
        w = int(rng.integers(1, 10))
        if big:
            w = min(w, total - have)
        lens.append(w)
        have += w
    if not big:
        while have % (128 // S) == 0:
            lens.append(1)
            have += 1
    lens = np.asarray(lens, dtype=np.int64)
    return lens[rng.permutation(len(lens))]


class Case:
    """Inputs of one case, as the C ABI takes them (CPU tensors)."""

    def __init__(self, S, sphere, h=2, big=False, lens=None):
        self.S, self.sphere, self.h, self.big = S, sphere, h, big
        rng = np.random.default_rng([20, S, int(sphere), h, int(big)])
        lens = window_lengths(S, big, rng) if lens is None else np.asarray(lens, dtype=np.int64)
        self.window_lengths = lens
        n = self.n = int(lens.sum())
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
        self.window_of = np.repeat(np.arange(len(lens)), lens)            # window index of every sorted position
        self.wstart = starts[self.window_of].astype(np.int32)
        self.wlen = lens[self.window_of].astype(np.int32)
        self.sort_idx = rng.permutation(n).astype(np.int32)
        self.qgl = QGL
        self.L = 2 * QGL if sphere else 2 * QGL - 1
        self.a = SPLIT_A if sphere else 0.0
        self.qc_span = 25 if sphere else 24       # (a spherical coordinate of 24: the clamped base of hist_base)
        self.qc = rng.integers(0, self.qc_span, (n, 3)).astype(np.int32)
        self.q_scale = Q_SCALE
        self.i0, self.i1 = pair_lists(self.wstart, self.wlen)
        self.radial, self.redraws = None, 0
        if sphere:
            # half the windows near the origin of the split (rows around 24), half far out (both clamp ends, rows 0 and 47)
            hi = np.where(np.arange(len(lens)) % 2 == 0, 2.0, 120.0)[self.window_of]
            radial = (rng.random(n) * hi).astype(np.float32)
            for self.redraws in range(200):
                bad = near_edge(radial, self.i0, self.i1, self.a)
                if not bad.any():
                    break
                tok = np.unique(np.concatenate([self.i0[bad], self.i1[bad]]))
                radial[tok] = (rng.random(len(tok)) * hi[tok]).astype(np.float32)
            else:
                raise AssertionError('radial redraw did not terminate')
            self.radial = radial
        f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
        self.q, self.k, self.v, self.dout = f(n, h, 16), f(n, h, 16), f(n, h, 16), f(n, h, 16)
        self.tq, self.tk, self.tv = (0.3 * f(self.L, 3, h, 16) for _ in range(3))
        self.rows = rel_rows(self.qc, self.radial, self.i0, self.i1, self.qgl, self.a)

    def edge_slack(self):
        """min over off-diagonal pairs of distance / margin (> 1: no pair near an edge); inf on the cubic branch."""
        if not self.sphere:
            return float('inf')
        _, x = exp_split_x(self.radial, self.i0, self.i1, self.a)
        off = self.i0 != self.i1
        return float((edge_distance(x[off]) / edge_margin(x[off])).min()) if off.any() else float('inf')


def gpu_cases():
    """(S, sphere, merge, h, big) of the 20 cases of tests/test_gpu_sptr_splits.py."""
    out = []
    for sphere in (False, True):
        for S in SPLITS:
            out.append((S, sphere, True, 3 if S == 4 else 2, False))        # one case per branch with three heads
            if S > 1:
                out.append((S, sphere, False, 2, False))
        out.append((1, sphere, True, 2, True))
    return out


def case_id(c):
    S, sphere, merge, h, big = c
    return '%s-S%d-h%d%s%s' % ('sphere' if sphere else 'cubic', S, h, '' if merge else '-twolaunch', '-66k' if big else '')


_CASES = {}


def get_case(S, sphere, h=2, big=False):
    key = (S, sphere, h, big)
    if key not in _CASES:
        _CASES[key] = Case(S, sphere, h, big)
    return _CASES[key]


# ---- the operation -------------------------------------------------------------------------------------------------

def _tsum(table, rows):
    return table[rows[:, 0], 0] + table[rows[:, 1], 1] + table[rows[:, 2], 2]            # [M, h, 16]


def forward(q, k, v, tq, tk, tv, sort_idx, i0, i1, rows, q_scale):
    """(out [n, h, 16] per token, lse [n, h] per sorted position, p [M, h]); differentiable torch operators."""
    n, h, _ = q.shape
    t0, t1 = sort_idx[i0], sort_idx[i1]
    kj = k[t1]
    s = ((q * q_scale)[t0] * (kj + _tsum(tq, rows))).sum(-1) + (kj * _tsum(tk, rows)).sum(-1)
    m = torch.full((n, h), -float('inf'), dtype=s.dtype, device=s.device)
    m = m.scatter_reduce(0, i0[:, None].expand_as(s), s.detach(), reduce='amax')
    l = torch.zeros_like(m).index_add(0, i0, (s - m[i0]).exp())
    lse = m + l.log()
    p = (s - lse[i0]).exp()
    out = torch.zeros_like(q).index_add(0, t0, p[..., None] * (v[t1] + _tsum(tv, rows)))
    return out, lse, p


def reference(case, dtype=torch.float64, device='cpu', i0=None, i1=None, rows=None, magnitudes=True):
    """{kind: tensor} and, with ``magnitudes``, the two {kind: magnitude sum}: explicit index sums in ``dtype``.  ``i0, i1,
    rows`` override the case's pair list and rows (the corruptions of test_sptr_f64_reference.py)."""
    dev = torch.device(device)
    t = lambda x: x.to(device=dev, dtype=dtype)
    ix = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.int64, device=dev)
    q, k, v, dout, tq, tk, tv = (t(x) for x in (case.q, case.k, case.v, case.dout, case.tq, case.tk, case.tv))
    i0 = ix(case.i0 if i0 is None else i0)
    i1 = ix(case.i1 if i1 is None else i1)
    rows = ix(case.rows if rows is None else rows)
    sort_idx = ix(case.sort_idx)
    qs = case.q_scale
    out, lse, p = forward(q, k, v, tq, tk, tv, sort_idx, i0, i1, rows, qs)
    t0, t1 = sort_idx[i0], sort_idx[i1]
    P = p[..., None]
    kq = k[t1] + _tsum(tq, rows)                      # what dq sums
    qk = (q * qs)[t0] + _tsum(tk, rows)               # what dk sums
    vt = v[t1] + _tsum(tv, rows)
    do, qi, kj = dout[t0], (q * qs)[t0], k[t1]
    delta = (dout * out).sum(-1)[t0]                  # [M, h]
    dp = (do * vt).sum(-1)
    ds = (p * (dp - delta))[..., None]

    def tok(index, src):
        return torch.zeros_like(q).index_add(0, index, src)

    def tab(src):
        g = torch.zeros_like(tq)
        for ax in range(3):
            g[:, ax] = torch.zeros_like(tq[:, 0]).index_add(0, rows[:, ax], src)
        return g

    res = {'out': out, 'lse': lse, 'dq': qs * tok(t0, ds * kq), 'dk': tok(t1, ds * qk), 'dv': tok(t1, P * do),
           'dTq': tab(ds * qi), 'dTk': tab(ds * kj), 'dTv': tab(P * do)}
    if not magnitudes:
        return res

    def asum(table):
        return _tsum(table.abs(), rows)

    def mags(akq, aqk, avt, adp, adelta, aout):
        ads = (p * (adp + adelta))[..., None]
        return {'out': aout, 'lse': 1 + lse.abs(), 'dq': qs * tok(t0, ads * akq), 'dk': tok(t1, ads * aqk),
                'dv': tok(t1, P * do.abs()), 'dTq': tab(ads * qi.abs()), 'dTk': tab(ads * kj.abs()),
                'dTv': tab(P * do.abs())}

    # the issue's sums: every FACTOR by its absolute value, ds by p (|dp| + |delta|)
    mag = mags(kq.abs(), qk.abs(), vt.abs(), dp.abs(), delta.abs(), tok(t0, P * vt.abs()))
    # every TERM by its absolute value: a factor that is itself a sum (k + Tq rows, v + Tv rows, dp, delta) can cancel
    avt = v[t1].abs() + asum(tv)
    aout = tok(t0, P * avt)
    mag_abs = mags(kj.abs() + asum(tq), qi.abs() + asum(tk), avt, (do.abs() * avt).sum(-1),
                   (dout.abs() * aout).sum(-1)[t0], aout)
    return res, mag, mag_abs


def violations(kind, got, ref, mag, kappa=None):
    """bool tensor: elements that miss  |got - ref| <= kappa * mag + 1e-30  (for lse, mag is 1 + |lse64|)."""
    kappa = KAPPA[kind] if kappa is None else kappa
    err = (got.to(torch.float64) - ref).abs()
    return ~(err <= kappa * mag + 1e-30)            # (a NaN misses)


def worst(kind, got, ref, mag):
    """max err / mag over the elements with a magnitude (reporting only)."""
    err = (got.to(torch.float64) - ref).abs()
    live = mag > 0
    return float((err[live] / mag[live]).max()) if bool(live.any()) else 0.0
