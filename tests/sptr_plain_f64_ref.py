"""float64 reference of the TABLE-FREE window attention (csrc/sptr_plain.hip) on a synthetic plan (test helper).

The statement of tests/sptr_f64_ref.py with the relative-position terms absent, on that file's cubic ``Case`` (its plan --
``sort_idx``, ``wstart``, ``wlen`` and the pair lists -- and its q, k, v, dout; the case's tables and quantised coordinates
are not read):

    s_ij   = (q_scale q_i) . k_j                       over the pairs (i, j) of a window
    lse_i  = log sum_j exp(s_ij),  p_ij = exp(s_ij - lse_i),  out_i = sum_j p_ij v_j
    delta_i = dout_i . out_i,  dp_ij = dout_i . v_j,  ds_ij = p_ij (dp_ij - delta_i)
    dq_i = q_scale sum_j ds_ij k_j,   dk_j = sum_i ds_ij q_scale q_i,   dv_j = sum_i p_ij dout_i

by explicit index sums (no autograd), in the dtype asked for, and with each result the two MAGNITUDE SUMS of
tests/sptr_f64_ref.py: the same sum with every factor replaced by its absolute value and ds by p (|dp| + |delta|)
(``mag``), and with every TERM by its absolute value (``mag_abs``: dp by sum_d |dout_d| |v_d|, delta by
sum_d |dout_d| sum_j p_ij |v_jd|).  Without tables the two differ in dp and delta only, i.e. for dq and dk.

The gate of tests/test_gpu_sptr_plain.py is that file's, elementwise, twice:

    |kernel - float64| <= KAPPA[kind]     * mag     + 1e-30
    |kernel - float64| <= KAPPA_ABS[kind] * mag_abs + 1e-30
    (lse: both magnitudes are 1 + |lse64|)

and the coefficients come from the same rule, re-measured for THIS formulation and never from a kernel:
tests/test_sptr_plain_f64_reference.py evaluates this module in fp32 on the CPU on every case of the GPU file (the five
splits x q_scale 0.25 and 1), takes rho[kind] = max(err / magnitude) against float64 and requires KAPPA[kind] = 8 * rho
rounded up to a power of two (8: __expf, the online softmax and another summation order).  Measured (torch 2.x CPU; the
test pins the recorded figure within a factor of two and the power of two exactly):

    kind   rho       KAPPA    rho_abs   KAPPA_ABS
    out    3.38e-6   2^-15    3.38e-6   2^-15
    lse    5.50e-7   2^-17    (the same: relative to 1 + |lse64|)
    dq     2.89e-5   2^-12    9.96e-7   2^-16
    dk     1.14e-5   2^-13    9.17e-7   2^-17
    dv     2.41e-6   2^-15    2.41e-6   2^-15

(dq and dk against ``mag``: dp = dout . v cancels in a few elements, which sets the maximum; ``mag_abs`` holds them tightly.)
"""
import numpy as np
import torch

import sptr_f64_ref as R

KINDS = ('out', 'lse', 'dq', 'dk', 'dv')
Q_SCALES = (0.25, 1.0)

# measured by tests/test_sptr_plain_f64_reference.py::test_kappa_is_eight_rho_of_the_fp32_evaluation over gpu_cases()
RHO = {'out': 3.38e-6, 'lse': 5.50e-7, 'dq': 2.89e-5, 'dk': 1.14e-5, 'dv': 2.41e-6}
RHO_ABS = {'out': 3.38e-6, 'lse': 5.50e-7, 'dq': 9.96e-7, 'dk': 9.17e-7, 'dv': 2.41e-6}
KAPPA = {k: R.pow2_ceil(8 * r) for k, r in RHO.items()}
KAPPA_ABS = {k: R.pow2_ceil(8 * r) for k, r in RHO_ABS.items()}


def gpu_cases():
    """(S, h, q_scale) of the cases of tests/test_gpu_sptr_plain.py: every split on sptr_f64_ref.window_lengths(S, big=False)
    with two heads (three at S = 4), the query scale inside the kernel at 0.25 and at 1."""
    return [(S, 3 if S == 4 else 2, qs) for S in R.SPLITS for qs in Q_SCALES]


def case_id(c):
    return 'S%d-h%d-scale%g' % c


def get_case(S, h):
    return R.get_case(S, False, h, False)


def reference(case, q_scale, dtype=torch.float64, device='cpu', i0=None, i1=None, magnitudes=True):
    """{kind: tensor} and, with ``magnitudes``, the two {kind: magnitude sum}.  ``i0, i1`` override the case's pair list (sorted
    positions of the query and the key of every pair: the corruptions of test_sptr_plain_f64_reference.py)."""
    dev = torch.device(device)
    t = lambda x: x.to(device=dev, dtype=dtype)
    ix = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.int64, device=dev)
    q, k, v, dout = (t(x) for x in (case.q, case.k, case.v, case.dout))
    i0 = ix(case.i0 if i0 is None else i0)
    i1 = ix(case.i1 if i1 is None else i1)
    sort_idx = ix(case.sort_idx)
    n, h, _ = q.shape
    qs = q_scale
    t0, t1 = sort_idx[i0], sort_idx[i1]
    qi, kj, vj, do = (q * qs)[t0], k[t1], v[t1], dout[t0]
    s = (qi * kj).sum(-1)                                                                 # [M, h]
    m = torch.full((n, h), -float('inf'), dtype=dtype, device=dev)
    m = m.scatter_reduce(0, i0[:, None].expand_as(s), s, reduce='amax')
    lse = m + torch.zeros_like(m).index_add(0, i0, (s - m[i0]).exp()).log()               # per sorted position
    p = (s - lse[i0]).exp()
    P = p[..., None]

    def tok(index, src):
        return torch.zeros_like(q).index_add(0, index, src)

    out = tok(t0, P * vj)
    delta = (dout * out).sum(-1)[t0]
    dp = (do * vj).sum(-1)
    ds = (p * (dp - delta))[..., None]
    res = {'out': out, 'lse': lse, 'dq': qs * tok(t0, ds * kj), 'dk': tok(t1, ds * qi), 'dv': tok(t1, P * do)}
    if not magnitudes:
        return res
    aout = tok(t0, P * vj.abs())

    def mags(adp, adelta):
        ads = (p * (adp + adelta))[..., None]
        return {'out': aout, 'lse': 1 + lse.abs(), 'dq': qs * tok(t0, ads * kj.abs()), 'dk': tok(t1, ads * qi.abs()),
                'dv': tok(t1, P * do.abs())}

    mag = mags(dp.abs(), delta.abs())
    mag_abs = mags((do.abs() * vj.abs()).sum(-1), (dout.abs() * aout).sum(-1)[t0])
    return res, mag, mag_abs


def violations(kind, got, ref, mag, kappa=None):
    return R.violations(kind, got, ref, mag, KAPPA[kind] if kappa is None else kappa)


worst = R.worst
