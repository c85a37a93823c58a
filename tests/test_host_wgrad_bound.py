"""The bound of tests/wgrad_f64_ref.py on the CPU, on the inputs of tests/test_gpu_conv_wgrad_f64.py: the honest evaluations
(plain fp32 in two summation orders, the six-product bf16x3 form) pass it, and each degraded evaluation -- a lost partial
product, an operand rounded to bf16, a skipped pair, pair columns not swapped -- fails it where the GPU test looks: on the
``rows`` spread, and on ``unit`` data in the offsets of at most 64 pairs.  (No detection is asked for on ``unit`` data in large
offsets: a lost m * m product is below the fp32 accumulation of 9000 randn terms, see the helper's docstring.)

Measured here, largest error / bound over the two shapes (64 x 64, 20 x 12) and the patterns ragged, ragged8-swap, heavy
(1 or less passes):

    evaluation                           rows spread          unit spread, offsets of 1..64 pairs
    honest fp32, slab order              0.25 .. 0.34         (all three spreads, every offset)
    honest bf16x3, six products          0.28 .. 0.57         (all three spreads, every offset; error / mag up to 2^-20.0)
    x3 without m*m                       37 .. 78             41 .. 77       (error / mag 2^-15.0 .. 2^-14.1)
    x3 without m*m and l*h               53 .. 108            73 .. 105      (2^-14.2 .. 2^-13.7)
    one operand rounded to bf16          3.4e3 .. 5.3e3       3.4e3 .. 5.3e3 (2^-8.7 .. 2^-8.0)
    last pair of every offset skipped    1.0e6 .. 1.4e6       1.4e6          (a whole term: error / mag 1)
    pair columns not swapped             1.7e8 and more       3.1e9 .. 3.9e9 (ragged8-swap only: elsewhere swap = 0)
"""
import functools

import pytest
import torch

import wgrad_f64_ref as R

SHAPES = [(64, 64), (20, 12)]
PATTERNS = ['ragged', 'ragged8-swap', 'heavy']


@functools.lru_cache(maxsize=None)
def _case(pattern, ca, cb, spread):
    c = R.make_case(pattern, ca, cb, spread)
    args = (c['a'], c['b'], c['pairs'], c['counts'], c['swap'])
    dw, mag = R.wgrad_f64(*args)
    r = R.rel_err(R.honest_fp32(*args), dw, mag)
    return c, args, dw, mag, r


def test_the_split_is_exact_and_its_planes_are_as_small_as_T_assumes():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(200000, generator=g) * torch.pow(10.0, torch.randint(-25, 26, (200000,), generator=g).float())
    x[:64] = torch.tensor([1.0 + 2.0 ** -7 - 2.0 ** -23, -(2.0 - 2.0 ** -23), 1.0 + 2.0 ** -23, 2.0 ** -110 * (2.0 - 2.0 ** -23)] * 16)     # the worst planes; the smallest binade
    h, m, l = R.split3(x)
    assert torch.equal(h.double() + m.double() + l.double(), x.double())
    for p in (h, m, l):         # each plane is a bf16: the low 16 bits of its fp32 image are clear
        assert int((p.view(torch.int32) & 0xffff).abs().max()) == 0
    assert bool((m.abs() < 2.0 ** -7 * x.abs()).all()) and bool((l.abs() < 2.0 ** -15 * x.abs()).all())
    assert bool((h * x >= 0).all()) and bool((m * x >= 0).all()) and bool((l * x >= 0).all())     # the planes carry the sign of x
    # and the three dropped products stay below T_X3 |a||b| (checked on the values with the worst planes too)
    a, b = x[:1000].double(), x.flip(0)[:1000].double()
    pa, pb = [p[:1000].double() for p in (h, m, l)], [p[:1000].double() for p in R.split3(x.flip(0))]
    dropped = pa[1] * pb[2] + pa[2] * pb[1] + pa[2] * pb[2]
    assert bool((dropped.abs() <= R.T_X3 * (a * b).abs()).all())
    assert bool((dropped * a * b >= 0).all())


@pytest.mark.parametrize('ca,cb', SHAPES)
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('spread', R.SPREADS)
def test_honest_evaluations_pass_the_bound(pattern, ca, cb, spread):
    c, args, dw, mag, r = _case(pattern, ca, cb, spread)
    ok, over, rel = R.check(R.honest_fp32(*args), dw, mag, R.T_EXACT, r)
    assert ok, (over, rel)      # (by construction: r is this evaluation's own error)
    # another honest order (chunks of 128 pairs, slabs added 16 lanes wide, as the kernels do): what the factor 4 is for
    ok, over, rel = R.check(R.slab_order_fp32(*args), dw, mag, R.T_EXACT, r)
    print('slab order: err / bound %.3f, err / mag 2^%.1f' % (over, torch.tensor(max(rel, 1e-300)).log2()))
    assert ok, (over, rel)
    ok, over, rel = R.check(R.x3_eval(*args), dw, mag, R.T_X3, r)
    print('bf16x3: err / bound %.3f, err / mag 2^%.1f' % (over, torch.tensor(max(rel, 1e-300)).log2()))
    assert ok, (over, rel)


# ('pair columns not swapped' is the honest evaluation where the pattern does not swap)
_DEGRADED_CASES = [(p, n) for p in PATTERNS for n in sorted(R.DEGRADED) if R.PATTERNS[p][2] or n != 'pair columns not swapped']


@pytest.mark.parametrize('ca,cb', SHAPES)
@pytest.mark.parametrize('pattern,name', _DEGRADED_CASES)
def test_degraded_evaluations_fail_the_bound(pattern, ca, cb, name):
    """Judged against the WIDER of the two bounds (T_X3): what fails it fails T = 0 as well."""
    for spread in ('rows', 'unit'):
        c, args, dw, mag, r = _case(pattern, ca, cb, spread)
        got = R.DEGRADED[name](*args)
        if spread == 'unit':      # only the offsets of 1 .. 64 pairs count
            small = torch.tensor([0 < n <= 64 for n in c['counts']])
            assert bool(small.any())
            got, dw, mag, r = got[small], dw[small], mag[small], r[small]
        ok, over, rel = R.check(got, dw, mag, R.T_X3, r)
        print('%s, %s: err / bound %.1f, err / mag 2^%.1f' % (name, spread, over, torch.tensor(rel).log2()))
        assert not ok and over > 1.0, (spread, over, rel)
