"""The row BatchNorm without a GPU: the float64 bound of tests/row_bn_f64_ref.py rejects every wrong formulation on a named case
and admits the honest fp32 evaluation (per-slab mean and centred M2, Chan's update) on every input set
tests/test_gpu_row_bn_f64.py runs, with at most 1 % of a case's elements undecided; the helper's restatement of the kernels'
shape agrees with the library and with the dispatch condition of csrc/bn.hip."""
import os
import re

import pytest
import torch

import row_bn_f64_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rejects(name, case, mode, dt):
    ref, bound, und, share = R.evaluate64(case, mode, dt)
    assert share <= R.UNDECIDED_CAP
    wrong = R.check(R.WRONG[name](case, mode, dt), ref, bound, und)
    honest = R.check(R.slab_chan_fp32(case, mode, dt), ref, bound, und)
    print('\n%s\n  wrong : %s\n  honest: %s' % (name, {k: '%.3g' % v[1] for k, v in wrong.items()},
                                                 {k: '%.3g' % v[1] for k, v in honest.items()}))
    assert all(v[0] for v in honest.values()), honest
    return wrong


# ------------------------------------------------------------------ the bound can fail
def test_bound_rejects_the_variance_as_e_x2_minus_mean2():
    """fp32 rows of mean 1e3 and spread 1: E[x^2] is 1e6 with an fp32 error near 0.1, the variance is 1"""
    wrong = _rejects('variance as E[x^2] - mean^2', R.make_case(8193, 96, 'mean1e3', torch.float32), 'plain', torch.float32)
    assert not wrong['y'][0] and not wrong['invstd'][0] and not wrong['running_var'][0] and not wrong['dx'][0], wrong


def test_bound_rejects_one_fp32_accumulator_per_channel():
    """32769 rows of mean 1e3: the accumulator passes 2^24, where its spacing is 2, and every further row is rounded to it"""
    wrong = _rejects('one fp32 accumulator per channel', R.make_case(32769, 32, 'mean1e3', torch.float32), 'plain', torch.float32)
    assert not wrong['mean'][0] and not wrong['y'][0], wrong


def test_bound_rejects_slab_means_merged_with_equal_weights():
    """129 rows: a slab of 128 and a slab of one row; the first 128 rows shifted by +4 so that the slab means differ"""
    case = R.make_case(129, 48, 'randn', torch.float32)
    case['x'][:128] += 4.0
    wrong = _rejects('slab means merged with equal weights', case, 'plain', torch.float32)
    assert not wrong['mean'][0] and not wrong['y'][0] and not wrong['dx'][0], wrong


def test_bound_rejects_statistics_accumulated_in_the_row_type():
    """bf16 rows: a bf16 accumulator stops taking terms of size 1 once it holds 256 (its spacing there is 2)"""
    wrong = _rejects('statistics accumulated in the row type', R.make_case(8193, 96, 'randn', torch.bfloat16), 'plain', torch.bfloat16)
    assert not wrong['mean'][0] and not wrong['invstd'][0] and not wrong['y'][0] and not wrong['dx'][0], wrong


def test_bound_rejects_parameter_gradients_summed_from_the_unmasked_dy():
    wrong = _rejects('parameter gradients from the unmasked dy', R.make_case(257, 128, 'randn', torch.float32), 'relu', torch.float32)
    assert wrong['y'][0] and not wrong['dgamma'][0] and not wrong['dbeta'][0] and not wrong['dx'][0], wrong


def test_worst_asks_for_equality_where_the_bound_is_zero_and_lets_an_undecided_element_take_either_branch():
    ref, alt = torch.tensor([1.0, 0.0, 2.0], dtype=torch.float64), torch.tensor([1.0, 3.0, 0.0], dtype=torch.float64)
    zero, und = torch.zeros(3, dtype=torch.float64), torch.tensor([False, True, False])
    assert R.worst(ref.float(), ref, zero) == (True, 0.0, 0.0)
    assert not R.worst(torch.tensor([1.0, 1e-30, 2.0]), ref, zero)[0]
    assert R.worst(torch.tensor([1.0, 3.0, 2.0]), ref, zero, alt, zero, und)[0]           # the undecided one took the other branch
    assert not R.worst(torch.tensor([1.0, 0.0, 0.0]), ref, zero, alt, zero, und)[0]       # a decided one may not


# ------------------------------------------------------------------ the GPU test is satisfiable
@pytest.mark.parametrize('tag', list(R.DTYPES))
@pytest.mark.parametrize('n,c', R.PAIRS)
def test_slab_chan_fp32_is_inside_the_bound_on_every_input_set_of_the_gpu_test(n, c, tag):
    dt = R.DTYPES[tag]
    top, top_share, failed = {}, 0.0, []
    for kind, mode, affine in R.cases(n, c):
        case = R.make_case(n, c, kind, dt, affine=affine)
        for training in (True, False):
            ref, bound, und, share = R.evaluate64(case, mode, dt, training=training)
            top_share = max(top_share, share)
            assert share <= R.UNDECIDED_CAP, (kind, mode, affine, training, share)
            got = R.slab_chan_fp32(case, mode, dt) if training else R.eval_fp32(case, mode, dt)
            names = [k for k in R.OUTPUTS if k in ref and (training or k not in ('mean', 'invstd'))]
            for name, (ok, over, _) in R.check(got, ref, bound, und, names).items():
                top[name] = max(top.get(name, 0.0), over)
                if not ok:
                    failed.append((kind, mode, affine, training, name, over))
    print('\nn=%d c=%d %s: largest error / bound of the honest fp32 evaluation: %s; largest undecided share %.5f'
          % (n, c, tag, '  '.join('%s %.3f' % kv for kv in top.items()), top_share))
    assert not failed, failed


# ------------------------------------------------------------------ the kernels' shape
def _constants(src):
    return {k: int(v) for k, v in re.findall(r'constexpr int (kBn\w+) = (\d+)', src)}


def test_shape_functions_agree_with_the_library_and_the_dispatch_of_bn_launch_stats_partial():
    from u2mkd_amd import _lib
    lib = _lib.load()
    for n in (0, 1, 2, 127, 128, 129, 257, 8192, 8193, 32769, 80000, (1 << 31) + 5):
        assert lib.u2mkd_bn_num_slabs(n) == R.num_slabs(n), n
    src = open(os.path.join(ROOT, 'u2mkd_amd', 'csrc', 'bn.hip')).read()
    k = _constants(src)
    assert (k['kBnThreads'], k['kBnSlabRows'], k['kBnRegRows'], k['kBnFinLanes']) == (R.THREADS, R.SLAB_ROWS, R.REG_ROWS, R.FIN_LANES)
    # the dispatch condition, as the file states it, evaluated with C's integer division
    cond = re.search(r'if \((c4 <= \d+ && kBnSlabRows / \(kBnThreads / c4\) <= kBnRegRows) && !bn_stats_serial\(\)\)', src)
    assert cond, 'the dispatch condition of bn_launch_stats_partial has changed: restate it in row_bn_f64_ref.register_form'
    expr = cond.group(1).replace('&&', 'and').replace('/', '//')
    for c in range(4, 1025, 4):
        assert R.supported(c)
        c4 = c // 4
        assert R.register_form(c) == bool(eval(expr, dict(k, c4=c4))), c
        assert R.register_form(c) == (c <= 128), c
        rl = R.row_lanes(c)
        assert rl == max(1, k['kBnThreads'] // c4) and rl * c4 <= k['kBnThreads']
        assert R.thread_rows(c) * rl >= k['kBnSlabRows'] > (R.thread_rows(c) - 1) * rl
        if R.register_form(c):
            assert R.thread_rows(c) <= k['kBnRegRows'] and k['kBnRegRows'] * rl >= k['kBnSlabRows'], c
    assert not R.supported(1028) and not R.supported(6) and not R.supported(0)
    # the widths the GPU test picks: both sides of the register form's limit, dead lanes, more lanes than rows, one lane
    assert R.register_form(128) and not R.register_form(132)
    assert all(256 % (c // 4) for c in (12, 48, 1020)) and R.row_lanes(4) == 256 > R.SLAB_ROWS and R.row_lanes(1024) == 1
    # and the slab counts: one slab, the slab edge, 65 and 257 slabs against the finalize kernel's 64 lanes x 4 loads
    assert [R.num_slabs(n) for n, _ in R.PAIRS] == [1, 1, 1, 1, 2, 2, 3, 3, 65, 65, 257]
    assert R.merge_depth(1) == 0 and R.merge_depth(2) == 1 and R.merge_depth(65) == 7 and R.merge_depth(257) == 10
