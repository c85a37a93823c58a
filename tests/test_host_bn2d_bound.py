"""The camera BatchNorm2d without a GPU: the float64 bound of tests/bn2d_f64_ref.py rejects every wrong formulation on a named
case of the GPU test and admits the honest fp32 evaluation in the kernels' order (``piece_chan_fp32``) on every input set
tests/test_gpu_bn2d_f64.py runs, with at most 1 % of a case's elements undecided; the helper's restatement of the kernels' shape
agrees with csrc/bn2d.hip, and the shape list reaches every boundary of that shape."""
import os
import re

import pytest
import torch

import bn2d_f64_ref as R2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the wrong formulation -> (shape, kind, mode) of a case of the GPU test, the outputs that have to be outside the bound there
REJECTED_ON = {
    # mean 1e3, spread 1: E[x^2] is 1e6 with an fp32 error near 0.1, the variance is 1
    'variance as E[x^2] - mean^2': (((2, 4, 64, 128), 'mean1e3', 'plain'), ('invstd', 'running_var', 'y', 'dx')),
    # 270 369 values of mean 1e3: the accumulator passes 2^24, where its spacing is 2, and ends at 2.7e8, where it is 16 or 32
    'one fp32 accumulator per channel': (((33, 4, 3, 2731), 'mean1e3', 'plain'), ('mean', 'y')),
    # a piece of 8192 and a piece of ONE element per plane, that element 8 spreads off
    'pieces merged with equal weights': (((2, 4, 3, 2731), 'first8', 'plain'), ('mean', 'y', 'dx')),
    'every piece counted as 8192 elements': (((2, 4, 3, 2731), 'first8', 'plain'), ('mean', 'invstd', 'y', 'dx')),
    # 66 pieces: the last image's two never arrive
    'pieces beyond the 64th dropped': (((33, 4, 3, 2731), 'randn', 'plain'), ('mean', 'y')),
    'inv_n = 1 / hw': (((2, 4, 7, 9), 'randn', 'plain'), ('dx',)),
    'parameter gradients from the unmasked dy': (((3, 8, 32, 32), 'randn', 'relu'), ('dgamma', 'dbeta', 'dx')),
}


# ------------------------------------------------------------------ the bound can fail
@pytest.mark.parametrize('name', list(R2.WRONG))
def test_bound_rejects_the_wrong_formulation_on_its_named_case(name):
    (shape, kind, mode), outputs = REJECTED_ON[name]
    assert shape in R2.SHAPES and (kind, mode, True) in R2.cases(shape)
    case = R2.make_case(shape, kind)
    ref, bound, und, share = R2.evaluate64(case, mode)
    assert share <= R2.UNDECIDED_CAP
    wrong = R2.check(R2.WRONG[name](case, mode), ref, bound, und)
    honest = R2.check(R2.piece_chan_fp32(case, mode), ref, bound, und)
    print('\n%s\n  wrong : %s\n  honest: %s' % (name, {k: '%.3g' % v[1] for k, v in wrong.items()},
                                                 {k: '%.3g' % v[1] for k, v in honest.items()}))
    assert all(v[0] for v in honest.values()), honest
    assert not any(wrong[k][0] for k in outputs), wrong
    if name in ('inv_n = 1 / hw', 'parameter gradients from the unmasked dy'):
        assert wrong['y'][0] and wrong['mean'][0] and wrong['invstd'][0]          # the forward pass of these two is the honest one


def test_every_wrong_formulation_has_a_named_case():
    assert sorted(REJECTED_ON) == sorted(R2.WRONG) and len(R2.WRONG) >= 7


def test_the_bound_needs_the_term_of_the_shift():
    """``first8``, one piece per plane: with q_b taken as if the sums carried M2_b alone (the row file's form), the honest fp32
    evaluation of the shifted sums is OUTSIDE the bound of invstd, y and dx -- the error of M2_b is u n_b (m_b - shift)^2, 64
    times M2_b here -- and inside with the term; on ``randn`` it is inside both"""
    shape = (2, 4, 64, 64)
    for kind, inside_without in (('first8', False), ('randn', True)):
        case = R2.make_case(shape, kind)
        got = R2.piece_chan_fp32(case, 'plain')
        for shift_terms in (True, False):
            ref, bound, und, _ = R2.evaluate64(case, 'plain', se=R2.stat_errors(case['x'], shift_terms=shift_terms))
            out = R2.check(got, ref, bound, und)
            print(kind, shift_terms, {k: '%.3g' % v[1] for k, v in out.items()})
            assert all(out[k][0] for k in ('invstd', 'y', 'dx')) == (shift_terms or inside_without), (kind, shift_terms, out)
            if not shift_terms and not inside_without:
                assert not any(out[k][0] for k in ('invstd', 'y', 'dx')), out


# ------------------------------------------------------------------ the GPU test is satisfiable
@pytest.mark.parametrize('shape', R2.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_piece_chan_fp32_is_inside_the_bound_on_every_input_set_of_the_gpu_test(shape):
    top, top_share, failed, se = {}, 0.0, [], {}
    for kind, mode, affine in R2.cases(shape):
        case = R2.make_case(shape, kind, affine=affine)
        if kind not in se:
            se[kind] = R2.stat_errors(case['x'])
        for training in (True, False):
            ref, bound, und, share = R2.evaluate64(case, mode, training=training, se=se[kind] if training else None)
            top_share = max(top_share, share)
            assert share <= R2.UNDECIDED_CAP, (kind, mode, affine, training, share)
            got = R2.piece_chan_fp32(case, mode, training)
            names = [k for k in R2.OUTPUTS if k in ref and (training or k not in ('mean',))]
            for name, (ok, over, _) in R2.check(got, ref, bound, und, names).items():
                top[name] = max(top.get(name, 0.0), over)
                if not ok:
                    failed.append((kind, mode, affine, training, name, over))
    print('\n%s: largest error / bound of the honest fp32 evaluation: %s; largest undecided share %.5f'
          % (shape, '  '.join('%s %.3f' % kv for kv in top.items()), top_share))
    assert not failed, failed


# ------------------------------------------------------------------ the kernels' shape
def test_shape_functions_agree_with_the_constants_of_bn2d_hip():
    src = open(os.path.join(ROOT, 'u2mkd_amd', 'csrc', 'bn2d.hip')).read()
    k = {name: int(v) for name, v in re.findall(r'constexpr int (kB2\w+) = (\d+);', src)}
    assert (k['kB2Threads'], k['kB2Chunk'], k['kB2ApplyChunk']) == (R2.THREADS, R2.CHUNK, R2.APPLY_CHUNK)
    # what the restated forms rest on, as the file states it
    assert src.count('if ((hw & 3) == 0) {') == 4                                   # the float4 form's condition, in the 4 map kernels
    assert src.count('e += kB2Threads * 4') == 4 and src.count('e += kB2Threads)') == 4
    assert 's1 += (d0 + d1) + (d2 + d3);' in src and 'const float shift = p[0];' in src
    assert src.count('for (int i = lane; i < np; i += 64)') == 2 and src.count('for (int off = 32; off >= 1; off >>= 1)') == 3
    assert 'const float nb = (float)min(kB2Chunk, hw - s * kB2Chunk);' in src and 'const int s = i % splits;' in src
    shapes = [(b, c, hw) for b in (1, 2, 33) for c in (1, 4, 130) for hw in (1, 2, 63, 4096, 4097, 8192, 8193, 8196, 106596)]
    for b, c, hw in shapes:
        assert R2.workspace_bytes(b, c, hw) == c * b * ((hw + k['kB2Chunk'] - 1) // k['kB2Chunk']) * 8
    try:
        from u2mkd_amd import _lib
        lib = _lib.load()
    except (OSError, RuntimeError):
        lib = None                                       # (no library on this machine: the source text has been compared)
    if lib is not None:
        for b, c, hw in shapes + [(0, 4, 8), (2, 0, 8), (2, 4, 0)]:
            assert lib.u2mkd_bn2d_workspace_bytes(b, c, hw) == R2.workspace_bytes(b, c, hw), (b, c, hw)
    # the depths: a full float4 piece, a full scalar one, both forms of the gradient kernel, the smallest pieces
    assert R2.piece_depth(8192, 8192) == 2 + 7 + 6 + 3 and R2.piece_depth(8192, 8193) == 31 + 6 + 3
    assert R2.bwd_piece_depth(8192, 8192) == R2.bwd_piece_depth(8192, 8193) == 31 + 6 + 3
    assert R2.piece_depth(1, 8193) == 0 and R2.piece_depth(2, 2) == 1 and R2.piece_depth(4, 8196) == 2
    assert R2.piece_depth(63, 63) == 6 and R2.piece_depth(144, 144) == 2 + 6 and R2.piece_depth(1024, 1024) == 2 + 6 + 3
    assert [R2.merge_depth(n) for n in (1, 2, 64, 65, 66, 70, 174)] == [0, 1, 6, 7, 7, 7, 8]


def test_the_shape_list_reaches_every_boundary_of_the_kernels():
    S = [(b, c, h * w) for b, c, h, w in R2.SHAPES]
    assert len(set(R2.SHAPES)) == len(R2.SHAPES) == 13 and max(b * c * hw for b, c, hw in S) < 2.2e6

    def some(cond):
        return any(cond(b, c, hw) for b, c, hw in S)
    last = lambda hw, chunk=R2.CHUNK: R2.piece_counts(hw, chunk)[-1]               # noqa: E731
    f4 = R2.float4_form
    # the second trip of the finalize kernels' loop, in both forms; piece counts that alternate inside it
    assert some(lambda b, c, hw: R2.num_pieces(b, hw) > 64 and f4(hw) and last(hw) != R2.CHUNK)
    assert some(lambda b, c, hw: R2.num_pieces(b, hw) > 64 and not f4(hw) and last(hw) == 1)
    # last pieces of one element and of one float4; one piece only
    assert some(lambda b, c, hw: not f4(hw) and R2.splits(hw) == 2 and last(hw) == 1)
    assert some(lambda b, c, hw: f4(hw) and R2.splits(hw) == 2 and last(hw) == 4)
    # a last apply chunk of one element; exactly full chunks of both kinds; more than two apply chunks
    assert some(lambda b, c, hw: R2.splits(hw, R2.APPLY_CHUNK) == 2 and last(hw, R2.APPLY_CHUNK) == 1)
    assert some(lambda b, c, hw: hw == R2.APPLY_CHUNK) and some(lambda b, c, hw: hw == R2.CHUNK)
    assert some(lambda b, c, hw: f4(hw) and R2.splits(hw, R2.APPLY_CHUNK) > 2 and last(hw, R2.APPLY_CHUNK) % (4 * R2.THREADS))
    # fewer elements than threads in both forms, exactly one float4 per thread, the smallest training case
    assert some(lambda b, c, hw: not f4(hw) and hw < R2.THREADS) and some(lambda b, c, hw: f4(hw) and hw // 4 < R2.THREADS)
    assert some(lambda b, c, hw: hw == 4 * R2.THREADS) and some(lambda b, c, hw: b * hw == 2)
    # the channel counts
    assert some(lambda b, c, hw: c == 1) and some(lambda b, c, hw: c > 128 and c & (c - 1))
    assert R2.AFFINE_FALSE_SHAPE in R2.SHAPES
