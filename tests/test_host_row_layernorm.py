"""The row LayerNorm without a GPU: the float64 bound of tests/row_ln_f64_ref.py rejects the wrong formulations and admits the
straightforward fp32 one on every input set tests/test_gpu_row_layernorm.py runs, and RowLayerNorm away from the device is
nn.LayerNorm."""
import os
import subprocess
import sys

import pytest
import torch
from torch import nn

import row_ln_f64_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the bound can fail
@pytest.mark.parametrize('c', R.CS)
def test_bound_rejects_the_variance_as_e_x2_minus_mean2(c):
    """fp32 rows of mean 1e3 and spread 1: E[x^2] is 1e6 with an fp32 error near 0.1, the variance is 1"""
    case = R.make_case(64, c, 'mean1e3', torch.float32)
    f = R.forward64(case['x'], case['gamma'], case['beta'])
    bound = R.forward_bound(case['x'], case['gamma'], case['beta'], torch.float32, f=f)
    ok, over, _ = R.worst(R.WRONG['variance as E[x^2] - mean^2'](case['x'], case['gamma'], case['beta'], torch.float32), f['y'], bound)
    assert not ok, over
    ok, over, _ = R.worst(R.two_pass_fp32(case['x'], case['gamma'], case['beta'], torch.float32), f['y'], bound)
    assert ok, over


@pytest.mark.parametrize('kind', ['randn', 'mean1e3'])
@pytest.mark.parametrize('c', [256, 512, 1024])
def test_bound_rejects_statistics_accumulated_in_bf16(c, kind):
    """bf16 rows: a bf16 accumulator stops taking terms of size 1 once it holds 256 (its spacing there is 2)"""
    dt = torch.bfloat16
    case = R.make_case(64, c, kind, dt)
    f = R.forward64(case['x'], case['gamma'], case['beta'])
    bound = R.forward_bound(case['x'], case['gamma'], case['beta'], dt, f=f)
    ok, over, _ = R.worst(R.WRONG['statistics accumulated in bf16'](case['x'], case['gamma'], case['beta'], dt), f['y'], bound)
    assert not ok, over
    ok, over, _ = R.worst(R.two_pass_fp32(case['x'], case['gamma'], case['beta'], dt), f['y'], bound)
    assert ok, over


@pytest.mark.parametrize('with_w', [False, True], ids=['plain', 'row_scale'])
@pytest.mark.parametrize('c', [64, 256])
def test_add_form_with_statistics_of_the_unrounded_sum_is_not_the_plain_form_on_the_stored_stream(c, with_w):
    """the add form's property is equality with the plain form applied to the STORED stream row; statistics taken from the fp32
    sum before its bf16 rounding give another y"""
    dt = torch.bfloat16
    case = R.make_case(257, c, 'randn', dt)
    w = case['w'] if with_w else None
    s, y_wrong = R.add_form_unrounded_stats(case['a'], case['b'], w, case['gamma'], case['beta'], dt)
    assert torch.equal(s, R.stream64(case['a'], case['b'], w, dt))
    y_plain = R.two_pass_fp32(s, case['gamma'], case['beta'], dt)
    assert not torch.equal(y_wrong, y_plain)
    assert int((y_wrong != y_plain).sum()) > y_plain.numel() // 100


# ------------------------------------------------------------------ the GPU test is satisfiable
@pytest.mark.parametrize('tag', list(R.DTYPES))
@pytest.mark.parametrize('c', R.CS)
def test_two_pass_fp32_is_inside_the_bound_on_every_input_set_of_the_gpu_test(c, tag):
    dt = R.DTYPES[tag]
    worst = {}
    for n in R.NS:
        for kind in R.KINDS:
            case = R.make_case(n, c, kind, dt)
            x, gm, bt = case['x'], case['gamma'], case['beta']
            f = R.forward64(x, gm, bt)
            ok, over, _ = R.worst(R.two_pass_fp32(x, gm, bt, dt), f['y'], R.forward_bound(x, gm, bt, dt, f=f))
            worst[(n, kind, 'y')] = over
            assert ok, (n, kind, 'y', over)
            for ds, w in ((None, None), (case['ds'], case['w'])):
                b = R.backward64(case['dy'], x, gm, ds=ds, w=w)
                bd = R.backward_bound(case['dy'], x, gm, dt, ds=ds, w=w, b=b)
                got = R.two_pass_backward_fp32(case['dy'], x, gm, dt, ds=ds, w=w)
                for name in bd:
                    ok, over, _ = R.worst(got[name], b[name], bd[name])
                    worst[(n, kind, name)] = max(over, worst.get((n, kind, name), 0.0))
                    assert ok, (n, kind, name, over)
    print('\nc=%d %s: largest error / bound of the fp32 two-pass evaluation: %.3f' % (c, tag, max(worst.values())))


def test_lane_forms_cover_every_supported_width():
    for c in range(8, 1100, 4):
        if not R.supported(c):
            continue
        g, v = R.lane_form(c)
        assert g in (8, 16, 32, 64) and v in (1, 2) and g * v * 8 >= c and (g == 8 or (g // 2) * v * 8 < c or v == 2)


# ------------------------------------------------------------------ host behaviour
def _pair(c, **kw):
    from u2mkd_amd.lidar.blocks import RowLayerNorm
    torch.manual_seed(c)
    ours, ref = RowLayerNorm(c, **kw), nn.LayerNorm(c, **kw)
    if ours.weight is not None:
        with torch.no_grad():
            ours.weight.normal_(1.0, 0.5)
            ours.bias.normal_()
        ref.load_state_dict(ours.state_dict())
    return ours, ref


@pytest.mark.parametrize('c,kw', [(64, {}), (36, {}), (64, {'elementwise_affine': False}), (40, {'eps': 1e-3})])
def test_row_layernorm_on_cpu_tensors_is_nn_layernorm_bit_for_bit(c, kw):
    ours, ref = _pair(c, **kw)
    x = torch.randn(19, c)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = ours(xa), ref(xb)
    assert torch.equal(ya, yb)
    g = torch.randn_like(ya)
    ya.backward(g)
    yb.backward(g)
    assert torch.equal(xa.grad, xb.grad)
    for p, q in zip(ours.parameters(), ref.parameters()):
        assert torch.equal(p.grad, q.grad)


@pytest.mark.parametrize('scaled', [False, True])
def test_add_norm_on_cpu_tensors_is_the_sum_followed_by_nn_layernorm(scaled):
    ours, ref = _pair(64)
    a, b = torch.randn(19, 64, requires_grad=True), torch.randn(19, 64, requires_grad=True)
    w = ((torch.rand(19, 1) < 0.7).float() / 0.7) if scaled else None
    stream, normed = ours.add_norm(a, b, w)
    want = torch.addcmul(a, b, w) if scaled else a + b
    assert torch.equal(stream, want) and torch.equal(normed, ref(want))
    (stream.sum() + (normed * normed).sum()).backward()
    assert a.grad is not None and b.grad is not None and ours.weight.grad is not None


def test_row_layernorm_keeps_the_state_dict_keys_and_the_class_of_nn_layernorm():
    from u2mkd_amd.lidar.sphereformer import SphereFormer
    ours, ref = _pair(64)
    assert isinstance(ours, nn.LayerNorm)
    assert list(ours.state_dict()) == list(ref.state_dict()) == ['weight', 'bias']
    import numpy as np
    w = np.array([0.3, 0.3, 0.3], dtype=np.float32)
    ws = np.array([2.0, 2.0, 120.0])
    block = SphereFormer(64, 4, w, ws, w / 24, ws / 24)
    assert isinstance(block.norm1, nn.LayerNorm) and isinstance(block.norm2, nn.LayerNorm)
    keys = set(block.state_dict())
    assert {'norm1.weight', 'norm1.bias', 'norm2.weight', 'norm2.bias'} <= keys
    assert not any(k.startswith('norm') and k.split('.')[1] not in ('weight', 'bias') for k in keys)
    # a checkpoint of plain nn.LayerNorm modules loads unchanged
    block.norm1.load_state_dict(ref.state_dict())
    assert torch.equal(block.norm1.weight, ref.weight)


def test_supported_widths_and_torchs_route_for_the_others(monkeypatch):
    from u2mkd_amd.torchsparse.nn import functional as spf
    for c in range(1, 1100):
        assert spf._ln_supported(c) == R.supported(c), c
    assert all(R.supported(c) for c in (32, 64, 128, 256, 512) + R.CS) and not R.supported(36)
    # whatever _ln_rows refuses goes to F.layer_norm with nn.LayerNorm's own arguments
    seen = []
    real = torch.nn.functional.layer_norm
    monkeypatch.setattr(torch.nn.functional, 'layer_norm', lambda *a, **k: (seen.append(a[1]), real(*a, **k))[1])
    ours, _ = _pair(36)
    ours(torch.randn(5, 36))
    assert seen == [(36,)]
    assert spf._ln_rows(torch.randn(5, 64), (64,), ours.weight, ours.bias) is None      # a CPU tensor


def test_switch_u2mkd_row_ln_is_read_at_import():
    code = ('from u2mkd_amd.torchsparse.nn import functional as spf; import torch; '
            'print(sorted((str(k), v) for k, v in spf._ROW_LN_ON.items()))')
    out = {}
    for val in ('0', '1'):
        env = dict(os.environ, U2MKD_ROW_LN=val)
        out[val] = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout
    assert out['0'].count('False') == 3 and 'True' not in out['0'], out['0']
    assert out['1'].count('True') == 3 and 'False' not in out['1'], out['1']
