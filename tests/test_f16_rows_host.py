"""FP16 storage, the parts that need no GPU: the arith-5 fragment size, the nine _f16 entries next to their _bf16 twins and
the row-dtype helper that routes the sparse operators under autocast."""
import os
import subprocess
import sys

import torch

from u2mkd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F16_ENTRIES = ['u2mkd_conv_forward_tiles', 'u2mkd_conv_wgrad_pairs', 'u2mkd_conv_forward_pairs', 'u2mkd_linear_forward',
               'u2mkd_pairs_gather_sum', 'u2mkd_voxelize_backward', 'u2mkd_devoxelize_forward', 'u2mkd_segment_sum',
               'u2mkd_segment_mean']


def test_arith_5_fragments_have_the_size_of_arith_3():
    lib = _lib.load()
    for k, r, c in ((27, 64, 64), (1, 32, 256), (8, 96, 128)):
        n3, n5 = lib.u2mkd_weight_fragments_bytes(k, r, c, 3), lib.u2mkd_weight_fragments_bytes(k, r, c, 5)
        assert n5 == n3 == k * r * c * 2 > 0          # one 2-byte plane, no scale trailer


def test_every_bf16_entry_has_an_f16_twin_with_the_same_arguments():
    lib = _lib.load()
    twins = sorted(n[:-len('_bf16')] for n in _lib.SIGNATURES if n.endswith('_bf16'))
    assert twins == sorted(F16_ENTRIES)
    for base in F16_ENTRIES:
        assert base + '_f16' in _lib.SIGNATURES, base
        assert _lib.SIGNATURES[base + '_f16'] == _lib.SIGNATURES[base + '_bf16'], base
        assert hasattr(lib, base + '_f16'), base


class _autocast_state:
    """torch's 'cuda' autocast state set directly: ``torch.autocast('cuda')`` switches itself off on a machine without a GPU,
    the thread-local state it would set -- all that the helper reads -- can be written anywhere."""

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.was = (torch.is_autocast_enabled('cuda'), torch.get_autocast_dtype('cuda'))
        torch.set_autocast_enabled('cuda', True)
        torch.set_autocast_dtype('cuda', self.dtype)

    def __exit__(self, *exc):
        torch.set_autocast_enabled('cuda', self.was[0])
        torch.set_autocast_dtype('cuda', self.was[1])
        return False


_STATE = ('class S:\n'
          '    def __init__(s, d): s.d = d\n'
          '    def __enter__(s):\n'
          '        s.w = (torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda"))\n'
          '        torch.set_autocast_enabled("cuda", True); torch.set_autocast_dtype("cuda", s.d)\n'
          '    def __exit__(s, *e):\n'
          '        torch.set_autocast_enabled("cuda", s.w[0]); torch.set_autocast_dtype("cuda", s.w[1])\n')


def test_row_dtype_follows_the_autocast_state():
    from u2mkd_amd.torchsparse.nn import functional as F
    assert F.row_dtype() is None and not F.bf16_rows()
    with _autocast_state(torch.bfloat16):
        assert F.row_dtype() == torch.bfloat16 and F.bf16_rows()
    with _autocast_state(torch.float16):
        assert F.row_dtype() == torch.float16 and not F.bf16_rows()
    assert F.row_dtype() is None


def test_row_dtype_with_the_switch_off():
    """U2MKD_F16_ROWS is read at import: a fresh interpreter"""
    code = ('import sys; sys.path.insert(0, %r)\n'
            'import torch\n'
            'from u2mkd_amd.torchsparse.nn import functional as F\n' + _STATE +
            'with S(torch.float16):\n'
            '    assert F.row_dtype() is None\n'
            'with S(torch.bfloat16):\n'
            '    assert F.row_dtype() == torch.bfloat16\n'
            'assert F.row_dtype() is None\n'
            'print("ok")\n') % ROOT
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, U2MKD_F16_ROWS='0'), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), (r.stdout[-1000:], r.stderr[-2000:])


def test_the_row_movers_keep_bf16_whatever_its_switch_says(monkeypatch):
    """voxelize / devoxelize backward and fusion's segment sums: a bf16 tensor stays bf16 even with U2MKD_BF16_ROWS=0 (as
    before fp16 rows existed); an fp16 tensor stays fp16 unless U2MKD_F16_ROWS=0; anything else is moved as fp32"""
    from u2mkd_amd.torchsparse.nn import functional as F
    for b, h in ((True, True), (False, True), (True, False), (False, False)):
        monkeypatch.setattr(F, '_BF16_ROWS', b)
        monkeypatch.setattr(F, '_F16_ROWS', h)
        assert F._moved16(torch.bfloat16) == torch.bfloat16
        assert F._moved16(torch.float16) == (torch.float16 if h else None)
        assert F._moved16(torch.float32) is None and F._moved16(torch.float64) is None
    t = torch.arange(6.0).reshape(2, 3).t()
    assert F._rows(t, None).dtype == torch.float32 and F._rows(t, None).is_contiguous()
    assert F._rows(t, torch.float16).dtype == torch.float16
    assert F._entry('u2mkd_segment_sum', torch.float32) == 'u2mkd_segment_sum'
    assert F._entry('u2mkd_segment_sum', torch.bfloat16) == 'u2mkd_segment_sum_bf16'
    assert F._entry('u2mkd_segment_sum', torch.float16) == 'u2mkd_segment_sum_f16'
    assert F._entry('u2mkd_segment_mean', torch.float32) == 'u2mkd_segment_mean'
    assert F._entry('u2mkd_segment_mean', torch.bfloat16) == 'u2mkd_segment_mean_bf16'
    assert F._entry('u2mkd_segment_mean', torch.float16) == 'u2mkd_segment_mean_f16'
