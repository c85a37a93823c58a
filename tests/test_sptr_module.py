"""sptr's module surface without a GPU: VarLengthMultiheadSA's state dict, the import paths install_as_sptr() serves, and the
position embedding against the reference's recorded outputs (tests/golden/sptr_pos_embedding.npz, made by
tests/golden/make_sptr_pe_golden.py from the reference's class).

Tolerance of the position embedding: 8 x the deviation of the fp32 evaluation of the formulas from their float64
evaluation (numpy, below) on the fixture's own scenes -- measured 7.96e-7 for 'sine' (arguments up to 2 pi) and 2.90e-6 for
'fourier' (arguments up to ~30: 2 pi u B with |B| up to ~3), so 6.4e-6 and 2.3e-5 absolute on values in [-1, 1].  (The
implementation evaluates the operators in the reference's order and gives the recorded outputs bit for bit on this CPU; the
tolerance is what another libm may move.)"""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sptr_pos_embedding.npz')
DEVIATION = {'sine': 7.96e-7, 'fourier': 2.90e-6}         # measured: test_position_embedding_tolerance_is_eight_times_...
TOL = {k: 8 * v for k, v in DEVIATION.items()}
LINEARS = {f'{m}.{p}': s for m in ('q', 'k', 'v', 'proj') for p, s in (('weight', (32, 32)), ('bias', (32,)))}


def _module(pe_type, **kw):
    from u2mkd_amd import sptr
    extra = dict(rel_query=True, rel_key=True, rel_value=True, quant_size=[0.025] * 3) if pe_type == 'contextual' else {}
    extra.update(kw)
    return sptr.VarLengthMultiheadSA(32, 2, 'key', [0.6, 0.6, 0.6], pe_type=pe_type, **extra)


@pytest.mark.parametrize('pe_type', ['none', 'sine', 'fourier', 'contextual'])
def test_state_dict_keys_and_shapes(pe_type):
    m = _module(pe_type)
    want = dict(LINEARS)
    if pe_type == 'contextual':
        want.update({f'relative_pos_{n}_table': (47, 3, 2, 16) for n in ('query', 'key', 'value')})     # 2 * 24 - 1 rows
    if pe_type == 'fourier':
        want['pos_enc.gauss_B'] = (3, 16)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert {n for n, _ in m.named_parameters()} == set(want) - {'pos_enc.gauss_B'}
    assert m.scale == 16 ** -0.5 and m.shift_win is False and m.indice_key == 'key'
    assert isinstance(m.attn_drop, torch.nn.Dropout) and isinstance(m.proj_drop, torch.nn.Dropout)
    assert all(isinstance(getattr(m, n), torch.nn.Linear) for n in ('q', 'k', 'v', 'proj'))
    if pe_type == 'contextual':
        assert m.quant_grid_length == 24
        t = m.relative_pos_query_table
        assert 0.018 < float(t.detach().std()) < 0.022                      # trunc_normal_(std=.02) with the cut at +-2


def test_constructor_defaults_and_own_errors():
    from u2mkd_amd import sptr
    m = sptr.VarLengthMultiheadSA(64, 4, None, 0.3)
    assert m.pe_type == 'none' and m.shift_win is False and m.q.bias is not None and m.attn_drop.p == 0.0
    assert sptr.VarLengthMultiheadSA(32, 2, 'k', 0.3, qkv_bias=False, qk_scale=0.5).q.bias is None
    assert np.array_equal(m.window_size, np.full(3, 0.3, dtype=np.float32))
    with pytest.raises(ValueError, match='head dim 16'):
        sptr.VarLengthMultiheadSA(64, 2, 'k', 0.3)
    with pytest.raises(ValueError, match='cells per window'):                # 48 cells: beyond the strips and the 50-row tables
        _module('contextual', quant_size=[0.0125] * 3)
    with pytest.raises(NotImplementedError):
        _module('contextual', rel_value=False)


def test_install_as_sptr_serves_the_import_paths_of_the_library():
    import sys
    import u2mkd_amd
    before = {k: v for k, v in sys.modules.items() if k == 'sptr' or k.startswith('sptr.')}
    try:
        drop_in = u2mkd_amd.install_as_sptr()
        from sptr import VarLengthMultiheadSA, SparseTrTensor, sparse_self_attention, get_indices_params, to_3d_numpy  # noqa: F401
        from sptr.modules import VarLengthMultiheadSA as a, sparse_self_attention as b
        from sptr.utils import to_3d_numpy as c, get_indices_params as d
        from sptr.position_embedding import PositionEmbeddingCoordsSine as e
        from third_party.SparseTransformer.sptr.modules import VarLengthMultiheadSA as f
        from third_party.SparseTransformer.sptr.position_embedding import PositionEmbeddingCoordsSine as g
        import third_party.SparseTransformer.sptr.utils  # noqa: F401
        assert a is f is VarLengthMultiheadSA is drop_in.VarLengthMultiheadSA and e is g is drop_in.PositionEmbeddingCoordsSine
        assert b is sparse_self_attention and c is to_3d_numpy and d is get_indices_params
    finally:
        for k in [k for k in sys.modules if k == 'sptr' or k.startswith('sptr.')]:
            del sys.modules[k]
        sys.modules.update(before)


def _float64_embedding(pos_type, d_pos, xyz, gauss_B=None):
    """the formulas in numpy float64: [points, d_pos]"""
    x = xyz.astype(np.float64)
    u = (x - x.min(0)) / (x.max(0) - x.min(0))
    if pos_type == 'fourier':
        z = (2 * np.pi * u) @ gauss_B.astype(np.float64)
        return np.concatenate([np.sin(z), np.cos(z)], 1)
    per_axis = d_pos // 3 - (d_pos // 3) % 2
    spare = d_pos - 3 * per_axis
    blocks = []
    for d in range(3):
        c = per_axis + (2 if spare > 0 else 0)
        spare -= 2 if spare > 0 else 0
        i = np.arange(c)
        phase = (2 * np.pi * u[:, d])[:, None] / 10000.0 ** (2 * (i // 2) / c)
        blocks.append(np.where(i % 2 == 0, np.sin(phase), np.cos(phase)))
    return np.concatenate(blocks, 1)


def _embed(pe, p):
    return pe(p[None], input_range=[p.min(0)[0][None], p.max(0)[0][None]])[0].permute(1, 0)


def _cases():
    return [(t, d, i) for t in ('sine', 'fourier') for d in (32, 48) for i in (0, 1)]


@pytest.mark.parametrize('pos_type,d_pos,scene', _cases())
def test_position_embedding_equals_the_reference_fixture(pos_type, d_pos, scene):
    from u2mkd_amd.sptr.position_embedding import PositionEmbeddingCoordsSine
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 100 * 1024
    pe = PositionEmbeddingCoordsSine(pos_type=pos_type, d_pos=d_pos, normalize=True)
    if pos_type == 'fourier':
        assert tuple(pe.gauss_B.shape) == (3, d_pos // 2)
        pe.load_state_dict({'gauss_B': torch.from_numpy(z[f'fourier_{d_pos}_gauss_B'])})
    p = torch.from_numpy(z[f'xyz{scene}'])
    keep = p.clone()
    got = _embed(pe, p)
    assert torch.equal(p, keep) and not got.requires_grad                      # the caller's points are not scaled in place
    want = z[f'{pos_type}_{d_pos}_scene{scene}']
    assert got.shape == want.shape == (p.shape[0], d_pos)
    assert float(np.abs(got.numpy() - want).max()) <= TOL[pos_type]
    # and the float64 statement of the formulas above says the same as the reference's recording
    f64 = _float64_embedding(pos_type, d_pos, z[f'xyz{scene}'], z[f'fourier_{d_pos}_gauss_B'] if pos_type == 'fourier' else None)
    assert float(np.abs(want - f64).max()) <= TOL[pos_type]


def test_position_embedding_tolerance_is_eight_times_the_fp32_deviation_from_float64():
    from u2mkd_amd.sptr.position_embedding import PositionEmbeddingCoordsSine
    z = np.load(GOLDEN)
    dev = {'sine': 0.0, 'fourier': 0.0}
    for pos_type, d_pos, scene in _cases():
        pe = PositionEmbeddingCoordsSine(pos_type=pos_type, d_pos=d_pos, normalize=True)
        B = z[f'fourier_{d_pos}_gauss_B'] if pos_type == 'fourier' else None
        if B is not None:
            pe.gauss_B.copy_(torch.from_numpy(B))
        got = _embed(pe, torch.from_numpy(z[f'xyz{scene}'])).numpy()
        dev[pos_type] = max(dev[pos_type], float(np.abs(got - _float64_embedding(pos_type, d_pos, z[f'xyz{scene}'], B)).max()))
    print(dev)
    for k in dev:
        assert DEVIATION[k] / 2 <= dev[k] <= DEVIATION[k] * 2, (k, dev[k])
        assert TOL[k] == 8 * DEVIATION[k]
