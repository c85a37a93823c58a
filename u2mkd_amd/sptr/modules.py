"""``sptr.VarLengthMultiheadSA``: the window self-attention module of SparseTransformer's public surface
(sptr/modules.py:69-199) on the fused HIP kernels -- same constructor, defaults, parameter / buffer names and shapes, so a
state dict of the reference's module loads, and the same forward on a :class:`~u2mkd_amd.sptr.SparseTrTensor`."""
import numpy as np
import torch
from torch import nn

from . import SparseTrTensor, to_3d_numpy
from .functional import get_indices_params, sparse_self_attention
from .position_embedding import PositionEmbeddingCoordsSine

__all__ = ['VarLengthMultiheadSA', 'sparse_self_attention']

_MAX_QGL = 24          # quantisation cells per window the backward's histogram strips hold (csrc/sptr.hip: kNB - 1)


class _Linear(nn.Linear):
    """nn.Linear over token rows [N, C] on the package's HIP linear (same parameters / state-dict keys)."""

    def forward(self, input):
        from ..torchsparse.nn import functional as spf
        return spf.linear(input, self.weight, self.bias)


def _trunc_normal(t, std):
    nn.init.trunc_normal_(t, std=std, a=-2.0, b=2.0)


class VarLengthMultiheadSA(nn.Module):
    def __init__(self, embed_dim, num_heads, indice_key, window_size, shift_win=False, pe_type='none', dropout=0., qk_scale=None,
                 qkv_bias=True, algo='native', **kwargs):
        super().__init__()
        if embed_dim % num_heads or embed_dim // num_heads != 16:
            raise ValueError(f'the window attention kernels run head dim 16; embed_dim={embed_dim} with num_heads={num_heads} '
                             f'gives {embed_dim / num_heads:g}')
        self.embed_dim, self.num_heads, self.indice_key = embed_dim, num_heads, indice_key
        self.shift_win, self.pe_type = shift_win, pe_type
        head_dim = embed_dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.window_size = to_3d_numpy(window_size)
        if pe_type == 'contextual':
            self.rel_query, self.rel_key, self.rel_value = kwargs['rel_query'], kwargs['rel_key'], kwargs['rel_value']
            if not (self.rel_query and self.rel_key and self.rel_value):
                raise NotImplementedError('pe_type="contextual" runs with rel_query = rel_key = rel_value = True only')
            self.quant_size = to_3d_numpy(kwargs['quant_size'])
            cells = [int((self.window_size[d] + 1e-4) / self.quant_size[d]) for d in range(3)]
            if cells[0] != cells[1]:
                raise ValueError(f'window / quant size must give the same grid length on x and y, got {cells[:2]}')
            qgl = cells[0]
            # what csrc/sptr.hip holds: table length 2 * qgl - 1 <= 50 (sptr_check) and at most 24 quantised cells per window
            # on every axis (the histogram strips of the backward)
            if not 1 <= qgl <= _MAX_QGL or max(cells) > _MAX_QGL:
                raise ValueError(f'contextual tables: window / quant size gives {cells} cells per window, the kernels hold 1..{_MAX_QGL} '
                                 f'(table length 2 * {qgl} - 1 <= 47)')
            for name in ('query', 'key', 'value'):
                table = nn.Parameter(torch.zeros(2 * qgl - 1, 3, num_heads, head_dim))
                _trunc_normal(table, .02)
                setattr(self, f'relative_pos_{name}_table', table)
            self.quant_grid_length = qgl
        elif pe_type in ('sine', 'fourier'):
            extra = {'gauss_scale': kwargs.get('gauss_scale', 1.0)} if pe_type == 'fourier' else {}
            self.pos_enc = PositionEmbeddingCoordsSine(pos_type=pe_type, d_pos=embed_dim,
                                                       normalize=kwargs.get('normalize_pos_enc', True), **extra)
        self.q = _Linear(embed_dim, embed_dim, bias=qkv_bias)
        self.k = _Linear(embed_dim, embed_dim, bias=qkv_bias)
        self.v = _Linear(embed_dim, embed_dim, bias=qkv_bias)
        self.attn_drop = nn.Dropout(dropout, inplace=True)        # constructed and never applied, as in the reference
        self.proj = _Linear(embed_dim, embed_dim)
        self.proj_drop = nn.Dropout(dropout, inplace=True)

    def _position_embedding(self, xyz, batch):
        """[N, C]: every scene embedded over its own bounding box (a scene = a run of equal batch index)"""
        sizes = torch.unique_consecutive(batch, return_counts=True)[1].tolist()
        if len(sizes) != int(batch.max()) + 1:
            raise ValueError('the position embedding needs the tokens grouped by scene: batch indices 0, 1, ... in order')
        rows = []
        for scene in torch.split(xyz, sizes):
            box = [scene.amin(0, keepdim=True), scene.amax(0, keepdim=True)]
            rows.append(self.pos_enc(scene.unsqueeze(0), input_range=box)[0].t())
        return torch.cat(rows)

    def _plan(self, sptr_tensor, xyz, batch):
        """The window plan of this tensor under ``indice_key``: built once, kept in ``indice_dict`` in the layout of the
        library's cache entries -- get_indices_params' six results, then the window size and shift the entry was built with."""
        entry = sptr_tensor.find_indice_params(self.indice_key)
        if entry is None:
            entry = get_indices_params(xyz, batch, self.window_size, self.shift_win) + (self.window_size, self.shift_win)
            sptr_tensor.indice_dict[self.indice_key] = entry
        elif not (np.array_equal(entry[6], self.window_size) and entry[7] == self.shift_win):
            raise AssertionError(f'modules that share the same indice_key ({self.indice_key!r}) on a tensor must agree on '
                                 f'window_size and shift_win; the cached entry has {entry[6]}, {entry[7]}')
        return entry

    def forward(self, sptr_tensor: SparseTrTensor):
        query = sptr_tensor.query_feats
        key = query.clone() if sptr_tensor.key_feats is None else sptr_tensor.key_feats
        value = query.clone() if sptr_tensor.value_feats is None else sptr_tensor.value_feats
        indices = sptr_tensor.query_indices
        if indices.dim() != 2 or indices.shape[1] != 4:
            raise ValueError(f'query_indices must be [N, 4] (batch, x, y, z), got {tuple(indices.shape)}')
        batch, xyz = indices[:, 0], indices[:, 1:]
        if self.pe_type in ('sine', 'fourier'):
            pos_emb = self._position_embedding(xyz, batch)
            query += pos_emb                       # in place, as the library does: the caller's query_feats (and key_feats) change
            key += pos_emb
        n, c = query.shape
        heads = (n, self.num_heads, c // self.num_heads)
        q = (self.q(query).reshape(heads) * self.scale).float()
        k = self.k(key).reshape(heads).float()
        v = self.v(value).reshape(heads).float()
        entry = self._plan(sptr_tensor, xyz, batch)
        tables = {}
        if self.pe_type == 'contextual':
            tables = dict(pe_type='contextual', rel_query=self.rel_query, rel_key=self.rel_key, rel_value=self.rel_value,
                          quant_size=self.quant_size, quant_grid_length=self.quant_grid_length,
                          relative_pos_query_table=self.relative_pos_query_table.float(),
                          relative_pos_key_table=self.relative_pos_key_table.float(),
                          relative_pos_value_table=self.relative_pos_value_table.float())
        x = sparse_self_attention(q, k, v, xyz.float(), *entry[:6], window_size=self.window_size, shift_win=self.shift_win, **tables)
        x = self.proj_drop(self.proj(x.view(n, c)))
        return SparseTrTensor(x, indices, sptr_tensor.spatial_shape, sptr_tensor.batch_size)
