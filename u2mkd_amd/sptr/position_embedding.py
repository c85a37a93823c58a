"""Absolute position embeddings of point coordinates for :class:`~u2mkd_amd.sptr.modules.VarLengthMultiheadSA`
(``pe_type`` 'sine' / 'fourier'): the class ``sptr.position_embedding.PositionEmbeddingCoordsSine`` of the library's import
surface, written from its formulas.

With ``normalize`` every coordinate is first mapped to [0, 1] over the box handed in, u = (x - lo) / (hi - lo).

sine     The ``d_pos`` channels are split over the three axes in even blocks: c = d_pos // 3 rounded down to an even number per
         axis, and what is left over goes, two channels at a time, to the first axes.  Channel i of an axis block of c
         channels has the wavelength factor w_i = temperature ** (2 * (i // 2) / c); even channels hold
         sin(scale * u / w_i), odd channels cos(scale * u / w_i); the axis blocks follow one another (x, y, z).
fourier  Random Fourier features: with a fixed Gaussian matrix B [3, d_pos / 2] (buffer ``gauss_B``, drawn once and
         multiplied by ``gauss_scale``), z = (2 pi u) B and the embedding is [sin z | cos z].

Input [batch, points, 3]; output [batch, d_pos, points], computed without gradient.  Everything is a handful of torch
element-wise operators on a [points, 3] array per scene (host plumbing, no hot path)."""
import math

import torch
from torch import nn

__all__ = ['PositionEmbeddingCoordsSine']


def _to_unit_box(points, box):
    """``points`` [B, N, 3] mapped affinely so that ``box`` = (lo [B, 3], hi [B, 3]) becomes the unit cube"""
    lo, hi = (edge.unsqueeze(1) for edge in box)
    if lo.shape != hi.shape or lo.shape[0] != points.shape[0] or lo.shape[2] != points.shape[2]:
        raise ValueError(f'input_range must be two [batch, 3] tensors for points {tuple(points.shape)}')
    return (points - lo) / (hi - lo)


class PositionEmbeddingCoordsSine(nn.Module):
    def __init__(self, temperature=10000, normalize=False, scale=None, pos_type='fourier', d_pos=None, d_in=3, gauss_scale=1.0):
        super().__init__()
        if pos_type not in ('sine', 'fourier'):
            raise ValueError(f'unknown position embedding {pos_type!r}: "sine" or "fourier"')
        if scale is not None and not normalize:
            raise ValueError('a scale applies to coordinates normalised to the unit box: pass normalize=True with it')
        self.temperature, self.normalize, self.pos_type, self.d_pos = temperature, normalize, pos_type, d_pos
        self.scale = 2 * math.pi if scale is None else scale
        if pos_type == 'fourier':
            if d_pos is None or d_pos % 2:
                raise ValueError(f'fourier features come in sin / cos pairs: d_pos={d_pos} must be even')
            self.register_buffer('gauss_B', gauss_scale * torch.randn(d_in, d_pos // 2))

    def _sine(self, u):
        """u [B, N, 3] -> [B, N, d_pos]"""
        batch, points, axes = u.shape
        block = self.d_pos // axes
        block -= block % 2
        widths = [block] * axes
        for d in range((self.d_pos - block * axes) // 2):        # the remainder, two channels at a time, to the first axes
            widths[d] += 2
        out = u.new_empty(batch, points, sum(widths))
        first = 0
        for d, c in enumerate(widths):
            i = torch.arange(c, dtype=torch.float32, device=u.device)
            wavelength = self.temperature ** (2 * (i // 2) / c)
            x = u[..., d] * self.scale if self.scale else u[..., d]
            phase = x.unsqueeze(-1) / wavelength
            chunk = out[..., first:first + c]
            chunk[..., 0::2] = phase[..., 0::2].sin()
            chunk[..., 1::2] = phase[..., 1::2].cos()
            first += c
        return out

    def _fourier(self, u, num_channels):
        """u [B, N, 3] -> [B, N, num_channels]"""
        rows, cols = self.gauss_B.shape
        half = cols if num_channels is None else num_channels // 2
        if u.shape[-1] != rows or not 0 < half <= cols or (num_channels is not None and num_channels % 2):
            raise ValueError(f'gauss_B {tuple(self.gauss_B.shape)} cannot give {num_channels} channels for points {tuple(u.shape)}')
        z = (u * (2 * math.pi)) @ self.gauss_B[:, :half]
        return torch.cat([z.sin(), z.cos()], dim=-1)

    @torch.no_grad()
    def forward(self, xyz, num_channels=None, input_range=None):
        if not (isinstance(xyz, torch.Tensor) and xyz.ndim == 3):
            raise ValueError('xyz must be a [batch, points, 3] tensor')
        u = _to_unit_box(xyz, input_range) if self.normalize else xyz
        e = self._sine(u) if self.pos_type == 'sine' else self._fourier(u, num_channels)
        return e.transpose(1, 2)
