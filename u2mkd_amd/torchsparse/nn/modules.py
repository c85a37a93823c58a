"""torchsparse.nn modules (core/models/build_blocks.py:25-80).

State-dict compatibility with the reference checkpoints: the conv weight is the
parameter ``kernel`` of shape [K, Cin, Cout] ([Cin, Cout] when K == 1), init
U(+-1/sqrt(fan * K)) with fan = Cout if transposed else Cin (v1.4.0).
BatchNorm / ReLU stay nn.BatchNorm1d / nn.ReLU subclasses so that
SparseSyncBatchNorm.convert_sync_batchnorm (core/models/utils.py:179) finds them.
"""
import math

import numpy as np
import torch
from torch import nn

from ..utils import make_ntuple
from . import functional as F
from .utils import fapply

__all__ = ['Conv3d', 'BatchNorm', 'ReLU', 'LeakyReLU', 'GroupNorm', 'GlobalAvgPool', 'GlobalMaxPool', 'SparseCrop',
           'ToBEVReduction', 'ToBEVConvolution', 'ToDenseBEVConvolution', 'ToBEVHeightCompression']


class Conv3d(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, dilation=1,
                 bias=False, transposed=False):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = make_ntuple(kernel_size, ndim=3)
        self.stride = make_ntuple(stride, ndim=3)
        self.dilation = dilation
        self.transposed = transposed
        self.kernel_volume = int(np.prod(self.kernel_size))
        if self.kernel_volume > 1:
            self.kernel = nn.Parameter(torch.zeros(self.kernel_volume, in_channels, out_channels))
        else:
            self.kernel = nn.Parameter(torch.zeros(in_channels, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def extra_repr(self):
        s = '{in_channels}, {out_channels}, kernel_size={kernel_size}'
        if self.stride != (1,) * len(self.stride):
            s += ', stride={stride}'
        if self.dilation != 1:
            s += ', dilation={dilation}'
        if self.bias is None:
            s += ', bias=False'
        if self.transposed:
            s += ', transposed=True'
        return s.format(**self.__dict__)

    def reset_parameters(self):
        std = 1 / math.sqrt((self.out_channels if self.transposed else self.in_channels)
                            * self.kernel_volume)
        self.kernel.data.uniform_(-std, std)
        if self.bias is not None:
            self.bias.data.uniform_(-std, std)

    def forward(self, input):
        return F.conv3d(input, self.kernel, kernel_size=self.kernel_size, bias=self.bias,
                        stride=self.stride, dilation=self.dilation, transposed=self.transposed)


class BatchNorm(nn.BatchNorm1d):
    """nn.BatchNorm1d over SparseTensor.feats on the HIP BatchNorm kernels."""

    def forward(self, input):
        return fapply(input, F.batch_norm, self)


class ReLU(nn.ReLU):
    def forward(self, input):
        return fapply(input, super().forward)


class LeakyReLU(nn.LeakyReLU):
    def forward(self, input):
        return fapply(input, super().forward)


class GroupNorm(nn.GroupNorm):
    """nn.GroupNorm (same parameters and state-dict keys) over the rows of every scene of a SparseTensor: mean and biased
    variance per (scene, group) over the (C / G) x N_k elements, on the scene kernels (F.group_norm)."""

    def forward(self, input):
        return F.group_norm(input, self.num_groups, self.weight, self.bias, self.eps)


class GlobalAvgPool(nn.Module):
    def forward(self, input):
        return F.global_avg_pool(input)


class GlobalMaxPool(nn.Module):
    def forward(self, input):
        return F.global_max_pool(input)


class SparseCrop(nn.Module):
    def __init__(self, coords_min=None, coords_max=None):
        super().__init__()
        self.coords_min = coords_min
        self.coords_max = coords_max

    def forward(self, input):
        return F.spcrop(input, self.coords_min, self.coords_max)


def _bev_kernel(module, n_kernels, in_channels, out_channels, bias):
    """``kernel`` [n_kernels, Cin, Cout] uniform in +-1 / sqrt(Cin); ``bias`` [1, Cout] of zeros, or the integer 0 (no state-dict key)"""
    module.kernel = nn.Parameter(torch.zeros(n_kernels, in_channels, out_channels))
    module.bias = nn.Parameter(torch.zeros(1, out_channels)) if bias else 0
    std = 1. / math.sqrt(in_channels)
    module.kernel.data.uniform_(-std, std)


class ToBEVReduction(nn.Module):
    """The rows of a BEV column (same batch index and BEV coordinates) become one row at height 0: their mean."""

    def __init__(self, dim=1):
        super().__init__()
        self.dim = dim

    def extra_repr(self):
        return 'dim = {}'.format(self.dim)

    def forward(self, input):
        return F.to_bev_reduction(input, self.dim)


class ToBEVConvolution(nn.Module):
    """A convolution whose offset is the row's own height index: y_r = feats_r @ kernel[z_r] + bias, summed per BEV cell."""

    def __init__(self, in_channels, out_channels, n_kernels, stride=1, dim=1, bias=False):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.n_kernels = n_kernels
        self.stride = stride
        self.dim = dim
        _bev_kernel(self, n_kernels, in_channels, out_channels, bias)

    def extra_repr(self):
        return 'in_channels={}, out_channels={}, n_kernels={}, stride={}'.format(self.in_channels, self.out_channels, self.n_kernels,
                                                                                 self.stride)

    def forward(self, input):
        return F.to_bev_convolution(input, self.kernel, self.bias, self.stride, self.dim)


class _BEVGrid(nn.Module):
    """shape, offset and height axis of the dense BEV modules.  ``offset`` is a persistent int32 buffer [1, 4] = offset + [0], as
    upstream; the host keeps its three values next to it (taken at construction and whenever a state dict brings the buffer), so
    no forward reads the buffer back from the device.  A state dict without ``offset`` loads: the constructor's value is kept."""

    def _init_grid(self, shape, offset, dim):
        self.dim = dim
        self.shape = tuple(int(v) for v in (shape.tolist() if isinstance(shape, torch.Tensor) else shape))
        self._offset = tuple(int(v) for v in list(offset)[:3])
        self.register_buffer('offset', torch.tensor([list(self._offset) + [0]], dtype=torch.int32))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        key = prefix + 'offset'
        if key in state_dict:
            self._offset = tuple(int(v) for v in state_dict[key].flatten().tolist()[:3])
        else:
            state_dict = dict(state_dict)
            state_dict[key] = self.offset
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)


class ToDenseBEVConvolution(_BEVGrid):
    """ToBEVConvolution onto a dense [B, Cout, H, W] grid: n_kernels = shape[dim], (H, W) = shape[BEV axes]."""

    def __init__(self, in_channels, out_channels, shape, offset=(0, 0, 0), dim=1, bias=False):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self._init_grid(shape, offset, dim)
        self.n_kernels = int(self.shape[dim])
        _bev_kernel(self, self.n_kernels, in_channels, out_channels, bias)

    def extra_repr(self):
        return 'in_channels={}, out_channels={}, n_kernels={}'.format(self.in_channels, self.out_channels, self.n_kernels)

    def forward(self, input):
        return F.to_dense_bev_convolution(input, self.kernel, self.bias, self.shape, self._offset, self.dim)


class ToBEVHeightCompression(_BEVGrid):
    """The Z height slots of every BEV cell become channel groups of a dense [B, C * Z, H, W] tensor (channel c * Z + w)."""

    def __init__(self, channels, shape, offset=(0, 0, 0), dim=1):
        super().__init__()
        self.channels = channels
        self._init_grid(shape, offset, dim)

    def extra_repr(self):
        return 'channels={}'.format(self.channels)

    def forward(self, input):
        return F.to_bev_height_compression(input, self.channels, self.shape, self._offset, self.dim)
