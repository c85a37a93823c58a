from . import functional, utils
from .modules import (Conv3d, BatchNorm, ReLU, LeakyReLU, GroupNorm, GlobalAvgPool, GlobalMaxPool, SparseCrop,
                      ToBEVReduction, ToBEVConvolution, ToDenseBEVConvolution, ToBEVHeightCompression)

__all__ = ['functional', 'utils', 'Conv3d', 'BatchNorm', 'ReLU', 'LeakyReLU', 'GroupNorm', 'GlobalAvgPool', 'GlobalMaxPool',
           'SparseCrop', 'ToBEVReduction', 'ToBEVConvolution', 'ToDenseBEVConvolution', 'ToBEVHeightCompression']
