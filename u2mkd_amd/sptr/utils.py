"""``sptr.utils`` import path of the reference (sptr/utils.py): the two names of it that exist here.  The CSR softmax and the
pair-list sampling of that file have no counterpart: the fused kernels never build the pair arrays they work on."""
from . import to_3d_numpy
from .functional import get_indices_params

__all__ = ['to_3d_numpy', 'get_indices_params']
