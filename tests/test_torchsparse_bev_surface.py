"""The BEV modules of torchsparse.nn (v1.4.0) through the drop-in: the four classes and the four functional forms resolve after
install_as_torchsparse(), carry upstream's parameters, buffers and state-dict keys, CPU tensors raise (there is no CPU path), and
the C entries of csrc/bev.hip are declared, exported and answer their argument checks before anything touches the device.  No GPU."""
import importlib
import math
import sys

import pytest
import torch
from torch import nn

CLASSES = ('ToBEVReduction', 'ToBEVConvolution', 'ToDenseBEVConvolution', 'ToBEVHeightCompression')
FUNCTIONS = ('to_bev_reduction', 'to_bev_convolution', 'to_dense_bev_convolution', 'to_bev_height_compression')
ENTRIES = ('u2mkd_bev_plan', 'u2mkd_bev_tables', 'u2mkd_bev_segment_mean', 'u2mkd_bev_dense_store', 'u2mkd_bev_dense_gather')


@pytest.fixture()
def torchsparse():
    import u2mkd_amd
    saved = {k: v for k, v in sys.modules.items() if k == 'torchsparse' or k.startswith('torchsparse.')}
    u2mkd_amd.install_as_torchsparse()
    try:
        yield importlib.import_module('torchsparse')
    finally:
        for k in [k for k in sys.modules if k == 'torchsparse' or k.startswith('torchsparse.')]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_names_resolve_and_are_exported(torchsparse):
    import torchsparse.nn as spnn
    import torchsparse.nn.functional as F
    for name in CLASSES:
        assert isinstance(getattr(spnn, name), type) and issubclass(getattr(spnn, name), nn.Module), name
        assert name in spnn.__all__
    for name in FUNCTIONS:
        assert callable(getattr(F, name)), name
        assert name in F.__all__
    from torchsparse.nn import ToBEVReduction, ToBEVConvolution, ToDenseBEVConvolution, ToBEVHeightCompression      # noqa: F401


def test_parameters_buffers_and_init(torchsparse):
    import torchsparse.nn as spnn
    torch.manual_seed(0)
    conv = spnn.ToBEVConvolution(16, 24, 5, stride=2, dim=2, bias=True)
    assert sorted(conv.state_dict()) == ['bias', 'kernel']
    assert conv.kernel.shape == (5, 16, 24) and conv.bias.shape == (1, 24) and int(torch.count_nonzero(conv.bias)) == 0
    assert isinstance(conv.kernel, nn.Parameter) and isinstance(conv.bias, nn.Parameter)
    lim = 1 / math.sqrt(16)
    assert float(conv.kernel.abs().max()) <= lim and float(conv.kernel.abs().max()) > 0.9 * lim
    assert float(conv.kernel.min()) < 0 < float(conv.kernel.max())
    assert (conv.n_kernels, conv.stride, conv.dim) == (5, 2, 2)
    plain = spnn.ToBEVConvolution(16, 24, 5)
    assert plain.bias == 0 and not isinstance(plain.bias, torch.Tensor) and sorted(plain.state_dict()) == ['kernel']
    assert (plain.stride, plain.dim) == (1, 1)

    dense = spnn.ToDenseBEVConvolution(8, 12, shape=(5, 3, 7), offset=(2, 0, 4), dim=1, bias=True)
    assert sorted(dense.state_dict()) == ['bias', 'kernel', 'offset']
    assert dense.kernel.shape == (3, 8, 12) and dense.n_kernels == 3 and dense.bias.shape == (1, 12)
    assert dense.offset.dtype == torch.int32 and dense.offset.tolist() == [[2, 0, 4, 0]]
    assert 'offset' in dict(dense.named_buffers()) and float(dense.kernel.abs().max()) <= 1 / math.sqrt(8)
    assert sorted(spnn.ToDenseBEVConvolution(8, 12, torch.tensor([5, 3, 7])).state_dict()) == ['kernel', 'offset']

    hc = spnn.ToBEVHeightCompression(8, shape=(5, 3, 7), offset=(2, 0, 4), dim=0)
    assert not list(hc.parameters()) and sorted(hc.state_dict()) == ['offset'] and hc.offset.tolist() == [[2, 0, 4, 0]]
    red = spnn.ToBEVReduction()
    assert red.dim == 1 and not red.state_dict()


def test_state_dict_without_offset_loads_and_keeps_the_constructors_value(torchsparse):
    import torchsparse.nn as spnn
    src = spnn.ToDenseBEVConvolution(8, 12, (5, 3, 7), offset=(9, 9, 9), bias=True)
    sd = {k: v for k, v in src.state_dict().items() if k != 'offset'}
    dst = spnn.ToDenseBEVConvolution(8, 12, (5, 3, 7), offset=(2, 0, 4), bias=True)
    dst.load_state_dict(sd)
    assert torch.equal(dst.kernel, src.kernel) and dst.offset.tolist() == [[2, 0, 4, 0]] and dst._offset == (2, 0, 4)
    dst.load_state_dict(src.state_dict())                  # ... and one with it brings it, for the host's copy too
    assert dst.offset.tolist() == [[9, 9, 9, 0]] and dst._offset == (9, 9, 9)
    hc = spnn.ToBEVHeightCompression(8, (5, 3, 7), offset=(1, 2, 3))
    hc.load_state_dict({})
    assert hc.offset.tolist() == [[1, 2, 3, 0]]


def test_extra_repr_does_not_raise(torchsparse):
    import torchsparse.nn as spnn
    for m in (spnn.ToBEVReduction(2), spnn.ToBEVConvolution(4, 8, 3, bias=True), spnn.ToDenseBEVConvolution(4, 8, (5, 3, 7)),
              spnn.ToBEVHeightCompression(4, (5, 3, 7))):
        assert type(m).__name__ in repr(m) and isinstance(m.extra_repr(), str)


def test_cpu_sparse_tensors_raise(torchsparse):
    import torchsparse.nn as spnn
    import torchsparse.nn.functional as F
    x = torchsparse.SparseTensor(torch.randn(6, 8), torch.zeros(6, 4, dtype=torch.int32))
    k, b = torch.randn(3, 8, 4), torch.zeros(1, 4)
    for call in (lambda: spnn.ToBEVReduction()(x), lambda: spnn.ToBEVConvolution(8, 4, 3)(x),
                 lambda: spnn.ToDenseBEVConvolution(8, 4, (5, 3, 7))(x), lambda: spnn.ToBEVHeightCompression(8, (5, 3, 7))(x),
                 lambda: F.to_bev_reduction(x), lambda: F.to_bev_convolution(x, k, b),
                 lambda: F.to_dense_bev_convolution(x, k, b, (5, 3, 7)), lambda: F.to_bev_height_compression(x, 8, (5, 3, 7))):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()


def test_bev_entries_are_declared_and_bound():
    from u2mkd_amd import _lib
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_errors_launch_nothing():
    """the argument checks of the BEV entries answer before anything touches the device: no GPU is needed to see them"""
    from u2mkd_amd import _lib
    lib = _lib.load()
    err = lambda: lib.u2mkd_last_error().decode()
    P = 4096      # (any aligned non-null address: a failing check returns before it is used)

    def plan(coords=P, dim=1, mode=1, hmode=1, s=(1, 1, 1), a=(0, 0, 0), h=5, w=7, nz=3, keys=P, block=P):
        return lib.u2mkd_bev_plan(coords, 10, dim, mode, hmode, *s, *a, h, w, nz, keys, P, block, None)
    assert plan(dim=3) == 2 and 'dim=3 outside 0..2' in err()
    assert plan(dim=-1) == 2 and 'outside 0..2' in err()
    assert plan(h=0) == 2 and 'non-positive shape' in err()
    assert plan(w=-7) == 2 and 'non-positive shape' in err()
    assert plan(nz=0) == 2 and 'non-positive shape' in err()
    assert plan(s=(1, 0, 1)) == 2 and 'non-positive tensor stride' in err()
    assert plan(mode=0, a=(1, 0, 1)) == 2 and 'non-positive cell size' in err()
    assert plan(mode=0, hmode=2, a=(1, 1, 1)) == 2 and 'hmode' in err()
    assert plan(coords=None) == 2 and 'null pointer' in err()
    assert plan(keys=None) == 2 and 'null pointer' in err()
    assert plan(block=None) == 2 and 'null pointer' in err()
    assert plan(coords=P + 4) == 2 and '16-byte aligned' in err()

    for name in ('u2mkd_bev_dense_store', 'u2mkd_bev_dense_gather'):
        def dense(a=P, rd=0, n=10, c=8, seg=P, order=P, nb=3, z=2, h=5, w=7, o=P):
            return getattr(lib, name)(a, rd, n, c, seg, order, nb, z, h, w, o, None)
        assert dense(rd=3) == 2 and 'row dtype' in err() and name in err()
        assert dense(rd=-1) == 2 and 'row dtype' in err()
        assert dense(c=6) == 2 and 'multiple of 4' in err()
        assert dense(c=0) == 2 and 'multiple of 4' in err()
        assert dense(h=0) == 2 and 'non-positive shape' in err()
        assert dense(z=0) == 2 and 'non-positive shape' in err()
        assert dense(z=33) == 2 and 'at most 32' in err()
        assert dense(a=None) == 2 and 'null pointer' in err()
        assert dense(o=None) == 2 and 'null pointer' in err()
        assert dense(a=P + 8) == 2 and '16-byte aligned' in err()
        assert dense(o=P + 4) == 2 and '16-byte aligned' in err()
        assert dense(order=None) == 2 and 'go together' in err()
        assert dense(seg=None, order=None) == 2 and 'the rows are the cells' in err()
        assert dense(nb=70000) == 2 and 'nb' in err()

    mean = lambda src=P, rd=0, c=8, seg=P, out=P: lib.u2mkd_bev_segment_mean(src, rd, 10, c, P, seg, 4, out, None)
    assert mean(rd=5) == 2 and 'row dtype' in err()
    assert mean(c=10) == 2 and 'multiple of 4' in err()
    assert mean(seg=None) == 2 and 'null pointer' in err()
    assert mean(out=P + 4) == 2 and '16-byte aligned' in err()
    tables = lambda nk=3, nbr=P: lib.u2mkd_bev_tables(P, P, 10, 6, nk, nbr, P, None)
    assert tables(nk=0) == 2 and 'non-positive shape' in err()
    assert tables(nbr=None) == 2 and 'null pointer' in err()
