"""The rest of torchsparse.nn (v1.4.0) through the drop-in: GroupNorm, GlobalAvgPool, GlobalMaxPool, SparseCrop and the functional
forms resolve after install_as_torchsparse(); GroupNorm is an nn.GroupNorm; CPU tensors raise (there is no CPU path).  No GPU."""
import importlib
import sys

import pytest
import torch
from torch import nn


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


def test_new_names_resolve(torchsparse):
    import torchsparse.nn as spnn
    import torchsparse.nn.functional as F
    for name in ('GroupNorm', 'GlobalAvgPool', 'GlobalMaxPool', 'SparseCrop', 'Conv3d', 'BatchNorm', 'ReLU', 'LeakyReLU'):
        assert isinstance(getattr(spnn, name), type) and issubclass(getattr(spnn, name), nn.Module), name
        assert name in spnn.__all__
    for name in ('group_norm', 'global_avg_pool', 'global_max_pool', 'spcrop', 'relu', 'leaky_relu'):
        assert callable(getattr(F, name)), name
        assert name in F.__all__
    from torchsparse.nn import GroupNorm, GlobalAvgPool, GlobalMaxPool, SparseCrop      # noqa: F401


def test_group_norm_is_an_nn_group_norm(torchsparse):
    import torchsparse.nn as spnn
    gn = spnn.GroupNorm(4, 32)
    assert isinstance(gn, nn.GroupNorm)
    assert (gn.num_groups, gn.num_channels, gn.eps, gn.affine) == (4, 32, 1e-5, True)
    ref = nn.GroupNorm(4, 32)
    with torch.no_grad():
        ref.weight.normal_()
        ref.bias.normal_()
    assert sorted(gn.state_dict()) == sorted(ref.state_dict()) == ['bias', 'weight']
    gn.load_state_dict(ref.state_dict())
    assert torch.equal(gn.weight, ref.weight) and torch.equal(gn.bias, ref.bias)
    plain = spnn.GroupNorm(2, 8, eps=1e-3, affine=False)
    assert plain.weight is None and plain.bias is None and plain.eps == 1e-3 and not plain.state_dict()
    crop = spnn.SparseCrop((0, 0, 0), (3, 3, 3))
    assert crop.coords_min == (0, 0, 0) and crop.coords_max == (3, 3, 3)


def test_cpu_sparse_tensors_raise(torchsparse):
    import torchsparse.nn as spnn
    import torchsparse.nn.functional as F
    x = torchsparse.SparseTensor(torch.randn(6, 8), torch.zeros(6, 4, dtype=torch.int32))
    for call in (lambda: spnn.GroupNorm(2, 8)(x), lambda: spnn.GlobalAvgPool()(x), lambda: spnn.GlobalMaxPool()(x),
                 lambda: spnn.SparseCrop((0, 0, 0), (1, 1, 1))(x), lambda: F.group_norm(x, 2), lambda: F.global_avg_pool(x),
                 lambda: F.global_max_pool(x), lambda: F.spcrop(x, (0, 0, 0)), lambda: F.relu(x), lambda: F.leaky_relu(x)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()


def test_scene_entries_are_declared_and_bound():
    from u2mkd_amd import _lib
    lib = _lib.load()
    for name in ('u2mkd_scene_num_slabs', 'u2mkd_scene_slabs', 'u2mkd_gn_forward', 'u2mkd_gn_backward',
                 'u2mkd_scene_pool_forward', 'u2mkd_scene_pool_backward'):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.u2mkd_scene_num_slabs(642, 5) == 6 + 5 and lib.u2mkd_scene_num_slabs(0, 3) == 0
    assert lib.u2mkd_scene_num_slabs(80000, 2) == 625 + 2


def test_errors_launch_nothing():
    """argument checks of the scene entries answer before anything touches the device: no GPU is needed to see them"""
    from u2mkd_amd import _lib
    lib = _lib.load()
    err = lambda: lib.u2mkd_last_error().decode()
    P = 4096      # (any aligned non-null address: a failing check returns before it is used)
    ns = lib.u2mkd_scene_num_slabs(10, 1)
    fwd = lambda x=P, rd=0, c=8, g=2, y=P, slabs=P, partial=P: lib.u2mkd_gn_forward(
        x, rd, 10, c, g, P, P, P, P, slabs, ns, 1, P, P, 1e-5, partial, P, P, y, None)
    assert fwd(g=3) == 2 and 'do not divide' in err()
    assert fwd(c=6, g=3) == 2 and 'multiple of 4' in err()
    assert fwd(rd=3) == 2 and 'row dtype' in err()
    assert fwd(x=P + 4) == 2 and '16-byte aligned' in err()
    assert fwd(partial=None) == 2 and 'null pointer' in err()
    bwd = lambda dy=P, g=2, dgamma=P: lib.u2mkd_gn_backward(dy, P, 0, 10, 8, g, P, P, P, P, P, ns, 1, P, P, P, P, P, dgamma, P, P, None)
    assert bwd(g=3) == 2 and 'do not divide' in err()
    assert bwd(dy=None) == 2 and 'null pointer' in err()
    assert bwd(dgamma=None) == 2 and 'go together' in err()
    pool = lambda mode=0, x=P, rd=0: lib.u2mkd_scene_pool_forward(x, rd, 10, 8, mode, P, P, P, P, ns, 1, P, P, P, None)
    assert pool(mode=2) == 2 and 'mode' in err()
    assert pool(x=None) == 2 and 'null pointer' in err()
    assert pool(rd=-1) == 2 and 'row dtype' in err()
    assert lib.u2mkd_scene_pool_backward(P, 0, 10, 8, 0, P, P, None, 1, None, None) == 2 and 'null pointer' in err()
    assert lib.u2mkd_scene_slabs(P, 1, 10, P, P, ns + 1, None) == 2 and 'u2mkd_scene_num_slabs' in err()
