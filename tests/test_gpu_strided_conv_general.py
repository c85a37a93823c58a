"""Strided sparse convs whose stride differs from the kernel size (k = 3, s = 2; kernel (3,3,3) with stride (2,2,1)): the general
branch of ``F.spdownsample`` (u2mkd_downsample_keys_general) and a non-symmetric K = 27 map with n_out unrelated to n_in / 8
through the map builders, the three convolution schedules, both gradients, the transposed form, bf16 rows, the v1.4.0
backend-format entries and the module level of the drop-in.  Coordinates and maps bit-exact against the numpy restatement
(tests/downsample_general_ref.py) and oracle.ts_ref; features against oracle.ts_ref, a dense float64 convolution and
oracle.torchsparse_cpu."""
import ctypes

import numpy as np
import pytest
import torch

from downsample_general_ref import max_candidates_per_row, ref_spdownsample_general
from oracle import ts_ref as R
from u2mkd_amd.synth import synth_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def F(hip):
    from u2mkd_amd.torchsparse.nn import functional as F
    return F


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _rel(a, b):
    a = a.double().cpu()
    b = b.double().cpu() if isinstance(b, torch.Tensor) else torch.from_numpy(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _t3(v):
    return R.make_ntuple(v)


def _level(coords, ts, seed=3):
    """the scene's voxels at tensor stride ts (floored, distinct), rows permuted"""
    c = coords.copy()
    c[:, :3] = c[:, :3] // ts * ts
    c = np.unique(c[:, [3, 0, 1, 2]], axis=0)[:, [1, 2, 3, 0]].astype(np.int32)
    return np.ascontiguousarray(c[np.random.default_rng(seed).permutation(len(c))])


_SCENES = {}


def _scene_map(ts=1, seed=7):
    """(coords, restated out_coords, oracle nbmaps, nbsizes) of the k = 3, s = 2 map of one synthetic scene; computed once"""
    hit = _SCENES.get((ts, seed))
    if hit is None:
        c = _level(synth_batch(3000, 2, seed)['coords'], ts)
        oc = ref_spdownsample_general(c, 2, 3, ts)
        nbmaps, nbsizes, _, _ = R.build_kmap(c, ts, 3, 2, out_coords=oc)
        hit = _SCENES[(ts, seed)] = (c, oc, nbmaps, nbsizes)
    return hit


def _check_map(F, c, ts, ks, st):
    ts, ks, st = _t3(ts), _t3(ks), _t3(st)
    general = not all(st[a] in (1, ks[a]) for a in range(3))
    want_oc = ref_spdownsample_general(c, st, ks, ts) if general else R.spdownsample(c, st, ks, ts)
    got_oc = F.spdownsample(_dev(c), st, ks, ts)
    assert got_oc.dtype == torch.int32 and got_oc.shape == want_oc.shape and got_oc.is_contiguous()
    assert (got_oc.cpu().numpy() == want_oc).all()
    nbmaps, nbsizes, oc, results = R.build_kmap(c, ts, ks, st, out_coords=want_oc)
    km = F.build_kmap(_dev(c), ts, ks, st)
    assert (km.out_coords.cpu().numpy() == oc).all()
    assert (km.nbr.cpu().numpy() == results).all()
    got_maps, got_sizes, sizes = km[0], km[1], km[2]
    assert sizes == (len(c), len(oc))
    assert (got_sizes.cpu().numpy() == nbsizes).all()
    assert (got_maps.cpu().numpy() == nbmaps).all()
    assert not km.symmetric and km.nbr_inv is not None
    inv = np.full((results.shape[0], len(c)), -1, np.int32)
    kk, jj = np.nonzero(results != -1)
    inv[kk, results[kk, jj]] = jj
    assert (km.nbr_inv.cpu().numpy() == inv).all()
    return km


# ------------------------------------------------------------------ 1. coordinates and maps, bit-exact
@pytest.mark.parametrize('ts,ks,st', [(1, 3, 2), (2, 3, 2), (1, (3, 3, 3), (2, 2, 1)), (1, (3, 3, 1), (2, 2, 1)), (1, 3, 3)])
def test_downsample_and_kmap_bit_exact(F, ts, ks, st):
    """(1, 3, 3) takes the floor branch and must still equal the oracle's; the others take the general branch"""
    c = _level(synth_batch(3000, 2, 7)['coords'], ts)
    km = _check_map(F, c, ts, ks, st)
    if (ks, st) == (3, 2):
        assert km.k == 27 and km.n_out != km.n_in


TINY = {
    'lone_odd': [(1, 1, 1, 0)],
    'n_out_exceeds_n_in': [(0, 0, 0, 0), (1, 1, 1, 0)],
    'two_batches': [(0, 0, 0, 0), (1, 1, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1)],
    'minimum_from_the_other_batch': [(1, 1, 1, 1), (0, 0, 0, 0), (1, 1, 1, 0)],
    'negative_odd': [(-3, 1, 1, 0), (-5, 1, 1, 0)],
}


@pytest.mark.parametrize('name', sorted(TINY))
def test_tiny_inputs(F, name):
    c = np.asarray(TINY[name], dtype=np.int32)
    km = _check_map(F, c, 1, 3, 2)
    if name == 'n_out_exceeds_n_in':
        assert km.n_out == 8 and km.n_in == 2
    _check_map(F, c, 1, 3, (2, 2, 1))
    c2 = c.copy()
    c2[:, :3] *= 2
    _check_map(F, c2, 2, 3, 2)


def test_empty_input(F):
    out = F.spdownsample(torch.zeros(0, 4, dtype=torch.int32, device='cuda'), 2, 3, 1)
    assert out.shape == (0, 4) and out.dtype == torch.int32 and out.is_cuda


def test_negative_scene_and_odd_minimum(F):
    base = _level(synth_batch(3000, 2, 9)['coords'], 1)
    neg = base.copy()
    neg[:, :3] -= neg[:, :3].max(0) + 5
    assert int(neg[:, :3].max()) < 0
    _check_map(F, neg, 1, 3, 2)
    odd = base.copy()
    odd[:, 0] += 1 - odd[:, 0].min() % 2
    assert int(odd[:, 0].min()) % 2 == 1
    _check_map(F, odd, 1, 3, 2)
    _check_map(F, odd, 1, 3, (2, 2, 1))


# ------------------------------------------------------------------ 2. range flag
def _out_of_range_scenes():
    legal = _level(synth_batch(3000, 2, 7)['coords'], 1)
    hi = np.concatenate([legal, np.asarray([[131071, 3, 3, 0]], dtype=np.int32)])        # candidate x + 1 = 2^17
    lo = np.concatenate([legal, np.asarray([[-131074, 3, 3, 0]], dtype=np.int32)])       # the row itself is its kept candidate
    return legal, hi, lo


def test_range_flag_immediate(F):
    legal, hi, lo = _out_of_range_scenes()
    for bad in (hi, lo):
        with pytest.raises(ValueError, match='packed key range'):
            F.spdownsample(_dev(bad), 2, 3, 1)
        got = F.spdownsample(_dev(legal), 2, 3, 1)            # the flag was cleared: the legal scene goes through
        assert (got.cpu().numpy() == ref_spdownsample_general(legal, 2, 3, 1)).all()
    # the largest legal odd coordinate on a stride-1 axis: candidate 131071 + 1 is out, on the strided axes nothing is
    edge = np.asarray([[4, 4, 131071, 0], [0, 0, 0, 0]], dtype=np.int32)
    with pytest.raises(ValueError, match='packed key range'):
        F.spdownsample(_dev(edge), (2, 2, 1), 3, 1)
    edge[0, 2] = 131070
    got = F.spdownsample(_dev(edge), (2, 2, 1), 3, 1)
    assert (got.cpu().numpy() == ref_spdownsample_general(edge, (2, 2, 1), 3, 1)).all()


def test_range_flag_deferred(F):
    legal, hi, _ = _out_of_range_scenes()
    with pytest.raises(ValueError, match='packed key range'):
        with F.deferred_range_check():
            F.spdownsample(_dev(legal), 2, 3, 1)
            F.spdownsample(_dev(hi), 2, 3, 1)                 # no error here: the flag is read when the context ends
            F.spdownsample(_dev(legal), 2, 2, 1)
    with F.deferred_range_check():
        got = F.spdownsample(_dev(legal), 2, 3, 1)
    assert (got.cpu().numpy() == ref_spdownsample_general(legal, 2, 3, 1)).all()


def test_padding_slots_leave_the_flag_alone(F):
    c = np.asarray([[1, 1, 1, 0]], dtype=np.int32)            # 1 kept candidate, 7 of the 8 slots are padding
    assert max_candidates_per_row(2, 3) == 8
    flag = F._range_flag(torch.device('cuda', torch.cuda.current_device()))
    flag.zero_()
    with F.deferred_range_check():
        got = F.spdownsample(_dev(c), 2, 3, 1)
        assert int(flag) == 0
    assert got.cpu().tolist() == [[2, 2, 2, 0]]
    # a coordinate off the tensor-stride lattice has no candidate at all: every slot is padding
    with F.deferred_range_check():
        got = F.spdownsample(_dev(c), 2, 3, 2)
        assert int(flag) == 0
    assert got.shape == (0, 4)


# ------------------------------------------------------------------ 3. convolution parity through ConvolutionFunction
def _conv_parity(F, c, oc, nbmaps, nbsizes, km, cin, cout, apply):
    sizes = (len(c), len(oc))
    k = len(nbsizes)
    x = torch.randn(len(c), cin)
    w = torch.randn(k, cin, cout) / (k * cin) ** 0.5
    g = torch.randn(len(oc), cout)
    want = R.conv_forward(x, w, nbmaps, nbsizes, sizes)
    wgi, wgw = R.conv_backward(x, w, g, nbmaps, nbsizes)
    xd, wd = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    out = apply(xd, wd, km, False)
    assert out.shape == want.shape and _rel(out, want) < 1e-4
    out.backward(g.cuda())
    assert _rel(xd.grad, wgi) < 1e-4 and _rel(wd.grad, wgw) < 1e-4
    # up (transposed): the same map with the roles swapped
    xc = torch.randn(len(oc), cin)
    gu = torch.randn(len(c), cout)
    want = R.conv_forward(xc, w, nbmaps, nbsizes, sizes, transposed=True)
    wgi, wgw = R.conv_backward(xc, w, gu, nbmaps, nbsizes, transposed=True)
    xd, wd = xc.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    out = apply(xd, wd, km, True)
    assert out.shape == want.shape and _rel(out, want) < 1e-4
    out.backward(gu.cuda())
    assert _rel(xd.grad, wgi) < 1e-4 and _rel(wd.grad, wgw) < 1e-4


# (32,32) (64,64): the tile-pair kernel; (48,16): the sorted tile walk; (256,128): the pair schedule
@pytest.mark.parametrize('cin,cout', [(32, 32), (64, 64), (48, 16), (256, 128)])
def test_strided_k27_and_transposed_conv(F, cin, cout):
    c, oc, nbmaps, nbsizes = _scene_map(1)
    torch.manual_seed(cin + cout)
    km = F.build_kmap(_dev(c), (1,) * 3, (3,) * 3, (2,) * 3)
    assert (km.out_coords.cpu().numpy() == oc).all() and not km.symmetric
    _conv_parity(F, c, oc, nbmaps, nbsizes, km, cin, cout, F.ConvolutionFunction.apply)


def test_strided_k27_conv_at_tensor_stride_two(F):
    c, oc, nbmaps, nbsizes = _scene_map(2)
    torch.manual_seed(2)
    km = F.build_kmap(_dev(c), (2,) * 3, (3,) * 3, (2,) * 3)
    assert (km.out_coords.cpu().numpy() == oc).all()
    _conv_parity(F, c, oc, nbmaps, nbsizes, km, 32, 32, F.ConvolutionFunction.apply)


def test_strided_k27_conv3d_pads_odd_channel_counts(F):
    """(20, 12) through F.conv3d: the lazily built map, zero padding to 16-byte rows, and the transposed conv3d that looks the
    forward map up under (tensor_stride, kernel_size, stride, dilation)"""
    import u2mkd_amd.torchsparse as ts
    c, oc, nbmaps, nbsizes = _scene_map(1)
    torch.manual_seed(32)
    cd = _dev(c)
    seen = {}

    def apply(xd, wd, km, transposed):
        if not transposed:
            t = ts.SparseTensor(xd, cd)
            t.cmaps[t.stride] = cd
            y = F.conv3d(t, wd, kernel_size=3, stride=2)
            seen['kmaps'], seen['cmaps'] = y.kmaps, y.cmaps
            assert y.stride == (2, 2, 2) and (y.coords.cpu().numpy() == oc).all()
            return y.F
        t = ts.SparseTensor(xd, seen['cmaps'][(2, 2, 2)], stride=2)
        t.kmaps, t.cmaps = seen['kmaps'], seen['cmaps']
        y = F.conv3d(t, wd, kernel_size=3, stride=2, transposed=True)
        assert y.stride == (1, 1, 1) and y.coords is cd
        return y.F
    _conv_parity(F, c, oc, nbmaps, nbsizes, None, 20, 12, apply)


# ------------------------------------------------------------------ 4. dense identity in float64
def test_k3s2_conv_equals_a_dense_float64_convolution(F):
    """F.conv3d(x, w, 3, stride=2) against torch.nn.functional.conv3d(dense, W, stride=2, padding=1) on the CPU in float64:
    nothing of the oracle's map code is involved.  Minimum 0 on every axis, so output sites are the even lattice points
    2 i >= 0 with an input in their 3 x 3 x 3 window: index i of the dense output.  Features within 2^-20 * sum |x| |w| per
    element, the bound tests/test_gpu_conv_f16x2.py holds the engine to against float64."""
    import u2mkd_amd.torchsparse as ts
    rng = np.random.default_rng(5)
    box, grid, cin, cout = 24, 26, 8, 8       # sites 0..24 -> dense output index 0..12 = (26 + 2 - 3) // 2 + 1 entries
    flat = rng.choice(box ** 3, 1500, replace=False)
    xyz = np.stack(np.unravel_index(flat, (box,) * 3), 1).astype(np.int32)
    assert (xyz.min(0) == 0).all()
    c = np.concatenate([xyz, np.zeros((len(xyz), 1), np.int32)], 1)
    torch.manual_seed(4)
    x = torch.randn(len(c), cin)
    w = torch.randn(27, cin, cout) / (27 * cin) ** 0.5
    y = F.conv3d(ts.SparseTensor(x.cuda(), _dev(c)), w.cuda(), kernel_size=3, stride=2)
    assert y.stride == (2, 2, 2)
    p = torch.from_numpy(xyz).long()
    dense = torch.zeros(1, cin, grid, grid, grid, dtype=torch.float64)
    dense[0][:, p[:, 0], p[:, 1], p[:, 2]] = x.double().t()
    occ = torch.zeros(1, 1, grid, grid, grid, dtype=torch.float64)
    occ[0, 0][p[:, 0], p[:, 1], p[:, 2]] = 1.0
    W = torch.zeros(cout, cin, 3, 3, 3, dtype=torch.float64)
    for k, (dx, dy, dz) in enumerate(R.get_kernel_offsets(3, 1).tolist()):
        W[:, :, dx + 1, dy + 1, dz + 1] = w[k].double().t()
    conv = torch.nn.functional.conv3d
    want = conv(dense, W, stride=2, padding=1)[0]
    mag = conv(dense.abs(), W.abs(), stride=2, padding=1)[0]
    active = conv(occ, torch.ones(1, 1, 3, 3, 3, dtype=torch.float64), stride=2, padding=1)[0, 0] > 0
    assert active.shape == (13, 13, 13)
    oc = y.coords.cpu().numpy()
    assert (oc[:, 3] == 0).all() and (oc[:, :3] % 2 == 0).all() and oc[:, :3].min() >= 0 and oc[:, :3].max() <= 24
    got_active = torch.zeros_like(active)
    i = torch.from_numpy(oc[:, :3] // 2).long()
    got_active[i[:, 0], i[:, 1], i[:, 2]] = True
    assert len(oc) == int(active.sum()) and bool((got_active == active).all())
    want_rows = want[:, i[:, 0], i[:, 1], i[:, 2]].t()
    mag_rows = mag[:, i[:, 0], i[:, 1], i[:, 2]].t()
    err = (y.F.double().cpu() - want_rows).abs()
    bound = mag_rows * 2.0 ** -20 + 1e-300
    assert bool((err <= bound).all()), float((err / bound).max())


# ------------------------------------------------------------------ 5. module level over the drop-in
def _encoder_decoder(pkg):
    spnn = pkg.nn

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.down = torch.nn.Sequential(spnn.Conv3d(16, 32, 3, stride=2), spnn.BatchNorm(32), spnn.ReLU(True))
            self.mid = torch.nn.Sequential(spnn.Conv3d(32, 32, 3), spnn.BatchNorm(32), spnn.ReLU(True))
            self.up = torch.nn.Sequential(spnn.Conv3d(32, 16, 3, stride=2, transposed=True), spnn.BatchNorm(16), spnn.ReLU(True))
            self.head = spnn.Conv3d(32, 20, 1)

        def forward(self, x):
            u = self.up(self.mid(self.down(x)))
            return u, self.head(pkg.cat([u, x]))
    return Net()


def test_encoder_decoder_over_the_drop_in_matches_the_cpu_oracle(hip):
    """spnn.Conv3d(16,32,3,stride=2) -> Conv3d(32,32,3) -> Conv3d(32,16,3,stride=2,transposed=True) with BatchNorm / ReLU in
    between and torchsparse.cat with the skip, one forward + backward, against the same modules of oracle.torchsparse_cpu with
    identical weights (its conv3d takes the pre-seeded k = 3, s = 2 map).  Logits within 1e-3, every parameter gradient within
    5e-3 relative: the gates of tests/test_gpu_reference_sequence.py."""
    import sys
    import u2mkd_amd
    from oracle import torchsparse_cpu as ots
    before = {k: v for k, v in sys.modules.items() if k == 'torchsparse' or k.startswith('torchsparse.')}
    u2mkd_amd.install_as_torchsparse()
    try:
        import torchsparse
        import torchsparse.nn as spnn
        assert torchsparse.__name__ == 'u2mkd_amd.torchsparse' and spnn is torchsparse.nn
    finally:                          # (the names stay bound to the objects; later tests find sys.modules as it was)
        for k in [k for k in sys.modules if k == 'torchsparse' or k.startswith('torchsparse.')]:
            del sys.modules[k]
        sys.modules.update(before)
    c, oc, nbmaps, nbsizes = _scene_map(1)
    torch.manual_seed(8)
    ref = _encoder_decoder(ots).train()
    net = _encoder_decoder(torchsparse)
    net.load_state_dict(ref.state_dict())
    net.cuda().train()
    feats = torch.randn(len(c), 16)
    gl = torch.randn(len(c), 20)
    # the CPU oracle
    xr = ots.SparseTensor(feats.clone(), torch.from_numpy(c))
    xr.cmaps[xr.stride] = xr.coords
    key = ((1, 1, 1), (3, 3, 3), (2, 2, 2), (1, 1, 1))
    xr.kmaps[key] = [torch.from_numpy(nbmaps), torch.from_numpy(nbsizes), (len(c), len(oc)), torch.from_numpy(oc)]
    ur, lr = ref(xr)
    (lr.F * gl).sum().backward()
    # the drop-in
    xd = torchsparse.SparseTensor(feats.cuda(), _dev(c))
    xd.cmaps[xd.stride] = xd.coords
    ud, ld = net(xd)
    (ld.F * gl.cuda()).sum().backward()
    assert ud.stride == (1, 1, 1) and torch.equal(ud.coords.cpu(), torch.from_numpy(c))      # level-0 rows, in order
    assert key in xd.kmaps and (xd.kmaps[key].out_coords.cpu().numpy() == oc).all()
    err = float((ld.F.detach().cpu() - lr.F.detach()).abs().max())
    assert err < 1e-3, err
    grads = dict(ref.named_parameters())
    for name, p in net.named_parameters():
        want = grads[name].grad
        assert p.grad is not None and want is not None, name
        rel = float((p.grad.cpu().double() - want.double()).norm() / want.double().norm())
        assert rel < 5e-3, (name, rel)


# ------------------------------------------------------------------ 6. bf16 rows
def test_strided_k27_conv_bf16_rows(F):
    """(64, 64) on the k = 3, s = 2 map under bf16 autocast, down and transposed, at the tolerance
    tests/test_gpu_bf16_rows.py holds the k = 2, s = 2 pair to: 2^-7 of the tensor's magnitude against the fp32 oracle on the
    same bf16-rounded inputs."""
    tol = 2.0 ** -7
    c, oc, nbmaps, nbsizes = _scene_map(1)
    sizes = (len(c), len(oc))
    km = F.build_kmap(_dev(c), (1,) * 3, (3,) * 3, (2,) * 3)
    torch.manual_seed(128)
    r = lambda t: t.bfloat16().float()
    for transposed in (False, True):
        n_in, n_out = (sizes[1], sizes[0]) if transposed else sizes
        x = r(torch.randn(n_in, 64))
        w = r(torch.randn(27, 64, 64) / (27 * 64) ** 0.5)
        g = r(torch.randn(n_out, 64))
        want = R.conv_forward(x, w, nbmaps, nbsizes, sizes, transposed=transposed)
        wgi, wgw = R.conv_backward(x, w, g, nbmaps, nbsizes, transposed=transposed)
        xd, wd = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            assert F.bf16_rows()
            out = F.ConvolutionFunction.apply(xd, wd, km, transposed)
        assert out.dtype == torch.bfloat16 and bool(torch.isfinite(out.float()).all())
        assert _rel(out, want) < tol
        out.backward(g.cuda().bfloat16())
        assert xd.grad.dtype == torch.float32 and wd.grad.dtype == torch.float32
        assert _rel(xd.grad, wgi) < tol and _rel(wd.grad, wgw) < tol


# ------------------------------------------------------------------ 7. backend-format entries
@pytest.mark.parametrize('transposed', [False, True])
def test_v140_backend_format_entries_take_the_k3s2_rulebook(F, transposed):
    """u2mkd_convolution_forward / _backward with (nbmaps, nbsizes) = kmap[0], kmap[1] of a k = 3, s = 2 map against
    ConvolutionFunction on the same map, at the bound tests/test_gpu_torchsparse_ops.py holds these entries to (1e-4)."""
    from u2mkd_amd import _lib as L
    c, oc, _, _ = _scene_map(1)
    cin, cout, k = 32, 64, 27
    torch.manual_seed(3)
    km = F.build_kmap(_dev(c), (1,) * 3, (3,) * 3, (2,) * 3)
    nb_dev, nbsizes, sizes = km[0].contiguous(), km[1].cpu().tolist(), km[2]
    assert sizes == (len(c), len(oc)) and nb_dev.shape == (sum(nbsizes), 2) and nb_dev.dtype == torch.int32
    n_in, n_out = (sizes[1], sizes[0]) if transposed else sizes
    xd = torch.randn(n_in, cin, device='cuda')
    wd = torch.randn(k, cin, cout, device='cuda') / (k * cin) ** 0.5
    gd = torch.randn(n_out, cout, device='cuda')
    xa, wa = xd.clone().requires_grad_(True), wd.clone().requires_grad_(True)
    want = F.ConvolutionFunction.apply(xa, wa, km, transposed)
    want.backward(gd)
    sizes_host = (ctypes.c_int32 * k)(*nbsizes)
    lib = L.load()
    nbytes = lib.u2mkd_convolution_workspace_bytes(n_in, n_out, cin, cout, sizes_host, k)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    out = torch.full((n_out, cout), float('nan'), device='cuda')
    L.call('u2mkd_convolution_forward', L.ptr(xd), n_in, cin, L.ptr(out), n_out, cout, L.ptr(wd), L.ptr(nb_dev),
           ctypes.addressof(sizes_host), k, int(transposed), L.ptr(ws), nbytes, L.stream())
    assert _rel(out, want.detach()) < 1e-4
    gi = torch.full((n_in, cin), float('nan'), device='cuda')
    gw = torch.full((k, cin, cout), float('nan'), device='cuda')
    L.call('u2mkd_convolution_backward', L.ptr(xd), n_in, cin, L.ptr(gi), L.ptr(gd), n_out, cout, L.ptr(wd), L.ptr(gw),
           L.ptr(nb_dev), ctypes.addressof(sizes_host), k, int(transposed), L.ptr(ws), nbytes, L.stream())
    assert _rel(gi, xa.grad) < 1e-4 and _rel(gw, wa.grad) < 1e-4
