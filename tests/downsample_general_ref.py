"""numpy restatement of the general branch of torchsparse v1.4.0's ``F.spdownsample`` (some stride[a] neither 1 nor
kernel_size[a]: k = 3, s = 2), written as the literal repeat + mask + unique it runs.  Shared by the host test and the GPU test."""
import numpy as np

from oracle import ts_ref as R


def kept_candidates(coords, stride, kernel_size, tensor_stride):
    """(candidates int64 [K, n, 4] as (x, y, z, b), kept bool [K, n]): every input row plus every kernel offset, and which of
    them the branch keeps -- on every axis a multiple of stride * tensor_stride (Python remainder: negative multiples count) and
    not below that axis's minimum over ALL rows."""
    stride, kernel_size, tensor_stride = (R.make_ntuple(v) for v in (stride, kernel_size, tensor_stride))
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, 4)
    offsets = R.get_kernel_offsets(kernel_size, tensor_stride).astype(np.int64)
    ss = np.asarray([stride[a] * tensor_stride[a] for a in range(3)], dtype=np.int64)
    cmin = coords[:, :3].min(0)
    cand = np.repeat(coords[None], len(offsets), 0)
    cand[:, :, :3] += offsets[:, None, :]
    kept = ((cand[:, :, :3] % ss == 0) & (cand[:, :, :3] >= cmin)).all(-1)
    return cand, kept


def ref_spdownsample_general(coords, stride, kernel_size, tensor_stride):
    """int32 [n_out, 4] (x, y, z, b): the distinct kept candidates sorted by (b, x, y, z)."""
    coords = np.asarray(coords).reshape(-1, 4)
    if len(coords) == 0:
        return np.zeros((0, 4), dtype=np.int32)
    cand, kept = kept_candidates(coords, stride, kernel_size, tensor_stride)
    rows = cand[kept]
    if len(rows) == 0:
        return np.zeros((0, 4), dtype=np.int32)
    u = np.unique(rows[:, [3, 0, 1, 2]], axis=0)
    return np.ascontiguousarray(u[:, [1, 2, 3, 0]]).astype(np.int32)


def max_candidates_per_row(stride, kernel_size):
    """M = prod_a ceil(kernel_size[a] / stride[a])"""
    stride, kernel_size = R.make_ntuple(stride), R.make_ntuple(kernel_size)
    m = 1
    for a in range(3):
        m *= -(-kernel_size[a] // stride[a])
    return m
