"""The loader's geometry on the device (csrc/prep.hip): raw samples (``LCNuScenesDataset.raw``) -> the device batch of
``train.kd_batch_to_device(collated_to_kd_batch(collate_fn([ds[i] ...])))``, same keys, dtypes, shapes and layout.

The loader workers only read files, decode images and draw random numbers; the main process uploads the raw arrays as
they are (one upload per array kind and batch: float32 points, int64 labels, float64 matrices, int32 tables, uint8 images)
and HIP kernels do the rest on the caller's current stream: sweep aggregation with a stable compaction, rotate / scale /
flip, voxelisation, the LiDAR -> camera projections, the first-point voxel sets and every gather by ``inds``.  The arithmetic
is numpy's, operation for operation (NOTES N30), so the batch equals the loader's wherever BLAS sums in the written order.

Sizes the schema needs as Python ints (points and voxels per sample) and the key-range flag come back in ONE host read per
call (``post_counts`` / ``wait_counts``): every buffer is allocated at its upper bound and cut to size afterwards.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib as L
from ..torchsparse.nn import functional as spf

__all__ = ['prepare_kd_batch', 'prepare_lidar_batch', 'MAX_BATCH']

MAX_BATCH = 64             # samples per call (the voxel key keeps 7 bits for the sample index)
_CAM_STRIDE = 60           # doubles per (sample, camera): 4 x (R[9], t[3]), K[9], im_w - 1, im_h - 1, pad
_INT32_MAX = 2 ** 31 - 1


def _require_device(device):
    dev = torch.device(device)
    if dev.type != 'cuda':
        L.require_cuda(torch.empty(0))           # raises: there is no CPU fallback
    L.load()                                     # raises when the library is missing
    return dev


def _up(a, dev, keep):
    # (`keep`: the host array stays referenced until the call's host read has seen the stream pass every upload)
    keep.append(torch.from_numpy(np.ascontiguousarray(a)))
    return keep[-1].to(dev, non_blocking=True)


class _Uploaded:
    """The raw arrays of a batch on the device: one upload per array kind."""

    def __init__(self, raws, dev, cameras):
        nb, self._host = len(raws), []
        if not 1 <= nb <= MAX_BATCH:
            raise ValueError('device_prep: 1 to %d samples per batch, got %d' % (MAX_BATCH, nb))
        r0 = raws[0]
        for key in ('train', 'multisweeps', 'voxel_size', 'ignore_index'):
            if any(r[key] != r0[key] for r in raws):
                raise ValueError('device_prep: samples of one batch must share `%s`' % key)
        if not isinstance(r0['voxel_size'], (int, float)):
            raise NotImplementedError('device_prep: per-axis voxel sizes are not served')
        self.nb, self.train, self.sweeps = nb, bool(r0['train']), r0['multisweeps'] != 0
        self.voxel_size, self.ignore = float(r0['voxel_size']), int(r0['ignore_index'])
        nks = [int(r['points'].shape[0]) for r in raws]
        self.nk = sum(nks)
        kseg = np.cumsum([0] + nks)
        # sweep tables: point offsets per sample (mseg) and per sweep (sseg), both into the batch's sweep points
        sw = [r['sweeps'] for r in raws] if self.sweeps else []
        ms = [int(s['points'].shape[0]) for s in sw] or [0] * nb
        self.m = sum(ms)
        mseg = np.cumsum([0] + ms)
        sseg = np.concatenate([[0]] + [s['seg'][1:].astype(np.int64) + mseg[b] for b, s in enumerate(sw)]) if sw else np.zeros(1, np.int64)
        self.n_sweeps = int(sseg.shape[0] - 1)
        # float32: key-frame points, then the sweep points
        f32 = np.concatenate([r['points'] for r in raws] + [s['points'] for s in sw], axis=0).astype(np.float32, copy=False)
        self.f32 = _up(f32.reshape(-1, 4), dev, self._host)
        self.labels = _up(np.concatenate([r['labels'] for r in raws]).astype(np.int64, copy=False), dev, self._host)
        # float64: teacher (rot, scale) [nb,10], student [nb,10], sweep transforms [n_sweeps,16], cameras [nb,ncam,60]
        par = lambda side: np.concatenate([np.concatenate([np.asarray(r[side]['rot'], np.float64).reshape(9), [float(r[side]['scale'])]])
                                           for r in raws])
        parts = [par('teacher'), par('student'), np.concatenate([s['tm'].reshape(-1) for s in sw]) if sw else np.zeros(0)]
        self.ncam = 0
        if cameras:
            self.ncam = len(r0['cams'])
            if self.ncam < 1 or any(len(r['cams']) != self.ncam for r in raws):
                raise ValueError('device_prep: every sample of a batch needs the same number (>= 1) of cameras')
            cam = np.zeros((nb, self.ncam, _CAM_STRIDE))
            for b, r in enumerate(raws):
                for c, cm in enumerate(r['cams']):
                    for k, (rot, t) in enumerate(cm['steps']):
                        cam[b, c, 12 * k:12 * k + 9] = np.asarray(rot, np.float64).reshape(9)
                        cam[b, c, 12 * k + 9:12 * k + 12] = t
                    cam[b, c, 48:57] = np.asarray(cm['K'], np.float64).reshape(9)
                    cam[b, c, 57], cam[b, c, 58] = cm['size'][0] - 1.0, cm['size'][1] - 1.0
            parts.append(cam.reshape(-1))
        f64 = _up(np.concatenate(parts).astype(np.float64, copy=False), dev, self._host)
        cut = np.cumsum([0] + [p.shape[0] for p in parts])
        self.par_t, self.par_s, self.tm = (f64[cut[i]:cut[i + 1]] for i in range(3))
        self.cam = f64[cut[3]:cut[4]] if cameras else None
        # int32: kseg, mseg, sseg, the teacher's flip kinds, zeros (the student's)
        tables = [kseg, mseg, sseg, [int(r['teacher']['flip']) for r in raws], np.zeros(nb + 1), np.zeros(1)]
        # a voting batch (nuscenes_lc.VoteBatch: copy v of scan s is sample s * num_vote + v): the scans' key-frame point
        # offsets in the voted output ride in the same upload
        self.num_vote = getattr(raws, 'num_vote', None)
        if self.num_vote:
            nv = self.num_vote
            if nb % nv or any(nks[b] != nks[b - b % nv] or raws[b].get('lidar_token') != raws[b - b % nv].get('lidar_token')
                              for b in range(nb)):
                raise ValueError('device_prep: a voting batch holds %d copies of every scan, each with the same key-frame points' % nv)
            self.scan_nk, self.kseg_host = nks[::nv], [int(k) for k in kseg]
            tables.append(np.cumsum([0] + self.scan_nk))
        i32 = _up(np.concatenate([np.asarray(t, np.int64) for t in tables]).astype(np.int32), dev, self._host)
        cut = np.cumsum([0] + [len(t) for t in tables])
        self.kseg, self.mseg, self.sseg, self.flip, self.zeros, self.zero = (i32[cut[i]:cut[i + 1]] for i in range(6))
        self.scan_seg = i32[cut[6]:cut[7]] if self.num_vote else None
        self.tokens = [r.get('lidar_token') for r in raws]
        self.images = _up(np.stack([r['images'] for r in raws]), dev, self._host) if cameras else None
        self.dev = dev

    @property
    def key_points(self):
        return self.f32[:self.nk]

    @property
    def sweep_points(self):
        return self.f32[self.nk:]


class _Side:
    """One network input's points on their way to a voxel set: everything at its upper bound ``cap``."""


def _points(u, teacher):
    """Aggregate (teacher with sweeps), augment and voxelise: the per-point arrays and the per-sample minima."""
    dev, nb = u.dev, u.nb
    st = _Side()
    m = u.m if teacher else 0
    st.cap = cap = u.nk + m
    st.feats = torch.empty(cap, 4, dtype=torch.float32, device=dev)
    st.vox = torch.empty(cap, 4, dtype=torch.int32, device=dev)
    st.mn = torch.full((nb, 3), _INT32_MAX, dtype=torch.int32, device=dev)
    st.counts = torch.zeros(2 * (nb + 1) + 1, dtype=torch.int32, device=dev)       # point offsets, voxel offsets, range flag
    st.off, st.voxoff, st.err = st.counts[:nb + 1], st.counts[nb + 1:2 * nb + 2], st.counts[2 * nb + 2:]
    with_mask = teacher and u.sweeps
    st.labels = torch.empty(cap, dtype=torch.int64, device=dev) if with_mask else u.labels
    st.kf = torch.empty(cap, dtype=torch.bool, device=dev) if with_mask else None
    ws = pos = None
    if m:
        ws = torch.empty(L.load().u2mkd_prep_scan_workspace_bytes(m), dtype=torch.uint8, device=dev)
        pos = torch.empty(m + 1, dtype=torch.int32, device=dev)
        L.call('u2mkd_prep_sweep_compact', L.ptr(u.sweep_points), m, L.ptr(ws), L.ptr(pos), L.stream())
    f32mode = 0 if (teacher and u.sweeps) else 1         # the teacher's points are float64 iff multisweeps != 0
    L.call('u2mkd_prep_points', L.ptr(u.key_points), L.ptr(u.labels), u.nk, L.ptr(u.sweep_points) if m else None, m, L.ptr(ws),
           L.ptr(pos) if m else L.ptr(u.zero), L.ptr(u.kseg), L.ptr(u.mseg) if m else L.ptr(u.zeros), L.ptr(u.sseg), u.n_sweeps,
           L.ptr(u.tm) if m else None, nb, L.ptr(u.par_t if teacher else u.par_s), L.ptr(u.flip if teacher else u.zeros),
           int(u.train), f32mode, u.voxel_size, u.ignore, L.ptr(st.feats), L.ptr(st.vox), L.ptr(st.labels) if with_mask else None,
           L.ptr(st.kf), L.ptr(st.mn), L.ptr(st.off), L.stream())
    return st


def _voxel_sets(u, st, cams=None):
    """Keys -> stable sort (torch) -> head flags, scan, inds, inverse map and the gathers (one launch)."""
    dev, nb, cap = u.dev, u.nb, st.cap
    keys = torch.empty(cap, dtype=torch.int64, device=dev)
    L.call('u2mkd_prep_voxel_keys', L.ptr(st.vox), L.ptr(st.mn), L.ptr(st.off), nb, cap, L.ptr(keys), L.ptr(st.err), L.stream())
    skeys, perm = torch.sort(keys, stable=True)
    new = lambda *shape, dtype: torch.empty(*shape, dtype=dtype, device=dev)
    st.inverse_map, st.inds = new(cap, dtype=torch.int64), new(cap, dtype=torch.int64)
    st.feats_o, st.coords_o, st.labels_o = new(cap, 4, dtype=torch.float32), new(cap, 4, dtype=torch.int32), new(cap, dtype=torch.int64)
    st.kf_o = new(cap, dtype=torch.bool) if st.kf is not None else None
    st.fov_o = st.masks_o = st.pc_o = None
    pwi = masks = pc = None
    if cams is not None:
        pwi, masks, pc = cams
        st.fov_o, st.masks_o, st.pc_o = new(cap, dtype=torch.bool), new(u.ncam * cap, dtype=torch.bool), new(u.ncam * cap, 2, dtype=torch.float32)
    ws = new(L.load().u2mkd_prep_scan_workspace_bytes(cap), dtype=torch.uint8)
    rank = new(cap + 1, dtype=torch.int32)
    L.call('u2mkd_prep_voxel_sets', L.ptr(skeys), L.ptr(perm), cap, L.ptr(ws), L.ptr(rank), L.ptr(st.off), nb, L.ptr(st.feats),
           L.ptr(st.vox), L.ptr(st.mn), L.ptr(st.labels), L.ptr(st.kf), L.ptr(pwi), L.ptr(masks), L.ptr(pc), u.ncam, u.nk,
           L.ptr(st.inverse_map), L.ptr(st.inds), L.ptr(st.feats_o), L.ptr(st.coords_o), L.ptr(st.labels_o), L.ptr(st.kf_o),
           L.ptr(st.fov_o), L.ptr(st.masks_o), L.ptr(st.pc_o), L.ptr(st.voxoff), L.stream())


def _project(u):
    pc = torch.empty(u.ncam, u.nk, 2, dtype=torch.float32, device=u.dev)
    masks = torch.empty(u.ncam, u.nk, dtype=torch.bool, device=u.dev)
    pwi = torch.empty(u.nk, dtype=torch.bool, device=u.dev)
    L.call('u2mkd_prep_project', L.ptr(u.key_points), u.nk, L.ptr(u.kseg), u.nb, u.ncam, L.ptr(u.cam), L.ptr(pc), L.ptr(masks),
           L.ptr(pwi), L.stream())
    return pwi, masks, pc


def _read(u, sides):
    """THE host read of a call: every side's point offsets, voxel offsets and range flag."""
    values = spf.wait_counts(spf.post_counts([s.counts[i:i + 1] for s in sides for i in range(s.counts.shape[0])]))
    out, at = [], 0
    for s in sides:
        n = s.counts.shape[0]
        v = values[at:at + n]
        at += n
        if v[-1]:
            bits = [L.load().u2mkd_prep_key_bits(a) for a in range(3)]
            raise ValueError('device_prep: a voxel coordinate span does not fit the sort key (x, y, z: %d, %d, %d bits)' % tuple(bits))
        out.append((v[:u.nb + 1], v[u.nb + 1:2 * u.nb + 2]))
    return out


def _sample_of(offsets, n, dev):
    """[n] int64: the sample of every row, from host-known offsets."""
    sizes = [b - a for a, b in zip(offsets[:-1], offsets[1:])]
    rows = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)
    assert rows.shape[0] == n
    return torch.from_numpy(rows).to(dev)


def _vote_tables(u, st, inverse_map):
    """The tables ``evaluate.vote_point_predictions`` takes for the network input ``st`` of a voting batch: views of the
    counts the kernels wrote (``off`` / ``voxoff``: every copy's first point and first voxel row) and the uploaded
    ``scan_seg``; the targets are vote 0's key-frame labels of every scan.  Everything stays on the device."""
    nv, k = u.num_vote, u.kseg_host
    firsts = range(0, u.nb, nv)
    targets = [u.labels[k[b]:k[b + 1]] for b in firsts]
    return {'num_vote': nv, 'copy_point_off': st.off[:u.nb], 'copy_voxel_off': st.voxoff[:u.nb], 'scan_seg': u.scan_seg,
            'inverse_map': inverse_map, 'targets': targets[0] if len(targets) == 1 else torch.cat(targets),
            'num_pts': list(u.scan_nk), 'lidar_tokens': [u.tokens[b] for b in firsts]}


def prepare_kd_batch(raws, device='cuda', with_eval=False):
    """Raw samples (``LCNuScenesDataset.raw``; a ``raw_collate_fn`` batch) -> the device batch ``train.KDStep`` takes, on the
    current stream.  ``with_eval``: also the tensors of the eval branch (run_training.kd_eval_feed) as a second dict.
    A ``VoteBatch`` (``VoteView``'s collate) additionally gets ``'vote'``: the student input's voting tables."""
    dev = _require_device(device)
    u = _Uploaded(raws, dev, cameras=True)
    tea = _points(u, teacher=True)
    stu = _points(u, teacher=False)
    cams = _project(u)
    _voxel_sets(u, tea)
    _voxel_sets(u, stu, cams)
    images = u.images.permute(0, 1, 4, 2, 3).float().contiguous()          # uint8 [B,ncam,H,W,3] -> f32 [B,ncam,3,H,W]
    (t_off, t_vox), (s_off, s_vox) = _read(u, [tea, stu])
    nb, ncam = u.nb, u.ncam
    nvt, nvs, npt = t_vox[nb], s_vox[nb], t_off[nb]
    cut = lambda t, off, b, scale=1: t[scale * off[b]:scale * off[b + 1]]
    nv = [s_vox[b + 1] - s_vox[b] for b in range(nb)]
    out = {
        's_feats': stu.feats_o[:nvs], 's_coords': stu.coords_o[:nvs], 'targets': stu.labels_o[:nvs], 'images': images,
        'pixel_coordinates': [cut(stu.pc_o, s_vox, b, ncam).view(ncam, nv[b], 2) for b in range(nb)],
        'masks': [cut(stu.masks_o, s_vox, b, ncam).view(ncam, nv[b]) for b in range(nb)],
        'fov_mask': stu.fov_o[:nvs], 'inds': [[cut(stu.inds, s_vox, b)] for b in range(nb)],
        't_feats': tea.feats_o[:nvt], 't_coords': tea.coords_o[:nvt], 'inverse_map': tea.inverse_map[:npt],
        'num_pts': [t_off[b + 1] - t_off[b] for b in range(nb)], 'num_vox_t': [t_vox[b + 1] - t_vox[b] for b in range(nb)],
        'keyframe_mask_full': tea.kf[:npt] if tea.kf is not None else None,
        'targets_t': tea.labels_o[:nvt],
    }
    if tea.kf_o is not None:
        out['keyframe_mask'] = tea.kf_o[:nvt]
    if u.num_vote:
        out['vote'] = _vote_tables(u, stu, stu.inverse_map[:u.nk])
    if not with_eval:
        return out
    ev = {'s_inverse_map': stu.inverse_map[:u.nk], 's_inverse_batch': _sample_of(s_off, u.nk, dev),
          'targets_mapped': stu.labels, 't_inverse_batch': _sample_of(t_off, npt, dev), 'targets_mapped_t': tea.labels[:npt]}
    ev['label_fov'] = ev['targets_mapped']
    return out, ev


def prepare_lidar_batch(raws, device='cuda'):
    """The teacher-only trainer's batch (``train.LidarStep`` and its ``evaluate``) from the same raw samples: the teacher
    half alone -- no projection, no images.  A ``VoteBatch`` additionally gets ``'vote'``: the teacher input's voting tables."""
    dev = _require_device(device)
    u = _Uploaded(raws, dev, cameras=False)
    tea = _points(u, teacher=True)
    _voxel_sets(u, tea)
    (t_off, t_vox), = _read(u, [tea])
    nb = u.nb
    nvt, npt = t_vox[nb], t_off[nb]
    out = {'feats': tea.feats_o[:nvt], 'coords': tea.coords_o[:nvt], 'targets': tea.labels_o[:nvt],
           'keyframe_mask': tea.kf_o[:nvt] if tea.kf_o is not None else None,
           'keyframe_mask_full': tea.kf[:npt] if tea.kf is not None else None,
           'inverse_map': tea.inverse_map[:npt], 'inverse_batch': _sample_of(t_off, npt, dev),
           'targets_mapped': tea.labels[:npt], 'num_pts': [t_off[b + 1] - t_off[b] for b in range(nb)],
           'num_vox': [t_vox[b + 1] - t_vox[b] for b in range(nb)]}
    if u.num_vote:
        out['vote'] = _vote_tables(u, tea, out['inverse_map'])
    return out
