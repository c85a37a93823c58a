"""The loader's geometry, CPU against GPU, on a synthetic raw batch at the loader's real size (2 samples of 34 720 key-frame
points, 9 sweeps of the same size, 6 cameras at 360 x 640, voxel 0.05):

(a) what ``LCNuScenesDataset.__getitem__`` + ``collate_fn`` + ``collated_to_kd_batch`` + ``train.kd_batch_to_device`` cost with
    the file reads and the image decode taken out (arrays in memory, ONE process -- a DataLoader spreads this over its workers):
    ``loader_geometry`` below is ``__getitem__``'s numpy, line for line, on a raw sample;
(b) ``device_prep.prepare_kd_batch`` on the same raw samples: between two device events, and its host time.

Alternated, ``--samples`` each after ``--warmup`` (measuring-on-mi355x §5); median (min, p90) per leg, the bytes each path uploads
per batch, and a check that the two batches agree.  Needs the GPU: there is no CPU timing of (b).

    python tools/time_device_prep.py [--samples 20] [--warmup 3] [--points 34720] [--sweeps 9] [--out profiles/device_prep.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from u2mkd_amd import train as T  # noqa: E402
from u2mkd_amd.data import device_prep, nuscenes_lc as D  # noqa: E402
from u2mkd_amd.synth import synth_raw_sample  # noqa: E402
from u2mkd_amd.torchsparse import SparseTensor  # noqa: E402
from u2mkd_amd.torchsparse.utils.quantize import sparse_quantize  # noqa: E402


def _voxel_set(pts, labels, voxel_size):
    voxel = np.round(pts[:, :3] / voxel_size).astype(np.int32)
    voxel -= voxel.min(0, keepdims=1)
    feat = pts.astype(np.float32)
    _, inds, inverse_map = sparse_quantize(voxel, return_index=True, return_inverse=True)
    return voxel, feat, inds, inverse_map


def loader_geometry(raw):
    """``LCNuScenesDataset.__getitem__`` from the sample's arrays instead of its files (same numpy calls, same order)."""
    pts0, labels_raw, vs = raw['points'], raw['labels'], raw['voxel_size']
    # teacher (_process_unimodal_input)
    pts, labels_, keyframe_mask = pts0.copy(), labels_raw, None
    if raw['multisweeps'] != 0:
        sw, agg_pts, agg_ts = raw['sweeps'], [], []
        for k in range(sw['tm'].shape[0]):
            p = sw['points'][sw['seg'][k]:sw['seg'][k + 1]]
            close = np.logical_and(np.fabs(p[:, 0]) < 1.0, np.fabs(p[:, 1]) < 1.0)
            p = p[~close]
            xyz = np.dot(sw['tm'][k], np.vstack((p[:, :3].T, np.ones(p.shape[0]))))[:3, :]
            agg_ts.append(sw['lag'][k] * np.ones((p.shape[0],)))
            agg_pts.append(np.concatenate([xyz.T, p[:, 3].reshape(-1, 1)], axis=-1))
        agg_ts = np.concatenate([np.zeros(shape=(pts.shape[0],))] + agg_ts, axis=0)
        pts = np.concatenate([pts] + agg_pts, axis=0)
        keyframe_mask = (agg_ts == 0)
        extra = int(np.sum(~keyframe_mask))
        labels_ = np.concatenate([labels_, np.full((extra,), raw['ignore_index'], dtype=labels_.dtype)], axis=0)
    if raw['train']:
        out = np.zeros_like(pts)
        out[:, :3] = np.dot(pts[:, :3], raw['teacher']['rot']) * raw['teacher']['scale']
        out[:, 3] = pts[:, 3]
        pts = out
        kind = raw['teacher']['flip']
        if kind in (1, 3):
            pts[:, 0] = -pts[:, 0]
        if kind in (2, 3):
            pts[:, 1] = -pts[:, 1]
    voxel, feat, inds, inverse_map = _voxel_set(pts, labels_, vs)
    voxel_full = voxel[inds]
    fd_t = {'lidar': SparseTensor(feat[inds], voxel_full), 'targets': SparseTensor(labels_[inds], voxel_full),
            'targets_mapped': SparseTensor(labels_, voxel), 'inverse_map': SparseTensor(inverse_map, voxel),
            'num_vox': voxel_full.shape[0], 'num_pts': voxel.shape[0]}
    if keyframe_mask is not None:
        fd_t['keyframe_mask'] = SparseTensor(keyframe_mask[inds], voxel_full)
        fd_t['keyframe_mask_full'] = SparseTensor(keyframe_mask, voxel)
    # cameras
    pixel_coordinates, masks = [], []
    valid = np.full(pts0.shape[0], -1)
    for idx, cam in enumerate(raw['cams']):
        (r1, t1), (r2, t2), (r3, t3), (r4, t4) = cam['steps']
        p = pts0[:, :3].T.astype(np.float64)
        p = r1.dot(p) + t1[:, None]
        p = r2.dot(p) + t2[:, None]
        p = r3.T.dot(p - t3[:, None])
        p = r4.T.dot(p - t4[:, None])
        mask = p[2, :] > 1
        with np.errstate(divide='ignore', invalid='ignore'):
            p = np.dot(cam['K'], p)
            p = p / p[2:3, :]
        uv = p[:2, :]
        uv[0, :] = uv[0, :] / (cam['size'][0] - 1.0) * 2.0 - 1.0
        uv[1, :] = uv[1, :] / (cam['size'][1] - 1.0) * 2.0 - 1.0
        mask = mask & (uv[0, :] > -1) & (uv[0, :] < 1) & (uv[1, :] > -1) & (uv[1, :] < 1)
        valid[mask] = idx
        masks.append(mask)
        pixel_coordinates.append(uv.T)
    pt_with_img = valid != -1
    pixel_coordinates, masks = np.stack(pixel_coordinates, axis=0), np.stack(masks, axis=0)
    # student
    pts_cp = np.zeros_like(pts0)
    if raw['train']:
        pts_cp[:, :3] = np.dot(pts0[:, :3], raw['student']['rot']) * raw['student']['scale']
    else:
        pts_cp[...] = pts0[...]
    pts_cp[:, 3] = pts0[:, 3]
    voxel, feat, inds, inverse_map = _voxel_set(pts_cp, labels_raw, vs)
    voxel_full = voxel[inds]
    fd_s = {'lidar': SparseTensor(feat[inds], voxel_full), 'targets': SparseTensor(labels_raw[inds], voxel_full),
            'targets_mapped': SparseTensor(labels_raw, voxel), 'inverse_map': SparseTensor(inverse_map, voxel),
            'images': raw['images'], 'pixel_coordinates': pixel_coordinates[:, inds, :], 'masks': masks[:, inds],
            'fov_mask': SparseTensor(pt_with_img[inds], voxel_full), 'inds': [inds], 'num_vox': voxel_full.shape[0]}
    return {'feed_dict_s': fd_s, 'feed_dict_t': fd_t, 'lidar_token': raw['lidar_token']}


def _nbytes(v):
    if isinstance(v, np.ndarray):
        return v.nbytes
    if isinstance(v, dict):
        return sum(_nbytes(x) for x in v.values())
    if isinstance(v, (list, tuple)):
        return sum(_nbytes(x) for x in v)
    return 0


def stats(ms):
    s = sorted(ms)
    return {'median_ms': round(float(np.median(s)), 3), 'min_ms': round(s[0], 3), 'p90_ms': round(s[min(len(s) - 1, int(0.9 * len(s)))], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--points', type=int, default=34720)
    ap.add_argument('--sweeps', type=int, default=9)
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'device_prep.json'))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_device_prep.py times the GPU path: no GPU is visible')
    raws = [synth_raw_sample(opt.points, [opt.points] * opt.sweeps, seed=100 + b, image_hw=(360, 640)) for b in range(opt.batch)]

    def cpu_path():
        numpy_batch = D.collated_to_kd_batch(D.collate_fn([loader_geometry(r) for r in raws]))
        d = T.kd_batch_to_device(numpy_batch)
        torch.cuda.synchronize()
        return d, numpy_batch

    def gpu_path():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        d = device_prep.prepare_kd_batch(raws)
        e1.record()
        host = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        return d, host, e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    legs = {'cpu_geometry_collate_upload': [], 'device_prep_events': [], 'device_prep_host': [], 'device_prep_wall': []}
    for i in range(opt.warmup + opt.samples):
        t0 = time.perf_counter()
        d_cpu, numpy_batch = cpu_path()
        t_cpu = (time.perf_counter() - t0) * 1e3
        d_gpu, host, events, wall = gpu_path()
        if i >= opt.warmup:
            legs['cpu_geometry_collate_upload'].append(t_cpu)
            legs['device_prep_events'].append(events)
            legs['device_prep_host'].append(host)
            legs['device_prep_wall'].append(wall)
    # the two batches: equal sizes; integer tensors equal and floats within 1 ulp wherever BLAS summed in the written order
    same = d_cpu['num_pts'] == d_gpu['num_pts'] and d_cpu['num_vox_t'] == d_gpu['num_vox_t']
    same = same and all(torch.equal(d_cpu[k], d_gpu[k]) for k in ('s_coords', 't_coords', 'targets', 'inverse_map', 'fov_mask'))
    worst = max(float((d_cpu[k] - d_gpu[k]).abs().max()) for k in ('s_feats', 't_feats'))
    result = {'config': {'batch': opt.batch, 'key_points': opt.points, 'sweeps': opt.sweeps, 'cameras': 6, 'image_hw': [360, 640],
                         'voxel_size': 0.05, 'samples': opt.samples, 'warmup': opt.warmup, 'device': torch.cuda.get_device_name(0),
                         'teacher_points': d_gpu['num_pts'], 'teacher_voxels': d_gpu['num_vox_t']},
              'legs': {k: stats(v) for k, v in legs.items()},
              'bytes_uploaded_per_batch': {'cpu_path': _nbytes(numpy_batch),
                                           'device_prep': sum(t.numel() * t.element_size() for t in device_prep._Uploaded(raws, torch.device('cuda'), True)._host)},
              'batches_agree': {'integers_equal': bool(same), 'worst_abs_feature_difference': worst}}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
