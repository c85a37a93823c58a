"""The specification of the device loader path (u2mkd_amd/data/device_prep.py, csrc/prep.hip) in numpy.

``prepare_numpy(raw)`` does to one raw sample (``LCNuScenesDataset.raw``) what ``__getitem__`` does, with every
floating-point operation written out ELEMENTWISE in the order of the arithmetic rule (NOTES N30): one IEEE multiply, add or
divide per numpy call -- numpy's elementwise kernels do not contract -- and no ``np.dot`` / ``@`` on point arrays, whose BLAS
summation order is not defined.  The device is held to this bit for bit; the loader agrees with it up to that summation
order.  It also returns every point's MARGIN: the smallest relative distance of a pre-decision value to its decision (the
fraction of p / voxel_size to .5; depth to 1; u and v to +-1) -- a fixture whose margins are not tiny cannot flip a
decision over a last-bit difference.

``collate(samples)`` stacks such samples into the numpy KD batch of ``nuscenes_lc.collated_to_kd_batch``.
"""
import numpy as np

KEY_BITS = (20, 20, 16)


def _rows3(m, x, y, z):
    """[((m[r][0] x + m[r][1] y) + m[r][2] z) for r in 0..2]"""
    return [((m[r][0] * x + m[r][1] * y) + m[r][2] * z) for r in range(3)]


def _cols3(m, x, y, z):
    """[((x m[0][c] + y m[1][c]) + z m[2][c]) for c in 0..2]"""
    return [((x * m[0][c] + y * m[1][c]) + z * m[2][c]) for c in range(3)]


def _aggregate(raw):
    """Key-frame points promoted to double, then the kept sweep points: (f64 [N', 4], key-frame mask, labels)."""
    pts, labels, sw = raw['points'], raw['labels'], raw['sweeps']
    rows, n_added = [pts.astype(np.float64)], 0
    for k in range(sw['tm'].shape[0]):
        p = sw['points'][sw['seg'][k]:sw['seg'][k + 1]]
        close = np.logical_and(np.fabs(p[:, 0]) < np.float32(1.0), np.fabs(p[:, 1]) < np.float32(1.0))
        p = p[~close]
        tm = sw['tm'][k]
        x, y, z = (p[:, c].astype(np.float64) for c in range(3))
        out = [((x * tm[r][0] + y * tm[r][1]) + z * tm[r][2]) + tm[r][3] for r in range(3)]
        rows.append(np.stack(out + [p[:, 3].astype(np.float64)], axis=1))
        n_added += p.shape[0]
    allp = np.concatenate(rows, axis=0)
    kf = np.concatenate([np.ones(pts.shape[0], bool), np.zeros(n_added, bool)])      # lag is never 0 for a real sweep
    lab = np.concatenate([labels, np.full(n_added, raw['ignore_index'], dtype=labels.dtype)])
    return allp, kf, lab


def _augment_voxelise(p, rot, scale, flip, train, voxel_size):
    """p [N,4] in the loader's dtype (float32 or float64) -> (feats f32, voxel int32 with its minimum subtracted, margin)."""
    dt = p.dtype
    if train:
        x, y, z = (p[:, c].astype(np.float64) for c in range(3))
        o = [(v * scale).astype(dt) for v in _cols3(rot, x, y, z)]           # (float32 points: rounded once, `zeros_like(pts)`)
        if flip in (1, 3):
            o[0] = -o[0]
        if flip in (2, 3):
            o[1] = -o[1]
    else:
        o = [p[:, c] for c in range(3)]
    q = [v / dt.type(voxel_size) for v in o]                                 # in the points' dtype
    assert all(v.dtype == dt for v in q)
    vox = np.stack([np.round(v) for v in q], axis=1).astype(np.int32)        # np.round: half to even
    frac = [np.abs((v - np.floor(v)) - dt.type(0.5)) / np.maximum(np.abs(v), dt.type(1.0)) for v in q]
    margin = np.minimum(np.minimum(frac[0], frac[1]), frac[2]).astype(np.float64)
    if vox.shape[0]:
        vox = vox - vox.min(0, keepdims=True)
    feats = np.stack(o + [p[:, 3]], axis=1).astype(np.float32)
    return feats, vox, margin


def _quantize(vox):
    """First point of every voxel, voxels in (x, y, z) lexicographic order: (inds, inverse_map)."""
    v = vox.astype(np.int64)
    for a in range(3):
        if v.shape[0] and int(v[:, a].max()) >= (1 << KEY_BITS[a]):
            raise ValueError('axis %d does not fit the sort key' % a)
    key = ((v[:, 0] << KEY_BITS[1] | v[:, 1]) << KEY_BITS[2]) | v[:, 2]
    _, inds, inverse = np.unique(key, return_index=True, return_inverse=True)
    return inds.astype(np.int64), inverse.reshape(-1).astype(np.int64)


def _project(pts, cam):
    """One camera: (uv f64 [N,2], mask [N], margin [N])."""
    x, y, z = (pts[:, c].astype(np.float64) for c in range(3))
    with np.errstate(all='ignore'):
        for k in (0, 1):
            rot, t = cam['steps'][k]
            x, y, z = [v + t[r] for r, v in enumerate(_rows3(rot, x, y, z))]
        for k in (2, 3):
            rot, t = cam['steps'][k]
            x, y, z = _rows3(rot.T, x - t[0], y - t[1], z - t[2])
        mask0 = z > 1
        kx, ky, kz = _rows3(cam['K'], x, y, z)
        u = (kx / kz) / (cam['size'][0] - 1.0) * 2.0 - 1.0
        v = (ky / kz) / (cam['size'][1] - 1.0) * 2.0 - 1.0
        mask = mask0 & (u > -1) & (u < 1) & (v > -1) & (v < 1)
        m = np.abs(z - 1.0)
        for w in (u, v):
            d = np.minimum(np.abs(w + 1.0), np.abs(w - 1.0))
            m = np.where(mask0 & np.isfinite(d), np.minimum(m, d), m)        # (behind the camera only the depth decides)
    return np.stack([u, v], axis=1), mask, m


def prepare_numpy(raw):
    pts, labels, train, vs = raw['points'], raw['labels'], raw['train'], raw['voxel_size']
    # teacher
    if raw['multisweeps'] != 0:
        tp, kf, tl = _aggregate(raw)
    else:
        tp, kf, tl = pts, None, labels
    t = raw['teacher']
    feats, vox, t_margin = _augment_voxelise(tp, t['rot'], t['scale'], t['flip'], train, vs)
    inds, inverse = _quantize(vox)
    teacher = {'feats': feats[inds], 'coords': vox[inds], 'targets': tl[inds], 'inverse_map': inverse, 'targets_mapped': tl,
               'num_pts': int(vox.shape[0]), 'num_vox': int(inds.shape[0])}
    if kf is not None:
        teacher['keyframe_mask'], teacher['keyframe_mask_full'] = kf[inds], kf
    # cameras
    n = pts.shape[0]
    uvs, masks, c_margin = [], [], np.full(n, np.inf)
    for cam in raw['cams']:
        uv, mask, m = _project(pts, cam)
        uvs.append(uv); masks.append(mask)
        c_margin = np.minimum(c_margin, m)
    masks = np.stack(masks, 0)
    pc = np.stack(uvs, 0)
    pt_with_img = masks.any(0)
    # student
    s = raw['student']
    feats, vox, s_margin = _augment_voxelise(pts, s['rot'], s['scale'], 0, train, vs)
    inds, inverse = _quantize(vox)
    student = {'feats': feats[inds], 'coords': vox[inds], 'targets': labels[inds], 'images': raw['images'],
               'pixel_coordinates': pc[:, inds, :].astype(np.float32), 'masks': masks[:, inds], 'fov_mask': pt_with_img[inds],
               'inds': inds, 'num_vox': int(inds.shape[0]), 'inverse_map': inverse, 'targets_mapped': labels}
    margin = min(float(t_margin.min()) if t_margin.size else np.inf, float(s_margin.min()) if s_margin.size else np.inf,
                 float(c_margin.min()) if n else np.inf)
    return {'student': student, 'teacher': teacher, 'margin': margin,
            'margins': {'teacher': t_margin, 'student': s_margin, 'cameras': c_margin}}


def collate(samples):
    """-> the numpy batch of ``collated_to_kd_batch(collate_fn([...]))``."""
    def coords(side):
        return np.concatenate([np.concatenate([x[side]['coords'], np.full((x[side]['coords'].shape[0], 1), b, np.int32)], 1)
                               for b, x in enumerate(samples)]).astype(np.int32)
    cat = lambda side, key, dt: np.concatenate([x[side][key] for x in samples]).astype(dt)
    student = {'coords': coords('student'), 'feats': cat('student', 'feats', np.float32), 'targets': cat('student', 'targets', np.int64),
               'images': np.stack([x['student']['images'] for x in samples]).astype(np.float32),
               'pixel_coordinates': [x['student']['pixel_coordinates'] for x in samples],
               'masks': [x['student']['masks'] for x in samples], 'fov_mask': cat('student', 'fov_mask', bool),
               'inds': [[x['student']['inds']] for x in samples], 'num_vox': [x['student']['num_vox'] for x in samples]}
    teacher = {'coords': coords('teacher'), 'feats': cat('teacher', 'feats', np.float32), 'targets': cat('teacher', 'targets', np.int64),
               'inverse_map': cat('teacher', 'inverse_map', np.int64), 'num_pts': [x['teacher']['num_pts'] for x in samples],
               'num_vox': [x['teacher']['num_vox'] for x in samples]}
    if 'keyframe_mask_full' in samples[0]['teacher']:
        teacher['keyframe_mask_full'] = cat('teacher', 'keyframe_mask_full', bool)
        teacher['keyframe_mask'] = cat('teacher', 'keyframe_mask', bool)
    return {'student': student, 'teacher': teacher}


def eval_feed(samples):
    """The eval-branch tensors of ``run_training.kd_eval_feed`` as numpy arrays."""
    batch_of = lambda side: np.concatenate([np.full(x[side]['inverse_map'].shape[0], b, np.int64) for b, x in enumerate(samples)])
    cat = lambda side, key: np.concatenate([x[side][key] for x in samples]).astype(np.int64)
    out = {'s_inverse_map': cat('student', 'inverse_map'), 's_inverse_batch': batch_of('student'),
           'targets_mapped': cat('student', 'targets_mapped'), 't_inverse_batch': batch_of('teacher'),
           'targets_mapped_t': cat('teacher', 'targets_mapped')}
    out['label_fov'] = out['targets_mapped']
    return out
