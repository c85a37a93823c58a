"""A/B of the table-free window attention (csrc/sptr_plain.hip) against the contextual kernels (csrc/sptr.hip) on the SAME plans,
through the C ABI, at two sizes of the student: its first SphereFormer stage's cubic branch (stride-2 voxels of the 80 000-voxel
synthetic scene, window 0.3 m, windows of a few tokens, one lane per (token, head)) and its last stage's spherical branch
(stride-16 voxels, window (16 deg, 16 deg, 120 m), windows of hundreds, 16 lanes per (token, head)).

    python tools/ab_sptr_plain.py OUT.json [samples]

Per sample one version runs `BATCH` launches between two device events; the versions alternate sample by sample, the figure is
the median over the samples per launch.  From the plan: the pairs, the bytes the plain kernels read and write (rows of q, k, v,
dout, out, the gradients, lse / delta) and their floating-point operations, and with them the achieved rates against the MI355X
peaks (fp32 vector 157.3 TFLOP/s; HBM 8.0 TB/s spec, 6.29 TB/s measured copy rate -- most of these bytes are re-reads of rows of
the same window and hit the caches, so two byte counts are kept apart: the COMPULSORY bytes (every row read or written once:
what HBM has to move, the roofline's byte bound) and the REQUESTED bytes (every row a lane loads, window re-reads included: what
the caches serve; the L2 of the chip moves ~17-19 TB/s of rows shared by many workgroups)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from u2mkd_amd import _lib as L
from u2mkd_amd import sptr
from u2mkd_amd.lidar.sphereformer import cart2sphere
from u2mkd_amd.synth import synth_batch

BATCH = 5
PEAK_FLOPS, PEAK_BW_SPEC, PEAK_BW_COPY, L2_BW = 157.3e12, 8.0e12, 6.29e12, 17.0e12
# floating-point operations per (query, key, head) pair of the plain kernels (head dim 16; exp counted as one)
FWD_FLOP = 2 * 16 + 3 * 16 + 6                       # q . k, acc = acc * corr + p * v, the online-softmax scalars
BWD_FLOP = (4 * 16 + 2 * 16 + 4) + (16 + 4 * 16 + 4 * 16 + 4)      # query role: s, dp, dq; key role: q scale, s, dp, dk, dv


def stage_tokens(coords, stride):
    c = torch.from_numpy(coords.astype(np.int64))
    c[:, :3] = torch.div(c[:, :3], stride, rounding_mode='floor') * stride
    c = torch.unique(c, dim=0)
    return (c[:, :3].float() * 0.05).cuda(), c[:, 3].int().cuda()


def sample(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(BATCH):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / BATCH              # us per launch


def run_case(name, pts, batch, window, quant, split_a, h, S, samples):
    forced_before = os.environ.get('U2MKD_SPTR_SPLIT')
    os.environ['U2MKD_SPTR_SPLIT'] = str(S)              # (read by the library on every call; put back below)
    n, qgl = pts.shape[0], 24
    sphere = split_a > 0
    tl = 2 * qgl if sphere else 2 * qgl - 1
    plan = sptr.WindowPlan(pts, batch, window)
    qc, radial, span = plan.quant_coords(pts, quant, sphere)
    g = torch.Generator(device='cuda').manual_seed(1)
    rn = lambda *s: torch.randn(*s, device='cuda', generator=g)
    q, k, v, dout = rn(n, h, 16), rn(n, h, 16), rn(n, h, 16), rn(n, h, 16)
    tabs = [0.3 * rn(tl, 3, h, 16) for _ in range(3)]
    st = L.stream()
    ld = h * 16
    P = (L.ptr(plan.sort_idx), L.ptr(plan.wstart), L.ptr(plan.wlen))
    T = (L.ptr(qc), L.ptr(radial), L.ptr(tabs[0]), L.ptr(tabs[1]), L.ptr(tabs[2]), tl, qgl, float(split_a))
    res = {}
    for ver in ('contextual', 'plain'):
        res[ver] = dict(out=torch.empty(n, h, 16, device='cuda'), lse=torch.empty(n, h, device='cuda'),
                        delta=torch.empty(n, h, device='cuda'), grads=torch.empty(3, n, h, 16, device='cuda'))
    nbytes = L.load().u2mkd_sptr_backward_workspace_bytes(n, h, tl)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device='cuda')
    dtabs = [torch.empty_like(t) for t in tabs]
    scale = 0.25

    def fwd(ver):
        r = res[ver]
        if ver == 'plain':
            L.call('u2mkd_sptr_plain_forward_strided', L.ptr(q), L.ptr(k), L.ptr(v), ld, scale, *P, n, h, 16, L.ptr(r['out']), ld,
                   L.ptr(r['lse']), st)
        else:
            L.call('u2mkd_sptr_attention_forward_strided', L.ptr(q), L.ptr(k), L.ptr(v), ld, scale, *P, *T, n, h, 16, L.ptr(r['out']),
                   ld, L.ptr(r['lse']), st)

    def bwd(ver):
        r = res[ver]
        gq, gk, gv = r['grads'][0], r['grads'][1], r['grads'][2]
        if ver == 'plain':
            L.call('u2mkd_sptr_plain_backward_strided', L.ptr(q), L.ptr(k), L.ptr(v), ld, scale, L.ptr(r['out']), L.ptr(dout), ld,
                   L.ptr(r['lse']), *P, n, h, 16, L.ptr(r['delta']), L.ptr(gq), L.ptr(gk), L.ptr(gv), ld, st)
        else:
            L.call('u2mkd_sptr_attention_backward_strided', L.ptr(q), L.ptr(k), L.ptr(v), ld, scale, L.ptr(r['out']), L.ptr(dout), ld,
                   L.ptr(r['lse']), *P, *T, span, n, h, 16, L.ptr(r['delta']), L.ptr(ws), nbytes, L.ptr(gq), L.ptr(gk), L.ptr(gv), ld,
                   L.ptr(dtabs[0]), L.ptr(dtabs[1]), L.ptr(dtabs[2]), st)

    times = {(ver, d): [] for ver in res for d in ('fwd', 'bwd')}
    for ver in res:                                           # warm-up: every kernel of the timed window
        for _ in range(3):
            fwd(ver), bwd(ver)
    torch.cuda.synchronize()
    for _ in range(samples):
        for d, fn in (('fwd', fwd), ('bwd', bwd)):
            for ver in ('contextual', 'plain'):               # alternated
                times[(ver, d)].append(sample(lambda: fn(ver)))
    wl = plan.wlen.double()
    pairs = float(wl.sum())
    # bytes the plain kernels request: per (token, head) a q row + its window's k and v rows, out + lse written; backward both roles
    fwd_bytes = h * (n * (64 + 64 + 4) + pairs * 128)
    bwd_bytes = h * (n * (4 * 64 + 3 * 64 + 8) + pairs * (128 + 128 + 8)) + h * n * (128 + 4)        # + the delta pass
    fwd_once = h * n * (3 * 64 + 64 + 4)                      # q, k, v read, out and lse written, each once
    bwd_once = h * n * (5 * 64 + 3 * 64 + 3 * 4)              # q, k, v, out, dout read, dq, dk, dv written; lse, delta
    out = dict(case=name, tokens=n, heads=h, lanes_per_token=S, windows=int((plan.wstart == torch.arange(n, device='cuda')).sum()),
               window_len_mean=float(wl.mean()), window_len_max=int(wl.max()), pair_weighted_window_len=float((wl * wl).sum() / pairs),
               pairs=int(pairs), samples=samples, launches_per_sample=BATCH)
    for (ver, d), ts in times.items():
        ts = np.asarray(ts)
        out[f'{ver}_{d}_us'] = dict(median=round(float(np.median(ts)), 2), min=round(float(ts.min()), 2), max=round(float(ts.max()), 2))
    for d, by, once, fl in (('fwd', fwd_bytes, fwd_once, FWD_FLOP * pairs * h), ('bwd', bwd_bytes, bwd_once, BWD_FLOP * pairs * h)):
        t = out[f'plain_{d}_us']['median'] * 1e-6
        bound_flop, bound_bw = fl / PEAK_FLOPS, once / PEAK_BW_COPY
        least = max(bound_flop, bound_bw)
        out[f'plain_{d}'] = dict(requested_bytes=int(by), compulsory_bytes=int(once), flop=int(fl), requested_bytes_per_s=by / t,
                                 compulsory_bytes_per_s=once / t, flop_per_s=fl / t, share_of_fp32_vector_peak=fl / t / PEAK_FLOPS,
                                 compulsory_share_of_hbm_copy_rate=once / t / PEAK_BW_COPY, requested_share_of_l2_rate=by / t / L2_BW,
                                 least_time_us=least * 1e6, bound='bytes' if bound_bw > bound_flop else 'flop',
                                 share_of_least_time=least / t)
        out[f'contextual_over_plain_{d}'] = round(out[f'contextual_{d}_us']['median'] / out[f'plain_{d}_us']['median'], 3)
    # same plan, same q k v: with all-zero tables the two forwards must agree (the A/B measures the same function)
    for t in tabs:
        t.zero_()
    fwd('contextual'), fwd('plain')
    torch.cuda.synchronize()
    out['max_abs_diff_forward_with_zero_tables'] = float((res['contextual']['out'] - res['plain']['out']).abs().max())
    if forced_before is None:
        del os.environ['U2MKD_SPTR_SPLIT']
    else:
        os.environ['U2MKD_SPTR_SPLIT'] = forced_before
    print(json.dumps(out), flush=True)
    return out


def main():
    dst = sys.argv[1]
    samples = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    coords = synth_batch(80000, 1)['coords']
    results = []
    xyz, b = stage_tokens(coords, 2)
    results.append(run_case('cubic branch, first stage (stride 2)', xyz, b, np.array([0.3, 0.3, 0.3]), np.array([0.3 / 24] * 3), 0.0, 2, 1,
                            samples))
    results.append(run_case('cubic branch, first stage (stride 2), 2 lanes', xyz, b, np.array([0.3, 0.3, 0.3]), np.array([0.3 / 24] * 3),
                            0.0, 2, 2, samples))
    xyz, b = stage_tokens(coords, 16)
    sph = cart2sphere(xyz - xyz.mean(0))                      # (the sensor in the middle of the scene: windows of hundreds)
    win = np.array([16.0, 16.0, 120.0])
    results.append(run_case('spherical branch, last stage (stride 16)', sph, b, win, win / 24, 0.0125, 8, 16, samples))
    results.append(run_case('spherical branch, last stage (stride 16), 2 heads', sph, b, win, win / 24, 0.0125, 2, 16, samples))
    doc = dict(tool='tools/ab_sptr_plain.py', device=torch.cuda.get_device_name(0),
               peaks=dict(fp32_vector_flops=PEAK_FLOPS, hbm_spec=PEAK_BW_SPEC, hbm_copy_measured=PEAK_BW_COPY, l2_shared_rows=L2_BW),
               flop_per_pair_head=dict(forward=FWD_FLOP, backward=BWD_FLOP), cases=results)
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    with open(dst, 'w') as f:
        json.dump(doc, f, indent=1)


if __name__ == '__main__':
    main()
