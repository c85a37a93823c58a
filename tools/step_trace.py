"""What a pipelined training loop ISSUES, as one hashable log: every library launch (`_lib.call`: entry name + the role of the
current stream), every stream-ordering call (`Stream.record_event` / `wait_event` / `wait_stream`, events numbered by creation)
and the `Tensor.record_stream` registrations (counted per stream between two other operations).  Four steps with `prefetch=`
and a fifth without, at the shapes of tests/test_gpu_configs.py (KD: 3 000 points, 64 x 112 images) and
tests/test_gpu_spvcnn.py (SPVCNN cr 0.5, 9 000 points).  Run it on two checkouts and compare (NOTES N28):

  U2MKD_STAGED_GEOMETRY=1 python tools/step_trace.py kd --out a.pt          # or: lidar;  --amp bf16
  python tools/step_trace.py compare a.pt b.pt

`compare` wants equal NORMALISED logs (below), equal losses for `lidar` (SPVCNN is bit-reproducible) and bit-equal frozen-teacher
logits of every step for `kd`.  The normal form removes what N28 allows to differ between the hand-written steps and
train.NextBatch: `record_event`s of events nobody waits for (an unused `entry`), and the order of the adjacent `wait_event` /
`record_event` pair on one stream in front of a step's first launch (LidarStep's `entry` and its wait on the previous
`_geo_done`); events are then renumbered by first appearance."""
import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


class Trace:
    def __init__(self):
        from u2mkd_amd import _lib as L
        self.log, self.events, self.keep, self.pending, self.depth = [], {}, [], {}, 0
        real_call = L.call

        def call(name, *a):
            self.add(('call', name, self.role(torch.cuda.current_stream())))
            return real_call(name, *a)
        L.call = call
        S = torch.cuda.Stream
        for op in ('record_event', 'wait_event', 'wait_stream'):
            setattr(S, op, self.wrap(op, getattr(S, op)))
        real_rs = torch.Tensor.record_stream

        def record_stream(t, stream):
            r = self.role(stream)
            self.pending[r] = self.pending.get(r, 0) + 1
            return real_rs(t, stream)
        torch.Tensor.record_stream = record_stream

    def role(self, stream):
        from u2mkd_amd import deferred
        for (_, role), s in deferred._STREAMS.items():
            if s.cuda_stream == stream.cuda_stream:
                return role
        return 'main' if stream.cuda_stream == torch.cuda.default_stream().cuda_stream else 'other'

    def number(self, ev):
        if id(ev) not in self.events:
            self.events[id(ev)] = len(self.events)
            self.keep.append(ev)             # (alive: an id is never reused)
        return self.events[id(ev)]

    def add(self, entry):
        for r in sorted(self.pending):
            self.log.append(('record_stream', r, self.pending[r]))
        self.pending = {}
        self.log.append(entry)

    def wrap(self, op, real):
        def f(stream, *a):
            self.depth += 1                  # (torch's wait_stream is a record_event + a wait_event of its own: one entry)
            try:
                out = real(stream, *a)
            finally:
                self.depth -= 1
            if self.depth == 0:
                if op == 'record_event':
                    self.add((op, self.role(stream), self.number(out)))
                elif op == 'wait_event':
                    self.add((op, self.role(stream), self.number(a[0])))
                else:
                    self.add((op, self.role(stream), self.role(a[0])))
            return out
        return f


def normalised(log):
    log = list(log)
    at = 0
    while at < len(log):                     # the pair in front of a step's first launch: record_event first
        if log[at][0] == 'step':
            j = at + 1
            while j + 1 < len(log) and log[j][0] not in ('call', 'step'):
                a, b = log[j], log[j + 1]
                if a[0] == 'wait_event' and b[0] == 'record_event' and a[1] == b[1]:
                    log[j], log[j + 1] = b, a
                    j += 1
                j += 1
        at += 1
    waited = {e[2] for e in log if e[0] == 'wait_event'}
    log = [e for e in log if not (e[0] == 'record_event' and e[2] not in waited)]
    names = {}
    out = []
    for e in log:
        if e[0] in ('record_event', 'wait_event'):
            e = (e[0], e[1], names.setdefault(e[2], len(names)))
        out.append(e)
    return out


def digest(log):
    return hashlib.sha256('\n'.join(repr(e) for e in log).encode()).hexdigest()


def run_kd(trace, amp):
    from u2mkd_amd import kd as KD, lidar, train as T
    from u2mkd_amd.synth import synth_kd_batch
    torch.manual_seed(0)
    sp = {k: v for k, v in lidar.spformer_kwargs().items() if k not in ('cr', 'in_channel', 'num_classes')}
    model = KD.TSDFull(cr=1.0, cr_t=2.0, in_channel=4, in_channel_t=4, num_classes=17, spformer=sp).cuda()
    run = T.KDStep(model, num_epochs=50, batch_size=2, amp=amp)
    run.train_mode()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if hasattr(m, 'drop_prob'):
            m.drop_prob = 0.0
    batches = [T.kd_batch_to_device(synth_kd_batch(3000 + 500 * i, 1, seed=31 + i, image_hw=(64, 112))) for i in range(3)]
    watch = T.TeacherWatch(model.model_t)
    losses, cur = [], T.fresh_batch(batches[0])
    for i in range(5):
        nxt = T.fresh_batch(batches[(i + 1) % 3]) if i < 4 else None
        watch.key = i
        trace.add(('step', i))
        losses.append(run(cur, prefetch=nxt))
        cur = nxt
    torch.cuda.synchronize()
    return [float(x) for x in losses], [t.cpu() for _, t in watch.log]


def run_lidar(trace, amp):
    from u2mkd_amd import lidar, train as T
    from u2mkd_amd.synth import synth_batch
    bs = [synth_batch(9000 + 1000 * i, 1, seed=60 + i) for i in range(3)]
    bs = [tuple(torch.from_numpy(b[k]).cuda() for k in ('feats', 'coords', 'labels')) for b in bs]
    torch.manual_seed(0)
    model = lidar.SPVCNN(cr=0.5, in_channel=4, num_classes=17, pres=0.05, vres=0.05).cuda().train()
    model.dropout.p = 0.0
    run = T.LidarStep(model, num_epochs=1, batch_size=1, amp=amp)
    losses, cur = [], [t.clone() for t in bs[0]]
    for i in range(5):
        nxt = [t.clone() for t in bs[(i + 1) % 3]] if i < 4 else None
        trace.add(('step', i))
        losses.append(run(*cur, prefetch=(nxt[0], nxt[1]) if nxt else None))
        cur = nxt
    torch.cuda.synchronize()
    return [float(x) for x in losses], []


def compare(pa, pb):
    a, b = torch.load(pa, weights_only=False), torch.load(pb, weights_only=False)
    na, nb = normalised(a['log']), normalised(b['log'])
    ok = na == nb
    print('normalised log: %s %s | %s %s' % (digest(na)[:16], len(na), digest(nb)[:16], len(nb)), 'EQUAL' if ok else 'DIFFERENT')
    if not ok:
        for i, (x, y) in enumerate(zip(na, nb)):
            if x != y:
                print('  first difference at %d: %r | %r' % (i, x, y))
                break
    if a['what'] == 'lidar':
        same = a['losses'] == b['losses']
        print('losses', a['losses'], 'EQUAL' if same else 'DIFFERENT: %r' % (b['losses'],))
        ok = ok and same
    else:
        same = len(a['teacher']) == len(b['teacher']) and all(torch.equal(x, y) for x, y in zip(a['teacher'], b['teacher']))
        print('teacher logits of %d steps' % len(a['teacher']), 'BIT-EQUAL' if same else 'DIFFERENT')
        print('losses', a['losses'], b['losses'])
        ok = ok and same
    return 0 if ok else 1


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['kd', 'lidar', 'compare'])
    ap.add_argument('files', nargs='*')
    ap.add_argument('--amp', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.what == 'compare':
        sys.exit(compare(*args.files))
    trace = Trace()
    losses, teacher = (run_kd if args.what == 'kd' else run_lidar)(trace, args.amp or False)
    trace.add(('end',))
    log = trace.log
    norm = normalised(log)
    print('%s amp=%s staged=%s: %d launches, %d ordering calls, %d registrations; sha256 raw %s normalised %s' % (
        args.what, args.amp, os.environ.get('U2MKD_STAGED_GEOMETRY'), sum(e[0] == 'call' for e in log),
        sum(e[0] in ('record_event', 'wait_event', 'wait_stream') for e in log), sum(e[2] for e in log if e[0] == 'record_stream'),
        digest(log)[:16], digest(norm)[:16]))
    print('losses', losses)
    if args.out:
        torch.save({'what': args.what, 'log': log, 'losses': losses, 'teacher': teacher}, args.out)
