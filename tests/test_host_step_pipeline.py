"""train.NextBatch -- the next-batch prefetch protocol of LidarStep and KDStep -- driven without a GPU: recorder stubs stand in
for streams, events and tensors, a three-slice toy generator for the geometry.  Every stub appends to ONE list, and the test
holds that list, for each trainer's configuration of the object and each mode it offers, to a literal written from the
trainers' bodies BEFORE the object existed (commit 2332682, `train.py` line numbers in the comments below).  Two departures
from those bodies are deliberate and marked `PERMITTED 1 / 2` where they occur:
  1. `entry` is recorded only by calls that start a side-stream preparation (KDStep recorded it on every CUDA call, :380);
  2. LidarStep records `entry` in front of the wait on the previous `_geo_done`, as KDStep always did (:380-382), not behind
     it (:152,:163).
Log entries: ('record_event' | 'wait_event', stream role, event number in creation order), ('slice', stream role, k, grad
mode), ('record_stream', reader's role, tensor name), ('hook', entry, geo_done, after_bwd), ('forward',), ('backward',)."""
import contextlib

import pytest
import torch

from u2mkd_amd import deferred, kd as KD, train as T


class _Event:
    def __init__(self, n):
        self.n = n


class _Stream:
    def __init__(self, role, rec):
        self.role, self.rec = role, rec

    def record_event(self):
        ev = _Event(self.rec.events)
        self.rec.events += 1
        self.rec.log.append(('record_event', self.role, ev.n))
        return ev

    def wait_event(self, ev):
        self.rec.log.append(('wait_event', self.role, ev.n))

    def wait_stream(self, other):
        self.rec.log.append(('wait_stream', self.role, other.role))


class _Tensor(torch.Tensor):
    """A host tensor that says it lives on the device (train._tensors_of yields device tensors only) and records its readers."""
    is_cuda = True

    def record_stream(self, stream):
        self.rec.log.append(('record_stream', stream.role, self.tag))


class _Recorder:
    def __init__(self, monkeypatch):
        self.log, self.events = [], 0
        self.streams = {r: _Stream(r, self) for r in ('main', 'geo', 'teacher', 'camera')}
        self.current = self.streams['main']
        monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a: self.current)
        monkeypatch.setattr(torch.cuda, 'stream', self._on)
        monkeypatch.setattr(KD, '_side_stream', lambda ref, role: self.streams[role])

    @contextlib.contextmanager
    def _on(self, stream):
        before, self.current = self.current, stream
        try:
            yield
        finally:
            self.current = before

    def tensor(self, name):
        t = torch.zeros(1).as_subclass(_Tensor)
        t.rec, t.tag = self, name
        return t

    def slices(self, in_mod, attach):
        """The toy preparation: three slices, each logging the stream and the grad mode it runs under."""
        for k in (1, 2, 3):
            self.log.append(('slice', self.current.role, k, torch.is_grad_enabled()))
            if k < 3:
                yield
        attach(in_mod)
        return in_mod

    def take(self):
        out, self.log = self.log, []
        return out


class _Ref:
    is_cuda = True


def _lidar(rec, cls=T.NextBatch):
    """The object as LidarStep.__init__ configures it: one reader (the caller's stream), the geometry pair walked."""
    def attach(nxt):
        nxt['_geometry'] = (rec.tensor(nxt['name'] + '.z'), rec.tensor(nxt['name'] + '.x0'))
    return cls(T._Amp(False), lambda b: {'name': b[0]}, lambda nxt: rec.slices(nxt, attach), T.LidarStep._roots, T.LidarStep._readers)


def _kd(rec, cls=T.NextBatch, hook=True):
    """The object as KDStep.__init__ configures it: three readers, [_geometry, masks] of student and teacher walked, the
    behind-the-backward form offered, a hook."""
    def attach(nxt):
        nxt['student']['_geometry'] = (rec.tensor(nxt['name'] + '.s_geo'),)
        nxt['teacher']['_geometry'] = (rec.tensor(nxt['name'] + '.t_geo'),)

    def in_mod_of(b):
        return {'name': b['name'], 'student': {'masks': [rec.tensor(b['name'] + '.s_mask')]}, 'teacher': {}}

    def teacher_ahead(nxt, entry, geo_done, after_bwd):
        rec.log.append(('hook', entry.n, geo_done.n, after_bwd.n if after_bwd is not None else None))
    return cls(T._Amp(False), in_mod_of, lambda nxt: rec.slices(nxt, attach), T.KDStep._roots, T.KDStep._readers,
               behind_backward=True, hook=teacher_ahead if hook else None)


def _step(rec, pipe, batch, prefetch, after_bwd=False):
    """The five phases in the order both trainers' ``__call__`` run them; no phase may leak a stream or no_grad context."""
    def clean():
        assert rec.current is rec.streams['main'] and torch.is_grad_enabled()
    in_mod = pipe.begin(batch, prefetch, _Ref())
    pipe.start()
    clean()
    rec.log.append(('forward',))
    pipe.before_backward()
    clean()
    rec.log.append(('backward',))
    ev = torch.cuda.current_stream().record_event() if after_bwd and pipe.mode == 'slices' else None
    pipe.after_step(in_mod, *([ev] if pipe.hook is not None else []))
    clean()
    return in_mod


def _three_calls(rec, pipe, batches, prefetch=True):
    """Two consecutive calls with ``prefetch=`` and a third without; each call's log, and that every call after the first ran
    on the in_mod the call before it had queued."""
    logs, queued = [], None
    for i, b in enumerate(batches):
        nxt = batches[i + 1] if (prefetch and i + 1 < len(batches)) else None
        in_mod = _step(rec, pipe, b, nxt)
        if queued is not None:
            assert in_mod is queued
        queued = pipe._queued[1] if pipe._queued is not None else None
        assert (queued is not None) == (nxt is not None)
        logs.append(rec.take())
    assert pipe._geo_done is None
    return logs


def _streams(readers, names):
    return [('record_stream', r, n) for n in names for r in readers]


FWD, BWD = ('forward',), ('backward',)
ON_GEO = [('slice', 'geo', k, False) for k in (1, 2, 3)]
ON_MAIN = [('slice', 'main', k, False) for k in (1, 2, 3)]
ALL3 = ('main', 'teacher', 'camera')

# LidarStep, slices (train.py:148-185)
LIDAR_SLICES = [
    [('record_event', 'main', 0), ('wait_event', 'geo', 0), ON_GEO[0],                  # :163 entry, :165, :169 slice 1
     FWD, ON_GEO[1], BWD, ON_GEO[2],                                                      # :171, :176, :177, :179
     ('record_event', 'geo', 1)] + _streams(['main'], ['b1.z', 'b1.x0']),               # :181 _geo_done, :183-184
    [('record_event', 'main', 2), ('wait_event', 'main', 1),                            # PERMITTED 2 (the parent: :152 then :163)
     ('wait_event', 'geo', 2), ON_GEO[0], FWD, ON_GEO[1], BWD, ON_GEO[2],
     ('record_event', 'geo', 3)] + _streams(['main'], ['b2.z', 'b2.x0']),
    [('wait_event', 'main', 3), FWD, BWD],                                              # :149-153: also with prefetch=None
]
# LidarStep, inline (U2MKD_STAGED_GEOMETRY=0; :186-195): the whole preparation on the caller's stream in front of the backward
LIDAR_INLINE = [[FWD] + ON_MAIN + [BWD], [FWD] + ON_MAIN + [BWD], [FWD, BWD]]
NONE = [[FWD, BWD]] * 3                                                                  # (KDStep: PERMITTED 1, no :380 record)

# KDStep, slices (train.py:378-419)
KD_SLICES = [
    [('record_event', 'main', 0), ('wait_event', 'geo', 0), ON_GEO[0],                  # :380 entry, :392, :394 slice 1
     FWD, ON_GEO[1], BWD, ON_GEO[2],                                                      # :396, :400, :401, :404
     ('record_event', 'geo', 1), ('hook', 0, 1, None)]                                  # :406 _geo_done, :411
    + _streams(ALL3, ['b1.s_geo', 'b1.s_mask']) + _streams(ALL3, ['b1.t_geo']),          # :412-418
    [('record_event', 'main', 2), ('wait_event', 'main', 1),                            # :380, :382
     ('wait_event', 'geo', 2), ON_GEO[0], FWD, ON_GEO[1], BWD, ON_GEO[2],
     ('record_event', 'geo', 3), ('hook', 2, 3, None)]
    + _streams(ALL3, ['b2.s_geo', 'b2.s_mask']) + _streams(ALL3, ['b2.t_geo']),
    [('wait_event', 'main', 3), FWD, BWD],                                              # PERMITTED 1 (the parent: :380 first); :382
]
# KDStep, behind the backward (U2MKD_STAGED_GEOMETRY=0; :420-446): no hook in this form
KD_BEHIND = [
    [('record_event', 'main', 0), FWD, BWD, ('wait_event', 'geo', 0)] + ON_GEO          # :380, :429, :432, :433-434
    + [('record_event', 'geo', 1)]                                                      # :435
    + _streams(ALL3, ['b1.s_geo', 'b1.s_mask']) + _streams(ALL3, ['b1.t_geo']),          # :440-445
    [('record_event', 'main', 2), ('wait_event', 'main', 1), FWD, BWD, ('wait_event', 'geo', 2)] + ON_GEO
    + [('record_event', 'geo', 3)]
    + _streams(ALL3, ['b2.s_geo', 'b2.s_mask']) + _streams(ALL3, ['b2.t_geo']),
    [('wait_event', 'main', 3), FWD, BWD],                                              # PERMITTED 1; :382
]
# KDStep, inline (reduced precision: deferred.overlap_ok() is False; :447-452).  PERMITTED 1: no :380 record in any call
KD_INLINE = LIDAR_INLINE

LIDAR_BATCHES = [('b0', 'c0'), ('b1', 'c1'), ('b2', 'c2')]
KD_BATCHES = [{'name': 'b%d' % i} for i in range(3)]


def _case(monkeypatch, name, cls=T.NextBatch):
    """(logs of the three calls, expected) of one trainer in one mode."""
    rec = _Recorder(monkeypatch)
    trainer, mode = name.split('-')
    monkeypatch.setenv('U2MKD_STAGED_GEOMETRY', '1' if mode == 'slices' else '0')
    monkeypatch.setattr(deferred, '_REDUCED', [trainer == 'kd' and mode == 'inline'])
    pipe, batches = (_lidar(rec, cls), LIDAR_BATCHES) if trainer == 'lidar' else (_kd(rec, cls), KD_BATCHES)
    logs = _three_calls(rec, pipe, batches, prefetch=mode != 'none')
    assert pipe.mode == 'none'                                     # (the last call's)
    return logs, EXPECTED[name]


EXPECTED = {'lidar-slices': LIDAR_SLICES, 'lidar-inline': LIDAR_INLINE, 'lidar-none': NONE,
            'kd-slices': KD_SLICES, 'kd-behind_backward': KD_BEHIND, 'kd-inline': KD_INLINE, 'kd-none': NONE}


def _check(monkeypatch, cls=T.NextBatch):
    for name in EXPECTED:
        logs, want = _case(monkeypatch, name, cls)
        for i, (got, exp) in enumerate(zip(logs, want)):
            assert got == exp, (name, 'call %d' % (i + 1), got, exp)


@pytest.mark.parametrize('name', list(EXPECTED))
def test_every_mode_of_both_trainers_issues_the_parents_operations(monkeypatch, name):
    logs, want = _case(monkeypatch, name)
    for i, (got, exp) in enumerate(zip(logs, want)):
        assert got == exp, ('call %d' % (i + 1), got, exp)


def test_the_mode_is_what_the_parents_conditions_chose(monkeypatch):
    """train.py:158 / :385 / :420 / :447 of the parent, as one function."""
    for staged in ('0', '1'):
        monkeypatch.setenv('U2MKD_STAGED_GEOMETRY', staged)
        for reduced in (False, True):
            monkeypatch.setattr(deferred, '_REDUCED', [reduced])
            for cuda in (False, True):
                for offers in (False, True):
                    assert T._prefetch_mode(None, cuda, offers) == 'none'
                    side = cuda and not reduced
                    want = 'slices' if side and staged == '1' else 'behind_backward' if side and offers else 'inline'
                    assert T._prefetch_mode(object(), cuda, offers) == want, (staged, reduced, cuda, offers)


def test_a_batch_that_is_not_the_queued_object_is_not_taken_from_the_queue(monkeypatch):
    monkeypatch.setenv('U2MKD_STAGED_GEOMETRY', '1')
    rec = _Recorder(monkeypatch)
    pipe = _kd(rec)
    _step(rec, pipe, KD_BATCHES[0], KD_BATCHES[1])
    queued = pipe._queued[1]
    rec.take()
    in_mod = _step(rec, pipe, dict(KD_BATCHES[1]), None)          # equal, not identical
    assert in_mod is not queued and '_geometry' not in in_mod['student'] and pipe._queued is None
    assert rec.take() == [('wait_event', 'main', 1), FWD, BWD]     # the previous call's geometry stream is waited for all the same
    # LidarStep's batch arrives in parts: both must be the queued objects
    rec = _Recorder(monkeypatch)
    pipe = _lidar(rec)
    _step(rec, pipe, LIDAR_BATCHES[0], LIDAR_BATCHES[1])
    queued = pipe._queued[1]
    assert _step(rec, pipe, (LIDAR_BATCHES[1][0], 'c1 of another batch'), None) is not queued
    rec = _Recorder(monkeypatch)
    pipe = _lidar(rec)
    _step(rec, pipe, LIDAR_BATCHES[0], LIDAR_BATCHES[1])
    queued = pipe._queued[1]
    assert _step(rec, pipe, tuple(LIDAR_BATCHES[1]), None) is queued


def test_the_hook_runs_behind_slice_3_with_entry_geo_done_after_bwd(monkeypatch):
    """KDStep with U2MKD_TEACHER_AHEAD=2 (train.py:403-411): `after_bwd` is recorded between the optimizer step and slice 3,
    and the hook receives (entry, _geo_done, after_bwd) once `_geo_done` is recorded, in front of the reader registration."""
    monkeypatch.setenv('U2MKD_STAGED_GEOMETRY', '1')
    rec = _Recorder(monkeypatch)
    pipe = _kd(rec)
    _step(rec, pipe, KD_BATCHES[0], KD_BATCHES[1], after_bwd=True)
    log = rec.take()
    at = log.index(BWD)
    assert log[at:at + 5] == [BWD, ('record_event', 'main', 1), ON_GEO[2], ('record_event', 'geo', 2), ('hook', 0, 2, 1)]
    assert all(e[0] == 'record_stream' for e in log[at + 5:]) and len(log) == at + 5 + 9
    # the one-piece form behind the backward never ran it (:420-446)
    monkeypatch.setenv('U2MKD_STAGED_GEOMETRY', '0')
    rec = _Recorder(monkeypatch)
    _step(rec, _kd(rec), KD_BATCHES[0], KD_BATCHES[1], after_bwd=True)
    assert not [e for e in rec.take() if e[0] == 'hook']


class _NoWaitWithoutPrefetch(T.NextBatch):
    """the wait on `_geo_done` inside the prefetching branch only."""
    def begin(self, batch, prefetch, ref):
        if prefetch is None:
            self._geo_done = None
        return super().begin(batch, prefetch, ref)


class _DoneBeforeSlice3(T.NextBatch):
    """`_geo_done` recorded in front of the last slice: the next forward would read kernel maps still being built."""
    def after_step(self, in_mod, *hook_args):
        if self.mode != 'slices':
            return super().after_step(in_mod, *hook_args)
        early = self._geo.record_event()
        self._geo.record_event = lambda: early          # (what after_step records behind slice 3 is this event)
        try:
            super().after_step(in_mod, *hook_args)
        finally:
            del self._geo.record_event


class _OneReaderFewer(T.NextBatch):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        readers = self.readers
        self.readers = lambda ref: readers(ref)[:-1]


class _NoEntryWait(T.NextBatch):
    """The geometry stream starts without waiting for `entry`."""
    def _geo_stream(self):
        self._geo = KD._side_stream(self._ref, 'geo')


MUTANTS = [_NoWaitWithoutPrefetch, _DoneBeforeSlice3, _OneReaderFewer, _NoEntryWait]


@pytest.mark.parametrize('cls', MUTANTS, ids=lambda c: c.__name__)
def test_each_broken_protocol_fails_the_operation_lists(monkeypatch, cls):
    _check(monkeypatch)                    # the lists hold for the object itself ...
    with pytest.raises(AssertionError):    # ... and not for the mutant
        _check(monkeypatch, cls)
    # and it is the slices mode of BOTH trainers that catches it
    for name in ('lidar-slices', 'kd-slices'):
        logs, want = _case(monkeypatch, name, cls)
        assert logs != want, name
