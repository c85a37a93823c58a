"""The optimizer of the shipped configurations -- ``torch.optim.SGD(lr, momentum=0.9, weight_decay=1e-4, nesterov=True)``
(core/builder.py:663-669, configs/nuscenes/default.yaml:18-23) -- with its update over all parameters of a group as ONE HIP
launch (csrc/optim.hip) instead of torch's multi-tensor path (~40 launches behind ~3.5 ms of host-side list handling per KD
step, plus ~2 ms of ``zero_grad``), in a step that is bound by the host.  Same class hierarchy, same ``param_groups`` /
``state`` / ``state_dict`` layout (``momentum_buffer`` per parameter: views of one flat buffer per group), same global step
hooks, and bit-identical parameters after every step (tests/test_gpu_optim.py): the kernel applies torch's five element-wise
operations in torch's order with torch's roundings.  Whatever the fused path does not cover (CPU parameters, dampening,
maximize, sparse or non-fp32 gradients, tensor learning rates) runs torch's own step.

Under fp16 autocast (the reference's amp mode) a ``torch.amp.GradScaler`` drives the optimizer.  ``FusedSGD`` speaks the
protocol of torch's fused optimizers (``_step_supports_amp_scaling``: the scaler hands over ``grad_scale`` / ``found_inf`` as
device tensors and calls ``step()`` unconditionally), and the kernel (``u2mkd_sgd_batch_amp``) unscales and decides on the
device whether anything is written -- the host read of torch's generic route (``GradScaler._maybe_opt_step``:
``found_inf.item()``) is gone.  ``GradScaler`` here is ``torch.amp.GradScaler`` with its unscale-and-check over a FusedSGD's
gradients as one launch per group (``u2mkd_grads_unscale_check``) instead of torch's multi-tensor launches; a plain
``torch.amp.GradScaler`` works as well.  Only a step in which a parameter has its first gradient (its momentum buffer does
not exist yet, and torch creates it only in a step that is applied) reads ``found_inf`` on the host.

``FusedAdam`` / ``FusedAdamW`` are ``torch.optim.Adam`` / ``torch.optim.AdamW`` (make_optimizer's `adam`, `adamw`,
`adamw_spformer`: core/builder.py:670-718) the same way, on the same machinery (the mixin ``_Fused``): one launch per group
(``u2mkd_adam_batch``), torch's ``param_groups`` and ``state`` layout (``step`` a CPU fp32 scalar, ``exp_avg`` / ``exp_avg_sq``
views of one flat buffer per moment and group), bit-identical parameters, moments and step counts
(tests/test_gpu_optim_adamw.py).  The bias corrections are computed on the host as torch computes them (``adam_scalars``) and ride
behind the job rows in the same upload.  Under a GradScaler (``u2mkd_adam_batch_amp``) a skipped step does not advance a
parameter's ``step``, and only the device knows which steps were skipped: it keeps a count of applied steps, the host learns it
late through a pinned ring it only polls, and sends the scalars of every count the device could be at -- the kernel picks its
row (``StepLedger``).  No step of a steady run reads anything back; ``state[p]['step']`` follows as the
outcomes arrive, exact after ``sync_steps()`` (which ``state_dict()`` and ``load_state_dict()`` call).  State entries come into
being at a parameter's first gradient whether or not that step is applied (zero moments, step 0), as with torch's
``fused=True`` Adam and unlike its unfused route.  ``U2MKD_FUSED_ADAM=0`` forces torch's own step."""
from __future__ import annotations

import os

import numpy as np
import torch

from torch.amp.grad_scaler import _MultiDeviceReplicator

from . import _lib as L

__all__ = ['FusedSGD', 'FusedAdam', 'FusedAdamW', 'GradScaler', 'StepLedger', 'adam_scalars']

_ENABLED = os.environ.get('U2MKD_FUSED_SGD', '1') != '0'      # 0: torch's own step (A/B runs)
_ADAM_ENABLED = os.environ.get('U2MKD_FUSED_ADAM', '1') != '0'      # 0: torch's own Adam / AdamW step (A/B runs)
_RING = 4
_COUNT_RING = 8                        # read-backs of the device's count of applied steps in flight (FusedAdam under a scaler)


class _Group:
    """Static part of one parameter group's job table."""

    def __init__(self, params, chunk, moments=1, extra=0):
        """``moments``: flat state buffers per group (SGD: the momentum; Adam: exp_avg and exp_avg_sq); ``extra``: int64 words
        per job behind the job rows in the staging buffers and the device table (Adam's per-job step scalars)."""
        self.params = params
        self.ptrs = [p.data_ptr() for p in params]
        dev = params[0].device
        self.device = dev
        numel = [p.numel() for p in params]
        chunks = [(n + chunk - 1) // chunk for n in numel]
        first = np.concatenate([[0], np.cumsum(chunks)]).astype(np.int64)
        self.total_chunks = int(first[-1])
        offs = np.concatenate([[0], np.cumsum([(n + 3) // 4 * 4 for n in numel])]).astype(np.int64)       # (16-byte aligned views)
        self.flat = torch.zeros(int(offs[-1]), dtype=torch.float32, device=dev)
        self.bufs = [self.flat[int(offs[i]):int(offs[i]) + numel[i]].view_as(p) for i, p in enumerate(params)]
        if moments == 2:
            self.flat2 = torch.zeros_like(self.flat)
            self.bufs2 = [self.flat2[int(offs[i]):int(offs[i]) + numel[i]].view_as(p) for i, p in enumerate(params)]
        self.has_buf = [False] * len(params)
        self.first_col = np.ones(len(params), dtype=np.int64)      # 1: no momentum buffer yet
        self.missing = len(params)
        n = len(params)
        self.stage = [torch.zeros(n * (6 + extra), dtype=torch.int64).pin_memory() for _ in range(_RING)]
        self.tabs = [s[:n * 6].view(n, 6).numpy() for s in self.stage]
        self.floats = [s[n * 6:].view(torch.float32).numpy() for s in self.stage]
        for t in self.tabs:
            t[:, 0] = self.ptrs
            t[:, 2] = [b.data_ptr() for b in self.bufs]
            t[:, 3] = numel
            t[:, 4] = first[:-1]
            t[:, 5] = 1
        self.events = [None] * _RING
        self.table = torch.zeros(n * (6 + extra), dtype=torch.int64, device=dev)
        self.turn = 0
        self.uploaded = None               # (stream, gradient pointers, first-use column) of the table on the device


class _Fused:
    """What the fused optimizers share, in front of torch's class in the hierarchy (``_torch_cls``): the per-group job tables and
    their staging ring, the upload, the plan, the scaler's check launch, the fast ``zero_grad`` and torch's own step for whatever
    the kernels do not cover.  A subclass gives ``_eligible(group)``, ``_make_group(params)`` and ``step``."""
    _step_supports_amp_scaling = True     # torch.amp.GradScaler.step: sets grad_scale / found_inf and calls step() unconditionally
    _torch_cls = None

    def _init_fused(self):
        self._fused_groups = {}
        self._adopt = True
        self._chunk = None

    def _make_group(self, params):
        return _Group(params, self._chunk)

    # ------------------------------------------------------------------ torch.optim.Optimizer surface
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._adopt = True               # (the loaded momentum buffers are new tensors: copied into the flat buffers at the next step)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, '_fused_groups'):
            self._fused_groups.clear()
            self._adopt = True

    def zero_grad(self, set_to_none: bool = True):
        if not set_to_none:
            return super().zero_grad(set_to_none=False)
        for group in self.param_groups:
            for p in group['params']:
                p.grad = None

    # ------------------------------------------------------------------ the job tables
    def _fused(self, gi, group):
        """The group's job table, rebuilt when its parameter list or a parameter's storage changed; None if a parameter is not
        a contiguous fp32 tensor on one HIP device."""
        ps = group['params']
        fg = self._fused_groups.get(gi)
        if fg is None or fg.params_list is not ps or len(fg.params) != len(ps) or fg.ptrs != [p.data_ptr() for p in ps]:
            dev = ps[0].device
            if dev.type != 'cuda' or not all(p.dtype == torch.float32 and p.device == dev and p.is_contiguous() for p in ps):
                return None
            if self._chunk is None:
                self._chunk = int(L.load().u2mkd_sgd_chunk_elements())
            fg = self._fused_groups[gi] = self._make_group(list(ps))
            fg.params_list = ps
            self._adopt = True
        return fg

    def _plan(self):
        """[(group, its job table, its gradients)] if every group can take the fused path, else None."""
        if not all(self._eligible(g) for g in self.param_groups):
            return None
        plans = []
        f32 = torch.float32
        for gi, group in enumerate(self.param_groups):
            fg = self._fused(gi, group)
            if fg is None:
                return None
            grads = [p.grad for p in fg.params]
            if any(g is not None and (g.dtype is not f32 or g.is_sparse or not g.is_contiguous()) for g in grads):
                return None
            plans.append((group, fg, grads))
        return plans

    def _scaler_scalars(self):
        """A GradScaler's two device scalars (torch.amp.GradScaler.step sets them around step(), as for torch's fused optimizers)."""
        grad_scale, found_inf = getattr(self, 'grad_scale', None), getattr(self, 'found_inf', None)
        if not isinstance(found_inf, torch.Tensor):
            # (no parameter had a gradient: torch's scaler hands over sum([]) = the int 0 -- no check ran, nothing to skip or apply)
            grad_scale = found_inf = None
        return grad_scale, found_inf

    def _upload(self, fg, grads, extra=None):
        """This step's job table on the device (the gradients' addresses and the first-use flags change from step to step); a
        table that the scaler's check of this very step sent -- same gradients, same stream -- is not sent again (step() forgets it
        at its end: without a scaler every step sends its table, as before).  ``extra``: a float32 array that goes behind the job
        rows in the same staging buffer and the same copy (Adam's per-job step scalars)."""
        key = (L.stream(), [0 if g is None else g.data_ptr() for g in grads], fg.first_col.tobytes()) \
            + (() if extra is None else (extra.tobytes(),))
        if fg.uploaded == key:
            return
        slot = fg.turn % _RING
        fg.turn += 1
        ev = fg.events[slot]
        if ev is not None and not ev.query():
            ev.synchronize()              # (the host is a whole ring ahead of the copy that reads this staging buffer)
        tab = fg.tabs[slot]
        tab[:, 1] = key[1]
        tab[:, 5] = fg.first_col
        if extra is None:
            fg.table.copy_(fg.stage[slot], non_blocking=True)
        else:
            fg.floats[slot][:extra.size] = extra.ravel()
            used = 6 * len(fg.params) + (extra.size + 1) // 2
            fg.table[:used].copy_(fg.stage[slot][:used], non_blocking=True)
        if ev is None:
            ev = fg.events[slot] = torch.cuda.Event()
        ev.record()
        fg.uploaded = key

    @staticmethod
    def _scalar_on(t, device):
        """A GradScaler's scalar as one fp32 element on ``device`` (it is that already unless the scaler lives elsewhere)."""
        if t.device != device or t.dtype is not torch.float32:
            t = t.to(device=device, dtype=torch.float32, non_blocking=True)
        return t

    def _check_extras(self, plans):
        """What ``_upload`` sends behind each group's job rows with the scaler's check (one per plan, or None)."""
        return [None] * len(plans)

    def _unscale_check(self, plans, inv_scale, found_inf):
        """GradScaler._unscale_grads_ over this optimizer's gradients: one launch per group.  ``inv_scale`` / ``found_inf``: the
        scaler's per-device replicators.  Returns the devices it launched on."""
        devices = []
        for (_, fg, grads), extra in zip(plans, self._check_extras(plans)):
            if all(g is None for g in grads):
                continue
            with torch.cuda.device(fg.device):
                self._upload(fg, grads, extra)
                L.call('u2mkd_grads_unscale_check', L.ptr(fg.table), len(fg.params), fg.total_chunks,
                       L.ptr(inv_scale.get(fg.device)), L.ptr(found_inf.get(fg.device)), L.stream())
            if fg.device not in devices:
                devices.append(fg.device)
        return devices

    def _torch_step(self, loss):
        """torch's own update (whatever the fused path does not cover); its buffers are adopted by the next fused step.  Under a
        GradScaler it does what the scaler's generic route does around torch's unfused step: unscale by 1 / grad_scale if one is
        given, read found_inf on the host and skip the step if it is set (torch's unfused step itself refuses the two)."""
        self._adopt = True
        held = {k: self.__dict__[k] for k in ('grad_scale', 'found_inf') if self.__dict__.get(k) is not None}      # (to be hidden from torch's step)
        if isinstance(held.get('grad_scale'), torch.Tensor):
            inv = _MultiDeviceReplicator(held['grad_scale'].double().reciprocal().float())
            for group in self.param_groups:
                for p in group['params']:
                    if p.grad is not None:
                        g = p.grad._values() if p.grad.is_sparse else p.grad
                        g.mul_(inv.get(g.device))
        if isinstance(held.get('found_inf'), torch.Tensor) and held['found_inf'].item() != 0:
            return loss
        fn = self._torch_cls.step
        if getattr(fn, 'hooked', False):      # (the class-level hook wrapper: this call is already inside the fused class's own)
            fn = fn.__wrapped__
        for k in held:
            setattr(self, k, None)
        try:
            fn(self)
        finally:
            for k, v in held.items():
                setattr(self, k, v)           # (the scaler deletes them after the step)
        return loss


class FusedSGD(_Fused, torch.optim.SGD):
    _torch_cls = torch.optim.SGD

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, **kw):
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, **kw)
        self._init_fused()
        self._contract = 1

    @staticmethod
    def _eligible(group):
        """The group's settings are ones the kernel implements (the parameters themselves are checked when the group's job
        table is built, ``_fused``)."""
        return _ENABLED and not group.get('maximize') and not group.get('differentiable') and group['dampening'] == 0 \
            and isinstance(group['lr'], (float, int)) and len(group['params']) > 0      # (numpy.float64 from a LambdaLR is a float)

    def _adopt_state(self, fg):
        """Momentum buffers that exist in ``self.state`` but are not this group's views (a loaded checkpoint, a first step that
        torch's own path ran) are copied into the flat buffer and replaced by the views."""
        for i, p in enumerate(fg.params):
            st = self.state.get(p)
            buf = None if st is None else st.get('momentum_buffer')
            if buf is None:
                fg.has_buf[i] = False
            elif buf.data_ptr() != fg.bufs[i].data_ptr():
                fg.bufs[i].copy_(buf)
                st['momentum_buffer'] = fg.bufs[i]
                fg.has_buf[i] = True
            else:
                fg.has_buf[i] = True
        fg.first_col[:] = [0 if h else 1 for h in fg.has_buf]
        fg.missing = fg.has_buf.count(False)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale, found_inf = self._scaler_scalars()
        plans = None if (found_inf is None and grad_scale is not None) else self._plan()
        if plans is None:
            return self._torch_step(loss)
        if self._adopt:
            for _, fg, _ in plans:
                self._adopt_state(fg)
            self._adopt = False
        written = []
        for group, fg, grads in plans:
            written += [p for p, g in zip(fg.params, grads) if g is not None]
            if group['momentum'] != 0:
                written.append(fg.flat)                 # (the momentum buffers are views of it: one counter for all)
        # torch creates a momentum buffer only in a step that is applied: a step that would create one is decided on the host
        # (the first steps of a run, the ones that usually overflow); every later step is decided by the kernel alone.
        skip = found_inf is not None and any(
            group['momentum'] != 0 and fg.missing and any(g is not None and not h for g, h in zip(grads, fg.has_buf))
            for group, fg, grads in plans) and found_inf.item() != 0
        if not skip:
            for group, fg, grads in plans:
                with torch.cuda.device(fg.device):          # (the launch goes to the current stream of the GROUP's device)
                    self._launch(group, fg, grads, grad_scale, found_inf)
        # torch's rule for in-place writes: the kernel wrote these through raw pointers, so their versions move as torch's
        # SGD moves them -- caches keyed by version (functional.eval_bn_affine) miss, autograd's saved-tensor check holds.
        # Before the global post hook re-stamps the weights' fragment images (functional.refresh_weight_fragments).
        # (Whether a scaled step was applied is known on the device only: the versions move on skipped steps too.)
        torch._C._increment_version(written)
        for _, fg, _ in plans:
            fg.uploaded = None            # (a table is reused between a scaler's check and this step, never from step to step)
        return loss

    def _launch(self, group, fg, grads, grad_scale=None, found_inf=None):
        self._upload(fg, grads)
        if found_inf is None:
            L.call('u2mkd_sgd_batch', L.ptr(fg.table), len(fg.params), fg.total_chunks, float(group['lr']), float(group['momentum']),
                   float(group['weight_decay']), int(bool(group['nesterov'])), self._contract, L.stream())
        else:
            scale = None if grad_scale is None else self._scalar_on(grad_scale, fg.device)
            found = self._scalar_on(found_inf, fg.device)
            L.call('u2mkd_sgd_batch_amp', L.ptr(fg.table), len(fg.params), fg.total_chunks, float(group['lr']),
                   float(group['momentum']), float(group['weight_decay']), int(bool(group['nesterov'])), self._contract,
                   L.ptr(scale), L.ptr(found), L.stream())
        if fg.missing and group['momentum'] != 0:
            # torch: a parameter's momentum buffer comes into being with its first gradient (buf = clone(grad))
            for i, g in enumerate(grads):
                if g is not None and not fg.has_buf[i]:
                    fg.has_buf[i] = True
                    fg.first_col[i] = 0
                    fg.missing -= 1
                    self.state[fg.params[i]]['momentum_buffer'] = fg.bufs[i]


def adam_scalars(lr, beta1, beta2, t):
    """``(step_size, bias_correction2_sqrt)`` of step count ``t`` (a float, as torch's ``_get_value(step)``), in Python float
    arithmetic with torch's expressions (torch/optim/adam.py:_multi_tensor_adam, the non-capturable branch)."""
    bias_correction1 = 1 - beta1 ** t
    bias_correction2 = 1 - beta2 ** t
    step_size = (lr / bias_correction1) * -1
    bias_correction2_sqrt = bias_correction2 ** 0.5
    return step_size, bias_correction2_sqrt


class StepLedger:
    """Per-parameter step counts of an optimizer whose steps a GradScaler may skip ON THE DEVICE: the host issues call after
    call without knowing which were applied and learns the outcomes late, in order, possibly several at once.  No GPU in here.

    ``known[i]``: parameter i's count after every call whose outcome has arrived.  ``applied_known``: how many of those calls
    were applied -- the device's own count is this plus the applied ones among the ``pending`` calls.  While every pending call
    and the next one have the SAME set of parameters with a gradient, a parameter of that set stands at ``known[i] + a`` where
    ``a`` = the device's count - ``applied_known`` lies in ``0 .. len(pending)``: the host sends the candidates for each ``a``
    (``candidates``) and the device picks its row.  ``must_resolve`` says how many of the oldest pending calls have to be waited
    for before a call can be issued: all of them if its gradient set differs from a pending one's, and enough to keep the
    window within ``ring`` otherwise."""

    def __init__(self, n_params, ring=_COUNT_RING):
        self.known = np.zeros(n_params, dtype=np.int64)
        self.applied_known = 0
        self.calls = 0                    # scaled calls issued so far: call n reads the device's count slot n & 1
        self.pending = []                 # [(call, gradient set as a bool array)] -- outcomes not seen yet, oldest first
        self.ring = ring

    def must_resolve(self, mask):
        if any(not np.array_equal(m, mask) for _, m in self.pending):
            return len(self.pending)
        return max(0, len(self.pending) - (self.ring - 1))

    def window(self):
        return len(self.pending) + 1

    def candidates(self):
        """int64 [n_params, window]: the step count a parameter WITH a gradient takes in the next call, per offset."""
        return self.known[:, None] + np.arange(1, self.window() + 1, dtype=np.int64)[None, :]

    def issue(self, mask):
        """A scaled call with this gradient set goes out; returns its number."""
        assert self.must_resolve(mask) == 0
        n = self.calls
        self.calls += 1
        self.pending.append((n, np.array(mask, dtype=bool)))
        return n

    def fold(self, counts):
        """The device's count of applied steps after each of the ``len(counts)`` oldest pending calls, in order."""
        for c in counts:
            _, mask = self.pending.pop(0)
            applied = int(c) - self.applied_known
            if applied not in (0, 1):
                raise RuntimeError(f'StepLedger: the device counts {int(c)} applied steps, the host knew of {self.applied_known}')
            if applied:
                self.known[mask] += 1
                self.applied_known += 1

    def advance(self, mask):
        """A step the host knows to be applied (no scaler)."""
        assert not self.pending
        self.known[np.asarray(mask, dtype=bool)] += 1


# the spelling of each stage that equals torch's build on gfx950, element for element (tests/test_gpu_optim_adamw.py's stage probes;
# bits as in include/u2mkd_hip.h)
ADAM_FORM = 1 | 2 | 4 | 8


class _AdamGroup(_Group):
    def __init__(self, params, chunk):
        n = len(params)
        super().__init__(params, chunk, moments=2, extra=_COUNT_RING)      # (window x 2 floats = window int64 words per job)
        self.first_col = np.array([b.data_ptr() for b in self.bufs2], dtype=np.int64)      # (column 5 of an Adam job: exp_avg_sq)
        self.steps = torch.zeros(n, dtype=torch.float32)                   # state[p]['step']: 0-dim views, torch's CPU fp32 layout
        self.steps_np = self.steps.numpy()
        self.step_views = [self.steps[i] for i in range(n)]
        self.has_state = np.zeros(n, dtype=bool)
        self.lo = 0                        # this group's first index in the optimizer's ledger


class _FusedAdamSteps(_Fused):
    """Adam and AdamW (torch 2.10: AdamW is Adam with ``decoupled_weight_decay`` in the group) on csrc/optim.hip's
    u2mkd_adam_batch / u2mkd_adam_batch_amp: one launch per group.

    ``state[p]`` has torch's keys: ``step`` (a CPU fp32 scalar), ``exp_avg``, ``exp_avg_sq`` (views of one flat buffer per
    moment and group).  Under a GradScaler the entries come into being at a parameter's first gradient whether or not that
    step is applied (zero moments, step 0: numerically the absence of state, and what torch's ``fused=True`` Adam does), where
    torch's unfused route leaves ``state`` empty after a skipped first step.  Whether a scaled step was applied is known on
    the device only; ``state[p]['step']`` follows as the outcomes arrive, and ``sync_steps()`` -- which ``state_dict()`` and
    ``load_state_dict()`` call -- waits for the outstanding ones."""

    def _init_adam(self):
        self._init_fused()
        self._form = ADAM_FORM
        self._ledger = None
        self._ledger_groups = []
        self._counts = None                # device int32 [2]: the count of applied scaled steps, read from slot n & 1 by call n
        self._count_host = None            # pinned int32 [_COUNT_RING]: call n's outcome arrives in slot n % _COUNT_RING
        self._count_events = [None] * _COUNT_RING
        self._prepared = None

    def _make_group(self, params):
        return _AdamGroup(params, self._chunk)

    # ------------------------------------------------------------------ torch.optim.Optimizer surface
    def state_dict(self):
        self.sync_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        self.sync_steps()
        super().load_state_dict(state_dict)

    def sync_steps(self):
        """Wait until the outcome of every scaled step issued so far has arrived: ``state[p]['step']`` is exact afterwards."""
        if getattr(self, '_ledger', None) is not None and self._ledger.pending:
            self._resolve(len(self._ledger.pending), wait=True)

    # ------------------------------------------------------------------ eligibility
    @staticmethod
    def _eligible(group):
        num = (float, int)                 # (numpy.float64 from a LambdaLR is a float)
        return _ADAM_ENABLED and len(group['params']) > 0 and not any(
            group.get(k) for k in ('amsgrad', 'maximize', 'capturable', 'differentiable', 'fused')) \
            and isinstance(group['lr'], num) and isinstance(group['eps'], num) and isinstance(group['weight_decay'], num) \
            and all(isinstance(b, num) for b in group['betas'])

    def _plan(self):
        plans = super()._plan()
        if plans is not None and any(fg.device != plans[0][1].device for _, fg, _ in plans):
            return None                    # (one device: the count of applied steps lives there)
        return plans

    # ------------------------------------------------------------------ state
    def _ready(self, plans):
        """After a change of groups or a loaded checkpoint: one ledger over all groups' parameters; moments that exist in
        ``self.state`` but are not the groups' views are copied in and replaced by them, step counts are read."""
        if not self._adopt:
            return
        self.sync_steps()
        lo = 0
        for _, fg, _ in plans:
            fg.lo = lo
            lo += len(fg.params)
        old, self._ledger = self._ledger, StepLedger(lo)
        self._ledger_groups = [fg for _, fg, _ in plans]      # (whose step tensors the ledger's counts are written to)
        if old is not None:                # (the device's count goes on: the ledger keeps in step with it)
            self._ledger.applied_known, self._ledger.calls = old.applied_known, old.calls
        for _, fg, _ in plans:
            for i, p in enumerate(fg.params):
                st = self.state.get(p)
                if not st or 'exp_avg' not in st:
                    if fg.has_state[i]:
                        fg.bufs[i].zero_()
                        fg.bufs2[i].zero_()
                    fg.has_state[i] = False
                    fg.steps_np[i] = 0
                    continue
                for key, views in (('exp_avg', fg.bufs), ('exp_avg_sq', fg.bufs2)):
                    if st[key].data_ptr() != views[i].data_ptr():
                        views[i].copy_(st[key])
                        st[key] = views[i]
                if st['step'] is not fg.step_views[i]:
                    fg.steps_np[i] = float(st['step'])
                    st['step'] = fg.step_views[i]
                fg.has_state[i] = True
            self._ledger.known[fg.lo:fg.lo + len(fg.params)] = fg.steps_np.astype(np.int64)
        if self._counts is None:
            dev = plans[0][1].device
            self._counts = torch.zeros(2, dtype=torch.int32, device=dev)
            self._count_host = torch.zeros(_COUNT_RING, dtype=torch.int32).pin_memory()
            self._count_np = self._count_host.numpy()
        self._prepared = None
        self._adopt = False

    def _resolve(self, k, wait):
        """Fold in the outcomes of up to ``k`` of the oldest pending calls: those whose read-back has arrived, or, with ``wait``,
        all k of them."""
        led, counts = self._ledger, []
        for n, _ in led.pending[:k]:
            ev = self._count_events[n % _COUNT_RING]
            if not ev.query():
                if not wait:
                    break
                ev.synchronize()
            counts.append(int(self._count_np[n % _COUNT_RING]))
        if counts:
            led.fold(counts)
            self._write_steps()

    def _write_steps(self):
        # (the groups the ledger was made over: after add_param_group these are the ones ``state`` still points into)
        for fg in self._ledger_groups:
            fg.steps_np[:] = self._ledger.known[fg.lo:fg.lo + len(fg.params)]

    def _group_scalars(self, group, counts):
        """float32 [n, window, 2]: (step_size, bias_correction2_sqrt) per step count, each computed once as torch computes it
        and rounded to fp32 once."""
        uniq, inverse = np.unique(counts, return_inverse=True)
        beta1, beta2 = group['betas']
        vals = np.array([adam_scalars(group['lr'], beta1, beta2, float(t)) for t in uniq], dtype=np.float64).astype(np.float32)
        return np.ascontiguousarray(vals[inverse.reshape(counts.shape)])

    def _prepare(self, plans, scaled):
        """This call's gradient sets, window and per-group scalar tables.  Under a scaler: outcomes that have arrived are folded
        in, and the host waits only where it must (StepLedger.must_resolve)."""
        self._ready(plans)
        led = self._ledger
        masks = [np.array([g is not None for g in grads], dtype=bool) for _, _, grads in plans]
        mask = np.concatenate(masks)
        if led.pending:
            self._resolve(len(led.pending), wait=False)
            k = led.must_resolve(mask) if scaled else len(led.pending)
            if k:
                self._resolve(k, wait=True)
        cand = led.candidates()
        extras = [self._group_scalars(group, cand[fg.lo:fg.lo + len(fg.params)]) for group, fg, _ in plans]
        return dict(sig=self._signature(plans, scaled), masks=masks, mask=mask, window=led.window(), extras=extras, known=led.applied_known)

    def _signature(self, plans, scaled):
        led = self._ledger
        return ([[0 if g is None else g.data_ptr() for g in grads] for _, _, grads in plans],
                [(g['lr'], g['betas']) for g, _, _ in plans], led.calls, len(led.pending), scaled)

    def _check_extras(self, plans):
        # the scaler's check uploads the step's table: its scalars ride along, and step() finds the table in place
        self._prepared = prep = self._prepare(plans, True)
        return prep['extras']

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale, found_inf = self._scaler_scalars()
        plans = None if (found_inf is None and grad_scale is not None) else self._plan()
        if plans is None:
            return self._torch_step(loss)
        scaled = found_inf is not None
        prep, self._prepared = self._prepared, None
        if prep is None or self._adopt or prep['sig'] != self._signature(plans, scaled):
            prep = self._prepare(plans, scaled)
        if not prep['mask'].any():
            return loss                    # (no parameter has a gradient: torch's step does nothing either)
        led = self._ledger
        written = []
        for (group, fg, grads), m in zip(plans, prep['masks']):
            if m.any():
                written += [p for p, g in zip(fg.params, grads) if g is not None] + [fg.flat, fg.flat2]
                for i in np.flatnonzero(m & ~fg.has_state):      # a parameter's first gradient: torch's lazy state, as views
                    st = self.state[fg.params[i]]
                    st['step'], st['exp_avg'], st['exp_avg_sq'] = fg.step_views[i], fg.bufs[i], fg.bufs2[i]
                    fg.has_state[i] = True
        launching = [k for k, m in enumerate(prep['masks']) if m.any()]
        n = led.issue(prep['mask']) if scaled else None
        device = plans[0][1].device
        with torch.cuda.device(device):        # (the launches go to the current stream of the parameters' device)
            for k in launching:
                group, fg, grads = plans[k]
                self._launch(group, fg, grads, prep, prep['extras'][k], n, k == launching[-1], grad_scale, found_inf)
            if scaled:
                slot = n % _COUNT_RING
                self._count_host[slot:slot + 1].copy_(self._counts[(n + 1) & 1:((n + 1) & 1) + 1], non_blocking=True)
                ev = self._count_events[slot]
                if ev is None:
                    ev = self._count_events[slot] = torch.cuda.Event()
                ev.record()
        if not scaled:
            led.advance(prep['mask'])
            self._write_steps()
        torch._C._increment_version(written)      # (torch's rule for in-place writes, as FusedSGD.step; on skipped steps too)
        for _, fg, _ in plans:
            fg.uploaded = None
        return loss

    def _launch(self, group, fg, grads, prep, extra, n, last, grad_scale, found_inf):
        self._upload(fg, grads, extra)
        lr, wd, (beta1, beta2) = group['lr'], group['weight_decay'], group['betas']
        njobs = len(fg.params)
        head = (L.ptr(fg.table), njobs, fg.total_chunks, fg.table.data_ptr() + 48 * njobs)
        k = (float(1 - lr * wd), float(wd), int(bool(group.get('decoupled_weight_decay'))), float(1 - beta1), float(beta2),
             float(1 - beta2), float(group['eps']), self._form)
        if found_inf is None:
            L.call('u2mkd_adam_batch', *head, *k, L.stream())
        else:
            scale = None if grad_scale is None else self._scalar_on(grad_scale, fg.device)
            found = self._scalar_on(found_inf, fg.device)
            base = self._counts.data_ptr()
            L.call('u2mkd_adam_batch_amp', *head, prep['window'], *k, base + 4 * (n & 1), (base + 4 * ((n + 1) & 1)) if last else None,
                   prep['known'], L.ptr(scale), L.ptr(found), L.stream())

    def _torch_step(self, loss):
        self.sync_steps()
        if any(g.get('fused') for g in self.param_groups):
            # torch's fused Adam takes grad_scale / found_inf itself
            self._adopt = True
            fn = self._torch_cls.step
            if getattr(fn, 'hooked', False):
                fn = fn.__wrapped__
            fn(self)
            return loss
        return super()._torch_step(loss)


class FusedAdam(_FusedAdamSteps, torch.optim.Adam):
    _torch_cls = torch.optim.Adam

    def __init__(self, params, *args, **kw):
        super().__init__(params, *args, **kw)
        self._init_adam()


class FusedAdamW(_FusedAdamSteps, torch.optim.AdamW):
    _torch_cls = torch.optim.AdamW

    def __init__(self, params, *args, **kw):
        super().__init__(params, *args, **kw)
        self._init_adam()


class GradScaler(torch.amp.GradScaler):
    """``torch.amp.GradScaler`` whose unscale-and-check over a FusedSGD's gradients is one launch per parameter group
    (``u2mkd_grads_unscale_check``) instead of torch's list handling and multi-tensor launches; every other optimizer, and a
    FusedSGD whose step would be torch's own (CPU parameters, sparse or non-fp32 gradients ...), takes the parent's route.  No
    state of its own: ``state_dict`` / ``load_state_dict`` are the parent's.  ``FusedAdam`` / ``FusedAdamW`` are served as
    ``FusedSGD`` is (their job tables have the same rows), with the same rules for ``.grad``.

    ``step(FusedSGD)`` leaves ``.grad`` as ``step(torch.optim.SGD)`` does -- unscaled, on skipped steps too: the check the
    parent runs for an optimizer that handles the scale itself (inverse scale 1, nothing stored) is ``unscale_`` here, the
    optimizer then receives ``found_inf`` alone, and the trainer's code after the step (gradient norms, logging) sees what it
    saw with torch's SGD.  Under a plain ``torch.amp.GradScaler`` the step kernel unscales, and a skipped step leaves the
    gradients scaled, as with torch's fused optimizers."""

    def _unscale_grads_(self, optimizer, inv_scale, found_inf, allow_fp16):
        plans = optimizer._plan() if isinstance(optimizer, _Fused) else None
        if plans is None:
            return super()._unscale_grads_(optimizer, inv_scale, found_inf, allow_fp16)
        per_device_inv_scale, per_device_found_inf = _MultiDeviceReplicator(inv_scale), _MultiDeviceReplicator(found_inf)
        for r in (per_device_inv_scale, per_device_found_inf):
            r._per_device_tensors[r.master.device] = r.master      # (its own device is served without the replicator's copy)
        with torch.no_grad():
            devices = optimizer._unscale_check(plans, per_device_inv_scale, per_device_found_inf)
        return {d: per_device_found_inf.get(d) for d in devices}      # (as the parent: only devices that hold a gradient)

    def _check_inf_per_device(self, optimizer):
        if isinstance(optimizer, _Fused):
            self.unscale_(optimizer)
            return self._per_optimizer_states[id(optimizer)]['found_inf_per_device']
        return super()._check_inf_per_device(optimizer)
