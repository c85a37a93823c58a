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
not exist yet, and torch creates it only in a step that is applied) reads ``found_inf`` on the host."""
from __future__ import annotations

import os

import numpy as np
import torch

from torch.amp.grad_scaler import _MultiDeviceReplicator

from . import _lib as L

__all__ = ['FusedSGD', 'GradScaler']

_ENABLED = os.environ.get('U2MKD_FUSED_SGD', '1') != '0'      # 0: torch's own step (A/B runs)
_RING = 4


class _Group:
    """Static part of one parameter group's job table."""

    def __init__(self, params, chunk):
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
        self.has_buf = [False] * len(params)
        self.first_col = np.ones(len(params), dtype=np.int64)      # 1: no momentum buffer yet
        self.missing = len(params)
        n = len(params)
        self.stage = [torch.zeros(n, 6, dtype=torch.int64).pin_memory() for _ in range(_RING)]
        self.tabs = [s.numpy() for s in self.stage]
        for t in self.tabs:
            t[:, 0] = self.ptrs
            t[:, 2] = [b.data_ptr() for b in self.bufs]
            t[:, 3] = numel
            t[:, 4] = first[:-1]
            t[:, 5] = 1
        self.events = [None] * _RING
        self.table = torch.zeros(n, 6, dtype=torch.int64, device=dev)
        self.turn = 0
        self.uploaded = None               # (stream, gradient pointers, first-use column) of the table on the device


class FusedSGD(torch.optim.SGD):
    _step_supports_amp_scaling = True     # torch.amp.GradScaler.step: sets grad_scale / found_inf and calls step() unconditionally

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, **kw):
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, **kw)
        self._fused_groups = {}
        self._adopt = True
        self._contract = 1
        self._chunk = None

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

    # ------------------------------------------------------------------ the step
    @staticmethod
    def _eligible(group):
        """The group's settings are ones the kernel implements (the parameters themselves are checked when the group's job
        table is built, ``_fused``)."""
        return _ENABLED and not group.get('maximize') and not group.get('differentiable') and group['dampening'] == 0 \
            and isinstance(group['lr'], (float, int)) and len(group['params']) > 0      # (numpy.float64 from a LambdaLR is a float)

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
            fg = self._fused_groups[gi] = _Group(list(ps), self._chunk)
            fg.params_list = ps
            self._adopt = True
        return fg

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

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # a GradScaler's two device scalars (torch.amp.GradScaler.step sets them around this call, as for torch's fused optimizers)
        grad_scale, found_inf = getattr(self, 'grad_scale', None), getattr(self, 'found_inf', None)
        if not isinstance(found_inf, torch.Tensor):
            # (no parameter had a gradient: torch's scaler hands over sum([]) = the int 0 -- no check ran, nothing to skip or apply)
            grad_scale = found_inf = None
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

    def _upload(self, fg, grads):
        """This step's job table on the device (the gradients' addresses and the first-use flags change from step to step); a
        table that the scaler's check of this very step sent -- same gradients, same stream -- is not sent again (step() forgets it
        at its end: without a scaler every step sends its table, as before)."""
        key = (L.stream(), [0 if g is None else g.data_ptr() for g in grads], fg.first_col.tobytes())
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
        fg.table.copy_(fg.stage[slot], non_blocking=True)
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

    def _unscale_check(self, plans, inv_scale, found_inf):
        """GradScaler._unscale_grads_ over this optimizer's gradients: one launch per group.  ``inv_scale`` / ``found_inf``: the
        scaler's per-device replicators.  Returns the devices it launched on."""
        devices = []
        for _, fg, grads in plans:
            if all(g is None for g in grads):
                continue
            with torch.cuda.device(fg.device):
                self._upload(fg, grads)
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
        fn = torch.optim.SGD.step
        if getattr(fn, 'hooked', False):      # (the class-level hook wrapper: this call is already inside FusedSGD's own)
            fn = fn.__wrapped__
        for k in held:
            setattr(self, k, None)
        try:
            fn(self)
        finally:
            for k, v in held.items():
                setattr(self, k, v)           # (the scaler deletes them after the step)
        return loss


class GradScaler(torch.amp.GradScaler):
    """``torch.amp.GradScaler`` whose unscale-and-check over a FusedSGD's gradients is one launch per parameter group
    (``u2mkd_grads_unscale_check``) instead of torch's list handling and multi-tensor launches; every other optimizer, and a
    FusedSGD whose step would be torch's own (CPU parameters, sparse or non-fp32 gradients ...), takes the parent's route.  No
    state of its own: ``state_dict`` / ``load_state_dict`` are the parent's.

    ``step(FusedSGD)`` leaves ``.grad`` as ``step(torch.optim.SGD)`` does -- unscaled, on skipped steps too: the check the
    parent runs for an optimizer that handles the scale itself (inverse scale 1, nothing stored) is ``unscale_`` here, the
    optimizer then receives ``found_inf`` alone, and the trainer's code after the step (gradient norms, logging) sees what it
    saw with torch's SGD.  Under a plain ``torch.amp.GradScaler`` the step kernel unscales, and a skipped step leaves the
    gradients scaled, as with torch's fused optimizers."""

    def _unscale_grads_(self, optimizer, inv_scale, found_inf, allow_fp16):
        plans = optimizer._plan() if isinstance(optimizer, FusedSGD) else None
        if plans is None:
            return super()._unscale_grads_(optimizer, inv_scale, found_inf, allow_fp16)
        per_device_inv_scale, per_device_found_inf = _MultiDeviceReplicator(inv_scale), _MultiDeviceReplicator(found_inf)
        for r in (per_device_inv_scale, per_device_found_inf):
            r._per_device_tensors[r.master.device] = r.master      # (its own device is served without the replicator's copy)
        with torch.no_grad():
            devices = optimizer._unscale_check(plans, per_device_inv_scale, per_device_found_inf)
        return {d: per_device_found_inf.get(d) for d in devices}      # (as the parent: only devices that hold a gradient)

    def _check_inf_per_device(self, optimizer):
        if isinstance(optimizer, FusedSGD):
            self.unscale_(optimizer)
            return self._per_optimizer_states[id(optimizer)]['found_inf_per_device']
        return super()._check_inf_per_device(optimizer)
