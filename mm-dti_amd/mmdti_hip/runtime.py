"""Host-side runtime plumbing: bf16 weight shadows, gradient buffers, the flat parameter arena and dropout seeds.

MI355X-first layout: all trainable parameters live in ONE flat fp32 arena (plus a flat fp32 gradient arena and a flat
bf16 shadow), so the per-step work on parameters is three streams over contiguous HBM -- zero the gradients, one
bucketed RCCL all-reduce over slices of the gradient arena, one fused Adam pass that also refreshes the bf16 shadow --
instead of ~350 small per-tensor launches.  ``nn.Parameter``s stay what the reference's code expects (named tensors in
``state_dict()``); they are simply views into the arena.
"""
from __future__ import annotations

import weakref
from typing import Dict, Iterable, List, Optional

import torch

from . import ops

_ALIGN = 8  # elements: 16 B for the bf16 shadow, 32 B for fp32


class ParamArena:
    """Flatten a module's trainable parameters into contiguous data / grad / bf16-shadow buffers."""

    def __init__(self, params: Iterable[torch.nn.Parameter], adjacent: Iterable[tuple] = ()):
        """adjacent: tuples of parameters to lay out back to back (e.g. the query/key/value weights of an attention
        block, so that one GEMM can use them as a single [3D, D] matrix -- see fused_views)."""
        plist = [p for p in params if p.requires_grad]
        assert plist, "no trainable parameters"
        group_of = {}
        for grp in adjacent:
            grp = tuple(p for p in grp if p.requires_grad)
            if len(grp) > 1 and all(id(p) not in group_of for p in grp):
                for p in grp:
                    group_of[id(p)] = grp
        self.params: List[torch.nn.Parameter] = []
        seen = set()
        for p in plist:
            for q in group_of.get(id(p), (p,)):
                if id(q) not in seen:
                    seen.add(id(q))
                    self.params.append(q)
        dev = self.params[0].device
        assert dev.type == "cuda", "ParamArena needs device parameters"
        self.offsets: Dict[int, int] = {}
        off = 0
        for p in self.params:
            self.offsets[id(p)] = off
            off += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.numel = off
        self.data = torch.zeros(off, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(off, device=dev, dtype=torch.float32)
        self.shadow = torch.zeros(off, device=dev, dtype=torch.bfloat16)
        for p in self.params:
            o, n = self.offsets[id(p)], p.numel()
            self.data[o:o + n].copy_(p.data.reshape(-1).float())
            p.data = self.data[o:o + n].view(p.shape)
            p.grad = self.grad[o:o + n].view(p.shape)
            p._mmdti_arena = self
        self._version: Dict[int, int] = {}
        self.shadow16: Optional[torch.Tensor] = None      # fp16 shadow (fp16 forward-operand mode), built on first use
        self._epoch, self._epoch16 = 0, -1                # the fp16 shadow is valid while _epoch16 == _epoch
        self.refresh_shadow()
        self.adam_m: Optional[torch.Tensor] = None
        self.adam_v: Optional[torch.Tensor] = None
        self.ema: Optional[torch.Tensor] = None           # the parameters' moving average (enable_ema), fp32 like `data`
        self.step_count = 0
        # parameters frozen after the arena was built (requires_grad cleared): their elements are skipped by the Adam pass
        self.skip_mask: Optional[torch.Tensor] = None
        self._flags = (True,) * len(self.params)
        # parameter groups (set_groups): per block of 8 elements a group id, per group (lr_scale, weight_decay) -- both on the device
        self.group_ids: Optional[torch.Tensor] = None
        self.group_table: Optional[torch.Tensor] = None
        self.decoupled = False

    def set_groups(self, ids: torch.Tensor, table: torch.Tensor, decoupled: bool = False):
        """Switch the Adam pass to ops.adam_step_grouped.  ids: host uint8, one group id per block of 8 elements
        (freeze.arena_group_ids); table: host fp32 [ngroups, 2] of (lr_scale, weight_decay).  Both are uploaded ONCE: their device
        addresses never move afterwards (a captured graph reads them; later changes are copies into group_table)."""
        assert ids.dtype == torch.uint8 and ids.numel() == (self.numel + _ALIGN - 1) // _ALIGN, "set_groups: one id per block of 8 elements"
        assert table.dtype == torch.float32 and table.dim() == 2 and table.shape[1] == 2 and 1 <= table.shape[0] <= 256, "set_groups: table is fp32 [ngroups <= 256, 2]"
        assert self.group_ids is None, "set_groups: the groups are set once (change a row with a copy into group_table)"
        self.group_ids = ops.upload(ids.contiguous(), self.data.device)
        self.group_table = ops.upload(table.contiguous(), self.data.device)
        self.decoupled = bool(decoupled)

    def sync_trainable(self) -> bool:
        """Re-read requires_grad of the arena's parameters; rebuild the Adam skip mask when it changed.  -> True on a change.  (A
        parameter frozen after construction keeps its slots: it gets no gradient and the masked Adam pass leaves it, and its moments,
        alone -- torch.optim.Adam skips a parameter whose grad is None.)"""
        flags = tuple(p.requires_grad for p in self.params)
        if flags == self._flags:
            return False
        from .freeze import arena_skip_mask
        self._flags = flags
        m = arena_skip_mask(flags, [self.offsets[id(p)] for p in self.params], [p.numel() for p in self.params], self.numel, _ALIGN)
        self.skip_mask = None if m is None else m.to(self.data.device)
        for p, f in zip(self.params, flags):
            if not f:
                p.grad = None
        return True

    def refresh_shadow(self):
        """Re-cast the whole fp32 arena into the bf16 shadow the GEMMs read."""
        ops.lib().mmdti_cast_f32_bf16(ops._stream(), self.data.data_ptr(), self.shadow.data_ptr(), self.numel, 0.0, 0, 0)
        for p in self.params:
            self._version[id(p)] = p._version
        self._epoch += 1

    def _fresh(self, p):
        """The shadow is refreshed by the constructor and by adam_step (which writes both through raw pointers).  Any
        OTHER in-place write to a parameter -- ``load_state_dict`` on a model already bound to the arena (the reference
        trains, then loads the best checkpoint into the same model, tasks/trainer.py:406-410), ``p.copy_()`` -- bumps the
        tensor's version counter: re-cast that parameter's slice before a GEMM reads it."""
        if p._version != self._version[id(p)]:
            o, n = self.offsets[id(p)], p.numel()
            ops.lib().mmdti_cast_f32_bf16(ops._stream(), self.data[o:o + n].data_ptr(), self.shadow[o:o + n].data_ptr(), n, 0.0, 0, 0)
            self._version[id(p)] = p._version
            self._epoch += 1

    def zero_grad(self):
        self.grad.zero_()
        for p in self.params:          # re-bind in case an optimizer dropped the views (set_to_none)
            if not p.requires_grad:    # (frozen after construction: no gradient, as after the reference's zero_grad)
                p.grad = None
                continue
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + 4 * self.offsets[id(p)]:
                o, n = self.offsets[id(p)], p.numel()
                p.grad = self.grad[o:o + n].view(p.shape)

    def bf16(self, p: torch.nn.Parameter) -> torch.Tensor:
        self._fresh(p)
        o, n = self.offsets[id(p)], p.numel()
        return self.shadow[o:o + n].view(p.shape)

    def _fresh16(self):
        """fp16 shadow of the whole arena (the weights of the fp16 forward-operand mode): one cast pass whenever the fp32 data
        has changed since the last one (an optimizer step, a reload)."""
        if self.shadow16 is None:
            self.shadow16 = torch.empty(self.numel, device=self.data.device, dtype=torch.float16)
        if self._epoch16 != self._epoch:
            ops.lib().mmdti_cast_f32_f16(ops._stream(), self.data.data_ptr(), self.shadow16.data_ptr(), self.numel, 0.0, 0, 0)
            self._epoch16 = self._epoch

    def f16(self, p: torch.nn.Parameter) -> torch.Tensor:
        self._fresh(p)
        self._fresh16()
        o, n = self.offsets[id(p)], p.numel()
        return self.shadow16[o:o + n].view(p.shape)

    def fused(self, plist):
        """(bf16 shadow, fp32 data, fp32 grad) views spanning parameters that sit back to back in the arena (rows
        concatenated), or None."""
        o0 = self.offsets.get(id(plist[0]))
        if o0 is None:
            return None
        o, cols = o0, plist[0].shape[1:]
        for p in plist:
            if self.offsets.get(id(p)) != o or p.shape[1:] != cols:
                return None
            o += p.numel()
        for p in plist:
            self._fresh(p)
        shape = (sum(p.shape[0] for p in plist),) + tuple(cols)
        w16 = None
        if ops.FWD_F16:
            self._fresh16()
            w16 = self.shadow16[o0:o].view(shape)
        # (bf16 shadow, fp32 data, fp32 gradient, forward-GEMM shadow: fp16 in the fp16 forward-operand mode, else the bf16 one)
        return self.shadow[o0:o].view(shape), self.data[o0:o].view(shape), self.grad[o0:o].view(shape), (w16 if w16 is not None else self.shadow[o0:o].view(shape))

    def adam_step(self, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, max_norm: Optional[float] = None, step_state=None, guard=None):
        """torch.optim.Adam semantics (tasks/trainer.py:160) + optional global-norm clipping (:274), one fused pass.
        step_state: device-resident schedule (ops.step_state_advance) -- lr and the step count then live on the device.
        guard: device state of the non-finite step guard (new_nonfinite_guard) -- GradScaler.step's skip (:280): one pass over the
        gradients counts inf / NaN elements (fused with the clipping norm) and, if there is any, the Adam pass writes nothing.  The
        bias corrections then follow the guard's count of steps actually taken (a table of the host's values indexed by it, or the
        step state's device expression), never the host's step_count, which cannot know about a skip without a synchronisation.
        -> (grad_norm, skipped): the pre-clip global norm (None when neither clipping nor the guard computed it) and this step's
        skip flag as a device scalar (None without a guard)."""
        if self.adam_m is None:
            self.adam_m = torch.zeros_like(self.data)
            self.adam_v = torch.zeros_like(self.data)
        self.step_count += 1
        scale = norm = skipped = None
        if guard is not None:
            table = None
            if step_state is None:
                table = self._bias_table(betas)
            buf = torch.zeros(3 + 4096, device=self.data.device, dtype=torch.float32)    # {sum, count, flag} | partials | counts
            ops.sumsq_check(self.grad, buf[:3], buf[3:], guard, table, betas[0], betas[1])
            ss, skipped = buf[:1], buf[2:3]
        elif max_norm is not None:
            buf = torch.zeros(1 + 2048, device=self.data.device, dtype=torch.float32)      # the sum | per-workgroup partials (fixed-order fold)
            ss = buf[:1]
            ops.sumsq(self.grad, ss, buf[1:])
        if guard is not None or max_norm is not None:
            norm = ss.sqrt()
        if max_norm is not None:
            # clip_grad_norm_: coef = max_norm / (norm + 1e-6), clamped to 1 (tiny scalar math; stays on device, no sync)
            scale = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
        # (the Adam pass writes BOTH 16-bit shadows -- bf16 for the backward GEMMs, fp16 for the forward ones -- through raw pointers:
        #  a captured graph's replays keep them fresh too; the fp16 one exists once a forward GEMM has asked for it)
        p_f16 = self.shadow16 if self._epoch16 == self._epoch else None
        if self.group_ids is not None:
            # (parameter groups: the table holds every group's weight decay; the by-value one is the default group's row)
            ops.adam_step_grouped(self.data, self.grad, self.adam_m, self.adam_v, self.shadow, lr, betas[0], betas[1], eps, self.step_count,
                                  self.group_ids, self.group_table, self.decoupled, self.skip_mask, guard, scale, step_state, p_f16=p_f16)
        elif self.skip_mask is not None:
            ops.adam_step_masked(self.data, self.grad, self.adam_m, self.adam_v, self.shadow, lr, betas[0], betas[1], eps, weight_decay,
                                 self.step_count, self.skip_mask, guard, scale, step_state, p_f16=p_f16)
        elif guard is None:
            ops.adam_step(self.data, self.grad, self.adam_m, self.adam_v, self.shadow, lr, betas[0], betas[1], eps, weight_decay,
                          self.step_count, scale, step_state, p_f16=p_f16)
        else:
            ops.adam_step_guarded(self.data, self.grad, self.adam_m, self.adam_v, self.shadow, lr, betas[0], betas[1], eps, weight_decay,
                                  guard, scale, step_state, p_f16=p_f16)
        self._epoch += 1
        if self.shadow16 is not None and self._epoch16 == self._epoch - 1:
            self._epoch16 = self._epoch
        return norm, skipped

    # ------------------------------------------------------------------ weight averaging (DESIGN.md "Weight averaging (EMA)")
    def enable_ema(self):
        """Allocate the average: an fp32 buffer like ``data``, initialised as a copy of it."""
        if self.ema is None:
            self.ema = self.data.clone()

    def ema_step(self, decay, warmup=True, guard=None, step_state=None):
        """One launch, right after adam_step and with its choice of the source of t: the guard's count of steps actually taken (a skipped
        step leaves the average alone), else the step state's counter, else this arena's step_count by value."""
        assert self.ema is not None, "ema_step: enable_ema() first"
        ops.ema_update(self.data, self.ema, decay, warmup, self.step_count, guard, step_state)

    def swap_average(self):
        """Exchange ``data`` and ``ema`` in one pass that also writes the bf16 shadow and -- once it exists -- the fp16 one from the new
        ``data``.  As in adam_step the kernel writes through raw pointers, so the bookkeeping follows here: every parameter's shadow
        slice is fresh at its current version (a pending in-place edit was part of what the pass read), and so is the fp16 shadow."""
        assert self.ema is not None, "swap_average: enable_ema() first"
        ops.ema_swap(self.data, self.ema, self.shadow, self.shadow16)
        for p in self.params:
            self._version[id(p)] = p._version
        self._epoch += 1
        if self.shadow16 is not None:
            self._epoch16 = self._epoch

    # ------------------------------------------------------------------ checkpoints (DESIGN.md "Resuming a run")
    _STATE_BUFFERS = (("exp_avg", "adam_m"), ("exp_avg_sq", "adam_v"), ("ema", "ema"))

    def _state_names(self, names):
        names = [str(i) for i in range(len(self.params))] if names is None else [str(n) for n in names]
        if len(names) != len(self.params) or len(set(names)) != len(names):
            raise ValueError(f"ParamArena: {len(self.params)} distinct parameter names expected, got {len(names)} ({len(set(names))} distinct)")
        return names

    def state_dict(self, names=None, sync=True):
        """The optimizer's side of the arena, keyed by parameter name (``names``: one per parameter in arena order; None: the positions),
        not a flat dump -- another layout of the same parameters reads it too.  Per parameter ``exp_avg``, ``exp_avg_sq`` and ``ema``
        where the buffer exists (moments never allocated are absent), each an fp32 host copy of the parameter's slice in its shape; and
        ``step_count`` and the trainable ``flags``.  The values themselves are the model's (``model.state_dict()``).  sync=False: the
        copies are only enqueued into pinned memory -- synchronise the stream before reading them."""
        names = self._state_names(names)
        host = {k: host_copy(getattr(self, a)) for k, a in self._STATE_BUFFERS if getattr(self, a) is not None}
        if sync:
            torch.cuda.current_stream().synchronize()
        params = {}
        for name, p in zip(names, self.params):
            o, n = self.offsets[id(p)], p.numel()
            params[name] = {k: h[o:o + n].view(p.shape) for k, h in host.items()}
        return {"step_count": int(self.step_count), "flags": tuple(bool(f) for f in self._flags), "params": params}

    def check_state_dict(self, sd, names):
        """What load_state_dict would refuse, without writing anything: ValueError."""
        names = self._state_names(names)
        params = sd["params"]
        if set(params) != set(names):
            odd = sorted(set(params) ^ set(names))
            raise ValueError(f"ParamArena.load_state_dict: the state and the arena hold different parameters: {odd[:5]}")
        for k, a in self._STATE_BUFFERS:
            have = [name for name in names if params[name].get(k) is not None]
            if have and len(have) != len(names):
                raise ValueError(f"ParamArena.load_state_dict: {k} is there for {len(have)} of {len(names)} parameters")
            if k == "ema" and bool(have) != (self.ema is not None):
                raise ValueError("ParamArena.load_state_dict: the state " + ("holds" if have else "has no") + " parameter average (ema), "
                                 "this arena " + ("has none" if have else "holds one"))
            for name, p in zip(names, self.params):
                t = params[name].get(k)
                if t is not None and t.numel() != p.numel():
                    raise ValueError(f"ParamArena.load_state_dict: {k} of {name} has {t.numel()} elements, the parameter {p.numel()}")
        return names

    def load_state_dict(self, sd, names=None):
        """Copy a state_dict() into the buffers this arena already has (no address moves: captured graphs stay valid); the moments are
        allocated first if no step has been taken yet, and zeroed if the state has none.  Then the bf16 shadow is re-cast from the
        fp32 data as it stands (load the model's values BEFORE this) and the fp16 one is rebuilt at its next use.  The trainable flags
        are the owner's to apply (requires_grad, then sync_trainable)."""
        names = self.check_state_dict(sd, names)
        params = sd["params"]
        for k, a in self._STATE_BUFFERS:
            saved = params[names[0]].get(k) is not None
            if not saved:
                if k != "ema" and getattr(self, a) is not None:
                    getattr(self, a).zero_()
                continue
            if getattr(self, a) is None:
                setattr(self, a, torch.zeros_like(self.data))
            flat = torch.zeros(self.numel, dtype=torch.float32, pin_memory=True)
            for name, p in zip(names, self.params):
                o, n = self.offsets[id(p)], p.numel()
                flat[o:o + n].copy_(params[name][k].reshape(-1))
            getattr(self, a).copy_(flat, non_blocking=True)
        self.step_count = int(sd["step_count"])
        self.refresh_shadow()           # (advances _epoch: the fp16 shadow, if there is one, is stale until _fresh16 re-casts it)
        tab = getattr(self, "_bias_tab", None)
        if tab is not None and tab[1].shape[0] < self.step_count:
            del self._bias_tab

    def _bias_table(self, betas):
        """Device table of the host's bias corrections for t = 1 .. >= step_count (the guard's t never exceeds the steps enqueued):
        rebuilt, at twice the length, when the step count outgrows it -- enqueued, no synchronisation."""
        tab = getattr(self, "_bias_tab", None)
        if tab is None or tab[0] != tuple(betas) or tab[1].shape[0] < self.step_count:
            steps = max(1024, 2 * self.step_count)
            tab = (tuple(betas), ops.adam_bias_table(betas[0], betas[1], steps, self.data.device))
            self._bias_tab = tab
        return tab[1]


def host_copy(t: torch.Tensor) -> torch.Tensor:
    """A device tensor's copy in pinned host memory, ENQUEUED on the current stream: valid once that stream has been synchronised (a
    checkpoint enqueues all its copies and synchronises once).  A host tensor is cloned."""
    if not t.is_cuda:
        return t.detach().clone()
    out = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    out.copy_(t.detach(), non_blocking=True)
    return out


def new_nonfinite_guard(device) -> torch.Tensor:
    """Device state of the non-finite step guard (ops.sumsq_check): fp32 {optimizer steps taken, steps skipped, this step's skip
    flag, 1-beta1^t, sqrt(1-beta2^t)} (+ padding), all zero."""
    return torch.zeros(8, device=device, dtype=torch.float32)


class _ShadowCache:
    """bf16 copies of parameters that are not arena-managed (unit tests, ad-hoc modules): re-cast when the parameter's
    version counter or storage changes."""

    def __init__(self):
        self._c: Dict[int, tuple] = {}

    def get(self, p: torch.Tensor, f16: bool = False) -> torch.Tensor:
        key = (id(p), f16)
        ent = self._c.get(key)
        ver = (p.data_ptr(), p._version, tuple(p.shape))
        # id() values are recycled once a parameter dies: the weak reference proves the entry belongs to THIS tensor
        if ent is None or ent[0]() is not p or ent[1] != ver:
            if len(self._c) > 4096:
                self._c = {k: e for k, e in self._c.items() if e[0]() is not None}
            src = p.detach().contiguous()
            ent = (weakref.ref(p), ver, ops.cast_act16(src) if f16 else ops.cast_bf16(src))
            self._c[key] = ent
        return ent[2]


_shadow_cache = _ShadowCache()


def wbf16(p: torch.Tensor) -> torch.Tensor:
    """bf16 view/copy of a weight for the MFMA GEMMs."""
    arena = getattr(p, "_mmdti_arena", None)
    if arena is not None:
        return arena.bf16(p)
    return _shadow_cache.get(p)


def wfwd(p: torch.Tensor) -> torch.Tensor:
    """The weight as the operand of a FORWARD GEMM: the bf16 shadow, or -- fp16 forward-operand mode (ops.FWD_F16) -- the fp16 one."""
    if not ops.FWD_F16:
        return wbf16(p)
    arena = getattr(p, "_mmdti_arena", None)
    if arena is not None:
        return arena.f16(p)
    return _shadow_cache.get(p, f16=True)


def fused_views(plist):
    """Views over parameters laid out back to back in one ParamArena (see ParamArena(adjacent=...)), else None."""
    arena = getattr(plist[0], "_mmdti_arena", None)
    if arena is None or any(getattr(p, "_mmdti_arena", None) is not arena or not p.requires_grad for p in plist):
        return None
    return arena.fused(plist)


def gbuf(p: torch.Tensor) -> Optional[torch.Tensor]:
    """fp32 gradient buffer of a parameter that kernels accumulate into (atomically); None if frozen."""
    if not p.requires_grad:
        return None
    if p.grad is None:
        p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
    return p.grad


class DropoutState:
    """Counter-based dropout: every forward call of a module takes a fresh 64-bit seed; sites within the call are
    numbered, and the backward regenerates the masks from (seed, site)."""

    def __init__(self, seed: int = 0x5EED):
        self.base = seed
        self._calls = 0                     # forward calls that have drawn a seed since the last reseed

    def next_seed(self) -> int:
        self._calls += 1
        return (self.base * 0x9E3779B97F4A7C15 + self._calls * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF

    def reseed(self, seed: int):
        self.base = seed
        self._calls = 0

    def mark(self) -> int:
        """The call counter as it stands: hand it to rewind() to draw the seeds that follow once more."""
        return self._calls

    def rewind(self, mark: int):
        """Set the call counter to a value mark() returned: the next calls draw the seeds (hence the masks) drawn after that mark.
        FineTuner.step_accumulated replays a micro-batch's forward with it; moving forwards (past a replay) is allowed as well."""
        if not (isinstance(mark, int) and mark >= 0):
            raise ValueError(f"DropoutState.rewind: not a mark() value: {mark!r}")
        self._calls = mark

    def state(self) -> dict:
        """{base, calls}: where the stream stands (checkpoints: FineTuner.state_dict)."""
        return {"base": int(self.base), "calls": int(self._calls)}

    def load_state(self, base: int, calls: int):
        """Continue the stream of ``base`` after ``calls`` forward calls: the next seeds are those that followed state()."""
        if not (isinstance(calls, int) and calls >= 0):
            raise ValueError(f"DropoutState.load_state: calls must be a count >= 0, got {calls!r}")
        self.base = int(base)
        self._calls = calls


dropout_state = DropoutState()


# ---- gradient-ready notifications (consumed by parallel.ArenaReducer to overlap the all-reduce with backward) ----
_grad_ready_hooks: Dict[int, object] = {}


def add_grad_ready_hook(owner, fn):
    """Register `fn(params)`; one hook per owner (a FineTuner).  Each reducer ignores parameters outside its own arena,
    so several engines in one process do not disturb each other.  Held weakly: a dead owner's hook disappears."""
    ref = weakref.WeakMethod(fn) if hasattr(fn, "__self__") else (lambda f=fn: f)
    _grad_ready_hooks[id(owner)] = ref


def remove_grad_ready_hook(owner):
    _grad_ready_hooks.pop(id(owner), None)


def notify_grads_ready(params):
    """Called by the backward of a module once every gradient of `params` has been enqueued on the stream."""
    if not _grad_ready_hooks:
        return
    params = list(params)
    for key, ref in list(_grad_ready_hooks.items()):
        fn = ref()
        if fn is None:
            del _grad_ready_hooks[key]
        else:
            fn(params)
