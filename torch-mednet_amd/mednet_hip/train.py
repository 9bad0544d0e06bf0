"""Training-step harness for the hot path: the callers' step contract (segmentation.py:58-65, landmarks.py:66-83,
configure_optimizers :119-120) plus what pytorch_lightning's Trainer(gpus=N) adds around it (train_seg.py:126): one
gradient all-reduce per step over RCCL and the Adam update.

MI355X-first layout: all parameters live in ONE flat fp32 buffer and all gradients in another.  Backward kernels
write each parameter gradient straight into its slice (no autograd accumulate kernels), the data-parallel exchange
is a single RCCL all-reduce of the flat gradient buffer (35 MB for config 3), its 1/world averaging is folded into the
fused Adam kernel, and Adam is one launch over the flat buffers.
"""
from __future__ import annotations

import os

import torch
import torch.distributed as dist

from . import ops, vis
from .unet import loss as HL


class FlatParams:
    """Re-homes a module's parameters into one flat fp32 buffer (+ a flat gradient buffer the kernels write into).

    Slices are 64-element aligned; the padding elements between them are zero in both buffers from construction on and must STAY
    zero: no kernel writes them, and the global gradient norm (ops.grad_norm_) runs over the whole buffer, padding included, and
    relies on it."""

    def __init__(self, module: torch.nn.Module):
        # (name, parameter, requires_grad) of EVERY parameter as the buffers were laid out: a flag changed later is an error
        # (verify), not a silently trained "frozen" parameter or a silently untrained thawed one
        self.flags = [(k, p, p.requires_grad) for k, p in module.named_parameters()]
        self.params = [p for p in module.parameters() if p.requires_grad]
        if not self.params:
            raise RuntimeError("FlatParams: the module has no trainable parameter")
        dev = self.params[0].device
        self.offsets = []
        total = 0
        for p in self.params:
            self.offsets.append(total)
            total += (p.numel() + 63) // 64 * 64  # 256-byte aligned slices
        self.total = total
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(total, dtype=torch.float32, device=dev)
        for p, off in zip(self.params, self.offsets):
            view = self.flat[off:off + p.numel()].view_as(p)
            view.copy_(p.data)
            p.data = view
            p._mednet_grad = self.grad[off:off + p.numel()].view_as(p)

    def verify(self):
        """The gradient slices are handed out once, here at construction: a parameter frozen afterwards would still be written by
        the kernels and moved by Adam, one thawed afterwards would never train.  Called by the step classes on every call (a loop
        over the recorded flags: no device work, nothing to capture)."""
        for name, p, flag in self.flags:
            if p.requires_grad != flag:
                raise RuntimeError(f"mednet_hip: requires_grad of parameter '{name}' changed from {flag} to {p.requires_grad} after the "
                                   f"training step was built; freeze or unfreeze first, then rebuild the step")

    def grads_as_attr(self):
        """Expose the flat slices as .grad (for inspection / torch optimizers)."""
        for p in self.params:
            p.grad = p._mednet_grad

    def release(self):
        for p in self.params:
            if hasattr(p, "_mednet_grad"):
                del p._mednet_grad


def _check_guard_args(who, clip_grad_norm, lr, weight_decay):
    if clip_grad_norm is not None and not clip_grad_norm > 0:
        raise ValueError(f"{who}: clip_grad_norm must be a positive number or None, got {clip_grad_norm!r}")
    if lr < 0 or weight_decay < 0:
        raise ValueError(f"{who}: negative lr {lr} or weight_decay {weight_decay}")


class _FlatOptimizer:
    """What FlatAdam and FlatSGD share: the hyper-parameters every form has, the device state of the guarded forms, the two step counts
    (host `t` / device), the state dict and ONE step body.  A subclass states MOMENTS (its moment buffers: attributes and state-dict
    keys), HYPER (state-dict key -> attribute of its hyper-parameters), `_norm_runs` and its one update launch `_update`."""

    MOMENTS, HYPER = (), {}

    def __init__(self, flat: FlatParams, lr, weight_decay, clip_grad_norm, skip_nonfinite):
        _check_guard_args(type(self).__name__, clip_grad_norm, lr, weight_decay)
        self.flat, self.lr, self.wd = flat, lr, weight_decay
        self.clip, self.skip_nonfinite = clip_grad_norm, bool(skip_nonfinite)
        self.t = 0  # calls so far; versions the parameters (_step).  The plain forms count their steps with it (FlatAdam's bias
        #             correction uses it); the guarded forms and every form behind a LossScaler count on the DEVICE, where a skipped
        #             step does not advance the count: steps_taken() reads the truth.
        self._scaled = None  # which of the two update forms this optimizer runs (they keep different step counts)

    def steps_taken(self, scaler: "LossScaler | None" = None) -> int:
        """Optimizer steps actually applied (synchronises when the count lives on the device)."""
        if scaler is not None:
            return int(scaler.state[2].item())
        return int(self.opt_state[4].item()) if self.guarded else self.t

    def state_dict(self, scaler: "LossScaler | None" = None):
        sd = {k: None if getattr(self, k) is None else getattr(self, k).detach().cpu().clone() for k in self.MOMENTS}
        sd["t"] = self.steps_taken(scaler)
        sd.update((k, getattr(self, attr)) for k, attr in self.HYPER.items())
        if self.opt_state is not None:
            sd["opt_state"] = self.opt_state.detach().cpu().clone()
        if scaler is not None:
            sd["scaler"] = scaler.state_dict()
        return sd

    def load_state_dict(self, sd, scaler: "LossScaler | None" = None):
        """Restores the moments, the step count and the hyper-parameters the state was saved with (torch.optim's load_state_dict
        restores its param_groups too).  A run that trains behind a loss scaler must find the scaler's state in `sd`: resuming fp16
        training with a fresh scale of 65536 and a device step count of 0 would silently restart the bias correction."""
        for k in self.MOMENTS:
            if getattr(self, k) is not None:
                getattr(self, k).copy_(sd[k].to(self.flat.flat.device))
        self.t = int(sd["t"])
        for k, attr in self.HYPER.items():
            if k in sd:
                setattr(self, attr, tuple(sd[k]) if k == "betas" else sd[k])
        if self.opt_state is not None:  # (a state saved by a plain form has no device state: its host count becomes the device count)
            _load_opt_state(self.opt_state, sd, self.t)
        if scaler is not None:
            if "scaler" not in sd:
                raise KeyError(f"{type(self).__name__}.load_state_dict: a LossScaler was passed but the saved state has no 'scaler' "
                               f"entry (it was saved by a run without loss scaling)")
            scaler.load_state_dict(sd["scaler"])

    def _step(self, gscale, scaler):
        scaled = scaler is not None
        if self._scaled is None:
            self._scaled = scaled
        elif self._scaled != scaled:
            raise RuntimeError(f"{type(self).__name__}: step() and step_scaled() keep different step counts (host / device) and cannot "
                               f"be mixed on one optimizer")
        self.t += 1
        ost = self.opt_state if self._norm_runs(scaler) else None
        if ost is not None:  # (behind a scaler the norm is taken of the UNSCALED gradient and its pass replaces the overflow sweep)
            ops.grad_norm_(self.flat.grad, ost, self.clip, gscale, None if scaler is None else scaler.state)
        self._update(gscale, ost, scaler)
        # torch's version counter only moves on torch in-place ops; a no-op in-place op on the flat buffer does not
        # reach the views' counters, so packed-weight caches are keyed on this step counter as well.
        for p in self.flat.params:
            p._mednet_step = self.t

    def step(self, grad_scale=1.0):
        self._step(grad_scale, None)

    def step_scaled(self, scaler: "LossScaler", inv_world=1.0):
        """The same update behind the loss scaler: unscale, skip on overflow, adjust the scale -- all on the device."""
        self._step(inv_world, scaler)


def _load_opt_state(opt_state, sd, steps):
    """Restore the device state of the guarded update forms; a saved state without one starts from `steps` steps taken."""
    if "opt_state" in sd:
        opt_state.copy_(sd["opt_state"].to(opt_state.device))
    else:
        opt_state.copy_(torch.tensor(ops.OPT_STATE_FRESH, dtype=torch.float32))
        opt_state[4] = float(steps)
    opt_state[3] = 0.0


class FlatAdam(_FlatOptimizer):
    """torch.optim.Adam(lr) semantics (betas .9/.999, eps 1e-8, weight_decay 0) as one kernel over FlatParams.

    decoupled_weight_decay=True is torch.optim.AdamW's rule (p *= 1 - lr wd, no L2 term).  clip_grad_norm (a float: clip the mean
    gradient to that global L2 norm, torch.nn.utils.clip_grad_norm_'s rule) and skip_nonfinite (skip the whole update when a gradient
    is NaN / inf, in every storage mode) route the step through the norm pass and the guarded update kernel (ops.grad_norm_ +
    ops.adamw_step_), as does the decoupled decay; the bias correction then uses the device-side count `opt_state[4]` of steps actually
    taken.  With all three off the launches are the ones this class always made (ops.adam_step_, or ops.adam_step_scaled_ behind a
    LossScaler, whose state[2] is then the count of the bias correction)."""

    MOMENTS, HYPER = ("m", "v"), {"lr": "lr", "betas": "betas", "eps": "eps", "weight_decay": "wd"}

    def __init__(self, flat: FlatParams, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False,
                 clip_grad_norm=None, skip_nonfinite=False):
        super().__init__(flat, lr, weight_decay, clip_grad_norm, skip_nonfinite)
        self.betas, self.eps, self.decoupled = betas, eps, bool(decoupled_weight_decay)
        self.guarded = self.decoupled or self.clip is not None or self.skip_nonfinite
        self.opt_state = ops.new_opt_state(flat.flat.device) if self.guarded else None
        self.m = torch.zeros_like(flat.flat)
        self.v = torch.zeros_like(flat.flat)

    def _norm_runs(self, scaler) -> bool:
        return self.guarded

    def _update(self, gscale, ost, scaler):
        f, hp = self.flat, (self.lr, self.betas[0], self.betas[1], self.eps, self.wd)
        if ost is not None:
            ops.adamw_step_(f.flat, f.grad, self.m, self.v, *hp, ost, self.decoupled, gscale, scaler)
        elif scaler is not None:
            ops.adam_step_scaled_(f.flat, f.grad, self.m, self.v, *hp, scaler, gscale)
        else:
            ops.adam_step_(f.flat, f.grad, self.m, self.v, *hp, self.t, gscale)


class FlatSGD(_FlatOptimizer):
    """torch.optim.SGD(lr, momentum, dampening 0, weight_decay, nesterov) as one kernel over FlatParams, with FlatAdam's surface.

    clip_grad_norm / skip_nonfinite put the norm pass (ops.grad_norm_) in front: clip coefficient and skip rule are read by the update
    kernel on the device.  Behind a LossScaler (step_scaled) the norm pass always runs: it is what finds the overflow.  With
    momentum 0 there is no buffer and no buffer traffic.  Weight decay applies to the whole flat buffer (no parameter groups)."""

    MOMENTS, HYPER = ("buf",), {"lr": "lr", "momentum": "momentum", "nesterov": "nesterov", "weight_decay": "wd"}

    def __init__(self, flat: FlatParams, lr, momentum=0.0, nesterov=False, weight_decay=0.0, clip_grad_norm=None, skip_nonfinite=False):
        super().__init__(flat, lr, weight_decay, clip_grad_norm, skip_nonfinite)
        if not 0.0 <= momentum < 1.0:
            raise ValueError(f"FlatSGD: momentum {momentum} outside [0, 1)")
        if nesterov and momentum == 0.0:
            raise ValueError("FlatSGD: nesterov needs momentum > 0 (torch.optim.SGD's rule)")
        self.momentum, self.nesterov = momentum, bool(nesterov)
        self.guarded = self.clip is not None or self.skip_nonfinite
        self.opt_state = ops.new_opt_state(flat.flat.device)
        self.buf = torch.zeros_like(flat.flat) if momentum != 0.0 else None

    def load_state_dict(self, sd, scaler: "LossScaler | None" = None):
        if (self.buf is None) != (sd["buf"] is None):
            raise ValueError("FlatSGD.load_state_dict: the saved state and this optimizer disagree about a momentum buffer")
        super().load_state_dict(sd, scaler)

    def _norm_runs(self, scaler) -> bool:
        return self.guarded or scaler is not None

    def _update(self, gscale, ost, scaler):
        f = self.flat
        ops.sgd_step_(f.flat, f.grad, self.buf, self.lr, self.momentum, self.nesterov, self.wd, gscale, ost, scaler)


class PolyLR:
    """lr(call_index) = base_lr * (1 - call_index / total_steps) ** power, 0 from total_steps on: the polynomial decay of the common 3D
    segmentation recipe.  A step class evaluates it on the host once per call, as a scheduler stepped once per iteration is; the index
    counts CALLS, skipped steps included.  The optimiser launch lies outside the captured graph and takes lr as a kernel argument, so
    a changing lr is graph-safe as it stands."""

    def __init__(self, base_lr, total_steps, power=0.9):
        if total_steps < 1:
            raise ValueError(f"PolyLR: total_steps {total_steps} < 1")
        self.base_lr, self.total_steps, self.power = float(base_lr), int(total_steps), float(power)

    def __call__(self, call_index):
        left = 1.0 - min(max(int(call_index), 0), self.total_steps) / self.total_steps
        return self.base_lr * left ** self.power


def make_optimizer(flat, optimizer="adam", optimizer_args=None, lr=1e-3, clip_grad_norm=None, skip_nonfinite=False):
    """-> (optimizer, lr callable or None) for the step classes.  optimizer: "adam" | "adamw" | "sgd"; optimizer_args go to FlatAdam /
    FlatSGD as they are and may not repeat what the step's own arguments set."""
    args = dict(optimizer_args or {})
    for k in ("lr", "clip_grad_norm", "skip_nonfinite", "flat"):
        if k in args:
            raise ValueError(f"optimizer_args: '{k}' is an argument of the step itself")
    lr_fn = lr if callable(lr) else None
    args.update(lr=0.0 if lr_fn is not None else lr, clip_grad_norm=clip_grad_norm, skip_nonfinite=skip_nonfinite)
    if optimizer in ("adam", "adamw"):
        if "decoupled_weight_decay" in args and bool(args["decoupled_weight_decay"]) != (optimizer == "adamw"):
            raise ValueError(f"optimizer='{optimizer}' conflicts with decoupled_weight_decay={args['decoupled_weight_decay']}")
        args["decoupled_weight_decay"] = optimizer == "adamw"
        return FlatAdam(flat, **args), lr_fn
    if optimizer == "sgd":
        return FlatSGD(flat, **args), lr_fn
    raise ValueError(f"optimizer must be 'adam', 'adamw' or 'sgd', got {optimizer!r}")


class BatchedRepack:
    """After an optimizer step every conv layer's packed weight images are stale; instead of one small launch per layer at
    its next forward (23 per step for cfg2) ONE launch rebuilds the matrix-core layers' images (mednet_conv3d_pack_many).
    The device table of (parameter, pack buffer, shape) is built once: parameters live in the flat buffer and the pack
    buffers are rewritten in place.  Layers without matrix-core images (first conv, 1x1x1 head) keep the per-layer path."""

    ENABLED = os.environ.get("MEDNET_BATCHED_PACK", "1") == "1"  # A/B knob
    # 16-bit storage modes: rewrite only the images the step's matrix-core kernels read (MEDNET_PACK_HIGH_ONLY) -- not the fp32
    # images of the direct / fp32-matrix kernels nor unrequested low images: 1.1 GB instead of 2.8 GB per step for config 5's 141 M
    # parameters.  The buffers are marked (`_mednet_lean`) and nn._PackedWeightMixin._packed(x) re-packs a layer in full before a
    # call that would read anything else.  Only when EVERY layer of the table always takes the matrix-core path on 16-bit tensors.
    LEAN = os.environ.get("MEDNET_LEAN_PACK", "1") == "1"

    def __init__(self, model):
        from . import nn as hnn
        self.mods = [m for m in model.modules() if isinstance(m, hnn._PackedWeightMixin) and m.kernel_size[0] == 3
                     and m.weight.shape[0] % 16 == 0 and m.weight.shape[1] % 16 == 0]
        self.sig = None
        self.table = None
        self.max_blocks = 0

    def _signature(self):
        from . import config
        return tuple((m.weight.data_ptr(), m._pack_buf.data_ptr()) for m in self.mods) + (config.act_dtype(), config.split_weights())

    def run(self):
        """Call right after the parameters changed (same stream).  No-op until every layer has been packed once."""
        import ctypes as C
        from . import _lib as L, config
        if not self.ENABLED or not self.mods or any(getattr(m, "_pack_buf", None) is None for m in self.mods):
            return
        lib = L.lib()
        sig = self._signature()
        if sig != self.sig:
            class Job(C.Structure):
                _fields_ = [("w", C.c_void_p), ("packed", C.c_void_p), ("cin", C.c_int), ("cout", C.c_int), ("ksize", C.c_int),
                            ("transposed_src", C.c_int)]
            jobs = (Job * len(self.mods))()
            for j, m in zip(jobs, self.mods):
                w = m.weight
                cin, cout = (w.shape[0], w.shape[1]) if m._transposed else (w.shape[1], w.shape[0])
                j.w, j.packed, j.cin, j.cout, j.ksize, j.transposed_src = w.data_ptr(), m._pack_buf.data_ptr(), cin, cout, 3, int(m._transposed)
            host = torch.empty(lib.mednet_conv3d_pack_table_bytes(len(self.mods)), dtype=torch.uint8)
            mb = C.c_uint(0)
            L.check(lib.mednet_conv3d_pack_table(C.addressof(jobs), len(self.mods), host.data_ptr(), C.addressof(mb)), "pack_table")
            self.table = host.to(self.mods[0].weight.device)
            self.max_blocks, self.sig = mb.value, sig
        elt = config.pack_elt()  # (fp32 storage: bf16 + the low images; fp16x2: fp16 + the low images)
        lean = self.LEAN and config.is_half_mode() and all(m._lean_layer_ok() for m in self.mods)
        L.check(lib.mednet_conv3d_pack_many(self.table.data_ptr(), len(self.mods), self.max_blocks, elt | (L.PACK_HIGH_ONLY if lean else 0),
                                            L.stream()), "pack_many")
        for m in self.mods:  # what _PackedWeightMixin._packed() will compute at the next forward
            w = m.weight
            m._pack_key = (w.data_ptr(), w._version, getattr(w, "_mednet_step", 0), str(w.device), config.act_dtype(), config.pack_elt())
            m._pack_buf._mednet_lean = lean


class LossScaler:
    """Dynamic loss scaling for fp16 storage (BASELINE config 5; the reference's hint is the commented-out `precision=16` of
    examples/train_seg.py:127).  torch.cuda.amp.GradScaler's rule -- scale 2^16, halve on overflow, double after 2000 clean
    steps -- with the whole state on the device: the loss is multiplied by a device scalar, the overflow test, the decision
    to skip the update and the scale update are kernels (mednet_adam_step_scaled), so a step never waits for the host."""

    def __init__(self, device, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        self.state = torch.tensor([init_scale, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=device)
        self.growth_factor, self.backoff_factor, self.growth_interval = growth_factor, backoff_factor, growth_interval

    def state_dict(self):
        """Everything a resumed run needs (synchronises): the device state {scale, good steps, optimizer steps taken,
        found_inf, skipped steps} and the rule's constants."""
        return {"state": self.state.detach().cpu().clone(), "growth_factor": self.growth_factor,
                "backoff_factor": self.backoff_factor, "growth_interval": self.growth_interval}

    def load_state_dict(self, sd):
        st = sd["state"].to(self.state.device).reshape(-1)
        if st.numel() > self.state.numel():
            raise ValueError(f"LossScaler.load_state_dict: saved state has {st.numel()} entries, this build keeps {self.state.numel()}")
        # (earlier builds kept 4 entries {scale, good steps, steps taken, found_inf}; the counters added since start at 0)
        self.state.zero_()
        self.state[:st.numel()].copy_(st)
        self.growth_factor, self.backoff_factor = sd["growth_factor"], sd["backoff_factor"]
        self.growth_interval = sd["growth_interval"]

    def skipped_steps(self) -> int:
        """Steps whose update was skipped for non-finite gradients (synchronises)."""
        return int(self.state[4].item())

    def scale_loss(self, loss):
        return loss * self.state[0]

    def snapshot(self):
        """(scale, good steps, optimizer steps taken, found_inf) -- synchronises; for tests and logging only."""
        return tuple(float(v) for v in self.state[:4].tolist())


def make_scaler(device):
    from . import config
    return LossScaler(device) if config.act_dtype() == torch.float16 else None


def finish_backward():
    """Join the weight-gradient side stream (ops.SIDE) before anything reads the flat gradient buffer."""
    ops.join_side_stream()


def allreduce_gradients(flat_grad: torch.Tensor, world_size: int, force: bool = False):
    """The data-parallel exchange: ONE all-reduce(sum) of the flat gradient buffer (RCCL over xGMI on GPUs; any
    torch.distributed backend in tests).  Returns the scale the optimizer must apply (1/world) so that the update uses
    the mean of the per-rank-batch gradients -- what PL's DDP does with the reference (Dice is reduced
    over the LOCAL batch, then gradients are averaged)."""
    if world_size > 1 or force:
        dist.all_reduce(flat_grad, op=dist.ReduceOp.SUM)
    return 1.0 / world_size


def late_bucket_split(model, flat: FlatParams, levels: int = 2):
    """Element offset in the flat buffers that separates the parameters whose gradients arrive LAST in backward -- the
    first `levels` encoders, which are the first parameters in module order -- from all the others.  For the U-Nets of
    the path the late bucket is tiny (cfg2: 0.34 M of 8.77 M parameters) while its backward is the longest stretch (the
    two full-resolution levels), so everything else can be exchanged underneath it.  None when the model has no such
    structure."""
    encs = getattr(model, "encoders", None)
    if encs is None or len(encs) <= levels:
        return None
    late = {id(p) for enc in list(encs)[:levels] for p in enc.parameters() if p.requires_grad}
    k = 0
    while k < len(flat.params) and id(flat.params[k]) in late:
        k += 1
    if k != len(late) or k == 0 or k == len(flat.params):
        return None  # not a prefix of the flat order: keep the single exchange
    return flat.offsets[k]


class BucketedExchange:
    """Two-bucket gradient exchange overlapped with backward.

    When autograd delivers the gradient of encoder[levels-1]'s output, every parameter outside the first `levels` encoders
    has its gradient launched: that slice of the flat buffer (cfg2: 96 % of the bytes) is all-reduced asynchronously --
    issued behind the weight-gradient stream, so RCCL waits for exactly the kernels that produce it -- while the backward
    of the full-resolution encoders runs.  The small remainder is exchanged after backward; `finish()` makes the
    compute stream wait for both.  Sums are identical to the single exchange (disjoint slices)."""

    def __init__(self, model, flat: FlatParams, world_size: int, force: bool = False, levels: int = 2):
        self.flat, self.world, self.work, self.force = flat, world_size, None, bool(force)
        self.split = late_bucket_split(model, flat, levels) if (world_size > 1 or force) else None
        # The overlapped form is OPT-IN (MEDNET_BUCKETS=1) until a multi-GPU measurement exists.  One-rank RCCL rehearsal on an
        # MI355X, round 4 (profiles/r04_ab.md section 15, after the side stream got a hardware queue of its own under a
        # process group): one all-reduce after backward 20.55 ms per step, two buckets 20.69 ms, no process group 20.58 -- the
        # collective inside backward costs the compute stream ~0.14 ms there, against a ring time over xGMI of ~0.4-1.2 ms
        # for cfg3's 35 MB that it would hide (the round-3 figure of 0.6 ms was taken with both streams on one queue).  For
        # cfg5 (565 MB, ~6.5 ms single-ring against a 47 ms step) hiding the exchange under the backward
        # of the full-resolution encoders is the obvious candidate -- to be switched on by a scaling run, not by a guess
        # (ADVICE r3).
        self.enabled = self.split is not None and self.overlap_selected(flat.total * 4)
        if self.enabled:
            list(model.encoders)[levels - 1].register_forward_hook(self._on_forward)

    @classmethod
    def overlap_selected(cls, grad_bytes: int) -> bool:
        """MEDNET_BUCKETS=1 selects the two-bucket overlapped exchange (any size); default: one all-reduce after backward."""
        return os.environ.get("MEDNET_BUCKETS") == "1"

    def describe(self) -> str:
        """For bench records: which exchange this step runs."""
        if not (self.world > 1 or self.force):
            return "none (1 rank)"
        mb = self.flat.total * 4 / 1e6
        if self.enabled:
            early = (self.flat.total - self.split) * 4 / 1e6
            return (f"2 buckets: {early:.1f} MB all-reduced under the backward of the full-resolution encoders, "
                    f"{mb - early:.1f} MB after backward")
        return f"one all-reduce of the flat fp32 gradient buffer ({mb:.1f} MB) after backward"

    def _on_forward(self, module, inputs, output):
        if isinstance(output, tuple):  # Encoder(x, with_skip=True) -> (skip, out): the hook belongs on the level's output
            output = output[-1]
        if self.enabled and torch.is_tensor(output) and output.requires_grad:
            output.register_hook(self._on_grad)

    def _on_grad(self, grad):
        early = self.flat.grad[self.split:]
        if self.work is None and not (early.is_cuda and torch.cuda.is_current_stream_capturing()):
            if early.is_cuda:
                main = torch.cuda.current_stream(early.device)
                side = ops.side_stream(early.device)
                side.wait_stream(main)  # main-stream gradients of the early bucket (GroupNorm affines, biases)
                with torch.cuda.stream(side):
                    self.work = dist.all_reduce(early, op=dist.ReduceOp.SUM, async_op=True)
            else:
                self.work = dist.all_reduce(early, op=dist.ReduceOp.SUM, async_op=True)
        return None

    # bench.py's `rccl` record: a list to which finish() appends (start, end) HIP events around the exchange on the compute
    # stream (the early bucket of the two-bucket form runs inside backward and is not in them: the record says which form ran)
    TIMING = None

    def finish(self):
        """After backward (and the side-stream join): exchange what is left, wait for the early bucket; -> 1/world."""
        timed = (BucketedExchange.TIMING is not None and (self.world > 1 or self.force) and self.flat.grad.is_cuda
                 and not torch.cuda.is_current_stream_capturing())
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        scale = self._finish()
        if timed:
            e1.record()
            BucketedExchange.TIMING.append((e0, e1))
        return scale

    def _finish(self):
        if self.work is not None:
            dist.all_reduce(self.flat.grad[:self.split], op=dist.ReduceOp.SUM)
            self.work.wait()
            self.work = None
        elif self.world > 1 or self.force:
            dist.all_reduce(self.flat.grad, op=dist.ReduceOp.SUM)
        return 1.0 / self.world


class _GraphedStep:
    """hipGraph capture of forward + loss + backward (everything up to the gradient exchange).

    A step is ~330 kernel launches from Python; the GPU stays ahead of the host only while the host is not disturbed.
    After `warm` eager calls the launch sequence of `_fwd_bwd` (both streams: the weight-gradient side stream forks from
    and re-joins the capture stream) is captured once and replayed with one call per step.  The all-reduce and the
    Adam launch stay outside the graph (Adam's bias correction is computed on the host from the step count).
    Shapes and dtypes of the batch must not change after capture; a new batch tensor is copied into the static one."""

    GRAPH_DEFAULT = os.environ.get("MEDNET_GRAPH", "0") == "1"

    def _setup(self, model, world_size, graph, optimizer, optimizer_args, lr, clip_grad_norm, skip_nonfinite, warm=2):
        """What every step class is built from, after its criteria: flat parameters, optimiser, repack, world, side stream, scaler,
        graph state and the (lazily built) gradient exchange."""
        self.model = model
        self.flat = FlatParams(model)
        self.opt, self._lr_fn = make_optimizer(self.flat, optimizer, optimizer_args, lr, clip_grad_norm, skip_nonfinite)
        self._opt_calls = 0
        self.repack = BatchedRepack(model)
        self.world = world_size
        use_side_stream()
        self.scaler = make_scaler(self.flat.flat.device)  # fp16 storage only
        self.use_graph = self.GRAPH_DEFAULT if graph is None else bool(graph)
        self._calls, self._warm, self._graph, self._static = 0, warm, None, None
        self._exchange = None

    def __call__(self, batch):
        """run, exchange, optimiser, repack -> the detached losses of _fwd_bwd."""
        if self._exchange is None:  # (built lazily: bench.py sets force_allreduce after construction)
            self._exchange = BucketedExchange(self.model, self.flat, self.world, getattr(self, "force_allreduce", False))
        out = self._run(batch)
        scale = self._exchange.finish()  # 1/world is folded into the optimiser (and into the gradient norm in front of it)
        self._optimizer_step(scale)
        self.repack.run()
        return out

    def _backward(self, loss):
        """The tail of every _fwd_bwd: backward of the (scaled) loss, then the side-stream join."""
        (loss if self.scaler is None else self.scaler.scale_loss(loss)).backward()
        finish_backward()

    def _run(self, batch):
        """-> tuple of detached loss tensors of this step's forward/backward (gradients are in self.flat.grad)."""
        self.flat.verify()  # (every call, capture and replay included: requires_grad must be what the flat buffers were built for)
        if not self.use_graph:
            return self._fwd_bwd(batch)
        self._calls += 1
        if self._graph is None:
            if self._calls <= self._warm:
                return self._fwd_bwd(batch)
            ops.PROFILE["enabled"] = False  # timing events cannot be recorded into a graph
            self._static = {k: v for k, v in batch.items()}
            torch.cuda.synchronize()
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):
                self._out = self._fwd_bwd(self._static)
        for k, v in batch.items():
            if v is not self._static[k]:
                self._static[k].copy_(v)
        self._graph.replay()
        return self._out

    # ---- the optimiser of a step (outside the graph: lr and the step count are kernel arguments / device state)
    def _optimizer_step(self, scale):
        if self._lr_fn is not None:
            self.opt.lr = float(self._lr_fn(self._opt_calls))  # (host arithmetic, once per call)
        self._opt_calls += 1
        if self.scaler is None:
            self.opt.step(grad_scale=scale)
        else:
            self.opt.step_scaled(self.scaler, inv_world=scale)

    def _norm_runs(self) -> bool:
        return self.opt._norm_runs(self.scaler)

    @property
    def grad_norm(self):
        """Device scalar: the last step's global L2 norm of the mean gradient (unscaled, after the exchange's 1/world) BEFORE
        clipping.  Reading the attribute synchronises nothing; float() / .item() of it does."""
        if not self._norm_runs():
            raise RuntimeError("grad_norm: this step takes no gradient norm (pass clip_grad_norm=... or skip_nonfinite=True)")
        return self.opt.opt_state[1]

    def skipped_steps(self) -> int:
        """Updates skipped for non-finite gradients so far (synchronises)."""
        if self.scaler is not None:
            return self.scaler.skipped_steps()
        return int(self.opt.opt_state[5].item()) if self._norm_runs() else 0


def use_side_stream():
    """Weight gradients on their own stream (ops.SIDE) for every step class: MEDNET_SIDE_STREAM=0 turns it off."""
    ops.SIDE["enabled"] = os.environ.get("MEDNET_SIDE_STREAM", "1") == "1"


def _call_is_hooked(model, final_conv) -> bool:
    """The fused head + loss nodes call model.forward_features() and never final_conv: they bypass `model.__call__` and
    `final_conv.__call__`, and in the landmark form no `outputs` tensor exists at all.  Any forward hook / pre-hook registered on
    those two modules, or a global module hook, would silently not fire -- the steps then take the stock `model(inputs)` path.
    (Hooks on encoder / decoder children still fire in the fused form: forward_features calls them through __call__.)"""
    import torch.nn.modules.module as M
    for name in ("_global_forward_hooks", "_global_forward_pre_hooks", "_global_forward_hooks_always_called"):
        if getattr(M, name, None):
            return True
    return any(bool(getattr(mod, attr, None)) for mod in (model, final_conv) for attr in ("_forward_hooks", "_forward_pre_hooks"))


def _class_criterion(loss, w):
    """The class criterion of a step: "DICE" -> DiceLoss, "DICE_CE" -> DiceCELoss (Dice + cross-entropy, one class-weight vector),
    anything else the nn.CrossEntropyLoss(weight) of segmentation.py:49 / landmarks.py:49."""
    if loss == "DICE_CE":
        return HL.DiceCELoss(weight=w)
    return HL.DiceLoss(weight=w) if loss == "DICE" else HL.CrossEntropyLoss(weight=w)


def _class_spec(crit):
    """A class criterion as the fused nodes take it: its kind ("DICE" | "CE" | "DICE_CE"; None: not one of this package's three) and
    the keyword arguments it sets -- loss_weight, eps, sigmoid, ignore_index; what a kind does not set stays at the nodes' defaults
    (CE: the default eps, its own ignore_index; Dice + CE: its eps, no ignore, no sigmoid)."""
    if isinstance(crit, HL.DiceCELoss):
        return "DICE_CE", dict(loss_weight=crit.weight, eps=crit.epsilon)
    if isinstance(crit, HL.DiceLoss):
        return "DICE", dict(loss_weight=crit.weight, eps=crit.epsilon, sigmoid=crit.sigmoid_normalization, ignore_index=crit.ignore_index)
    if isinstance(crit, HL.CrossEntropyLoss):
        return "CE", dict(loss_weight=crit.weight, ignore_index=crit.ignore_index)
    return None, {}


def _head_fusable(model, crit, inputs) -> bool:
    """The conditions every fused head + loss node shares: this package's U-Net, not testing, a planar 1x1x1 head, one of the three
    class criteria (DiceLoss without skip_last_target), CUDA, and no hook that the node would bypass (_call_is_hooked)."""
    from .unet.model import _UNetCore
    fc = getattr(model, "final_conv", None)
    return (isinstance(model, _UNetCore) and not model.testing and _class_spec(crit)[0] is not None
            and not getattr(crit, "skip_last_target", False) and fc is not None and getattr(fc, "planar_output", False)
            and fc.kernel_size[0] == 1 and inputs.is_cuda and not _call_is_hooked(model, fc))


def deep_supervision_weights(k, ds_weights=None):
    """The level weights w_0 .. w_k of a deep-supervision loss: 2^-s / sum_t 2^-t by default, or `ds_weights` (k + 1 non-negative
    numbers, used as given)."""
    if ds_weights is None:
        total = sum(2.0 ** -t for t in range(k + 1))
        return [2.0 ** -s / total for s in range(k + 1)]
    ws = [float(v) for v in ds_weights]
    if len(ws) != k + 1:
        raise ValueError(f"ds_weights: {k + 1} weights expected (levels 0 .. {k}), got {len(ws)}")
    if any(not v >= 0.0 for v in ws):
        raise ValueError(f"ds_weights must be non-negative, got {ws}")
    return ws


class SegmentationStep(_GraphedStep):
    """One data-parallel training step of SegmentationNet (segmentation.py:58-65) on the MI355X path.

    optimizer: "adam" (the reference's rule and the default), "adamw" or "sgd"; optimizer_args: a dict for FlatAdam / FlatSGD
    (betas, eps, weight_decay / momentum, nesterov, weight_decay; weight decay defaults to 0 for all three).  lr: a float, or a callable
    lr(call_index) -> float such as PolyLR, evaluated on the host once per call -- the optimiser launch is outside the captured graph,
    so a changing lr is graph-safe.  clip_grad_norm: clip the mean gradient to this global L2 norm (taken after the gradient exchange
    with 1/world folded in, so every rank clips by the same number; of the UNSCALED gradient in fp16 storage).  skip_nonfinite: skip
    the update when a gradient is NaN / inf, in any storage mode.  Neither makes the step wait for the host: `grad_norm` is a device
    scalar, `skipped_steps()` synchronises.  With the defaults the step launches exactly what it always launched."""

    def __init__(self, model, loss_weight=None, lr=1e-3, loss="DICE", world_size=1, graph=None, optimizer="adam", optimizer_args=None,
                 clip_grad_norm=None, skip_nonfinite=False, ds_weights=None):
        dev = next(model.parameters()).device
        w = None if loss_weight is None else torch.tensor(loss_weight, dtype=torch.float32, device=dev)
        self.loss = _class_criterion(loss, w).to(dev)
        # deep supervision (a model built with deep_supervision=k): loss = sum_s w_s L_s over the levels 0 .. k, w_s = 2^-s / sum_t 2^-t
        # unless `ds_weights` gives them; scale_losses = the detached, unweighted L_0 .. L_k of the last step (device scalars)
        self.ds_weights = deep_supervision_weights(len(getattr(model, "ds_heads", ())), ds_weights)
        self.scale_losses = []
        self._setup(model, world_size, graph, optimizer, optimizer_args, lr, clip_grad_norm, skip_nonfinite)

    def _head_loss(self, inputs, label_u8):
        """`outputs = self(inputs); loss = self.loss(outputs, labels)` (segmentation.py:61-62).  When the model is this package's
        U-Net with a 1x1x1 head of at most 4 classes and the loss is DiceLoss, CrossEntropyLoss or DiceCELoss, the head and the loss run
        as one fused node (ops.head_dice / ops.head_ce / ops.head_dice_ce: logits written once, no logit-gradient tensor, the label
        volume's uint8 channel consumed where it lies); with 5 to 16 classes on a 32-feature head in a 16-bit storage mode they run as the matrix-core node
        ops.head_seg, which writes no logit tensor at all: `outputs` is None in that form (as LandmarkStep has no outputs tensor).
        Anything else takes the two calls as they stand."""
        m, fc = self.model, getattr(self.model, "final_conv", None)
        kind, kw = _class_spec(self.loss)
        if _head_fusable(m, self.loss, inputs):
            feats = m.forward_features(inputs)
            small = "head_" + kind.lower()  # ops.head_dice / head_ce / head_dice_ce: the fused heads of at most 4 classes
            if getattr(ops, small + "_supported")(feats, fc.in_channels, fc.out_channels, label_u8):
                return getattr(ops, small)(feats, fc.weight, fc.bias, fc._packed(), label_u8, **kw)
            if ops.head_seg_supported(feats, fc.in_channels, fc.out_channels, label_u8):
                return ops.head_seg(feats, fc.weight, fc.bias, fc._packed(), label_u8, class_loss=kind, **kw)
            outputs = fc(feats)
        else:
            outputs = m(inputs)
        # (Dice + CE consumes the uint8 labels where they lie)
        return outputs, self.loss(outputs, label_u8 if kind == "DICE_CE" else label_u8.long())

    def _ds_level(self, s, feats, label_u8, inputs, aux):
        """Level s >= 1 of deep supervision, called from the model's decoder loop on that level's block output: L_s = the step's
        criterion on ds_heads[s-1](feats) against the labels picked at stride 2^s -> aux[s]; returns the tensor that goes on to the
        next decoder.  Fused (ops.ds_head: one node at the junction, the full-resolution uint8 labels read where they lie) when
        ops.ds_head_supported says yes; otherwise -- fp32 storage, other label types, the ds_head_fuse knob at 0, hooked modules -- the
        composed form: the head, then the existing loss on a contiguous strided label slice."""
        head, crit = self.model.ds_heads[s - 1], self.loss
        kind, kw = _class_spec(crit)
        if (inputs.is_cuda and label_u8.dtype == torch.uint8 and not _call_is_hooked(self.model, head) and kind is not None
                and not getattr(crit, "skip_last_target", False)
                and ops.ds_head_supported(feats, head.in_channels, head.out_channels, label_u8, s)):
            feats, aux[s] = ops.ds_head(feats, head.weight, head.bias, head._packed(), label_u8, s, class_loss=kind, **kw)
            return feats
        d, h, w = feats.shape[2:]
        lab = label_u8[:, :d << s:1 << s, :h << s:1 << s, :w << s:1 << s].contiguous()
        aux[s] = crit(head(feats), lab if kind == "DICE_CE" else lab.long())
        return feats

    def _fwd_bwd(self, batch):
        inputs = batch["data"].float()
        label_u8 = batch["label"][:, -1, ...]
        k = len(self.ds_weights) - 1
        if k == 0:
            _, loss = self._head_loss(inputs, label_u8)
            self.scale_losses = [loss.detach()]
        else:
            from . import config
            aux = {}
            self.model._ds_tap = lambda s, feats: self._ds_level(s, feats, label_u8, inputs, aux)
            try:
                # fp32 storage asks for exact fp32 products under deep supervision (config.exact_products): a coarse level's loss
                # reaches the encoders above it through the max-pooling arg-max alone, one window entry in eight, and a window
                # whose two largest entries lie within the split-bf16 contraction's 2^-16 takes the other one; a single such
                # window of 2.6e5 moves the first block's gradients by sqrt(2 / 2.6e5) = 2.8e-3.  Nothing changes in 16-bit storage.
                with config.exact_products(not config.is_half_mode()):
                    _, aux[0] = self._head_loss(inputs, label_u8)
            finally:
                del self.model._ds_tap
            loss = aux[0] * self.ds_weights[0]
            for s in range(1, k + 1):
                loss = loss + aux[s] * self.ds_weights[s]
            self.scale_losses = [aux[s].detach() for s in range(k + 1)]
        self._backward(loss)
        return (loss.detach(),)

    def __call__(self, batch):
        (loss,) = super().__call__(batch)
        return loss


class _Validation:
    """What the two validation classes share: the evaluation-mode bracket, sample logging's arguments and rule, the `val_dice{c}`
    naming and validation_epoch_end."""

    def _setup(self, model, log_interval, log_vis_mip, on_samples):
        self.model = model
        self.log_interval, self.log_vis_mip, self.on_samples = log_interval, log_vis_mip, on_samples

    def _logs_samples(self, batch_nb) -> bool:
        """`if batch_nb % self.log_interval == 0` of the reference's validation_step, off without an interval or a callback."""
        return bool(self.log_interval) and self.on_samples is not None and batch_nb % self.log_interval == 0

    def _in_eval_mode(self, fn, *args):
        """fn(*args) with the model in evaluation mode; its training flag is put back whatever happens."""
        was_training = self.model.training
        self.model.eval()
        try:
            return fn(*args)
        finally:
            self.model.train(was_training)

    @staticmethod
    def _with_dice(results, per_channel_dice):
        for c in range(per_channel_dice.shape[0]):
            results[f"val_dice{c}"] = per_channel_dice[c]
        return results

    @staticmethod
    def validation_epoch_end(outputs):
        logs = {k: torch.stack([o[k] for o in outputs]).mean() for k in outputs[0]}
        return {"val_loss": logs["val_loss"], "log": logs, "progress_bar": logs}


class SegmentationValidation(_Validation):
    """SegmentationNet.validation_step / validation_epoch_end (segmentation.py:94-118) on the MI355X
    path: forward kernels only, the configured loss and `dice_metric` each as ONE fused pass over the logits, results as
    device scalars (no host synchronisation per batch).  Sample logging (`log_samples`, segmentation.py:67-92,100-101): with
    log_interval set, every batch with batch_nb % log_interval == 0 hands on_samples(panels, batch_nb) the vis.SamplePanels of
    sample 0 -- what the reference draws, computed on the device from `outputs` and the batch where they lie, still without a
    synchronisation; drawing and the one host copy (panels.to_host()) are the callback's.  log_vis_mip: the hparams' "mean" | "max".
    log_interval=None (the default) logs nothing; the results are the same either way."""

    def __init__(self, model, loss_weight=None, loss="DICE", log_interval=None, log_vis_mip="mean", on_samples=None):
        dev = next(model.parameters()).device
        w = None if loss_weight is None else torch.tensor(loss_weight, dtype=torch.float32, device=dev)
        self.loss = _class_criterion(loss, w).to(dev)
        self._setup(model, log_interval, log_vis_mip, on_samples)

    @torch.no_grad()
    def validation_step(self, batch, batch_nb=0):
        inputs = batch["data"].float()
        labels = batch["label"][:, -1, ...].long()
        outputs = self._in_eval_mode(self.model, inputs)
        if self._logs_samples(batch_nb):
            label = batch["label"]
            # (the class map: the label volume's last channel where it lies when the kernel reads its type, else the int64 copy)
            class_map = label[:, -1, ...] if label.dtype in (torch.uint8, torch.int64) else labels
            self.on_samples(vis.sample_panels(outputs, class_map, inputs, 0, projection_type=self.log_vis_mip), batch_nb)
        return self._with_dice({"val_loss": self.loss(outputs, labels)}, HL.dice_metric(outputs, labels))


def _landmark_losses(class_weight, regression_weight, class_loss, regression, dev):
    """LandmarkNet's two criteria (landmarks.py:43-56): DiceLoss, nn.CrossEntropyLoss(weight) or their sum for the class channels, the fused
    per-channel heat-map regression for the others."""
    if class_loss not in ("DICE", "CE", "DICE_CE"):
        raise ValueError(f"class_loss must be 'DICE', 'CE' or 'DICE_CE', not {class_loss!r}")
    w = torch.tensor(class_weight, dtype=torch.float32, device=dev)
    loss_class = _class_criterion(class_loss, w).to(dev)
    return loss_class, HL.HeatmapRegressionLoss(regression_weight, regression).to(dev)


def _landmark_head_fusable(model, loss_class, loss_reg, inputs) -> bool:
    """The fused landmark head: _head_fusable's conditions and L1 / L2 regression.  Its node never forms `outputs`: with a hook it
    would bypass, the stock m(inputs) path runs and the hook sees its tensor."""
    return _head_fusable(model, loss_class, inputs) and loss_reg.kind in ("L1", "L2")


class LandmarkStep(_GraphedStep):
    """LandmarkNet.training_step (landmarks.py:66-83, loss :125-134) with the per-channel regression loop fused.  class_loss:
    the hparams' `loss_class`, "DICE" (DiceLoss), "CE" (nn.CrossEntropyLoss(weight=class_weight)) or "DICE_CE" (their sum).  optimizer,
    optimizer_args, lr as a callable, clip_grad_norm and skip_nonfinite: as SegmentationStep's.  -> (loss, class loss, regression loss)."""

    def __init__(self, model, class_weight, regression_weight, regression="L2", lr=1e-3, world_size=1, graph=None, class_loss="DICE",
                 optimizer="adam", optimizer_args=None, clip_grad_norm=None, skip_nonfinite=False):
        self.class_loss = class_loss
        self.loss_class, self.loss_reg = _landmark_losses(class_weight, regression_weight, class_loss, regression,
                                                          next(model.parameters()).device)
        self._setup(model, world_size, graph, optimizer, optimizer_args, lr, clip_grad_norm, skip_nonfinite)

    def _head_losses(self, inputs, heatmaps, labels, nh):
        """`outputs = self(inputs)` and the two terms of LandmarkNet.loss (landmarks.py:71-75, 125-134).  In the 16-bit storage
        modes, with this package's U-Net, a 32-feature 1x1x1 head and uint8 targets, head and losses run as one fused node on the
        matrix cores (ops.head_landmark: no logit tensor); anything else takes the calls as they stand."""
        m, fc = self.model, getattr(self.model, "final_conv", None)
        if _landmark_head_fusable(m, self.loss_class, self.loss_reg, inputs):
            feats = m.forward_features(inputs)
            if ops.head_landmark_supported(feats, fc.in_channels, nh, fc.out_channels - nh, heatmaps, labels):
                kind, kw = _class_spec(self.loss_class)
                return ops.head_landmark(feats, fc.weight, fc.bias, fc._packed(), heatmaps, labels, kw.pop("loss_weight"),
                                         self.loss_reg.channel_weights, self.loss_reg.kind, class_loss=kind, **kw)
            outputs = fc(feats)
        else:
            outputs = m(inputs)
        out_hm, out_cls = ops.split_channels(outputs, nh)  # (= outputs[:, :nh], outputs[:, nh:]; one gradient join)
        return self.loss_class(out_cls, labels), self.loss_reg(out_hm, heatmaps)

    def _fwd_bwd(self, batch):
        inputs = batch["data"].float()
        heatmaps = batch["label"][:, :-1, ...]  # uint8 is consumed directly by the fused regression kernel
        nh = heatmaps.shape[1]
        labels = batch["label"][:, -1, ...]  # uint8, consumed where it lies (ops.dice_loss takes uint8 or int64 labels)
        if not labels.is_cuda:
            labels = labels.long()
        class_loss, regression_loss = self._head_losses(inputs, heatmaps, labels, nh)
        loss = regression_loss + class_loss
        self._backward(loss)
        return loss.detach(), class_loss.detach(), regression_loss.detach()


class LandmarkValidation(_Validation):
    """LandmarkNet.validation_step / validation_epoch_end (landmarks.py:136-174) on the MI355X path: forward kernels only, results
    as device scalars (no host synchronisation per batch).  With this package's
    U-Net and a head the fused landmark kernel serves (16-bit storage, 32 features), the head, both loss terms and dice_metric
    come from ONE pass over the features (ops.head_landmark_eval: no autograd node, no logit tensor); otherwise
    `outputs = model(inputs)` and the two losses and dice_metric as fused passes over its channel slices.
    Sample logging (`log_samples`, landmarks.py:85-123,148-149): log_interval, log_vis_mip and on_samples as for
    SegmentationValidation; the panels include the heat-map projections.  Where the step forms `outputs` the panels come from that
    tensor; on the fused path, which has no logit tensor, from final_conv(feats[0:1]) -- the head on the one sample that is drawn
    -- while the metric path stays as it is."""

    def __init__(self, model, class_weight, regression_weight, class_loss="DICE", regression="L2", log_interval=None,
                 log_vis_mip="mean", on_samples=None):
        self.class_loss = class_loss
        self.loss_class, self.loss_reg = _landmark_losses(class_weight, regression_weight, class_loss, regression,
                                                          next(model.parameters()).device)
        self._setup(model, log_interval, log_vis_mip, on_samples)

    def _log_samples(self, outputs, batch, inputs, nh, batch_nb, first=slice(None)):
        """`outputs`: the logits of the whole batch, or (first = slice(0, 1)) of its first sample alone."""
        label = batch["label"]
        if label.dtype != torch.uint8:  # (heat maps and class map of another type: the float / int64 forms the reference takes)
            panels = vis.sample_panels(outputs, label[first, -1].long(), inputs[first], nh, projection_type=self.log_vis_mip,
                                       heatmaps=label[first, :-1].float())
        else:
            panels = vis.sample_panels(outputs, label[first], inputs[first], nh, projection_type=self.log_vis_mip)
        self.on_samples(panels, batch_nb)

    def _forward(self, inputs, heatmaps, labels, nh, batch=None, batch_nb=None):
        m, fc = self.model, getattr(self.model, "final_conv", None)
        lc = self.loss_class
        kind, kw = _class_spec(lc)
        # (the Dice forward's sums serve dice_metric only when they are its sums: softmax, no ignore mask)
        metric_ok = kind != "DICE" or (not lc.sigmoid_normalization and lc.ignore_index is None)
        if metric_ok and _landmark_head_fusable(m, lc, self.loss_reg, inputs):
            feats = m.forward_features(inputs)
            if ops.head_landmark_supported(feats, fc.in_channels, nh, fc.out_channels - nh, heatmaps, labels):
                if batch is not None:
                    self._log_samples(fc(feats[0:1]), batch, inputs, nh, batch_nb, first=slice(0, 1))
                kw.pop("sigmoid", None)  # (False here, and the forward-only node takes none)
                return ops.head_landmark_eval(feats, fc.weight, fc.bias, fc._packed(), heatmaps, labels, kw.pop("loss_weight"),
                                              self.loss_reg.channel_weights, self.loss_reg.kind, class_loss=kind, **kw)
            outputs = fc(feats)
        else:
            outputs = m(inputs)
        if batch is not None:
            self._log_samples(outputs, batch, inputs, nh, batch_nb)
        out_hm, out_cls = outputs[:, :nh], outputs[:, nh:]
        return lc(out_cls, labels), self.loss_reg(out_hm, heatmaps), HL.dice_metric(out_cls, labels)

    @torch.no_grad()
    def validation_step(self, batch, batch_nb=0):
        inputs = batch["data"].float()
        heatmaps = batch["label"][:, :-1, ...]  # uint8, consumed where it lies
        nh = heatmaps.shape[1]
        labels = batch["label"][:, -1, ...]
        if not labels.is_cuda:
            labels = labels.long()
        class_loss, regression_loss, per_channel_dice = self._in_eval_mode(
            self._forward, inputs, heatmaps, labels, nh, batch if self._logs_samples(batch_nb) else None, batch_nb)
        return self._with_dice({"val_loss": regression_loss + class_loss, "val_class_loss": class_loss,
                                "val_regression_loss": regression_loss}, per_channel_dice)
