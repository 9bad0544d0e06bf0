"""torch.autograd.Function wrappers around the C ABI: one per fused device op of the U-Net path.

Every forward/backward here is a handful of libmednet_hip launches on torch's current HIP stream; PyTorch only
provides memory (caching allocator), the stream and the autograd graph.  Internal activations are channels-last
(`torch.channels_last_3d`: logical N,C,D,H,W, physical N,D,H,W,C) so the MFMA kernels read 16-byte channel
fragments; the network input (C=1) and the logits (written planar by the 1x1x1 head) are plain NCDHW.
"""
from __future__ import annotations

import contextlib
import os

import torch
from torch.autograd import Function

from . import _lib as L
from . import config, debug

CL = torch.channels_last_3d

# Optional profiling of the dominant kernel (bench.py): list of (start_event, end_event, flops) per matching launch
PROFILE = {"enabled": False, "events": [], "match": None}


# ---- weight gradients on a side stream (trainer mode only) ------------------------------------------------------------
# In the backward pass the weight gradient of a layer is off the critical path (nothing needs dW before the all-reduce /
# Adam), while the data gradient -> GroupNorm backward chain is HBM-bound.  When the trainer provides in-place gradient
# targets, weight-gradient kernels are launched on a second HIP stream so the matrix-core work overlaps the bandwidth
# work of the main stream.  train.py joins the streams before the gradient exchange.
# Workgroups of a weight-gradient launch on the side stream: HALF the CUs.  A weight-gradient workgroup takes a CU's whole
# register file; with one per CU nothing of the main stream -- not even the 32-workgroup reducer in front of a GroupNorm backward
# pass -- starts before they retire, and the two streams merely take turns.  With 128 the other 128 CUs run the bandwidth-bound
# GroupNorm passes of the main stream beside them, and the main stream's persistent kernels (256 / 512 workgroups) still divide
# evenly over what is left (profiles/r04_ab.md section 9: 144 or 192 are worse than 128 AND than 256).  0: the library's default.
SIDE = {"enabled": False, "stream": None, "keepalive": [], "wgrad_wgs": int(os.environ.get("MEDNET_SIDE_WGRAD_WGS", "128"))}


SIDE_MIN_VOXELS = int(os.environ.get("MEDNET_SIDE_MIN_VOXELS", "0"))  # (A/B knob: half-chip weight gradients from this layer size on)
SIDE_CORESIDENT = os.environ.get("MEDNET_SIDE_CORESIDENT", "1") == "1"  # (A/B knob: 0 = half the CUs for the co-resident kernel too)


def wgrad_coresident(n, d, h, w, cin, cout, ksize, x, dy) -> bool:
    return bool(L.lib().mednet_conv3d_wgrad_coresident(n, d, h, w, cin, cout, ksize, L.dt(x), L.dt(dy), config.conv_algo()))


def _runs_beside(main, cand, device) -> bool:
    """Does work queued on `cand` execute while `main` is busy?  HIP multiplexes its streams onto a few hardware queues (4 by
    default) in creation order; two streams that land on the same queue take turns whatever the program says."""
    x = torch.zeros(64, device=device)
    e0, em, ec = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    with torch.cuda.stream(cand):
        x.add_(1.0)  # (a stream's first launch creates its hardware queue: milliseconds that would read as "did not overlap")
    torch.cuda.synchronize(device)
    with torch.cuda.stream(main):
        e0.record(main)
        torch.cuda._sleep(3_000_000)  # main is busy for a millisecond or two
        em.record(main)
    with torch.cuda.stream(cand):
        x.add_(1.0)
        ec.record(cand)
    torch.cuda.synchronize(device)
    return e0.elapsed_time(ec) < 0.5 * e0.elapsed_time(em)


def side_stream(device):
    """The weight-gradient stream: a stream that really runs beside the current one.  With a process group up (RCCL and c10d have
    taken streams of their own by then) the first new stream shared the compute stream's hardware queue: the one-rank rehearsal
    of the data-parallel step ran every kernel on one queue, 23.7 ms instead of 20.5 (profiles/r04_ab.md section 15).  So the
    candidates are TESTED, once, at the first use (an eager warm-up step): up to 8 new streams, the first that overlaps wins."""
    if SIDE["stream"] is None:
        main = torch.cuda.current_stream(device)
        probe = os.environ.get("MEDNET_SIDE_PROBE", "1") == "1" and not torch.cuda.is_current_stream_capturing()
        cands, chosen = [], None
        prio = int(os.environ.get("MEDNET_SIDE_PRIORITY", "0"))  # (A/B knob: HIP stream priority of the weight-gradient stream)
        for _ in range(8 if probe else 1):
            c = torch.cuda.Stream(device=device, priority=prio) if prio else torch.cuda.Stream(device=device)
            cands.append(c)  # (kept alive until the choice is made: a released stream's slot would be handed out again)
            if not probe or _runs_beside(main, c, device):
                chosen = c
                break
        SIDE["stream"] = chosen if chosen is not None else cands[0]
        # True / False: MEASURED; None: the probe did not run (hipGraph capture, MEDNET_SIDE_PROBE=0) -- the first new stream is
        # taken on trust and may share the compute stream's hardware queue (bench.py reports the tri-state)
        SIDE["overlaps"] = (chosen is not None) if probe else None
        SIDE["candidates_tried"] = len(cands)
        if probe and chosen is None:  # no queue to itself: one workgroup per CU again (half the chip for twice as long gains nothing in turns)
            SIDE["wgrad_wgs"] = 0
    return SIDE["stream"]


def join_side_stream():
    if SIDE["stream"] is not None:
        torch.cuda.current_stream().wait_stream(SIDE["stream"])
    SIDE["keepalive"].clear()


class _OnSide:
    """Context: run the enclosed launches on the side stream after everything queued so far on the main stream."""

    def __init__(self, active, device, *tensors, coresident=False):
        # coresident: the enclosed launch leaves half of every CU free (mednet_conv3d_wgrad_coresident): it gets ALL the CUs, and
        # the main stream's bandwidth-bound passes run on the same CUs beside it (round 5; profiles/r05_ab.md)
        self.active, self.device, self.tensors, self.coresident = active, device, tensors, bool(coresident) and SIDE_CORESIDENT
        # the `workgroups` argument of the weight-gradient launch AND its workspace query inside this context (0: the library's
        # plan, one workgroup per CU -- a weight gradient launched on the main stream keeps the whole chip)
        self.workgroups = 0

    def __enter__(self):
        if self.active:
            main = torch.cuda.current_stream(self.device)
            side = side_stream(self.device)
            side.wait_stream(main)
            for t in self.tensors:
                if t is not None:
                    # Operands stay referenced until join_side_stream(), i.e. until the main stream has been made to
                    # wait for the side stream: (1) the caching allocator cannot recycle memory the side stream still
                    # reads (no Tensor.record_stream: its per-block events made every later allocation poll hundreds of
                    # events -- 9 of the host's 15 ms per step), and (2) autograd cannot accumulate INTO them: a
                    # gradient handed on to autograd (ConvTranspose's skip gradient is `dy` itself) is summed in place
                    # with later arrivals when nobody else holds it.
                    SIDE["keepalive"].append(t)
            self.ctx = torch.cuda.stream(side)
            self.ctx.__enter__()
            t = self.tensors[-1] if self.tensors else None
            vox = (t.shape[0] * t[0, 0].numel()) if (t is not None and t.dim() == 5) else 1 << 40
            if SIDE["wgrad_wgs"] > 0 and vox >= SIDE_MIN_VOXELS and not self.coresident:
                self.workgroups = SIDE["wgrad_wgs"]
        return self

    def __exit__(self, *exc):
        if self.active:
            self.ctx.__exit__(*exc)
        return False


class profiled_conv:
    """bench.py's live timing of the dominant kernel: HIP events on the launch stream around matching conv launches."""

    def __init__(self, ksize, cin, cout, n, d, h, w):
        self.on = PROFILE["enabled"] and PROFILE["match"] is not None and PROFILE["match"](ksize, cin, cout, d, h, w)
        self.flops = 2.0 * n * d * h * w * cin * cout * ksize ** 3

    def __enter__(self):
        if self.on:
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.on:
            self.e1.record()
            PROFILE["events"].append((self.e0, self.e1, self.flops))
        return False


class profiled_wgrad(profiled_conv):
    """The same for the weight gradient of matching layers (bench.py's second roofline object): the events go on the stream the
    launch runs on -- inside _OnSide that is the weight-gradient stream, where the kernel shares the CUs with the main stream's
    bandwidth-bound passes."""

    def __init__(self, ksize, cin, cout, n, d, h, w):
        super().__init__(ksize, cin, cout, n, d, h, w)
        self.on = self.on and PROFILE.get("wgrad_events") is not None

    def __exit__(self, *exc):
        if self.on:
            self.e1.record()
            PROFILE["wgrad_events"].append((self.e0, self.e1, self.flops))
        return False


class profiled_dgrad(profiled_conv):
    """The same for the DATA gradient of matching layers (bench.py's `roofline_dgrad` / `roofline.family`): `variant` names the
    epilogue the launch carries ("gn": GroupNorm-backward sums, "add+gn": summed residual gradient + sums, "plain")."""

    def __init__(self, variant, ksize, cin, cout, n, d, h, w):
        super().__init__(ksize, cin, cout, n, d, h, w)
        self.on = self.on and PROFILE.get("dgrad_events") is not None
        self.variant = variant

    def __exit__(self, *exc):
        if self.on:
            self.e1.record()
            PROFILE["dgrad_events"].append((self.e0, self.e1, self.flops, self.variant))
        return False


def _with_algo(backward):
    """backward of a conv-family Function: replays the algorithm choice (config.conv_algo()) captured at forward."""
    def wrapped(ctx, *grads):
        with config.algo_scope(getattr(ctx, "algo", None)):
            return backward(ctx, *grads)
    return wrapped


def _grad_target(param, shape):
    """Trainer hook (train.FlatParams): when a Parameter carries `_mednet_grad` (a contiguous fp32 view into the flat
    gradient buffer) the kernels write the gradient there and autograd gets None -> no copy / accumulate kernels."""
    tgt = getattr(param, "_mednet_grad", None)
    if tgt is not None:
        assert tuple(tgt.shape) == tuple(shape) and tgt.dtype == torch.float32 and tgt.is_contiguous()
        return tgt, True
    return torch.empty(shape, dtype=torch.float32, device=param.device), False


def to_cl(x: torch.Tensor) -> torch.Tensor:
    """Physical NDHWC. No-op for tensors produced by this package."""
    return x.contiguous(memory_format=CL)


def empty_cl(n, c, d, h, w, dtype, device):
    return torch.empty((n, c, d, h, w), dtype=dtype, device=device, memory_format=CL)


def _storage_dtype(x: torch.Tensor) -> torch.dtype:
    return config.act_dtype()


def _as_act(x: torch.Tensor) -> torch.Tensor:
    """Inputs that are neither fp32 nor the mode's 16-bit storage type (e.g. fp64 user tensors, bf16 in fp16 mode) are
    brought to the activation dtype."""
    if x.dtype == torch.float32 or x.dtype == config.act_dtype():
        return x
    return x.to(config.act_dtype())


def first_layer_input(x, cout, ksize, out_dtype, plain=True):
    """-> (tensor, layout) a 3x3x3 convolution reads its input from.  One channel: planar and channels-last coincide.  2-4 fp32
    channels into a 16-bit channels-last output (the multi-channel network input, mednet_conv3d_cm_supported; `plain`: no bias,
    output not planar): the kernels read the batch where it lies, planar or channels-last -- no layout copy.  Everything else is
    brought to channels-last."""
    cin = x.shape[1]
    if cin == 1:
        return x.contiguous(), L.NDHWC
    if (plain and 2 <= cin <= 4 and x.dtype == torch.float32 and out_dtype in config.HALF_TYPES
            and L.lib().mednet_conv3d_cm_supported(cin, cout, ksize, L.F32, L.dt_of(out_dtype), config.conv_algo())):
        if x.is_contiguous(memory_format=CL) and not x.is_contiguous():
            return x, L.NDHWC
        return x.contiguous(), L.NCDHW
    return to_cl(x), L.NDHWC


# ------------------------------------------------------------------------------------------------- weights
def pack_conv_weight(weight: torch.Tensor, ksize: int, transposed: bool, out: torch.Tensor = None) -> torch.Tensor:
    """PyTorch-layout fp32 weight -> opaque packed buffer read by the forward / data-gradient kernels (`out`: rewrite that buffer)."""
    L.require_gpu(weight, "pack_conv_weight")
    w = weight.detach()
    if w.dtype != torch.float32 or not w.is_contiguous():
        w = w.float().contiguous()
    cin, cout = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    nbytes = L.lib().mednet_conv3d_pack_bytes(cin, cout, ksize)
    if out is not None and (out.numel() != nbytes or out.device != w.device):
        raise RuntimeError("pack_conv_weight: `out` is not this layer's pack buffer")
    buf = out if out is not None else torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    # element type of the matrix-core fragment images; fp32 storage: bf16 high + low images (split-bf16 contraction); fp16x2: fp16 + low
    elt = config.pack_elt()
    L.check(L.lib().mednet_conv3d_pack_elt(w.data_ptr(), buf.data_ptr(), cin, cout, ksize, int(transposed), elt, L.stream()),
            "conv3d_pack")
    return buf


# ------------------------------------------------------------------------------------------------- Conv3d
class GN3Hook:
    """Carried by the output tensor of an ExtResNetBlock (`out._mednet_gn3`): lets the op that consumes `out` -- the 1x1x1
    head or the pooling + skip join -- take the first pass of the block's GroupNorm-3 backward while it produces the block's
    output gradient (mednet_head_dgrad_gn / mednet_pool2_bwd_gn).  The block's backward uses the sums only if the gradient it
    receives IS that tensor, untouched (same object, same version counter): any other consumer of `out` makes autograd
    accumulate into / replace it, and the block falls back to its stand-alone pass."""
    __slots__ = ("gn_in", "act", "partial", "dx", "version", "lazy", "lazy_head_ok")

    def __init__(self):
        self.gn_in = None  # the GroupNorm's input (y3 of an ExtResNetBlock; x of a plain GroupNorm)
        self.act = 0
        self.partial = self.dx = None
        self.version = -1
        # `dx` was NOT written, the block's apply pass rebuilds it: (dy_pool, skip gradient, pool mode) of SkipPool2Fn, or
        # ("head", ...) of the small fused heads (_valu_head_bwd)
        self.lazy = None
        # set by the producing block (block.res_block) when its own backward will consume the gradient of its output and the caller
        # hands that output to the head and to nothing else: the head's backward may then leave the gradient unwritten (LAZY_HEAD)
        self.lazy_head_ok = False

    def offer(self, dx, partial, lazy=None):
        self.dx, self.partial, self.version, self.lazy = dx, partial, dx._version, lazy

    def take(self, dout):
        """The sums, if `dout` is exactly the tensor they were taken from; releases the references either way.  A LAZY offer (the
        gradient tensor is a placeholder nobody wrote: SkipPool2Fn with sole_consumer) cannot be declined -- the caller asserted
        that the block output has no other consumer; a violated contract is an error, not a silent wrong gradient."""
        partial, dx, version, lazy = self.partial, self.dx, self.version, self.lazy
        self.partial = self.dx = self.lazy = None
        ok = partial is not None and dout is dx and dout._version == version
        if lazy is not None and not ok:
            raise RuntimeError("mednet_hip: the block output handed to skip_pool2(sole_consumer=True), or to a fused head as its sole "
                               "consumer, has another consumer (or its gradient was replaced by a hook): the pooling / head backward did "
                               "not materialise its gradient (MEDNET_LAZY_POOL=0 / MEDNET_LAZY_HEAD=0 turn the optimisation off)")
        GN3_COUNT["taken" if ok else ("declined" if partial is not None else "absent")] += 1
        GN3_COUNT["lazy_head"] += int(ok and lazy is not None and isinstance(lazy[0], str))
        self.lazy = lazy if ok else None  # (read and cleared by the block's backward)
        return partial if ok else None


FUSE_GN3 = os.environ.get("MEDNET_FUSE_GN3", "1") == "1"  # A/B knob


class GNBHook(GN3Hook):
    """The same contract for a plain GroupNorm (+ activation) whose output feeds a 3x3x3 convolution directly (the 'gcr'
    orders of UNet3D, components.py:12-67): the conv's data gradient takes {sum du, sum du * x} of that GroupNorm's backward
    in its epilogue (mednet_conv3d_dgrad_gn) and offers them with the gradient tensor it produced."""
    __slots__ = ("coef",)

    def __init__(self):
        super().__init__()
        self.coef = None


class BNBHook(GNBHook):
    """GNBHook of a BatchNorm (ops.batch_norm_act): `coef` rows are equal for all samples, and the consumer's per-sample rows are
    summed over samples as well (mednet_bn_act_bwd_fused).  A type of its own because the plain convolution (Conv3dFn) takes the
    first backward pass for these only -- the 'c b .' orders; a GroupNorm's hook is honoured where it always was."""
    __slots__ = ()


class ActMaskHook:
    """Carried by the output z of a fused conv -> activation layer: if z goes straight into a GroupNorm, that GroupNorm's
    backward multiplies the gradient it produces by act'(z) (z is its own input, in registers anyway) and says so here; the
    conv layer's backward then skips its activation-backward pass -- if the gradient it receives is that very tensor."""
    __slots__ = ("act", "dx", "version")

    def __init__(self, act):
        self.act, self.dx, self.version = act, None, -1

    def offer(self, dx):
        self.dx, self.version = dx, dx._version

    def take(self, dz):
        dx, version = self.dx, self.version
        self.dx = None
        ok = dx is not None and dz is dx and dz._version == version
        GN3_COUNT["masked"] += int(ok)
        return ok


def _gnb_hook_of(x, dtype):
    h = getattr(x, "_mednet_gnb", None) if FUSE_GN3 else None
    if h is None or h.gn_in is None or h.gn_in.shape != x.shape or h.gn_in.dtype != dtype or dtype not in config.HALF_TYPES:
        return None
    return h
# (tests: how the blocks' backward passes found their sums; "lazy_head": those of "taken" whose gradient the head left unwritten)
GN3_COUNT = {"taken": 0, "declined": 0, "absent": 0, "masked": 0, "lazy_head": 0}


def _gn3_hook_of(x, dtype):
    # (any storage type: the head's data gradient and the pooling backward take the sums in fp32 storage too; the
    #  ConvTranspose data gradient answers rows = 0 there and the block runs its stand-alone pass)
    h = getattr(x, "_mednet_gn3", None) if FUSE_GN3 else None
    if h is None or h.gn_in is None or h.gn_in.shape != x.shape or h.gn_in.dtype != dtype:
        return None
    return h


# One path for Conv3dFn, ConvActFn, ConvT3dFn and the ExtResNetBlock node (block.py): the fused partial rows (fused_partial_rows),
# the stride-1 forward (conv_forward), the stride-1 data gradient (conv_dgrad), the weight gradient (conv_wgrad) and the two
# gradients in the trainer's order (conv_backward).  What the call sites do differently comes in as arguments.
FUSE_GNB = os.environ.get("MEDNET_FUSE_GNB", "1") == "1"  # A/B knob: GroupNorm-backward sums in the data-gradient epilogue
WGRAD_FIRST = os.environ.get("MEDNET_WGRAD_FIRST", "1") == "1"  # A/B knob: launch order of the two gradients


def fused_partial_rows(n, d, h, w, cin, cout, ksize, x_dt, y_dt, device):
    """-> the rows [n][chunks][cout][2] that the convolution's epilogue fills with the GroupNorm sums of its output (saves a pass
    over y), or None when no kernel takes this call with them."""
    chunks = L.lib().mednet_conv3d_fused_stats_chunks(n, d, h, w, cin, cout, ksize, x_dt, y_dt, config.conv_algo())
    return torch.empty((n, chunks, cout, 2), dtype=torch.float32, device=device) if chunks > 0 else None


def _partial_out(ctx, partial, device):
    """A node's second output: autograd needs a tensor, so "no fused statistics" leaves as an empty one (_partial_in: back)."""
    if partial is None:
        partial = torch.empty(0, device=device)
    ctx.mark_non_differentiable(partial)
    return partial


def _partial_in(partial):
    return partial if partial.numel() else None


def conv_forward(x, x_layout, packed, bias, cout, ksize, out_planar, out_dtype, want_stats):
    """Stride-1 convolution of x (read in `x_layout`) -> (y, fused partial rows or None)."""
    n, cin, d, h, w = x.shape
    if out_planar:
        y = torch.empty((n, cout, d, h, w), dtype=out_dtype, device=x.device)
    else:
        y = empty_cl(n, cout, d, h, w, out_dtype, x.device)
    partial = fused_partial_rows(n, d, h, w, cin, cout, ksize, L.dt(x), L.dt(y), x.device) if want_stats else None
    with profiled_conv(ksize, cin, cout, n, d, h, w):
        L.check(L.lib().mednet_conv3d_fwd(x.data_ptr(), packed.data_ptr(), L.ptr(bias), y.data_ptr(), n, d, h, w, cin, cout, ksize,
                                          L.dt(x), x_layout, L.dt(y), L.NCDHW if out_planar else L.NDHWC, 0, config.conv_algo(),
                                          L.ptr(partial), L.stream()), "conv3d_fwd")
    return y, partial


def conv_dgrad(dy, packed, x_shape, cout, ksize, dx_dtype, dy_planar=False, head=None, gnb=None, add=None, profiled=False):
    """Data gradient of a stride-1 convolution whose input had `x_shape` -> (dx, partial rows or None), by the first form that
    applies:
      head = (y3, out, act): the convolution is the 1x1x1 head on an ExtResNetBlock's output `out` -- + the first pass of the block's
        GroupNorm-3 backward (mednet_head_dgrad_gn);
      gnb = (y_prev, coef_prev, act): x is act(norm(y_prev)) -- + the first pass of that GroupNorm's / BatchNorm's backward over the
        dx it stores, with or without `add` (mednet_conv3d_dgrad_gn; 16-bit storage: the bf16 / fp16 matrix-core kernel, fp32
        storage: the split-bf16 kernel);
      add: a second gradient of x, summed in the epilogue (mednet_conv3d_dgrad_add);
      plain.
    `profiled`: the launch counts for bench.py's data-gradient roofline."""
    n, cin, d, h, w = x_shape
    lib, algo = L.lib(), config.conv_algo()
    dx = empty_cl(n, cin, d, h, w, dx_dtype, dy.device)
    head_rows = lib.mednet_head_dgrad_gn_rows(n, d, h, w, cin, L.dt(dx)) if head is not None else 0
    gn_rows = 0
    if head_rows == 0 and gnb is not None and dx.dtype == dy.dtype and (add is None or add.dtype == dy.dtype):
        gn_rows = lib.mednet_conv3d_dgrad_gn_rows_dt(n, d, h, w, cin, cout, algo, L.dt(dy))
    rows = head_rows or gn_rows
    variant = ("add+gn" if add is not None else "gn") if rows > 0 else ("add" if add is not None else "plain")
    with profiled_dgrad(variant, ksize, cout, cin, n, d, h, w) if profiled else contextlib.nullcontext():
        partial = torch.empty((n, rows, cin, 2), dtype=torch.float32, device=dy.device) if rows > 0 else None
        if head_rows > 0:
            y3, out, act = head
            L.check(lib.mednet_head_dgrad_gn(dy.data_ptr(), packed.data_ptr(), dx.data_ptr(), y3.data_ptr(), out.data_ptr(), act,
                                             partial.data_ptr(), n, d, h, w, cin, cout, L.dt(dx), L.stream()), "head_dgrad_gn")
        elif gn_rows > 0:
            y_prev, coef_prev, act_prev = gnb
            L.check(lib.mednet_conv3d_dgrad_gn(dy.data_ptr(), packed.data_ptr(), L.ptr(add), dx.data_ptr(), y_prev.data_ptr(),
                                               coef_prev.data_ptr(), act_prev, partial.data_ptr(), n, d, h, w, cin, cout, algo,
                                               L.dt(dy), L.stream()), "conv3d_dgrad_gn")
        elif add is not None:
            L.check(lib.mednet_conv3d_dgrad_add(dy.data_ptr(), packed.data_ptr(), add.data_ptr(), dx.data_ptr(), n, d, h, w, cin, cout,
                                                algo, L.dt(dy), L.stream()), "conv3d_dgrad_add")
        else:
            L.check(lib.mednet_conv3d_fwd(dy.data_ptr(), packed.data_ptr(), None, dx.data_ptr(), n, d, h, w, cout, cin, ksize, L.dt(dy),
                                          L.NCDHW if dy_planar else L.NDHWC, L.dt(dx), L.NDHWC, 1, algo, None, L.stream()), "conv3d_dgrad")
    return dx, partial


def conv_wgrad(x, dy, weight_p, bias_p, ksize, x_layout=L.NDHWC, dy_planar=False, coresident=False, profiled=False, transposed=False,
               want_dw=True):
    """Weight (and, with `bias_p`, bias) gradient of a stride-1 convolution or (`transposed`) of ConvTranspose3d -> (dw, db), each None
    when the kernel wrote it into the trainer's buffer (_grad_target).  With in-place targets for everything it writes, the launch
    goes to the side stream; `coresident`: the caller wants all CUs for it there when the kernel leaves room beside it
    (wgrad_coresident).  `profiled`: the launch counts for bench.py's weight-gradient roofline.  `want_dw=False`: a trainable bias
    behind a frozen weight -- the bias sum comes out of this entry, so it runs with a scratch dw that nobody gets (a rare path)."""
    n, cin, d, h, w = x.shape
    cout = dy.shape[1]
    lib = L.lib()
    w_shape = (cin, cout, 3, 3, 3) if transposed else (cout, cin, ksize, ksize, ksize)
    if want_dw:
        dw, direct_w = _grad_target(weight_p, w_shape)
    else:
        dw, direct_w = torch.empty(w_shape, dtype=torch.float32, device=dy.device), False
    db, direct_b = _grad_target(bias_p, (cout,)) if bias_p is not None else (None, False)
    on_side = SIDE["enabled"] and direct_w and (db is None or direct_b)
    cores = on_side and coresident and wgrad_coresident(n, d, h, w, cin, cout, ksize, x, dy)
    with _OnSide(on_side, dy.device, x, dy, coresident=cores) as side:
        if transposed:
            ws = L.workspace(lib.mednet_convt3d_wgrad_ws_bytes(n, d, h, w, cin, cout, side.workgroups), dy.device)
            L.check(lib.mednet_convt3d_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), L.ptr(db), n, d, h, w, cin, cout, L.dt(x),
                                             L.dt(dy), config.conv_algo(), side.workgroups, ws.data_ptr(), ws.numel(), L.stream()),
                    "convt3d_wgrad")
        else:
            ws = L.workspace(lib.mednet_conv3d_wgrad_ws_bytes(n, d, h, w, cin, cout, ksize, side.workgroups), dy.device)
            with profiled_wgrad(ksize, cin, cout, n, d, h, w) if profiled else contextlib.nullcontext():
                L.check(lib.mednet_conv3d_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), L.ptr(db), n, d, h, w, cin, cout, ksize,
                                                L.dt(x), x_layout, L.dt(dy), L.NCDHW if dy_planar else L.NDHWC, config.conv_algo(),
                                                side.workgroups, ws.data_ptr(), ws.numel(), L.stream()), "conv3d_wgrad")
    return (None if (direct_w or not want_dw) else dw), (None if direct_b else db)


def conv_backward(x, dy, packed, weight_p, need_dx, dx_dtype, add=None, gnb=None, x_layout=L.NDHWC, wgrad_first=False):
    """The two gradients of a 3x3x3 layer inside a block-style node (ExtResNetBlock, ConvActFn), launches counted for bench.py's
    rooflines: weight gradient (side stream in trainer mode) and data gradient (conv_dgrad's `add` / `gnb` forms), the weight
    gradient first if `wgrad_first`.  Queued behind the data gradient, the weight gradient overlaps the next GroupNorm backward
    (HBM-bound) instead of fighting the data gradient for the matrix cores.  -> (dx, dw-or-None, partial-or-None)."""
    dx = partial = None
    if need_dx and not wgrad_first:
        dx, partial = conv_dgrad(dy, packed, x.shape, dy.shape[1], 3, dx_dtype, gnb=gnb, add=add, profiled=True)
    dw, _ = conv_wgrad(x, dy, weight_p, None, 3, x_layout=x_layout, coresident=True, profiled=True)
    if need_dx and wgrad_first:
        dx, partial = conv_dgrad(dy, packed, x.shape, dy.shape[1], 3, dx_dtype, gnb=gnb, add=add, profiled=True)
    return dx, dw, partial


def block_dx_dtype(x):
    """Type of the data gradient inside a block-style node: x's own if that is fp32 or the storage type, else the storage type."""
    return x.dtype if x.dtype in (torch.float32, config.act_dtype()) else config.act_dtype()


class Conv3dFn(Function):
    """nn.Conv3d(k in {1,3}, stride 1, padding k//2)  -- components.py:8-9,44; model.py:77,179."""

    @staticmethod
    def forward(ctx, x, weight, bias, packed, ksize, out_planar, out_dtype, want_stats=False):
        L.require_gpu(x, "conv3d")
        ctx.algo = config.conv_algo()
        x = _as_act(x)
        n, cin, d, h, w = x.shape
        cout = weight.shape[0]
        # Cin == 1: NCDHW and NDHWC coincide, so the network input is consumed as it arrives; so are 2-4 fp32 channels
        xin, x_layout = first_layer_input(x, cout, ksize, out_dtype, plain=bias is None and not out_planar)
        y, partial = conv_forward(xin, x_layout, packed, bias, cout, ksize, out_planar, out_dtype,
                                  want_stats and bias is None and not out_planar)
        ctx.save_for_backward(xin, packed)
        ctx.x_layout = x_layout
        ctx.meta = (ksize, out_planar, cin, cout, bias is not None, x.dtype)
        ctx.params = (weight, bias)
        ctx.gn3 = _gn3_hook_of(x, xin.dtype) if (ksize == 1 and out_planar and xin is x) else None
        # 'c b .' orders: x is act(BatchNorm(y_prev)) of the layer before, this conv is followed by its own BatchNorm (no fused
        # activation, so it runs here and not in ConvActFn): its data gradient takes that BatchNorm's first backward pass
        ctx.gnb = None
        if ksize == 3 and not out_planar and xin is x:
            hook = _gnb_hook_of(x, xin.dtype)
            ctx.gnb = hook if isinstance(hook, BNBHook) else None
        if debug.TRACE is not None:
            debug.trace(f"conv3d.fwd k{ksize} {cin}->{cout}", y, partial)
        return (y, _partial_out(ctx, partial, x.device)) if want_stats else y

    @staticmethod
    @_with_algo
    def backward(ctx, dy, _dpartial=None):
        xin, packed = ctx.saved_tensors
        ksize, out_planar, cin, cout, has_bias, x_dtype = ctx.meta
        dy = dy.contiguous() if out_planar else to_cl(dy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            # the 1x1x1 head on a block's output (xin IS that output): + the first pass of the block's GroupNorm-3 backward; the 'c b .'
            # orders: + the first pass of the backward of the BatchNorm (+ activation) that produced xin
            hook, bnb = ctx.gn3, ctx.gnb
            head = None
            if hook is not None and dy.dtype == torch.float32 and x_dtype == xin.dtype and config.conv_algo() != L.ALGO_DIRECT:
                head = (hook.gn_in, xin, hook.act)
            dx, partial = conv_dgrad(dy, packed, xin.shape, cout, ksize, x_dtype, dy_planar=out_planar, head=head,
                                     gnb=None if bnb is None else (bnb.gn_in, bnb.coef, bnb.act))
            if partial is not None:
                (hook if head is not None else bnb).offer(dx, partial)
        want_db = has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_db:  # (a trainable bias behind a frozen weight still gets its gradient)
            weight, bias = ctx.params
            dw, db = conv_wgrad(xin, dy, weight, bias if want_db else None, ksize, x_layout=ctx.x_layout,
                                dy_planar=out_planar, coresident=not out_planar, want_dw=ctx.needs_input_grad[1])
        return dx, dw, db, None, None, None, None, None


def conv3d(x, weight, bias, packed, ksize, out_planar=False, out_dtype=None):
    return Conv3dFn.apply(x, weight, bias, packed, ksize, out_planar, out_dtype or config.act_dtype())


def conv3d_with_stats(x, weight, bias, packed, ksize):
    """conv + (when the kernel can) the GroupNorm partial sums of its output; returns (y, partial-or-None)."""
    y, partial = Conv3dFn.apply(x, weight, bias, packed, ksize, False, config.act_dtype(), True)
    return y, _partial_in(partial)


class ConvActFn(Function):
    """conv 3x3x3 (no bias) -> ReLU / LeakyReLU / ELU in ONE kernel (the conv's epilogue): the 'gcr'-style orders of
    components.py:12-67 (UNet3D).  Optionally also the GroupNorm partial sums of the ACTIVATED output, for the GroupNorm
    that opens the next SingleConv.  Backward: activation' from the saved output, then the conv's two gradients."""

    @staticmethod
    def forward(ctx, x, weight, packed, act, want_stats, mask=None):
        L.require_gpu(x, "conv3d+act")
        ctx.algo = config.conv_algo()
        ctx.mask = mask
        xin = to_cl(_as_act(x))
        ctx.gnb = _gnb_hook_of(x, xin.dtype) if xin is x else None
        n, cin, d, h, w = xin.shape
        cout = weight.shape[0]
        lib = L.lib()
        z = empty_cl(n, cout, d, h, w, config.act_dtype(), x.device)
        partial = fused_partial_rows(n, d, h, w, cin, cout, 3, L.dt(xin), L.dt(z), x.device) if want_stats else None
        with profiled_conv(3, cin, cout, n, d, h, w):
            L.check(lib.mednet_conv3d_act_fwd(xin.data_ptr(), packed.data_ptr(), z.data_ptr(), n, d, h, w, cin, cout, act,
                                              config.conv_algo(), L.ptr(partial), L.dt(z), L.stream()), "conv3d_act_fwd")
        ctx.save_for_backward(xin, packed, z)
        ctx.act = act
        ctx.weight = weight
        return z, _partial_out(ctx, partial, x.device)

    @staticmethod
    @_with_algo
    def backward(ctx, dz, _dpartial=None):
        xin, packed, z = ctx.saved_tensors
        masked = ctx.mask is not None and ctx.mask.take(dz)  # (before any conversion: identity matters)
        dz = to_cl(dz.to(z.dtype))
        if masked:  # the GroupNorm that consumed z already multiplied its input gradient by act'(z)
            du = dz
        else:
            du = torch.empty_like(z, memory_format=CL)
            L.check(L.lib().mednet_act_bwd(dz.data_ptr(), z.data_ptr(), du.data_ptr(), z.numel(), ctx.act, L.dt(z), L.stream()),
                    "act_bwd")
        hook = ctx.gnb
        dx, dw, partial = conv_backward(xin, du, packed, ctx.weight, ctx.needs_input_grad[0], block_dx_dtype(xin),
                                        gnb=(hook.gn_in, hook.coef, hook.act) if hook is not None and FUSE_GNB else None,
                                        wgrad_first=WGRAD_FIRST)
        if partial is not None:
            hook.offer(dx, partial)
        return dx, dw, None, None, None, None


def conv3d_act_supported(x, cin, cout):
    # mednet_conv3d_act_fwd reads and writes ONE 16-bit type.  An fp32 tensor handed to a bf16-mode layer (a block
    # called stand-alone, a 16/32-channel network input) takes the unfused conv, which passes its dtypes.
    if not (x.is_cuda and config.is_half_mode() and x.dtype == config.act_dtype() and x.dim() == 5):
        return False
    n, _, d, h, w = x.shape
    return bool(L.lib().mednet_conv3d_act_supported(n, d, h, w, cin, cout, config.conv_algo()))


def conv3d_act(x, weight, packed, act, want_stats=False):
    """-> (activated output, GroupNorm partials of it or None)."""
    mask = ActMaskHook(act) if (FUSE_GN3 and torch.is_grad_enabled() and act != L.ACT_NONE) else None
    z, partial = ConvActFn.apply(x, weight, packed, act, want_stats, mask)
    if mask is not None:
        z._mednet_actmask = mask
    return z, _partial_in(partial)


# ------------------------------------------------------------------------------------------------- ConvTranspose3d (+ skip add)
class ConvT3dFn(Function):
    """nn.ConvTranspose3d(k=3,s=2,p=1,output_padding=1) with the decoder's `x += encoder_features` fused into the
    epilogue  -- components.py:259-264,283-284."""

    @staticmethod
    def forward(ctx, x, weight, bias, skip, packed):
        L.require_gpu(x, "conv_transpose3d")
        ctx.algo = config.conv_algo()
        x0 = x
        x = to_cl(_as_act(x))
        ctx.gn3 = _gn3_hook_of(x0, x.dtype) if x is x0 else None
        n, cin, d, h, w = x.shape
        cout = weight.shape[1]
        y = empty_cl(n, cout, 2 * d, 2 * h, 2 * w, config.act_dtype(), x.device)
        sk = None
        if skip is not None:
            if tuple(skip.shape) != tuple(y.shape):
                raise RuntimeError(f"conv_transpose3d: skip shape {tuple(skip.shape)} != output {tuple(y.shape)}")
            sk = to_cl(skip.to(y.dtype))
        L.check(L.lib().mednet_convt3d_fwd(x.data_ptr(), packed.data_ptr(), L.ptr(bias), L.ptr(sk), y.data_ptr(), n, d, h,
                                           w, cin, cout, L.dt(x), L.dt(y), config.conv_algo(), L.stream()), "convt3d_fwd")
        ctx.save_for_backward(x, packed)
        ctx.meta = (cin, cout, bias is not None, skip is not None, None if skip is None else skip.dtype)
        ctx.params = (weight, bias)
        if debug.TRACE is not None:
            debug.trace(f"convt3d.fwd {cin}->{cout}", y)
        return y

    @staticmethod
    @_with_algo
    def backward(ctx, dy):
        x, packed = ctx.saved_tensors
        cin, cout, has_bias, has_skip, skip_dtype = ctx.meta
        n, _, d, h, w = x.shape
        dy = to_cl(dy)
        lib = L.lib()
        dx = dw = db = dskip = None
        if ctx.needs_input_grad[0]:
            dx = empty_cl(n, cin, d, h, w, x.dtype, dy.device)
            hook = ctx.gn3
            rows = 0
            if hook is not None and dy.dtype == dx.dtype:
                rows = lib.mednet_convt3d_dgrad_gn_rows(n, d, h, w, cin, cout, L.dt(dx), config.conv_algo())
            if rows > 0:  # + the first pass of the producing block's GroupNorm-3 backward (x IS that block's output)
                partial = torch.empty((n, rows, cin, 2), dtype=torch.float32, device=dy.device)
                L.check(lib.mednet_convt3d_dgrad_gn(dy.data_ptr(), packed.data_ptr(), dx.data_ptr(), hook.gn_in.data_ptr(),
                                                    x.data_ptr(), hook.act, partial.data_ptr(), n, d, h, w, cin, cout, L.dt(dx),
                                                    config.conv_algo(), L.stream()), "convt3d_dgrad_gn")
                hook.offer(dx, partial)
            else:
                L.check(lib.mednet_convt3d_dgrad(dy.data_ptr(), packed.data_ptr(), dx.data_ptr(), n, d, h, w, cin, cout,
                                                 L.dt(dy), L.dt(dx), config.conv_algo(), L.stream()), "convt3d_dgrad")
        want_db = has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_db:  # (a trainable bias behind a frozen weight still gets its gradient)
            weight, bias = ctx.params
            dw, db = conv_wgrad(x, dy, weight, bias if want_db else None, 3, transposed=True, want_dw=ctx.needs_input_grad[1])
        if has_skip and ctx.needs_input_grad[3]:
            dskip = dy if dy.dtype == skip_dtype else dy.to(skip_dtype)
        if debug.TRACE is not None:
            debug.trace(f"convt3d.bwd {cin}->{cout}", dx, ctx.gn3.partial if ctx.gn3 is not None else None)
        return dx, dw, db, dskip, None


def conv_transpose3d(x, weight, bias, skip, packed):
    return ConvT3dFn.apply(x, weight, bias, skip, packed)


# ------------------------------------------------------------------------------------------------- GroupNorm / BatchNorm3d (+act, +residual)
# One path for ops.GroupNormActFn, ops.BatchNormActFn and the ExtResNetBlock node (block.py): the statistics (gn_statistics; BatchNorm's
# are its own), the apply pass (norm_apply), the backward's buffers (_NormBackward) and its entries (gn_backward / bn_backward).
def gn_statistics(x, gamma, beta, groups, eps, partial=None):
    """-> (stats [n][groups][2], coef [n][c][2]) of GroupNorm over the channels-last x.  `partial`: the sums came out of the
    producer's epilogue (a convolution, upsample_concat) and only the finalize pass runs."""
    n, c, d, h, w = x.shape
    spatial = d * h * w
    lib = L.lib()
    stats = torch.empty((n, groups, 2), dtype=torch.float32, device=x.device)
    coef = torch.empty((n, c, 2), dtype=torch.float32, device=x.device)
    ws = L.workspace(lib.mednet_gn_ws_bytes(n, c, spatial), x.device)
    if partial is not None:
        L.check(lib.mednet_gn_finalize(partial.data_ptr(), partial.shape[1], L.ptr(gamma), L.ptr(beta), stats.data_ptr(),
                                       coef.data_ptr(), n, spatial, c, groups, eps, ws.data_ptr(), ws.numel(),
                                       L.stream()), "gn_finalize")
    else:
        L.check(lib.mednet_gn_stats(x.data_ptr(), L.ptr(gamma), L.ptr(beta), stats.data_ptr(), coef.data_ptr(), n,
                                    spatial, c, groups, eps, L.dt(x), ws.data_ptr(), ws.numel(), L.stream()), "gn_stats")
    return stats, coef


def norm_apply(x, coef, residual, act, pool_mode=None):
    """z = act(coef_a * x + coef_b [+ residual]) -> (z, pooled).  `pool_mode`: also write the 2x2x2-pooled z in the same pass
    (mednet_gn_act_pool_fwd) when the shape allows; `pooled` is None otherwise."""
    n, c, d, h, w = x.shape
    lib = L.lib()
    z = torch.empty_like(x, memory_format=CL)
    if pool_mode is not None and lib.mednet_gn_act_pool_supported(d, h, w, c, L.dt(x)):
        pooled = empty_cl(n, c, d // 2, h // 2, w // 2, x.dtype, x.device)
        L.check(lib.mednet_gn_act_pool_fwd(x.data_ptr(), coef.data_ptr(), L.ptr(residual), z.data_ptr(), pooled.data_ptr(), n, d, h, w,
                                           c, act, pool_mode, L.dt(x), L.stream()), "gn_act_pool_fwd")
        return z, pooled
    L.check(lib.mednet_gn_act_fwd(x.data_ptr(), coef.data_ptr(), L.ptr(residual), z.data_ptr(), n, d * h * w, c, act,
                                  L.dt(x), L.dt(z), L.stream()), "gn_act_fwd")
    return z, None


class _NormBackward:
    """What the backward of a normalisation (+ activation) layer sets up -- the gradient of its input, of the residual branch when
    there is one, the targets of the parameter gradients (_grad_target), the workspace -- and what autograd gets for the parameters."""

    def __init__(self, x, gamma_p, beta_p, want_dres):
        n, c, d, h, w = x.shape
        self.dx = torch.empty_like(x, memory_format=CL)
        self.dres = torch.empty_like(x, memory_format=CL) if want_dres else None
        self.dgamma, self.direct_g = _grad_target(gamma_p, (c,)) if gamma_p is not None else (None, False)
        self.dbeta, self.direct_b = _grad_target(beta_p, (c,)) if beta_p is not None else (None, False)
        self.ws = L.workspace(L.lib().mednet_gn_ws_bytes(n, c, d * h * w), x.device)

    def param_grads(self):
        return (None if self.direct_g else self.dgamma), (None if self.direct_b else self.dbeta)


def gn_backward(b, dz, x, z, coef, stats, gamma, act, in_act, partial, groups, dz2=None, lazy=None):
    """GroupNorm (+ activation, + residual) backward into the buffers of `b`, in one of four forms.  No `partial`: all three
    passes (mednet_gn_act_bwd; `dz2`: a second gradient stream, read beside dz).  `partial` = the first pass's rows, taken by the
    producer of dz (GNBHook / GN3Hook): the plain layer (mednet_gn_act_bwd_fused); with the activated output `z`, the residual layer
    of a block (_fused_res); with `lazy` = (dy_pool, skip gradient, pool mode), the residual layer of an encoder block whose dz was
    NOT written (SkipPool2Fn, lazy): the apply pass rebuilds its rows per pooling window (_fused_res_pool); with `lazy` = ("head",
    logits, labels, label dtype, label stride, packed, loss weight, saved, dloss, eps, sigmoid, ignore_index, class kind), the last
    block in front of a small fused head that wrote no dz (_valu_head_bwd): the rows are rebuilt per voxel (_fused_res_head)."""
    n, c, d, h, w = x.shape
    spatial = d * h * w
    lib = L.lib()
    grads, tail = (L.ptr(b.dgamma), L.ptr(b.dbeta)), (L.dt(x), b.ws.data_ptr(), b.ws.numel(), L.stream())
    if partial is None:
        L.check(lib.mednet_gn_act_bwd(dz.data_ptr(), L.ptr(dz2), x.data_ptr(), L.ptr(z), coef.data_ptr(), stats.data_ptr(), L.ptr(gamma),
                                      b.dx.data_ptr(), L.ptr(b.dres), *grads, n, spatial, c, groups, act, in_act, *tail), "gn_act_bwd")
        return
    assert dz2 is None and (z is None) == (b.dres is None)
    if lazy is not None and isinstance(lazy[0], str):  # ("head", ...)
        _, lg, lab, lab_dt, lab_sn, packed, wt, saved, dl, eps, sigmoid, ii, kind = lazy
        L.check(lib.mednet_gn_act_bwd_fused_res_head(lg.data_ptr(), lab.data_ptr(), lab_dt, lab_sn, packed.data_ptr(), L.ptr(wt),
                                                     saved.data_ptr(), dl.data_ptr(), eps, sigmoid, ii, kind, lg.shape[1], x.data_ptr(),
                                                     z.data_ptr(), stats.data_ptr(), gamma.data_ptr(), partial.data_ptr(),
                                                     partial.shape[1], b.dx.data_ptr(), b.dres.data_ptr(), *grads, n, spatial, c, groups,
                                                     act, *tail), "gn_act_bwd_fused_res_head")
    elif lazy is not None:
        dy_pool, dskip, pool_mode = lazy
        L.check(lib.mednet_gn_act_bwd_fused_res_pool(dy_pool.data_ptr(), L.ptr(dskip), x.data_ptr(), z.data_ptr(), stats.data_ptr(),
                                                     gamma.data_ptr(), partial.data_ptr(), partial.shape[1], b.dx.data_ptr(),
                                                     b.dres.data_ptr(), *grads, n, d, h, w, c, groups, act, pool_mode, *tail),
                "gn_act_bwd_fused_res_pool")
    elif z is not None:
        assert in_act == L.ACT_NONE
        L.check(lib.mednet_gn_act_bwd_fused_res(dz.data_ptr(), x.data_ptr(), z.data_ptr(), coef.data_ptr(), stats.data_ptr(),
                                                gamma.data_ptr(), partial.data_ptr(), partial.shape[1], b.dx.data_ptr(),
                                                b.dres.data_ptr(), *grads, n, spatial, c, groups, act, *tail), "gn_act_bwd_fused_res")
    else:
        L.check(lib.mednet_gn_act_bwd_fused(dz.data_ptr(), x.data_ptr(), coef.data_ptr(), stats.data_ptr(), L.ptr(gamma),
                                            partial.data_ptr(), partial.shape[1], b.dx.data_ptr(), *grads, n, spatial, c, groups, act,
                                            in_act, *tail), "gn_act_bwd_fused")


def bn_backward(b, dz, x, z, coef, stats, gamma, act, in_act, partial, frozen):
    """BatchNorm3d (+ activation, + residual) backward into the buffers of `b`: all three passes (mednet_bn_act_bwd), or the last
    two over the rows the producer of dz took (BNBHook, mednet_bn_act_bwd_fused).  `frozen`: evaluation mode, constant statistics."""
    n, c, d, h, w = x.shape
    lib = L.lib()
    tail = (n, d * h * w, c, act, in_act, int(frozen), L.dt(x), b.ws.data_ptr(), b.ws.numel(), L.stream())
    if partial is not None:
        L.check(lib.mednet_bn_act_bwd_fused(dz.data_ptr(), x.data_ptr(), coef.data_ptr(), stats.data_ptr(), L.ptr(gamma),
                                            partial.data_ptr(), partial.shape[1], b.dx.data_ptr(), L.ptr(b.dgamma), L.ptr(b.dbeta),
                                            *tail), "bn_act_bwd_fused")
    else:
        L.check(lib.mednet_bn_act_bwd(dz.data_ptr(), x.data_ptr(), L.ptr(z), coef.data_ptr(), stats.data_ptr(), L.ptr(gamma),
                                      b.dx.data_ptr(), L.ptr(b.dres), L.ptr(b.dgamma), L.ptr(b.dbeta), *tail), "bn_act_bwd")


def _norm_input(ctx, x, who):
    """Forward prologue of both nodes: x in channels-last storage, and ctx.inmask = the ActMaskHook x carries, if it is honoured."""
    L.require_gpu(x, who)
    x0 = x
    x = to_cl(_as_act(x))
    ctx.inmask = getattr(x0, "_mednet_actmask", None) if (x is x0 and FUSE_GN3) else None
    # The fold multiplies dx by act'(x) HERE; the conv layer skips its own activation backward only if the gradient it
    # receives is this very tensor (ActMaskHook.take).  If it declines (x has a second consumer, a tensor hook replaced
    # the gradient) act' is applied twice to this contribution: idempotent for ReLU (a 0/1 mask), wrong for
    # LeakyReLU / ELU -- so only ReLU layers are folded.
    if ctx.inmask is not None and ctx.inmask.act != L.ACT_RELU:
        ctx.inmask = None
    return x


def _norm_output(ctx, x, stats, coef, gamma, beta, residual, act, hook, extra):
    """The apply pass of both nodes and what they keep for the backward (`extra`: groups / frozen)."""
    res = None
    if residual is not None:
        res = to_cl(residual.to(x.dtype))
    z, _ = norm_apply(x, coef, res, act)
    # the activated output is only read back when a residual entered the pre-activation; otherwise the backward
    # recomputes act' from x and `coef` (one tensor less to read in each of its two passes)
    keep_z = act != L.ACT_NONE and residual is not None
    ctx.save_for_backward(x, z if keep_z else None, stats, gamma, coef)
    ctx.meta = (act, residual is not None, extra)
    ctx.params = (gamma, beta)
    ctx.gnb = hook
    if hook is not None:
        hook.gn_in, hook.coef, hook.act = x, coef, act
    return z


def _norm_backward(ctx, dz, entries, n_inputs):
    """Backward of both nodes around `entries` (gn_backward / bn_backward): takes the hook's rows, sets the buffers up, offers dx to
    the activation mask -> the gradients of (x, gamma, beta, residual), None for every input behind them."""
    x, z, stats, gamma, coef = ctx.saved_tensors
    act, has_res, extra = ctx.meta
    fused = ctx.gnb.take(dz) if ctx.gnb is not None else None  # (before any conversion: identity matters)
    dz = to_cl(dz.to(x.dtype))
    b = _NormBackward(x, *ctx.params, has_res)
    inmask = ctx.inmask  # x is the output of a fused conv -> activation layer: fold act'(x) into dx (ActMaskHook)
    in_act = inmask.act if inmask is not None else L.ACT_NONE
    if inmask is not None:
        inmask.offer(b.dx)
    # (the rows only without a residual: the first pass was taken by the conv data gradient that produced dz)
    entries(b, dz, x, z, coef, stats, gamma, act, in_act, None if has_res else fused, extra)
    return (b.dx, *b.param_grads(), b.dres) + (None,) * (n_inputs - 4)


def _norm_hook(kind, gamma, residual):
    """GNBHook / BNBHook for a layer whose consumer may take its first backward pass, or None."""
    if FUSE_GN3 and residual is None and config.is_half_mode() and torch.is_grad_enabled() and gamma is not None:
        return kind()
    return None


class GroupNormActFn(Function):
    """z = act(GroupNorm(x) [+ residual])  -- components.py:57, :36-40, :177-178."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, groups, eps, act, partial=None, hook=None):
        x = _norm_input(ctx, x, "group_norm_act")
        if x.shape[1] % groups:
            raise RuntimeError(f"group_norm: C={x.shape[1]} not divisible by num_groups={groups}")
        stats, coef = gn_statistics(x, gamma, beta, groups, eps, partial)
        return _norm_output(ctx, x, stats, coef, gamma, beta, residual, act, hook, groups)

    @staticmethod
    def backward(ctx, dz):
        return _norm_backward(ctx, dz, gn_backward, 9)


def group_norm_act(x, gamma, beta, groups, eps=1e-5, act=L.ACT_NONE, residual=None, partial=None):
    hook = _norm_hook(GNBHook, gamma, residual)
    z = GroupNormActFn.apply(x, gamma, beta, residual, groups, eps, act, partial, hook)
    if hook is not None:
        z._mednet_gnb = hook
    return z


class BatchNormActFn(Function):
    """z = act(BatchNorm3d(x) [+ residual])  -- components.py:58-63, :36-40, :177-178.  The statistics pass and both backward
    first passes are GroupNorm's kernels over the channels-last batch; the reduction across samples, the running statistics and
    the evaluation coefficients are mednet_bn_* (csrc/norm_act.hip).  `running` = (running_mean, running_var,
    num_batches_tracked) or None: updated on the device when `training`, read when not."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running, training, momentum, eps, act, hook=None):
        x = _norm_input(ctx, x, "batch_norm_act")
        n, c, d, h, w = x.shape
        spatial = d * h * w
        lib = L.lib()
        batch_stats = training or running is None
        stats = torch.empty((n, c, 2), dtype=torch.float32, device=x.device)
        coef = torch.empty((n, c, 2), dtype=torch.float32, device=x.device)
        if batch_stats:
            if n * spatial <= 1:
                raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
            rm, rv, nbt = running if (training and running is not None) else (None, None, None)
            ws = L.workspace(lib.mednet_gn_ws_bytes(n, c, spatial), x.device)
            L.check(lib.mednet_bn_stats(x.data_ptr(), L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), L.ptr(nbt), momentum,
                                        stats.data_ptr(), coef.data_ptr(), n, spatial, c, eps, L.dt(x), ws.data_ptr(), ws.numel(),
                                        L.stream()), "bn_stats")
        else:
            rm, rv, _ = running
            L.check(lib.mednet_bn_eval_coef(rm.data_ptr(), rv.data_ptr(), L.ptr(gamma), L.ptr(beta), stats.data_ptr(),
                                            coef.data_ptr(), n, c, eps, L.stream()), "bn_eval_coef")
        return _norm_output(ctx, x, stats, coef, gamma, beta, residual, act, hook, not batch_stats)

    @staticmethod
    def backward(ctx, dz):
        return _norm_backward(ctx, dz, bn_backward, 10)


def batch_norm_act(x, gamma, beta, running_mean=None, running_var=None, num_batches_tracked=None, training=True, momentum=0.1,
                   eps=1e-5, act=L.ACT_NONE, residual=None):
    """act(F.batch_norm(x, running_mean, running_var, gamma, beta, training, momentum, eps) [+ residual]) on a 5-D tensor.  The
    running buffers (fp32 [C] on x's device; num_batches_tracked one int64, optional) are updated in place by the statistics
    kernel when `training`; without them batch statistics are used in both modes."""
    if momentum is None:
        raise NotImplementedError("mednet_hip batch_norm: momentum=None (cumulative moving average) is not implemented; pass a float")
    running = None
    if running_mean is not None:
        for name, t, dt in (("running_mean", running_mean, torch.float32), ("running_var", running_var, torch.float32),
                            ("num_batches_tracked", num_batches_tracked, torch.int64)):
            if t is None and name == "num_batches_tracked":
                continue
            if t is None or t.dtype != dt or t.device != x.device or not t.is_contiguous():
                raise RuntimeError(f"batch_norm: {name} must be a contiguous {dt} tensor on {x.device}")
        running = (running_mean, running_var, num_batches_tracked)
    hook = _norm_hook(BNBHook, gamma, residual)
    z = BatchNormActFn.apply(x, gamma, beta, residual, running, bool(training), float(momentum), float(eps), act, hook)
    if hook is not None:
        z._mednet_gnb = hook
    return z


# ------------------------------------------------------------------------------------------------- stand-alone activation
class ActFn(Function):
    @staticmethod
    def forward(ctx, x, act):
        L.require_gpu(x, "activation")
        x = _as_act(x)
        xc = x if (x.is_contiguous() or x.is_contiguous(memory_format=CL)) else x.contiguous()
        z = torch.empty_like(xc)  # preserves the memory format
        L.check(L.lib().mednet_act_fwd(xc.data_ptr(), z.data_ptr(), xc.numel(), act, L.dt(xc), L.stream()), "act_fwd")
        ctx.save_for_backward(z)
        ctx.act = act
        return z

    @staticmethod
    def backward(ctx, dz):
        (z,) = ctx.saved_tensors
        if z.dim() == 5 and z.is_contiguous(memory_format=CL) and not z.is_contiguous():
            dz = to_cl(dz)
        else:
            dz = dz.contiguous()
        dz = dz.to(z.dtype)
        dx = torch.empty_like(z)
        L.check(L.lib().mednet_act_bwd(dz.data_ptr(), z.data_ptr(), dx.data_ptr(), z.numel(), ctx.act, L.dt(z),
                                       L.stream()), "act_bwd")
        return dx, None


def activation(x, act):
    return ActFn.apply(x, act)


class AddFn(Function):
    """out = a + b for two same-shape activations (only used when a residual join cannot be folded into a GroupNorm)."""

    @staticmethod
    def forward(ctx, a, b):
        L.require_gpu(a, "add")
        a = to_cl(_as_act(a))
        b = to_cl(b.to(a.dtype))
        out = torch.empty_like(a, memory_format=CL)
        L.check(L.lib().mednet_add(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), L.dt(a), L.stream()), "add")
        return out

    @staticmethod
    def backward(ctx, g):
        return g, g


# ------------------------------------------------------------------------------------------------- channel split
class _SplitGrad:
    """Shared gradient buffer of a channel split: the loss backward kernels of the two halves write their slices of ONE
    full-size tensor (they index the gradient with the strides of the logits slice they were given), so the split's backward
    is that tensor, not a concatenation."""
    __slots__ = ("shape", "base", "k", "claimed")

    def __init__(self, shape, k):
        self.shape, self.k, self.base = tuple(shape), k, None
        self.claimed = set()  # slice offsets whose view has been handed to a loss backward (one writer per slice)


class SplitChannelsFn(Function):
    """(x[:, :k], x[:, k:]) as ONE autograd node (landmarks.py:71-72 slices the network output into heat-map and class
    channels): backward is the shared buffer both loss kernels wrote into (or, if the gradients came from somewhere else, a
    single concatenation) instead of autograd's zero-fill + copy per slice + add over the full logits tensor."""

    @staticmethod
    def forward(ctx, x, k, holder):
        ctx.k, ctx.shape, ctx.holder = k, x.shape, holder
        return x[:, :k], x[:, k:]

    @staticmethod
    def backward(ctx, d0, d1):
        k, shape, holder = ctx.k, ctx.shape, ctx.holder
        base = holder.base if holder is not None else None
        if holder is not None:
            holder.base = None
            holder.claimed.clear()
        if (base is not None and d0 is not None and d1 is not None and d0.dtype == base.dtype == d1.dtype
                and d0.data_ptr() == base.data_ptr() and d1.data_ptr() == base[:, k:].data_ptr()
                and d0.stride() == base[:, :k].stride() and d1.stride() == base[:, k:].stride()):
            return base, None, None
        ref = d0 if d0 is not None else d1
        if d0 is None:
            d0 = ref.new_zeros((shape[0], k) + tuple(shape[2:]))
        if d1 is None:
            d1 = ref.new_zeros((shape[0], shape[1] - k) + tuple(shape[2:]))
        return torch.cat((d0, d1), dim=1), None, None


SPLIT_SHARED = os.environ.get("MEDNET_SPLIT_SHARED", "1") == "1"  # A/B knob


def split_channels(x, k):
    holder = _SplitGrad(x.shape, k) if (SPLIT_SHARED and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()) else None
    a, b = SplitChannelsFn.apply(x, k, holder)
    if holder is not None:
        a._mednet_split, b._mednet_split = (holder, 0), (holder, k)
    return a, b


def _loss_grad_like(lg, split):
    """fp32 gradient buffer with the STRIDES of the logits view `lg` (the loss backward kernels write with those strides):
    a slice of the shared buffer of a channel split when there is one, else a fresh tensor of that layout."""
    if split is not None:
        holder, c0 = split
        # ONE writer per slice: a second loss on the same slice (Dice + CE on the class logits, a loss applied twice) gets a
        # tensor of its own -- autograd then sums the two, and SplitChannelsFn.backward sees a gradient that is not the
        # shared view and takes its concatenation path.  (Two kernels writing one view would leave 2*G2, not G1+G2.)
        if c0 not in holder.claimed:
            if holder.base is None:
                holder.base = torch.empty(holder.shape, dtype=torch.float32, device=lg.device)
            view = holder.base[:, c0:c0 + lg.shape[1]]
            if tuple(view.shape) == tuple(lg.shape) and view.stride() == lg.stride():
                holder.claimed.add(c0)
                return view
    return torch.empty_strided(tuple(lg.shape), lg.stride(), dtype=torch.float32, device=lg.device)


# ------------------------------------------------------------------------------------------------- pooling
class Pool2Fn(Function):
    """nn.MaxPool3d(2) / nn.AvgPool3d(2)  -- components.py:208-212."""

    @staticmethod
    def forward(ctx, x, mode):
        L.require_gpu(x, "pool3d")
        x0 = x
        x = to_cl(_as_act(x))
        n, c, d, h, w = x.shape
        stash = getattr(x0, "_mednet_pooled", None) if x is x0 else None
        # (the stash pooled the values the block WROTE: an in-place change of the output since then -- a forward hook's clamp_(),
        #  user code between the levels -- shows in the version counter, and the pooling kernel runs on the current values)
        if (stash is not None and stash.mode == mode and stash.pooled is not None and stash.pooled.dtype == x.dtype
                and stash.version == x0._version):
            y, stash.pooled = stash.pooled, None  # written by the producing block's last apply pass (block.PoolStash)
        else:
            y = empty_cl(n, c, d // 2, h // 2, w // 2, x.dtype, x.device)
            L.check(L.lib().mednet_pool2_fwd(x.data_ptr(), y.data_ptr(), n, d, h, w, c, mode, L.dt(x), L.stream()), "pool2_fwd")
        ctx.save_for_backward(x)
        ctx.mode = mode
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        n, c, d, h, w = x.shape
        dy = to_cl(dy.to(x.dtype))
        dx = torch.empty_like(x, memory_format=CL)
        L.check(L.lib().mednet_pool2_bwd(dy.data_ptr(), x.data_ptr(), None, dx.data_ptr(), n, d, h, w, c, ctx.mode, L.dt(x),
                                         L.stream()), "pool2_bwd")
        return dx, None


def pool2(x, mode=L.POOL_MAX):
    return Pool2Fn.apply(x, mode)


class SkipPool2Fn(Function):
    """(skip, pooled) = (x, pool(x)): the encoder output that feeds both the next level's pooling and the decoder's
    skip join (model.py:194-205).  As ONE node its backward receives both gradients and sums them inside the pooling
    backward kernel, instead of autograd adding two full-resolution tensors with a separate kernel."""

    @staticmethod
    def forward(ctx, x, mode, sole_consumer=False):
        L.require_gpu(x, "pool3d")
        x0 = x
        x = to_cl(_as_act(x))
        n, c, d, h, w = x.shape
        stash = getattr(x0, "_mednet_pooled", None) if x is x0 else None
        # (the stash pooled the values the block WROTE: an in-place change of the output since then -- a forward hook's clamp_(),
        #  user code between the levels -- shows in the version counter, and the pooling kernel runs on the current values)
        if (stash is not None and stash.mode == mode and stash.pooled is not None and stash.pooled.dtype == x.dtype
                and stash.version == x0._version):
            y, stash.pooled = stash.pooled, None  # written by the producing block's last apply pass (block.PoolStash)
        else:
            y = empty_cl(n, c, d // 2, h // 2, w // 2, x.dtype, x.device)
            L.check(L.lib().mednet_pool2_fwd(x.data_ptr(), y.data_ptr(), n, d, h, w, c, mode, L.dt(x), L.stream()), "pool2_fwd")
        ctx.save_for_backward(x)
        ctx.mode = mode
        ctx.gn3 = _gn3_hook_of(x0, x.dtype) if x is x0 else None
        # x is the output of a fused conv -> activation layer (UNet3D's blocks): the join below folds act'(x) into the gradient it
        # produces and that layer's backward skips its activation pass (ActMaskHook) -- for even extents (mednet_pool2_bwd_act)
        ctx.inmask = getattr(x0, "_mednet_actmask", None) if (x is x0 and FUSE_GN3 and POOL_ACT_MASK and not ((d | h | w) & 1)) else None
        # sole_consumer: the caller (the U-Net's own forward) hands x to nothing else, so the gradient of x goes to the producing
        # block and nowhere else -- the backward may then leave it unwritten and let the block's apply pass rebuild it (LAZY_POOL)
        # (a tensor hook or retain_grad() on x would READ that gradient: then it is written as before)
        ctx.lazy_ok = (bool(sole_consumer) and LAZY_POOL and ctx.gn3 is not None and not x0._backward_hooks
                       and not getattr(x0, "retains_grad", False))
        if debug.TRACE is not None:
            debug.trace(f"skip_pool2.fwd c{c}", y)
        return x.view_as(x), y

    @staticmethod
    def backward(ctx, dskip, dy):
        (x,) = ctx.saved_tensors
        n, c, d, h, w = x.shape
        if dy is None:
            return dskip, None, None
        dy = to_cl(dy.to(x.dtype))
        hook = ctx.gn3
        add_c = 0
        if dskip is not None:
            # (UNet3D: the skip gradient is the leading channels of the concatenation's gradient -- read in place by the plain join)
            add_c = _channel_slice_of_cl(dskip, c) if (hook is None and dskip.dtype == x.dtype and c % 8 == 0 and not ((d | h | w) & 1)) else 0
            if add_c == 0 or add_c % 8:
                add_c = 0
                dskip = to_cl(dskip.to(x.dtype))
        dx = torch.empty_like(x, memory_format=CL)
        rows = L.lib().mednet_pool2_bwd_gn_rows(n, d, h, w, c, L.dt(x)) if hook is not None else 0
        if rows > 0:  # + the first pass of the producing block's GroupNorm-3 backward (x IS that block's output)
            partial = torch.empty((n, rows, c, 2), dtype=torch.float32, device=x.device)
            lazy = ctx.lazy_ok and bool(L.lib().mednet_gn_act_pool_supported(d, h, w, c, L.dt(x)))
            # lazy: sums only -- dx stays an unwritten placeholder (autograd needs a tensor of the right shape to hand on), the
            # block's GroupNorm-3 apply pass rebuilds its rows from dy, the arg-max of x and dskip (mednet_gn_act_bwd_fused_res_pool)
            L.check(L.lib().mednet_pool2_bwd_gn(dy.data_ptr(), x.data_ptr(), L.ptr(dskip), None if lazy else dx.data_ptr(),
                                                hook.gn_in.data_ptr(), hook.act, partial.data_ptr(), n, d, h, w, c, ctx.mode, L.dt(x),
                                                L.stream()), "pool2_bwd_gn")
            hook.offer(dx, partial, (dy, dskip, ctx.mode) if lazy else None)
            if debug.TRACE is not None:
                debug.trace(f"skip_pool2.bwd c{c}", None if lazy else dx, partial)
            return dx, None, None
        mask = ctx.inmask
        L.check(L.lib().mednet_pool2_bwd_act(dy.data_ptr(), x.data_ptr(), L.ptr(dskip), add_c, dx.data_ptr(), n, d, h, w, c, ctx.mode,
                                             L.ACT_NONE if mask is None else mask.act, L.dt(x), L.stream()), "pool2_bwd")
        if mask is not None:
            mask.offer(dx)
        if debug.TRACE is not None:
            debug.trace(f"skip_pool2.bwd c{c}", dx)
        return dx, None, None


POOL_ACT_MASK = os.environ.get("MEDNET_POOL_ACT_MASK", "1") == "1"  # A/B knob
LAZY_POOL = os.environ.get("MEDNET_LAZY_POOL", "1") == "1"  # A/B knob


def skip_pool2(x, mode=L.POOL_MAX, sole_consumer=False):
    """(skip, pooled).  `sole_consumer`: the caller guarantees that x -- a block output -- is used by nothing but this call (the
    returned `skip` IS the tensor to use as x from here on); the backward then need not materialise the gradient of x."""
    return SkipPool2Fn.apply(x, mode, sole_consumer)


# ------------------------------------------------------------------------------------------------- nearest upsample + concat
class UpCatFn(Function):
    """F.interpolate(x, size=enc.shape[2:], mode='nearest') ; torch.cat((enc, x), 1)  -- components.py:277-280."""

    @staticmethod
    def forward(ctx, enc, x, want_stats=False):
        L.require_gpu(x, "upsample_concat")
        enc = to_cl(_as_act(enc))
        x = to_cl(_as_act(x)).to(enc.dtype)
        n, ce, d, h, w = enc.shape
        _, cx, xd, xh, xw = x.shape
        out = empty_cl(n, ce + cx, d, h, w, enc.dtype, enc.device)
        lib = L.lib()
        chunks = lib.mednet_upcat_stats_chunks(n, d, h, w, ce, cx, L.dt(enc)) if want_stats else 0
        if chunks > 0:  # + the GroupNorm partial sums of the concatenated tensor (the 'g c r' block that follows opens with one)
            partial = torch.empty((n, chunks, ce + cx, 2), dtype=torch.float32, device=enc.device)
            L.check(lib.mednet_upcat_fwd_stats(enc.data_ptr(), x.data_ptr(), out.data_ptr(), partial.data_ptr(), n, d, h, w, ce, xd, xh,
                                               xw, cx, L.dt(enc), L.stream()), "upcat_fwd_stats")
        else:
            partial = torch.empty(0, device=enc.device)
            L.check(lib.mednet_upcat_fwd(enc.data_ptr(), x.data_ptr(), out.data_ptr(), n, d, h, w, ce, xd, xh, xw, cx,
                                         L.dt(enc), L.stream()), "upcat_fwd")
        ctx.dims = (n, ce, d, h, w, cx, xd, xh, xw)
        if not want_stats:
            return out
        ctx.mark_non_differentiable(partial)
        return out, partial

    @staticmethod
    def backward(ctx, dout, _dpartial=None):
        n, ce, d, h, w, cx, xd, xh, xw = ctx.dims
        dout = to_cl(dout)
        # the encoder part of the gradient is a VIEW of dout (its leading channels): the pooling join that consumes it reads it
        # where it lies (SkipPool2Fn, mednet_pool2_bwd_act's add_channels); any other consumer makes it dense itself
        view = UPCAT_VIEW and ce % 8 == 0 and cx % 8 == 0
        denc = dout.narrow(1, 0, ce) if view else empty_cl(n, ce, d, h, w, dout.dtype, dout.device)
        dx = empty_cl(n, cx, xd, xh, xw, dout.dtype, dout.device)
        L.check(L.lib().mednet_upcat_bwd(dout.data_ptr(), None if view else denc.data_ptr(), dx.data_ptr(), n, d, h, w, ce, xd, xh,
                                         xw, cx, L.dt(dout), L.stream()), "upcat_bwd")
        return denc, dx, None


UPCAT_VIEW = os.environ.get("MEDNET_UPCAT_VIEW", "1") == "1"  # A/B knob


def _channel_slice_of_cl(t, c):
    """Channels per voxel of the channels-last tensor `t` is a leading-channel slice of (0: `t` is not such a view)."""
    if t.dim() != 5 or t.shape[1] != c:
        return 0
    n, _, d, h, w = t.shape
    sn, sc, sd, sh, sw = t.stride()
    ct = sw
    if sc == 1 and ct > c and sh == w * ct and sd == h * w * ct and sn == d * h * w * ct:
        return ct
    return 0


def upsample_concat(enc, x, want_stats=False):
    """cat((enc, nearest-upsampled x), 1); with want_stats -> (tensor, GroupNorm partial sums of it or None)."""
    if not want_stats:
        return UpCatFn.apply(enc, x)
    out, partial = UpCatFn.apply(enc, x, True)
    return out, (partial if partial.numel() else None)


# ------------------------------------------------------------------------------------------------- losses
def _planar_logits(logits: torch.Tensor):
    """fp32 logits whose (D,H,W) block is dense: returns (tensor, stride_n, stride_c)."""
    t = logits if logits.dtype == torch.float32 else logits.float()
    sp = t.shape[2:]
    dense = []
    acc = 1
    for s in reversed(sp):
        dense.insert(0, acc)
        acc *= s
    if tuple(t.stride()[2:]) != tuple(dense):
        t = t.contiguous()
    return t, t.stride(0), t.stride(1)


def _labels_i64(labels: torch.Tensor, shape):
    if labels.dtype != torch.int64:
        labels = labels.long()
    if tuple(labels.shape) != tuple(shape):
        raise AssertionError("'input' and 'target' must have the same shape")
    return labels.contiguous()


class DiceLossFn(Function):
    """DiceLoss.forward  -- loss.py:114-130 (softmax|sigmoid, one-hot, per-channel dice over the WHOLE batch)."""

    @staticmethod
    def forward(ctx, logits, labels, weight, eps, sigmoid, ignore_index):
        L.require_gpu(logits, "dice_loss")
        opnd = _class_loss_operands(logits, labels, weight)
        n, c, spatial = opnd[3][:3]
        ws = L.workspace(L.lib().mednet_loss_ws_bytes(n, c, spatial), logits.device)
        ii = L.NO_IGNORE if ignore_index is None else int(ignore_index)
        return _class_loss_fwd(ctx, "dice", logits, opnd, (c, 2), (eps, int(sigmoid), ii), ws)

    @staticmethod
    def backward(ctx, dloss):
        return _class_loss_bwd(ctx, dloss, 6)


def dice_loss(logits, labels, weight=None, eps=1e-5, sigmoid=False, ignore_index=None):
    return DiceLossFn.apply(logits, labels, weight, eps, sigmoid, ignore_index)


# ------------------------------------------------------------------------------------------------- 1x1x1 head + loss, one node
FUSE_HEAD_LOSS = os.environ.get("MEDNET_FUSE_HEAD_LOSS", "1") == "1"  # A/B knob


def _dense_view(t: torch.Tensor, block_shape):
    """`t` = N x block_shape with every sample's block dense and any stride between samples (a block that is no such view is copied)
    -> (tensor, sample stride)."""
    n = t.shape[0]
    dense, acc = [], 1
    for sdim in reversed(tuple(block_shape)):
        dense.insert(0, acc)
        acc *= sdim
    if tuple(t.stride()[1:]) != tuple(dense) or (n > 1 and t.stride(0) < acc):
        t = t.contiguous()
    return t, (t.stride(0) if n > 1 else acc)


def _label_view(labels: torch.Tensor, n: int, spatial_shape):
    """Labels as the fused kernels take them: uint8 or int64, N x spatial, each sample's block dense; the stride between samples
    is free (the last channel of a uint8 N x C x D x H x W label volume is consumed where it lies, segmentation.py:60)."""
    if labels.dtype not in (torch.uint8, torch.int64):
        labels = labels.long()
    if tuple(labels.shape) != (n,) + tuple(spatial_shape):
        raise AssertionError("'input' and 'target' must have the same shape")
    labels, sn = _dense_view(labels, spatial_shape)
    return labels, sn, _label_dt(labels)


def _heatmap_view(heatmaps: torch.Tensor, n: int, nh: int, spatial_shape):
    """uint8 heat-map targets as the fused landmark head takes them: N x nh x spatial, channels dense, any stride between samples
    (the first channels of a uint8 label volume are consumed where they lie, landmarks.py:69)."""
    if tuple(heatmaps.shape) != (n, nh) + tuple(spatial_shape):
        raise RuntimeError(f"heatmap_loss: target shape {tuple(heatmaps.shape)} != output {(n, nh) + tuple(spatial_shape)}")
    return _dense_view(heatmaps, (nh,) + tuple(spatial_shape))


def _aligned4(t: torch.Tensor, sn: int):
    """The matrix-core heads read uint8 targets and labels four voxels at a time: base pointer and sample stride must be multiples of
    4 bytes.  A view with an odd storage offset / stride (e.g. a label volume sliced at an odd channel offset) is copied once."""
    if t.data_ptr() % 4 or (t.shape[0] > 1 and sn % 4):
        t = t.contiguous().clone() if t.is_contiguous() else t.contiguous()
        sn = t[0].numel()
    return t, sn


def _loss_weight(weight, device):
    """Per-class / per-channel loss weights (a tensor or a list), or None -> fp32 on the device."""
    return None if weight is None else torch.as_tensor(weight, dtype=torch.float32, device=device).contiguous()


def _class_loss_operands(logits, labels, weight, i64=False):
    """The operands of a stand-alone class loss (dice_loss, cross_entropy, dice_ce_loss, per_channel_dice): planar fp32 logits, the
    labels -- uint8 / int64 as they lie, no cast kernel; `i64`: contiguous int64, what mednet_ce_* takes --, the class weights
    -> (logits, labels, weights, (n, c, spatial, stride_n, stride_c), the label arguments behind the pointer)."""
    lg, sn, sc = _planar_logits(logits)
    n, c = lg.shape[:2]
    if i64:
        lab, lab_args = _labels_i64(labels, (n,) + tuple(lg.shape[2:])), ()
    else:
        lab, lab_sn, lab_dt = _label_view(labels, n, tuple(lg.shape[2:]))
        lab_args = (lab_dt, lab_sn)
    return lg, lab, _loss_weight(weight, lg.device), (n, c, lg[0, 0].numel(), sn, sc), lab_args


def _class_loss_fwd(ctx, name, logits, opnd, saved_shape, scalars, ws, dice=None):
    """What the forwards of the stand-alone class losses do alike: the outputs, the launch of mednet_<name>_fwd[_lt] and what
    _class_loss_bwd finds on ctx (None: no gradient, no loss either -- per_channel_dice wants `dice` alone).  The workspace is the
    caller's: the footprint tests name a request by the function that asks.  -> loss."""
    lg, lab, wt, geom, lab_args = opnd
    loss = None if ctx is None else torch.empty((), dtype=torch.float32, device=lg.device)
    saved = torch.empty(saved_shape, dtype=torch.float32, device=lg.device)
    outs = (L.ptr(loss), saved.data_ptr()) + ((L.ptr(dice),) if lab_args else ())
    entry = getattr(L.lib(), f"mednet_{name}_fwd" + ("_lt" if lab_args else ""))
    L.check(entry(lg.data_ptr(), lab.data_ptr(), *lab_args, L.ptr(wt), *outs, *geom, *scalars, ws.data_ptr(), ws.numel(), L.stream()),
            name + "_fwd")
    if ctx is None:
        return None
    ctx.save_for_backward(lg, lab, wt, saved)
    ctx.meta = (name, lab_args, geom, scalars, logits.dtype)
    ctx.split = getattr(logits, "_mednet_split", None) if lg is logits else None
    if debug.TRACE is not None and name != "ce":
        debug.trace(name + ".fwd", lg, loss, saved)
    return loss


def _class_loss_bwd(ctx, dloss, n_inputs):
    """The matching backward: the logit gradient with the strides of the logits (a slice of a channel split's shared buffer when
    there is one), mednet_<name>_bwd[_lt].  -> the node's gradients."""
    lg, lab, wt, saved = ctx.saved_tensors
    name, lab_args, geom, scalars, in_dtype = ctx.meta
    dl = dloss.to(torch.float32).contiguous()
    dlogits = _loss_grad_like(lg, ctx.split)
    entry = getattr(L.lib(), f"mednet_{name}_bwd" + ("_lt" if lab_args else ""))
    L.check(entry(lg.data_ptr(), lab.data_ptr(), *lab_args, L.ptr(wt), saved.data_ptr(), dl.data_ptr(), dlogits.data_ptr(), *geom,
                  *scalars, L.stream()), name + "_bwd")
    if debug.TRACE is not None and name != "ce":
        debug.trace(name + ".bwd", dlogits)
    return (dlogits.to(in_dtype),) + (None,) * (n_inputs - 1)


def _head_supported(x: torch.Tensor, *targets, mfma: bool) -> bool:
    """The gate of every fused head + loss node; the library's own `_supported` answer comes after it.  `mfma`: the matrix-core heads
    (16-bit storage, uint8 targets, and no activation mask to fold in)."""
    if not (FUSE_HEAD_LOSS and x.is_cuda and x.dim() == 5 and all(t.is_cuda for t in targets)):
        return False
    if x.dtype != config.act_dtype() or not x.is_contiguous(memory_format=CL):
        return False
    if not mfma:
        return True
    if x.dtype == torch.float32 or any(t.dtype != torch.uint8 for t in targets):
        return False
    # (a network whose last block ends in conv -> activation hands the head an activation mask to fold in: the stock path does that)
    return getattr(x, "_mednet_actmask", None) is None or _gn3_hook_of(x, x.dtype) is not None


def _label_dt(labels):
    return L.U8 if labels.dtype == torch.uint8 else L.I64


class _HeadBackward:
    """What the backward of every fused head + loss node sets up -- the feature gradient, the targets of the head's weight / bias
    gradients, the producing block's GroupNorm-3 hook with this node's partial rows (`gn_rows()` of them per sample) or the activation
    mask of a fused conv -> activation layer, the workspace -- and how it ends (`finish`)."""

    def __init__(self, ctx, x, cout, gn_rows, ws_bytes):
        weight, self.bias = ctx.params
        n, cin = x.shape[:2]
        self.dx = torch.empty_like(x, memory_format=CL)
        self.dw, self.direct_w = _grad_target(weight, (cout, cin, 1, 1, 1))
        self.db, self.direct_b = (None, True) if self.bias is None else _grad_target(self.bias, (cout,))
        self.hook, self.inmask = ctx.gn3, getattr(ctx, "inmask", None)
        self.partial = None if self.hook is None else torch.empty((n, gn_rows(), cin, 2), dtype=torch.float32, device=x.device)
        self.gn_in = None if self.hook is None else self.hook.gn_in.data_ptr()
        self.act = self.hook.act if self.hook is not None else (self.inmask.act if self.inmask is not None else 0)
        self.ws = L.workspace(ws_bytes, x.device)

    def finish(self, name, n_inputs, lazy=None):
        """Offers dx (and the rows) to the hook or the mask -> the node's gradients, None for every input behind x, weight, bias.
        `lazy`: dx is an unwritten placeholder, and these are the operands the block's apply pass rebuilds it from (GN3Hook.lazy)."""
        if self.hook is not None:
            self.hook.offer(self.dx, self.partial, lazy)
        elif self.inmask is not None:
            self.inmask.offer(self.dx)
        if debug.TRACE is not None:
            debug.trace(name + ".bwd", None if lazy is not None else self.dx, self.partial, self.dw, self.db)
        return (self.dx, (None if self.direct_w else self.dw),
                (None if (self.bias is None or self.direct_b) else self.db)) + (None,) * (n_inputs - 3)


def head_dice_supported(x: torch.Tensor, cin: int, cout: int, labels: torch.Tensor) -> bool:
    return _head_supported(x, labels, mfma=False) and bool(L.lib().mednet_head_dice_supported(cin, cout, L.dt(x), _label_dt(labels)))


def _valu_head_fwd(ctx, name, x, weight, bias, packed, labels, loss_weight, saved_shape, scalars):
    """Forward of HeadDiceFn / HeadCEFn / HeadDiceCEFn: mednet_<name>_fwd, whose arguments differ in `scalars` (between cout and the dtype) only."""
    L.require_gpu(x, name)
    n, cin, d, h, w = x.shape
    cout = weight.shape[0]
    spatial = d * h * w
    lab, lab_sn, lab_dt = _label_view(labels, n, (d, h, w))
    wt = _loss_weight(loss_weight, x.device)
    logits = torch.empty((n, cout, d, h, w), dtype=torch.float32, device=x.device)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    saved = torch.empty(saved_shape, dtype=torch.float32, device=x.device)
    lib = L.lib()
    ws = L.workspace(getattr(lib, f"mednet_{name}_ws_bytes")(n, spatial, cin, cout), x.device)
    L.check(getattr(lib, f"mednet_{name}_fwd")(x.data_ptr(), packed.data_ptr(), L.ptr(bias), lab.data_ptr(), lab_dt, lab_sn, L.ptr(wt),
                                               logits.data_ptr(), loss.data_ptr(), saved.data_ptr(), n, spatial, cin, cout, *scalars,
                                               L.dt(x), ws.data_ptr(), ws.numel(), L.stream()), name + "_fwd")
    ctx.save_for_backward(x, packed, logits, lab, wt, saved)
    ctx.meta = (scalars, lab_sn, lab_dt)
    ctx.params = (weight, bias)
    ctx.gn3 = _gn3_hook_of(x, x.dtype)
    # x is the output of a fused conv -> activation layer (UNet3D's last block): the backward folds act'(x) into the feature
    # gradient it stores and that layer skips its activation pass (ActMaskHook), as SkipPool2Fn does for the encoder levels
    ctx.inmask = getattr(x, "_mednet_actmask", None) if (ctx.gn3 is None and FUSE_GN3 and POOL_ACT_MASK) else None
    # The producing block said that its backward consumes the gradient of x and that x goes nowhere else (GN3Hook.lazy_head_ok):
    # the backward may then take the sums only and leave the gradient unwritten -- the block's GroupNorm-3 apply pass rebuilds its
    # rows (mednet_gn_act_bwd_fused_res_head).  A tensor hook or retain_grad() on x would READ that gradient: then it is written as
    # before (looked at again in the backward: both can still arrive after this forward).
    ctx.lazy_ok = (LAZY_HEAD and ctx.gn3 is not None and ctx.gn3.lazy_head_ok and not _reads_grad(x)
                   and bool(lib.mednet_gn_act_bwd_fused_res_head_supported(cin, cout, L.dt(x), lab_dt)))
    ctx.mark_non_differentiable(logits)
    if debug.TRACE is not None:
        debug.trace(name + ".fwd", logits, loss, saved)
    return logits, loss


LAZY_HEAD = os.environ.get("MEDNET_LAZY_HEAD", "1") == "1"  # A/B knob
_HEAD_KIND = {"head_dice": L.CLASS_DICE, "head_ce": L.CLASS_CE, "head_dice_ce": L.CLASS_DICE_CE}


def _reads_grad(x) -> bool:
    """Will autograd hand the gradient of x to anyone but the node that produced x?  (a tensor hook, retain_grad())"""
    return bool(x._backward_hooks) or bool(getattr(x, "retains_grad", False))


def _valu_head_bwd(ctx, name, dloss, n_inputs):
    x, packed, logits, lab, wt, saved = ctx.saved_tensors
    scalars, lab_sn, lab_dt = ctx.meta
    n, cin = x.shape[:2]
    cout = logits.shape[1]
    spatial = x[0, 0].numel()
    lib = L.lib()
    dl = dloss.to(torch.float32).contiguous()
    b = _HeadBackward(ctx, x, cout, lambda: getattr(lib, f"mednet_{name}_gn_rows")(n, spatial, cin),
                      getattr(lib, f"mednet_{name}_ws_bytes")(n, spatial, cin, cout))
    if ctx.lazy_ok and b.hook is not None and debug.TRACE is None and not _reads_grad(x):
        # sums only: b.dx stays an unwritten placeholder (autograd needs a tensor of the right shape to hand on)
        L.check(getattr(lib, f"mednet_{name}_bwd_sums")(logits.data_ptr(), lab.data_ptr(), lab_dt, lab_sn, packed.data_ptr(), L.ptr(wt),
                                                        saved.data_ptr(), dl.data_ptr(), b.gn_in, x.data_ptr(), b.act,
                                                        b.partial.data_ptr(), b.dw.data_ptr(), L.ptr(b.db), n, spatial, cin, cout,
                                                        *scalars, L.dt(x), b.ws.data_ptr(), b.ws.numel(), L.stream()), name + "_bwd_sums")
        eps, sigmoid, ii = scalars if len(scalars) == 3 else (0.0, 0, scalars[0])  # (head_ce: ignore_index only)
        return b.finish(name, n_inputs, lazy=("head", logits, lab, lab_dt, lab_sn, packed, wt, saved, dl, eps, sigmoid, ii,
                                             _HEAD_KIND[name]))
    L.check(getattr(lib, f"mednet_{name}_bwd")(logits.data_ptr(), lab.data_ptr(), lab_dt, lab_sn, packed.data_ptr(), L.ptr(wt),
                                               saved.data_ptr(), dl.data_ptr(), b.dx.data_ptr(), b.gn_in, x.data_ptr(), b.act,
                                               L.ptr(b.partial), b.dw.data_ptr(), L.ptr(b.db), n, spatial, cin, cout, *scalars,
                                               L.dt(x), b.ws.data_ptr(), b.ws.numel(), L.stream()), name + "_bwd")
    return b.finish(name, n_inputs)


class HeadDiceFn(Function):
    """logits = final_conv(x) (model.py:207, 1x1x1 with bias, planar fp32) and loss = DiceLoss(logits, labels) (loss.py:114-130)
    as ONE autograd node: forward is one pass over the features (mednet_head_dice_fwd), backward one pass that produces the
    feature gradient, the head's weight and bias gradients and the first pass of the producing block's GroupNorm-3 backward
    without ever storing the logit gradient (mednet_head_dice_bwd).  Returns (logits, loss); the logits are a result for the
    caller (metrics, `outputs`), not a differentiable output of this node."""

    @staticmethod
    def forward(ctx, x, weight, bias, packed, labels, loss_weight, eps, sigmoid, ignore_index):
        ii = L.NO_IGNORE if ignore_index is None else int(ignore_index)
        return _valu_head_fwd(ctx, "head_dice", x, weight, bias, packed, labels, loss_weight, (weight.shape[0], 2),
                              (eps, int(sigmoid), ii))

    @staticmethod
    def backward(ctx, _dlogits, dloss):
        return _valu_head_bwd(ctx, "head_dice", dloss, 9)


def head_dice(x, weight, bias, packed, labels, loss_weight=None, eps=1e-5, sigmoid=False, ignore_index=None):
    """-> (logits N x C x D x H x W fp32, Dice loss)."""
    return HeadDiceFn.apply(x, weight, bias, packed, labels, loss_weight, eps, sigmoid, ignore_index)


def head_ce_supported(x: torch.Tensor, cin: int, cout: int, labels: torch.Tensor) -> bool:
    return _head_supported(x, labels, mfma=False) and bool(L.lib().mednet_head_ce_supported(cin, cout, L.dt(x), _label_dt(labels)))


class HeadCEFn(Function):
    """logits = final_conv(x) and loss = nn.CrossEntropyLoss(weight, ignore_index)(logits, labels) (segmentation.py:49, 61-62) as
    ONE autograd node -- HeadDiceFn with the cross-entropy closed form (mednet_head_ce_fwd / _bwd): no int64 label copy, no
    logit-gradient tensor.  Returns (logits, loss); the logits are not a differentiable output of this node."""

    @staticmethod
    def forward(ctx, x, weight, bias, packed, labels, loss_weight, ignore_index):
        return _valu_head_fwd(ctx, "head_ce", x, weight, bias, packed, labels, loss_weight, (2,), (int(ignore_index),))

    @staticmethod
    def backward(ctx, _dlogits, dloss):
        return _valu_head_bwd(ctx, "head_ce", dloss, 7)


def head_ce(x, weight, bias, packed, labels, loss_weight=None, ignore_index=-100):
    """-> (logits N x C x D x H x W fp32, cross-entropy loss)."""
    return HeadCEFn.apply(x, weight, bias, packed, labels, loss_weight, ignore_index)


def head_dice_ce_supported(x: torch.Tensor, cin: int, cout: int, labels: torch.Tensor) -> bool:
    return _head_supported(x, labels, mfma=False) and bool(L.lib().mednet_head_dice_ce_supported(cin, cout, L.dt(x), _label_dt(labels)))


class HeadDiceCEFn(Function):
    """logits = final_conv(x) and loss = DiceLoss(weight, eps)(logits, labels) + nn.CrossEntropyLoss(weight)(logits, labels) as ONE
    autograd node -- HeadDiceFn with the sum of the two closed forms (mednet_head_dice_ce_fwd / _bwd): one softmax per voxel each way,
    no logit-gradient tensor.  Softmax only, no ignore_index.  Returns (logits, loss); the logits are not a differentiable output."""

    @staticmethod
    def forward(ctx, x, weight, bias, packed, labels, loss_weight, eps):
        return _valu_head_fwd(ctx, "head_dice_ce", x, weight, bias, packed, labels, loss_weight, (2 * weight.shape[0] + 1,),
                              (eps, 0, L.NO_IGNORE))

    @staticmethod
    def backward(ctx, _dlogits, dloss):
        return _valu_head_bwd(ctx, "head_dice_ce", dloss, 7)


def head_dice_ce(x, weight, bias, packed, labels, loss_weight=None, eps=1e-5):
    """-> (logits N x C x D x H x W fp32, Dice + cross-entropy loss)."""
    return HeadDiceCEFn.apply(x, weight, bias, packed, labels, loss_weight, eps)


def _class_head_fwd(ctx, name, what, x, weight, bias, packed, labels, loss_weight, eps, sigmoid, ignore_index, class_kind, launch):
    """What the forwards of the matrix-core class heads (HeadSegFn, DsHeadFn) do alike: the label check, the loss operands, the
    outputs, and what the backward (_HeadBackward) finds on ctx.  `what`: None, or what is wrong with the labels' shape;
    `launch(wt, ii, loss, saved)` runs the node's forward entry -> (labels as passed to it, their sample stride, the node's own
    entries of ctx.meta).  -> loss."""
    if labels.dtype != torch.uint8 or what is not None:
        raise RuntimeError(f"{name}: labels must be {what or 'uint8'}, not {labels.dtype} (see {name}_supported)")
    ncls = weight.shape[0]
    wt = _loss_weight(loss_weight, x.device)
    nsaved, ii = _class_operands(class_kind, ncls, sigmoid, ignore_index, name)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    saved = torch.empty((ncls, 2) if nsaved == 2 * ncls else (nsaved,), dtype=torch.float32, device=x.device)
    lab, lab_sn, extra = launch(wt, ii, loss, saved)
    ctx.save_for_backward(x, packed, lab, wt, saved)
    ctx.meta = (eps, int(sigmoid), ii, lab_sn, ncls, class_kind) + extra
    ctx.params = (weight, bias)
    if debug.TRACE is not None:
        debug.trace(name + ".fwd", loss, saved)
    return loss


def head_seg_supported(x: torch.Tensor, cin: int, ncls: int, labels: torch.Tensor) -> bool:
    """Does the matrix-core segmentation head (5 .. 16 classes, 16-bit storage, uint8 labels) take this head?"""
    return _head_supported(x, labels, mfma=True) and bool(L.lib().mednet_head_seg_supported(cin, ncls, L.dt(x), L.U8, x[0, 0].numel()))


class HeadSegFn(Function):
    """SegmentationNet's head and loss (segmentation.py:58-62) for 5 .. 16 classes as ONE autograd node in the 16-bit storage modes:
    loss = DiceLoss | nn.CrossEntropyLoss (final_conv(x), labels).  Forward: one matrix-core pass over the features that writes nothing
    but loss partials, and the planar fp32 logits only when `want_logits` (mednet_head_seg_fwd); backward: one pass that rebuilds the
    logits the same way and produces the feature gradient, the head's weight / bias gradients and the first pass of the producing
    block's GroupNorm-3 backward (mednet_head_seg_bwd).  No logit-gradient tensor exists.  Returns (logits or None, loss); the logits
    are not a differentiable output of this node."""

    @staticmethod
    def forward(ctx, x, weight, bias, packed, labels, loss_weight, eps, sigmoid, ignore_index, class_kind, want_logits):
        L.require_gpu(x, "head_seg")
        n, cin, d, h, w = x.shape
        ncls = weight.shape[0]
        spatial = d * h * w
        logits = torch.empty((n, ncls, d, h, w), dtype=torch.float32, device=x.device) if want_logits else None
        lib = L.lib()
        ws = L.workspace(lib.mednet_head_seg_ws_bytes(n, spatial, ncls), x.device)

        def launch(wt, ii, loss, saved):
            lab, lab_sn = _aligned4(*_label_view(labels, n, (d, h, w))[:2])
            L.check(lib.mednet_head_seg_fwd(x.data_ptr(), packed.data_ptr(), L.ptr(bias), lab.data_ptr(), lab_sn, L.ptr(wt), L.ptr(logits),
                                            loss.data_ptr(), saved.data_ptr(), n, spatial, cin, ncls, class_kind, eps, int(sigmoid), ii,
                                            L.dt(x), ws.data_ptr(), ws.numel(), L.stream()), "head_seg_fwd")
            return lab, lab_sn, ()

        loss = _class_head_fwd(ctx, "head_seg", None, x, weight, bias, packed, labels, loss_weight, eps, sigmoid, ignore_index,
                               class_kind, launch)
        ctx.gn3 = _gn3_hook_of(x, x.dtype)
        if logits is not None:
            ctx.mark_non_differentiable(logits)
        return logits, loss

    @staticmethod
    def backward(ctx, _dlogits, dloss):
        x, packed, lab, wt, saved = ctx.saved_tensors
        eps, sigmoid, ii, lab_sn, ncls, class_kind = ctx.meta
        n, cin = x.shape[:2]
        spatial = x[0, 0].numel()
        lib = L.lib()
        dl = dloss.to(torch.float32).contiguous()
        b = _HeadBackward(ctx, x, ncls, lambda: lib.mednet_head_seg_gn_rows(spatial), lib.mednet_head_seg_ws_bytes(n, spatial, ncls))
        L.check(lib.mednet_head_seg_bwd(x.data_ptr(), packed.data_ptr(), L.ptr(b.bias), lab.data_ptr(), lab_sn, L.ptr(wt), saved.data_ptr(),
                                        dl.data_ptr(), b.dx.data_ptr(), b.gn_in, b.act, L.ptr(b.partial), b.dw.data_ptr(), L.ptr(b.db), n,
                                        spatial, cin, ncls, class_kind, eps, sigmoid, ii, L.dt(x), b.ws.data_ptr(), b.ws.numel(),
                                        L.stream()), "head_seg_bwd")
        return b.finish("head_seg", 11)


def head_seg(x, weight, bias, packed, labels, loss_weight=None, eps=1e-5, sigmoid=False, ignore_index=None, class_loss="DICE",
             want_logits=False):
    """-> (logits N x C x D x H x W fp32 or None, loss) of SegmentationNet's loss on final_conv(x), 5 <= C <= 16; class_loss "DICE"
    (DiceLoss), "CE" (nn.CrossEntropyLoss: softmax, `ignore_index` as that module's, -100 by default there) or "DICE_CE" (their sum
    with one class-weight vector: softmax, no ignore_index)."""
    return HeadSegFn.apply(x, weight, bias, packed, labels, loss_weight, eps, sigmoid, ignore_index, _class_kind(class_loss),
                           want_logits)


def ds_head_supported(x: torch.Tensor, cin: int, ncls: int, labels: torch.Tensor, shift: int) -> bool:
    """Does the deep-supervision node take this level?  x: the level's block output (16-bit storage, channels-last), labels: the
    FULL-resolution N x D x H x W uint8 labels, of which the level is the nearest-neighbour pick at stride 2^shift."""
    if not _head_supported(x, labels, mfma=True) or labels.dim() != 4 or getattr(x, "_mednet_actmask", None) is not None:
        return False
    d, h, w = x.shape[2:]
    if tuple(s >> shift for s in labels.shape[1:]) != (d, h, w) or labels.shape[0] != x.shape[0]:
        return False
    return bool(L.lib().mednet_ds_head_supported(cin, ncls, L.dt(x), L.U8, d, h, w, shift))


class DsHeadFn(Function):
    """Deep supervision on a coarser decoder level as ONE autograd node at the junction "block output -> {next decoder, auxiliary
    head}": (x_pass, loss) = (x, criterion(head(x), labels[..., ::2^shift, ::2^shift, ::2^shift])).  The forward is one matrix-core
    pass that writes loss partials only and reads the full-resolution uint8 labels at a stride (mednet_ds_head_fwd); the backward
    receives BOTH gradients -- d_pass from the next decoder, dloss -- and in one launch rebuilds the logits, adds W^T dl to d_pass in
    fp32, rounds once and writes the block's output gradient, plus the head's weight / bias gradients (mednet_ds_head_bwd).  No
    down-sampled label tensor, logit tensor, logit-gradient tensor or autograd add exists.  As with SkipPool2Fn the caller uses
    `x_pass` in place of x from here on.  The producing block's GroupNorm-3 sums are taken when mednet_ds_head_gn_rows says so (0 rows
    in this version: the block runs its stand-alone pass, and nothing is offered that it could decline)."""

    @staticmethod
    def forward(ctx, x, weight, bias, packed, labels, shift, loss_weight, eps, sigmoid, ignore_index, class_kind):
        L.require_gpu(x, "ds_head")
        n, cin, d, h, w = x.shape
        ncls = weight.shape[0]
        full = tuple(labels.shape[1:])
        lib = L.lib()
        ws = L.workspace(lib.mednet_ds_head_ws_bytes(n, d, h, w, cin, ncls), x.device)

        def launch(wt, ii, loss, saved):
            lab, lab_sn = _label_view(labels, n, full)[:2]  # (byte loads: no alignment rule)
            L.check(lib.mednet_ds_head_fwd(x.data_ptr(), packed.data_ptr(), L.ptr(bias), lab.data_ptr(), L.U8, lab_sn, L.ptr(wt),
                                           loss.data_ptr(), saved.data_ptr(), n, d, h, w, *full, shift, cin, ncls, class_kind, eps,
                                           int(sigmoid), ii, L.dt(x), ws.data_ptr(), ws.numel(), L.stream()), "ds_head_fwd")
            return lab, lab_sn, (full, shift)

        loss = _class_head_fwd(ctx, "ds_head", None if labels.dim() == 4 else "a uint8 N x D x H x W volume", x, weight, bias, packed,
                               labels, loss_weight, eps, sigmoid, ignore_index, class_kind, launch)
        rows = lib.mednet_ds_head_gn_rows(d, h, w, cin, L.dt(x))
        ctx.gn3 = _gn3_hook_of(x, x.dtype) if rows > 0 else None
        ctx.gn_rows = rows
        return x.view_as(x), loss

    @staticmethod
    def backward(ctx, d_pass, dloss):
        x, packed, lab, wt, saved = ctx.saved_tensors
        eps, sigmoid, ii, lab_sn, ncls, class_kind, full, shift = ctx.meta
        if dloss is None:  # (the loss went nowhere: the node is the identity on x)
            return (d_pass,) + (None,) * 10
        n, cin, d, h, w = x.shape
        lib = L.lib()
        dl = dloss.to(torch.float32).contiguous()
        if d_pass is not None:
            d_pass = to_cl(d_pass.to(x.dtype))
        b = _HeadBackward(ctx, x, ncls, lambda: ctx.gn_rows, lib.mednet_ds_head_ws_bytes(n, d, h, w, cin, ncls))
        L.check(lib.mednet_ds_head_bwd(x.data_ptr(), packed.data_ptr(), L.ptr(b.bias), lab.data_ptr(), L.U8, lab_sn, L.ptr(wt),
                                       saved.data_ptr(), dl.data_ptr(), L.ptr(d_pass), b.dx.data_ptr(), b.gn_in, b.act, L.ptr(b.partial),
                                       b.dw.data_ptr(), L.ptr(b.db), n, d, h, w, *full, shift, cin, ncls, class_kind, eps, sigmoid, ii,
                                       L.dt(x), b.ws.data_ptr(), b.ws.numel(), L.stream()), "ds_head_bwd")
        return b.finish("ds_head", 11)


def ds_head(x, weight, bias, packed, labels, shift, loss_weight=None, eps=1e-5, sigmoid=False, ignore_index=None, class_loss="DICE"):
    """-> (x_pass, loss): the deep-supervision loss of level `shift` (class_loss "DICE", "CE" or "DICE_CE" as ops.head_seg) on
    head(x) against the full-resolution uint8 `labels` picked at stride 2^shift, and x handed through for the next decoder."""
    return DsHeadFn.apply(x, weight, bias, packed, labels, shift, loss_weight, eps, sigmoid, ignore_index, _class_kind(class_loss))


def head_landmark_supported(x: torch.Tensor, cin: int, nh: int, ncls: int, heatmaps: torch.Tensor, labels: torch.Tensor) -> bool:
    return (_head_supported(x, labels, heatmaps, mfma=True)
            and bool(L.lib().mednet_head_landmark_supported(cin, nh, ncls, L.dt(x), x[0, 0].numel())))


class HeadLandmarkFn(Function):
    """LandmarkNet's head and loss (landmarks.py:66-83, 125-134) as ONE autograd node in the 16-bit storage modes:
    outputs = final_conv(x) (model.py:207), class_loss = DiceLoss(outputs[:, nh:], labels), regression_loss = sum_c w_c *
    mean f(outputs[:, c] - heatmaps[:, c]).  Forward: one matrix-core pass over the features that writes nothing but loss partials
    (mednet_head_landmark_cls_fwd); backward: one pass that rebuilds the logits the same way and produces the feature gradient, the
    head's weight / bias gradients and the first pass of the producing block's GroupNorm-3 backward
    (mednet_head_landmark_cls_bwd).  No logit or logit-gradient tensor exists.  Returns (class_loss, regression_loss).
    class_kind CLASS_CE: the class term is nn.CrossEntropyLoss(class_weight, ignore_index) (landmarks.py:49)."""

    @staticmethod
    def forward(ctx, x, weight, bias, packed, heatmaps, labels, class_weight, reg_weight, kind, eps, sigmoid, ignore_index,
                class_kind=L.CLASS_DICE):
        L.require_gpu(x, "head_landmark")
        nh = heatmaps.shape[1]
        ncls = weight.shape[0] - nh
        hm, hm_sn, lab, lab_sn, cw, rw, ii = _landmark_operands(x, heatmaps, labels, class_weight, reg_weight, ignore_index)
        closs, rloss, saved, _ = _landmark_fwd(x, packed, bias, hm, hm_sn, lab, lab_sn, cw, rw, nh, ncls, kind, eps, sigmoid, ii,
                                               class_kind, False)
        ctx.save_for_backward(x, packed, hm, lab, cw, rw, saved)
        ctx.meta = (kind, eps, int(sigmoid), ii, hm_sn, lab_sn, nh, ncls, class_kind)
        ctx.params = (weight, bias)
        ctx.gn3 = _gn3_hook_of(x, x.dtype)
        if debug.TRACE is not None:
            debug.trace("head_landmark.fwd", closs, rloss, saved)
        return closs, rloss

    @staticmethod
    def backward(ctx, dclass, dreg):
        x, packed, hm, lab, cw, rw, saved = ctx.saved_tensors
        kind, eps, sigmoid, ii, hm_sn, lab_sn, nh, ncls, class_kind = ctx.meta
        n, cin = x.shape[:2]
        spatial = x[0, 0].numel()
        lib = L.lib()
        zero = None
        if dclass is None or dreg is None:
            zero = torch.zeros((), dtype=torch.float32, device=x.device)
        dc = zero if dclass is None else dclass.to(torch.float32).contiguous()
        dr = zero if dreg is None else dreg.to(torch.float32).contiguous()
        b = _HeadBackward(ctx, x, nh + ncls, lambda: lib.mednet_head_landmark_gn_rows(spatial),
                          lib.mednet_head_landmark_ws_bytes(n, spatial, nh, ncls))
        L.check(lib.mednet_head_landmark_cls_bwd(x.data_ptr(), packed.data_ptr(), L.ptr(b.bias), hm.data_ptr(), hm_sn, lab.data_ptr(),
                                                 lab_sn, L.ptr(cw), L.ptr(rw), saved.data_ptr(), dc.data_ptr(), dr.data_ptr(),
                                                 b.dx.data_ptr(), b.gn_in, b.act, L.ptr(b.partial), b.dw.data_ptr(), L.ptr(b.db), n,
                                                 spatial, cin, nh, ncls, kind, class_kind, eps, sigmoid, ii, L.dt(x), b.ws.data_ptr(),
                                                 b.ws.numel(), L.stream()), "head_landmark_cls_bwd")
        return b.finish("head_landmark", 13)


def head_landmark(x, weight, bias, packed, heatmaps, labels, class_weight=None, reg_weight=None, kind="L2", eps=1e-5, sigmoid=False,
                  ignore_index=None, class_loss="DICE"):
    """-> (class_loss, regression_loss) of LandmarkNet.loss on final_conv(x); class_loss "DICE" (DiceLoss), "CE"
    (nn.CrossEntropyLoss: softmax, `ignore_index` as that module's, -100 by default there) or "DICE_CE" (their sum with one
    class-weight vector: softmax, no ignore_index)."""
    return HeadLandmarkFn.apply(x, weight, bias, packed, heatmaps, labels, class_weight, reg_weight,
                                L.REG_L2 if kind == "L2" else L.REG_L1, eps, sigmoid, ignore_index, _class_kind(class_loss))


def head_landmark_eval(x, weight, bias, packed, heatmaps, labels, class_weight=None, reg_weight=None, kind="L2", eps=1e-5,
                       ignore_index=None, class_loss="DICE"):
    """Forward only (LandmarkNet.validation_step, landmarks.py:136-162): -> (class_loss, regression_loss, dice_metric [ncls]) of
    final_conv(x) from ONE pass over the features, no autograd node, no logit tensor (mednet_head_landmark_cls_fwd)."""
    L.require_gpu(x, "head_landmark")
    nh = heatmaps.shape[1]
    ncls = weight.shape[0] - nh
    hm, hm_sn, lab, lab_sn, cw, rw, ii = _landmark_operands(x, heatmaps, labels, class_weight, reg_weight, ignore_index)
    closs, rloss, _, dice = _landmark_fwd(x, packed, bias, hm, hm_sn, lab, lab_sn, cw, rw, nh, ncls, L.REG_L2 if kind == "L2" else L.REG_L1,
                                          eps, False, ii, _class_kind(class_loss), True)
    return closs, rloss, dice


def _class_kind(class_loss):
    if class_loss not in ("DICE", "CE", "DICE_CE"):
        raise ValueError(f"class_loss must be 'DICE', 'CE' or 'DICE_CE', not {class_loss!r}")
    return {"DICE": L.CLASS_DICE, "CE": L.CLASS_CE, "DICE_CE": L.CLASS_DICE_CE}[class_loss]


def _class_operands(class_kind, ncls, sigmoid, ignore_index, who):
    """-> (floats of `saved`, ignore_index as the C entries take it) for a class-loss kind.  "DICE_CE" is a softmax form without
    ignore_index."""
    if class_kind == L.CLASS_DICE_CE:
        if sigmoid or ignore_index is not None:
            raise ValueError(f"{who}: class_loss 'DICE_CE' is a softmax form without ignore_index")
        return 2 * ncls + 1, L.NO_IGNORE
    if ignore_index is None:
        return 2 * ncls, (L.NO_IGNORE if class_kind == L.CLASS_DICE else -100)
    return 2 * ncls, int(ignore_index)


def _landmark_operands(x, heatmaps, labels, class_weight, reg_weight, ignore_index):
    n, _, d, h, w = x.shape
    hm, hm_sn = _aligned4(*_heatmap_view(heatmaps, n, heatmaps.shape[1], (d, h, w)))
    lab, lab_sn = _aligned4(*_label_view(labels, n, (d, h, w))[:2])
    ii = L.NO_IGNORE if ignore_index is None else int(ignore_index)
    return hm, hm_sn, lab, lab_sn, _loss_weight(class_weight, x.device), _loss_weight(reg_weight, x.device), ii


def _landmark_fwd(x, packed, bias, hm, hm_sn, lab, lab_sn, cw, rw, nh, ncls, kind, eps, sigmoid, ii, class_kind, metric):
    n, cin = x.shape[:2]
    spatial = x[0, 0].numel()
    closs = torch.empty((), dtype=torch.float32, device=x.device)
    rloss = torch.empty((), dtype=torch.float32, device=x.device)
    # (Dice + CE: [ncls][2] = {I, D}, then sum w_y)
    saved = torch.empty((2 * ncls + 1,) if class_kind == L.CLASS_DICE_CE else (ncls, 2), dtype=torch.float32, device=x.device)
    dice = torch.empty((ncls,), dtype=torch.float32, device=x.device) if metric else None
    lib = L.lib()
    ws = L.workspace(lib.mednet_head_landmark_ws_bytes(n, spatial, nh, ncls), x.device)
    L.check(lib.mednet_head_landmark_cls_fwd(x.data_ptr(), packed.data_ptr(), L.ptr(bias), hm.data_ptr(), hm_sn, lab.data_ptr(), lab_sn,
                                             L.ptr(cw), L.ptr(rw), None, closs.data_ptr(), rloss.data_ptr(), saved.data_ptr(),
                                             L.ptr(dice), n, spatial, cin, nh, ncls, kind, class_kind, eps, int(sigmoid), ii, L.dt(x),
                                             ws.data_ptr(), ws.numel(), L.stream()), "head_landmark_cls_fwd")
    return closs, rloss, saved, dice


def per_channel_dice(logits, labels, weight=None, eps=1e-5, sigmoid=False, ignore_index=None):
    """dice_metric  -- loss.py:51-55 (no gradient)."""
    L.require_gpu(logits, "dice_metric")
    opnd = _class_loss_operands(logits.detach(), labels, weight)
    n, c, spatial = opnd[3][:3]
    dice = torch.empty((c,), dtype=torch.float32, device=logits.device)
    ws = L.workspace(L.lib().mednet_loss_ws_bytes(n, c, spatial), logits.device)
    ii = L.NO_IGNORE if ignore_index is None else int(ignore_index)
    _class_loss_fwd(None, "dice", logits, opnd, (c, 2), (eps, int(sigmoid), ii), ws, dice)
    return dice


class CrossEntropyFn(Function):
    """nn.CrossEntropyLoss(weight)(logits, labels), mean reduction  -- segmentation.py:49; landmarks.py:49."""

    @staticmethod
    def forward(ctx, logits, labels, weight, ignore_index):
        L.require_gpu(logits, "cross_entropy")
        opnd = _class_loss_operands(logits, labels, weight, i64=True)
        n, c, spatial = opnd[3][:3]
        ws = L.workspace(L.lib().mednet_loss_ws_bytes(n, c, spatial), logits.device)
        return _class_loss_fwd(ctx, "ce", logits, opnd, (2,), (int(ignore_index),), ws)

    @staticmethod
    def backward(ctx, dloss):
        return _class_loss_bwd(ctx, dloss, 4)


def cross_entropy(logits, labels, weight=None, ignore_index=-100):
    return CrossEntropyFn.apply(logits, labels, weight, ignore_index)


class DiceCELossFn(Function):
    """DiceLoss(weight, eps)(logits, labels) + nn.CrossEntropyLoss(weight)(logits, labels) (softmax, no ignore_index) as ONE node: one
    pass over the logits each way, one softmax per voxel, one logit-gradient tensor (mednet_dice_ce_fwd_lt / _bwd_lt).  Loss and
    gradient are bit for bit those of dice_loss(...) + cross_entropy(...) on the same tensors; uint8 labels are consumed where they lie."""

    @staticmethod
    def forward(ctx, logits, labels, weight, eps):
        L.require_gpu(logits, "dice_ce_loss")
        opnd = _class_loss_operands(logits, labels, weight)
        n, c, spatial = opnd[3][:3]
        ws = L.workspace(L.lib().mednet_dice_ce_ws_bytes(n, c, spatial), logits.device)
        return _class_loss_fwd(ctx, "dice_ce", logits, opnd, (2 * c + 1,), (eps,), ws)  # saved: [c][2] = {I, D}, then sum w_y

    @staticmethod
    def backward(ctx, dloss):
        return _class_loss_bwd(ctx, dloss, 4)


def dice_ce_loss(logits, labels, weight=None, eps=1e-5):
    """DiceLoss(weight=weight, epsilon=eps)(logits, labels) + nn.CrossEntropyLoss(weight)(logits, labels), softmax, unit coefficients."""
    return DiceCELossFn.apply(logits, labels, weight, eps)


class HeatmapLossFn(Function):
    """sum_c w_c * mean_{n,v} f(out[:,c] - hm[:,c])  -- landmarks.py:129-132 (f = square | abs)."""

    @staticmethod
    def forward(ctx, out, target, cweight, kind):
        L.require_gpu(out, "heatmap_loss")
        lg, sn, sc = _planar_logits(out)
        n, c = lg.shape[:2]
        spatial = lg[0, 0].numel()
        if tuple(target.shape) != tuple(lg.shape):
            raise RuntimeError(f"heatmap_loss: target shape {tuple(target.shape)} != output {tuple(lg.shape)}")
        tgt = target if target.dtype in (torch.uint8, torch.float32) else target.float()
        # channels dense, any stride between samples: the heat-map channels of a label volume are read where they lie
        tgt, tgt_sn = _dense_view(tgt, tuple(tgt.shape[1:]))
        wt = _loss_weight(cweight, lg.device)
        loss = torch.empty((), dtype=torch.float32, device=lg.device)
        lib = L.lib()
        ws = L.workspace(lib.mednet_loss_ws_bytes(n, c, spatial), lg.device)
        u8 = int(tgt.dtype == torch.uint8)
        L.check(lib.mednet_heatmap_loss_fwd_strided(lg.data_ptr(), tgt.data_ptr(), tgt_sn, L.ptr(wt), loss.data_ptr(), n, c, spatial,
                                                    sn, sc, kind, u8, ws.data_ptr(), ws.numel(), L.stream()), "heatmap_loss_fwd")
        ctx.save_for_backward(lg, tgt, wt)
        ctx.meta = (kind, u8, sn, sc, out.dtype, tgt_sn)
        ctx.split = getattr(out, "_mednet_split", None) if lg is out else None
        return loss

    @staticmethod
    def backward(ctx, dloss):
        lg, tgt, wt = ctx.saved_tensors
        kind, u8, sn, sc, in_dtype, tgt_sn = ctx.meta
        n, c = lg.shape[:2]
        spatial = lg[0, 0].numel()
        dl = dloss.to(torch.float32).contiguous()
        dout = _loss_grad_like(lg, ctx.split)
        L.check(L.lib().mednet_heatmap_loss_bwd_strided(lg.data_ptr(), tgt.data_ptr(), tgt_sn, L.ptr(wt), dl.data_ptr(), dout.data_ptr(),
                                                        n, c, spatial, sn, sc, kind, u8, L.stream()), "heatmap_loss_bwd")
        return dout.to(in_dtype), None, None, None


def heatmap_loss(out, target, channel_weights=None, kind="L2"):
    return HeatmapLossFn.apply(out, target, channel_weights, L.REG_L2 if kind == "L2" else L.REG_L1)


# ------------------------------------------------------------------------------------------------- optimiser
def adam_step_(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    """In-place Adam on flat fp32 buffers (torch.optim.Adam defaults: segmentation.py:119-120)."""
    L.require_gpu(p, "adam_step")
    L.check(L.lib().mednet_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, beta1, beta2,
                                     eps, weight_decay, step, grad_scale, L.stream()), "adam_step")


def adam_step_scaled_(p, g, m, v, lr, beta1, beta2, eps, weight_decay, scaler, inv_world=1.0):
    """The same update behind a train.LossScaler: overflow sweep, unscale, skip on overflow, scale update -- all on the device."""
    L.require_gpu(p, "adam_step_scaled")
    sc, growth, backoff, interval = _scaler_args(scaler)
    L.check(L.lib().mednet_adam_step_scaled(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, beta1, beta2, eps,
                                            weight_decay, inv_world, sc, growth, backoff, interval, L.stream()), "adam_step_scaled")


OPT_STATE_FRESH = (0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)  # {sumsq, norm, coef, nonfinite, steps taken, steps skipped, -, -}


def new_opt_state(device):
    """The 8-float device state the norm pass writes and the update kernels read (include/mednet_hip.h)."""
    return torch.tensor(OPT_STATE_FRESH, dtype=torch.float32, device=device)


def grad_norm_rows(count: int) -> int:
    """Partial rows (workgroups) of the norm pass over `count` elements; needs no GPU."""
    return L.lib().mednet_grad_norm_ws_bytes(count) // 4


def grad_norm_(g, opt_state, max_norm=None, inv_world=1.0, scaler_state=None, ws=None):
    """Global L2 norm of g * gscale (gscale = inv_world, over the loss scale when scaler_state is given) into opt_state:
    {sumsq, norm, coef = min(1, max_norm / (norm + 1e-6)), nonfinite}.  Two launches, no host synchronisation, bitwise
    reproducible.  max_norm None: coef = 1.  ws: a workspace of the caller's (at least mednet_grad_norm_ws_bytes bytes)."""
    L.require_gpu(g, "grad_norm")
    need = L.lib().mednet_grad_norm_ws_bytes(g.numel())
    if ws is None:
        ws = L.workspace(need, g.device)
    L.check(L.lib().mednet_grad_norm(g.data_ptr(), g.numel(), inv_world, L.ptr(scaler_state), 0.0 if max_norm is None else max_norm,
                                     opt_state.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(), L.stream()), "grad_norm")
    return opt_state


def _scaler_args(scaler):
    """(state pointer, growth, backoff, interval) of a train.LossScaler, or the null form."""
    if scaler is None:
        return None, 2.0, 0.5, 1
    return scaler.state.data_ptr(), scaler.growth_factor, scaler.backoff_factor, scaler.growth_interval


def sgd_step_(p, g, buf, lr, momentum=0.0, nesterov=False, weight_decay=0.0, inv_world=1.0, opt_state=None, scaler=None):
    """In-place torch.optim.SGD (dampening 0) on flat fp32 buffers behind grad_norm_: the clip coefficient and the skip rule are
    read from opt_state on the device.  buf is None when momentum == 0.  opt_state None (no scaler): the plain update, one launch."""
    L.require_gpu(p, "sgd_step")
    sc, growth, backoff, interval = _scaler_args(scaler)
    L.check(L.lib().mednet_sgd_step(p.data_ptr(), g.data_ptr(), L.ptr(buf), p.numel(), lr, momentum, int(bool(nesterov)), weight_decay,
                                    inv_world, L.ptr(opt_state), sc, growth, backoff, interval, L.stream()), "sgd_step")


def adamw_step_(p, g, m, v, lr, beta1, beta2, eps, weight_decay, opt_state, decoupled=True, inv_world=1.0, scaler=None):
    """In-place torch.optim.AdamW (decoupled) or torch.optim.Adam (not) on flat fp32 buffers behind grad_norm_; the bias correction
    uses the device-side count of steps actually taken (opt_state[4], or the scaler's)."""
    L.require_gpu(p, "adamw_step")
    sc, growth, backoff, interval = _scaler_args(scaler)
    L.check(L.lib().mednet_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, beta1, beta2, eps,
                                      weight_decay, int(bool(decoupled)), inv_world, opt_state.data_ptr(), sc, growth, backoff, interval,
                                      L.stream()), "adamw_step")
