"""SHA-256 digests of what the convolution family computes -- ops.conv3d, ops.conv3d_act, ops.conv_transpose3d, the layers and blocks
whose data gradients take a neighbour's sums (GNBHook / BNBHook, GN3Hook into a ConvTranspose3d and into the 1x1x1 head), two whole
networks -- on seeded random fp32 inputs that are NOT numbers of the storage type: two commits whose host code launches the same
kernels with the same arguments print the same lines.  Only the package's public surface is used, so the tool runs against any
commit's package and library:
HD_PKG=<directory that holds that commit's mednet_hip/> MEDNET_LIB_PATH=<its libmednet_hip.so> python tools/conv_digest.py
(as tools/norm_digest.py); without them it takes this tree's.  One process per package; compare the outputs with diff.

One JSON line per case: its name and ONE SHA-256 over the digests of every tensor it returns and every gradient, in every storage
mode (fp32, bf16, fp16, fp16x2 = split weights), at every shape of the case and in both execution modes: "plain" (autograd owns
the gradients) and "trainer" (train.FlatParams gives the kernels in-place gradient targets and the weight gradients go to the side
stream).  DIGEST_FULL=1 adds each tensor's digest under "mode/exec/shape/tensor".
Shapes (n, (d, h, w)), as tools/conv_routes.py shows what reaches which kernel: (2, (3, 5, 7)) below one brick; (1, (9, 17, 20)) odd,
18 bricks -- conv2b's row-per-brick form under split weights, wgrad_mfma4_kernel; (2, (32, 32, 8)) narrow: 8-wide bricks,
wgrad_mfma2_kernel<8>; (2, (32, 32, 32)): 128 bricks -- conv2b's accumulating form under split weights, and for a ConvTranspose3d
input 512 bricks of its data gradient, convt_dgrad32_mfma_kernel; (1, (64, 64, 64)), 512 bricks, for 32 -> 32 (conv32_mfma_kernel)
and 64 -> 64 (conv2b_mfma_kernel) only.  ConvTranspose3d, the layers and the blocks run at the first four (their outputs are eight
times the input, or their inner layers repeat the above); the networks at (2, (32, 32, 32)) and (1, (8, 16, 20)): the odd shape
with its extents made even for the one pooling level.
The last line holds ops.GN3_COUNT and block.C1GN_COUNT: that the fused forms really ran, equally on both sides.
Usage: python tools/conv_digest.py [forms, default all] > digest.jsonl"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("HD_PKG") or os.path.join(ROOT, "torch-mednet_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import mednet_hip  # noqa: E402
from mednet_hip import _lib as L  # noqa: E402
from mednet_hip import block, ops, train  # noqa: E402
from mednet_hip import nn as hnn  # noqa: E402
from mednet_hip.unet import components as HC  # noqa: E402
from mednet_hip.unet import model as HM  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

DEV = "cuda:0"
BELOW, ODD, NARROW, CUBE, BIG = (2, (3, 5, 7)), (1, (9, 17, 20)), (2, (32, 32, 8)), (2, (32, 32, 32)), (1, (64, 64, 64))
MODES = ("fp32", "bf16", "fp16", "fp16x2")
PAIRS = ((1, 32), (3, 32), (16, 16), (32, 32), (64, 64), (32, 64), (24, 24))
FULL = os.environ.get("DIGEST_FULL", "0") == "1"
FORMS = (sys.argv[1] if len(sys.argv) > 1 else "conv,act,convt,double,block,junction,net").split(",")
_CACHE = {}


def rnd(tag, *shape):
    """Seeded on the CPU by the tag alone; cached, so every case of a shape sees the same tensor."""
    if (tag, shape) not in _CACHE:
        g = torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(tag.encode()).digest()[:6], "little"))
        _CACHE[(tag, shape)] = torch.randn(*shape, generator=g, dtype=torch.float32)
    return _CACHE[(tag, shape)]


def digest(t):
    if t is None:
        return None
    t = t.detach().contiguous().cpu()
    if t.dtype in (torch.bfloat16, torch.float16):
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def leaf(tag, n, c, *shape):
    """The network input (1 to 4 channels: planar fp32) or a channels-last leaf in the mode's storage type."""
    x = rnd(tag, n, c, *shape).to(DEV)
    return (x if c <= 4 else ops.to_cl(x.to(mednet_hip.config.act_dtype()))).requires_grad_(True)


class Run:
    """One forward + backward of `modules` in an execution mode: `trainer` re-homes their parameters (train.FlatParams) so that the
    kernels write the gradients in place, and enables the side stream for the weight gradients, as train._GraphedStep does."""

    def __init__(self, trainer, *modules):
        self.trainer, self.modules = trainer, modules
        self.holder = torch.nn.ModuleList(modules)
        self.flat = train.FlatParams(self.holder) if trainer and any(True for _ in self.holder.parameters()) else None
        ops.SIDE["enabled"] = trainer

    def backward(self, outs, mode):
        """Backward of sum(out * seeded weights) over the outputs (scaled as train.LossScaler does where fp16 stores gradients)."""
        try:
            total = sum((o.float() * rnd(f"lw{i}", *o.shape).to(DEV)).sum() for i, o in enumerate(outs))
            (total * (1024.0 if mode.startswith("fp16") else 1.0)).backward()
            ops.join_side_stream()
            torch.cuda.synchronize()
        finally:
            ops.SIDE["enabled"] = False

    def grads(self):
        if self.flat is not None:
            self.flat.grads_as_attr()
        out = {"d_" + k: digest(p.grad) for k, p in self.holder.named_parameters()}
        if self.flat is not None:
            self.flat.release()
        return out


def init(m):
    return O.keyed_init_(m).to(DEV)


def conv_cases():
    for cin, cout in PAIRS:
        for k, bias, planar, stats in ((3, 0, 0, 0), (3, 1, 0, 0), (3, 0, 0, 1), (3, 0, 1, 0), (1, 1, 1, 0), (1, 0, 0, 0)):
            shapes = (BELOW, ODD, NARROW, CUBE) + ((BIG,) if k == 3 and (cin, cout) in ((32, 32), (64, 64)) else ())
            yield f"conv3d k={k} {cin}->{cout} bias={bias} planar={planar} stats={stats}", shapes, (cin, cout, k, bias, planar, stats)


def conv(mode, trainer, n, shape, cin, cout, k, bias, planar, stats):
    m = init(hnn.Conv3d(cin, cout, k, bias=bool(bias), planar_output=bool(planar)))
    run = Run(trainer, m)
    x = leaf(f"x{cin}", n, cin, *shape)
    y, partial = m.forward_with_stats(x) if stats else (m(x), None)
    run.backward([y], mode)
    return {"y": digest(y), "rows": None if partial is None else partial.shape[1], "partial": digest(partial), "dx": digest(x.grad), **run.grads()}


def act_cases():
    for act in (L.ACT_NONE, L.ACT_RELU, L.ACT_LEAKY, L.ACT_ELU):
        for stats in (0, 1):
            for cin, cout in ((32, 32), (16, 64)):
                yield f"conv3d_act act={act} {cin}->{cout} stats={stats}", (BELOW, ODD, NARROW, CUBE), (cin, cout, act, stats)


def conv_act(mode, trainer, n, shape, cin, cout, act, stats):
    if mode == "fp32":
        return {"skipped": "16-bit storage only"}  # (ops.conv3d_act_supported answers False: the layers take ops.conv3d + activation)
    m = init(hnn.Conv3d(cin, cout, 3, bias=False))
    run = Run(trainer, m)
    x = leaf(f"x{cin}", n, cin, *shape)
    z, partial = ops.conv3d_act(x, m.weight, m._packed(x), act, want_stats=bool(stats))
    run.backward([z], mode)
    return {"z": digest(z), "rows": None if partial is None else partial.shape[1], "partial": digest(partial), "dx": digest(x.grad), **run.grads()}


def convt_cases():
    for cin, cout in ((64, 32), (32, 32)):
        for skip in (0, 1):
            for bias in (0, 1):
                yield f"conv_transpose3d {cin}->{cout} skip={skip} bias={bias}", (BELOW, ODD, NARROW, CUBE), (cin, cout, skip, bias)


def convt(mode, trainer, n, shape, cin, cout, skip, bias):
    m = init(hnn.ConvTranspose3d(cin, cout))
    if not bias:
        m.bias = None
    run = Run(trainer, m)
    x = leaf(f"x{cin}", n, cin, *shape)
    sk = leaf(f"s{cout}", n, cout, *[2 * s for s in shape]) if skip else None
    y = ops.conv_transpose3d(x, m.weight, m.bias, sk, m._packed(x, converts=True))
    run.backward([y], mode)
    return {"y": digest(y), "dx": digest(x.grad), "dskip": digest(sk.grad if skip else None), **run.grads()}


def double_cases():
    for order in ("gcr", "cbe"):
        for c in (16, 32, 64):
            yield f"double {order} C={c}", (BELOW, ODD, NARROW, CUBE), (order, c)


def double(mode, trainer, n, shape, order, c):
    m = init(HC.DoubleConv(c, c, encoder=False, order=order, num_groups=8))
    run = Run(trainer, m)
    x = leaf(f"x{c}", n, c, *shape)
    out = m(x)
    run.backward([out], mode)
    return {"out": digest(out), "dx": digest(x.grad), **run.grads()}


def block_cases():
    for cin, c in ((1, 32), (3, 32), (32, 32), (64, 64), (24, 24)):
        yield f"block cge {cin}->{c}", (BELOW, ODD, NARROW, CUBE), (cin, c)


def resblock(mode, trainer, n, shape, cin, c):
    m = init(HC.ExtResNetBlock(cin, c, order="cge", num_groups=8))
    run = Run(trainer, m)
    x = leaf(f"x{cin}", n, cin, *shape)
    out = m(x)
    run.backward([out], mode)
    return {"out": digest(out), "dx": digest(x.grad), **run.grads()}


def junction_cases():
    yield "block -> conv_transpose3d 64->32", (BELOW, ODD, NARROW, CUBE), ("convt", 64, 32)
    yield "block -> conv_transpose3d 32->32", (BELOW, ODD, NARROW, CUBE), ("convt", 32, 32)
    for c in (16, 32, 64):
        yield f"block -> head {c}->3", (BELOW, ODD, NARROW, CUBE), ("head", c, 3)


def junction(mode, trainer, n, shape, kind, c, cout):
    """An ExtResNetBlock whose output feeds a ConvTranspose3d (the stride-2 data gradient takes the block's GroupNorm-3 sums) or the
    1x1x1 head (mednet_head_dgrad_gn)."""
    b = init(HC.ExtResNetBlock(c, c, order="cge", num_groups=8))
    top = init(hnn.ConvTranspose3d(c, cout) if kind == "convt" else hnn.Conv3d(c, cout, 1, bias=True, planar_output=True))
    run = Run(trainer, b, top)
    x = leaf(f"x{c}", n, c, *shape)
    out = top(b(x))
    run.backward([out], mode)
    return {"out": digest(out), "dx": digest(x.grad), **run.grads()}


def net_cases():
    for kind in ("res", "unet_gcr"):
        yield f"net {kind}", (CUBE, ODD), (kind,)


def net(mode, trainer, n, shape, kind):
    shape = tuple(max(s // 2 * 2, 2) for s in shape)  # (one pooling level)
    if kind == "res":
        m = HM.ResidualUNet3D(1, 2, False, f_maps=[32, 64])
    else:
        m = HM.UNet3D(1, 2, False, f_maps=[32, 64], layer_order="gcr")
    m = init(m)
    run = Run(trainer, m)
    out = m(rnd("in1", n, 1, *shape).to(DEV))
    run.backward([out], mode)
    return {"out": digest(out), **run.grads()}


RUN = {"conv": (conv_cases, conv), "act": (act_cases, conv_act), "convt": (convt_cases, convt), "double": (double_cases, double),
       "block": (block_cases, resblock), "junction": (junction_cases, junction), "net": (net_cases, net)}
for form in FORMS:
    cases, fn = RUN[form]
    for name, shapes, axes in cases():
        res = {}
        for mode in MODES:
            for trainer in (False, True):
                for n, shape in shapes:
                    with mednet_hip.precision(mode):
                        try:
                            out = fn(mode, trainer, n, shape, *axes)
                        except (RuntimeError, NotImplementedError, AssertionError) as e:
                            # a refusal (shape, dtype, workspace, unsupported) is part of the record; a device error ends the run
                            if isinstance(e, RuntimeError) and not any(f"failed ({rc})" in str(e) for rc in (-1, -2, -3, -5)):
                                raise
                            out = {"error": f"{type(e).__name__}: {e}"}
                            print(f"{name} {mode} {shape}: {out['error']}", file=sys.stderr, flush=True)
                        finally:
                            ops.SIDE["enabled"] = False
                        for k, v in out.items():
                            res[f"{mode}/{'trainer' if trainer else 'plain'}/{'x'.join(map(str, shape))}/{k}"] = v
        line = {"case": name, "tensors": len(res), "sha256": hashlib.sha256("".join(f"{k}={v};" for k, v in res.items()).encode()).hexdigest()}
        print(json.dumps({**line, **res} if FULL else line), flush=True)
        torch.cuda.empty_cache()
print(json.dumps({"GN3_COUNT": ops.GN3_COUNT, "C1GN_COUNT": block.C1GN_COUNT}), flush=True)
