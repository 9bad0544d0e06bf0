"""SHA-256 digests of what the normalisation family computes -- ops.group_norm_act, ops.batch_norm_act, the layers and blocks that
fuse their passes into neighbours (GNBHook / BNBHook, GN3Hook, the lazy pooling join, the pooled apply, the first layer's
mednet_gn_bwd_coefficients path, upsample_concat's statistics) -- on seeded random fp32 inputs that are NOT numbers of the storage
type: two commits whose host code launches the same kernels with the same arguments print the same lines.  Only the package's public
surface is used, so the tool runs against any commit's package and library:
HD_PKG=<directory that holds that commit's mednet_hip/> MEDNET_LIB_PATH=<its libmednet_hip.so> python tools/norm_digest.py
(as tools/head_digest.py); without them it takes this tree's.  One process per package; compare the outputs with diff.

One JSON line per case: its name and ONE SHA-256 over the digests of every tensor it returns and every gradient, in every storage
mode (fp32, bf16, fp16) and at every shape of the case (DIGEST_FULL=1 adds each tensor's digest under "mode/shape/tensor").
Shapes: (12, 10, 6) with n = 3 (even extents: the pooled apply and the lazy pooling join run; one chunk per sample) and
(24, 20, 21) with n = 2 (an odd extent: the unfused forms; a ragged last chunk).  (C, groups): (16, 8) two columns, LDS-free sums,
one-launch backward; (24, 8) three channels per group -> the three-kernel backward, three columns -> column_reduce; (12, 4) the
scalar 16-bit path and the width-4 fp32 path; (512, 8) 64 columns and (1024, 8) 128 columns, two rows per workgroup, both at the
small shape only.  Forms: "gn" (every activation x residual x affine), "bn" (training / evaluation / untracked x residual),
"double" (DoubleConv 'gcr', 'cge', 'cbe': the second convolution's data gradient takes the first backward pass of the norm in front
of it), "block" (ExtResNetBlock alone), "encoder" (two ExtResNetBlock levels joined by max / average pooling, 1, 3 and 16 input
channels), "net" (ResidualUNet3D and UNet3D 'gcr', 1 and 3 input channels, small shape), "upcat" (upsample_concat(want_stats=True)
into a GroupNorm), "head" (ExtResNetBlock(32) -> ops.head_dice / head_ce / head_dice_ce, 2 to 4 classes, 16-bit storage, the block told
that the head is its sole consumer: the GroupNorm-3 apply pass rebuilds the head's feature gradient; N = 2 at (8, 8, 16), whole
trips, and (5, 7, 9), 315 voxels: rows with five voxels, a last trip with one), "pool" (ops.pool2 and ops.skip_pool2 alone, max and
average, C in {8, 16, 24}, small shape: without and with the skip gradient, behind a 'gcr' DoubleConv whose ReLU mask the join folds
in, with the skip gradient as the leading channels of a concatenation's gradient; max pooling also on inputs with ties and with NaNs
inside windows).  The last line holds ops.GN3_COUNT and block.C1GN_COUNT: that the fused forms really ran, equally on both sides.
Usage: python tools/norm_digest.py [forms, default all] > digest.jsonl"""
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
from mednet_hip import block, ops  # noqa: E402
from mednet_hip import nn as hnn  # noqa: E402
from mednet_hip.unet import components as HC  # noqa: E402
from mednet_hip.unet import model as HM  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

DEV = "cuda:0"
SMALL, ODD = (3, (12, 10, 6)), (2, (24, 20, 21))
MODES = ("fp32", "bf16", "fp16")
CG = ((16, 8), (24, 8), (12, 4), (512, 8), (1024, 8))
FULL = os.environ.get("DIGEST_FULL", "0") == "1"
FORMS = (sys.argv[1] if len(sys.argv) > 1 else "gn,bn,double,block,encoder,net,upcat,head,pool").split(",")
HALF = ("bf16", "fp16")
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


def shapes_of(c):
    return (SMALL,) if c >= 512 else (SMALL, ODD)


def leaf(tag, *shape):
    """A channels-last leaf in the mode's storage type."""
    return ops.to_cl(rnd(tag, *shape).to(DEV).to(mednet_hip.config.act_dtype())).requires_grad_(True)


def param(tag, c, shift=0.0):
    return (rnd(tag, c) * 0.5 + shift).to(DEV).requires_grad_(True)


def backward(outs, mode):
    """Backward of sum(out * seeded weights) over the outputs (scaled as train.LossScaler does where fp16 stores gradients)."""
    total = sum((o.float() * rnd(f"lw{i}", *o.shape).to(DEV)).sum() for i, o in enumerate(outs))
    (total * (1024.0 if mode == "fp16" else 1.0)).backward()
    torch.cuda.synchronize()


def grads(module):
    return {"d_" + k: digest(p.grad) for k, p in module.named_parameters()}


def gn_cases():
    for c, g in CG:
        for act in (L.ACT_NONE, L.ACT_RELU, L.ACT_LEAKY, L.ACT_ELU):
            for res in (False, True):
                for affine in (True, False):
                    yield f"gn C={c} groups={g} act={act} residual={int(res)} affine={int(affine)}", shapes_of(c), (c, g, act, res, affine)


def gn(mode, n, shape, c, g, act, res, affine):
    x = leaf(f"x{c}", n, c, *shape)
    r = leaf(f"r{c}", n, c, *shape) if res else None
    gamma, beta = (param("gamma", c, 1.0), param("beta", c)) if affine else (None, None)
    z = ops.group_norm_act(x, gamma, beta, g, 1e-5, act, r)
    backward([z], mode)
    return {"z": digest(z), "dx": digest(x.grad), "dres": digest(r.grad if res else None),
            "dgamma": digest(gamma.grad if affine else None), "dbeta": digest(beta.grad if affine else None)}


def bn_cases():
    for c, _ in CG:
        for how in ("train", "eval", "untracked"):
            for res in (False, True):
                yield f"bn C={c} {how} residual={int(res)}", shapes_of(c), (c, how, res)


def bn(mode, n, shape, c, how, res):
    x = leaf(f"x{c}", n, c, *shape)
    r = leaf(f"r{c}", n, c, *shape) if res else None
    gamma, beta = param("gamma", c, 1.0), param("beta", c)
    rm, rv = (rnd("rm", c) * 0.1).to(DEV), (rnd("rv", c).abs() + 0.5).to(DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    running = (None, None, None) if how == "untracked" else (rm, rv, nbt)
    z = ops.batch_norm_act(x, gamma, beta, *running, how != "eval", 0.1, 1e-5, L.ACT_ELU if res else L.ACT_RELU, r)
    backward([z], mode)
    return {"z": digest(z), "dx": digest(x.grad), "dres": digest(r.grad if res else None), "dgamma": digest(gamma.grad),
            "dbeta": digest(beta.grad), "running_mean": digest(rm), "running_var": digest(rv), "batches": digest(nbt)}


def double_cases():
    for order in ("gcr", "cge", "cbe"):
        for c, g in ((16, 8), (24, 8), (32, 8)):
            yield f"double {order} C={c} groups={g}", (SMALL, ODD), (order, c, g)


def double(mode, n, shape, order, c, g):
    m = O.keyed_init_(HC.DoubleConv(c, c, encoder=False, order=order, num_groups=g)).to(DEV)
    x = leaf(f"x{c}", n, c, *shape)
    out = m(x)
    backward([out], mode)
    return {"out": digest(out), "dx": digest(x.grad), **grads(m)}


def block_cases():
    for c, g in ((16, 8), (24, 8), (32, 8), (12, 4)):
        yield f"block cge C={c} groups={g}", (SMALL, ODD), (c, g)


def resblock(mode, n, shape, c, g):
    m = O.keyed_init_(HC.ExtResNetBlock(c, c, order="cge", num_groups=g)).to(DEV)
    x = leaf(f"x{c}", n, c, *shape)
    out = m(x)
    backward([out], mode)
    return {"out": digest(out), "dx": digest(x.grad), **grads(m)}


def encoder_cases():
    for cin in (1, 3, 16):
        for pool in ("max", "avg"):
            yield f"encoder cin={cin} pool={pool}", (SMALL, ODD), (cin, pool)


def encoder(mode, n, shape, cin, pool):
    """Two levels as the U-Net's forward joins them: the first block writes the pooled tensor too, the second level's pooling and the
    skip consumer meet in one node that may leave the block's output gradient unwritten."""
    e0 = O.keyed_init_(HC.Encoder(cin, 16, apply_pooling=False, basic_module=HC.ExtResNetBlock, conv_layer_order="cge")).to(DEV)
    e1 = O.keyed_init_(HC.Encoder(16, 32, apply_pooling=True, pool_type=pool, basic_module=HC.ExtResNetBlock,
                                  conv_layer_order="cge")).to(DEV)
    x = rnd(f"in{cin}", n, cin, *shape).to(DEV) if cin <= 4 else leaf(f"x{cin}", n, cin, *shape)
    x0 = e0(x, pool_next=e1.pooling.mode)
    skip, x1 = e1(x0, with_skip=True, sole_consumer=True)
    backward([skip, x1], mode)
    return {"skip": digest(skip), "out": digest(x1), "dx": digest(x.grad), **grads(e0), **{"1" + k: v for k, v in grads(e1).items()}}


def net_cases():
    for kind in ("res", "unet_gcr"):
        for cin in (1, 3):
            yield f"net {kind} cin={cin}", (SMALL,), (kind, cin)


def net(mode, n, shape, kind, cin):
    if kind == "res":
        m = HM.ResidualUNet3D(cin, 2, False, f_maps=[16, 32])
    else:
        m = HM.UNet3D(cin, 2, False, f_maps=[16, 32], layer_order="gcr")
    m = O.keyed_init_(m).to(DEV)
    out = m(rnd(f"in{cin}", n, cin, *shape).to(DEV))
    backward([out], mode)
    return {"out": digest(out), **grads(m)}


def upcat_cases():
    for ce, cx, g in ((16, 32, 8), (8, 8, 8)):
        yield f"upcat {ce}+{cx} groups={g}", (SMALL, ODD), (ce, cx, g)


def upcat(mode, n, shape, ce, cx, g):
    enc = leaf(f"x{ce}", n, ce, *shape)
    x = leaf(f"u{cx}", n, cx, *[max(s // 2, 1) for s in shape])
    gamma, beta = param("gamma", ce + cx, 1.0), param("beta", ce + cx)
    cat, partial = ops.upsample_concat(enc, x, want_stats=True)
    z = ops.group_norm_act(cat, gamma, beta, g, 1e-5, L.ACT_RELU, None, partial)
    backward([z], mode)
    return {"z": digest(z), "rows": None if partial is None else partial.shape[1], "partial": digest(partial), "denc": digest(enc.grad),
            "dx": digest(x.grad), "dgamma": digest(gamma.grad), "dbeta": digest(beta.grad)}


def head_cases():
    for kind in ("head_dice", "head_ce", "head_dice_ce"):
        for cout in (2, 3, 4):
            yield f"head {kind} classes={cout}", ((2, (8, 8, 16)), (2, (5, 7, 9))), (kind, cout)


def head(mode, n, shape, kind, cout):
    blk = O.keyed_init_(HC.ExtResNetBlock(32, 32)).to(DEV)
    conv = O.keyed_init_(hnn.Conv3d(32, cout, 1, planar_output=True)).to(DEV)
    x = leaf("x32", n, 32, *shape)
    lab = (rnd(f"lab{cout}", n, *shape).abs() * 1.5).floor().clamp_(0, cout - 1).to(torch.uint8).to(DEV)
    wt = torch.tensor([0.05, 1.0, 0.7, 1.3][:cout], device=DEV)
    out = blk(x, head_next=True)
    logits, loss = getattr(ops, kind)(out, conv.weight, conv.bias, conv._packed(), lab, wt)
    (loss * (1024.0 if mode == "fp16" else 1.0)).backward()
    torch.cuda.synchronize()
    return {"logits": digest(logits), "loss": digest(loss), "dx": digest(x.grad), **grads(blk), **{"h" + k: v for k, v in grads(conv).items()}}


def pool_cases():
    for pool in ("max", "avg"):
        for c in (8, 16, 24):
            for form in ("pool2", "noskip", "skip", "act", "slice", "act_slice"):
                yield f"pool {form} {pool} C={c}", (SMALL,), (form, pool, c, None)
    for special in ("tie", "nan"):
        for c in (8, 16):
            for form in ("pool2", "skip", "slice"):
                yield f"pool {form} max C={c} input={special}", (SMALL,), (form, "max", c, special)


def pool(mode, n, shape, form, how, c, special):
    pmode = L.POOL_MAX if how == "max" else L.POOL_AVG
    v = rnd(f"x{c}", n, c, *shape)
    if special is not None:
        v = (v * 2).round() / 2  # half-integers: most windows hold their maximum more than once
    if special == "nan":
        v = torch.where(rnd(f"nan{c}", n, c, *shape) > 1.5, torch.full_like(v, float("nan")), v)  # ~7 % of the elements
    x = ops.to_cl(v.to(DEV).to(mednet_hip.config.act_dtype())).requires_grad_(True)
    res, front, src = {}, None, x
    if form.startswith("act"):
        front = O.keyed_init_(HC.DoubleConv(c, c, encoder=False, order="gcr", num_groups=4 if c == 8 else 8)).to(DEV)
        src = front(x)
        res["masked"] = getattr(src, "_mednet_actmask", None) is not None
    if form == "pool2":
        outs = [ops.pool2(src, pmode)]
    else:
        skip, y = ops.skip_pool2(src, pmode)
        outs = [y] if form == "noskip" else [skip, y]
        if form.endswith("slice"):  # the skip gradient arrives as the leading channels of the concatenation's gradient
            up = leaf("u8", n, 8, *[s // 2 for s in shape])
            outs = [ops.upsample_concat(skip, up), y]
    backward(outs, mode)
    res.update({f"out{i}": digest(o) for i, o in enumerate(outs)})
    res["dx"] = digest(x.grad)
    if front is not None:
        res.update(grads(front))
    if form.endswith("slice"):
        res["dup"] = digest(up.grad)
    return res


RUN = {"gn": (gn_cases, gn), "bn": (bn_cases, bn), "double": (double_cases, double), "block": (block_cases, resblock),
       "encoder": (encoder_cases, encoder), "net": (net_cases, net), "upcat": (upcat_cases, upcat), "head": (head_cases, head),
       "pool": (pool_cases, pool)}
for form in FORMS:
    cases, fn = RUN[form]
    for name, shapes, axes in cases():
        res = {}
        for mode in (HALF if form == "head" else MODES):
            for n, shape in shapes:
                with mednet_hip.precision(mode):
                    try:
                        out = fn(mode, n, shape, *axes)
                    except (RuntimeError, NotImplementedError, AssertionError) as e:
                        # a refusal (shape, dtype, workspace, unsupported) is part of the record; a device error ends the run
                        if isinstance(e, RuntimeError) and not any(f"failed ({rc})" in str(e) for rc in (-1, -2, -3, -5)):
                            raise
                        out = {"error": f"{type(e).__name__}: {e}"}
                        print(f"{name} {mode} {shape}: {out['error']}", file=sys.stderr, flush=True)
                    for k, v in out.items():
                        res[f"{mode}/{'x'.join(map(str, shape))}/{k}"] = v
        line = {"case": name, "tensors": len(res), "sha256": hashlib.sha256("".join(f"{k}={v};" for k, v in res.items()).encode()).hexdigest()}
        print(json.dumps({**line, **res} if FULL else line), flush=True)
        torch.cuda.empty_cache()
print(json.dumps({"GN3_COUNT": ops.GN3_COUNT, "C1GN_COUNT": block.C1GN_COUNT}), flush=True)
