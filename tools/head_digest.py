"""SHA-256 digests of what the fused head + loss nodes compute -- the matrix-core landmark head (ops.head_landmark / _eval), the
matrix-core segmentation head for 5-16 classes (ops.head_seg), the VALU heads for <= 4 classes (ops.head_dice / ops.head_ce /
ops.head_dice_ce) and the stand-alone class losses (ops.dice_loss / cross_entropy / dice_ce_loss / per_channel_dice) -- on
seeded random fp32 inputs that are NOT numbers of the storage type: two commits whose kernels run the same arithmetic in the same
order print the same lines.  Only the package's public surface is used, so the tool runs against any commit's package and library:
HD_PKG=<directory that holds that commit's mednet_hip/> MEDNET_LIB_PATH=<its libmednet_hip.so> python tools/head_digest.py
(as tools/first_layer_digest.py); without them it takes this tree's.  One process per package; compare the outputs with diff.

A case is one combination of a head's own axes (below); it runs in every storage mode of that head, both forms and both shapes.
One JSON line per case: its name and ONE SHA-256 over the digests of all its tensors (DIGEST_FULL=1 adds the digest of every
tensor under "mode/form/shape/tensor", to find which one moved).  form = "op": the node on random features, no GroupNorm hook -> the losses (the Dice metric of the _eval
form), the logits where the node returns them, dx, dw, db (the `saved` sums show through the backward).  form = "block": the
features come out of ExtResNetBlock(cin, cin, "cge"), so the node takes the first pass of that block's GroupNorm-3 backward ->
the losses and every parameter gradient of block and head.
Shapes: (12, 10, 6) with n = 3 (720 voxels: five whole runs of 128 and a ragged sixth, one chunk of 64 runs) and (24, 20, 21) with
n = 2 (10080 voxels: two chunks, the second short with a ragged last run).
Cases.  landmark (bf16, fp16): (nh, ncls, regression) in {(16, 2, L2), (5, 3, L1), (1, 4, L2)} x class loss Dice softmax / Dice
sigmoid / CE x class and regression weights on / off, one ignore_index case per class loss; head_landmark_eval on the same inputs is
part of every softmax case without a Dice mask.  seg (bf16, fp16): C in {5, 8, 9, 16} x the three losses x want_logits x weights,
one ignore_index case per loss, labels at an odd byte offset once per loss.  valu (fp32, bf16, fp16): head_dice / head_ce /
head_dice_ce x cin in {16, 32, 64} x C in {1, 2, 4} x uint8 / int64 labels, and once per loss the features out of a fused conv ->
ReLU layer (SingleConv 'gcr', the end of UNet3D's last block: the backward that folds the activation's derivative in).  loss (planar
fp32 logits, the two shapes; tensors: the loss, the gradient of the logits, the metric): dice_loss / cross_entropy / dice_ce_loss /
per_channel_dice x C in {1, 2, 3, 4, 5, 8, 9, 16, 17, 32} (every class bucket of the kernels at its top and just past its bottom) x
class weights on / off x uint8 / int64 labels; Dice sigmoid at C in {1, 4}; one ignore_index case for Dice and for CE; once per
function the logits as a channel slice of a wider tensor, the uint8 labels as the last channel of a label volume, and an
out-of-range label (the NaN pattern is hashed like anything else).  ds (bf16, fp16; the deep-supervision node ops.ds_head, which has its own runs:
n = 2, with and without the next decoder's gradient d_pass, tensors loss, dx, dw, db): (level, shift, cin, C) as
tests/test_gpu_ds_head.py's CASES -- one run of 128 voxels, a ragged run, five workgroups, 2 / 4 / 8 tiles, C in {1, 2, 4, 5, 8, 16} --
and C = 9 at (6, 6, 6), shift 1, cin 128, x Dice softmax / Dice sigmoid / CE / Dice + CE x weights, one ignore_index case for Dice
and for CE.
Usage: python tools/head_digest.py [heads, default landmark,seg,valu; all: landmark,seg,valu,ds,loss] > digest.jsonl"""
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
from mednet_hip import nn as hnn  # noqa: E402
from mednet_hip import ops  # noqa: E402
from mednet_hip.unet import components as HC  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

DEV = "cuda:0"
SHAPES = [(3, (12, 10, 6)), (2, (24, 20, 21))]
FULL = os.environ.get("DIGEST_FULL", "0") == "1"
HEADS = (sys.argv[1] if len(sys.argv) > 1 else "landmark,seg,valu").split(",")
_CACHE = {}


def _gen(tag):
    return torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(tag.encode()).digest()[:6], "little"))


def rnd(tag, *shape):
    """Seeded on the CPU by the tag alone; cached, so every case of a shape sees the same tensor."""
    if (tag, shape) not in _CACHE:
        _CACHE[(tag, shape)] = torch.randn(*shape, generator=_gen(tag), dtype=torch.float32)
    return _CACHE[(tag, shape)]


def labels(tag, hi, *shape):
    """uint8 values in [0, hi), seeded by the tag."""
    if (tag, hi, shape) not in _CACHE:
        _CACHE[(tag, hi, shape)] = torch.randint(0, hi, shape, generator=_gen(tag), dtype=torch.uint8)
    return _CACHE[(tag, hi, shape)]


def digest(t):
    if t is None:
        return None
    t = t.detach().contiguous().cpu()
    if t.dtype in (torch.bfloat16, torch.float16):
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def weights(c):
    return torch.tensor([0.05] + [0.6 + 0.1 * (k % 7) for k in range(1, c)])


def features(form, cin, n, shape):
    """-> (features for the head, the leaf to read dx from or None, the block or None)."""
    x = rnd(f"x{cin}", n, cin, *shape).to(DEV)
    if form == "op":
        xg = ops.to_cl(x.to(mednet_hip.config.act_dtype())).requires_grad_(True)
        return xg, xg, None
    if form == "fold":  # GroupNorm -> conv -> ReLU, the conv and the ReLU in one kernel where the mode has it
        blk = O.keyed_init_(HC.SingleConv(cin, cin, order="gcr", num_groups=8)).to(DEV)
    else:
        blk = O.keyed_init_(HC.ExtResNetBlock(cin, cin, order="cge", num_groups=8)).to(DEV)
    return blk(x), None, blk


def head_conv(cin, cout):
    conv = hnn.Conv3d(cin, cout, 1, planar_output=True).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(rnd(f"w{cin}_{cout}", cout, cin, 1, 1, 1) * 0.3)
        conv.bias.copy_(rnd(f"b{cout}", cout))
    return conv


def finish(out, total, leaf, blk, conv, mode):
    """Backward of `total` (scaled as train.LossScaler does where fp16 stores the feature gradient) and the gradients' digests."""
    (total * (3.0 * 16384.0 if mode == "fp16" else 3.0)).backward()
    torch.cuda.synchronize()
    if leaf is not None:
        out["dx"] = digest(leaf.grad)
    out["dw"], out["db"] = digest(conv.weight.grad), digest(conv.bias.grad)
    if blk is not None:
        for k, p in blk.named_parameters():
            out["d_" + k] = digest(p.grad)
    return out


def sh(shape):
    return "x".join(map(str, shape))


def landmark_cases():
    for nh, ncls, kind in ((16, 2, "L2"), (5, 3, "L1"), (1, 4, "L2")):
        cases = [(cl, sig, wtd, None) for cl, sig in (("DICE", False), ("DICE", True), ("CE", False)) for wtd in (True, False)]
        for cl, sig, wtd, ign in cases + ([("DICE", False, True, 1), ("CE", False, True, 1)] if ncls == 3 else []):
            yield f"landmark nh={nh} ncls={ncls} {kind} {cl} sig={int(sig)} w={int(wtd)} ign={ign}", (nh, ncls, kind, cl, sig, wtd, ign)


def landmark(mode, form, n, shape, nh, ncls, kind, cl, sig, wtd, ign):
    hm = labels(f"hm{nh}", 256, n, nh, *shape).to(DEV)
    lab = labels(f"lab{ncls}", ncls, n, *shape).to(DEV)
    cw = weights(ncls).to(DEV) if wtd else None
    rw = [0.015 + 0.003 * i for i in range(nh)] if wtd else None
    x, leaf, blk = features(form, 32, n, shape)
    fc = head_conv(32, nh + ncls)
    if not ops.head_landmark_supported(x, 32, nh, ncls, hm, lab):
        raise RuntimeError("head_landmark does not take this case")
    closs, rloss = ops.head_landmark(x, fc.weight, fc.bias, fc._packed(), hm, lab, cw, rw, kind, 1e-5, sig, ign, cl)
    out = finish({"class_loss": digest(closs), "reg_loss": digest(rloss)}, closs * 0.75 + rloss * 1.25, leaf, blk, fc, mode)
    if form == "op" and not sig and not (cl == "DICE" and ign is not None):  # (the metric is a softmax form without a mask)
        with torch.no_grad():
            ev = ops.head_landmark_eval(x.detach(), fc.weight, fc.bias, fc._packed(), hm, lab, cw, rw, kind, 1e-5, ign, cl)
        torch.cuda.synchronize()
        out.update({"eval_class_loss": digest(ev[0]), "eval_reg_loss": digest(ev[1]), "eval_dice": digest(ev[2])})
    return out


def seg_cases():
    for c in (5, 8, 9, 16):
        cases = [(cl, sig, wtd, None, wl, False) for cl, sig in (("DICE", False), ("DICE", True), ("CE", False)) for wtd in (True, False)
                 for wl in (False, True)]
        if c == 9:
            cases += [("DICE", False, True, 2, False, False), ("CE", False, True, 3, False, False),
                      ("DICE", False, False, None, False, True), ("CE", False, False, None, False, True)]
        for cl, sig, wtd, ign, wl, odd in cases:
            yield f"seg C={c} {cl} sig={int(sig)} w={int(wtd)} ign={ign} logits={int(wl)} odd={int(odd)}", (c, cl, sig, wtd, ign, wl, odd)


def seg(mode, form, n, shape, c, cl, sig, wtd, ign, wl, odd):
    lab = labels(f"lab{c}", c, n, *shape).to(DEV)
    if odd:  # the same labels behind an odd base address
        buf = torch.zeros(lab.numel() + 1, dtype=torch.uint8, device=DEV)
        buf[1:] = lab.flatten()
        lab = buf[1:].view(n, *shape)
    wt = weights(c).to(DEV) if wtd else None
    x, leaf, blk = features(form, 32, n, shape)
    fc = head_conv(32, c)
    if not ops.head_seg_supported(x, 32, c, lab):
        raise RuntimeError("head_seg does not take this case")
    lg, loss = ops.head_seg(x, fc.weight, fc.bias, fc._packed(), lab, wt, 1e-5, sig, ign, cl, wl)
    return finish({"loss": digest(loss), "logits": digest(lg)}, loss, leaf, blk, fc, mode)


def valu_cases():
    for cl in ("DICE", "CE", "DICE_CE"):
        for cin in (16, 32, 64):
            for c in (1, 2, 4):
                for u8 in (True, False):
                    yield f"valu {cl} cin={cin} C={c} labels={'u8' if u8 else 'i64'}", (cl, cin, c, u8, False)
        yield f"valu {cl} cin=32 C=4 labels=u8 fold", (cl, 32, 4, True, True)


def valu(mode, form, n, shape, cl, cin, c, u8, fold):
    lab = labels(f"lab{c}", c, n, *shape).to(DEV)
    lab = lab if u8 else lab.long()
    x, leaf, blk = features("fold" if fold else form, cin, n, shape)
    fc = head_conv(cin, c)
    wt = weights(c).to(DEV)
    if not getattr(ops, f"head_{cl.lower()}_supported")(x, cin, c, lab):
        raise RuntimeError(f"head_{cl.lower()} does not take this case")
    if cl == "DICE":
        lg, loss = ops.head_dice(x, fc.weight, fc.bias, fc._packed(), lab, wt, 1e-5, c == 1, None)
    elif cl == "CE":
        lg, loss = ops.head_ce(x, fc.weight, fc.bias, fc._packed(), lab, wt, -100)
    else:
        lg, loss = ops.head_dice_ce(x, fc.weight, fc.bias, fc._packed(), lab, wt, 1e-5)
    return finish({"loss": digest(loss), "logits": digest(lg)}, loss, leaf, blk, fc, mode)


LOSS_C = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)


def loss_cases():
    for fn in ("dice", "ce", "dice_ce", "metric"):
        cases = [(c, wtd, u8, False, None, None) for c in LOSS_C for wtd in (True, False) for u8 in (True, False)]
        if fn in ("dice", "metric"):
            cases += [(c, True, True, True, None, None) for c in (1, 4)] + [(9, True, True, False, 1, None)]
        if fn == "ce":
            cases += [(9, True, True, False, 3, None)]
        cases += [(5, True, True, False, None, var) for var in ("slice", "labvol", "oor")]
        for c, wtd, u8, sig, ign, var in cases:
            yield f"loss {fn} C={c} w={int(wtd)} labels={'u8' if u8 else 'i64'} sig={int(sig)} ign={ign} {var or 'plain'}", (fn, c, wtd, u8, sig, ign, var)


def loss(mode, n, shape, fn, c, wtd, u8, sig, ign, var):
    if var == "slice":  # channels 2 .. 2 + c of a wider tensor: stride_n != c * spatial
        leaf = (rnd(f"lgw{c}", n, c + 3, *shape) * 3.0).to(DEV).requires_grad_(True)
        z = leaf[:, 2:2 + c]
    else:
        leaf = z = (rnd(f"lg{c}", n, c, *shape) * 3.0).to(DEV).requires_grad_(True)
    if var == "labvol":  # the last channel of a uint8 label volume: sample stride != spatial
        lab = labels(f"vol{c}", c, n, 3, *shape).to(DEV)[:, -1]
    else:
        lab = labels(f"lab{c}", c, n, *shape).to(DEV)
    if var == "oor":
        lab = lab.clone()
        lab[0, 0, 0, 1] = c
    lab = lab if u8 else lab.long()
    wt = weights(c).to(DEV) if wtd else None
    if fn == "metric":
        out = {"dice": digest(ops.per_channel_dice(z, lab, wt, 1e-5, sig, ign))}
        torch.cuda.synchronize()
        return out
    if fn == "dice":
        val = ops.dice_loss(z, lab, wt, 1e-5, sig, ign)
    elif fn == "ce":
        val = ops.cross_entropy(z, lab, wt, -100 if ign is None else ign)
    else:
        val = ops.dice_ce_loss(z, lab, wt, 1e-5)
    (val * 3.0).backward()
    torch.cuda.synchronize()
    return {"loss": digest(val), "dlogits": digest(leaf.grad)}


DS_LEVELS = [((4, 4, 8), 1, 64, 1), ((4, 4, 8), 2, 128, 2), ((4, 4, 8), 3, 256, 4), ((6, 6, 6), 1, 64, 5), ((6, 6, 6), 1, 256, 8),
             ((6, 6, 6), 1, 128, 16), ((24, 24, 16), 1, 64, 16), ((4, 4, 8), 1, 256, 16), ((4, 4, 8), 2, 64, 8), ((6, 6, 6), 1, 128, 9)]


def ds_cases():
    for lev, s, cin, c in DS_LEVELS:
        cases = [(cl, sig, wtd, None) for cl, sig in (("DICE", False), ("DICE", True), ("CE", False), ("DICE_CE", False))
                 for wtd in (True, False)]
        if c == 9:
            cases += [("DICE", False, True, 2), ("CE", False, True, 3)]
        for cl, sig, wtd, ign in cases:
            yield f"ds lev={sh(lev)} shift={s} cin={cin} C={c} {cl} sig={int(sig)} w={int(wtd)} ign={ign}", (lev, s, cin, c, cl, sig, wtd, ign)


def ds(mode, with_pass, lev, s, cin, c, cl, sig, wtd, ign):
    n = 2
    lab = labels(f"dslab{c}", c, n, *(v << s for v in lev)).to(DEV)
    wt = weights(c).to(DEV) if wtd else None
    xg = ops.to_cl(rnd(f"x{cin}", n, cin, *lev).to(DEV).to(mednet_hip.config.act_dtype())).requires_grad_(True)
    fc = head_conv(cin, c)
    if not ops.ds_head_supported(xg, cin, c, lab, s):
        raise RuntimeError("ds_head does not take this case")
    xp, loss = ops.ds_head(xg, fc.weight, fc.bias, fc._packed(), lab, s, wt, 1e-5, sig, ign, cl)
    scale = 3.0 * 16384.0 if mode == "fp16" else 3.0  # (finish's)
    outs, grads = [loss], [torch.tensor(scale, device=DEV)]
    if with_pass:  # the gradient from the next decoder, in the storage type
        d_pass = ops.to_cl((rnd(f"p{cin}", n, cin, *lev) * (1e-3 * scale)).to(DEV).to(xg.dtype))
        outs, grads = [xp] + outs, [d_pass] + grads
    torch.autograd.backward(outs, grads)
    torch.cuda.synchronize()
    return {"loss": digest(loss), "dx": digest(xg.grad), "dw": digest(fc.weight.grad), "db": digest(fc.bias.grad)}


# per head: its cases, its function, its storage modes and its runs of a case (key, the function's arguments in front of the axes)
FORMS = [(f"{form}/{sh(shape)}", (form, n, shape)) for form in ("op", "block") for n, shape in SHAPES]
RUN = {"landmark": (landmark_cases, landmark, ("bf16", "fp16"), FORMS), "seg": (seg_cases, seg, ("bf16", "fp16"), FORMS),
       "valu": (valu_cases, valu, ("fp32", "bf16", "fp16"), FORMS),
       "ds": (ds_cases, ds, ("bf16", "fp16"), [("d_pass=0", (False,)), ("d_pass=1", (True,))]),
       "loss": (loss_cases, loss, ("fp32",), [(sh(shape), (n, shape)) for n, shape in SHAPES])}
for head in HEADS:
    cases, fn, modes, runs = RUN[head]
    for name, axes in cases():
        res = {}
        for mode in modes:
            for key, args in runs:
                with mednet_hip.precision(mode):
                    for k, v in fn(mode, *args, *axes).items():
                        res[f"{mode}/{key}/{k}"] = v
        line = {"case": name, "sha256": hashlib.sha256("".join(f"{k}={v};" for k, v in res.items()).encode()).hexdigest()}
        print(json.dumps({**line, **res} if FULL else line), flush=True)
        torch.cuda.empty_cache()
