"""Deep supervision restated from the oracle's own pieces (the reference has no deep supervision, so no golden fixture exists):

  * operator level (`head_ref`): the auxiliary 1x1x1 head on a level's stored 16-bit features, the nearest-neighbour label pick
    label[z << s][y << s][x << s], the oracle's DiceLoss / torch's cross-entropy in fp64, and the junction dz = d_pass + W^T dl with
    ONE rounding to the storage type;
  * network level (`network_ref`): the oracle's ResidualUNet3D with forward hooks on its `decoders`, nn.Conv3d 1x1x1 heads, strided
    label slices and the same losses, live on the CPU.

`head_ref(..., fault=...)` can commit each of the faults the checkers are there for -- an off-by-one pick, an averaged label, a
double-rounded join, a dropped d_pass -- and tests/test_ds_util.py shows on the CPU that each is rejected."""
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import ref_cpu as O

STORE = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp16x2": torch.float16, "fp32": torch.float32}
U_STORE = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp16x2": 2.0 ** -11}   # half an ulp, relative (a number in [1, 2))
FAULTS = ("pick_off_by_one", "averaged_label", "double_round", "drop_d_pass")


def default_weights(k):
    total = sum(2.0 ** -t for t in range(k + 1))
    return [2.0 ** -s / total for s in range(k + 1)]


def pick(labels, s, offset=0):
    """labels [..., D, H, W] -> the level's labels [..., D >> s, H >> s, W >> s]: element (z, y, x) = labels[z << s, y << s, x << s]
    (`offset`: the off-by-one fault)."""
    D, H, W = labels.shape[-3:]
    d, h, w = D >> s, H >> s, W >> s
    step = 1 << s
    return labels[..., offset:offset + (d << s):step, offset:offset + (h << s):step, offset:offset + (w << s):step]


def averaged(labels, s):
    """The averaged-label fault: the rounded mean of every 2^s cube instead of its first voxel."""
    D, H, W = labels.shape[-3:]
    d, h, w = D >> s, H >> s, W >> s
    crop = labels[..., :d << s, :h << s, :w << s].double()
    lead = crop.shape[:-3]
    return F.avg_pool3d(crop.reshape((-1, 1) + crop.shape[-3:]), 1 << s).round().reshape(lead + (d, h, w)).to(labels.dtype)


def class_loss(kind, logits, lab, wt=None, eps=1e-5, sigmoid=False, ignore=None):
    """The step's criterion from the oracle's pieces, in the precision of `logits`: "DICE" O.DiceLoss, "CE" F.cross_entropy,
    "DICE_CE" their sum with one class-weight vector."""
    wt = None if wt is None else wt.to(logits.dtype)
    dice = lambda: O.DiceLoss(epsilon=eps, weight=wt, ignore_index=ignore if kind == "DICE" else None, sigmoid_normalization=sigmoid)(logits, lab)
    ce = lambda: F.cross_entropy(logits, lab, weight=wt, ignore_index=-100 if (ignore is None or kind != "CE") else ignore)
    return dice() if kind == "DICE" else ce() if kind == "CE" else dice() + ce()


def head_ref(z, W, b, labels, s, kind, wt=None, d_pass=None, dloss=1.0, mode="bf16", eps=1e-5, sigmoid=False, ignore=None, fault=None):
    """fp64 on the CPU.  z [n, cin, d, h, w]: the STORED features (numbers of the storage type); W [ncls, cin], b [ncls] fp32; labels:
    the full-resolution [n, D, H, W] uint8 volume; d_pass [n, cin, d, h, w] (stored numbers) or None.
    -> loss, dz (= W^T dl, the head's own share), join (= d_pass + dz, unrounded), stored (= join rounded ONCE to the storage type),
    dW, db, and `norm` = |d_pass| + sum_k |W_k| |dl_k|, the sum of absolute terms of an element of the join."""
    assert fault in (None,) + FAULTS
    lab = averaged(labels, s) if fault == "averaged_label" else pick(labels, s, 1 if fault == "pick_off_by_one" else 0)
    lab = lab.long()
    z64 = z.double().clone().requires_grad_(True)
    W64 = W.double().reshape(W.shape[0], -1).clone().requires_grad_(True)
    b64 = b.double().clone().requires_grad_(True)
    logits = torch.einsum("kc,ncdhw->nkdhw", W64, z64) + b64[None, :, None, None, None]
    logits.retain_grad()
    loss = class_loss(kind, logits, lab, wt, eps, sigmoid, ignore)
    (loss * dloss).backward()
    dz = z64.grad
    dp = torch.zeros_like(dz) if (d_pass is None or fault == "drop_d_pass") else d_pass.double()
    join = dp + dz
    dt = STORE[mode]
    stored = (dz.to(dt).double() + dp).to(dt) if fault == "double_round" else join.to(dt)
    norm = dp.abs() + torch.einsum("kc,nkdhw->ncdhw", W64.detach().abs(), logits.grad.abs())
    return types.SimpleNamespace(loss=float(loss.detach()), dz=dz, join=join, stored=stored, dW=W64.grad, db=b64.grad, norm=norm, lab=lab,
                                 dl=logits.grad)


def half_ulp(x, mode):
    """Half the spacing of the storage type's numbers at |x| (fp64 tensor): 2^(e - 8) for bf16, 2^(e - 11) for fp16, e =
    floor(log2 |x|) held at the smallest normal exponent (-126 / -14: the subnormals' fixed spacing)."""
    _, ex = torch.frexp(x.abs())                                    # |x| = m 2^ex, m in [1/2, 1)
    e = (ex - 1).clamp(min=-126 if mode == "bf16" else -14).double()
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - (8 if mode == "bf16" else 11))


def check_join(got, ref, mode, eps_rel, what):
    """Every element of the stored junction gradient: |got - join64| <= half an ulp of the storage type at join64 + eps_rel * norm
    -- ONE rounding of the fp64 sum, plus the kernel's own arithmetic (eps_rel, in units of the element's sum of absolute terms).
    A second rounding (round(dz) first), a dropped d_pass or a wrong label leaves this bound.  -> the worst observed
    (|got - join64| - half ulp) / norm."""
    got = got.detach().double().cpu()
    assert got.shape == ref.join.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.join.shape)}"
    assert not bool(torch.isnan(got).any()), f"{what}: NaN (an element nobody wrote)"
    # (+ 2^-24 |join64|: torch converts fp64 to a 16-bit type through fp32, so the restatement's own "one rounding" sits that far
    #  from the fp64 sum where the sum is within 2^-24 of a tie)
    over = ((got - ref.join).abs() - half_ulp(ref.join, mode) - 2.0 ** -24 * ref.join.abs()).clamp(min=0)
    bad = over > eps_rel * ref.norm
    nbad = int(bad.sum())
    if nbad:
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {nbad} of {got.numel()} elements outside half an ulp + {eps_rel:.2e} * sum |terms|; first at {i}: "
                             f"got {got[i].item()!r} want {ref.join[i].item()!r} (sum |terms| {ref.norm[i].item():.3e})")
    live = ref.norm > 0
    return float((over[live] / ref.norm[live]).max()) if bool(live.any()) else 0.0


def check_loss(got, ref, bound, what):
    err = abs(float(got) - ref.loss)
    assert not np.isnan(float(got)) and err <= bound * max(1.0, abs(ref.loss)), f"{what}: |loss - loss64| = {err:.3e} > {bound:.1e} (got {float(got)!r} want {ref.loss!r})"
    return err


OUTSIDE = 255   # the class of every non-pick position of exact_pick_labels: no pick position holds it, and it is out of range


def exact_pick_labels(n, lev, s, ncls, seed=5):
    """A label volume N x 2 x D x H x W (the labels are its LAST channel; extents lev << s) in which the pick positions (multiples of
    2^s in every dim) hold every class 0 .. ncls-1 equally often over the batch, shuffled, and every other position OUTSIDE.  With
    p = 1 / ncls in every voxel the Dice sums are I_k = V / ncls^2 and D_k = 2 V / ncls (V = the batch's level voxels), every
    per-class Dice term is exactly 1 / ncls and the loss exactly 1 - 1 / ncls, in fp32 and in fp64 alike; a pick that strays by one
    voxel, or an averaged label, reads an out-of-range class."""
    V = n * int(np.prod(lev))
    assert V % ncls == 0, f"{V} level voxels do not split evenly over {ncls} classes"
    g = np.random.Generator(np.random.PCG64(seed + 17 * s + ncls))
    full = tuple(v << s for v in lev)
    vol = np.full((n, 2) + full, OUTSIDE, dtype=np.uint8)
    step = 1 << s
    vol[:, :, ::step, ::step, ::step] = g.permutation(np.repeat(np.arange(ncls), V // ncls)).astype(np.uint8).reshape((n, 1) + tuple(lev))
    return torch.from_numpy(vol)


def random_labels(n, full, ncls, seed=7):
    """N x 2 x D x H x W uint8, every voxel an in-range class."""
    g = np.random.Generator(np.random.PCG64(seed + ncls))
    return torch.from_numpy(g.integers(0, ncls, size=(n, 2) + tuple(full)).astype(np.uint8))


# ------------------------------------------------------------------------------------------------------------ network level
def oracle_with_heads(ctor, k, dtype=torch.float32):
    """The oracle's ResidualUNet3D plus `ds_heads` (nn.Conv3d 1x1x1 on f_maps[1 .. k]) under the HIP model's parameter names, so
    keyed_init_ gives both the same values."""
    ora = O.ResidualUNet3D(**ctor)
    f_maps = list(ctor["f_maps"])
    if k > 0:
        ora.ds_heads = nn.ModuleList(nn.Conv3d(f_maps[s], ctor["out_channels"], 1) for s in range(1, k + 1))
    return O.keyed_init_(ora).to(dtype)


def network_ref(ora, k, batch, kind, wt=None, weights=None):
    """loss = sum_s w_s L_s by forward hooks on the oracle's decoders (decoder i writes level len(decoders) - 1 - i); backward run.
    -> (loss, [L_0 .. L_k]) as Python floats; the gradients are in ora's parameters."""
    dtype = next(ora.parameters()).dtype
    weights = default_weights(k) if weights is None else list(weights)
    feats, hooks = {}, []
    top = len(ora.decoders) - 1
    for i, dec in enumerate(ora.decoders):
        if 1 <= top - i <= k:
            hooks.append(dec.register_forward_hook(lambda m, a, out, s=top - i: feats.__setitem__(s, out)))
    try:
        logits = ora(batch["data"].to(dtype))
    finally:
        for h in hooks:
            h.remove()
    lab = batch["label"][:, -1]
    wt = None if wt is None else torch.as_tensor(wt, dtype=dtype)
    levels = [class_loss(kind, logits, lab.long(), wt)]
    for s in range(1, k + 1):
        levels.append(class_loss(kind, ora.ds_heads[s - 1](feats[s]), pick(lab, s).contiguous().long(), wt))
    loss = sum(w * l for w, l in zip(weights, levels))
    loss.backward()
    return float(loss.detach()), [float(l.detach()) for l in levels]
