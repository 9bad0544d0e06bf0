"""Gradients when only a SUBSET of a node's inputs, or of a model's parameters, wants one (fine-tuning: frozen encoder, head only,
norm affines only, biases only) on the MI355X (-m gpu).  The rules are tests/partial_grad_util.py's (check_partial, check_step /
hold_steps); tests/test_partial_grad_util.py shows on the CPU that they reject the faults they are there for.

Node level: every hand-written autograd node, every non-empty subset S of its differentiable inputs, in the three storage modes.
requires_grad is set on S only; the gradients are compared with (a) the same node with every input wanted -- bit for bit: the same
kernel ran on the same operands (the weight-gradient side stream is off, so no split depends on stream placement) -- and (b) torch
autograd of the plain fp64 restatement of the operation under the same flags, at the tolerance of the existing operator test of
that node, named beside each case.  No tolerance is new here.

Trainer level: ResidualUNet3D([32, 64]) on 2 x 16^3, two eager SegmentationStep calls per scenario; fp32 mode against the CPU oracle
with the same flags and torch.optim.Adam over its trainable parameters (1e-3 per gradient slice, 2e-4 per loss: the bounds of
test_gpu_network.test_trainer_direct_gradients_and_fused_adam), bf16 mode bit for bit against the same scenario with everything
trainable.  profiles/partial_grads.md lists the routes that differ with the flags and the gradients that are computed unasked."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import block, ops
from mednet_hip.unet import components as HC
from mednet_hip.unet import loss as HL
from mednet_hip.unet import model as HM
from oracle import ref_cpu as O

import partial_grad_util as P
from gpu_util import DEV, DT, TOL, half_round, rnd

pytestmark = pytest.mark.gpu
MODES = ["fp32", "bf16", "fp16"]
HALF = ["bf16", "fp16"]
ACTS = {"none": (L.ACT_NONE, lambda u: u), "relu": (L.ACT_RELU, F.relu), "elu": (L.ACT_ELU, F.elu)}


@pytest.fixture(autouse=True)
def _side_stream_off():
    """Weight gradients stay on the main stream: a launch on the side stream asks for another workgroup count, and which stream a
    launch takes depends on which of its targets are trainer slices.  (The fp32 trainer scenarios switch it back on themselves.)"""
    old = ops.SIDE["enabled"]
    ops.SIDE["enabled"] = False
    try:
        yield
    finally:
        ops.SIDE["enabled"] = old


def _dev(t, mode, want, act=True):
    """A leaf on the device: activations in the mode's storage type, parameters in fp32."""
    t = t.to(DEV)
    if act:
        t = t.to(DT[mode])
    return t.requires_grad_(bool(want))


def _ref(t, want):
    return t.double().clone().requires_grad_(bool(want))


def _grads(leaves):
    return {k: (None if v.grad is None else v.grad.detach().clone()) for k, v in leaves.items()}


def _gscale(mode):
    """The heads STORE the feature gradient in the storage type: a Dice gradient of 1e-7 sits in fp16's subnormals, so the loss is
    scaled as train.LossScaler does (the existing head tests' factor)."""
    return 3.0 * 16384.0 if mode == "fp16" else 3.0


def _sweep(names, hip, ref, tol, what, sets=None, routes=None):
    """check_partial over `sets` (default: every non-empty subset of names): hip(wanted) / ref(wanted) -> {name: gradient or None}."""
    full = hip(tuple(names))
    lines = []
    for wanted in (sets or P.subsets(names)):
        seen = P.check_partial(hip(wanted), full, ref(wanted), wanted, tol, f"{what} wanted={'+'.join(wanted)}",
                               routes=routes(wanted) if routes else None)
        lines.append("+".join(wanted) + ": " + " ".join(f"{k} {v:.1e}" for k, v in seen.items()))
    print(f"[partial] {what}\n  " + "\n  ".join(lines))


# ------------------------------------------------------------------------------------------------- Conv3dFn
@pytest.mark.parametrize("mode", MODES)
def test_conv3d_k3_with_bias(mode):
    """Conv3dFn, k = 3, 32 -> 32 WITH bias, N = 2 (6, 8, 10); (b) F.conv3d at TOL[mode] for dx, dw and db
    (test_gpu_ops.test_conv3d_k3).  The subset {b} is the bias bug: db was computed only with the weight gradient."""
    n, c, shape = 2, 32, (6, 8, 10)
    x, w, cot = (half_round(t, mode) for t in (rnd("pgc3x", n, c, *shape), rnd("pgc3w", c, c, 3, 3, 3, scale=0.2), rnd("pgc3g", n, c, *shape)))
    b = rnd("pgc3b", c)

    def hip(wanted):
        with mednet_hip.precision(mode):
            lv = dict(x=_dev(x, mode, "x" in wanted), w=_dev(w, mode, "w" in wanted, False), b=_dev(b, mode, "b" in wanted, False))
            y = ops.conv3d(lv["x"], lv["w"], lv["b"], ops.pack_conv_weight(lv["w"], 3, False), 3)
            (y.float() * cot.to(DEV)).sum().backward()
        return _grads(lv)

    def ref(wanted):
        lv = dict(x=_ref(x, "x" in wanted), w=_ref(w, "w" in wanted), b=_ref(b, "b" in wanted))
        (F.conv3d(lv["x"], lv["w"], lv["b"], padding=1) * cot.double()).sum().backward()
        return _grads(lv)

    _sweep(("x", "w", "b"), hip, ref, TOL[mode], f"conv3d k3 32->32 bias {mode}")


def _head_ops(mode, tag, n, cin, cout, shape):
    x, w = half_round(rnd(tag + "x", n, cin, *shape), mode), half_round(rnd(tag + "w", cout, cin, 1, 1, 1, scale=0.3), mode)
    return x, w, rnd(tag + "b", cout), rnd(tag + "g", n, cout, *shape)


@pytest.mark.parametrize("mode", MODES)
def test_conv3d_k1_planar_head(mode):
    """Conv3dFn, the 1x1x1 head with planar fp32 logits, 32 -> 4 with bias, N = 2 (6, 8, 10); (b) F.conv3d at TOL[mode] for dx and dw,
    1e-4 for db (test_gpu_ops.test_conv1x1_head_planar_logits)."""
    x, w, b, cot = _head_ops(mode, "pgh1", 2, 32, 4, (6, 8, 10))

    def hip(wanted):
        with mednet_hip.precision(mode):
            lv = dict(x=_dev(x, mode, "x" in wanted), w=_dev(w, mode, "w" in wanted, False), b=_dev(b, mode, "b" in wanted, False))
            y = ops.conv3d(lv["x"], lv["w"], lv["b"], ops.pack_conv_weight(lv["w"], 1, False), 1, out_planar=True, out_dtype=torch.float32)
            (y * cot.to(DEV)).sum().backward()
        return _grads(lv)

    def ref(wanted):
        lv = dict(x=_ref(x, "x" in wanted), w=_ref(w, "w" in wanted), b=_ref(b, "b" in wanted))
        (F.conv3d(lv["x"], lv["w"], lv["b"]) * cot.double()).sum().backward()
        return _grads(lv)

    _sweep(("x", "w", "b"), hip, ref, dict(x=TOL[mode], w=TOL[mode], b=1e-4), f"conv3d k1 planar head 32->4 {mode}")


def _block_flags(blk, wanted_of):
    for k, p in blk.named_parameters():
        p.requires_grad = bool(wanted_of(k, p))


def test_conv3d_k1_planar_head_on_a_block_output_bf16():
    """Conv3dFn as the 1x1x1 head on an ExtResNetBlock output that carries `_mednet_gn3`, bf16: with the features wanted the head's
    data gradient takes the first pass of the block's GroupNorm-3 backward (mednet_head_dgrad_gn) and the block must TAKE those sums;
    without, nothing is offered.  The block's parameters are frozen; 'x' is the gradient that arrives at the block's INPUT, through
    the hand-off.  (b): the oracle's block and F.conv3d in fp64 for x at 4e-2 (the ExtResNetBlock bound of
    test_gpu_network.test_fused_groupnorm_partials_any_group_size); F.conv3d on the block output the device produced for w at TOL and b
    at 1e-4 (test_gpu_ops.test_conv1x1_head_planar_logits)."""
    mode, n, c, shape = "bf16", 2, 32, (6, 8, 10)
    x = half_round(rnd("pghbx", n, c, *shape), mode)
    w, b, cot = half_round(rnd("pghbw", 4, c, 1, 1, 1, scale=0.3), mode), rnd("pghbb", 4), rnd("pghbg", n, 4, *shape)
    feats = {}

    def hip(wanted):
        before = dict(ops.GN3_COUNT)
        with mednet_hip.precision(mode):
            blk = O.keyed_init_(HC.ExtResNetBlock(c, c, order="cge", num_groups=8)).to(DEV)
            _block_flags(blk, lambda k, p: False)
            lv = dict(x=_dev(x, mode, "x" in wanted), w=_dev(w, mode, "w" in wanted, False), b=_dev(b, mode, "b" in wanted, False))
            out = blk(lv["x"])
            assert getattr(out, "_mednet_gn3", None) is not None and out.requires_grad == ("x" in wanted)
            y = ops.conv3d(out, lv["w"], lv["b"], ops.pack_conv_weight(lv["w"], 1, False), 1, out_planar=True, out_dtype=torch.float32)
            (y * cot.to(DEV)).sum().backward()
            torch.cuda.synchronize()
        feats["out"] = out.detach().float().cpu()
        taken = ops.GN3_COUNT["taken"] - before["taken"]
        assert taken == int("x" in wanted), f"wanted={wanted}: the block took the head's GroupNorm-3 sums {taken} times"
        assert all(p.grad is None for p in blk.parameters())
        return _grads(lv)

    def ref(wanted):
        blk = O.keyed_init_(O.ExtResNetBlock(c, c, order="cge", num_groups=8)).double()
        _block_flags(blk, lambda k, p: False)
        lv = dict(x=_ref(x, "x" in wanted), w=_ref(w, "w" in wanted), b=_ref(b, "b" in wanted))
        (F.conv3d(blk(lv["x"]), lv["w"], lv["b"]) * cot.double()).sum().backward()
        got = _grads(lv)
        if "w" in wanted or "b" in wanted:   # the head's own gradients: from the features the device produced
            l2 = dict(w=_ref(w, "w" in wanted), b=_ref(b, "b" in wanted))
            (F.conv3d(feats["out"].double(), l2["w"], l2["b"]) * cot.double()).sum().backward()
            got.update(_grads(l2))
        return got

    _sweep(("x", "w", "b"), hip, ref, dict(x=4e-2, w=TOL[mode], b=1e-4), "conv3d k1 planar head on a block output bf16")


# ------------------------------------------------------------------------------------------------- ConvT3dFn
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,cin,cout,shape,skip", [(2, 64, 32, (3, 5, 4), True), (1, 16, 8, (4, 4, 4), False)])
def test_conv_transpose3d(mode, n, cin, cout, shape, skip):
    """ConvT3dFn, 64 -> 32 (3, 5, 4) with the fused skip add and 16 -> 8 (4, 4, 4) without; (b) F.conv_transpose3d (+ skip) at
    TOL[mode] for dx, dw and dskip, 1e-4 (fp32) / 1e-3 for db (test_gpu_ops.test_conv_transpose3d_with_skip).  The subsets with b
    and without w are the bias bug."""
    tag = f"pgct{cin}{cout}"
    oshape = tuple(2 * s for s in shape)
    x, w, sk, cot = (half_round(t, mode) for t in (rnd(tag + "x", n, cin, *shape), rnd(tag + "w", cin, cout, 3, 3, 3, scale=0.2),
                                                  rnd(tag + "s", n, cout, *oshape), rnd(tag + "g", n, cout, *oshape)))
    b = rnd(tag + "b", cout)
    names = ("x", "w", "b") + (("skip",) if skip else ())

    def hip(wanted):
        with mednet_hip.precision(mode):
            lv = dict(x=_dev(x, mode, "x" in wanted), w=_dev(w, mode, "w" in wanted, False), b=_dev(b, mode, "b" in wanted, False))
            if skip:
                lv["skip"] = _dev(sk, mode, "skip" in wanted)
            y = ops.conv_transpose3d(lv["x"], lv["w"], lv["b"], lv.get("skip"), ops.pack_conv_weight(lv["w"], 3, True))
            (y.float() * cot.to(DEV)).sum().backward()
        return _grads(lv)

    def ref(wanted):
        lv = dict(x=_ref(x, "x" in wanted), w=_ref(w, "w" in wanted), b=_ref(b, "b" in wanted))
        y = F.conv_transpose3d(lv["x"], lv["w"], lv["b"], stride=2, padding=1, output_padding=1)
        if skip:
            lv["skip"] = _ref(sk, "skip" in wanted)
            y = y + lv["skip"]
        (y * cot.double()).sum().backward()
        return _grads(lv)

    tol = dict(x=TOL[mode], w=TOL[mode], skip=TOL[mode], b=1e-4 if mode == "fp32" else 1e-3)
    _sweep(names, hip, ref, tol, f"conv_transpose3d {cin}->{cout} skip={skip} {mode}")


# ------------------------------------------------------------------------------------------------- ConvActFn
@pytest.mark.parametrize("mode", HALF)
def test_conv3d_act(mode):
    """ConvActFn (conv 3x3x3 -> ELU in one kernel), 32 -> 32, N = 2 (8, 8, 16); the node exists in the 16-bit storage modes only
    (ops.conv3d_act_supported).  (b) F.elu(F.conv3d) at 4e-2 for dx and dw: the bound of the conv -> activation layers in
    test_gpu_network.test_conv_act_orders_bf16_without_pooling (a bf16 bound; fp16 storage carries three more bits)."""
    n, c, shape = 2, 32, (8, 8, 16)
    x, w, cot = (half_round(t, mode) for t in (rnd("pgcax", n, c, *shape), rnd("pgcaw", c, c, 3, 3, 3, scale=0.1), rnd("pgcag", n, c, *shape)))

    def hip(wanted):
        with mednet_hip.precision(mode):
            lv = dict(x=_dev(x, mode, "x" in wanted), w=_dev(w, mode, "w" in wanted, False))
            assert ops.conv3d_act_supported(lv["x"], c, c)
            z, _ = ops.conv3d_act(lv["x"], lv["w"], ops.pack_conv_weight(lv["w"], 3, False), L.ACT_ELU)
            (z.float() * cot.to(DEV)).sum().backward()
        return _grads(lv)

    def ref(wanted):
        lv = dict(x=_ref(x, "x" in wanted), w=_ref(w, "w" in wanted))
        (F.elu(F.conv3d(lv["x"], lv["w"], None, padding=1)) * cot.double()).sum().backward()
        return _grads(lv)

    _sweep(("x", "w"), hip, ref, 4e-2, f"conv3d+act 32->32 {mode}")


# ------------------------------------------------------------------------------------------------- GroupNormActFn / BatchNormActFn
def _norm_ops(tag, mode, n, c, shape):
    x, r, cot = (half_round(t, mode) for t in (rnd(tag + "x", n, c, *shape, scale=2.0) + 0.5, rnd(tag + "r", n, c, *shape), rnd(tag + "g", n, c, *shape)))
    return x, r, cot, rnd(tag + "ga", c) * 0.3 + 1.0, rnd(tag + "be", c) * 0.3


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("act", ["relu", "elu"])
@pytest.mark.parametrize("res", [False, True])
def test_group_norm_act(mode, act, res):
    """GroupNormActFn, C = 32, 8 groups, N = 2 (5, 6, 7), with and without the residual, ReLU and ELU; (b) act(F.group_norm + residual)
    at TOL[mode] for dx, dgamma, dbeta and dres (test_gpu_ops.test_group_norm_act)."""
    n, c, groups, shape = 2, 32, 8, (5, 6, 7)
    x, r, cot, gamma, beta = _norm_ops(f"pggn{act}{res}", mode, n, c, shape)
    code, fn = ACTS[act]
    names = ("x", "gamma", "beta") + (("residual",) if res else ())

    def hip(wanted):
        with mednet_hip.precision(mode):
            lv = dict(x=_dev(x, mode, "x" in wanted), gamma=_dev(gamma, mode, "gamma" in wanted, False), beta=_dev(beta, mode, "beta" in wanted, False))
            if res:
                lv["residual"] = _dev(r, mode, "residual" in wanted)
            z = ops.group_norm_act(lv["x"], lv["gamma"], lv["beta"], groups, 1e-5, code, lv.get("residual"))
            (z.float() * cot.to(DEV)).sum().backward()
        return _grads(lv)

    def ref(wanted):
        lv = dict(x=_ref(x, "x" in wanted), gamma=_ref(gamma, "gamma" in wanted), beta=_ref(beta, "beta" in wanted))
        u = F.group_norm(lv["x"], groups, lv["gamma"], lv["beta"], 1e-5)
        if res:
            lv["residual"] = _ref(r, "residual" in wanted)
            u = u + lv["residual"]
        (fn(u) * cot.double()).sum().backward()
        return _grads(lv)

    _sweep(names, hip, ref, TOL[mode], f"group_norm_act {act} res={res} {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("act,res,training", [("elu", True, True), ("relu", False, True), ("relu", True, False), ("elu", False, False)])
def test_batch_norm_act(mode, act, res, training):
    """BatchNormActFn, the same shape, training (batch statistics, running statistics updated) and evaluation (running statistics);
    (b) act(F.batch_norm + residual) at TOL[mode] (test_gpu_batchnorm.test_batch_norm_act_against_fp64,
    test_eval_mode_uses_running_statistics)."""
    n, c, shape = 2, 32, (5, 6, 7)
    tag = f"pgbn{act}{res}{training}"
    x, r, cot, gamma, beta = _norm_ops(tag, mode, n, c, shape)
    rm0, rv0 = rnd(tag + "rm", c) * 0.2, rnd(tag + "rv", c).abs() + 0.5
    code, fn = ACTS[act]
    names = ("x", "gamma", "beta") + (("residual",) if res else ())

    def hip(wanted):
        with mednet_hip.precision(mode):
            lv = dict(x=_dev(x, mode, "x" in wanted), gamma=_dev(gamma, mode, "gamma" in wanted, False), beta=_dev(beta, mode, "beta" in wanted, False))
            if res:
                lv["residual"] = _dev(r, mode, "residual" in wanted)
            nbt = torch.zeros((), dtype=torch.int64, device=DEV)
            z = ops.batch_norm_act(lv["x"], lv["gamma"], lv["beta"], rm0.clone().to(DEV), rv0.clone().to(DEV), nbt, training, 0.1, 1e-5,
                                   code, lv.get("residual"))
            (z.float() * cot.to(DEV)).sum().backward()
        return _grads(lv)

    def ref(wanted):
        lv = dict(x=_ref(x, "x" in wanted), gamma=_ref(gamma, "gamma" in wanted), beta=_ref(beta, "beta" in wanted))
        u = F.batch_norm(lv["x"], rm0.double().clone(), rv0.double().clone(), lv["gamma"], lv["beta"], training, 0.1, 1e-5)
        if res:
            lv["residual"] = _ref(r, "residual" in wanted)
            u = u + lv["residual"]
        (fn(u) * cot.double()).sum().backward()
        return _grads(lv)

    _sweep(names, hip, ref, TOL[mode], f"batch_norm_act {act} res={res} training={training} {mode}")


# ------------------------------------------------------------------------------------------------- ResBlockFn
def _group_of(k, p):
    return "W" if p.dim() == 5 else ("gamma" if k.endswith("weight") else "beta")


BLOCK_SETS = P.subsets(("x", "W", "gamma", "beta")) + [("w2",), ("x", "w1", "w2", "gamma", "beta")]
# = x only, the parameters only (W + gamma + beta), gamma / beta only, ... and: w2 only; everything but w3


def _block_wanted(wanted, k, p):
    g = _group_of(k, p)
    if g == "W":
        return "W" in wanted or {"conv1.": "w1", "conv2.": "w2", "conv3.": "w3"}[k[:6]] in wanted
    return g in wanted


def _block_tol(mode, names_and_sizes):
    """fp32: 1e-4, every tensor (test_gpu_ops.test_split_bf16_kernels_keep_the_groupnorm_sums).  16-bit storage: 4e-2 for dx and the
    parameter gradients of 1024 elements and more -- the rule of test_gpu_network.test_fused_groupnorm_partials_any_group_size (a bf16
    bound; fp16 storage carries three more bits), which holds no smaller tensor per tensor (a 32-element sum does not average the
    storage rounding out): those have no (b) bound here either and are held by the None pattern and by bit equality with (a)."""
    if mode == "fp32":
        return {k: 1e-4 for k, _ in names_and_sizes}
    return {k: (4e-2 if (k == "x" or size >= 1024) else None) for k, size in names_and_sizes}


def _block_runs(mode, cin, tail=None, tag="pgrb", store=None):
    """-> (parameter names, hip, ref, [(name, elements)]) of ExtResNetBlock(cin, 32, 'cge') as ResBlockFn at N = 2 (8, 8, 16);
    `tail(out, device?)` -> the scalar to differentiate (default: the sum against a fixed cotangent); `store["out"]`: the block
    output the device produced."""
    n, c, shape = 2, 32, (8, 8, 16)
    x = rnd(f"{tag}x{cin}", n, cin, *shape)
    x = half_round(x, mode) if cin > 1 else x    # (the one-channel network input stays fp32, as the U-Net receives it)
    cot = rnd(f"{tag}g{cin}", n, c, *shape)
    pnames = [k for k, _ in O.ExtResNetBlock(cin, c, order="cge", num_groups=8).named_parameters()]

    def hip(wanted):
        with mednet_hip.precision(mode):
            blk = O.keyed_init_(HC.ExtResNetBlock(cin, c, order="cge", num_groups=8)).to(DEV)
            _block_flags(blk, functools.partial(_block_wanted, wanted))
            xg = _dev(x, mode, "x" in wanted, act=cin > 1)
            out = blk(xg)
            (tail(out, True) if tail else (out.float() * cot.to(DEV)).sum()).backward()
            torch.cuda.synchronize()
            if store is not None:
                store["out"] = out.detach().float().cpu()
        got = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in blk.named_parameters()}
        got["x"] = None if xg.grad is None else xg.grad.detach().clone()
        return got

    def ref(wanted):
        blk = O.keyed_init_(O.ExtResNetBlock(cin, c, order="cge", num_groups=8)).double()
        _block_flags(blk, functools.partial(_block_wanted, wanted))
        xr = _ref(x, "x" in wanted)
        out = blk(xr)
        (tail(out, False) if tail else (out * cot.double()).sum()).backward()
        got = {k: p.grad for k, p in blk.named_parameters()}
        got["x"] = xr.grad
        return got

    sizes = [(k, p.numel()) for k, p in O.ExtResNetBlock(cin, c, order="cge", num_groups=8).named_parameters()] + [("x", x.numel())]
    return pnames, hip, ref, sizes


def _expand(wanted, sizes, cin):
    """The group names of BLOCK_SETS -> the parameter names (and 'x') that want a gradient."""
    blk = O.ExtResNetBlock(cin, 32, order="cge", num_groups=8)
    return tuple(k for k, p in blk.named_parameters() if _block_wanted(wanted, k, p)) + (("x",) if "x" in wanted else ())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin", [32, 1])
def test_res_block(mode, cin):
    """ResBlockFn (ExtResNetBlock 'cge' as one node), 32 -> 32 and 1 -> 32 at N = 2 (8, 8, 16); the nine parameters grouped as conv
    weights W / gamma / beta, plus x: every subset of the groups, w2 alone, everything but w3.  (b): the oracle's ExtResNetBlock in
    fp64 (_block_tol).
    Route that depends on the flags: 1 -> 32 in the 16-bit modes WITHOUT a gradient of x runs the first layer's GroupNorm backward
    inside its weight gradient (block._c1_gn_applies: mednet_gn_bwd_coefficients + mednet_conv3d_wgrad_c1_gn), with it the stand-alone
    pass and the plain weight gradient.  The route's own test, test_gpu_network.
    test_first_layer_groupnorm_backward_inside_its_weight_gradient, holds the two forms to BIT equality in every parameter gradient, so
    no exception from (a) is taken here: w1, gamma1 and beta1 of the fused route must equal the all-wanted run's bits."""
    pnames, hip, ref, sizes = _block_runs(mode, cin)
    tol = _block_tol(mode, sizes)
    full = hip(("x", "W", "gamma", "beta"))
    before = block.C1GN_COUNT["fused"]
    lines = []
    for wanted in BLOCK_SETS:
        names = _expand(wanted, sizes, cin)
        c1 = block.C1GN_COUNT["fused"]
        got = hip(wanted)
        fused_c1 = block.C1GN_COUNT["fused"] - c1
        assert fused_c1 == int(cin == 1 and mode != "fp32" and "x" not in wanted), (wanted, fused_c1)
        seen = P.check_partial(got, full, ref(wanted), names, tol, f"res_block {cin}->32 {mode} wanted={'+'.join(wanted)}")
        lines.append("+".join(wanted) + ": worst " + (f"{max(seen.values()):.1e}" if seen else "-"))
    print(f"[partial] res_block {cin}->32 {mode} (first-layer fused route ran {block.C1GN_COUNT['fused'] - before} times)\n  " + "\n  ".join(lines))


# ------------------------------------------------------------------------------------------------- SkipPool2Fn + producing block
def _max_pool_at(out64, dev_out):
    """2x2x2 max pooling of out64 that picks, in every window, the element F.max_pool3d picks in `dev_out` (first maximum: the
    kernel's rule, test_gpu_ops.test_max_pool_ties_route_to_first_maximum)."""
    _, idx = F.max_pool3d(dev_out, 2, return_indices=True)
    return out64.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pool", ["max", "avg"])
def test_skip_pool2_behind_its_producing_block(mode, pool):
    """SkipPool2Fn on the output of an ExtResNetBlock(32, 32) with sole_consumer=True (the U-Net's call), N = 2 (8, 8, 16): only the skip
    consumer, only the pooling consumer, both wanting a gradient.  The three are different operands, not different flags, so (a) does
    not apply between them.  Routes: skip only -- the node passes dskip on and the block runs its stand-alone GroupNorm-3 pass; pool
    only / both -- mednet_pool2_bwd_gn without / with dskip, the gradient of the block output never written and rebuilt by
    mednet_gn_act_bwd_fused_res_pool.  In place of (a) each is held bit for bit to the same consumers with the gradient MATERIALISED
    (ops.LAZY_POOL off), the rule of test_gpu_network.test_the_unwritten_gradient_of_an_encoder_level_changes_nothing; (b): the
    oracle's block and the pooling in fp64 (_block_tol); the max pooling takes its arg-max from the block output the DEVICE stored (in
    16-bit storage two of eight neighbours round to one number often enough that the fp64 block would route a few percent of the
    gradient elsewhere: a property of the storage type, equalised as test_gpu_network._ForcedReLU equalises ReLU masks)."""
    n, c, shape = 2, 32, (8, 8, 16)
    c1, c2 = rnd("pgspc1", n, c, *shape), rnd("pgspc2", n, c, *(s // 2 for s in shape))
    pm = L.POOL_MAX if pool == "max" else L.POOL_AVG
    all_names = ("x", "W", "gamma", "beta")
    for consumers in (("skip",), ("pool",), ("skip", "pool")):
        def tail(out, device):
            if device:
                skip, pooled = ops.skip_pool2(out, pm, sole_consumer=True)
                terms = ([(skip.float() * c1.to(DEV)).sum()] if "skip" in consumers else []) + \
                        ([(pooled.float() * c2.to(DEV)).sum()] if "pool" in consumers else [])
            else:
                pooled = _max_pool_at(out, store["out"]) if pool == "max" else F.avg_pool3d(out, 2)
                terms = ([(out * c1.double()).sum()] if "skip" in consumers else []) + \
                        ([(pooled * c2.double()).sum()] if "pool" in consumers else [])
            return sum(terms)

        store = {}
        pnames, hip, ref, sizes = _block_runs(mode, c, tail=tail, tag="pgsp", store=store)
        tol = _block_tol(mode, sizes)
        names = _expand(all_names, sizes, c)
        old = ops.LAZY_POOL
        try:
            ops.LAZY_POOL = False
            full = hip(all_names)
        finally:
            ops.LAZY_POOL = old
        seen = P.check_partial(hip(all_names), full, ref(all_names), names, tol, f"skip_pool2 {pool} {mode} consumers={'+'.join(consumers)}")
        print(f"[partial] skip_pool2 {pool} {mode} consumers={'+'.join(consumers)}: worst {max(seen.values()):.1e}")


# ------------------------------------------------------------------------------------------------- UpCatFn
@pytest.mark.parametrize("mode", MODES)
def test_upsample_concat(mode):
    """UpCatFn, 32 + 64 channels at (8, 12, 16) / (4, 6, 8), N = 2 (the encoder part of the gradient leaves as a VIEW of the incoming
    one); (b) cat(enc, interpolate(x)) at 1e-6 for denc, 1e-6 (fp32) / 1e-2 for dx (test_gpu_ops.test_upsample_concat)."""
    n, ce, cx, es, xs = 2, 32, 64, (8, 12, 16), (4, 6, 8)
    e, x, cot = (half_round(t, mode) for t in (rnd("pguce", n, ce, *es), rnd("pgucx", n, cx, *xs), rnd("pgucg", n, ce + cx, *es)))

    def hip(wanted):
        with mednet_hip.precision(mode):
            lv = dict(enc=_dev(e, mode, "enc" in wanted), x=_dev(x, mode, "x" in wanted))
            y = ops.upsample_concat(lv["enc"], lv["x"])
            (y.float() * cot.to(DEV)).sum().backward()
        return _grads(lv)

    def ref(wanted):
        lv = dict(enc=_ref(e, "enc" in wanted), x=_ref(x, "x" in wanted))
        (torch.cat((lv["enc"], F.interpolate(lv["x"], size=es, mode="nearest")), dim=1) * cot.double()).sum().backward()
        return _grads(lv)

    _sweep(("enc", "x"), hip, ref, dict(enc=1e-6, x=1e-6 if mode == "fp32" else 1e-2), f"upsample_concat {mode}")


# ------------------------------------------------------------------------------------------------- the fused heads
def _head_case(mode, tag, cout, nh=0):
    n, cin, shape = 2, 32, (8, 8, 16)
    x = half_round(rnd(tag + "x", n, cin, *shape), mode)
    w, b = rnd(tag + "w", cout, cin, 1, 1, 1, scale=0.3), rnd(tag + "b", cout)
    g = np.random.Generator(np.random.PCG64(91 + cout))
    hm = torch.from_numpy(g.integers(0, 256, size=(n, nh) + shape).astype(np.uint8))
    lab = torch.from_numpy(g.integers(0, cout - nh, size=(n, 1) + shape).astype(np.uint8))
    return x, w, b, torch.cat([hm, lab], dim=1)


def _head_sweep(mode, what, x, w, b, device_loss, cpu_loss):
    """{features, w, b} of a fused head + loss node; (b) F.conv3d + the CPU loss at max(TOL[mode], 1e-4) for all three -- the bound
    every fused head's operator test uses against ATen (test_gpu_ops.test_fused_head_dice_against_the_unfused_launches,
    test_gpu_ce_heads.test_fused_head_ce_against_the_unfused_launches, test_gpu_seg_heads._compare)."""
    gs = _gscale(mode)
    cout, cin = w.shape[:2]

    def hip(wanted):
        with mednet_hip.precision(mode):
            lv = dict(features=ops.to_cl(x.to(DEV).to(DT[mode])).requires_grad_("features" in wanted),
                      w=_dev(w, mode, "w" in wanted, False), b=_dev(b, mode, "b" in wanted, False))
            loss = device_loss(lv["features"], lv["w"], lv["b"], ops.pack_conv_weight(lv["w"], 1, False))
            (loss * gs).backward()
            torch.cuda.synchronize()
        return _grads(lv)

    def ref(wanted):
        lv = dict(features=_ref(x, "features" in wanted), w=_ref(w, "w" in wanted), b=_ref(b, "b" in wanted))
        (cpu_loss(F.conv3d(lv["features"], lv["w"], lv["b"])) * gs).backward()
        return _grads(lv)

    _sweep(("features", "w", "b"), hip, ref, max(TOL[mode], 1e-4), what)


WT4 = [0.05, 1.0, 0.7, 1.3]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["dice", "ce", "dice_ce"])
def test_small_fused_heads(mode, kind):
    """HeadDiceFn, HeadCEFn, HeadDiceCEFn: 32 -> 4 at N = 2 (8, 8, 16), weighted, uint8 labels where they lie."""
    x, w, b, vol = _head_case(mode, "pghd" + kind, 4)
    wt = torch.tensor(WT4)
    lab = vol[:, -1].long()

    def device_loss(f, wd, bd, pk):
        labd, wtd = vol.to(DEV)[:, -1], wt.to(DEV)
        if kind == "dice":
            assert ops.head_dice_supported(f, 32, 4, labd)
            return ops.head_dice(f, wd, bd, pk, labd, wtd)[1]
        if kind == "ce":
            assert ops.head_ce_supported(f, 32, 4, labd)
            return ops.head_ce(f, wd, bd, pk, labd, wtd)[1]
        assert ops.head_dice_ce_supported(f, 32, 4, labd)
        return ops.head_dice_ce(f, wd, bd, pk, labd, wtd)[1]

    def cpu_loss(lg):
        w64 = wt.double()
        dice = O.DiceLoss(weight=w64)(lg, lab)
        ce = F.cross_entropy(lg, lab, weight=w64)
        return dice if kind == "dice" else (ce if kind == "ce" else dice + ce)

    _head_sweep(mode, f"head_{kind} 32->4 {mode}", x, w, b, device_loss, cpu_loss)


@pytest.mark.parametrize("mode", HALF)
@pytest.mark.parametrize("kind", ["DICE", "CE"])
def test_seg_head(mode, kind):
    """HeadSegFn: 8 classes on 32 features, N = 2 (8, 8, 16), the 16-bit storage modes (the node exists there only)."""
    x, w, b, vol = _head_case(mode, "pghs" + kind, 8)
    wt = torch.tensor([0.05] + [0.6 + 0.1 * k for k in range(1, 8)])
    lab = vol[:, -1].long()

    def device_loss(f, wd, bd, pk):
        labd = vol.to(DEV)[:, -1]
        assert ops.head_seg_supported(f, 32, 8, labd)
        return ops.head_seg(f, wd, bd, pk, labd, wt.to(DEV), class_loss=kind)[1]

    def cpu_loss(lg):
        return O.DiceLoss(weight=wt.double())(lg, lab) if kind == "DICE" else F.cross_entropy(lg, lab, weight=wt.double())

    _head_sweep(mode, f"head_seg {kind} 32->8 {mode}", x, w, b, device_loss, cpu_loss)


@pytest.mark.parametrize("mode", HALF)
def test_landmark_head(mode):
    """HeadLandmarkFn: 5 heat maps + 2 classes on 32 features, L2 regression, N = 2 (8, 8, 16), the 16-bit storage modes."""
    nh, ncls = 5, 2
    x, w, b, vol = _head_case(mode, "pghl", nh + ncls, nh)
    cw, rw = torch.tensor([0.05, 1.0]), [0.015 + 0.003 * i for i in range(nh)]
    lab, hm = vol[:, -1].long(), vol[:, :nh]

    def device_loss(f, wd, bd, pk):
        vd = vol.to(DEV)
        assert ops.head_landmark_supported(f, 32, nh, ncls, vd[:, :nh], vd[:, nh])
        cl, rg = ops.head_landmark(f, wd, bd, pk, vd[:, :nh], vd[:, nh], cw.to(DEV), rw, "L2")
        return cl + rg

    def cpu_loss(out):
        return O.DiceLoss(weight=cw.double())(out[:, nh:], lab) + sum(rw[c] * F.mse_loss(out[:, c], hm[:, c].double()) for c in range(nh))

    _head_sweep(mode, f"head_landmark 5+2 {mode}", x, w, b, device_loss, cpu_loss)


# ================================================================================================= trainer level
CTOR = dict(in_channels=1, out_channels=2, final_sigmoid=False, f_maps=[32, 64])
W2 = [0.05, 1.0]
GRAD_TOL, LOSS_TOL = 1e-3, 2e-4     # test_gpu_network.test_trainer_direct_gradients_and_fused_adam


def _conv_bias(k, p):
    return k.endswith("upsample.bias") or k == "final_conv.bias"


# name -> is the parameter FROZEN
SCENARIOS = {
    "encoder frozen": lambda k, p: k.startswith("encoders."),
    "head only": lambda k, p: not k.startswith("final_conv."),
    "decoder frozen": lambda k, p: k.startswith("decoders."),                      # the gradient flows THROUGH frozen layers
    "level-1 encoder block frozen": lambda k, p: k.startswith("encoders.1."),      # the lazy pooled gradient into a block with no trainable parameter
    "conv weights frozen": lambda k, p: p.dim() == 5,                              # gamma, beta and the biases train
    "biases only": lambda k, p: not _conv_bias(k, p),                              # ConvTranspose3d's and the head's bias: the bias bug
}
NOTHING = lambda k, p: False


@functools.lru_cache(maxsize=None)
def _batch():
    return O.synthetic_batch(2, 1, (16, 16, 16), 2, 0, seed=77)


def _freeze(net, frozen):
    for k, p in net.named_parameters():
        p.requires_grad = not frozen(k, p)
    return net


@functools.lru_cache(maxsize=None)
def _oracle_steps(scenario, cls="ResidualUNet3D", steps=2):
    """The CPU oracle with the scenario's flags and torch.optim.Adam over its trainable parameters -> (losses, gradients of step 1)."""
    ctor = CTOR if cls == "ResidualUNet3D" else UNET_CTOR
    ora = _freeze(O.keyed_init_(getattr(O, cls)(**ctor)), ENC if scenario == "unet encoder frozen" else SCENARIOS[scenario])
    opt = torch.optim.Adam([p for p in ora.parameters() if p.requires_grad], lr=1e-3)
    losses, first = [], None
    for i in range(steps):
        opt.zero_grad()
        loss = O.seg_training_step(ora, O.DiceLoss(weight=torch.tensor(W2)), _batch())
        loss.backward()
        if i == 0:
            first = {k: p.grad.clone() for k, p in ora.named_parameters() if p.grad is not None}
        opt.step()
        losses.append(float(loss.detach()))
    return losses, first


def _seg_start(frozen, cls=HM.ResidualUNet3D, ctor=CTOR, side=False, graph=None):
    from mednet_hip.train import SegmentationStep

    def start():
        net = _freeze(O.keyed_init_(cls(**ctor)).to(DEV), frozen)
        step = SegmentationStep(net, loss_weight=W2, lr=1e-3, graph=graph)   # (switches the side stream on)
        ops.SIDE["enabled"] = bool(side)
        gb = {k: v.to(DEV) for k, v in _batch().items()}

        def call(i):
            loss = float(step(gb))
            torch.cuda.synchronize()
            return loss

        def close():
            step.flat.release()
            ops.SIDE["enabled"] = False
        return net, step.flat, call, close
    return start


@functools.lru_cache(maxsize=None)
def _all_trainable_bf16(cls="ResidualUNet3D"):
    """Step 1 of the all-trainable run in bf16 mode, side stream off -> {name: gradient slice}: computed once, shared, never changed."""
    ctor = CTOR if cls == "ResidualUNet3D" else UNET_CTOR
    with mednet_hip.precision("bf16"):
        _, first, _ = P.hold_steps(_seg_start(NOTHING, getattr(HM, cls), ctor), f"{cls}, everything trainable, bf16", steps=1)
    return first


@pytest.mark.parametrize("scenario", list(SCENARIOS))
def test_partly_frozen_segmentation_step_fp32_against_the_oracle(scenario):
    """fp32 mode, the weight-gradient side stream ON as the step runs it: after step 1 every trainable slice within 1e-3 of the oracle's
    gradient, both losses within 2e-4; after each step the trainer rule (check_step), and the refilled gradient buffer ends step 2 with
    the clean run's bits."""
    want_losses, ref = _oracle_steps(scenario)
    with mednet_hip.precision("fp32"):
        losses, first, seen = P.hold_steps(_seg_start(SCENARIOS[scenario], side=True), f"{scenario}, fp32", ref=ref, tol=GRAD_TOL)
    print(f"[partial] {scenario} fp32: losses {losses} (oracle {want_losses}); worst slice {max(seen.values()):.2e} of {len(seen)}")
    for i, (a, b) in enumerate(zip(losses, want_losses)):
        assert abs(a - b) <= LOSS_TOL, f"{scenario}: loss of step {i + 1} {a!r} against the oracle's {b!r}"


@pytest.mark.parametrize("scenario", list(SCENARIOS))
def test_partly_frozen_segmentation_step_bf16_against_everything_trainable(scenario):
    """bf16 mode, side stream off: after step 1 every trainable slice bit-identical to the all-trainable run's slice (the same
    kernels ran on the same operands: no route differs with these flags, so no exception is taken), plus the trainer rule after each
    step and the refill."""
    full = _all_trainable_bf16()
    with mednet_hip.precision("bf16"):
        losses, first, _ = P.hold_steps(_seg_start(SCENARIOS[scenario]), f"{scenario}, bf16", full=full)
    assert all(np.isfinite(losses)) and set(first) <= set(full)
    print(f"[partial] {scenario} bf16: {len(first)} slices bit-identical to the all-trainable run; losses {losses}")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_everything_frozen_and_the_input_wants_a_gradient(mode):
    """All parameters frozen, inputs.requires_grad_(True), through model(inputs) and the loss: no parameter receives a gradient;
    fp32: the input gradient within 1e-3 of the oracle's and the loss within 2e-4 (the trainer test's bounds); bf16: bit-identical to the
    input gradient of the network with everything trainable."""
    batch = _batch()
    y = batch["label"][:, -1].long()

    def run(frozen):
        net = _freeze(O.keyed_init_(HM.ResidualUNet3D(**CTOR)).to(DEV), frozen)
        xg = batch["data"].detach().float().to(DEV).requires_grad_(True)
        loss = HL.DiceLoss(weight=torch.tensor(W2, device=DEV)).to(DEV)(net(xg), y.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        return net, xg.grad.detach().clone(), float(loss.detach())

    with mednet_hip.precision(mode):
        net, dx, loss = run(lambda k, p: True)
        assert all(p.grad is None and not hasattr(p, "_mednet_grad") for p in net.parameters())
        assert bool(torch.isfinite(dx).all()) and float(dx.abs().max()) > 0
        if mode == "bf16":
            _, dx_all, loss_all = run(NOTHING)
            assert loss == loss_all and P.same_bits(dx, dx_all), "the input gradient depends on whether the parameters are frozen"
            return
    ora = _freeze(O.keyed_init_(O.ResidualUNet3D(**CTOR)), lambda k, p: True)
    xo = batch["data"].detach().float().clone().requires_grad_(True)   # (a leaf of its own: the batch is shared between the tests)
    lo = O.DiceLoss(weight=torch.tensor(W2))(ora(xo), y)
    lo.backward()
    lo = lo.detach()
    r = P.rel_l2(dx, xo.grad)
    print(f"[partial] everything frozen, fp32: input gradient rel-L2 {r:.2e}, loss {loss!r} (oracle {float(lo)!r})")
    assert r <= GRAD_TOL and abs(loss - float(lo)) <= LOSS_TOL


UNET_CTOR = dict(in_channels=1, out_channels=2, final_sigmoid=False, f_maps=[32, 64], layer_order="gcr")
ENC = lambda k, p: k.startswith("encoders.")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_unet3d_gcr_with_the_encoder_frozen(mode):
    """UNet3D ('gcr': GroupNorm -> conv -> ReLU, concatenation joining) with the encoder frozen: trainable blocks behind frozen ones,
    through UpCatFn, the GroupNorm / activation-mask hand-offs and the plain pooling.  fp32 against the oracle, bf16 bit for bit against
    everything trainable."""
    if mode == "fp32":
        want_losses, ref = _oracle_steps("unet encoder frozen", "UNet3D")
        with mednet_hip.precision("fp32"):
            losses, _, seen = P.hold_steps(_seg_start(ENC, HM.UNet3D, UNET_CTOR, side=True), "UNet3D encoder frozen, fp32", ref=ref, tol=GRAD_TOL)
        print(f"[partial] UNet3D encoder frozen fp32: losses {losses} (oracle {want_losses}); worst slice {max(seen.values()):.2e}")
        assert all(abs(a - b) <= LOSS_TOL for a, b in zip(losses, want_losses)), (losses, want_losses)
    else:
        full = _all_trainable_bf16("UNet3D")
        with mednet_hip.precision("bf16"):
            P.hold_steps(_seg_start(ENC, HM.UNet3D, UNET_CTOR), "UNet3D encoder frozen, bf16", full=full)


LM_CTOR = dict(in_channels=1, out_channels=7, final_sigmoid=False, f_maps=[32, 64])
LM_REGW = [0.015 + 0.003 * i for i in range(5)]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_landmark_step_with_everything_but_the_head_frozen(mode):
    """LandmarkStep (5 heat maps + 2 classes), everything but final_conv frozen: the fused landmark head (bf16) / the channel split and
    the two losses (fp32) with no gradient wanted behind them.  fp32: the head's two slices within 1e-3 of the oracle's gradient and the
    total loss within 2e-4 relative (test_gpu_network.test_landmark_step_matches_oracle); bf16: bit-identical to everything trainable."""
    from mednet_hip.train import LandmarkStep
    batch = O.synthetic_batch(2, 1, (16, 16, 16), 2, 5, seed=4321)
    head_only = SCENARIOS["head only"]

    def starter(frozen, side):
        def start():
            net = _freeze(O.keyed_init_(HM.ResidualUNet3D(**LM_CTOR)).to(DEV), frozen)
            step = LandmarkStep(net, class_weight=W2, regression_weight=LM_REGW, regression="L2", lr=1e-3)
            ops.SIDE["enabled"] = side
            gb = {k: v.to(DEV) for k, v in batch.items()}

            def call(i):
                loss = float(step(gb)[0])
                torch.cuda.synchronize()
                return loss

            def close():
                step.flat.release()
                ops.SIDE["enabled"] = False
            return net, step.flat, call, close
        return start

    if mode == "bf16":
        with mednet_hip.precision("bf16"):
            _, full, _ = P.hold_steps(starter(NOTHING, False), "landmark, everything trainable, bf16", steps=1)
            _, first, _ = P.hold_steps(starter(head_only, False), "landmark head only, bf16", full=full)
        assert set(first) == {"final_conv.weight", "final_conv.bias"}
        return
    ora = _freeze(O.keyed_init_(O.ResidualUNet3D(**LM_CTOR)), head_only)
    opt = torch.optim.Adam([p for p in ora.parameters() if p.requires_grad], lr=1e-3)
    want, ref = [], None
    for i in range(2):
        opt.zero_grad()
        tot = O.ldmk_training_step(ora, O.DiceLoss(weight=torch.tensor(W2)), nn.MSELoss(), LM_REGW, batch)[0]
        tot.backward()
        if i == 0:
            ref = {k: p.grad.clone() for k, p in ora.named_parameters() if p.grad is not None}
        opt.step()
        want.append(float(tot.detach()))
    with mednet_hip.precision("fp32"):
        losses, _, seen = P.hold_steps(starter(head_only, True), "landmark head only, fp32", ref=ref, tol=GRAD_TOL)
    print(f"[partial] landmark head only fp32: losses {losses} (oracle {want}); slices {seen}")
    assert all(abs(a - b) <= LOSS_TOL * abs(b) for a, b in zip(losses, want)), (losses, want)


def test_encoder_frozen_bf16_graph_replay_equals_eager():
    """The bf16 encoder-frozen scenario with graph=True: two eager warm-up calls, capture, and the replayed step 3 equals eager step 3
    bit for bit in loss, gradient buffer and parameters (side stream on, as test_gpu_network.test_graph_replay_matches_eager_steps)."""
    res = {}
    for graph in (False, True):
        with mednet_hip.precision("bf16"):
            net, flat, call, close = _seg_start(SCENARIOS["encoder frozen"], side=True, graph=graph)()
            try:
                probe = P.StepProbe(net, flat)
                losses = [call(i) for i in range(3)]
                P.check_step(probe, f"encoder frozen, bf16, graph={graph}, step 3")
                res[graph] = (losses, flat.grad.clone(), flat.flat.clone())
            finally:
                close()
    assert res[True][0] == res[False][0], (res[True][0], res[False][0])
    assert P.same_bits(res[True][1], res[False][1]) and P.same_bits(res[True][2], res[False][2])


@pytest.mark.parametrize("direction", ["frozen after construction", "unfrozen after construction"])
def test_requires_grad_changed_after_the_step_was_built_is_an_error(direction):
    """Freezing later would leave the kernels writing and Adam moving the "frozen" parameter; thawing later would never train it.  The
    step refuses the call and names the first changed parameter."""
    with mednet_hip.precision("fp32"):
        net, flat, call, close = _seg_start(SCENARIOS["encoder frozen"])()
        try:
            call(0)
            name = "decoders.0.upsample.bias" if direction.startswith("frozen") else "encoders.1.basic_module.conv2.conv.weight"
            p = dict(net.named_parameters())[name]
            p.requires_grad = not p.requires_grad
            before = flat.flat.clone()
            with pytest.raises(RuntimeError, match=f"'{name}' changed from .* rebuild the step"):
                call(1)
            torch.cuda.synchronize()
            assert P.same_bits(before, flat.flat), "the refused call moved the parameters"
        finally:
            close()
