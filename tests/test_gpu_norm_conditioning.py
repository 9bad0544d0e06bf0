"""Conditioning tests of the normalisation kernels (csrc/norm_act.hip): data with a large mean / std ratio R, a constant group, a
near-constant group and a negated sample, against the fp64 two-pass reference of tests/norm_cond_util.py, element by element,
inside bounds that are linear in R (derived there, and shown there to hold for ATen's own fp32 kernels).  A variance taken as
sum x^2 / N - mean^2 from fp32 sums has an error quadratic in R and leaves these bounds from R = 16 on.

Through the C ABI: mednet_gn_stats, mednet_gn_act_fwd (ReLU), mednet_gn_act_bwd (ReLU from the stored z), mednet_bn_stats (with
running statistics), mednet_bn_act_bwd; one case per storage type through hnn.GroupNorm / hnn.BatchNorm3d.  Compared: stats (mean,
rstd), coef, z, dx, dgamma, dbeta, running_mean, running_var -- every element; outputs and workspaces start as NaN.  Lines
`[cond] ...` give the worst error / bound per quantity (pytest -s / -rP); profiles/norm_conditioning.md records them.

A second set covers partial rows produced elsewhere -- a convolution's epilogue, mednet_upcat_fwd_stats, rows handed to
mednet_gn_finalize -- which keep the {sum x, sum x^2} form: output mean / std ~ 16, at the rel-L2 tolerance of test_group_norm_act.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import nn as hnn
from mednet_hip import ops

import norm_cond_util as C
from gpu_util import CL, DEV, DT, TOL, rel

pytestmark = pytest.mark.gpu
ACT = {"relu": L.ACT_RELU, "none": L.ACT_NONE}
GN_PARAMS = [(k, "fp32", R) for k in ("small", "ragged", "first") for R in C.RATIOS["fp32"]] + \
            [("wide", m, R) for m in ("fp16", "bf16") for R in C.RATIOS[m]]
BN_PARAMS = [(m, R) for m in ("fp32", "fp16", "bf16") for R in C.RATIOS[m]]
MODULE_R = {"fp32": 4096, "fp16": 64, "bf16": 16}
_CACHE = {}


def prepared(key, R, mode, act="relu"):
    """The case, its reference and its bounds: computed once, shared, never written to."""
    k = (key, R, mode, act)
    if k not in _CACHE:
        if key == "bn":
            n, c, shape = C.BN_SHAPE
            case = C.make_case("bn", n, c, None, shape, R, mode, batch=True)
            g = C._rng(f"cond:running:{R}:{mode}")
            rm0, rv0 = torch.from_numpy(g.uniform(-1, 1, c)).float().double(), torch.from_numpy(g.uniform(0.5, 2, c)).float().double()
            if act == "none":       # the module's fresh buffers
                rm0, rv0 = torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64)
            ref = C.reference(case, act, rm0=rm0, rv0=rv0)
            ref.rm0, ref.rv0 = rm0, rv0
        else:
            case = C.make_case(key, *C.GN_SHAPES[key], R, mode)
            ref = C.reference(case, act)
        _CACHE[k] = (case, ref, C.bounds(case, ref))
    return _CACHE[k]


def vol(t, mode):
    return t.to(DT[mode]).to(DEV).contiguous(memory_format=CL)


def f32(t):
    return t.to(torch.float32).contiguous().to(DEV)


def nan_f32(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


def nan_vol(case):
    return torch.full((case.n, case.c, *case.shape), float("nan"), device=DEV).to(DT[case.mode]).contiguous(memory_format=CL)


def workspace(case):
    nbytes = L.lib().mednet_gn_ws_bytes(case.n, case.c, case.spatial)
    ws = nan_f32((nbytes + 3) // 4)
    return ws, ws.numel() * 4


def ok(rc, what):
    assert rc == 0, f"{what}: {rc} {L.lib().mednet_last_error().decode()}"
    torch.cuda.synchronize()


def conclude(what, ratios):
    print(f"[cond] {what}: " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{what}: error / bound above 1 for {bad} (all: {ratios})"


def stats_ratios(case, r, B, stats, coef, out):
    """stats[n][units][2] (BatchNorm: a row per sample, all equal), coef[n][c][2]."""
    rows = stats.reshape(case.n, -1, 2) if case.batch else stats.reshape(1, -1, 2)
    for i in range(rows.shape[0]):
        for j, name in enumerate(("mean", "rstd")):
            ref, bound = (r.mean, B.mean) if j == 0 else (r.rstd, B.rstd)
            C.worst_ratio(rows[i, :, j], ref, bound, name)
            for k, v in C.unit_ratios(case, rows[i, :, j], ref, bound).items():
                out[f"{name}[{k}]"] = max(out.get(f"{name}[{k}]", 0.0), v)
    out["coef_a"] = C.worst_ratio(coef[..., 0], r.coef_a.expand(case.n, -1), B.coef_a.expand(case.n, -1), "coef a")
    out["coef_b"] = C.worst_ratio(coef[..., 1], C.coef_b_reference(case, r, coef[..., 0]), B.coef_b.expand(case.n, -1), "coef b")


@pytest.mark.parametrize("key,mode,R", GN_PARAMS, ids=lambda v: str(v))
def test_groupnorm_on_offset_data(key, mode, R):
    case, r, B = prepared(key, R, mode)
    lib, dc = L.lib(), L.dt_of(DT[mode])
    xg, gam, bet = vol(case.x, mode), f32(case.gamma), f32(case.beta)
    stats, coef, z = nan_f32(case.n, case.groups, 2), nan_f32(case.n, case.c, 2), nan_vol(case)
    ws, wsb = workspace(case)
    ok(lib.mednet_gn_stats(xg.data_ptr(), gam.data_ptr(), bet.data_ptr(), stats.data_ptr(), coef.data_ptr(), case.n, case.spatial, case.c,
                           case.groups, case.eps, dc, ws.data_ptr(), wsb, L.stream()), "gn_stats")
    ok(lib.mednet_gn_act_fwd(xg.data_ptr(), coef.data_ptr(), None, z.data_ptr(), case.n, case.spatial, case.c, ACT["relu"], dc, dc, L.stream()),
       "gn_act_fwd")
    out = {}
    stats_ratios(case, r, B, stats, coef, out)
    out["z"] = C.worst_ratio(z, r.z, B.z, "z")
    dzg, zg = vol(case.dz, mode), vol(r.z_stored, mode)          # act' from the REFERENCE's stored z: the same mask on both sides
    dx, dgamma, dbeta = nan_vol(case), nan_f32(case.c), nan_f32(case.c)
    ws, wsb = workspace(case)
    ok(lib.mednet_gn_act_bwd(dzg.data_ptr(), None, xg.data_ptr(), zg.data_ptr(), coef.data_ptr(), stats.data_ptr(), gam.data_ptr(),
                             dx.data_ptr(), None, dgamma.data_ptr(), dbeta.data_ptr(), case.n, case.spatial, case.c, case.groups, ACT["relu"],
                             ACT["none"], dc, ws.data_ptr(), wsb, L.stream()), "gn_act_bwd")
    out["dx"] = C.worst_ratio(dx, r.dx, B.dx, "dx")
    out["dgamma"] = C.worst_ratio(dgamma, r.dgamma, B.dgamma, "dgamma")
    out["dbeta"] = C.worst_ratio(dbeta, r.dbeta, B.dbeta, "dbeta")
    conclude(f"gn {key} {case.n}x{case.c}/{case.groups}x{case.shape} R={R} {mode}", out)


@pytest.mark.parametrize("mode,R", BN_PARAMS, ids=lambda v: str(v))
def test_batchnorm_on_offset_data(mode, R):
    case, r, B = prepared("bn", R, mode)
    lib, dc = L.lib(), L.dt_of(DT[mode])
    xg, gam, bet = vol(case.x, mode), f32(case.gamma), f32(case.beta)
    stats, coef, z = nan_f32(case.n, case.c, 2), nan_f32(case.n, case.c, 2), nan_vol(case)
    rm, rv, nbt = f32(r.rm0), f32(r.rv0), torch.tensor([0], dtype=torch.int64, device=DEV)
    ws, wsb = workspace(case)
    ok(lib.mednet_bn_stats(xg.data_ptr(), gam.data_ptr(), bet.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), C.MOMENTUM,
                           stats.data_ptr(), coef.data_ptr(), case.n, case.spatial, case.c, case.eps, dc, ws.data_ptr(), wsb, L.stream()), "bn_stats")
    ok(lib.mednet_gn_act_fwd(xg.data_ptr(), coef.data_ptr(), None, z.data_ptr(), case.n, case.spatial, case.c, ACT["relu"], dc, dc, L.stream()),
       "gn_act_fwd")
    assert int(nbt.item()) == 1
    out = {}
    stats_ratios(case, r, B, stats, coef, out)
    out["running_mean"] = C.worst_ratio(rm, r.running_mean, B.running_mean, "running_mean")
    out["running_var"] = C.worst_ratio(rv, r.running_var, B.running_var, "running_var")
    out["z"] = C.worst_ratio(z, r.z, B.z, "z")
    dzg, zg = vol(case.dz, mode), vol(r.z_stored, mode)
    dx, dgamma, dbeta = nan_vol(case), nan_f32(case.c), nan_f32(case.c)
    ws, wsb = workspace(case)
    ok(lib.mednet_bn_act_bwd(dzg.data_ptr(), xg.data_ptr(), zg.data_ptr(), coef.data_ptr(), stats.data_ptr(), gam.data_ptr(), dx.data_ptr(), None,
                             dgamma.data_ptr(), dbeta.data_ptr(), case.n, case.spatial, case.c, ACT["relu"], ACT["none"], 0, dc, ws.data_ptr(), wsb,
                             L.stream()), "bn_act_bwd")
    out["dx"] = C.worst_ratio(dx, r.dx, B.dx, "dx")
    out["dgamma"] = C.worst_ratio(dgamma, r.dgamma, B.dgamma, "dgamma")
    out["dbeta"] = C.worst_ratio(dbeta, r.dbeta, B.dbeta, "dbeta")
    conclude(f"bn {case.n}x{case.c}x{case.shape} R={R} {mode}", out)


@pytest.mark.parametrize("mode", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("layer", ["gn", "bn"])
def test_modules_on_offset_data(layer, mode):
    """hnn.GroupNorm / hnn.BatchNorm3d (ops.py's path: workspaces, autograd, the running buffers) at the largest ratio of the mode, no
    activation (a module computes its own z: an activation's mask would not be the reference's)."""
    R = MODULE_R[mode]
    case, r, B = prepared("bn" if layer == "bn" else ("small" if mode == "fp32" else "wide"), R, mode, act="none")
    with mednet_hip.precision(mode):
        m = (hnn.BatchNorm3d(case.c, eps=case.eps, momentum=C.MOMENTUM) if layer == "bn" else hnn.GroupNorm(case.groups, case.c, eps=case.eps)).to(DEV)
        with torch.no_grad():
            m.weight.copy_(case.gamma)
            m.bias.copy_(case.beta)
        m.train()
        xg = vol(case.x, mode).requires_grad_(True)
        z = m(xg)
        (z.float() * case.dz.float().to(DEV)).sum().backward()
        torch.cuda.synchronize()
    out = {"z": C.worst_ratio(z, r.z, B.z, "z"), "dx": C.worst_ratio(xg.grad, r.dx, B.dx, "dx"),
           "dgamma": C.worst_ratio(m.weight.grad, r.dgamma, B.dgamma, "dgamma"), "dbeta": C.worst_ratio(m.bias.grad, r.dbeta, B.dbeta, "dbeta")}
    if layer == "bn":
        out["running_mean"] = C.worst_ratio(m.running_mean, r.running_mean, B.running_mean, "running_mean")
        out["running_var"] = C.worst_ratio(m.running_var, r.running_var, B.running_var, "running_var")
        assert int(m.num_batches_tracked.item()) == 1
    conclude(f"hnn.{type(m).__name__} R={R} {mode}", out)


# ------------------------------------------------------------------------------------------------ partial rows produced elsewhere
PRODUCED_SHAPE = (8, 16, 16)
PRODUCED_RATIO = 16.0


def check_produced(what, y, partial, mode, groups=8):
    """GroupNorm of the stored tensor y from the producer's rows against F.group_norm in fp64 of the same y: z and the statistics at
    the rel-L2 tolerance of test_group_norm_act."""
    n, c = y.shape[:2]
    g = C._rng("cond:produced:" + what)
    gamma, beta = torch.from_numpy(g.uniform(0.5, 1.5, c)).float(), torch.from_numpy(g.uniform(-0.5, 0.5, c)).float()
    y64 = y.detach().double().cpu()
    yu = y64.reshape(n * groups, -1)
    mean, var = yu.mean(1), yu.var(1, unbiased=False)
    ratio = float((mean.abs() / var.sqrt()).min())
    assert 0.5 * PRODUCED_RATIO <= ratio <= 2.0 * PRODUCED_RATIO, f"{what}: the output has mean / std {ratio:.2f}"
    with mednet_hip.precision(mode):
        stats, coef = ops.gn_statistics(y, gamma.to(DEV), beta.to(DEV), groups, C.EPS, partial)
        z = ops.group_norm_act(y, gamma.to(DEV), beta.to(DEV), groups, C.EPS, L.ACT_NONE, None, partial)
        torch.cuda.synchronize()
    for t in (stats, coef, z):
        assert bool(torch.isfinite(t.float()).all()), what
    zr = F.group_norm(y64, groups, gamma.double(), beta.double(), C.EPS)
    res = {"z": rel(z, zr), "mean": rel(stats[..., 0], mean.reshape(n, groups)), "rstd": rel(stats[..., 1], (1.0 / torch.sqrt(var + C.EPS)).reshape(n, groups))}
    print(f"[cond] produced rows, {what} {mode}: mean/std {ratio:.1f} rel-L2 " + " ".join(f"{k}={v:.3g}" for k, v in res.items()))
    assert max(res.values()) <= TOL[mode], (what, mode, res)


FP32_FUSED_SHAPE = (32, 32, 64)     # 2 x 128 tiles of 4 x 8 x 16: the smallest at which the fp32 forward kernel keeps the sums (256 CUs)


@pytest.mark.parametrize("mode,shape", [("fp32", PRODUCED_SHAPE), ("bf16", PRODUCED_SHAPE), ("fp32", FP32_FUSED_SHAPE)], ids=lambda v: str(v))
def test_rows_of_a_convolutions_epilogue_on_offset_output(mode, shape):
    """conv 32 -> 32 (no bias: the layers that fuse the sums have none): input channel 0 is the constant 1 and its centre tap carries the
    offset, the other 31 channels give an output deviation of ~1.  At (8, 16, 16) the fp32 forward kernel has too few tiles to keep
    the sums (mednet_conv3d_fused_stats_chunks = 0, by its plan): the GroupNorm behind it takes the stand-alone pass, and that is
    what the case checks there; the fp32 epilogue's rows are checked at the smallest shape that has them."""
    n, c = 2, 32
    g = C._rng("cond:conv")
    x = torch.from_numpy(g.standard_normal((n, c, *shape))).float()
    x[:, 0] = 1.0
    w = torch.from_numpy(g.standard_normal((c, c, 3, 3, 3))).float() / np.sqrt(31 * 27.0)
    w[:, 0] = 0.0
    w[:, 0, 1, 1, 1] = torch.from_numpy(PRODUCED_RATIO * (1.0 + g.uniform(-1, 1, c) / 64))
    with mednet_hip.precision(mode):
        conv = hnn.Conv3d(c, c, 3, bias=False).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(w)
        with torch.no_grad():
            y, partial = conv.forward_with_stats(vol(x.double(), mode))
        torch.cuda.synchronize()
        chunks = L.lib().mednet_conv3d_fused_stats_chunks(n, *shape, c, c, 3, L.dt_of(DT[mode]), L.dt_of(DT[mode]), mednet_hip.config.conv_algo())
    assert (partial is not None) == (chunks > 0), "the rows and the plan query disagree"
    if mode == "fp32" and shape == PRODUCED_SHAPE:
        assert partial is None, "the fp32 kernel now keeps the sums at this shape: drop the larger case"
        return check_produced("conv, stand-alone pass behind it", y, None, mode)
    assert partial is not None, "the convolution did not produce the rows"
    check_produced(f"conv epilogue {shape}", y, partial, mode)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_rows_of_the_concatenation_on_offset_input(mode):
    n, ce, cx = 2, 16, 16
    g = C._rng("cond:upcat")
    enc = PRODUCED_RATIO + torch.from_numpy(g.standard_normal((n, ce, *PRODUCED_SHAPE)))
    x = -PRODUCED_RATIO + torch.from_numpy(g.standard_normal((n, cx, *(s // 2 for s in PRODUCED_SHAPE))))
    with mednet_hip.precision(mode):
        with torch.no_grad():
            out, partial = ops.upsample_concat(vol(enc, mode), vol(x, mode), True)
        torch.cuda.synchronize()
    assert partial is not None, "the concatenation did not produce the rows"
    check_produced("upcat", out, partial, mode)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_finalize_of_rows_from_outside_on_offset_data(mode):
    """mednet_gn_finalize on rows the test writes: the exact sums of 64-voxel chunks, rounded to fp32."""
    n, c, chunk = 2, 32, 64
    g = C._rng("cond:foreign")
    sign = torch.tensor([1.0, -1.0]).reshape(n, 1, 1, 1, 1)
    y = vol(sign * PRODUCED_RATIO + torch.from_numpy(g.standard_normal((n, c, *PRODUCED_SHAPE))), mode)
    rows = y.detach().double().cpu().reshape(n, c, -1, chunk)                      # [n][c][chunks][chunk]
    partial = torch.stack((rows.sum(-1), (rows * rows).sum(-1)), -1).permute(0, 2, 1, 3).contiguous().float().to(DEV)   # [n][chunks][c][2]
    check_produced("rows from outside", y, partial, mode)
