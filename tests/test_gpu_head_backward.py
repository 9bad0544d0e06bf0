"""The backward kernels of the five fused head-and-loss nodes at operator level (-m gpu), through the C ABI with dz, gn_partial,
dW and db pre-filled with NaN, the GroupNorm-3 sums (gn_partial = {sum du, sum du * gn_y}, du = dz * act'(z)) included -- the
output every default training step uses and no other operator test reads.

A. mednet_head_dice_bwd / mednet_head_ce_bwd (head_loss.hip, <= 4 classes) against the three unfused launches on the same device
   tensors (mednet_conv3d_fwd k = 1, mednet_dice_bwd_lt / mednet_ce_bwd, mednet_head_dgrad_gn): dz and every row of gn_partial
   EQUAL, the row counts equal, for gn_act none / ReLU / LeakyReLU / ELU; with gn_y == NULL the stored dz equals mednet_act_bwd of
   the unfused stored dz (the fold rule).  dW / db are summed in another order than the unfused weight gradient: they are held to
   2^-16 * sum |dl| |z| per element against the fp64 sum of the unfused logit gradient (at most 32 fp32 accumulations per lane
   and 3 in the wave sum, the rest of the sum is made in fp64: under 2^-19).

B. mednet_head_seg_bwd and mednet_head_landmark_cls_bwd (head_mfma.hip, the matrix-core heads) against ATen in fp64 on the CPU,
   per element (gpu_util.check_gradient / check_gn_sums):
     GroupNorm sums   |got - want| <= 2^-16 * sum |terms|, want formed in fp64 from the kernel's own STORED dz: a lane adds at most
                      64 terms (16 trips of 4 voxels), the workgroup's fixed-order sum 128 more, ELU's dz * (z + 1) rounds once per
                      term -- under 256 fp32 roundings of 2^-24; the fp64 row total adds none.
     dz               |dz - dz64| <= u |dz64| + eps_case * A + s, u = 2^-8 (bf16) / 2^-11 (fp16) the store's rounding,
                      A[c, v] = sum_k |W[k, c]| |dl64[k, v]|, s = 2^-25 in fp16 (half the smallest subnormal).
     dW, db           |dW - dW64| <= eps_case * B, B[k, c] = sum_{n, v} |dl64[k, v]| |z[c, v]| (db: sum |dl64|).
   eps_case = max(2^-15, 8 * r32), per tensor, with r32 = max |x32 - x64| / A (resp. / B) of ATen's own fp32 evaluation of the
   same chain on the CPU: the reference is the yardstick, never the kernel.  2^-15 is the kernel's arithmetic (the 16-bit-pair
   image of dl, the dropped lo * lo product, up to about 264 fp32 accumulations per lane in dW: each at or below 2^-16), doubled;
   the factor 8 covers expf / reciprocal a few ulp apart, fixed-order against pairwise sums, and `saved` taken from fp32 partial
   sums.  Every case prints one `[exact] item=head_bwd ...` line with r32, eps_case and the observed worst ratio; the worst per head
   and mode are recorded in profiles/head_backward_bounds.md.
   The heads do not fold an activation into dz: gn_act only enters the sums, so dz / dW / db of the runs of one case that differ
   in gn_act or in gn_y == NULL must be the very bits of the run that was checked against fp64.
   Delivery: ops.head_seg / ops.head_landmark hand the same gn_partial to the producing node through ops.GN3Hook.

tests/test_exact_util.py runs the checkers on the CPU: they pass for ATen's fp32 results of every case of part B and reject a
dropped voxel run, a wrong activation factor, a missing class, a swapped dW row and a bf16-rounded fp16 gradient.
"""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import nn as hnn
from mednet_hip import ops
from oracle import ref_cpu as O

from gpu_util import DEV, DT, SUM_BOUND, U_STORE, check_gn_sums, check_gradient, half_round, ref_error, rnd, split_weight

pytestmark = pytest.mark.gpu
CL = torch.channels_last_3d
ACTS = (L.ACT_NONE, L.ACT_RELU, L.ACT_LEAKY, L.ACT_ELU)
ACT_NAME = {L.ACT_NONE: "none", L.ACT_RELU: "relu", L.ACT_LEAKY: "leaky", L.ACT_ELU: "elu"}
Z_MIN = -1.0 + 2.0 ** -8   # an ELU output is > -1; this is the smallest such bf16 (and an fp16) number


def gscale_of(mode):
    """The loss scalar of the existing head tests: fp16 stores the feature gradient, scaled as train.LossScaler does."""
    return 3.0 * 16384.0 if mode == "fp16" else 3.0


def act_output(u, act, mode):
    """The activation applied to a pre-activation and rounded to the storage type: what a block hands the head."""
    z = {L.ACT_NONE: u, L.ACT_RELU: F.relu(u), L.ACT_LEAKY: F.leaky_relu(u, 0.1), L.ACT_ELU: F.elu(u)}[act]
    z = half_round(z, mode)
    return z.clamp(min=Z_MIN) if act == L.ACT_ELU else z


def nan_like(shape, dtype, cl=False):
    t = torch.full(shape, float("nan"), device=DEV).to(dtype)
    return t.contiguous(memory_format=CL) if cl else t


def to_dev_cl(t, dtype):
    return t.to(DEV).to(dtype).contiguous(memory_format=CL)


# ============================================================================================ A. heads with up to 4 classes
# spatial sizes per cin, read off hl_bwd_blocks: a workgroup takes (256 / (cin / 8)) * 32 voxels, two per lane and trip.
# First: less than one workgroup's share and odd (a last trip with one voxel); second: three workgroups, the last one ragged.
A_SHAPES = {16: [(5, 7, 33), (9, 23, 41)], 32: [(5, 7, 33), (9, 11, 43)], 64: [(4, 6, 7), (5, 7, 63)]}
A_CASES = [(cin, shape) for cin in (16, 32, 64) for shape in A_SHAPES[cin]]
# (loss, classes, sigmoid, ignore_index): weighted Dice and weighted CE with an ignore_index that occurs in the labels
A_LOSSES = [("DICE", 1, True, None), ("DICE", 2, False, 1), ("DICE", 4, False, 2), ("CE", 2, False, 1), ("CE", 4, False, 3)]
A_WEIGHT = [0.05, 1.0, 0.7, 1.3]


def _share(cin):
    return (256 // (cin // 8)) * 32


def test_part_a_shapes_sit_where_the_plan_says():
    for cin, (small, big) in A_SHAPES.items():
        s, b, trip = int(np.prod(small)), int(np.prod(big)), 2 * (256 // (cin // 8))    # a trip of the workgroup takes 2 voxels per lane
        assert s < _share(cin) and s % trip != 0 and s % (trip // 2) != 0
        assert 2 * _share(cin) < b <= 3 * _share(cin) and b % trip != 0 and b % (trip // 2) != 0
        if torch.cuda.is_available():
            assert L.lib().mednet_head_dice_gn_rows(2, b, cin) == 12 and L.lib().mednet_head_dice_gn_rows(2, s, cin) == 4


def _unfused(lib, kind, zg, pk, bias, lab, lab_dt, lab_sn, lab64, wt, gyg, act, n, shape, cin, cout, dcode, dl, eps, sigmoid, ii, dt):
    """mednet_conv3d_fwd (planar fp32 logits) -> loss forward (saved) -> mednet_dice_bwd_lt / mednet_ce_bwd -> mednet_head_dgrad_gn."""
    d, h, w = shape
    spatial = d * h * w
    logits = nan_like((n, cout, d, h, w), torch.float32)
    L.check(lib.mednet_conv3d_fwd(zg.data_ptr(), pk.data_ptr(), bias.data_ptr(), logits.data_ptr(), n, d, h, w, cin, cout, 1, dcode,
                                  L.NDHWC, L.F32, L.NCDHW, 0, mednet_hip.config.conv_algo(), None, L.stream()), "conv3d_fwd")
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    saved = torch.zeros((max(cout, 1), 2), dtype=torch.float32, device=DEV)
    ws = L.workspace(lib.mednet_loss_ws_bytes(n, cout, spatial), zg.device)
    dlg = nan_like((n, cout, d, h, w), torch.float32)
    sn, sc = cout * spatial, spatial
    if kind == "DICE":
        L.check(lib.mednet_dice_fwd_lt(logits.data_ptr(), lab.data_ptr(), lab_dt, lab_sn, wt.data_ptr(), loss.data_ptr(), saved.data_ptr(),
                                       None, n, cout, spatial, sn, sc, eps, int(sigmoid), ii, ws.data_ptr(), ws.numel(), L.stream()), "dice_fwd_lt")
        L.check(lib.mednet_dice_bwd_lt(logits.data_ptr(), lab.data_ptr(), lab_dt, lab_sn, wt.data_ptr(), saved.data_ptr(), dl.data_ptr(),
                                       dlg.data_ptr(), n, cout, spatial, sn, sc, eps, int(sigmoid), ii, L.stream()), "dice_bwd_lt")
    else:
        L.check(lib.mednet_ce_fwd(logits.data_ptr(), lab64.data_ptr(), wt.data_ptr(), loss.data_ptr(), saved.data_ptr(), n, cout, spatial,
                                  sn, sc, ii, ws.data_ptr(), ws.numel(), L.stream()), "ce_fwd")
        L.check(lib.mednet_ce_bwd(logits.data_ptr(), lab64.data_ptr(), wt.data_ptr(), saved.data_ptr(), dl.data_ptr(), dlg.data_ptr(), n,
                                  cout, spatial, sn, sc, ii, L.stream()), "ce_bwd")
    rows = lib.mednet_head_dgrad_gn_rows(n, d, h, w, cin, dcode)
    assert rows > 0
    dz = nan_like((n, cin, d, h, w), dt, cl=True)
    part = nan_like((n, rows, cin, 2), torch.float32)
    L.check(lib.mednet_head_dgrad_gn(dlg.data_ptr(), pk.data_ptr(), dz.data_ptr(), gyg.data_ptr(), zg.data_ptr(), act, part.data_ptr(),
                                     n, d, h, w, cin, cout, dcode, L.stream()), "head_dgrad_gn")
    return logits, loss, saved, dlg, dz, part, rows


def _fused(lib, kind, zg, pk, bias, lab, lab_dt, lab_sn, wt, gyg, act, n, shape, cin, cout, dcode, dl, eps, sigmoid, ii, dt):
    """mednet_head_dice_fwd / _bwd or mednet_head_ce_fwd / _bwd; gyg None: no sums (and the fold rule if act is not none)."""
    d, h, w = shape
    spatial = d * h * w
    logits = nan_like((n, cout, d, h, w), torch.float32)
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    saved = torch.zeros((max(cout, 1), 2), dtype=torch.float32, device=DEV)
    nbytes = lib.mednet_head_dice_ws_bytes(n, spatial, cin, cout) if kind == "DICE" else lib.mednet_head_ce_ws_bytes(n, spatial, cin, cout)
    ws = L.workspace(nbytes, zg.device)
    rows = lib.mednet_head_dice_gn_rows(n, spatial, cin) if kind == "DICE" else lib.mednet_head_ce_gn_rows(n, spatial, cin)
    dz = nan_like((n, cin, d, h, w), dt, cl=True)
    part = nan_like((n, rows, cin, 2), torch.float32) if gyg is not None else None
    dw, db = nan_like((cout, cin), torch.float32), nan_like((cout,), torch.float32)
    if kind == "DICE":
        L.check(lib.mednet_head_dice_fwd(zg.data_ptr(), pk.data_ptr(), bias.data_ptr(), lab.data_ptr(), lab_dt, lab_sn, wt.data_ptr(),
                                         logits.data_ptr(), loss.data_ptr(), saved.data_ptr(), n, spatial, cin, cout, eps, int(sigmoid),
                                         ii, dcode, ws.data_ptr(), ws.numel(), L.stream()), "head_dice_fwd")
        L.check(lib.mednet_head_dice_bwd(logits.data_ptr(), lab.data_ptr(), lab_dt, lab_sn, pk.data_ptr(), wt.data_ptr(), saved.data_ptr(),
                                         dl.data_ptr(), dz.data_ptr(), L.ptr(gyg), zg.data_ptr(), act, L.ptr(part), dw.data_ptr(),
                                         db.data_ptr(), n, spatial, cin, cout, eps, int(sigmoid), ii, dcode, ws.data_ptr(), ws.numel(),
                                         L.stream()), "head_dice_bwd")
    else:
        L.check(lib.mednet_head_ce_fwd(zg.data_ptr(), pk.data_ptr(), bias.data_ptr(), lab.data_ptr(), lab_dt, lab_sn, wt.data_ptr(),
                                       logits.data_ptr(), loss.data_ptr(), saved.data_ptr(), n, spatial, cin, cout, ii, dcode,
                                       ws.data_ptr(), ws.numel(), L.stream()), "head_ce_fwd")
        L.check(lib.mednet_head_ce_bwd(logits.data_ptr(), lab.data_ptr(), lab_dt, lab_sn, pk.data_ptr(), wt.data_ptr(), saved.data_ptr(),
                                       dl.data_ptr(), dz.data_ptr(), L.ptr(gyg), zg.data_ptr(), act, L.ptr(part), dw.data_ptr(),
                                       db.data_ptr(), n, spatial, cin, cout, ii, dcode, ws.data_ptr(), ws.numel(), L.stream()), "head_ce_bwd")
    return logits, loss, saved, dz, part, dw, db, rows


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("cin,shape", A_CASES)
def test_small_heads_backward_equals_the_unfused_launches_sums_included(mode, cin, shape):
    """Part A of the module docstring, n = 2; losses, label forms (the last channel of a uint8 volume where it lies, int64) and the
    activations are looped inside."""
    n, eps = 2, 1e-5
    dt, dcode = DT[mode], L.dt_of(DT[mode])
    lib = L.lib()
    d, h, w = shape
    spatial = d * h * w
    tag = f"hbA{cin}{shape}"
    u = rnd(tag + "u", n, cin, *shape)
    gy = half_round(rnd(tag + "y", n, cin, *shape), mode)
    gyg = to_dev_cl(gy, dt)
    dl = torch.tensor(gscale_of(mode), dtype=torch.float32, device=DEV)
    zs = {act: act_output(u, act, mode) for act in ACTS}
    zgs = {act: to_dev_cl(zs[act], dt) for act in ACTS}
    compared = 0
    with mednet_hip.precision(mode):
        compared = _part_a_loop(lib, mode, cin, shape, n, eps, dt, dcode, tag, gyg, dl, zs, zgs)
    print(f"[exact] item=head_bwd A cin={cin} {shape} {mode} kernel=head_dice_bwd_kernel elements={compared}")


def _part_a_loop(lib, mode, cin, shape, n, eps, dt, dcode, tag, gyg, dl, zs, zgs):
    d, h, w = shape
    spatial = d * h * w
    compared = 0
    for kind, cout, sigmoid, ignore in A_LOSSES:
        assert lib.mednet_head_dice_supported(cin, cout, dcode, L.U8) == 1 and lib.mednet_head_ce_supported(cin, cout, dcode, L.I64) == 1
        wgt, b = rnd(tag + f"w{cout}", cout, cin, 1, 1, 1, scale=0.3), rnd(tag + f"b{cout}", cout).to(DEV)
        pk = ops.pack_conv_weight(wgt.to(DEV), 1, False)
        wt = torch.tensor(A_WEIGHT[:cout], device=DEV)
        g = np.random.Generator(np.random.PCG64(91 + cout))
        vol = torch.from_numpy(g.integers(0, cout, size=(n, 2) + shape).astype(np.uint8)).to(DEV)   # (one class: every label is 0)
        lab_u8 = vol[:, -1]
        lab64 = lab_u8.long().contiguous()
        ii = (L.NO_IGNORE if kind == "DICE" else -100) if ignore is None else ignore
        for lab, lab_dt, lab_sn in ((lab_u8, L.U8, 2 * spatial), (lab64, L.I64, spatial)):
            for act in ACTS:
                zg, what = zgs[act], f"{kind} C={cout} {mode} cin={cin} {shape} labels={lab_dt} act={ACT_NAME[act]}"
                args = (n, shape, cin, cout, dcode, dl, eps, sigmoid, ii, dt)
                lg0, loss0, saved0, dlg, dz0, part0, rows0 = _unfused(lib, kind, zg, pk, b, lab, lab_dt, lab_sn, lab64, wt, gyg, act, *args)
                lg1, loss1, saved1, dz1, part1, dw1, db1, rows1 = _fused(lib, kind, zg, pk, b, lab, lab_dt, lab_sn, wt, gyg, act, *args)
                torch.cuda.synchronize()
                nsaved = 2 * cout if kind == "DICE" else 1
                assert torch.equal(lg0, lg1) and torch.equal(loss0, loss1), what + ": logits / loss of the fused forward differ"
                assert torch.equal(saved0.flatten()[:nsaved], saved1.flatten()[:nsaved]), what + ": saved differs"
                assert not bool(torch.isnan(dz0).any()) and torch.equal(dz0, dz1), what + ": dz differs from the unfused dz"
                assert rows1 == rows0, f"{what}: {rows1} rows of gn_partial against mednet_head_dgrad_gn_rows = {rows0}"
                assert not bool(torch.isnan(part1).any()), what + ": a row of gn_partial was not written"
                assert torch.equal(part0, part1), what + ": gn_partial differs from mednet_head_dgrad_gn's rows"
                # dW / db: fp64 sums of the unfused logit gradient
                dl64, z64 = dlg.double().cpu().reshape(n, cout, spatial), zs[act].double().reshape(n, cin, spatial)
                dw64, bw = torch.einsum("nkv,ncv->kc", dl64, z64), torch.einsum("nkv,ncv->kc", dl64.abs(), z64.abs())
                check_gradient(dw1, dw64, bw, SUM_BOUND, what + ": dW")
                check_gradient(db1, dl64.sum((0, 2)), dl64.abs().sum((0, 2)), SUM_BOUND, what + ": db")
                compared += 2 * dz1.numel() + part1.numel()
                # gn_y == NULL: no sums; an activation is folded into the stored gradient as mednet_act_bwd would
                _, _, _, dz2, part2, dw2, db2, _ = _fused(lib, kind, zg, pk, b, lab, lab_dt, lab_sn, wt, None, act, *args)
                want = dz0
                if act != L.ACT_NONE:
                    want = nan_like((n, cin, d, h, w), dt, cl=True)
                    L.check(lib.mednet_act_bwd(dz0.data_ptr(), zg.data_ptr(), want.data_ptr(), dz0.numel(), act, dcode, L.stream()), "act_bwd")
                torch.cuda.synchronize()
                assert part2 is None
                assert not bool(torch.isnan(want).any()) and torch.equal(dz2, want), what + ": the folded dz differs from mednet_act_bwd(unfused dz)"
                assert torch.equal(dw2, dw1) and torch.equal(db2, db1), what + ": dW / db depend on gn_y"
                compared += dz2.numel()
    return compared


# ============================================================================================ B. the matrix-core heads
# (n, shape): half a run; two runs and two idle waves; a ragged last run; two chunks per sample, the second one short
B_SHAPES = [(2, (4, 4, 4)), (1, (4, 6, 10)), (3, (12, 10, 6)), (2, (16, 16, 36))]
B_MODES = ["bf16", "fp16"]
SEG_CLASSES = (5, 9, 16)
LM_HEADS = ((1, 1), (5, 3), (16, 2), (16, 4))
Z_KINDS = ("elu", "relu")   # the block output: of an ELU (> -1; serves none and LeakyReLU too) or of a ReLU (>= 0)
RUN_ACTS = {"elu": (L.ACT_ELU, L.ACT_NONE, L.ACT_LEAKY), "relu": (L.ACT_RELU,)}


def seg_weights(c):
    return torch.tensor([0.05] + [0.6 + 0.1 * (k % 7) for k in range(1, c)])


def variants_of(head):
    """seg: (ncls, class loss, sigmoid, ignore_index); lm: (nh, ncls, class loss, regression, sigmoid, ignore_index).  All class
    losses weighted."""
    if head == "seg":
        return [(c, kind, False, ig) for c in SEG_CLASSES for kind, ig in (("DICE", 2), ("CE", 3))]
    out = []
    for nh, ncls in LM_HEADS:
        for reg in ("L2", "L1"):
            out.append((nh, ncls, "DICE", reg, ncls == 1, None))
            if ncls > 1:   # (nn.CrossEntropyLoss is softmax only)
                out.append((nh, ncls, "CE", reg, False, ncls - 1 if ncls > 2 else None))
    return out


@functools.lru_cache(maxsize=4)
def head_case(head, mode, n, shape, variant, zkind):
    """Inputs of one case of part B (fp32 tensors holding numbers of the storage type where the kernel stores them) and both ATen
    references, fp64 and fp32, with the norms A, B of the bounds and eps_case per tensor.  Cached: the tests share it."""
    c = types.SimpleNamespace(head=head, mode=mode, n=n, shape=shape, variant=variant, zkind=zkind, gscale=gscale_of(mode))
    if head == "seg":
        c.ncls, c.kind, c.sigmoid, c.ignore = variant
        c.nh, c.reg = 0, None
        c.cw = seg_weights(c.ncls)
    else:
        c.nh, c.ncls, c.kind, c.reg, c.sigmoid, c.ignore = variant
        c.cw = torch.tensor([0.05, 1.0, 0.7, 1.2][:c.ncls])
        c.rw = torch.tensor([0.015 + 0.003 * i for i in range(c.nh)])
    m = c.m = c.nh + c.ncls
    tag = f"hbB{head}{n}{shape}{m}"
    u = rnd(tag + "u", n, 32, *shape)
    c.z = act_output(u, L.ACT_ELU if zkind == "elu" else L.ACT_RELU, mode)
    assert float(c.z.min()) > -1 if zkind == "elu" else float(c.z.min()) >= 0
    assert bool((c.z < 0).any()) if zkind == "elu" else bool((c.z == 0).any())
    c.gy = half_round(rnd(tag + "y", n, 32, *shape), mode)
    c.W = split_weight(rnd(tag + "w", m, 32, scale=0.3), mode)
    c.b = rnd(tag + "b", m)
    if head == "lm":
        c.b[:c.nh] = 8.0 + 0.25 * c.b[:c.nh]       # heat maps are 0 or 16: sign(out - heatmap) of L1 cannot depend on rounding
    g = np.random.Generator(np.random.PCG64(1000 * m + n + shape[2]))
    vol = np.empty((n, c.nh + 1) + shape, dtype=np.uint8)       # the label volume: heat maps, then the class labels
    vol[:, :c.nh] = 16 * g.integers(0, 2, size=(n, c.nh) + shape)
    vol[:, c.nh] = g.integers(0, c.ncls, size=(n,) + shape)       # (one class: every label is 0)
    c.vol = torch.from_numpy(vol)
    c.hm, c.lab = c.vol[:, :c.nh], c.vol[:, c.nh]
    r64, r32 = _chain(c, torch.float64), _chain(c, torch.float32)
    if c.reg == "L1":   # a condition on the inputs, checked before any GPU run: no element is left out of a comparison
        gap = float((r64.logits[:, :c.nh] - c.hm.double()).abs().min())
        assert gap >= 2.0 ** -6, f"L1: min |out - heatmap| = {gap:.3e} < 2^-6"
    dl, z64, W64 = r64.dl.reshape(n, m, -1), c.z.double().reshape(n, 32, -1), c.W.double()
    c.ref, c.ref32 = r64, r32
    c.A = torch.einsum("kc,nkv->ncv", W64.abs(), dl.abs()).reshape(c.z.shape)
    c.B = torch.einsum("nkv,ncv->kc", dl.abs(), z64.abs())
    c.Bb = dl.abs().sum((0, 2))
    c.r32, c.eps = {}, {}
    for name, x32, x64, norm in (("dz", r32.dz, r64.dz, c.A), ("dW", r32.dW, r64.dW, c.B), ("db", r32.db, r64.db, c.Bb)):
        c.r32[name], c.eps[name] = ref_error(x32, x64, norm, f"{name} of {case_name(c)}")
    return c


def case_name(c):
    v = f"C={c.ncls} {c.kind}" if c.head == "seg" else f"nh={c.nh} C={c.ncls} {c.kind} {c.reg}"
    return f"{c.head} {c.mode} n={c.n} {c.shape} {v} sig={int(c.sigmoid)} ign={c.ignore} z={c.zkind}"


def _chain(c, dtype):
    """ATen on the CPU in `dtype`: conv3d -> class loss (oracle DiceLoss | F.cross_entropy) [+ weighted MSE / L1 sum], both scaled by
    the loss scalar; autograd for the logit gradient dl and dz, dW, db."""
    z, W, b = (t.detach().clone().to(dtype).requires_grad_(True) for t in (c.z, c.W, c.b))   # (.to(float32) alone would alias the inputs)
    lg = F.conv3d(z, W[:, :, None, None, None], b)
    lg.retain_grad()
    cls = lg[:, c.nh:]
    lab = c.lab.long()
    if c.kind == "DICE":
        closs = O.DiceLoss(weight=c.cw.to(dtype), sigmoid_normalization=c.sigmoid, ignore_index=c.ignore)(cls, lab)
    else:
        closs = F.cross_entropy(cls, lab, weight=c.cw.to(dtype), ignore_index=-100 if c.ignore is None else c.ignore)
    total = c.gscale * closs
    if c.head == "lm":
        diff = lg[:, :c.nh] - c.hm.to(dtype)
        per = (diff * diff if c.reg == "L2" else diff.abs()).mean((0, 2, 3, 4))
        total = total + c.gscale * (c.rw.to(dtype) * per).sum()
    total.backward()
    return types.SimpleNamespace(logits=lg.detach(), dl=lg.grad, dz=z.grad, dW=W.grad, db=b.grad)


def check_case_gradients(c, dz, dW, db, what=""):
    """dz (n x 32 x shape, the stored values), dW [m][32], db [m] of a case against its fp64 reference.  -> observed ratios."""
    name = what or case_name(c)
    s = 2.0 ** -25 if c.mode == "fp16" else 0.0
    return dict(dz=check_gradient(dz, c.ref.dz, c.A, c.eps["dz"], name + ": dz", u=U_STORE[c.mode], s=s),
                dW=check_gradient(dW, c.ref.dW, c.B, c.eps["dW"], name + ": dW"),
                db=check_gradient(db, c.ref.db, c.Bb, c.eps["db"], name + ": db"))


def report_case(c, seen, sums):
    print(f"[exact] item=head_bwd {case_name(c)} kernel={'head_seg_kernel' if c.head == 'seg' else 'head_lm_kernel'} "
          + " ".join(f"{k}: r32 {c.r32[k]:.2e} eps {c.eps[k]:.2e} seen {seen[k]:.2e}" for k in ("dz", "dW", "db"))
          + f" sums: bound {SUM_BOUND:.2e} seen {sums:.2e}")


class _Device:
    """The device tensors of a case and one call of the library's forward + backward, as the autograd node makes them."""

    def __init__(self, c):
        self.c, self.dt, self.dcode = c, DT[c.mode], L.dt_of(DT[c.mode])
        self.z, self.gy = to_dev_cl(c.z, self.dt), to_dev_cl(c.gy, self.dt)
        with mednet_hip.precision(c.mode):
            self.pk = ops.pack_conv_weight(c.W[:, :, None, None, None].to(DEV), 1, False)
        self.b, self.cw = c.b.to(DEV), c.cw.to(DEV)
        self.vol = c.vol.to(DEV)
        self.spatial = int(np.prod(c.shape))
        self.vol_sn = (c.nh + 1) * self.spatial
        self.hm, self.lab = self.vol[:, :c.nh], self.vol[:, c.nh]
        assert self.lab.data_ptr() % 4 == 0 and self.vol_sn % 4 == 0
        self.rw = c.rw.to(DEV) if c.head == "lm" else None
        self.dl = torch.tensor(c.gscale, dtype=torch.float32, device=DEV)
        self.ck = L.CLASS_DICE if c.kind == "DICE" else L.CLASS_CE
        self.ii = (L.NO_IGNORE if c.kind == "DICE" else -100) if c.ignore is None else int(c.ignore)
        self.rk = L.REG_L1 if c.reg == "L1" else L.REG_L2
        lib = L.lib()
        if c.head == "seg":
            assert lib.mednet_head_seg_supported(32, c.ncls, self.dcode, L.U8, self.spatial) == 1
            self.ws = L.workspace(lib.mednet_head_seg_ws_bytes(c.n, self.spatial, c.ncls), self.z.device)
            self.rows = lib.mednet_head_seg_gn_rows(self.spatial)
        else:
            assert lib.mednet_head_landmark_supported(32, c.nh, c.ncls, self.dcode, self.spatial) == 1
            self.ws = L.workspace(lib.mednet_head_landmark_ws_bytes(c.n, self.spatial, c.nh, c.ncls), self.z.device)
            self.rows = lib.mednet_head_landmark_gn_rows(self.spatial)
        assert self.rows == -(-(-(-self.spatial // 128)) // 64)
        self.saved = torch.zeros((max(c.ncls, 1), 2), dtype=torch.float32, device=DEV)
        self.forward()

    def forward(self):
        c, lib, ws = self.c, L.lib(), self.ws
        loss, rloss = (torch.empty((), dtype=torch.float32, device=DEV) for _ in range(2))
        if c.head == "seg":
            L.check(lib.mednet_head_seg_fwd(self.z.data_ptr(), self.pk.data_ptr(), self.b.data_ptr(), self.lab.data_ptr(), self.vol_sn,
                                            self.cw.data_ptr(), None, loss.data_ptr(), self.saved.data_ptr(), c.n, self.spatial, 32, c.ncls,
                                            self.ck, 1e-5, int(c.sigmoid), self.ii, self.dcode, ws.data_ptr(), ws.numel(), L.stream()),
                    "head_seg_fwd")
        else:
            L.check(lib.mednet_head_landmark_cls_fwd(self.z.data_ptr(), self.pk.data_ptr(), self.b.data_ptr(), self.hm.data_ptr(), self.vol_sn,
                                                     self.lab.data_ptr(), self.vol_sn, self.cw.data_ptr(), self.rw.data_ptr(), None,
                                                     loss.data_ptr(), rloss.data_ptr(), self.saved.data_ptr(), None, c.n, self.spatial, 32,
                                                     c.nh, c.ncls, self.rk, self.ck, 1e-5, int(c.sigmoid), self.ii, self.dcode,
                                                     ws.data_ptr(), ws.numel(), L.stream()), "head_landmark_cls_fwd")

    def backward(self, act, with_gy):
        c, lib, ws = self.c, L.lib(), self.ws
        dz = nan_like((c.n, 32) + c.shape, self.dt, cl=True)
        part = nan_like((c.n, self.rows, 32, 2), torch.float32) if with_gy else None
        dw, db = nan_like((c.m, 32), torch.float32), nan_like((c.m,), torch.float32)
        gy = self.gy.data_ptr() if with_gy else None
        if c.head == "seg":
            L.check(lib.mednet_head_seg_bwd(self.z.data_ptr(), self.pk.data_ptr(), self.b.data_ptr(), self.lab.data_ptr(), self.vol_sn,
                                            self.cw.data_ptr(), self.saved.data_ptr(), self.dl.data_ptr(), dz.data_ptr(), gy, act,
                                            L.ptr(part), dw.data_ptr(), db.data_ptr(), c.n, self.spatial, 32, c.ncls, self.ck, 1e-5,
                                            int(c.sigmoid), self.ii, self.dcode, ws.data_ptr(), ws.numel(), L.stream()), "head_seg_bwd")
        else:
            L.check(lib.mednet_head_landmark_cls_bwd(self.z.data_ptr(), self.pk.data_ptr(), self.b.data_ptr(), self.hm.data_ptr(), self.vol_sn,
                                                     self.lab.data_ptr(), self.vol_sn, self.cw.data_ptr(), self.rw.data_ptr(),
                                                     self.saved.data_ptr(), self.dl.data_ptr(), self.dl.data_ptr(), dz.data_ptr(), gy, act,
                                                     L.ptr(part), dw.data_ptr(), db.data_ptr(), c.n, self.spatial, 32, c.nh, c.ncls, self.rk,
                                                     self.ck, 1e-5, int(c.sigmoid), self.ii, self.dcode, ws.data_ptr(), ws.numel(),
                                                     L.stream()), "head_landmark_cls_bwd")
        torch.cuda.synchronize()
        return dz, part, dw, db


@pytest.mark.parametrize("mode", B_MODES)
@pytest.mark.parametrize("n,shape", B_SHAPES)
@pytest.mark.parametrize("head", ["seg", "lm"])
def test_matrix_core_heads_backward_per_element_against_fp64(head, mode, n, shape):
    """Part B of the module docstring for one head, mode and shape; class counts, loss variants and activations are looped inside."""
    for variant in variants_of(head):
        for zkind in Z_KINDS:
            c = head_case(head, mode, n, shape, variant, zkind)
            dev = _Device(c)
            first, worst_sum = None, 0.0
            for act in RUN_ACTS[zkind]:
                for with_gy in (True, False):
                    dz, part, dw, db = dev.backward(act, with_gy)
                    what = f"{case_name(c)} act={ACT_NAME[act]} gn_y={'given' if with_gy else 'NULL'}"
                    if first is None:
                        seen = check_case_gradients(c, dz, dw, db, what)
                        first = (dz, dw, db)
                    else:   # gn_act and gn_y only enter the sums: the bits of the run checked against fp64
                        for got, ref, name in zip((dz, dw, db), first, ("dz", "dW", "db")):
                            assert torch.equal(got, ref), f"{what}: {name} depends on gn_act / gn_y"
                    if with_gy:
                        worst_sum = max(worst_sum, check_gn_sums(part, dz.float(), c.z, c.gy, act, what))
                    else:
                        assert part is None
            report_case(c, seen, worst_sum)


# ---------------------------------------------------------------------------------------------- delivery through ops
class _Producer(torch.autograd.Function):
    """Stands where the ExtResNetBlock stands: its backward receives the head's feature gradient as autograd hands it on and asks
    the hook for the sums there (block.py does the same before any conversion).  A leaf's .grad is a detached alias made by
    autograd, never the tensor the head produced, so the hook is asked here and not with x.grad."""

    @staticmethod
    def forward(ctx, x, hook, box):
        ctx.hook, ctx.box = hook, box
        return x.view_as(x)

    @staticmethod
    def backward(ctx, dout):
        ctx.box["dout"] = dout
        ctx.box["partial"] = ctx.hook.take(dout)
        return dout, None, None


def _deliver(c, call):
    """ops.<head> on a feature tensor that carries a hand-made ops.GN3Hook (gn_in, act = ELU), backward(): -> what the producing node
    received (dout, partial) and the ABI call's (dz, gn_partial) for the same inputs."""
    dev = _Device(c)
    dz, part, _, _ = dev.backward(L.ACT_ELU, True)
    with mednet_hip.precision(c.mode):
        conv = hnn.Conv3d(32, c.m, 1, planar_output=True).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(c.W[:, :, None, None, None])
            conv.bias.copy_(c.b)
        leaf = dev.z.clone().requires_grad_(True)
        hook, box = ops.GN3Hook(), {}
        hook.gn_in, hook.act = dev.gy, L.ACT_ELU
        x = _Producer.apply(leaf, hook, box)
        x._mednet_gn3 = hook
        assert ops._gn3_hook_of(x, x.dtype) is hook
        taken = ops.GN3_COUNT["taken"]
        loss = call(dev, conv, x)
        (loss * c.gscale).backward()
        torch.cuda.synchronize()
    assert ops.GN3_COUNT["taken"] == taken + 1, "the hook declined the head's gradient"
    assert box["partial"] is not None and box["partial"].dtype == torch.float32
    assert not bool(torch.isnan(box["partial"]).any())
    assert torch.equal(box["partial"], part), "ops delivers other GroupNorm sums than the ABI call wrote"
    assert torch.equal(box["dout"], dz) and torch.equal(leaf.grad, dz)
    assert hook.partial is None and hook.dx is None


@pytest.mark.parametrize("mode", B_MODES)
def test_head_seg_hands_its_groupnorm_sums_to_the_hook(mode):
    c = head_case("seg", mode, 3, (12, 10, 6), (9, "DICE", False, 2), "elu")
    _deliver(c, lambda dev, conv, x: ops.head_seg(x, conv.weight, conv.bias, conv._packed(), dev.lab, dev.cw, 1e-5, False, 2, "DICE")[1])


@pytest.mark.parametrize("mode", B_MODES)
def test_head_landmark_hands_its_groupnorm_sums_to_the_hook(mode):
    c = head_case("lm", mode, 3, (12, 10, 6), (5, 3, "CE", "L2", False, 2), "elu")

    def call(dev, conv, x):
        closs, rloss = ops.head_landmark(x, conv.weight, conv.bias, conv._packed(), dev.hm, dev.lab, dev.cw, dev.rw, "L2", 1e-5, False, 2, "CE")
        return closs + rloss
    _deliver(c, call)
