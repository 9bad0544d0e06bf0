"""The deep-supervision node at operator level (csrc/ds_head.hip through ops.ds_head) on the MI355X (-m gpu): the exact label pick,
per-element bounds against the fp64 restatement of tests/ds_util.py, the junction's one rounding, the footprint under guard bands,
repeatability and the refusals of the C ABI.  profiles/deep_supervision_bounds.md derives the bounds and records the measured values."""
import functools
import math

import numpy as np
import pytest
import torch

import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import config
from mednet_hip import nn as hnn
from mednet_hip import ops

import ds_util as U
from fence import Fence
from gpu_util import DEV, EPS_FLOOR, half_round, rnd

pytestmark = pytest.mark.gpu
MODES = ["bf16", "fp16", "fp16x2"]
KINDS = ["DICE", "CE", "DICE_CE"]
N = 2
# (level extents, shift, cin, ncls): one 128-voxel run (4 x 4 x 8), a ragged last run of 216 voxels (6 x 6 x 6), more than one
# workgroup per sample (24 x 24 x 16 = 72 runs: more than 64, five workgroups of 16 runs, the last with 8); every cin path (2, 4 and 8 tiles: the 4- and the 8-tile instantiation) and every
# class count; shift 3 runs at 4 x 4 x 8 (a 32 x 32 x 64 label volume), where the level still fills a run.
CASES = [((4, 4, 8), 1, 64, 1), ((4, 4, 8), 2, 128, 2), ((4, 4, 8), 3, 256, 4), ((6, 6, 6), 1, 64, 5), ((6, 6, 6), 1, 256, 8),
         ((6, 6, 6), 1, 128, 16), ((24, 24, 16), 1, 64, 16), ((4, 4, 8), 1, 256, 16), ((4, 4, 8), 2, 64, 8)]
# dloss.  fp16 stores the feature gradient and the 16-bit-pair image of dl: scaled as train.LossScaler does (tests/test_gpu_seg_heads.py)
GSCALE = {"bf16": 3.0, "fp16": 3.0 * 16384.0, "fp16x2": 3.0 * 16384.0}
LOSS_FLOOR = 2e-6        # the fused heads' loss against the unfused launches (tests/test_gpu_seg_heads.py), relative above 1
E_SHAPE, E_WORKSPACE, E_UNSUPPORTED = -1, -3, -5


def _weights(c):
    return torch.tensor([0.05] + [0.6 + 0.1 * (k % 7) for k in range(1, c)])


@functools.lru_cache(maxsize=None)
def _inputs(mode, lev, s, cin, ncls):
    tag = f"dsh{lev}{s}{cin}{ncls}"
    full = tuple(v << s for v in lev)
    z = half_round(rnd(tag + "z", N, cin, *lev), "bf16" if mode == "bf16" else "fp16")
    W, b = rnd(tag + "w", ncls, cin, 1, 1, 1, scale=1.0 / math.sqrt(cin)), rnd(tag + "b", ncls)
    d_pass = half_round(rnd(tag + "p", N, cin, *lev, scale=1e-3 * GSCALE[mode]), "bf16" if mode == "bf16" else "fp16")
    return z, W, b, U.random_labels(N, full, ncls), d_pass


@functools.lru_cache(maxsize=None)
def _reference(mode, lev, s, cin, ncls, kind, with_pass):
    """Computed once per case and shared (fp64 on the CPU)."""
    z, W, b, vol, d_pass = _inputs(mode, lev, s, cin, ncls)
    return U.head_ref(z, W, b, vol[:, -1], s, kind, _weights(ncls), d_pass if with_pass else None, GSCALE[mode], mode)


def _head(cin, ncls, W, b):
    conv = hnn.Conv3d(cin, ncls, 1, planar_output=True).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(W)
        conv.bias.copy_(b)
    return conv


def _run(mode, fused, case, kind, d_pass=None, dloss=None, vol_dev=None, z_dev=None):
    """-> (loss, dx, dW, db) of ops.ds_head, or of the composed form: the head, then the existing loss on the picked labels."""
    lev, s, cin, ncls = case
    z, W, b, vol, _ = _inputs(mode, *case)
    dloss = GSCALE[mode] if dloss is None else dloss
    with mednet_hip.precision(mode):
        conv = _head(cin, ncls, W, b)
        xg = (ops.to_cl(z.to(DEV).to(config.act_dtype())) if z_dev is None else z_dev).requires_grad_(True)
        lab = (vol.to(DEV) if vol_dev is None else vol_dev)[:, -1]   # the last channel of a uint8 volume, where it lies
        wd = _weights(ncls).to(DEV)
        if fused:
            assert ops.ds_head_supported(xg, cin, ncls, lab, s), case
            xp, loss = ops.ds_head(xg, conv.weight, conv.bias, conv._packed(), lab, s, wd, 1e-5, False, None, kind)
            assert xp.data_ptr() == xg.data_ptr()
            outs, grads = [loss], [torch.tensor(dloss, device=DEV)]
            if d_pass is not None:
                outs, grads = [xp] + outs, [d_pass] + grads
            torch.autograd.backward(outs, grads)
        else:
            lg = conv(xg)
            pl = U.pick(lab, s).contiguous()
            loss = (ops.dice_loss(lg, pl.long(), wd, 1e-5, False, None) if kind == "DICE" else
                    ops.cross_entropy(lg, pl.long(), wd, -100) if kind == "CE" else ops.dice_ce_loss(lg, pl, wd, 1e-5))
            (loss * dloss).backward()
        torch.cuda.synchronize()
    return loss.detach(), xg.grad, conv.weight.grad, conv.bias.grad


def _ratios(res, ref, mode, z):
    """The errors of a run in the norms of the bounds: loss absolute; dx beyond the one storage rounding, per sum of absolute terms;
    dW per sum_v |dl| |z|; db per sum_v |dl|."""
    loss, dx, dW, db = res
    dx = dx.double().cpu()
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dW).all()) and bool(torch.isfinite(db).all())
    over = ((dx - ref.join).abs() - U.half_ulp(ref.join, mode) - 2.0 ** -24 * ref.join.abs()).clamp(min=0)
    live = ref.norm > 0
    assert not bool((over[~live] != 0).any())
    nW = torch.einsum("nkdhw,ncdhw->kc", ref.dl.abs(), z.double().abs())
    nb = ref.dl.abs().sum((0, 2, 3, 4))
    eW = (dW.double().cpu().reshape(nW.shape) - ref.dW).abs()
    eb = (db.double().cpu() - ref.db).abs()
    rat = lambda e, nrm: float((e[nrm > 0] / nrm[nrm > 0]).max()) if bool((nrm > 0).any()) else 0.0
    assert not bool((eW[nW == 0] != 0).any()) and not bool((eb[nb == 0] != 0).any())
    return dict(loss=abs(float(loss) - ref.loss), dx=rat(over, ref.norm), dW=rat(eW, nW), db=rat(eb, nb))


def _bounds(composed, ref):
    """Twice the composed path's error against the same fp64 values (the same fp32-level products in another order), never below
    the floors derived in profiles/deep_supervision_bounds.md."""
    return dict(loss=max(LOSS_FLOOR * max(1.0, abs(ref.loss)), 2.0 * composed["loss"]), dx=max(EPS_FLOOR, 2.0 * composed["dx"]),
                dW=max(EPS_FLOOR, 2.0 * composed["dW"]), db=max(EPS_FLOOR, 2.0 * composed["db"]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_loss_and_gradients_against_fp64_per_element(mode, kind):
    for case in CASES:
        z = _inputs(mode, *case)[0]
        ref = _reference(mode, *case, kind, False)
        composed = _ratios(_run(mode, False, case, kind), ref, mode, z)
        fused = _ratios(_run(mode, True, case, kind), ref, mode, z)
        bound = _bounds(composed, ref)
        print(f"[ds head {mode} {kind} {case}] " + " ".join(f"{k}: fused {fused[k]:.2e} composed {composed[k]:.2e} bound {bound[k]:.2e}" for k in fused))
        for k in fused:
            assert fused[k] <= bound[k], (mode, kind, case, k, fused[k], bound[k])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [((6, 6, 6), 1, 128, 5), ((4, 4, 8), 2, 64, 4), ((24, 24, 16), 1, 64, 16)])
def test_the_junction_rounds_once(mode, kind, case):
    d_pass = ops.to_cl(_inputs(mode, *case)[4].to(DEV).to(U.STORE[mode]))
    # dloss = 0: the pass-through gradient comes back bit for bit
    _, dx0, dW0, _ = _run(mode, True, case, kind, d_pass=d_pass, dloss=0.0)
    assert torch.equal(dx0.view(torch.int16), d_pass.view(torch.int16))
    assert not bool(dW0.any())
    # no d_pass = a zero d_pass
    a = _run(mode, True, case, kind)
    b = _run(mode, True, case, kind, d_pass=torch.zeros_like(d_pass))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # both: one rounding of fp64(d_pass) + dz64, plus the head's own bound (from the run without d_pass)
    z = _inputs(mode, *case)[0]
    ref0 = _reference(mode, *case, kind, False)
    eps = _bounds(_ratios(_run(mode, False, case, kind), ref0, mode, z), ref0)["dx"]
    ref = _reference(mode, *case, kind, True)
    _, dx, dW, db = _run(mode, True, case, kind, d_pass=d_pass)
    worst = U.check_join(dx, ref, mode, eps, f"junction {mode} {kind} {case}")
    print(f"[ds junction {mode} {kind} {case}] beyond half an ulp: {worst:.2e} of the sum of |terms| (bound {eps:.2e})")
    assert torch.equal(dW, a[2]) and torch.equal(db, a[3])   # the head's own gradients do not see d_pass
    assert L.lib().mednet_ds_head_gn_rows(*case[0], case[2], L.dt(dx)) == 0   # (rows > 0 would be checked here as test_gpu_head_backward does)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("ncls", [2, 4, 8, 16])
@pytest.mark.parametrize("lev,s,cin", [((4, 4, 8), 1, 64), ((4, 4, 8), 2, 128), ((4, 4, 8), 3, 256), ((6, 6, 6), 1, 64), ((24, 24, 16), 1, 64)])
def test_exact_label_pick(mode, ncls, lev, s, cin):
    """Zero features and weights, equal biases: p = 1 / ncls exactly, every fp32 partial sum is exact in any order, and every
    position a wrong pick would read holds an out-of-range class (which poisons the sums with NaN).  Dice: the sums equal
    I_k = V / ncls^2, D_k = 2 V / ncls and the loss 1 - 1 / ncls bit for bit (each step of the finalize kernel is exact on these
    values, so its fp32 result IS the fp64 value rounded to fp32).  Cross-entropy: sum w_y = V bit for bit; the loss is log(ncls) up to
    the fp32 evaluation of logf and at most 16 accumulations per lane: 32 * 2^-24 relative (to 1/4 + log ncls, the size of lse)."""
    vol = U.exact_pick_labels(N, lev, s, ncls).to(DEV)
    V = N * lev[0] * lev[1] * lev[2]
    with mednet_hip.precision(mode):
        conv = _head(cin, ncls, torch.zeros(ncls, cin, 1, 1, 1), torch.full((ncls,), 0.25))
        x = ops.to_cl(torch.zeros(N, cin, *lev, device=DEV, dtype=config.act_dtype()))
        for kind in ("DICE", "CE"):
            _, loss = ops.ds_head(x.clone().requires_grad_(True), conv.weight, conv.bias, conv._packed(), vol[:, -1], s, None, 1e-5, False, None, kind)
            saved = loss.grad_fn.saved_tensors[4].cpu()
            got = np.float32(loss.detach().cpu().numpy())
            if kind == "DICE":
                want = torch.tensor([[V / ncls ** 2, 2.0 * V / ncls]] * ncls, dtype=torch.float32)
                assert torch.equal(saved, want), (kind, saved, want)
                assert got == np.float32(np.float64(1.0) - 1.0 / ncls), (got, 1.0 - 1.0 / ncls)
            else:
                assert float(saved.flatten()[0]) == float(V)
                assert abs(float(got) - math.log(ncls)) <= 32 * 2.0 ** -24 * (0.25 + math.log(ncls)), (got, math.log(ncls))


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("kind", KINDS)
def test_footprint_under_guard_bands(mode, kind):
    """The label volume ends at the guard band (the labels are its last channel, the last sample's last voxel its last byte), every
    workspace is exactly mednet_ds_head_ws_bytes, no guard byte changes and the result equals the unfenced run bit for bit."""
    case = ((6, 6, 6), 1, 128, 5)
    lev, s, cin, ncls = case
    z, W, b, vol, dp = _inputs(mode, *case)
    d_pass = ops.to_cl(dp.to(DEV).to(U.STORE[mode]))
    plain = _run(mode, True, case, kind, d_pass=d_pass)
    with Fence() as fence:
        fvol = fence.put(vol.to(DEV))
        fz = fence.put(ops.to_cl(z.to(DEV).to(U.STORE[mode])))
        fenced = _run(mode, True, case, kind, d_pass=fence.put(d_pass), vol_dev=fvol, z_dev=fz)
        fence.check()
        assert fence.owns(fenced[1]) and fence.owns(fenced[0])
        want = L.lib().mednet_ds_head_ws_bytes(N, *lev, cin, ncls)
        mine = [r for r in fence.ws_requests if r[2] in ("forward", "backward", "__init__")]
        assert len(mine) >= 2 and all(asked == served == want for asked, served, _ in mine), (fence.ws_requests, want)
    for x, y in zip(plain, fenced):
        assert torch.equal(x, y)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_two_runs_are_bit_equal(mode):
    for case in (((24, 24, 16), 1, 64, 16), ((6, 6, 6), 1, 256, 8)):
        d_pass = ops.to_cl(_inputs(mode, *case)[4].to(DEV).to(U.STORE[mode]))
        a = _run(mode, True, case, "DICE_CE", d_pass=d_pass)
        b = _run(mode, True, case, "DICE_CE", d_pass=d_pass)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_refusals_are_held_to_their_error_codes():
    lib = L.lib()
    n, (d, h, w), s, cin, ncls = 2, (4, 4, 8), 1, 64, 4
    D, H, W = d << s, h << s, w << s
    with mednet_hip.precision("bf16"):
        conv = _head(cin, ncls, torch.zeros(ncls, cin, 1, 1, 1), torch.zeros(ncls))
        packed = conv._packed()
    z = torch.zeros(n, d * h * w, cin, dtype=torch.bfloat16, device=DEV)
    lab = torch.zeros(n, D, H, W, dtype=torch.uint8, device=DEV)
    loss, saved = torch.zeros((), device=DEV), torch.zeros(ncls, 2, device=DEV)
    dl, dz, dw, db = torch.ones((), device=DEV), torch.empty_like(z), torch.zeros(ncls, cin, device=DEV), torch.zeros(ncls, device=DEV)
    need = lib.mednet_ds_head_ws_bytes(n, d, h, w, cin, ncls)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def fwd(label_dt=L.U8, dims=(d, h, w), full=(D, H, W), shift=s, dt=L.BF16, nbytes=need, kind=L.CLASS_DICE, sig=0, ign=L.NO_IGNORE):
        return lib.mednet_ds_head_fwd(z.data_ptr(), packed.data_ptr(), conv.bias.data_ptr(), lab.data_ptr(), label_dt, D * H * W, None,
                                      loss.data_ptr(), saved.data_ptr(), n, *dims, *full, shift, cin, ncls, kind, 1e-5, sig, ign, dt,
                                      ws.data_ptr(), nbytes, L.stream())

    def bwd(gn_y=None, gn_partial=None, shift=s, full=(D, H, W), dt=L.BF16, nbytes=need, label_dt=L.U8):
        return lib.mednet_ds_head_bwd(z.data_ptr(), packed.data_ptr(), conv.bias.data_ptr(), lab.data_ptr(), label_dt, D * H * W, None,
                                      saved.data_ptr(), dl.data_ptr(), None, dz.data_ptr(), gn_y, 0, gn_partial, dw.data_ptr(), db.data_ptr(),
                                      n, d, h, w, *full, shift, cin, ncls, L.CLASS_DICE, 1e-5, 0, L.NO_IGNORE, dt, ws.data_ptr(), nbytes,
                                      L.stream())

    assert fwd() == 0 and bwd() == 0
    for call in (fwd, bwd):
        assert call(shift=0) == E_UNSUPPORTED and call(shift=4) == E_UNSUPPORTED
        assert call(full=(D + 2, H, W)) == E_SHAPE and call(full=(D, H - 2, W)) == E_SHAPE   # D >> s != d
        assert call(label_dt=L.I64) == E_UNSUPPORTED
        assert call(dt=L.F32) == E_UNSUPPORTED
        assert call(nbytes=need - 1) == E_WORKSPACE
    assert fwd(kind=L.CLASS_CE, sig=1) == E_UNSUPPORTED and fwd(kind=L.CLASS_DICE_CE, ign=2) == E_UNSUPPORTED and fwd(kind=7) == E_UNSUPPORTED
    gn = torch.zeros_like(z)
    part = torch.zeros(n, 1, cin, 2, device=DEV)
    assert bwd(gn_y=gn.data_ptr()) == E_SHAPE and bwd(gn_partial=part.data_ptr()) == E_SHAPE
    if lib.mednet_ds_head_gn_rows(d, h, w, cin, L.BF16) == 0:
        assert bwd(gn_y=gn.data_ptr(), gn_partial=part.data_ptr()) == E_UNSUPPORTED
    try:
        lib.mednet_set_option(b"ds_head_fuse", 0)
        assert fwd() == E_UNSUPPORTED and bwd() == E_UNSUPPORTED
    finally:
        lib.mednet_set_option(b"ds_head_fuse", 1)
    torch.cuda.synchronize()
