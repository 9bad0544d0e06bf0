"""BatchNorm3d of the 'b' layer orders (components.py:58-63) on the GPU: the mednet_bn_* kernels through ops.batch_norm_act
against torch.nn.functional.batch_norm in fp64, the module in both modes, the fused backward forms, whole networks against the
CPU oracle, the graphed training step and grid prediction."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import nn as hnn
from mednet_hip import ops as hops
from mednet_hip import predict as HP
from mednet_hip.unet import components as HC
from mednet_hip.unet import loss as HL
from mednet_hip.unet import model as HM
from oracle import ref_cpu as O
from oracle import ref_predict as P

from gpu_util import DEV, TOL, assert_close, half_round, rel, rnd
from test_gpu_network import NET_TOL

pytestmark = pytest.mark.gpu

MODES = ["fp32", "bf16", "fp16"]
_ACTS = {"none": (L.ACT_NONE, lambda u: u), "relu": (L.ACT_RELU, F.relu), "leaky": (L.ACT_LEAKY, lambda u: F.leaky_relu(u, 0.1)),
         "elu": (L.ACT_ELU, F.elu)}
CBE = dict(in_channels=1, out_channels=3, final_sigmoid=False, f_maps=[16, 32, 64], conv_layer_order="cbe")
CBR = dict(in_channels=1, out_channels=3, final_sigmoid=False, f_maps=[16, 32, 64], layer_order="cbr")


def _no_aten_batch_norm(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("ATen's batch norm was called")
    for mod, name in ((torch, "batch_norm"), (F, "batch_norm"), (torch, "native_batch_norm")):
        monkeypatch.setattr(mod, name, boom)


# ---------------------------------------------------------------------------------------------- 2: nothing of ATen runs
@pytest.mark.parametrize("order", ["cbe", "cbr", "bcr", "cbl"])
def test_b_orders_run_no_aten_batch_norm_and_stay_16_bit_channels_last(order, monkeypatch):
    _no_aten_batch_norm(monkeypatch)
    seen = []
    x = half_round(rnd("bnaten" + order, 2, 16, 6, 10, 12), "bf16")
    with mednet_hip.precision("bf16"):
        net = O.keyed_init_(HC.SingleConv(16, 32, 3, order, 8)).to(DEV)
        assert isinstance(net.batchnorm, hnn.BatchNorm3d)
        net.batchnorm.register_forward_hook(lambda m, args, out: seen.append((args[0], out)))
        xg = x.to(DEV).bfloat16().contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
        y = net(xg)
        (y.float() * y.float()).sum().backward()
        torch.cuda.synchronize()
    assert len(seen) == 1
    for t in seen[0]:
        assert t.dtype == torch.bfloat16 and t.is_contiguous(memory_format=torch.channels_last_3d), (t.dtype, t.stride())
    assert xg.grad is not None and all(p.grad is not None for p in net.parameters())
    assert int(net.batchnorm.num_batches_tracked) == 1


# ---------------------------------------------------------------------------------------------- 3: kernel parity
def _bn_ref(x, gamma, beta, rm, rv, training, act, r):
    """fp64 reference on the CPU; rm / rv (fp64) are updated in place when training."""
    u = F.batch_norm(x, rm, rv, gamma, beta, training, 0.1, 1e-5)
    if r is not None:
        u = u + r
    return _ACTS[act][1](u)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,c,shape,act,res", [
    (2, 1, (5, 6, 7), "relu", False), (3, 4, (9, 11, 21), "leaky", True), (1, 16, (6, 10, 12), "elu", False),
    (2, 32, (8, 8, 8), "none", True), (3, 48, (5, 6, 7), "elu", True), (2, 256, (2, 3, 4), "relu", False),
    (2, 32, (9, 11, 21), "none", False), (3, 16, (7, 9, 11), "relu", True), (1, 4, (5, 6, 7), "leaky", False),
    (4, 32, (64, 64, 64), "elu", False)])
def test_batch_norm_act_against_fp64(mode, n, c, shape, act, res):
    """z, dx, dresidual, dgamma, dbeta, the running statistics after one and after three training steps and the batch counter,
    at the bounds the GroupNorm kernels are held to (the same arithmetic and rounding points)."""
    tag = f"bn{n}{c}{shape}{act}{res}"
    tol = TOL[mode]
    xs = [half_round(rnd(tag + f"x{i}", n, c, *shape, scale=2.0 - 0.5 * i) + 0.5 * (i + 1), mode) for i in range(3)]
    r, cot = half_round(rnd(tag + "r", n, c, *shape), mode), half_round(rnd(tag + "g", n, c, *shape), mode)
    gamma, beta = rnd(tag + "ga", c) * 0.3 + 1.0, rnd(tag + "be", c) * 0.3
    rm0, rv0 = rnd(tag + "rm", c) * 0.2, rnd(tag + "rv", c).abs() + 0.5
    # reference
    xr, rr = xs[0].double().requires_grad_(True), r.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm, rv = rm0.double().clone(), rv0.double().clone()
    zr = _bn_ref(xr, gr, br, rm, rv, True, act, rr if res else None)
    (zr * cot.double()).sum().backward()
    rm1, rv1 = rm.clone(), rv.clone()
    with torch.no_grad():
        for i in (1, 2):
            _bn_ref(xs[i].double(), gr, br, rm, rv, True, act, rr if res else None)
    with mednet_hip.precision(mode):
        dt = mednet_hip.config.act_dtype()
        g_rm, g_rv = rm0.clone().to(DEV), rv0.clone().to(DEV)
        nbt = torch.zeros((), dtype=torch.int64, device=DEV)
        gg, bg = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
        xg = xs[0].to(DEV).to(dt).requires_grad_(True)
        rg = r.to(DEV).to(dt).requires_grad_(True)
        z = hops.batch_norm_act(xg, gg, bg, g_rm, g_rv, nbt, True, 0.1, 1e-5, _ACTS[act][0], rg if res else None)
        (z.float() * cot.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        got1 = (g_rm.clone(), g_rv.clone(), int(nbt))
        with torch.no_grad():
            for i in (1, 2):
                hops.batch_norm_act(xs[i].to(DEV).to(dt), gg, bg, g_rm, g_rv, nbt, True, 0.1, 1e-5, _ACTS[act][0], rg if res else None)
        torch.cuda.synchronize()
    figures = {"z": rel(z, zr), "dx": rel(xg.grad, xr.grad), "dgamma": rel(gg.grad, gr.grad), "dbeta": rel(bg.grad, br.grad),
               "running_mean@1": rel(got1[0], rm1), "running_var@1": rel(got1[1], rv1), "running_mean@3": rel(g_rm, rm),
               "running_var@3": rel(g_rv, rv)}
    if res:
        figures["dres"] = rel(rg.grad, rr.grad)
    print(f"[bn parity] {mode} {tag}: " + " ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    assert z.dtype == dt and z.is_contiguous(memory_format=torch.channels_last_3d)
    for k, v in figures.items():
        assert v <= tol, f"{k}: rel-L2 {v:.3e} > {tol:.1e}"
    assert got1[2] == 1 and int(nbt) == 3


@pytest.mark.parametrize("mode", MODES)
def test_batch_norm_equals_group_norm_over_the_flattened_batch(mode):
    """Training-mode BatchNorm is GroupNorm with n = 1, spatial = N * S, groups = C on the channels-last batch: the new
    cross-sample kernels against the existing entry points (same first passes, another reduction order)."""
    n, c, shape = 3, 32, (9, 11, 21)
    x, cot = half_round(rnd("bngnx", n, c, *shape, scale=2.0) + 0.5, mode), half_round(rnd("bngng", n, c, *shape), mode)
    gamma, beta = rnd("bngnga", c) * 0.3 + 1.0, rnd("bngnbe", c) * 0.3

    def flat(t):  # [N, C, D, H, W] channels-last -> [1, C, N*S, 1, 1] channels-last: the same memory
        return t.permute(0, 2, 3, 4, 1).reshape(1, -1, 1, 1, c).permute(0, 4, 1, 2, 3)

    out = {}
    with mednet_hip.precision(mode):
        dt = mednet_hip.config.act_dtype()
        for kind in ("bn", "gn"):
            gg, bg = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
            xg = x.to(DEV).to(dt).contiguous(memory_format=torch.channels_last_3d)
            cg = cot.to(DEV).contiguous(memory_format=torch.channels_last_3d)
            if kind == "gn":
                xg, cg = flat(xg), flat(cg)
                assert xg.is_contiguous(memory_format=torch.channels_last_3d)
            xg = xg.detach().requires_grad_(True)
            if kind == "bn":
                z = hops.batch_norm_act(xg, gg, bg, None, None, None, True, 0.1, 1e-5, L.ACT_ELU)
            else:
                z = hops.group_norm_act(xg, gg, bg, c, 1e-5, L.ACT_ELU)
            (z.float() * cg).sum().backward()
            out[kind] = [t.detach().float().reshape(-1)  # (memory order [N * S][C] in both forms)
                         for t in (z.permute(0, 2, 3, 4, 1), xg.grad.permute(0, 2, 3, 4, 1), gg.grad, bg.grad)]
    for k, a, b in zip(("z", "dx", "dgamma", "dbeta"), out["bn"], out["gn"]):
        assert_close(a, b, TOL[mode], f"BatchNorm vs GroupNorm(n=1) {k}")


# ---------------------------------------------------------------------------------------------- 4: evaluation mode
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,c,shape,act,res", [(2, 32, (8, 8, 8), "elu", True), (3, 4, (5, 6, 7), "relu", False),
                                               (2, 48, (4, 6, 5), "none", False), (1, 1, (9, 11, 21), "leaky", False)])
def test_eval_mode_uses_running_statistics(mode, n, c, shape, act, res, monkeypatch):
    tag = f"bnev{n}{c}{act}"
    tol = TOL[mode]
    x, r, cot = (half_round(t, mode) for t in (rnd(tag + "x", n, c, *shape, scale=2.0) + 0.5, rnd(tag + "r", n, c, *shape),
                                               rnd(tag + "g", n, c, *shape)))
    gamma, beta = rnd(tag + "ga", c) * 0.3 + 1.0, rnd(tag + "be", c) * 0.3
    rm0, rv0 = rnd(tag + "rm", c) * 0.4 + 0.3, rnd(tag + "rv", c).abs() + 0.5
    xr, rr = x.double().requires_grad_(True), r.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    zr = _bn_ref(xr, gr, br, rm0.double(), rv0.double(), False, act, rr if res else None)
    (zr * cot.double()).sum().backward()  # frozen BatchNorm: autograd through the plain affine
    _no_aten_batch_norm(monkeypatch)
    with mednet_hip.precision(mode):
        dt = mednet_hip.config.act_dtype()
        bn = hnn.BatchNorm3d(c).to(DEV)
        with torch.no_grad():
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
            bn.running_mean.copy_(rm0)
            bn.running_var.copy_(rv0)
            bn.num_batches_tracked.fill_(7)
        bn.eval()
        xg, rg = x.to(DEV).to(dt).requires_grad_(True), r.to(DEV).to(dt).requires_grad_(True)
        z = bn(xg, act=_ACTS[act][0], residual=rg if res else None)
        (z.float() * cot.to(DEV)).sum().backward()
        with torch.no_grad():
            z2 = bn(xg.detach(), act=_ACTS[act][0], residual=rg.detach() if res else None)
        torch.cuda.synchronize()
    assert torch.equal(z, z2)
    assert torch.equal(bn.running_mean.cpu(), rm0) and torch.equal(bn.running_var.cpu(), rv0) and int(bn.num_batches_tracked) == 7
    assert_close(z, zr, tol, "eval z")
    assert_close(xg.grad, xr.grad, tol, "eval dx")
    assert_close(bn.weight.grad, gr.grad, tol, "eval dgamma")
    assert_close(bn.bias.grad, br.grad, tol, "eval dbeta")
    if res:
        assert_close(rg.grad, rr.grad, tol, "eval dres")


def test_untracked_statistics_use_the_batch_in_both_modes():
    x = rnd("bnuntracked", 2, 8, 5, 6, 7, scale=2.0) + 0.5
    want = F.batch_norm(x.double(), None, None, None, None, True, 0.1, 1e-5)
    with mednet_hip.precision("fp32"):
        bn = hnn.BatchNorm3d(8, affine=False, track_running_stats=False).to(DEV)
        for train in (True, False):
            bn.train(train)
            assert_close(bn(x.to(DEV)), want, TOL["fp32"], f"train={train}")


# ---------------------------------------------------------------------------------------------- 5: fused backward forms
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("order,cin,cout,shape", [("bcr", 32, 32, (16, 24, 32)), ("bcr", 96, 32, (9, 11, 21)), ("bcl", 32, 64, (8, 8, 16)),
                                                  ("bce", 64, 64, (8, 16, 16)), ("cbr", 32, 32, (16, 24, 32))])
def test_batchnorm_backward_sums_from_the_following_conv(mode, order, cin, cout, shape):
    """Two SingleConv layers in a row, N = 3.  'b c .': both BatchNorm backward passes take {sum du, sum du * x} from the conv data
    gradient's epilogue (ops.GNBHook), summed over rows and samples by mednet_bn_act_bwd_fused; 'c b r': the first layer's
    BatchNorm + ReLU feeds the second conv (one pass taken).  Against the stand-alone passes."""
    x = torch.from_numpy(O._rng(f"bnb2{order}{cin}{shape}").standard_normal((3, cin) + shape).astype(np.float32))
    res = {}
    want_taken = 1 if order == "cbr" else 2
    for fused in (True, False):
        old = hops.FUSE_GN3
        hops.FUSE_GN3 = fused
        before = dict(hops.GN3_COUNT)
        try:
            with mednet_hip.precision(mode):
                net = nn.Sequential(O.keyed_init_(HC.SingleConv(cin, cout, 3, order, 8)), O.keyed_init_(HC.SingleConv(cout, cout, 3, order, 8))).to(DEV)
                xg = x.to(DEV).to(torch.bfloat16 if mode == "bf16" else torch.float16).requires_grad_(True)
                y = net(xg)
                cot = torch.from_numpy(O._rng("bnb2c").standard_normal(tuple(y.shape)).astype(np.float32)).to(DEV)
                (y.float() * cot).sum().backward()
                res[fused] = [xg.grad.float().clone()] + [p.grad.clone() for p in net.parameters()]
        finally:
            hops.FUSE_GN3 = old
        taken = hops.GN3_COUNT["taken"] - before["taken"]
        assert taken == (want_taken if fused else 0), f"fused={fused}: {taken} BatchNorm backward passes took the conv's sums"
        masked = hops.GN3_COUNT["masked"] - before.get("masked", 0)
        assert masked == (1 if fused and order == "bcr" else 0), f"fused={fused}: {masked} activation-backward passes were folded away"
    names = ["dx"] + [k for k, _ in net.named_parameters()]
    for k, a, b in zip(names, res[True], res[False]):
        assert_close(a, b, 4e-3 if mode == "bf16" else 1e-3, f"fused vs stand-alone {k}")


# ---------------------------------------------------------------------------------------------- 6, 9: networks against the oracle
def _oracle_run(cls, ctor, batch, dtype):
    ora = O.keyed_init_(cls(**ctor)).to(dtype)
    lo = ora(batch["data"].to(dtype))
    loss = O.DiceLoss()(lo, batch["label"][:, -1].long())
    loss.backward()
    return ora, lo, loss


def _hip_run(cls, ctor, batch, mode):
    with mednet_hip.precision(mode):
        net = O.keyed_init_(cls(**ctor)).to(DEV)
        lg = net(batch["data"].to(DEV))
        loss = HL.DiceLoss().to(DEV)(lg, batch["label"][:, -1].long().to(DEV))
        loss.backward()
        torch.cuda.synchronize()
    return net, lg, loss


@pytest.mark.parametrize("kind", ["res_cbe", "unet_cbr"])
def test_b_networks_against_the_oracle_fp32(kind, monkeypatch):
    ocls, hcls, ctor = (O.ResidualUNet3D, HM.ResidualUNet3D, CBE) if kind == "res_cbe" else (O.UNet3D, HM.UNet3D, CBR)
    batch = O.synthetic_batch(2, 1, (32, 32, 32), 3, 0, seed=5)
    ora, lo, loss_o = _oracle_run(ocls, ctor, batch, torch.float32)
    ora64, _, _ = _oracle_run(ocls, ctor, batch, torch.float64)
    cond = {k: max(1.0, rel(p.grad, q.grad) / 1e-6) for (k, p), (_, q) in zip(ora.named_parameters(), ora64.named_parameters())}
    _no_aten_batch_norm(monkeypatch)
    net, lg, loss_g = _hip_run(hcls, ctor, batch, "fp32")
    tl, tg = NET_TOL["fp32"]
    rl = rel(lg, lo)
    worst = max((rel(p.grad, q.grad) / cond[k], k) for (k, p), (_, q) in zip(net.named_parameters(), ora.named_parameters()))
    bufs = max(rel(a, b) for (_, a), (_, b) in zip(net.named_buffers(), ora.named_buffers()) if a.dtype.is_floating_point)
    print(f"[bn nets] {kind} fp32: logits {rl:.2e} worst gradient / cond {worst[0]:.2e} ({worst[1]}) running buffers {bufs:.2e} "
          f"loss {float(loss_g.detach()):.6f} (oracle {float(loss_o.detach()):.6f})")
    assert rl <= tl, f"logits rel-L2 {rl:.3e}"
    for (k, p), (_, q) in zip(net.named_parameters(), ora.named_parameters()):
        r = rel(p.grad, q.grad)
        assert r <= tg * cond[k], f"grad {k}: rel-L2 {r:.3e} (cond {cond[k]:.1f})"
    assert bufs <= tl, f"running buffers rel-L2 {bufs:.3e}"
    for (k, a), (_, b) in zip(net.named_buffers(), ora.named_buffers()):
        if not a.dtype.is_floating_point:
            assert int(a) == int(b) == 1, k


def test_cbe_network_bf16_within_the_references_own_drift(monkeypatch):
    """bf16 storage against the fp64 oracle; the yardstick is the reference's own bf16 drift computed here (oracle with
    .bfloat16() parameters and input against the fp64 oracle): within max(NET_TOL["bf16"], 1.5 x drift).  The same step run
    twice gives the same bits (gradients and buffers)."""
    batch = O.synthetic_batch(2, 1, (32, 32, 32), 3, 0, seed=5)
    ora64, l64, _ = _oracle_run(O.ResidualUNet3D, CBE, batch, torch.float64)
    ora16, l16, _ = _oracle_run(O.ResidualUNet3D, CBE, batch, torch.bfloat16)
    drift_l = rel(l16, l64)
    drift_g = max(rel(p.grad, q.grad) for p, q in zip(ora16.parameters(), ora64.parameters()))
    _no_aten_batch_norm(monkeypatch)
    net, lg, _ = _hip_run(HM.ResidualUNet3D, CBE, batch, "bf16")
    rl = rel(lg, l64)
    worst = max((rel(p.grad, q.grad), k) for (k, p), (_, q) in zip(net.named_parameters(), ora64.named_parameters()))
    bufs = max(rel(a, b) for (_, a), (_, b) in zip(net.named_buffers(), ora64.named_buffers()) if a.dtype.is_floating_point)
    tl, tg = max(NET_TOL["bf16"][0], 1.5 * drift_l), max(NET_TOL["bf16"][1], 1.5 * drift_g)
    print(f"[bn nets] res_cbe bf16: logits {rl:.2e} (reference's bf16 drift {drift_l:.2e}, bound {tl:.2e}) worst gradient {worst[0]:.2e} "
          f"({worst[1]}; drift {drift_g:.2e}, bound {tg:.2e}) running buffers {bufs:.2e}")
    assert rl <= tl and worst[0] <= tg and bufs <= tl, (rl, tl, worst, tg, bufs)
    net2, lg2, _ = _hip_run(HM.ResidualUNet3D, CBE, batch, "bf16")
    assert torch.equal(lg, lg2)
    for (k, p), (_, q) in zip(net.named_parameters(), net2.named_parameters()):
        assert torch.equal(p.grad, q.grad), f"gradient {k} differs between two runs"
    for (k, a), (_, b) in zip(net.named_buffers(), net2.named_buffers()):
        assert torch.equal(a, b), f"buffer {k} differs between two runs"


# ---------------------------------------------------------------------------------------------- 7: training step, graph
def _train(order, graph, batches):
    from mednet_hip.train import SegmentationStep
    ctor = dict(CBE, conv_layer_order=order)
    with mednet_hip.precision("fp32"):
        net = O.keyed_init_(HM.ResidualUNet3D(**ctor)).to(DEV)
        step = SegmentationStep(net, lr=1e-3, graph=graph)
        losses = [float(step({k: v.to(DEV) for k, v in b.items()})) for b in batches]
        torch.cuda.synchronize()
        state = {k: v.detach().clone().cpu() for k, v in net.state_dict().items()}
        step.flat.release()
    return losses, state


def test_training_step_graphed_and_eager_and_against_the_oracle():
    """Five Adam steps of SegmentationStep on the 'cbe' network: captured graph (two eager warm-up calls, then capture + replay)
    against the eager step -- the running statistics and the batch counter are updated INSIDE the graph --, and the losses against
    the oracle + torch.optim.Adam."""
    batches = [O.synthetic_batch(2, 1, (32, 32, 32), 3, 0, seed=5 + i) for i in range(5)]
    # is the step bit-reproducible between its two forms for the GroupNorm network of this size?  Then BatchNorm must be too.
    gn = [_train("cge", g, batches) for g in (False, True)]
    gn_exact = gn[0][0] == gn[1][0] and all(torch.equal(gn[0][1][k], gn[1][1][k]) for k in gn[0][1])
    (l_e, s_e), (l_g, s_g) = (_train("cbe", g, batches) for g in (False, True))
    worst = max(rel(s_g[k], s_e[k]) for k in s_e if s_e[k].dtype.is_floating_point)
    print(f"[bn step] GroupNorm net graph == eager bitwise: {gn_exact}; 'cbe' losses eager {l_e} graph {l_g}; worst state rel-L2 {worst:.2e}")
    assert int(s_e["encoders.0.basic_module.conv1.batchnorm.num_batches_tracked"]) == 5
    for k in s_e:
        if k.endswith("num_batches_tracked"):
            assert int(s_e[k]) == int(s_g[k]) == 5, k
        elif gn_exact:
            assert torch.equal(s_e[k], s_g[k]), f"{k}: graph and eager differ"
        else:
            assert rel(s_g[k], s_e[k]) <= 1e-6, k
    if gn_exact:
        assert l_e == l_g
    else:
        assert max(abs(a - b) for a, b in zip(l_e, l_g)) <= 1e-6
    ora = O.keyed_init_(O.ResidualUNet3D(**CBE))
    opt = torch.optim.Adam(ora.parameters(), lr=1e-3)
    for i, b in enumerate(batches):
        opt.zero_grad()
        lo = O.seg_training_step(ora, O.DiceLoss(), b)
        lo.backward()
        opt.step()
        assert abs(l_e[i] - float(lo)) <= 2e-4, (i, l_e[i], float(lo))


# ---------------------------------------------------------------------------------------------- 8: inference
def test_grid_predictor_on_an_eval_cbe_network_equals_the_oracle(monkeypatch):
    ora = O.keyed_init_(O.ResidualUNet3D(**CBE))
    opt = torch.optim.Adam(ora.parameters(), lr=1e-3)
    for seed in (5, 6, 7):
        opt.zero_grad()
        O.seg_training_step(ora, O.DiceLoss(), O.synthetic_batch(2, 1, (32, 32, 32), 3, 0, seed=seed)).backward()
        opt.step()
    ora.eval()
    rmean = ora.encoders[0].basic_module.conv1.batchnorm.running_mean
    assert float(rmean.abs().max()) > 0 and int(ora.encoders[0].basic_module.conv1.batchnorm.num_batches_tracked) == 3
    img = O.synthetic_batch(1, 1, (48, 40, 56), 3, 0, seed=11)["data"][0].numpy()
    patch, ov = [32, 32, 32], [4, 4, 4]

    def fwd(x):  # channel 0 (a "heat map", clipped to uint8 by the post-processing): 255 where the two largest probabilities tie
        with torch.no_grad():
            lg = ora(torch.from_numpy(x))
        top = torch.softmax(lg, dim=1).topk(2, dim=1).values
        near = ((top[:, 0] - top[:, 1]) < 1e-3).float()[:, None] * 255.0
        return torch.cat([near, lg], dim=1).numpy()

    want = P.predict_volume(fwd, img, patch, ov, 1, batch_size=2, pad_kwargs={"mode": "symmetric"})
    _no_aten_batch_norm(monkeypatch)
    with mednet_hip.precision("fp32"):
        net = HM.ResidualUNet3D(**CBE)
        net.load_state_dict(ora.state_dict())
        net = net.to(DEV)
        before = {k: v.clone() for k, v in net.state_dict().items()}
        got = HP.GridPredictor(net, patch, ov, num_heatmaps=0, pad_mode="symmetric", batch_size=2)(img).cpu().numpy()
        for k, v in net.state_dict().items():
            assert torch.equal(v, before[k]), f"{k} changed during prediction"
    exempt = want[0] != 0
    differ = got[0] != want[1]
    print(f"[bn predict] voxels that differ {differ.mean():.4%}, exempted (oracle's top two within 1e-3) {exempt.mean():.4%}")
    assert got.shape == (1,) + img.shape[1:] and got.dtype == np.uint8
    assert exempt.mean() < 0.01
    assert not (differ & ~exempt).any(), f"{int((differ & ~exempt).sum())} label voxels differ away from ties"

