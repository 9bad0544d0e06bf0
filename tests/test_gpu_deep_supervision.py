"""Deep supervision at network level on the MI355X (-m gpu): train.SegmentationStep on ResidualUNet3D(deep_supervision=2) against
the live CPU restatement of tests/ds_util.py (the oracle's network with forward hooks on its decoders, nn.Conv3d heads, strided
labels, the oracle's losses), the fused step against the ds_head_fuse=0 step, the GroupNorm-3 bookkeeping, graph capture, and
the unchanged behaviour without the keyword and at inference."""
import functools

import pytest
import torch

import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import ops
from mednet_hip.train import SegmentationStep
from mednet_hip.unet import model as HM
from oracle import ref_cpu as O

import ds_util as U
from gpu_util import DEV, rel
from test_gpu_network import NET_TOL, NET_TOL_BF16_CONCAT

pytestmark = pytest.mark.gpu
K = 2
SHAPE, N = (32, 32, 32), 2
KINDS = ["DICE", "CE", "DICE_CE"]
# 16-bit storage, fused against composed: the two steps differ by storage roundings (one rounding at the junction instead of two,
# another summation order in the heads), so each gradient tensor is held to the bf16 parity bound of tests/test_gpu_network.py
# (per tensor of >= 1024 elements, and concatenated), scaled by the unit roundoff for fp16 storage (2^-11 against 2^-8).
PAIR_TOL = {"bf16": (NET_TOL["bf16"][1], NET_TOL_BF16_CONCAT), "fp16": (NET_TOL["bf16"][1] / 8, NET_TOL_BF16_CONCAT / 8),
            "fp16x2": (NET_TOL["bf16"][1] / 8, NET_TOL_BF16_CONCAT / 8)}


def _ctor(c):
    return dict(in_channels=1, out_channels=c, final_sigmoid=False, f_maps=[32, 64, 128, 256])


def _weights(c):
    return [0.05] + [1.0] * (c - 1)


def _batch(c):
    return O.synthetic_batch(N, 1, SHAPE, c, 0, seed=40 + c)


@functools.lru_cache(maxsize=None)
def _restatement(c, kind, dtype):
    """The CPU restatement, run once per (classes, loss, precision) and shared: (loss, [L_s], {name: gradient})."""
    ora = U.oracle_with_heads(_ctor(c), K, dtype)
    loss, levels = U.network_ref(ora, K, _batch(c), kind, _weights(c))
    return loss, levels, {k: p.grad.detach().clone() for k, p in ora.named_parameters()}


def _step_grads(mode, c, kind, fuse=True, k=K, graph=None, calls=1):
    """-> (loss, scale_losses, {name: unscaled gradient}, GN3_COUNT deltas, flat parameters) of SegmentationStep on the HIP model."""
    lib = L.lib()
    batch = {key: v.to(DEV) for key, v in _batch(c).items()}
    try:
        lib.mednet_set_option(b"ds_head_fuse", int(fuse))
        with mednet_hip.precision(mode):
            kw = {} if k is None else dict(deep_supervision=k)
            net = O.keyed_init_(HM.ResidualUNet3D(**_ctor(c), **kw)).to(DEV)
            step = SegmentationStep(net, loss_weight=_weights(c), lr=1e-3, loss=kind, graph=graph)
            before = dict(ops.GN3_COUNT)
            if calls == 1:
                scale = 1.0 if step.scaler is None else float(step.scaler.snapshot()[0])
                (loss,) = step._fwd_bwd(batch)
            else:
                for _ in range(calls):
                    loss = step(batch)
                scale = 1.0
            torch.cuda.synchronize()
            count = {key: ops.GN3_COUNT[key] - before[key] for key in before}
            flat = step.flat.grad.clone()
            grads = {name: flat[off:off + p.numel()].reshape(p.shape) / scale for (name, p), off in zip(net.named_parameters(), step.flat.offsets)}
            out = (float(loss), [float(v) for v in step.scale_losses], grads, count, step.flat.flat.clone(), flat)
            step.flat.release()
    finally:
        lib.mednet_set_option(b"ds_head_fuse", 1)
    return out


@pytest.mark.parametrize("c", [4, 14])
@pytest.mark.parametrize("kind", KINDS)
def test_fp32_storage_against_the_live_restatement(c, kind):
    """fp32 storage takes the composed path: loss, scale_losses and every parameter gradient against the restatement, at the bounds
    tests/test_gpu_network.py applies to fp32 storage at this size (NET_TOL["fp32"]; a gradient that fp32 rounding alone moves by
    cond * 1e-6, measured against the fp64 restatement, is held to cond * 3e-6 as there).

    The step asks for exact fp32 products here (config.exact_products, train.SegmentationStep._fwd_bwd).  With the split-bf16
    contraction the block outputs are 6e-6 .. 1e-5 from the oracle's, and on this batch one pooling window of encoder 0's output (of
    262144; relative gap of its two largest entries 6.5e-6) and three of encoder 1's took the other entry; a coarse level's loss reaches
    the encoders above it through that arg-max alone, so `encoders.0.basic_module.conv1.conv.weight` sat at 1.47e-3 (DICE) / 1.26e-3
    (CE, DICE_CE) for C = 4, outside 1e-3.  Measured on the MI355X with exact products: no window differs, worst tensor 3.8e-6 (C = 4)
    and 4.8e-6 (C = 14)."""
    loss_r, levels_r, grads_r = _restatement(c, kind, torch.float32)
    _, _, grads_64 = _restatement(c, kind, torch.float64)
    loss, levels, grads, _, _, _ = _step_grads("fp32", c, kind)
    tl, tg = NET_TOL["fp32"]
    assert abs(loss - loss_r) <= 1e-4 * max(1.0, abs(loss_r)), (loss, loss_r)
    assert len(levels) == K + 1
    for s, (a, b) in enumerate(zip(levels, levels_r)):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (s, a, b)
    want = sum(w * l for w, l in zip(U.default_weights(K), levels))
    assert abs(loss - want) <= 1e-6 * max(1.0, abs(want))
    assert set(grads) == set(grads_r)
    worst = 0.0
    for name, g in grads.items():
        cond = max(1.0, rel(grads_r[name], grads_64[name]) / 1e-6)
        r = rel(g, grads_r[name])
        worst = max(worst, r)
        assert r <= max(tg, cond * 3e-6), f"{name}: rel-L2 {r:.3e} (cond {cond:.1f})"
    print(f"[deep supervision fp32 C={c} {kind}] loss {loss:.6f} (restatement {loss_r:.6f}) worst gradient rel-L2 {worst:.2e}")


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp16x2"])
@pytest.mark.parametrize("c", [4, 14])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_step_against_the_composed_step_and_the_restatement(mode, c, kind):
    loss_r, levels_r, grads_r = _restatement(c, kind, torch.float32)
    loss_f, levels_f, gf, count_f, _, _ = _step_grads(mode, c, kind, fuse=True)
    loss_c, levels_c, gc, count_c, _, _ = _step_grads(mode, c, kind, fuse=False)
    # the bookkeeping: the two supervised blocks find their GroupNorm-3 sums taken, or absent where the node offers no rows -- never declined
    rows = L.lib().mednet_ds_head_gn_rows(8, 8, 8, 128, L.dt_of(U.STORE[mode]))
    print(f"[deep supervision {mode} C={c} {kind}] GN3_COUNT fused {count_f} composed {count_c}")
    assert count_f["declined"] == 0, count_f
    assert (count_f["taken"] - count_c["taken"] >= K) if rows > 0 else (count_f["absent"] >= K), (count_f, count_c)
    tol_t, tol_all = PAIR_TOL[mode]
    tl = 2e-2
    for a, b in zip([loss_f] + levels_f, [loss_c] + levels_c):
        assert abs(a - b) <= tl * max(1.0, abs(b)), (a, b)
    for a, b in zip([loss_f] + levels_f, [loss_r] + levels_r):
        assert abs(a - b) <= tl * max(1.0, abs(b)), (a, b)
    num = den = 0.0
    worst_pair = worst_ratio = 0.0
    for name in gf:
        pair = rel(gf[name], gc[name])
        ef, ec = rel(gf[name], grads_r[name]), rel(gc[name], grads_r[name])
        num += float((gf[name].double() - gc[name].double()).pow(2).sum())
        den += float(gc[name].double().pow(2).sum())
        worst_pair, worst_ratio = max(worst_pair, pair), max(worst_ratio, ef / ec if ec > 0 else 0.0)
        print(f"    {name}: fused/composed {pair:.2e}  fused/restatement {ef:.2e}  composed/restatement {ec:.2e}")
        if gf[name].numel() >= 1024:
            assert pair <= tol_t, f"{name}: fused against composed rel-L2 {pair:.3e} > {tol_t:.1e}"
        assert ef <= 1.5 * ec, f"{name}: fused error {ef:.3e} > 1.5 x composed error {ec:.3e}"
    total = (num / den) ** 0.5
    print(f"[deep supervision {mode} C={c} {kind}] concatenated fused/composed {total:.2e} worst tensor {worst_pair:.2e} worst error ratio {worst_ratio:.2f}")
    assert total <= tol_all, (total, tol_all)


def test_graph_capture_after_two_warm_calls_is_bit_equal_to_eager():
    res = {g: _step_grads("bf16", 4, "DICE_CE", graph=g, calls=3) for g in (False, True)}
    assert res[True][0] == res[False][0] and res[True][1] == res[False][1], (res[True][:2], res[False][:2])
    assert torch.equal(res[True][5], res[False][5]), "gradients of the third call differ between the captured and the eager step"
    assert torch.equal(res[True][4], res[False][4]), "parameters after three steps differ"


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_depth_zero_is_the_model_without_the_keyword(mode):
    a = _step_grads(mode, 4, "DICE", k=0)
    b = _step_grads(mode, 4, "DICE", k=None)
    assert a[0] == b[0] and a[1] == b[1] == [a[0]]
    assert torch.equal(a[5], b[5]) and a[3] == b[3]


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_inference_never_runs_the_auxiliary_heads(mode):
    x = _batch(4)["data"].to(DEV)
    outs = []
    with mednet_hip.precision(mode), torch.no_grad():
        for kw in ({}, dict(deep_supervision=K)):
            net = O.keyed_init_(HM.ResidualUNet3D(**_ctor(4), **kw)).to(DEV).eval()
            outs.append((net(x), net.forward_features(x)))
        deep = net.forward_deep(x)
        pyr = net.forward_pyramid(x)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(deep[0], outs[1][0]) and torch.equal(pyr[0], outs[1][1])
    assert [tuple(t.shape) for t in deep] == [(N, 4) + tuple(v >> s for v in SHAPE) for s in range(K + 1)]
    assert [t.shape[1] for t in pyr] == [32, 64, 128]
