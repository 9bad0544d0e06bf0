"""CPU side of the conditioning tests (tests/norm_cond_util.py): the written-out fp64 reference equals ATen's fp64 GroupNorm /
BatchNorm; ATen's own fp32 kernels stay inside the derived bounds at every ratio the GPU tests use (the bounds are no tighter than
the reference the project is held to); the restated sum-of-squares statistics pass leaves them at R = 4096 and the restated pivoted
pass does not (the GPU test can see the fault it is for)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_cond_util as C

GN_F32 = [(k, R) for k in ("small", "ragged", "first") for R in C.RATIOS["fp32"]]
GN_16 = [(m, R) for m in ("fp16", "bf16") for R in C.RATIOS[m]]
_CASES = {}


def gn_case(key, R, mode):
    k = ("gn", key, R, mode)
    if k not in _CASES:
        _CASES[k] = C.make_case(key, *C.GN_SHAPES[key], R, mode)
    return _CASES[k]


def bn_case(R, mode):
    k = ("bn", R, mode)
    if k not in _CASES:
        n, c, shape = C.BN_SHAPE
        _CASES[k] = C.make_case("bn", n, c, None, shape, R, mode, batch=True)
    return _CASES[k]


def aten(case, dtype, act="relu"):
    """ATen's forward and autograd in `dtype` on the case's (already rounded) inputs; the ReLU mask comes from the reference's z."""
    r = C.reference(case, act)
    x, g, b = (t.clone().to(dtype).requires_grad_(True) for t in (case.x, case.gamma, case.beta))     # (clones: the case is shared)
    if case.batch:
        y = F.batch_norm(x, None, None, g, b, True, 0.0, case.eps)
    else:
        y = F.group_norm(x, case.groups, g, b, case.eps)
    y.backward(r.du.to(dtype))
    return r, y.detach(), x.grad, g.grad, b.grad


def test_reference_is_atens_fp64_normalisation():
    for case in (gn_case("small", 16, "fp32"), gn_case("first", 256, "fp32"), bn_case(16, "fp32")):
        r, y, dx, dg, db = aten(case, torch.float64, act="none")
        for name, got, ref in (("y", y, r.y), ("dx", dx, r.dx), ("dgamma", dg, r.dgamma), ("dbeta", db, r.dbeta)):
            err = float((got - ref).abs().max() / ref.abs().max())
            assert err <= 1e-9, (case.tag, case.R, name, err)      # (R^2 * 2^-53 of ATen's own fp64 pass)


def test_special_units_of_the_reference():
    case = gn_case("small", 256, "fp32")
    r = C.reference(case)
    k, cg = case.special["constant"], case.cg
    assert float(r.var[k]) == 0.0 and float(r.rstd[k]) == 1.0 / np.sqrt(case.eps) and float(r.mean[k]) == C.CONSTANT
    assert torch.equal(r.z[0, k * cg:(k + 1) * cg], torch.relu(case.beta[k * cg:(k + 1) * cg]).reshape(cg, 1, 1, 1).expand(-1, *case.shape))
    k = case.special["near-constant"]
    assert 900 <= float(r.R[k]) <= 1150
    assert bool((case.x[-1] < 0).all()) and bool((case.x[0, :cg] > 0).all())       # the negated sample
    plain = [i for i in range(case.n * case.groups) if i not in case.special.values()]
    assert all(0.8 * 256 <= float(r.R[i]) <= 1.25 * 256 for i in plain), r.R         # the jitter does not dilute the ratio


def check_aten_fp32(case):
    r, y, dx, dg, db = aten(case, torch.float32)
    B = C.bounds(case, r)
    st = lambda t: t.to(C.DT[case.mode])
    out = {"z": C.worst_ratio(st(torch.relu(y)), r.z, B.z, "z"), "dx": C.worst_ratio(st(dx), r.dx, B.dx, "dx"),
           "dgamma": C.worst_ratio(dg, r.dgamma, B.dgamma, "dgamma"), "dbeta": C.worst_ratio(db, r.dbeta, B.dbeta, "dbeta")}
    if not case.batch:
        _, mean, rstd = torch.ops.aten.native_group_norm(case.x.float().contiguous(), None, None, case.n, case.c, case.spatial, case.groups, case.eps)
        out["mean"] = C.worst_ratio(mean, r.mean, B.mean, "mean")
        out["rstd"] = C.worst_ratio(rstd, r.rstd, B.rstd, "rstd")
    print(f"[cond] ATen fp32 {case.tag} R={case.R} {case.mode}: " + " ".join(f"{k}={v:.3f}" for k, v in out.items()))
    assert max(out.values()) <= 1.0, (case.tag, case.R, case.mode, out)


@pytest.mark.parametrize("key,R", GN_F32)
def test_atens_fp32_group_norm_stays_inside_the_bounds(key, R):
    check_aten_fp32(gn_case(key, R, "fp32"))


@pytest.mark.parametrize("mode,R", GN_16)
def test_atens_fp32_group_norm_on_16_bit_inputs_stays_inside_the_bounds(mode, R):
    check_aten_fp32(gn_case("wide", R, mode))


@pytest.mark.parametrize("mode,R", [(m, R) for m in ("fp32", "fp16", "bf16") for R in C.RATIOS[m]])
def test_atens_fp32_batch_norm_stays_inside_the_bounds(mode, R):
    check_aten_fp32(bn_case(R, mode))


def test_running_statistics_of_the_reference():
    case = bn_case(16, "fp32")
    rm0, rv0 = torch.linspace(-1, 1, case.c, dtype=torch.float64), torch.linspace(0.5, 2, case.c, dtype=torch.float64)
    r = C.reference(case, rm0=rm0, rv0=rv0)
    rm, rv = rm0.clone(), rv0.clone()
    F.batch_norm(case.x, rm, rv, None, None, True, C.MOMENTUM_F32, case.eps)
    assert float((rm - r.running_mean).abs().max()) <= 1e-12 * 16 and float((rv - r.running_var).abs().max()) <= 1e-9
    B = C.bounds(case, r)
    assert bool((B.running_var > 0).all()) and bool((B.running_mean > 0).all())


@pytest.mark.parametrize("key,R", GN_F32)
def test_restated_statistics_pass(key, R):
    """The sum-of-squares form leaves the bound of rstd at R = 4096 on the 8^3 shape (and by a wide margin: its error has an R^2
    term); the pivoted form stays inside at every R and shape, the constant unit included."""
    case = gn_case(key, R, "fp32")
    r = C.reference(case)
    B = C.bounds(case, r)
    res = {}
    for pivoted in (False, True):
        mean, rstd = C.gn_stats_model(case, pivoted)
        res[pivoted] = (C.unit_ratios(case, mean, r.mean, B.mean), C.unit_ratios(case, rstd, r.rstd, B.rstd))
        print(f"[cond] model pivoted={int(pivoted)} {key} R={R}: mean {res[pivoted][0]} rstd {res[pivoted][1]}")
    assert max(res[True][0].values()) <= 1.0 and max(res[True][1].values()) <= 1.0, res[True]
    if R == 4096:
        assert res[False][1]["plain"] > 100.0, res[False]
    if R >= 16:
        assert res[False][1]["plain"] > 1.0, res[False]             # (the R^2 term shows from the smallest offset on)
    if case.special:
        assert res[False][1]["near-constant"] > 10.0, res[False]    # mean / std = 1024 at every R
