"""CPU side of tests/test_gpu_losses.py: (1) the three exact input builders meet their premises -- every workgroup's sum of |terms|
is below 2^24 lattice steps, every product is exact, ATen's fp32 softmax / sigmoid give the dyadic probabilities bit for bit; (2)
ATen's fp32 results pass every bound of parts A to C at the small and medium shapes; (3) each checker refuses the fault it is there
for.  The faults run through a model of the kernels' summation on the CPU: fp32 sums per block of 2048 voxels, the partial rows
added in fp64, the finalize arithmetic in fp32 -- with no fault the model passes the exact checks, bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gpu_util as U
import test_gpu_losses as T

MEDIUM = [k for k in T.SHAPES if k != "large"]


# ------------------------------------------------------------------------------------------------ a model of the kernels
def block_sums32(terms):
    """[..., S] fp32 -> [..., blocks] fp32: one partial per workgroup."""
    S = terms.shape[-1]
    nb = -(-S // U.LOSS_BLOCK_VOX)
    t = F.pad(terms.float(), (0, nb * U.LOSS_BLOCK_VOX - S))
    return t.reshape(t.shape[:-1] + (nb, U.LOSS_BLOCK_VOX)).sum(-1)


def keep_mask(n, S, fault):
    keep = torch.ones(n, 1, S)
    if fault == "last_voxel":
        keep[:, :, S - 1] = 0.0          # every sample's last voxel, as a loop bound of `v < spatial - 1` would drop it
    elif fault == "block":
        keep[0, :, U.LOSS_BLOCK_VOX:2 * U.LOSS_BLOCK_VOX] = 0.0
    return keep


def rows_total(part, fault):
    """part [n, c, blocks] fp32 -> fp64 totals per channel; fault "row_twice": the last row is added a second time."""
    tot = part.double().sum((0, 2))
    return tot + part[-1, :, -1].double() if fault == "row_twice" else tot


def hm_model(case, kind, fault=None):
    n, c, S = case.n, case.c, case.spatial
    tgt = case.target.float().reshape(n, c, S).clone()
    if fault == "stride":
        tgt[1] = tgt[0]
    d = case.out.reshape(n, c, S) - tgt
    f = (d * d if kind == "L2" else d.abs()) * keep_mask(n, S, fault)
    Sc = rows_total(block_sums32(f), fault)
    w = case.w.flip(0).numpy() if fault == "weight" else case.w.numpy()
    count = 1.0 if fault == "count" else float(case.count)
    tot = np.float32(0)
    for k in range(c):
        tot = np.float32(tot + np.float32(w[k]) * np.float32(float(Sc[k]) / count))
    scale = torch.from_numpy((np.float32(case.dloss) * w) * np.float32(1.0 / count))[None, :, None]
    if kind == "L2":
        dout = 2.0 * d * scale
    else:
        dout = torch.where(d > 0, scale, torch.where((d < 0) if fault != "sign0" else (d <= 0), -scale, torch.zeros(())))
        if fault == "sign0":
            dout = torch.where(d == 0, scale, dout)
    return tot, dout


def ce_model(case, fault=None):
    n, c, S = case.n, case.c, case.spatial
    lab = case.lab.clone()
    if fault == "stride":
        lab[1] = lab[0]
    live = lab != case.ignore
    idx = lab.clamp(0, c - 1)
    wy = torch.where(live, case.w[(idx + 1) % c if fault == "weight" else idx], torch.zeros(()))
    term = wy * 200.0 * (lab != case.hot)
    keep = keep_mask(n, S, fault)[:, 0]
    num = rows_total(block_sums32(term * keep)[:, None], fault)[0]
    den = rows_total(block_sums32(wy * keep)[:, None], fault)[0]
    with np.errstate(invalid="ignore"):
        return np.float32(np.float64(num) / np.float64(den)), np.float32(float(den))


def dice_model(case, ignore, fault=None):
    n, c, S = case.n, case.c, case.spatial
    p = torch.sigmoid(case.lg) if case.sigmoid else torch.softmax(case.lg, 1)
    lab = case.lab.clone()
    if fault == "stride":
        lab[1] = lab[0]
    t = F.one_hot(lab, c).permute(0, 2, 1).float()
    m = torch.ones_like(t) if ignore is None else (t != ignore).float()
    keep = keep_mask(n, S, fault)
    I = rows_total(block_sums32(p * t * m * keep), fault).float()
    D = rows_total(block_sums32((p + t) * m * keep), fault).float()
    w = case.w.roll(1) if fault == "weight" else case.w
    dice = 2.0 * (w * I) / D.clamp(min=case.eps)
    s = torch.zeros(())
    for k in range(c):
        s = s + (1.0 - dice[k])
    return torch.stack((I, D), -1), dice, s / c


SUM_FAULTS = ("last_voxel", "block", "row_twice", "stride", "weight")


# ------------------------------------------------------------------------------------------------ (1) premises
def test_fp32_premises_of_the_exact_inputs():
    assert float(torch.exp(torch.tensor(-200.0))) == 0.0 and float(np.exp(np.float32(-200.0))) == 0.0
    assert float(torch.sigmoid(torch.tensor(-200.0))) == 0.0 and float(torch.sigmoid(torch.tensor(200.0))) == 1.0
    for w in U.CE_WEIGHTS:
        assert float(np.float32(w) * np.float32(200.0)) == w * 200.0 and (w * 200.0) % 50.0 == 0.0


@pytest.mark.parametrize("key", MEDIUM)
def test_exact_builders_meet_their_premises(key):
    """The references assert the premises (block sums below 2^24 steps, weights powers of two) for every case they are built for;
    here for all class and channel counts of the GPU module, with the products and probabilities checked in fp32 on top."""
    shape = T.SHAPES[key]
    for c in (1, 3, 16, 17, 300) if key in ("tiny", "block") else (3,):
        for tgt in ("u8", "f32"):
            case = U.hm_exact_case(f"p{key}{c}", 2, c, shape, tgt)
            for kind in ("L2", "L1"):
                ref = U.hm_reference(case, kind)
                assert float(U.block_abs_sums(ref.d * ref.d).max()) <= 2.0 ** 23
                prod = case.w.double() * (ref.Sc / case.count).float().double()      # w_c * f32(S_c / count) is an fp32 number
                assert torch.equal(prod.float().double(), prod)
    for c in T.CLASSES:
        case = U.ce_exact_case(f"p{key}{c}", 2, c, shape, 1 if c > 1 else -100)
        ref = U.ce_exact_reference(case)
        assert ref.den64 * 4 == round(ref.den64 * 4) and ref.num64 % 50 == 0
        nll = -torch.log_softmax(case.lg, 1)                                        # ATen's fp32 terms: exactly 200 or 0
        assert set(nll.gather(1, case.hot[:, None])[:, 0].unique().tolist()) == {0.0} and set(nll.unique().tolist()) <= {0.0, 200.0}
        for sigmoid in (False, True):
            dc = U.dice_exact_case(f"p{key}{c}", 2, c, shape, sigmoid)
            p32 = torch.sigmoid(dc.lg) if sigmoid else torch.softmax(dc.lg, 1)
            assert torch.equal(p32.double(), dc.p) and set(dc.p.unique().tolist()) <= {0.0, 0.25, 0.5, 1.0}
            for ignore in (None, 0, 1):
                U.dice_exact_reference(dc, ignore)


def test_exact_loss_recipes_agree_with_aten_in_fp64():
    """The heat-map recipe lands within 2.5e-8 relative of ATen's fp64 loss; f32(num64 / den64) is ATen's fp64 cross-entropy rounded to
    fp32; every voxel ignored gives NaN in ATen too."""
    shape = T.SHAPES["three"]
    case = U.hm_exact_case("agree", 2, 3, shape)
    for kind, fn in (("L2", F.mse_loss), ("L1", F.l1_loss)):
        ref = U.hm_reference(case, kind)
        aten = sum(float(case.w[k]) * float(fn(case.out[:, k].double(), case.target[:, k].double())) for k in range(3))
        assert abs(ref.loss64 - aten) <= 1e-14 * aten and abs(float(ref.loss32) - aten) <= 2.5e-8 * aten
    for ignored in ("some", "sample", "all"):
        cc = U.ce_exact_case("agree", 2, 5, shape, -100, ignored)
        aten = F.cross_entropy(cc.lg.double(), cc.lab, weight=cc.w.double(), ignore_index=-100)
        U.assert_same_f32(np.float32(float(aten)), U.ce_exact_reference(cc).loss32, "CE " + ignored)


# ------------------------------------------------------------------------------------------------ (2) ATen in fp32 passes
@pytest.mark.parametrize("key,n,c,edge", [t for t in T.RANDOM_CASES if t[0] != "large"])
def test_aten_fp32_passes_the_bounds_of_part_b(key, n, c, edge):
    case = T.random_case(key, n, c, edge)
    for sigmoid, ignore in T.dice_variants(key, c):
        r64, r32 = U.dice_chain(case, sigmoid, ignore, torch.float64), U.dice_chain(case, sigmoid, ignore, torch.float32)
        norm = U.dice_grad_norm(case, r64, sigmoid)
        e32, eps_case = U.loss_grad_eps(r32.dlg, r64.dlg, norm, "dice")
        assert e32 <= 4e-6, f"ATen's own fp32 error {e32:.2e}: the norm of the bound does not fit the gradient"
        U.check_dice_random(case, r64, norm, eps_case, r32.saved, r32.loss, r32.dlg, f"ATen fp32 Dice {key} C={c} {sigmoid} {ignore}")
    if c > 1:
        for ignore in (-100, c - 1):
            r64, r32 = U.ce_chain(case, ignore, torch.float64), U.ce_chain(case, ignore, torch.float32)
            e32, eps_case = U.loss_grad_eps(r32.dlg, r64.dlg, r64.norm, "ce")
            assert e32 <= 8e-6
            U.check_ce_random(case, r64, eps_case, r32.den, r32.loss, r32.dlg, f"ATen fp32 CE {key} C={c} {ignore}")


def test_aten_fp32_passes_the_tolerances_of_part_a():
    shape = T.SHAPES["three"]
    case = U.hm_exact_case("aten", 2, 3, shape)
    ref = U.hm_reference(case, "L2")
    out = case.out.clone().requires_grad_(True)
    loss = sum(case.w[k] * F.mse_loss(out[:, k], case.target[:, k].float()) for k in range(3))
    (loss * case.dloss).backward()
    U.check_gradient(out.grad.reshape(2, 3, -1), ref.grad64, ref.grad64.abs(), 4.0 * U.U32, "ATen fp32 heat-map L2 gradient")
    for c in (1, 4, 17):
        for sigmoid in (False, True):
            dc = U.dice_exact_case("aten", 2, c, shape, sigmoid)
            for ignore in (None, 0, 1):
                p = torch.sigmoid(dc.lg) if sigmoid else torch.softmax(dc.lg, 1)
                _, _, I, D = U.dice_sums(p, dc.lab, ignore)
                dice, loss = U.dice_from_sums(I, D, dc.w, dc.eps)
                U.check_dice_exact(dc, U.dice_exact_reference(dc, ignore), torch.stack((I, D), -1), dice, loss, "ATen fp32 Dice")
    cc = U.ce_exact_case("aten", 2, 5, shape, 1)
    r = U.ce_exact_reference(cc)
    U.assert_same_f32(U.f32_scalar(F.cross_entropy(cc.lg, cc.lab, weight=cc.w, ignore_index=1)), r.loss32, "ATen fp32 CE")


# ------------------------------------------------------------------------------------------------ (3) the checkers refuse faults
@pytest.mark.parametrize("tgt", ["u8", "f32"])
def test_heatmap_checker_passes_the_model_and_refuses_each_fault(tgt):
    case = U.hm_exact_case("fault", 2, 3, T.SHAPES["three"], tgt)
    case.w = torch.tensor([0.25, 2.0, 0.5])       # three different weights: one taken from the wrong index shows
    for kind in ("L2", "L1"):
        ref = U.hm_reference(case, kind)
        assert bool((ref.d == 0).any())
        U.check_hm(case, ref, *hm_model(case, kind), "model")
        for fault in SUM_FAULTS + ("count",) + (("sign0",) if kind == "L1" else ()):
            with pytest.raises(AssertionError):
                U.check_hm(case, ref, *hm_model(case, kind, fault), fault)
        loss, dout = hm_model(case, kind)
        miss = dout.clone()
        miss[1, 2, -1] = float("nan")          # the last voxel's gradient not written
        with pytest.raises(AssertionError):
            U.check_hm(case, ref, loss, miss, "unwritten")
        if kind == "L2":
            off = dout.clone()
            off[0, 1, 2048] *= 1.0 + 8.0 * U.U32
            with pytest.raises(AssertionError, match="1 of"):
                U.check_hm(case, ref, loss, off, "eight roundings")


@pytest.mark.parametrize("ignore,ignored", [(-100, "some"), (1, "sample")])
def test_ce_checker_passes_the_model_and_refuses_each_fault(ignore, ignored):
    case = U.ce_exact_case("fault", 2, 5, T.SHAPES["three"], ignore, ignored)
    case.lab[:, -1] = 0          # the last voxel of every sample is live and its class is not the voxel's 0-logit class
    case.hot[:, -1] = 1
    case.lg[:, :, -1] = -200.0
    case.lg[:, 1, -1] = 0.0
    ref = U.ce_exact_reference(case)
    U.check_ce_exact(ref, *ce_model(case), "model")
    for fault in SUM_FAULTS:
        if fault == "block" and ignored == "sample":
            continue    # (sample 0 is ignored as a whole: its second block holds no term)
        with pytest.raises(AssertionError):
            U.check_ce_exact(ref, *ce_model(case, fault), fault)
    allc = U.ce_exact_case("fault", 2, 5, T.SHAPES["three"], ignore, "all")
    rall = U.ce_exact_reference(allc)
    U.check_ce_exact(rall, *ce_model(allc), "all ignored")
    with pytest.raises(AssertionError):
        U.check_ce_exact(rall, np.float32(0.0), np.float32(0.0), "0 instead of NaN")


@pytest.mark.parametrize("sigmoid", [False, True])
def test_dice_checker_passes_the_model_and_refuses_each_fault(sigmoid):
    case = U.dice_exact_case("fault", 2, 4, T.SHAPES["three"], sigmoid)
    for ignore in (None, 0, 1):
        ref = U.dice_exact_reference(case, ignore)
        U.check_dice_exact(case, ref, *dice_model(case, ignore), "model")
        for fault in SUM_FAULTS:
            if fault == "weight" and ignore == 1:
                continue      # (ignore_index 1 masks every voxel of its own class: I_c = 0 and the weight multiplies nothing)
            with pytest.raises(AssertionError):
                U.check_dice_exact(case, ref, *dice_model(case, ignore, fault), fault)


def test_a_dropped_voxel_at_128_cubed_is_below_the_old_tolerance_and_above_the_new_bounds():
    """What the suite held the losses to (|loss - ref| <= 2e-6) against one voxel of 598 975: invisible there, refused here."""
    case = U.dice_exact_case("big", 1, 2, T.SHAPES["large"], False)
    ref = U.dice_exact_reference(case, None)
    saved, dice, loss = dice_model(case, None, "last_voxel")
    assert abs(float(loss) - ref.loss64) <= 2e-6
    with pytest.raises(AssertionError, match="saved"):
        U.check_dice_exact(case, ref, saved, dice, loss, "last voxel")
    U.check_dice_exact(case, ref, *dice_model(case, None), "model")


def _other(case, **kw):
    import copy
    c = copy.copy(case)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_gradient_checkers_refuse_stride_weight_and_count_faults():
    case = T.random_case("three", 2, 4, False)
    lab0 = case.lab.clone()
    lab0[1] = lab0[0]
    for sigmoid in (False, True):
        r64, r32 = U.dice_chain(case, sigmoid, None, torch.float64), U.dice_chain(case, sigmoid, None, torch.float32)
        norm = U.dice_grad_norm(case, r64, sigmoid)
        _, eps_case = U.loss_grad_eps(r32.dlg, r64.dlg, norm, "dice")
        for name, other in (("stride", _other(case, lab=lab0)), ("weight", _other(case, w=case.w.roll(1))), ("dloss", _other(case, dloss=1.0 + 1e-4))):
            f = U.dice_chain(other, sigmoid, None, torch.float32)
            with pytest.raises(AssertionError):
                U.check_dice_random(case, r64, norm, eps_case, r64.saved, r64.loss, f.dlg, name)
        with pytest.raises(AssertionError, match="saved"):
            U.check_dice_random(case, r64, norm, eps_case, r64.saved * (1.0 + 2.0 ** -17), r64.loss, r32.dlg, "saved")
        with pytest.raises(AssertionError, match="loss"):
            U.check_dice_random(case, r64, norm, eps_case, r64.saved, r64.loss + 2e-5, r32.dlg, "loss")
    r64, r32 = U.ce_chain(case, -100, torch.float64), U.ce_chain(case, -100, torch.float32)
    _, eps_case = U.loss_grad_eps(r32.dlg, r64.dlg, r64.norm, "ce")
    for name, dlg in (("stride", U.ce_chain(_other(case, lab=lab0), -100, torch.float32).dlg),
                      ("weight", U.ce_chain(_other(case, w=case.w.roll(1)), -100, torch.float32).dlg),
                      ("count", r32.dlg * r64.den), ("ignored voxel", U.ce_chain(_other(case, ign=torch.zeros_like(case.ign)), -100, torch.float32).dlg)):
        with pytest.raises(AssertionError):
            U.check_ce_random(case, r64, eps_case, r64.den, r64.loss, dlg, name)
    with pytest.raises(AssertionError):
        U.check_ce_random(case, r64, eps_case, r64.den * (1 + 1e-5), r64.loss, r32.dlg, "den")


# ------------------------------------------------------------------------------------------------ Adam
def test_adam_lines_equal_torch_optim_adam_in_fp64():
    case = U.adam_case("optim", 1000)
    hp = {k: float(np.float32(v)) for k, v in U.ADAM_HP.items()}      # the fp32 numbers the ABI receives, given to both
    for wd in (0.0, float(np.float32(0.01))):
        ref = case.p.double().clone().requires_grad_(True)
        opt = torch.optim.Adam([ref], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=wd)
        p, m, v = case.p.double(), torch.zeros(1000, dtype=torch.float64), torch.zeros(1000, dtype=torch.float64)
        g = np.random.Generator(np.random.PCG64(7))
        for step in (1, 2, 3):
            grad = torch.from_numpy(g.standard_normal(1000))
            ref.grad = grad.clone()
            opt.step()
            r = U.adam_lines(p, grad, m, v, wd=wd, step=step, gscale=1.0, dtype=torch.float64, **U.ADAM_HP)
            p, m, v = r.p, r.m, r.v
            st = opt.state[ref]     # (values of size 1: a few ulp of fp64 -- ATen forms m with lerp and the update with addcdiv)
            for name, got, want in (("p", p, ref.detach()), ("m", m, st["exp_avg"]), ("v", v, st["exp_avg_sq"])):
                assert float((got - want).abs().max()) <= 2e-15, (name, wd, step)


@pytest.mark.parametrize("count", [c for c in T.ADAM_COUNTS if c != T.ADAM_LARGE])
def test_adam_fp32_lines_pass_and_each_fault_is_refused(count):
    case = U.adam_case(f"adam{count}", count)
    assert count < 16 or bool(((case.g == 0) & (case.v == 0)).any())
    for step, wd, gs in T.ADAM_ALL:
        ref = U.adam_reference(case, wd, step, gs)
        assert max(ref.r32s[k] for k in ("m", "v", "pt")) <= 5e-6, ref.r32s
        U.check_adam(ref, ref.r32.p, ref.r32.m, ref.r32.v, "fp32 lines")
        kw = dict(wd=wd, step=step, gscale=gs, dtype=torch.float32, **U.ADAM_HP)
        faults = {"no bias correction": dict(kw, bias_correction=False), "step off by one": dict(kw, step=step + 1),
                  "grad_scale ignored": dict(kw, gscale=1.0)}
        if wd:
            faults["no weight decay"] = dict(kw, wd=0.0)
        if gs == 1.0:
            del faults["grad_scale ignored"]
        if count == 1:
            continue      # (the single element has g = 0 and v = 0: its denominator is eps, whatever the bias correction)
        for name, f in faults.items():
            r = U.adam_lines(case.p, case.g, case.m, case.v, **f)
            with pytest.raises(AssertionError):
                U.check_adam(ref, r.p, r.m, r.v, name)
        skip = ref.r32.p.clone()
        skip[count - 1] = case.p[count - 1]                 # the last element not updated
        if float(ref.r64.delta[count - 1].abs()) > 1e-6:
            with pytest.raises(AssertionError):
                U.check_adam(ref, skip, ref.r32.m, ref.r32.v, "last element skipped")
