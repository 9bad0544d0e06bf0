"""csrc/optim.hip on the MI355X: the global gradient norm (exact on lattice inputs, against fp64 with the derived bound on random
ones), the skip rule for non-finite gradients with and without a loss scaler, the SGD / AdamW / Adam updates (bit for bit on dyadic
inputs, against the fp64 restatement on random ones), every buffer between guard bands, and the step classes end to end against
torch.nn.utils.clip_grad_norm_ + torch.optim in fp64.  Helpers and bounds: tests/optim_util.py, profiles/optim_bounds.md."""
import numpy as np
import pytest
import torch

import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import ops
from mednet_hip.train import LandmarkStep, LossScaler, PolyLR, SegmentationStep

import gpu_util as U
import optim_util as OU
from fence import Fence
from gpu_util import DEV

pytestmark = pytest.mark.gpu
ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
SMALL = [1, 3, 4, 255, 1024, 1025]
UPDATE_TWO_TRIPS = OU.MAX_ROWS * 1024 + 1029          # the update kernels take 1024 elements per workgroup and trip


def placed(t, offset=0):
    """`t` on the device behind a pointer `offset` floats past a 16-byte boundary."""
    buf = torch.zeros(t.numel() + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + t.numel()]
    view.copy_(t)
    return view


def scaler(scale=65536.0, good=0.0, steps=0.0, skipped=0.0, growth=2.0, backoff=0.5, interval=2000):
    sc = LossScaler(DEV, growth_factor=growth, backoff_factor=backoff, growth_interval=interval)
    sc.state.copy_(torch.tensor([scale, good, steps, 0.0, skipped, 0.0, 0.0, 0.0]))
    return sc


def norm_state(g, max_norm=None, inv_world=1.0, sc=None):
    ost = ops.new_opt_state(DEV)
    ops.grad_norm_(g, ost, max_norm, inv_world, None if sc is None else sc.state)
    torch.cuda.synchronize()
    return ost.cpu().numpy()


# ================================================================================================ the norm
@pytest.mark.parametrize("count", SMALL + [OU.max_rows_count(), OU.ragged_count()])
def test_norm_is_exact_on_lattice_gradients(count):
    assert OU.rows_of(OU.max_rows_count()) == OU.MAX_ROWS > OU.rows_of(OU.max_rows_count() - 1)
    g = OU.lattice_grad(f"lat{count}", count, e=-3)
    g[-1] = np.float32(0.375)                                   # the last element counts
    gt = torch.from_numpy(g)
    seen = []
    for offset in range(4):
        gd = placed(gt, offset)
        st = norm_state(gd, max_norm=1.0)
        OU.check_norm_exact(st, g, 1.0, f"count {count} pointer offset {offset}")
        assert st[2] == np.float32(min(1.0, 1.0 / (np.sqrt(OU.exact_sumsq(g)) + 1e-6))), f"coef {st[2]!r}"
        again = norm_state(gd, max_norm=1.0)
        assert st[:4].tobytes() == again[:4].tobytes(), f"count {count} offset {offset}: two runs differ"
        seen.append(st[:4].tobytes())
    assert len(set(seen)) == 1                                  # (exact inputs: the same bits whatever the alignment)
    U.report("optim", f"norm exact count={count} rows={OU.rows_of(count)}", "grad_sumsq_partial_kernel+grad_norm_finalize_kernel", 4 * count)


@pytest.mark.parametrize("count", [OU.max_rows_count(), OU.ragged_count()])
def test_norm_of_random_gradients_against_fp64(count):
    rows = OU.rows_of(count)
    g = np.random.default_rng(count).standard_normal(count).astype(np.float32)
    for offset in (0, 3):
        gd = placed(torch.from_numpy(g), offset)
        st = norm_state(gd)
        e_s, e_n = OU.check_norm_random(st, g.astype(np.float64), count, rows, OU.head_of(offset), f"count {count} offset {offset}")
        print(f"[bound] norm count={count} offset={offset} rows={rows} k={OU.sumsq_terms(count, rows, OU.head_of(offset))} "
              f"sumsq: seen {e_s:.3e} bound {OU.gamma(OU.sumsq_terms(count, rows, OU.head_of(offset))):.3e}  "
              f"norm: seen {e_n:.3e} bound {OU.norm_bound(count, rows, OU.head_of(offset)):.3e}")
        assert st[2] == 1.0 and st[3] == 0.0
    # magnitudes up to 2^30 behind a loss scale of 2^16: scaled before squared, finite, the unscaled result times an exact power of two
    big = np.clip(g * np.float32(2.0 ** 28), -2.0 ** 30, 2.0 ** 30).astype(np.float32)
    gd = placed(torch.from_numpy(big))
    a = norm_state(gd, sc=scaler(65536.0))
    b = norm_state(placed(torch.from_numpy(big * np.float32(2.0 ** -16))))
    c = norm_state(gd)
    d = norm_state(gd, inv_world=0.5, sc=scaler(32768.0))
    assert np.isfinite(a[:2]).all() and a[3] == 0.0
    assert a[:2].tobytes() == b[:2].tobytes() == d[:2].tobytes(), (a[:2], b[:2], d[:2])
    assert c[0] == a[0] * np.float32(2.0 ** 32) and c[1] == a[1] * np.float32(2.0 ** 16) and np.isfinite(c[0])
    OU.check_norm_random(a, big.astype(np.float64) * 2.0 ** -16, count, rows, 0, f"count {count}, loss scale 2^16")


# ================================================================================================ running the update entries
def dev(state, offset=0):
    return {k: placed(v.float(), offset) for k, v in state.items()}


def cpu(state):
    torch.cuda.synchronize()
    return {k: v.cpu().clone() for k, v in state.items()}


def update(kind, st, g, hp, ost, sc=None, inv_world=1.0):
    if kind == "sgd":
        ops.sgd_step_(st["p"], g, st.get("buf"), hp["lr"], hp.get("mu", 0.0), hp.get("nesterov", False), hp.get("wd", 0.0), inv_world, ost, sc)
    else:
        ops.adamw_step_(st["p"], g, st["m"], st["v"], hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp.get("wd", 0.0), ost, kind == "adamw",
                        inv_world, sc)


def full_step(kind, st, g, hp, ost, max_norm=None, sc=None, inv_world=1.0):
    ops.grad_norm_(g, ost, max_norm, inv_world, None if sc is None else sc.state)
    update(kind, st, g, hp, ost, sc, inv_world)


def zero_state(kind, p, hp):
    st = dict(p=p.clone())
    if kind == "sgd":
        if hp.get("mu"):
            st["buf"] = torch.zeros_like(p)
    else:
        st["m"], st["v"] = torch.zeros_like(p), torch.zeros_like(p)
    return st


KINDS = {"sgd": dict(lr=1e-2, mu=0.99, nesterov=True, wd=3e-5), "adamw": dict(ADAM, wd=1e-2), "adam": dict(ADAM, wd=1e-2)}


# ================================================================================================ non-finite gradients
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_nonfinite_gradient_skips_the_whole_step(kind, bad):
    count, hp = 4101, KINDS[kind]
    p0, gs = OU.random_case(f"nf{kind}", count, steps=3)
    for k, where in enumerate((0, count // 2, count - 1)):
        st, ost = dev(zero_state(kind, p0, hp), offset=k), ops.new_opt_state(DEV)
        full_step(kind, st, placed(gs[0]), hp, ost, max_norm=20.0)                 # one clean step: the moments are not zero
        before = cpu(st)
        assert ost.cpu().tolist()[3:6] == [0.0, 1.0, 0.0]
        poisoned = gs[1].clone()
        poisoned[where] = bad
        gd = placed(poisoned, offset=(k + 1) % 4)
        ops.grad_norm_(gd, ost, 20.0)
        assert ost.cpu().tolist()[3] == 1.0, f"{bad} at {where}: nonfinite is not set"
        update(kind, st, gd, hp, ost)
        OU.check_unchanged(cpu(st), before, f"{kind}: {bad} at {where}")
        o = ost.cpu().tolist()
        OU.check_counts(int(o[4]), int(o[5]), 1, 1, f"{kind}: {bad} at {where}")
        assert o[3] == 0.0                                                         # cleared for the next step
        # the next clean step: bias correction of the UNSKIPPED count (step 2)
        ref = OU.update_reference(kind, before, gs[2], hp, 2, 1.0, 20.0)
        full_step(kind, st, placed(gs[2]), hp, ost, max_norm=20.0)
        OU.check_update(kind, ref, cpu(st), hp, f"{kind}: the clean step after {bad} at {where}")
        o = ost.cpu().tolist()
        OU.check_counts(int(o[4]), int(o[5]), 2, 1, f"{kind}: after the clean step")
    # a finite gradient whose square overflows fp32 is skipped as well (documented in the header)
    huge = gs[1].clone()
    huge[7] = 3.0e19
    before = cpu(st)
    full_step(kind, st, placed(huge), hp, ost)
    OU.check_unchanged(cpu(st), before, f"{kind}: |g| = 3e19")
    assert ost.cpu().tolist()[3:6] == [0.0, 2.0, 2.0]


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_nonfinite_behind_a_loss_scaler_follows_the_existing_rule(kind):
    import test_gpu_losses as LS
    count, hp = 4101, KINDS[kind]
    p0, gs = OU.random_case(f"nfs{kind}", count, steps=3)
    scale = 1024.0
    st, ost, sc = dev(zero_state(kind, p0, hp)), ops.new_opt_state(DEV), scaler(scale, 1.0, 4.0, 7.0, interval=3)
    poisoned = gs[0] * scale
    poisoned[count // 3] = float("inf")
    gd = placed(poisoned)
    before = cpu(st)
    ops.grad_norm_(gd, ost, 5.0, 0.5, sc.state)
    assert sc.state.cpu().tolist()[3] == 1.0 and ost.cpu().tolist()[3] == 1.0           # found_inf is raised with nonfinite
    update(kind, st, gd, hp, ost, sc, 0.5)
    OU.check_unchanged(cpu(st), before, f"{kind} behind a scaler")
    # the existing entry on the same gradient from the same scaler state
    old = LS.scaler_state(scale, 1.0, 4.0, 7.0)
    z = lambda: torch.zeros(count, device=DEV)
    LS.scaled_step(p0.to(DEV).clone(), gd, z(), z(), old, 0.0, 0.5, interval=3)
    assert sc.state.cpu().tolist() == old.cpu().tolist() == [512.0, 0.0, 4.0, 0.0, 8.0, 0.0, 0.0, 0.0]
    assert ost.cpu().tolist()[3:6] == [0.0, 0.0, 0.0]                                     # (the counts live in the scaler state)
    # growth_interval = 2: two clean steps double the scale
    sc2, ost2 = scaler(scale, interval=2), ops.new_opt_state(DEV)
    for k, want in ((1, [scale, 1.0, 1.0]), (2, [2 * scale, 0.0, 2.0])):
        ref = OU.update_reference(kind, cpu(st), gs[k] * scale, hp, k, 0.5 / scale, 5.0)
        full_step(kind, st, placed(gs[k] * scale), hp, ost2, 5.0, sc2, 0.5)
        OU.check_update(kind, ref, cpu(st), hp, f"{kind}: clean scaled step {k}")
        assert sc2.state.cpu().tolist()[:5] == want + [0.0, 0.0]
        assert abs(float(ost2[1]) - ref.norm) <= OU.norm_bound(count, OU.rows_of(count), 0) * ref.norm   # the UNSCALED mean gradient's norm


# ================================================================================================ updates, exact
@pytest.mark.parametrize("mu,nesterov,wd", [(0.0, False, 0.0), (0.0, False, 0.5), (0.5, False, 0.0), (0.5, False, 0.5), (0.5, True, 0.0),
                                            (0.5, True, 0.5)])
def test_sgd_is_exact_on_dyadic_inputs(mu, nesterov, wd):
    count = 2 * 1024 + 5 + 1                                       # three workgroups, two trailing elements
    hp = dict(lr=OU.DYADIC["lr"], mu=mu, nesterov=nesterov, wd=wd)
    p0, gs = OU.dyadic_case(f"dy{mu}{nesterov}{wd}", count)
    what = f"SGD mu={mu} nesterov={nesterov} wd={wd}"
    for coef in (OU.DYADIC["coef"], 1.0):
        ref = OU.Reference("sgd", p0, hp)
        for g in gs:
            ref.step(g, coef=coef)
        for offset in (0, 1):                                      # 16-byte loads / element by element
            by_hand = lambda: torch.tensor([0.0, 0.0, coef, 0.0, 0.0, 0.0, 0.0, 0.0], device=DEV)
            st, ost = dev(zero_state("sgd", p0, hp), offset), by_hand()
            for g in gs:
                update("sgd", st, placed(g, offset), hp, ost)
            OU.check_bits(cpu(st), ref.state(), f"{what} coef={coef} offset={offset}")
            assert ost.cpu().tolist() == [0.0, 0.0, coef, 0.0, 5.0, 0.0, 0.0, 0.0]
            # a power-of-two loss scale (and world size) gives the same bits
            st, ost, sc = dev(zero_state("sgd", p0, hp), offset), by_hand(), scaler(1024.0, interval=100)
            for g in gs:
                update("sgd", st, placed(g * 2048.0, offset), hp, ost, sc, 0.5)
            OU.check_bits(cpu(st), ref.state(), f"{what} coef={coef} offset={offset}, loss scale 1024, world 2")
            assert sc.state.cpu().tolist()[:5] == [1024.0, 5.0, 5.0, 0.0, 0.0]
    # coef == 1 from a norm below max_norm, clipping off, and the unguarded form: all the bits of the reference with coef 1
    for form in ("below", "off", "unguarded"):
        st, ost = dev(zero_state("sgd", p0, hp)), ops.new_opt_state(DEV)
        for g in gs:
            gd = placed(g)
            if form == "unguarded":
                update("sgd", st, gd, hp, None)
            else:
                full_step("sgd", st, gd, hp, ost, max_norm=1.0e6 if form == "below" else None)
                assert float(ost[2]) == 1.0 and float(ost[1]) > 0
        OU.check_bits(cpu(st), ref.state(), f"{what} {form}")
    U.report("optim", what, "sgd_kernel", 5 * count)


# ================================================================================================ updates, random
@pytest.mark.parametrize("count", [1000, UPDATE_TWO_TRIPS])
@pytest.mark.parametrize("kind", ["sgd", "adamw", "adam"])
def test_updates_against_the_fp64_restatement_with_clipping_active(kind, count):
    hp = KINDS[kind]
    p0, gs = OU.random_case(f"rnd{kind}{count}", count, steps=5)
    max_norm = 0.25 * float(np.sqrt(count))                         # the gradients' norm is about sqrt(count)
    st, ost = dev(zero_state(kind, p0, hp)), ops.new_opt_state(DEV)
    rows = OU.rows_of(count)
    for k, g in enumerate(gs, 1):
        ref = OU.update_reference(kind, cpu(st), g, hp, k, 1.0, max_norm)
        assert ref.coef < 0.5
        full_step(kind, st, placed(g), hp, ost, max_norm)
        seen = OU.check_update(kind, ref, cpu(st), hp, f"{kind} count={count} step {k}")
        o = ost.cpu().tolist()
        e_n = abs(o[1] - ref.norm) / ref.norm
        assert e_n <= OU.norm_bound(count, rows, 0) and abs(o[2] - ref.coef) <= (OU.norm_bound(count, rows, 0) + OU.U32) * ref.coef
        assert o[3:6] == [0.0, float(k), 0.0]
        print(f"[bound] {kind} count={count} step={k} norm seen {e_n:.2e} " + " ".join(
            f"{n}: r32 {ref.r32s[n]:.2e} eps {ref.eps[n]:.2e} seen {seen[n]:.2e}" for n in seen))


@pytest.mark.parametrize("count", [1000, UPDATE_TWO_TRIPS])
def test_adam_on_the_new_path_equals_the_scaled_entry_bit_for_bit(count):
    """Clipping off, nonfinite clear, L2 decay: adam_guarded_kernel computes what adam_scaled_kernel computes, at scale 1."""
    import test_gpu_losses as LS
    case = U.adam_case(f"bits{count}", count)
    wd, inv_world = 0.01, 0.125
    p, g, m, v = LS.dev_state(case)
    old = LS.scaler_state(1.0, 1.0, 3.0, 0.0)
    LS.scaled_step(p, g, m, v, old, wd, inv_world, interval=3)
    st = dict(zip("pgmv", LS.dev_state(case)))
    sc, ost = scaler(1.0, 1.0, 3.0, 0.0, interval=3), ops.new_opt_state(DEV)
    hp = dict(lr=U.ADAM_HP["lr"], b1=U.ADAM_HP["b1"], b2=U.ADAM_HP["b2"], eps=U.ADAM_HP["eps"], wd=wd)
    full_step("adam", st, st["g"], hp, ost, None, sc, inv_world)
    torch.cuda.synchronize()
    for name, a, b in (("p", st["p"], p), ("m", st["m"], m), ("v", st["v"], v)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: {int((a != b).sum())} of {count} elements differ"
    assert sc.state.cpu().tolist() == old.cpu().tolist() == [1.0, 2.0, 4.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    # and without a scaler from the same count of steps taken
    st2, ost2 = dict(zip("pgmv", LS.dev_state(case))), ops.new_opt_state(DEV)
    ost2[4] = 3.0
    full_step("adam", st2, st2["g"], hp, ost2, None, None, inv_world)
    for name in "pmv":
        assert torch.equal(st2[name].view(torch.int32), st[name].view(torch.int32)), name


# ================================================================================================ footprint
@pytest.mark.parametrize("count", [1, 1025, OU.ragged_count()])
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_every_buffer_between_guard_bands(kind, count):
    hp = KINDS[kind]
    p0, (g,) = OU.random_case(f"fp{kind}{count}", count, steps=1)
    g[0] = 1.5
    start = zero_state(kind, p0, hp)
    for k in start:
        if k != "p":
            start[k] = 0.1 * p0.abs()
    need = L.lib().mednet_grad_norm_ws_bytes(count)
    assert need == 4 * OU.rows_of(count)

    def run(put, ws):
        st, gd, ost = {k: put(v.to(DEV)) for k, v in start.items()}, put(g.to(DEV)), put(ops.new_opt_state(DEV))
        sc = scaler(4.0, interval=5)
        sc.state = put(sc.state)
        ops.grad_norm_(gd, ost, 0.03 * float(np.sqrt(count)), 0.5, sc.state, ws=ws)    # (gscale 1/8: the norm is about sqrt(count) / 8)
        update(kind, st, gd, hp, ost, sc, 0.5)
        torch.cuda.synchronize()
        return st, gd, ost, sc.state

    want = run(lambda t: t.clone(), torch.empty(need, dtype=torch.uint8, device=DEV))
    with Fence() as fence:
        got = run(fence.put, fence.workspace(need))
        fence.check()
        assert fence.ws_requests[0][:2] == (need, need)
    for name in want[0]:
        assert torch.equal(got[0][name].view(torch.int32), want[0][name].view(torch.int32)), f"{kind} count={count}: {name}"
        assert fence.owns(got[0][name])
    assert torch.equal(got[1].cpu(), g), "the gradient was written"
    assert torch.equal(got[2].view(torch.int32), want[2].view(torch.int32)) and torch.equal(got[3], want[3])
    assert got[3].cpu().tolist()[:5] == [4.0, 1.0, 1.0, 0.0, 0.0] and float(got[2][2]) < 1.0


# ================================================================================================ the step classes
def _recording(cls):
    class Recording(cls):
        """Copies the step's own gradient (and the state the update starts from) before the optimiser runs; `poison` puts a
        non-finite value into the flat gradient between the backward pass and the optimiser."""
        poison = None

        def _optimizer_step(self, scale):
            torch.cuda.synchronize()
            if self.poison is not None and bool(torch.isfinite(self.flat.grad).all()):
                self.flat.grad[self.poison[0]] = self.poison[1]
                self.poisoned = True
            opt = self.opt
            self.seen = dict(grad=self.flat.grad.cpu().clone(), scale=scale, p=self.flat.flat.cpu().clone(),
                             loss_scale=1.0 if self.scaler is None else float(self.scaler.state[0]), lr_index=self._opt_calls)
            self.seen["state"] = {k: getattr(opt, k).cpu().clone() for k in ("buf", "m", "v") if getattr(opt, k, None) is not None}
            super()._optimizer_step(scale)
    return Recording


def _torch_one_step(kind, state, g, hp, step, max_norm, dtype):
    """clip_grad_norm_ + torch.optim.SGD / AdamW, one step from `state` in `dtype` -> p'."""
    f = lambda x: float(np.float32(x))
    p = torch.nn.Parameter(state["p"].to(dtype).clone())
    p.grad = g.to(dtype).clone()
    if kind == "sgd":
        opt = torch.optim.SGD([p], lr=f(hp["lr"]), momentum=f(hp["mu"]), nesterov=hp["nesterov"], weight_decay=f(hp["wd"]))
        if step > 1:
            opt.state[p]["momentum_buffer"] = state["buf"].to(dtype).clone()
    else:
        opt = torch.optim.AdamW([p], lr=f(hp["lr"]), betas=(f(hp["b1"]), f(hp["b2"])), eps=f(hp["eps"]), weight_decay=f(hp["wd"]))
        opt.state[p] = dict(step=torch.tensor(float(step - 1), dtype=dtype), exp_avg=state["m"].to(dtype).clone(),
                            exp_avg_sq=state["v"].to(dtype).clone())
    torch.nn.utils.clip_grad_norm_([p], max_norm)
    opt.step()
    return p.detach()


def _step_case(which, mode, **kw):
    from oracle import ref_cpu as O
    from mednet_hip.unet import model as HM
    if which == "seg":
        net = O.keyed_init_(HM.ResidualUNet3D(1, 3, False, f_maps=[16, 32])).to(DEV)
        batches = [{k: v.to(DEV) for k, v in O.synthetic_batch(2, 1, (16, 16, 16), 3, 0, seed=900 + i).items()} for i in range(3)]
        return _recording(SegmentationStep)(net, loss_weight=[0.05, 1.0, 1.0], **kw), batches
    net = O.keyed_init_(HM.ResidualUNet3D(1, 4, False, f_maps=[16, 32])).to(DEV)
    batches = [{k: v.to(DEV) for k, v in O.synthetic_batch(2, 1, (16, 16, 16), 2, 2, seed=900 + i).items()} for i in range(3)]
    return _recording(LandmarkStep)(net, [0.05, 1.0], [0.015] * 2, "L2", **kw), batches


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("which,kind", [("seg", "sgd"), ("landmark", "adamw")])
def test_step_classes_against_clip_grad_norm_and_torch_optim(which, kind, mode):
    hp = dict(lr=1e-2, mu=0.99, nesterov=True, wd=3e-5) if kind == "sgd" else dict(ADAM, lr=1e-3, wd=1e-2)
    args = dict(momentum=0.99, nesterov=True, weight_decay=3e-5) if kind == "sgd" else dict(weight_decay=1e-2)
    sched = PolyLR(hp["lr"], 10)
    with mednet_hip.precision(mode):
        probe, batches = _step_case(which, mode, optimizer=kind, optimizer_args=args, lr=0.0, skip_nonfinite=True)
        assert (probe.scaler is not None) == (mode == "fp16")
        probe(batches[0])
        first = float(probe.grad_norm)
        assert np.isfinite(first) and first > 0, f"the probe's gradient norm is {first}"
        probe.flat.release()
        clip = 0.5 * first                                            # below the first step's observed norm: the clip is active
        step, batches = _step_case(which, mode, optimizer=kind, optimizer_args=args, lr=sched, clip_grad_norm=clip)
        count, taken = step.flat.total, 0
        rows = OU.rows_of(count)
        for k, batch in enumerate(batches):
            step(batch)
            norm_dev = step.grad_norm                                 # a device scalar: nothing synchronises here
            assert norm_dev.is_cuda and norm_dev.dim() == 0
            seen = step.seen
            assert seen["lr_index"] == k and step.opt.lr == sched(k)
            gscale = seen["scale"] / seen["loss_scale"]
            g = seen["grad"].double() * gscale                        # the unscaled mean gradient, exact in fp64
            assert bool(torch.isfinite(g).all()), "a non-finite gradient in a clean run"
            taken += 1
            hp_k = dict(hp, lr=sched(k))
            before = dict(seen["state"], p=seen["p"])
            if kind == "sgd" and taken == 1:
                before["buf"] = torch.zeros_like(seen["p"])
            want64 = _torch_one_step(kind, before, g, hp_k, taken, clip, torch.float64)
            # the per-tensor rule's eps: max(2^-20, 8 r32), r32 the error of the restatement's update in fp32 (torch's own step in
            # fp64 is that restatement, asserted below; its fp32 step is not used: the rounding of p' itself would swamp the update's)
            ref = OU.update_reference(kind, before, seen["grad"], hp_k, taken, gscale, clip)
            if k == 0:
                assert ref.coef < 1.0
            assert float((want64 - ref.r64.p).abs().max()) <= 1e-12 * float(want64.abs().max())
            r32, eps = ref.r32s["p"], ref.eps["p"]
            got = step.flat.flat.cpu()
            ratio = U.check_gradient(got, want64, ref.r64.terms_d, eps, f"{which} {kind} {mode} call {k}: parameters", u=OU.U32)
            norm64 = float(g.norm())
            e_n = abs(float(norm_dev) - norm64) / norm64
            assert e_n <= OU.norm_bound(count, rows, 0), f"grad_norm {float(norm_dev)!r} against {norm64!r}"
            print(f"[bound] step {which} {kind} {mode} call={k} count={count} coef {ref.coef:.4f} norm seen {e_n:.2e} "
                  f"p: r32 {r32:.2e} eps {eps:.2e} seen {ratio:.2e}")
        assert step.skipped_steps() == 0 and step.opt.steps_taken(step.scaler) == 3
        step.flat.release()


def test_a_bad_batch_is_skipped_in_bf16_storage():
    """An out-of-range label under skip_nonfinite=True: the parameters, the momentum buffer and the step count stay as they are."""
    with mednet_hip.precision("bf16"):
        step, batches = _step_case("seg", "bf16", optimizer="sgd", optimizer_args=dict(momentum=0.9), lr=1e-2, skip_nonfinite=True)
        assert step.scaler is None
        step(batches[0])
        p1, buf1 = step.flat.flat.clone(), step.opt.buf.clone()
        bad = {k: v.clone() for k, v in batches[1].items()}
        bad["label"][0, -1, 3, 4, 5] = 200
        step.poison = (step.flat.offsets[-1], float("nan"))          # used only if that label leaves every gradient finite
        step.poisoned = False
        step(bad)
        torch.cuda.synchronize()
        print(f"[bound] bad batch: the label made the gradient non-finite: {not step.poisoned}")
        assert not bool(torch.isfinite(step.seen["grad"]).all())
        assert torch.equal(step.flat.flat.view(torch.int32), p1.view(torch.int32)) and torch.equal(step.opt.buf.view(torch.int32), buf1.view(torch.int32))
        assert step.skipped_steps() == 1 and step.opt.steps_taken() == 1
        assert not np.isfinite(float(step.grad_norm))
        step.poison = None
        step(batches[2])
        assert step.skipped_steps() == 1 and step.opt.steps_taken() == 2 and not torch.equal(step.flat.flat, p1)
        assert bool(torch.isfinite(step.flat.flat).all())
        step.flat.release()


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_a_checkpoint_behind_the_loss_scaler_resumes_bit_for_bit(kind):
    """fp16 storage, the guarded FlatAdam / FlatSGD behind the LossScaler: two calls, state_dict, a fresh step with the parameters copied
    and load_state_dict -- its third call leaves the bits of the uninterrupted run in parameters, buffers, optimiser and scaler state."""
    args = dict(weight_decay=1e-2) if kind == "adamw" else dict(momentum=0.99, nesterov=True, weight_decay=3e-5)
    kw = dict(optimizer=kind, optimizer_args=args, lr=1e-2, clip_grad_norm=0.5)
    bits = lambda t: t.detach().view(torch.int32).cpu()

    def state(step):
        bufs = {k: bits(getattr(step.opt, k)) for k in ("buf", "m", "v") if getattr(step.opt, k, None) is not None}
        return dict(p=bits(step.flat.flat), ost=bits(step.opt.opt_state), scaler=bits(step.scaler.state), **bufs)

    with mednet_hip.precision("fp16"):
        step, batches = _step_case("seg", "fp16", **kw)
        assert step.scaler is not None and step.opt.guarded
        step(batches[0])
        step(batches[1])
        sd, params = step.opt.state_dict(step.scaler), step.flat.flat.clone()
        assert sd["t"] == step.opt.steps_taken(step.scaler) == 2
        step(batches[2])
        want = state(step)
        step.flat.release()
        fresh, _ = _step_case("seg", "fp16", **kw)
        fresh.flat.flat.copy_(params)
        fresh.opt.load_state_dict(sd, fresh.scaler)
        fresh(batches[2])
        got = state(fresh)
        fresh.flat.release()
    assert got.keys() == want.keys() and sorted(got) == sorted(["p", "ost", "scaler"] + (["m", "v"] if kind == "adamw" else ["buf"]))
    for k in want:
        assert torch.equal(got[k], want[k]), f"{kind}: {k} differs after the round trip"
    assert fresh.opt.steps_taken(fresh.scaler) == 3 and not torch.equal(want["p"], bits(params))
