"""The helpers of the optimiser tests (tests/optim_util.py) on the CPU: the fp64 restatements equal torch.optim.SGD / Adam / AdamW and
torch.nn.utils.clip_grad_norm_ over five steps, the numpy model of the norm pass shows every fp32 partial exact on the lattice
inputs of the GPU tests, and the checkers reject each fault they are there for."""
import numpy as np
import pytest
import torch

import optim_util as OU

ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def _torch_run(make, p0, grads, max_norm=None):
    p = torch.nn.Parameter(p0.double().clone())
    opt = make([p])
    coefs = []
    for g in grads:
        p.grad = g.double().clone()
        if max_norm is not None:
            before = p.grad.clone()
            torch.nn.utils.clip_grad_norm_([p], max_norm)
            nz = before != 0
            coefs.append(float((p.grad[nz] / before[nz]).mean()))
        opt.step()
    return p.detach(), coefs


def _close(a, b, what, tol=1e-12):
    err = float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))
    assert err <= tol, f"{what}: {err:.3e}"


@pytest.mark.parametrize("wd", [0.0, 3e-5])
@pytest.mark.parametrize("mu,nesterov", [(0.0, False), (0.9, False), (0.9, True), (0.99, False), (0.99, True)])
def test_sgd_restatement_is_torch_optim_sgd(mu, nesterov, wd):
    p0, gs = OU.random_case(f"sgd{mu}{nesterov}{wd}", 257)
    # (the restatement takes the fp32 numbers the C ABI receives: torch gets the same ones)
    f = lambda x: float(np.float32(x))
    want, _ = _torch_run(lambda ps: torch.optim.SGD(ps, lr=f(1e-2), momentum=f(mu), nesterov=nesterov, weight_decay=f(wd)), p0, gs)
    ref = OU.Reference("sgd", p0, dict(lr=1e-2, mu=mu, nesterov=nesterov, wd=wd))
    for g in gs:
        assert ref.step(g)
    _close(ref.p, want, f"SGD mu={mu} nesterov={nesterov} wd={wd}")
    assert ref.steps == 5 and ref.skipped == 0


@pytest.mark.parametrize("kind,wd", [("adam", 0.0), ("adam", 1e-2), ("adamw", 1e-2), ("adamw", 0.0)])
def test_adam_restatements_are_torch_optim_adam_and_adamw(kind, wd):
    p0, gs = OU.random_case(f"{kind}{wd}", 257)
    f = lambda x: float(np.float32(x))
    cls = torch.optim.AdamW if kind == "adamw" else torch.optim.Adam
    want, _ = _torch_run(lambda ps: cls(ps, lr=f(1e-3), betas=(f(0.9), f(0.999)), eps=f(1e-8), weight_decay=f(wd)), p0, gs)
    ref = OU.Reference(kind, p0, dict(ADAM, wd=wd))
    for g in gs:
        ref.step(g)
    _close(ref.p, want, f"{kind} wd={wd}")


def test_clip_coefficient_is_clip_grad_norm():
    p0, gs = OU.random_case("clip", 257)
    norms = [float(g.double().norm()) for g in gs]
    max_norm = float(np.median(norms)) * 0.5          # active on every step
    want, coefs = _torch_run(lambda ps: torch.optim.SGD(ps, lr=float(np.float32(1e-2))), p0, gs, max_norm)
    ref = OU.Reference("sgd", p0, dict(lr=1e-2), max_norm=max_norm)
    for g, c, n in zip(gs, coefs, norms):
        ref.step(g)
        assert abs(ref.coef - c) <= 1e-12 and ref.coef < 1.0 and abs(ref.norm - n) <= 1e-12 * n
    _close(ref.p, want, "clipped SGD")
    assert OU.clip_coef(3.0, None) == 1.0 and OU.clip_coef(1.0, 12.0) == 1.0 and OU.clip_coef(24.0, 12.0) == 12.0 / (24.0 + 1e-6)


def test_loss_scale_and_world_fold_into_the_gradient_before_the_norm():
    """A gradient that arrives times 2^16 from two ranks' sum: the reference unscales first, so norm and update are the unscaled ones."""
    p0, gs = OU.random_case("fold", 129)
    plain = OU.Reference("sgd", p0, dict(lr=1e-2, mu=0.9), max_norm=1.0)
    scaled = OU.Reference("sgd", p0, dict(lr=1e-2, mu=0.9), max_norm=1.0, inv_world=0.5, scaler=[65536.0, 0, 0, 0, 0], rule=(2.0, 0.5, 2))
    for g in gs[:2]:
        plain.step(g)
        scaled.step(g * 131072.0)
        assert scaled.norm == plain.norm and scaled.coef == plain.coef
    assert torch.equal(plain.p, scaled.p)
    assert scaled.scaler == [131072.0, 0.0, 2.0, 0.0, 0]          # two clean steps at growth_interval 2 doubled the scale


# ------------------------------------------------------------------------------------------------ the norm pass, modelled
def _counts():
    return [1, 3, 4, 255, 1024, 1025, OU.max_rows_count(), OU.ragged_count()]


def test_plan_numbers_are_the_librarys():
    assert OU.rows_of(OU.max_rows_count()) == OU.MAX_ROWS and OU.rows_of(OU.max_rows_count() - 1) == OU.MAX_ROWS - 1
    assert OU.rows_of(OU.ragged_count()) == OU.MAX_ROWS and OU.rows_of(1 << 31) == OU.MAX_ROWS
    for count in (1, 4096, 4097, 1025):
        assert OU.rows_of(count) == -(-count // OU.PER_ROW)
    assert OU.rows_of(0) == 0


@pytest.mark.parametrize("count", _counts())
def test_every_partial_is_exact_on_the_lattice_inputs(count):
    g = OU.lattice_grad(f"lat{count}", count, e=-3)
    rows = OU.rows_of(count)
    for offset in ((0, 1, 2, 3) if count <= 1025 else (0, 3)):
        head = OU.head_of(offset)
        part, chain, exact = OU.norm_model(g, 1.0, rows, head)
        assert exact, f"count {count} offset {offset}: an fp32 addition of the model was not exact"
        assert chain <= OU.chain_length(count, rows, head)
        assert float(part.max()) * 64 < 2 ** 24          # (integers, in units of 4^-3, far below 2^24)
        OU.check_norm_exact(OU.finalize64(part, None), g, 1.0, f"model count {count} offset {offset}")
    assert OU.chain_length(count, rows, 0) <= 4 * 5 + 1


def test_the_model_covers_every_element_once():
    """A single non-zero element anywhere is found with its exact square (head, body, tail; first and last workgroup)."""
    count = 3 * OU.PER_ROW + 7
    rows = OU.rows_of(count)
    for head in (0, 1, 3):
        for i in (0, 1, 2, 3, 4, 5000, count - 5, count - 4, count - 1):
            g = np.zeros(count, dtype=np.float32)
            g[i] = 3.0
            part, _, _ = OU.norm_model(g, 1.0, rows, head)
            assert float(part.sum()) == 9.0, (head, i)


@pytest.mark.parametrize("fault,count", [("skip_last", 1024), ("skip_last", 1025), ("drop_tail", 1025), ("drop_tail", 3)])
def test_norm_checker_rejects_a_skipped_element(fault, count):
    g = OU.lattice_grad(f"lat{count}", count)
    g[-1] = 3.0
    part, _, _ = OU.norm_model(g, 1.0, OU.rows_of(count), 0, fault=fault)
    with pytest.raises(AssertionError, match="sumsq"):
        OU.check_norm_exact(OU.finalize64(part, None), g, 1.0, fault)


def test_norm_bound_terms():
    count, rows = OU.ragged_count(), OU.MAX_ROWS
    k = OU.sumsq_terms(count, rows, 0)
    assert k == 2 + OU.chain_length(count, rows, 0) + 14 and OU.gamma(k) < 4e-6 and OU.norm_bound(count, rows, 0) < 2.2e-6
    g = np.random.default_rng(5).standard_normal(50001).astype(np.float32)
    rows = OU.rows_of(g.size)
    part, chain, _ = OU.norm_model(g, 1.0, rows, 1)
    assert chain <= OU.chain_length(g.size, rows, 1)
    OU.check_norm_random(OU.finalize64(part, None), g.astype(np.float64), g.size, rows, 1, "model, random")


# ------------------------------------------------------------------------------------------------ the update checkers
def _run(kind, hp, p0, gs, fault=None, dtype=torch.float64, **kw):
    ref = OU.Reference(kind, p0, hp, fault=fault, dtype=dtype, **kw)
    for g in gs:
        ref.step(g)
    return ref


def test_bit_checker_rejects_a_missing_nesterov_term():
    p0, gs = OU.dyadic_case("dy", 300)
    hp = dict(lr=OU.DYADIC["lr"], mu=OU.DYADIC["mu"], nesterov=True, wd=OU.DYADIC["wd"])
    good, bad = _run("sgd", hp, p0, gs), _run("sgd", hp, p0, gs, fault="no_nesterov")
    OU.check_bits({k: v.float() for k, v in good.state().items()}, good.state(), "exact SGD")
    with pytest.raises(AssertionError, match="differs"):
        OU.check_bits({k: v.float() for k, v in bad.state().items()}, good.state(), "no Nesterov term")


def test_tolerance_checker_rejects_coupled_decay_and_a_clip_before_the_unscale():
    p0, gs = OU.random_case("tol", 1000)
    state = dict(p=p0, m=0.1 * gs[1], v=0.01 * gs[2] ** 2)
    hp = dict(ADAM, wd=1e-2)
    ref = OU.update_reference("adamw", state, gs[0], hp, 3, 1.0, None)
    as32 = lambda r: dict(p=r.p.float(), m=r.m.float(), v=r.v.float())
    OU.check_update("adamw", ref, as32(ref.r32), hp, "fp32 restatement")
    with pytest.raises(AssertionError, match="outside"):
        OU.check_update("adamw", ref, as32(OU.one_step("adamw", state, gs[0], hp, 3, 1.0, 1.0, torch.float32, fault="coupled")), hp, "coupled")
    # clip before the unscale: the coefficient comes from the norm of the gradient times the loss scale
    scale, max_norm = 1024.0, 8.0
    g = gs[0] * scale
    ref = OU.update_reference("sgd", dict(p=p0), g, dict(lr=1e-2), 1, 1.0 / scale, max_norm)
    assert ref.coef < 1.0
    OU.check_update("sgd", ref, dict(p=ref.r32.p.float()), dict(lr=1e-2), "fp32 restatement")
    wrong = OU.Reference("sgd", p0, dict(lr=1e-2), max_norm=max_norm, scaler=[scale, 0, 0, 0, 0], fault="clip_before_unscale", dtype=torch.float32)
    wrong.step(g)
    with pytest.raises(AssertionError, match="outside"):
        OU.check_update("sgd", ref, dict(p=wrong.p.float()), dict(lr=1e-2), "clip before unscale")


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_skip_checkers_reject_an_update_and_a_count_on_a_nonfinite_step(bad):
    p0, gs = OU.random_case("skip", 100)
    hp = dict(lr=1e-2, mu=0.9)
    gs[1][37] = bad
    good = OU.Reference("sgd", p0, hp, dtype=torch.float32)
    good.step(gs[0])
    before = {k: v.clone() for k, v in good.state().items()}
    assert not good.step(gs[1])
    OU.check_unchanged(good.state(), before, "skipped")
    OU.check_counts(good.steps, good.skipped, 1, 1, "skipped")
    for fault, match in (("no_skip", "changed on a skipped step"), ("count_on_skip", "steps taken")):
        wrong = OU.Reference("sgd", p0, hp, dtype=torch.float32, fault=fault)
        wrong.step(gs[0])
        wrong.step(gs[1])
        with pytest.raises(AssertionError, match=match):
            OU.check_unchanged(wrong.state(), before, fault)
            OU.check_counts(wrong.steps, wrong.skipped, 1, 1, fault)
    # a finite gradient whose square overflows fp32 is skipped as well
    huge = gs[2].clone()
    huge[5] = 3.0e19
    assert not good.step(huge) and good.skipped == 2
