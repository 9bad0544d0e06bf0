"""Host logic of the optimiser options, without a GPU: PolyLR against its closed form, a callable lr evaluated once per call,
FlatSGD's state-dict round trip and its refusal, unknown / conflicting arguments, and the default construction: a plain FlatAdam
whose step reaches ops.adam_step_ with the arguments it always got."""
import pytest
import torch

from test_ddp_gloo import _cpu_hybrid_of_product_model, _torch_adam_step_


def test_poly_lr_closed_form():
    from mednet_hip.train import PolyLR
    lr = PolyLR(1e-2, 1000)
    assert lr(0) == 1e-2
    assert lr(500) == 1e-2 * (1 - 500 / 1000) ** 0.9
    assert lr(999) == 1e-2 * (1 - 999 / 1000) ** 0.9 > 0
    assert lr(1000) == 0.0 and lr(1500) == 0.0
    assert PolyLR(0.5, 10, power=2.0)(5) == 0.5 * 0.25
    assert [PolyLR(1.0, 4, power=1.0)(k) for k in range(5)] == [1.0, 0.75, 0.5, 0.25, 0.0]
    with pytest.raises(ValueError):
        PolyLR(1e-2, 0)


def _cpu_step(monkeypatch, **kw):
    from oracle import ref_cpu as O
    from mednet_hip import ops
    from mednet_hip.train import SegmentationStep
    calls = []

    def spy(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
        calls.append(dict(lr=lr, betas=(beta1, beta2), eps=eps, wd=weight_decay, step=step, grad_scale=grad_scale))
        _torch_adam_step_(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale)

    monkeypatch.setattr(ops, "adam_step_", spy)
    w = [0.05, 1.0]
    step = SegmentationStep(_cpu_hybrid_of_product_model(O), loss_weight=w, **kw)
    step.loss = O.DiceLoss(weight=torch.tensor(w))   # (the product's DiceLoss is a HIP kernel)
    step.flat.grads_as_attr()
    return step, calls, lambda it: O.synthetic_batch(1, 1, (16, 16, 16), 2, 0, seed=700 + it)


def test_default_construction_is_plain_adam_and_reaches_adam_step(monkeypatch):
    from mednet_hip.train import FlatAdam
    step, calls, batch = _cpu_step(monkeypatch, lr=1e-3)
    assert type(step.opt) is FlatAdam and not step.opt.guarded and step.opt.opt_state is None and not step.opt.decoupled
    assert (step.opt.lr, step.opt.betas, step.opt.eps, step.opt.wd) == (1e-3, (0.9, 0.999), 1e-8, 0.0)
    assert step._lr_fn is None and step.scaler is None
    before = step.flat.flat.clone()
    for it in range(2):
        step.flat.grad.zero_()
        step(batch(it))
    assert calls == [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.0, step=k, grad_scale=1.0) for k in (1, 2)]
    assert not torch.equal(step.flat.flat, before) and step.opt.steps_taken() == 2
    assert step.skipped_steps() == 0
    with pytest.raises(RuntimeError, match="grad_norm"):
        step.grad_norm


def test_a_callable_lr_is_evaluated_once_per_call(monkeypatch):
    from mednet_hip.train import PolyLR
    seen = []
    sched = PolyLR(1e-2, 4)

    def lr(k):
        seen.append(k)
        return sched(k)

    step, calls, batch = _cpu_step(monkeypatch, lr=lr)
    assert seen == []                      # nothing is evaluated at construction
    for it in range(3):
        step.flat.grad.zero_()
        step(batch(it))
    assert seen == [0, 1, 2]
    assert [c["lr"] for c in calls] == [sched(0), sched(1), sched(2)] and step.opt.lr == sched(2)


def _flat(n=24):
    from mednet_hip.train import FlatParams
    return FlatParams(torch.nn.Linear(n, 3))


def test_flat_adam_scaler_round_trip_and_refusals():
    """What test_flat_sgd_state_round_trip_and_refusals does for FlatSGD, on FlatAdam: the shared state-dict code has both on it."""
    from mednet_hip.train import FlatAdam, LossScaler
    opt = FlatAdam(_flat(), lr=1e-2, betas=(0.8, 0.99), eps=1e-6, weight_decay=3e-5, clip_grad_norm=12.0)
    assert opt.guarded and not opt.decoupled and opt.opt_state.tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    opt.m.copy_(torch.arange(opt.m.numel(), dtype=torch.float32))
    opt.v.copy_(torch.arange(opt.v.numel(), dtype=torch.float32) * 0.5)
    opt.opt_state.copy_(torch.tensor([4.0, 2.0, 0.5, 0.0, 7.0, 2.0, 0.0, 0.0]))
    assert opt.steps_taken() == 7
    sd = opt.state_dict()
    assert set(sd) == {"m", "v", "t", "lr", "betas", "eps", "weight_decay", "opt_state"}
    sd["betas"] = list(sd["betas"])                # (as a checkpoint that went through JSON holds them)
    opt2 = FlatAdam(_flat(), lr=1.0, skip_nonfinite=True)
    opt2.load_state_dict(sd)
    assert (opt2.lr, opt2.betas, opt2.eps, opt2.wd, opt2.t) == (1e-2, (0.8, 0.99), 1e-6, 3e-5, 7)
    assert torch.equal(opt2.m, opt.m) and torch.equal(opt2.v, opt.v) and torch.equal(opt2.opt_state, opt.opt_state)
    assert opt2.steps_taken() == 7
    sc = LossScaler("cpu")
    with pytest.raises(KeyError, match="scaler"):
        opt2.load_state_dict(sd, scaler=sc)        # saved without a scaler: resuming WITH one must not restart at 65536
    sc.state[0], sc.state[2], sc.state[4] = 1024.0, 5.0, 2.0
    sd_s = opt.state_dict(scaler=sc)
    assert sd_s["t"] == 5 and "scaler" in sd_s
    sc2 = LossScaler("cpu")
    opt2.load_state_dict(sd_s, scaler=sc2)
    assert torch.equal(sc2.state, sc.state) and opt2.steps_taken(sc2) == 5 and sc2.skipped_steps() == 2
    plain = FlatAdam(_flat(), lr=1e-3)             # the plain form keeps no device state: none in its state dict either
    plain.t = 3
    assert plain.opt_state is None and "opt_state" not in plain.state_dict() and plain.state_dict()["t"] == 3
    plain.load_state_dict(sd)                      # a guarded run's state into the plain form: the host count takes over
    assert plain.steps_taken() == 7 and plain.opt_state is None


def test_flat_sgd_state_round_trip_and_refusals():
    from mednet_hip.train import FlatSGD, LossScaler
    opt = FlatSGD(_flat(), lr=1e-2, momentum=0.99, nesterov=True, weight_decay=3e-5, clip_grad_norm=12.0)
    assert opt.guarded and opt.buf is not None and opt.opt_state.tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    opt.buf.copy_(torch.arange(opt.buf.numel(), dtype=torch.float32))
    opt.opt_state.copy_(torch.tensor([4.0, 2.0, 0.5, 0.0, 7.0, 2.0, 0.0, 0.0]))
    assert opt.steps_taken() == 7
    sd = opt.state_dict()
    opt2 = FlatSGD(_flat(), lr=1.0, momentum=0.5, clip_grad_norm=1.0)
    opt2.load_state_dict(sd)
    assert (opt2.lr, opt2.momentum, opt2.nesterov, opt2.wd, opt2.t) == (1e-2, 0.99, True, 3e-5, 7)
    assert torch.equal(opt2.buf, opt.buf) and torch.equal(opt2.opt_state, opt.opt_state) and opt2.steps_taken() == 7
    sc = LossScaler("cpu")
    with pytest.raises(KeyError, match="scaler"):
        opt2.load_state_dict(sd, scaler=sc)        # saved without a scaler: resuming WITH one must not restart at 65536
    sc.state[2] = 5.0
    sd_s = opt.state_dict(scaler=sc)
    assert sd_s["t"] == 5 and "scaler" in sd_s
    sc2 = LossScaler("cpu")
    opt2.load_state_dict(sd_s, scaler=sc2)
    assert torch.equal(sc2.state, sc.state) and opt2.steps_taken(sc2) == 5
    with pytest.raises(ValueError, match="momentum buffer"):
        FlatSGD(_flat(), lr=1e-2).load_state_dict(sd)
    plain = FlatSGD(_flat(), lr=1e-2)
    assert plain.buf is None and not plain.guarded and plain.state_dict()["buf"] is None
    # a FlatAdam on the guarded path keeps its device state in the state dict too; a plain one's host count becomes the device count
    from mednet_hip.train import FlatAdam
    a = FlatAdam(_flat(), lr=1e-3, skip_nonfinite=True)
    a.opt_state[4], a.opt_state[5] = 9.0, 1.0
    b = FlatAdam(_flat(), lr=1e-3, decoupled_weight_decay=True, weight_decay=1e-2)
    b.load_state_dict(a.state_dict())
    assert b.steps_taken() == 9 and b.opt_state[5] == 1.0
    old = FlatAdam(_flat(), lr=1e-3)
    old.t = 4
    b.load_state_dict(old.state_dict())
    assert b.steps_taken() == 4 and b.opt_state.tolist() == [0, 0, 1, 0, 4, 0, 0, 0]


def test_unknown_and_conflicting_arguments_raise():
    from mednet_hip.train import FlatAdam, FlatSGD, make_optimizer
    flat = _flat()
    with pytest.raises(ValueError, match="optimizer must be"):
        make_optimizer(flat, "lamb")
    with pytest.raises(ValueError, match="argument of the step"):
        make_optimizer(flat, "sgd", dict(lr=1e-2))
    with pytest.raises(ValueError, match="argument of the step"):
        make_optimizer(flat, "adam", dict(clip_grad_norm=1.0))
    with pytest.raises(ValueError, match="conflicts"):
        make_optimizer(flat, "adam", dict(decoupled_weight_decay=True))
    with pytest.raises(ValueError, match="conflicts"):
        make_optimizer(flat, "adamw", dict(decoupled_weight_decay=False))
    with pytest.raises(TypeError):
        make_optimizer(flat, "sgd", dict(betas=(0.9, 0.99)))
    with pytest.raises(ValueError, match="nesterov"):
        FlatSGD(flat, lr=1e-2, nesterov=True)
    for mu in (-0.1, 1.0):
        with pytest.raises(ValueError, match="momentum"):
            FlatSGD(flat, lr=1e-2, momentum=mu)
    for kw in (dict(clip_grad_norm=0.0), dict(clip_grad_norm=-1.0), dict(weight_decay=-1e-3)):
        with pytest.raises(ValueError):
            FlatSGD(flat, lr=1e-2, **kw)
        with pytest.raises(ValueError):
            FlatAdam(flat, **kw)
    opt, lr_fn = make_optimizer(flat, "adamw", dict(weight_decay=1e-2, betas=(0.8, 0.9)), lr=3e-4, skip_nonfinite=True)
    assert type(opt) is FlatAdam and opt.decoupled and opt.guarded and opt.skip_nonfinite and lr_fn is None
    assert (opt.lr, opt.wd, opt.betas) == (3e-4, 1e-2, (0.8, 0.9))
    opt, lr_fn = make_optimizer(flat, "sgd", dict(momentum=0.99, nesterov=True, weight_decay=3e-5), lr=lambda k: 0.1, clip_grad_norm=12.0)
    assert type(opt) is FlatSGD and opt.guarded and opt.clip == 12.0 and lr_fn(3) == 0.1 and opt.lr == 0.0
    opt, _ = make_optimizer(flat)
    assert type(opt) is FlatAdam and not opt.guarded
