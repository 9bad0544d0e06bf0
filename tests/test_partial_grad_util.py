"""tests/partial_grad_util.py on the CPU: with plain torch stand-ins for an autograd node (an affine map with a skip input) and for a
flat-buffer trainer over a tiny model, each checker passes the clean case and rejects every fault it is there for:
  a None for a wanted gradient; a gradient returned or written for an unwanted input; a wanted gradient one element off the
  all-wanted one; a trainable flat slice left at its previous content; a slice accumulated instead of overwritten; a frozen
  parameter moved by the optimizer; padding between the slices written; requires_grad changed after construction."""
import pytest
import torch
import torch.nn as nn

import partial_grad_util as P
from mednet_hip.train import FlatParams

NAMES = ("x", "w", "b", "skip")


# ------------------------------------------------------------------------------------------------- node level
def _operands():
    g = torch.Generator().manual_seed(5)
    return dict(x=torch.randn(7, 5, generator=g), w=torch.randn(3, 5, generator=g), b=torch.randn(3, generator=g),
                skip=torch.randn(7, 3, generator=g), cot=torch.randn(7, 3, generator=g))


def _node(wanted, dtype=torch.float32):
    """The stand-in node y = x w^T + b + skip under torch autograd, requires_grad on `wanted` only -> {name: gradient or None}."""
    o = _operands()
    leaf = {k: o[k].to(dtype).clone().requires_grad_(k in wanted) for k in NAMES}
    y = leaf["x"] @ leaf["w"].t() + leaf["b"] + leaf["skip"]
    (y * o["cot"].to(dtype)).sum().backward()
    return {k: leaf[k].grad for k in NAMES}


def test_the_enumerator_lists_every_non_empty_subset_once():
    subs = P.subsets(NAMES)
    assert len(subs) == 15 and len(set(subs)) == 15 and subs[0] == ("x",) and subs[-1] == NAMES
    assert all(s == tuple(k for k in NAMES if k in s) for s in subs)
    assert P.subsets(("a",)) == [("a",)]


@pytest.mark.parametrize("wanted", P.subsets(NAMES))
def test_check_partial_passes_the_clean_node_and_rejects_each_fault(wanted):
    full, ref = _node(NAMES), _node(wanted, torch.float64)
    seen = P.check_partial(_node(wanted), full, ref, wanted, 1e-6, "clean")
    assert set(seen) == set(wanted) and max(seen.values()) <= 1e-6
    victim = wanted[-1]
    # None for a wanted gradient: the bias bug
    got = _node(wanted)
    got[victim] = None
    with pytest.raises(AssertionError, match="no gradient"):
        P.check_partial(got, full, ref, wanted, 1e-6, "none")
    # a gradient for an input that did not ask
    others = [k for k in NAMES if k not in wanted]
    if others:
        got = _node(wanted)
        got[others[0]] = torch.zeros_like(full[others[0]])
        with pytest.raises(AssertionError, match="did not ask"):
            P.check_partial(got, full, ref, wanted, 1e-6, "unasked")
    # one element one ulp off the all-wanted gradient: far inside the tolerance, only bit equality sees it
    got = _node(wanted)
    flat = got[victim].view(-1)
    flat[flat.numel() // 2] = torch.nextafter(flat[flat.numel() // 2], torch.tensor(float("inf")))
    with pytest.raises(AssertionError, match="bit-identical"):
        P.check_partial(got, full, ref, wanted, 1e-6, "one element")
    # ... a named route exempts it from bit equality, and only from that
    P.check_partial(got, full, ref, wanted, 1e-6, "route", routes={victim: "another kernel"})
    flat[0] += 1.0
    with pytest.raises(AssertionError, match="rel-L2"):
        P.check_partial(got, full, ref, wanted, 1e-6, "route, wrong", routes={victim: "another kernel"})
    # an unwritten (NaN) element, and a reference that does not follow the flags
    got = _node(wanted)
    got[victim].view(-1)[0] = float("nan")
    with pytest.raises(AssertionError, match="not finite"):
        P.check_partial(got, full, ref, wanted, 1e-6, "nan")
    with pytest.raises(AssertionError, match="does not follow the flags"):
        P.check_partial(_node(wanted), full, _node(NAMES, torch.float64) if len(wanted) < 4 else _node(("x",), torch.float64), wanted,
                        1e-6, "reference")


def test_same_bits_sees_the_sign_of_zero_and_the_dtype():
    z = torch.zeros(3)
    assert P.same_bits(z, z.clone()) and not P.same_bits(z, -z) and not P.same_bits(z, z.double()) and not P.same_bits(z, torch.zeros(4))


# ------------------------------------------------------------------------------------------------- trainer level
class _Tiny(nn.Module):
    """Four parameters, none a multiple of 64 elements, so every slice is followed by padding."""

    def __init__(self):
        super().__init__()
        self.enc = nn.Linear(5, 9)
        self.dec = nn.Linear(9, 3)

    def forward(self, x):
        return self.dec(torch.tanh(self.enc(x)))


def _tiny(frozen):
    torch.manual_seed(3)
    m = _Tiny()
    for k, p in m.named_parameters():
        p.requires_grad = k not in frozen
    return m


def _batch():
    g = torch.Generator().manual_seed(9)
    return torch.randn(11, 5, generator=g), torch.randn(11, 3, generator=g)


def _loss(model):
    x, y = _batch()
    return (model(x) - y).square().mean()


class _Trainer:
    """The stand-in for a step class over train.FlatParams: autograd's gradients are written into the `_mednet_grad` slices (the
    kernels' part), then one Adam-like update runs over the WHOLE flat buffer.  `fault` at step `at` (0-based) and later."""

    def __init__(self, model, fault=None, at=0):
        self.model, self.flat, self.fault, self.at, self.t = model, FlatParams(model), fault, at, 0
        self.m = torch.zeros_like(self.flat.flat)

    def __call__(self, i):
        flat, faulty = self.flat, self.fault is not None and i >= self.at
        loss = _loss(self.model)
        grads = torch.autograd.grad(loss, flat.params)
        for k, (p, g) in enumerate(zip(flat.params, grads)):
            hit = faulty and k == len(flat.params) - 1
            if hit and self.fault in ("none", "stale"):
                continue
            if hit and self.fault == "accumulate":
                p._mednet_grad.add_(g)
                continue
            p._mednet_grad.copy_(g)
            if hit and self.fault == "one element":
                p._mednet_grad.view(-1)[0] += 1e-2
        frozen = [p for p in self.model.parameters() if not p.requires_grad]
        if faulty and self.fault == "padding":
            flat.grad[flat.offsets[1] - 1] = 1.0
        if faulty and self.fault == "frozen written" and frozen:
            frozen[0]._mednet_grad = torch.zeros_like(frozen[0])
        if faulty and self.fault == "frozen grad" and frozen:
            frozen[0].grad = torch.zeros_like(frozen[0])
        with torch.no_grad():
            self.m.mul_(0.9).add_(flat.grad, alpha=0.1)
            flat.flat.sub_(1e-2 * self.m.clamp(-1, 1))
            if faulty and self.fault == "frozen moved" and frozen:
                frozen[0].view(-1)[0] += 1e-3
            if faulty and self.fault == "freeze later":
                flat.params[0].requires_grad = False
            if faulty and self.fault == "thaw later" and frozen:
                frozen[0].requires_grad = True
        return float(loss.detach())


def _oracle_grads(frozen):
    m = _tiny(frozen).double()
    _loss_d = (m(_batch()[0].double()) - _batch()[1].double()).square().mean()
    _loss_d.backward()
    return {k: p.grad for k, p in m.named_parameters() if p.grad is not None}


def _hold(frozen, fault=None, at=0, full=None):
    def start():
        model = _tiny(frozen)
        tr = _Trainer(model, fault, at)
        return model, tr.flat, tr, tr.flat.release
    return P.hold_steps(start, f"tiny {sorted(frozen)} {fault}", ref=_oracle_grads(frozen), tol=1e-6, full=full)


SCENARIOS = [(), ("enc.weight", "enc.bias"), ("dec.weight",), ("enc.weight", "dec.weight"), ("enc.bias", "dec.weight", "enc.weight")]


@pytest.mark.parametrize("frozen", SCENARIOS)
def test_check_step_passes_the_clean_trainer(frozen):
    _, full, _ = _hold(())
    losses, first, seen = _hold(frozen, full=full)
    assert len(losses) == 2 and losses[1] < losses[0]
    assert set(first) == {k for k in ("enc.weight", "enc.bias", "dec.weight", "dec.bias") if k not in frozen}
    assert seen == {}       # (every slice was held to the all-trainable run bit for bit, none fell back to the reference)
    _, _, seen = _hold(frozen)
    assert set(seen) == set(first) and max(seen.values()) <= 1e-6


@pytest.mark.parametrize("fault,at,match", [
    ("none", 0, "rel-L2"),                              # the slice of a wanted gradient never written: zeros against the oracle
    ("stale", 1, "still hold the sentinel"),            # written at step 1, left at its previous content at step 2
    ("accumulate", 1, "depends on what the buffer held"),
    ("one element", 0, "rel-L2"),
    ("padding", 0, "padding elements"),
    ("padding", 1, "padding elements"),
    ("frozen moved", 1, "frozen parameter 'enc.weight' changed"),
    ("frozen written", 0, "carries a gradient target"),
    ("frozen grad", 1, "received a .grad"),
    ("freeze later", 0, "requires_grad of 'enc.bias' changed to False"),
    ("thaw later", 1, "requires_grad of 'enc.weight' changed to True"),
])
def test_check_step_rejects_each_fault(fault, at, match):
    with pytest.raises(AssertionError, match=match):
        _hold(("enc.weight",), fault, at)


def test_check_step_holds_a_slice_to_the_all_trainable_run_bit_for_bit():
    _, full, _ = _hold(())
    with pytest.raises(AssertionError, match="not bit-identical to the all-trainable"):
        def start():
            model = _tiny(("enc.weight",))
            tr = _Trainer(model)
            first = tr.flat.params[-1]._mednet_grad

            def call(i):
                out = tr(i)
                first.view(-1)[1] = torch.nextafter(first.view(-1)[1], torch.tensor(float("inf")))
                return out
            return model, tr.flat, call, tr.flat.release
        P.hold_steps(start, "one ulp", full=full)
    # a named route falls back to the reference, and needs one
    with pytest.raises(AssertionError, match="need a reference"):
        def start2():
            model = _tiny(("enc.weight",))
            tr = _Trainer(model)
            return model, tr.flat, tr, tr.flat.release
        P.hold_steps(start2, "route", full=full, routes={"dec.bias": "another kernel"})


def test_check_step_wants_the_reference_to_name_the_trainable_parameters():
    with pytest.raises(AssertionError, match="does not train"):
        def start():
            model = _tiny(("enc.weight",))
            tr = _Trainer(model)
            return model, tr.flat, tr, tr.flat.release
        P.hold_steps(start, "names", ref=_oracle_grads(()), tol=1e-6)


def test_flat_params_records_the_flags_and_verify_names_the_first_change():
    for frozen, flip, now in ((("enc.weight",), "dec.weight", False), (("enc.weight",), "enc.weight", True)):
        model = _tiny(frozen)
        flat = FlatParams(model)
        flat.verify()
        assert flat.total == P.flat_layout(model)[1] and all(p is q for p, (_, q, _) in zip(flat.params, P.flat_layout(model)[0]))
        dict(model.named_parameters())[flip].requires_grad = now
        with pytest.raises(RuntimeError, match=f"'{flip}' changed from {not now} to {now}.*rebuild the step"):
            flat.verify()
        flat.release()
    with pytest.raises(RuntimeError, match="no trainable parameter"):
        FlatParams(_tiny(("enc.weight", "enc.bias", "dec.weight", "dec.bias")))


@pytest.mark.parametrize("name,now", [("final_conv.bias", False), ("encoders.0.basic_module.conv2.conv.weight", True)])
def test_the_step_classes_refuse_a_call_after_a_flag_changed(name, now):
    """Both directions, on the host alone: the check runs before the step touches the batch or the device."""
    from mednet_hip.train import LandmarkStep, SegmentationStep
    from mednet_hip.unet import model as HM
    for make in (lambda net: SegmentationStep(net, loss_weight=[0.05, 1.0], graph=False),
                 lambda net: LandmarkStep(net, class_weight=[0.05, 1.0], regression_weight=[0.015], graph=True)):
        net = HM.ResidualUNet3D(in_channels=1, out_channels=2, final_sigmoid=False, f_maps=[8])
        for k, p in net.named_parameters():
            p.requires_grad = not k.startswith("encoders.")
        step = make(net)
        step.flat.verify()
        dict(net.named_parameters())[name].requires_grad = now
        with pytest.raises(RuntimeError, match=f"'{name}' changed from {not now} to {now}.*rebuild the step"):
            step({})
        step.flat.release()
