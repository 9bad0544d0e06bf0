"""Checkers of tests/test_gpu_partial_grads.py: gradients when only a SUBSET of a node's inputs, or of a model's parameters, wants
one (fine-tuning: frozen encoder, head only, norm affines only, biases only).  tests/test_partial_grad_util.py shows on the CPU, with
plain torch stand-ins, that each checker passes the clean case and fails for every fault it is there for.

Node level (check_partial): an autograd node is run with requires_grad on a subset S of its differentiable inputs and compared with
(a) the same node with every input wanted -- the same kernel ran on the same operands, so every wanted gradient is BIT-identical,
unless the node legitimately takes another kernel route, which the caller names -- and (b) torch autograd of the plain restatement
of the operation under the same flags: None exactly where (b) has None, and within the tolerance of the existing operator test.

Trainer level (StepProbe / check_step): the flat trainer hands every trainable parameter a slice of ONE gradient buffer once, at
construction, and nothing zeroes that buffer between steps.  So every trainable slice must be written in full by exactly one kernel
every step, nothing else in the buffer may be written, and a frozen parameter is neither written nor moved."""
import itertools

import torch

SENTINEL = -7777.0     # what refill() plants in the whole gradient buffer: finite (the fp16 loss scaler tests the buffer for inf / NaN)
ALIGN = 64             # elements: train.FlatParams aligns its slices to 256 bytes


def subsets(names):
    """Every non-empty subset of `names`, as tuples in the order of `names`, smallest first."""
    names = tuple(names)
    return [c for k in range(1, len(names) + 1) for c in itertools.combinations(names, k)]


def rel_l2(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


def same_bits(a, b):
    """Bit-for-bit equality of two tensors of one dtype and shape (+0 and -0 differ, a NaN equals only the same NaN)."""
    if a.dtype != b.dtype or tuple(a.shape) != tuple(b.shape):
        return False
    a, b = a.detach().contiguous().cpu(), b.detach().contiguous().cpu()
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _first_difference(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    bad = (a != b) | (a.isnan() != b.isnan())
    idx = bad.nonzero()
    if idx.numel() == 0:
        return "signs of zero differ"
    i = tuple(idx[0].tolist())
    return f"{int(bad.sum())} of {a.numel()} elements differ; first at {i}: got {a[i].item()!r} want {b[i].item()!r}"


def check_partial(got, full, ref, wanted, tol, what, routes=None):
    """got / full / ref: {input name: gradient or None} of the node with `wanted` inputs requiring a gradient, of the same node with all of
    them, and of autograd on the plain restatement with the SAME flags as `got`.
      - every name: got is None exactly where ref is None, and ref itself is None exactly outside `wanted` (a reference that disagrees
        with the flags it was given is a mistake of the test);
      - every wanted gradient: finite, bit-identical to full[name] unless routes names it (routes: {name: why another kernel ran});
      - every wanted gradient: rel-L2 against ref within tol (a number, or {name: number or None}; None: no bound against ref for
        that tensor, the two rules above still hold).
    -> {name: observed rel-L2}."""
    routes = routes or {}
    wanted = set(wanted)
    assert set(got) == set(ref) == set(full), f"{what}: the three results name different inputs"
    assert wanted <= set(got), f"{what}: wanted {sorted(wanted)} of {sorted(got)}"
    seen = {}
    for name in got:
        g, r = got[name], ref[name]
        assert (r is not None) == (name in wanted), f"{what}: the reference's gradient of '{name}' does not follow the flags"
        if name not in wanted:
            assert g is None, f"{what}: a gradient came back for '{name}', which did not ask for one"
            continue
        assert g is not None, f"{what}: no gradient (None) for '{name}', which wants one (wanted: {sorted(wanted)})"
        assert tuple(g.shape) == tuple(r.shape), f"{what}: gradient of '{name}' has shape {tuple(g.shape)}, not {tuple(r.shape)}"
        assert bool(torch.isfinite(g).all()), f"{what}: the gradient of '{name}' is not finite (an unwritten element?)"
        if name not in routes:
            f = full[name]
            assert f is not None, f"{what}: the all-wanted run has no gradient of '{name}'"
            assert same_bits(g, f), (f"{what}: the gradient of '{name}' with {sorted(wanted)} wanted is not bit-identical to the all-wanted "
                                     f"one: {_first_difference(g, f)}")
        t = tol[name] if isinstance(tol, dict) else tol
        seen[name] = rel_l2(g, r)
        if t is None:     # (the existing operator test holds this tensor to no bound of its own, the caller says why: reported only)
            continue
        assert seen[name] <= t,f"{what}: gradient of '{name}' rel-L2 {seen[name]:.3e} > {t:.1e} against the restatement" + (
            f" (route: {routes[name]})" if name in routes else "")
    return seen


# ------------------------------------------------------------------------------------------------- the flat trainer
def flat_layout(model):
    """The layout train.FlatParams must have for `model` AS ITS FLAGS STAND NOW, restated: the trainable parameters in module order,
    each slice starting at a multiple of ALIGN elements.  -> ([(name, parameter, offset)], total elements)."""
    out, total = [], 0
    for k, p in model.named_parameters():
        if p.requires_grad:
            out.append((k, p, total))
            total += (p.numel() + ALIGN - 1) // ALIGN * ALIGN
    return out, total


class StepProbe:
    """Built right after the training step object (before its first call): remembers the model's flags, a copy of every frozen
    parameter and the packed-weight buffers of the frozen layers, and owns the rule the step is held to (check_step)."""

    def __init__(self, model, flat):
        self.model, self.flat = model, flat
        self.flags = {k: p.requires_grad for k, p in model.named_parameters()}
        self.layout, self.total = flat_layout(model)
        self.frozen = {k: p.detach().clone() for k, p in model.named_parameters() if not p.requires_grad}
        self.pad = torch.ones(self.total, dtype=torch.bool)
        for _, p, off in self.layout:
            self.pad[off:off + p.numel()] = False
        self.pad_value = 0.0      # FlatParams zero-fills; refill() changes it
        self.packs = {}           # name of a layer whose weight is frozen -> the pack buffer it holds now (None: not packed yet)
        for name, m in model.named_modules():
            w = getattr(m, "weight", None)
            if hasattr(m, "_packed") and w is not None and not w.requires_grad:
                self.packs[name] = (m, getattr(m, "_pack_buf", None))

    def refill(self):
        """Plants SENTINEL in every element of the gradient buffer, padding included: the next step must overwrite every trainable
        element (no stale slice, no accumulation) and nothing else."""
        self.flat.grad.fill_(SENTINEL)
        self.pad_value = SENTINEL

    def slices(self):
        """{name: clone of the parameter's slice of flat.grad} by the restated layout."""
        g = self.flat.grad.detach()
        return {k: g[off:off + p.numel()].view_as(p).clone() for k, p, off in self.layout}


def check_step(probe, what, ref=None, tol=None, full=None, routes=None, clean=None):
    """After a call of the training step.  Always:
      - the model's requires_grad flags are what they were when the step was built;
      - flat.total and the slices are those of the trainable parameters ALONE, every `_mednet_grad` is its parameter's slice;
      - every frozen parameter is bit-unchanged, carries no `_mednet_grad` and no .grad;
      - the padding between the slices holds what it held (zeros, or the sentinel after refill()), and no trainable element still holds
        the sentinel;
      - the pack buffer of every layer with a frozen weight is still the one it was: `m._packed()` does not rebuild it.
    ref = {name: gradient} (the oracle's, this step) with tol: every trainable slice within tol rel-L2 of it, and ref names exactly the
    trainable parameters.  full = {name: slice} of the run with everything trainable: every trainable slice bit-identical to it, except
    the names in routes ({name: why another kernel ran}), which need ref.  clean = the whole flat.grad of the same step of a run
    WITHOUT refill(): every trainable element has the same bits (each one was overwritten, none accumulated).  -> {name: rel-L2}."""
    model, flat = probe.model, probe.flat
    routes = routes or {}
    for k, p in model.named_parameters():
        assert p.requires_grad == probe.flags[k], (f"{what}: requires_grad of '{k}' changed to {p.requires_grad} after the step was built: "
                                                   f"its gradient slice was " + ("never handed out" if p.requires_grad else "handed out and is still written"))
    layout, total = flat_layout(model)
    assert flat.total == total == probe.total, f"{what}: flat.total {flat.total} != {total} elements of the trainable parameters alone"
    assert flat.grad.numel() == total and flat.flat.numel() == total, f"{what}: the flat buffers hold {flat.grad.numel()} / {flat.flat.numel()} elements, not {total}"
    assert [id(p) for p in flat.params] == [id(p) for _, p, _ in layout], f"{what}: flat.params are not the trainable parameters in module order"
    esz = flat.grad.element_size()
    for k, p, off in layout:
        tgt = getattr(p, "_mednet_grad", None)
        assert tgt is not None and tgt.data_ptr() == flat.grad.data_ptr() + off * esz and tuple(tgt.shape) == tuple(p.shape), \
            f"{what}: '{k}' does not own the slice at element {off} of flat.grad"
        assert p.data_ptr() == flat.flat.data_ptr() + off * esz, f"{what}: '{k}' does not live at element {off} of flat.flat"
    for k, p in model.named_parameters():
        if p.requires_grad:
            continue
        assert not hasattr(p, "_mednet_grad"), f"{what}: the frozen parameter '{k}' carries a gradient target the kernels would write"
        assert p.grad is None, f"{what}: the frozen parameter '{k}' received a .grad"
        assert same_bits(p.detach(), probe.frozen[k]), f"{what}: the frozen parameter '{k}' changed: {_first_difference(p.detach(), probe.frozen[k])}"
    g = flat.grad.detach().cpu()
    pad = g[probe.pad]
    bad = int((pad != probe.pad_value).sum())
    assert bad == 0, f"{what}: {bad} of {pad.numel()} padding elements of flat.grad were written (they held {probe.pad_value})"
    got = probe.slices()
    for k, t in got.items():
        t = t.cpu()
        assert bool(torch.isfinite(t).all()), f"{what}: the gradient slice of '{k}' is not finite"
        if probe.pad_value == SENTINEL:
            stale = int((t == SENTINEL).sum())
            assert stale == 0, f"{what}: {stale} of {t.numel()} elements of the slice of '{k}' still hold the sentinel: not written this step"
    if clean is not None:
        c = clean.detach().cpu()
        assert c.numel() == g.numel(), f"{what}: the clean run's buffer has {c.numel()} elements, this one {g.numel()}"
        for k, p, off in layout:
            a, b = g[off:off + p.numel()], c[off:off + p.numel()]
            assert same_bits(a, b), (f"{what}: the slice of '{k}' depends on what the buffer held before the step (left stale or "
                                     f"accumulated into): {_first_difference(a, b)}")
    for name, (m, buf) in probe.packs.items():
        if buf is None:
            probe.packs[name] = (m, getattr(m, "_pack_buf", None))   # first packed by this step's forward
            continue
        assert m._packed() is buf, f"{what}: the packed weight of the frozen layer '{name}' was rebuilt"
    seen = {}
    if full is not None:
        missing = [k for k in got if k in routes and ref is None]
        assert not missing, f"{what}: route exceptions {missing} need a reference"
        for k, t in got.items():
            if k in routes:
                continue
            assert k in full, f"{what}: the all-trainable run has no slice of '{k}'"
            assert same_bits(t, full[k]), (f"{what}: the slice of '{k}' is not bit-identical to the all-trainable run's: "
                                           f"{_first_difference(t, full[k])}")
    if ref is not None:
        assert set(ref) == set(got), (f"{what}: the reference has gradients of {sorted(set(ref) - set(got))} that the trainer does not "
                                      f"train, and none of {sorted(set(got) - set(ref))}")
        for k, t in got.items():
            if full is not None and k not in routes:
                continue
            seen[k] = rel_l2(t, ref[k])
            assert seen[k] <= tol, f"{what}: gradient slice of '{k}' rel-L2 {seen[k]:.3e} > {tol:.1e} against the reference"
    return seen


def hold_steps(start, what, ref=None, tol=None, full=None, routes=None, steps=2):
    """The trainer rule over `steps` calls, twice: a clean run, then a run whose gradient buffer is refilled with the sentinel before the
    last call and must end with the clean run's bits in every trainable element.  start() builds a fresh model and step and returns
    (model, flat, call, close): call(i) runs step i and returns its loss as a float, close() releases the step.  ref / full (check_step)
    are held after step 1, where the oracle's gradient and the all-trainable run's slices were taken.
    -> (losses of the clean run, {name: slice} after its step 1, {name: rel-L2} of step 1)."""
    clean = first = seen = losses = None
    for refill in (False, True):
        model, flat, call, close = start()
        try:
            probe = StepProbe(model, flat)
            out = []
            for i in range(steps):
                last = i == steps - 1
                if refill and last:
                    probe.refill()
                out.append(call(i))
                tag = f"{what}, step {i + 1}" + (" after a refill" if refill and last else "")
                s = check_step(probe, tag, ref=ref if i == 0 else None, tol=tol, full=full if i == 0 else None, routes=routes,
                               clean=clean if (refill and last) else None)
                if i == 0 and not refill:
                    first, seen = probe.slices(), s
            if not refill:
                clean, losses = flat.grad.detach().clone(), out
            else:
                assert out == losses, f"{what}: the refilled run's losses {out} are not the clean run's {losses}"
        finally:
            close()
    return losses, first, seen
