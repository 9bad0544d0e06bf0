"""Helpers for the -m gpu parity tests (HIP path vs the CPU oracle on identical seeded inputs)."""
import numpy as np
import torch

from oracle import ref_cpu as O

DEV = "cuda:0"
# tolerance of the parity metric ||a-b||2/||b||2: fp32 mode must meet the north-star 1e-3 with margin;
# bf16 mode stores activations/gradients in bf16 (8 significant bits): the reference's own bf16 drift is 8e-3/2e-2.
TOL = {"fp32": 1e-4, "bf16": 2.5e-2, "fp16": 4e-3}  # fp16 storage: 11 significant bits


def rnd(tag, *shape, scale=1.0):
    return torch.from_numpy((O._rng("in:" + tag).standard_normal(shape) * scale).astype(np.float32))


def bf16_round(t):
    return t.bfloat16().float()


def half_round(t, mode):
    """Inputs representable in the mode's storage type, so the comparison sees the kernels' error, not the input cast."""
    return t.bfloat16().float() if mode == "bf16" else (t.half().float() if mode == "fp16" else t)


def rel(a, b):
    return O.rel_l2(a.detach().float().cpu(), b.detach().float().cpu())


def assert_close(a, b, tol, what):
    r = rel(a, b)
    assert r <= tol, f"{what}: rel-L2 {r:.3e} > {tol:.1e}"
    return r


def copy_params(dst, src):
    """Same names => same values (the oracle/HIP module trees are key-compatible)."""
    dst.load_state_dict(src.state_dict())
    return dst


# --------------------------------------------------------------------------------------------- exact arithmetic
# Inputs on a lattice (small integers, or integers times a power of two) for which the mathematically exact result is
# representable in the kernel's output type and every fp32 partial sum is exact in ANY summation order: accumulation order,
# MFMA blocking, split products and output rounding drop out, and a correct kernel equals ATen's fp64 result in every element.
FP32_EXACT = float(2 ** 24)   # every integer of magnitude <= 2^24 is an fp32 number


def lattice(tag, *shape, values=(-2, -1, 1, 2), density=0.25, scale=1.0):
    """Seeded like `rnd`: entries drawn from `values` (times `scale`, a power of two), zero with probability 1 - density."""
    g = O._rng("in:" + tag)
    keep = g.random(shape) < density
    v = g.choice(np.asarray(values, dtype=np.float64), size=shape)
    return torch.from_numpy((np.where(keep, v, 0.0) * scale).astype(np.float32))


def assert_representable(ref, dtype, what):
    """Condition 1: EVERY reference element survives a round trip through the kernel's output type."""
    ref = ref.detach().double()
    bad = int((ref.to(dtype).double() != ref).sum())
    assert bad == 0, f"{what}: {bad} of {ref.numel()} reference elements are not {dtype} numbers (max |ref| {float(ref.abs().max())})"


def assert_sums_exact(abs_sum, what, unit=1.0):
    """Condition 2: the sum of the ABSOLUTE values of the terms of every output element (in lattice steps of `unit`) is below
    2^24, so every fp32 partial sum, in any order, is an exact multiple of the step."""
    m = float(abs_sum.detach().double().abs().max()) / unit if abs_sum.numel() else 0.0
    assert m < FP32_EXACT, f"{what}: sum of |terms| reaches {m:.4g} lattice steps >= 2^24"


def _residues(idx, names, mods):
    out = []
    for k, name in enumerate(names):
        col = idx[:, k]
        for m in mods.get(name, ()):
            out.append(f"{name}%{m} in {sorted(set((col % m).tolist()))}")
    return "; ".join(out)


def assert_exact(a, ref, what, first=10):
    """Numeric equality of every element (+0 == -0), no NaN.  The failure message gives the number of differing elements, the
    first few as (n, c, z, y, x) with got / want, and the residues of the failing coordinates modulo the brick sizes (z: 4,
    y: 8, x: 16 and 8 for the narrow bricks) and the channel-block sizes (16 / 32): a halo, ragged-edge or channel-block fault is
    recognisable from the message."""
    a = a.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert a.shape == ref.shape, f"{what}: shape {tuple(a.shape)} != {tuple(ref.shape)}"
    assert not bool(torch.isnan(ref).any()), f"{what}: NaN in the reference"
    bad = a != ref     # (NaN != anything: an unwritten / NaN element counts as a difference)
    nbad = int(bad.sum())
    if nbad == 0:
        return a.numel()
    idx = bad.nonzero()
    lines = [f"{tuple(i.tolist())}: got {a[tuple(i.tolist())].item()!r} want {ref[tuple(i.tolist())].item()!r}" for i in idx[:first]]
    names = ("n", "c", "z", "y", "x") if a.dim() == 5 else tuple(f"d{k}" for k in range(a.dim()))
    mods = {"c": (16, 32), "z": (4,), "y": (8,), "x": (16, 8)}
    where = _residues(idx, names, mods) if a.dim() == 5 else ""
    nan = int(torch.isnan(a).sum())
    raise AssertionError(f"{what}: {nbad} of {a.numel()} elements differ ({nan} NaN); first at " + " | ".join(lines)
                         + (f"; residues: {where}" if where else ""))
