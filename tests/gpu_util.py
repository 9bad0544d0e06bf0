"""Helpers for the -m gpu parity tests (HIP path vs the CPU oracle on identical seeded inputs)."""
import types

import numpy as np
import torch

from oracle import ref_cpu as O

DEV = "cuda:0"
CL = torch.channels_last_3d
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}   # storage type of a mode
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


def report(item, what, kernel, elements):
    """One line per comparison group of the exact-arithmetic suites (pytest -s / -rP shows them)."""
    print(f"[exact] item={item} {what} kernel={kernel} elements={elements}")


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


# ------------------------------------------------------------------------------- exact arithmetic: normalisation
# Inputs for GroupNorm / BatchNorm whose statistics, coefficients and gradients are dyadic numbers of the storage types.
def snap(ref, step=2.0 ** -12, moved=1e-9):
    """An fp64 ATen reference rounded to the grid of the exact result.  ATen's fp64 rstd is 1 / sqrt(var + eps) and not
    exactly 1 / sigma: the snapped tensor is the reference, and NO element may have moved by more than `moved`, so that
    snapping cannot hide a real difference (the grid step is 2.4e-4)."""
    ref = ref.detach().double()
    out = torch.round(ref / step) * step
    d = float((out - ref).abs().max()) if ref.numel() else 0.0
    assert d <= moved, f"snap: an element moved by {d:.3e} > {moved:.1e}: the reference is not on the 2^{int(np.log2(step))} grid"
    return out


def norm_lattice(tag, n, c, groups, shape, eps, batch=False, nonneg=False):
    """Seeded like `lattice`.  Per (sample, group): x = m + sigma * s and du = e + p + q * s with s in {-1, +1} balanced so
    that the group mean is exactly m and the variance exactly sigma^2 (eps 0: sigma in {1, 2, 4}, rstd = 1 / sigma; eps 3:
    sigma = 1, rstd = 1 / 2); e in {+-1, +-2} (0 for an odd leftover) comes in +t / -t pairs among the voxels of equal s of a channel, so every sum
    the backward divides by `count` is an exact multiple of it -- also when an activation masks du by the sign of s.  Even
    spatial size: s is balanced inside every channel; odd: channel 2j + 1 carries -s of channel 2j and shares its gamma (odd
    size with an odd channel count per group raises).  gamma in {1, 2} with a dyadic group mean (uniform from {1/2, 1, 2}
    when a group has fewer than four channels), beta a small integer; beta_act, for the variants that recompute an
    activation mask from the forward coefficients, is uniform per group: +-3 (all pass / all blocked) or +-1/8 (the mask
    is the sign of s), never giving a pre-activation of 0.
    batch=True (BatchNorm, groups == c): one (m, sigma, p, q) row per channel for all samples; the balance of s and the pairs
    of e run over the n * S voxels of a channel (n * S even).  nonneg=True: m = sigma, so x is 0 or 2 * sigma (the output of
    a ReLU).  Returns x, du [n, c, *shape], gamma, beta, beta_act [c] (fp32) and m, sigma, p, q [n, groups] (fp64)."""
    if float(eps) not in (0.0, 3.0):
        raise ValueError("norm_lattice: eps must be 0 or 3")
    if c % groups:
        raise ValueError("norm_lattice: c % groups != 0")
    g = O._rng("in:" + tag)
    cg, S = c // groups, int(np.prod(shape))
    if batch:
        if groups != c or (n * S) % 2:
            raise ValueError("norm_lattice: BatchNorm wants groups == c and an even n * S")
    ns, ln = (1, n * S) if batch else (n, S)
    if ln % 2 and cg % 2:
        raise ValueError(f"norm_lattice: odd spatial size {ln} with an odd channel count per group {cg}")
    sigma = g.choice(np.asarray([1.0, 2.0, 4.0]), size=(ns, groups)) if float(eps) == 0.0 else np.ones((ns, groups))
    m = sigma.copy() if nonneg else g.integers(-3, 4, size=(ns, groups)).astype(np.float64)
    p = g.choice(np.asarray([-2.0, -1.0, 1.0, 2.0]), size=(ns, groups))
    q = g.choice(np.asarray([-2.0, -1.0, 1.0, 2.0]), size=(ns, groups))
    s = np.empty((ns, c, ln))
    e = np.zeros((ns, c, ln))
    for i in range(ns):
        for ch in range(c):
            if ln % 2 and ch % 2:
                s[i, ch] = -s[i, ch - 1]
            else:
                k = ln // 2 + (int(g.integers(0, 2)) if ln % 2 else 0)
                row = -np.ones(ln)
                row[g.permutation(ln)[:k]] = 1.0
                s[i, ch] = row
            for sign in (1.0, -1.0):
                idx = g.permutation(np.flatnonzero(s[i, ch] == sign))
                h = len(idx) // 2
                t = g.choice(np.asarray([-2.0, -1.0, 1.0, 2.0]), size=h)
                e[i, ch, idx[:h]] = t
                e[i, ch, idx[h:2 * h]] = -t
    per_ch = lambda a: np.repeat(a, cg, axis=1)[:, :, None]
    x = per_ch(m) + per_ch(sigma) * s
    du = e + per_ch(p) + per_ch(q) * s
    gamma = np.empty(c)
    for gi in range(groups):
        if cg >= 4 and cg % 4 == 0:
            unit = 2 if ln % 2 else 1                                  # odd size: the 2s come in channel pairs
            ks = [k for k in range(0, cg + 1, cg // 4) if k % unit == 0]
            k = int(g.choice(np.asarray(ks)))
            row = np.ones(cg)
            chosen = g.permutation(cg // unit)[:k // unit]
            for j in chosen:
                row[j * unit:(j + 1) * unit] = 2.0
            gamma[gi * cg:(gi + 1) * cg] = row
        else:
            gamma[gi * cg:(gi + 1) * cg] = float(g.choice(np.asarray([0.5, 1.0, 2.0])))
    beta = g.integers(-3, 4, size=c).astype(np.float64)
    beta_act = np.repeat(g.choice(np.asarray([3.0, -3.0, 0.125, -0.125]), size=groups, p=[0.3, 0.15, 0.3, 0.25]), cg)

    def vol(a):
        if batch:
            a = a.reshape(c, n, S).transpose(1, 0, 2)
        return torch.from_numpy(np.ascontiguousarray(a.reshape(n, c, *shape)).astype(np.float32))

    rows = lambda a: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (n, groups))).astype(np.float64))
    f32 = lambda a: torch.from_numpy(a.astype(np.float32))
    return types.SimpleNamespace(x=vol(x), du=vol(du), gamma=f32(gamma), beta=f32(beta), beta_act=f32(beta_act), m=rows(m),
                                 sigma=rows(sigma), p=rows(p), q=rows(q), n=n, c=c, groups=groups, shape=tuple(shape), eps=float(eps),
                                 spatial=S, cg=cg, batch=batch)


# ------------------------------------------------------------------------------- the fused heads' backward
# Inputs and checkers of tests/test_gpu_head_backward.py and of the ELU cases of tests/test_gpu_exact.py; tests/test_exact_util.py
# shows on the CPU that the checkers reject the faults they are there for.
ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_ELU = 0, 1, 2, 3       # mednet_hip._lib's codes
ELU_Z = (-0.75, -0.5, -0.25, 0.0, 1.0, 2.0)               # block outputs of an ELU: act' = z + 1 in {1/4, 1/2, 3/4, 1} for z <= 0
U_STORE = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp32": 0.0}   # the rounding of a stored gradient
EPS_FLOOR = 2.0 ** -15    # the matrix-core heads' own arithmetic (16-bit-pair image of dl, dropped lo * lo, fp32 sums), doubled
SUM_BOUND = 2.0 ** -16    # < 256 fp32 roundings of 2^-24 per GroupNorm sum


def split_weight(w0, mode):
    """fp32 weights of the form hi + lo, both parts numbers of the mode's storage type (hi = round(w0), lo = round(w0 - hi)):
    17 significant bits in bf16, 23 in fp16.  A kernel that splits its fp32 weights as hi' = round(w), lo' = round(w - hi')
    reproduces them exactly, and both images carry data."""
    hi = half_round(w0, mode)
    return hi + half_round(w0 - hi, mode)


def elu_lattice(tag, *shape, density=0.8, window_max=False):
    """Seeded like `lattice`: block outputs on the dyadic lattice ELU_Z (bf16 and fp16 numbers; zero with probability
    1 - density on top of the lattice's own zero), so that du = dx * (z + 1) is exact in fp32 in steps of 1/4 for an integer dx.
    window_max: the three trailing dims are even and every 2 x 2 x 2 window has a UNIQUE maximum -- one element holds a lattice
    value above -3/4 (negative ones included: a max pooling routes its gradient there), the seven others lie strictly below it."""
    if not window_max:
        return lattice(tag, *shape, values=ELU_Z, density=density)
    d, h, w = shape[-3:]
    lead = tuple(shape[:-3])
    k = len(lead)
    wshape = lead + (d // 2, h // 2, w // 2)
    g = O._rng("in:" + tag + ":max")
    top = g.integers(1, len(ELU_Z), size=wshape)                                   # index of the window's maximum
    idx = np.floor(g.random(wshape + (8,)) * top[..., None]).astype(np.int64)      # the others: uniform below it
    np.put_along_axis(idx, g.integers(0, 8, size=wshape)[..., None], top[..., None], axis=-1)
    win = torch.from_numpy(np.asarray(ELU_Z, dtype=np.float32)[idx]).reshape(wshape + (2, 2, 2))
    return win.permute(*range(k), k, k + 3, k + 1, k + 4, k + 2, k + 5).reshape(shape).contiguous()


def act_grad_from_out(z, act):
    """act'(.) through the activation OUTPUT z, in z's precision (ATen's in-place forms; LeakyReLU(0.1), ELU(alpha = 1))."""
    one = torch.ones_like(z)
    if act == ACT_RELU:
        return (z > 0).to(z.dtype)
    if act == ACT_LEAKY:
        return torch.where(z > 0, one, 0.1 * one)
    if act == ACT_ELU:
        return torch.where(z > 0, one, z + 1)
    return one


def _first_bad(bad, got, ref, bound, first=6):
    idx = bad.nonzero()[:first]
    return " | ".join(f"{tuple(i.tolist())}: got {got[tuple(i.tolist())].item()!r} want {ref[tuple(i.tolist())].item()!r} "
                      f"bound {bound[tuple(i.tolist())].item():.3e}" for i in idx)


def ref_error(x32, x64, norm, what):
    """r32 = max |x32 - x64| / norm over all elements: what ATen's fp32 evaluation shows against its fp64 one in the
    normalisation of the bound (an element whose norm is 0 has no terms: both references must be 0 there).  -> (r32, eps_case),
    eps_case = max(EPS_FLOOR, 8 * r32)."""
    x32, x64, norm = x32.detach().double(), x64.detach().double(), norm.detach().double()
    diff = (x32 - x64).abs()
    dead = norm == 0
    assert not bool((diff[dead] != 0).any()), f"{what}: the fp32 and fp64 references differ where the bound's norm is 0"
    r32 = float((diff[~dead] / norm[~dead]).max()) if bool((~dead).any()) else 0.0
    return r32, max(EPS_FLOOR, 8.0 * r32)


def check_gradient(got, ref64, norm, eps, what, u=0.0, s=0.0):
    """Every element, no NaN: |got - ref64| <= u * |ref64| + eps * norm + s.  -> the worst observed ratio
    max(|got - ref64| - u * |ref64| - s, 0) / norm, to be read against eps."""
    got, ref64, norm = got.detach().double().cpu(), ref64.detach().double(), norm.detach().double()
    assert got.shape == ref64.shape == norm.shape, f"{what}: shapes {tuple(got.shape)} / {tuple(ref64.shape)} / {tuple(norm.shape)}"
    nan = int(torch.isnan(got).sum())
    assert nan == 0, f"{what}: {nan} of {got.numel()} elements are NaN (not written)"
    diff = (got - ref64).abs()
    bound = u * ref64.abs() + eps * norm + s
    bad = diff > bound
    nbad = int(bad.sum())
    assert nbad == 0, f"{what}: {nbad} of {got.numel()} elements outside u |ref| + eps * norm + s (u {u:.3e} eps {eps:.3e} s {s:.3e}); first at " + _first_bad(bad, got, ref64, bound)
    over = (diff - u * ref64.abs() - s).clamp(min=0)
    live = norm > 0
    return float((over[live] / norm[live]).max()) if bool(live.any()) else 0.0


def check_gn_sums(partial, dz_stored, z, gn_y, act, what):
    """gn_partial[n][rows][c][2] against {sum du, sum du * gn_y}, du = dz_stored * act'(z), in fp64 from the STORED gradient
    (n x c x spatial dims, as z and gn_y): |got - want| <= SUM_BOUND * sum |terms| per (sample, channel, entry), no NaN.
    -> the worst observed |got - want| / sum |terms|."""
    p = partial.detach().double().cpu()
    nan_rows = int(torch.isnan(p).any(-1).any(-1).sum())
    assert nan_rows == 0, f"{what}: {nan_rows} of {p.shape[0] * p.shape[1]} rows of gn_partial hold a NaN (not written)"
    got = p.sum(1)
    z64, y64 = z.detach().double().cpu(), gn_y.detach().double().cpu()
    du = dz_stored.detach().double().cpu() * act_grad_from_out(z64, act)
    dims = tuple(range(2, du.dim()))
    want = torch.stack((du.sum(dims), (du * y64).sum(dims)), -1)
    mag = torch.stack((du.abs().sum(dims), (du * y64).abs().sum(dims)), -1)
    assert got.shape == want.shape, f"{what}: gn_partial totals {tuple(got.shape)} != {tuple(want.shape)}"
    diff = (got - want).abs()
    bound = SUM_BOUND * mag
    bad = diff > bound
    nbad = int(bad.sum())
    assert nbad == 0, f"{what}: {nbad} of {got.numel()} GroupNorm sums outside 2^-16 * sum |terms|; first at " + _first_bad(bad, got, want, bound)
    live = mag > 0
    return float((diff[live] / mag[live]).max()) if bool(live.any()) else 0.0
