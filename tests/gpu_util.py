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


def ref_error(x32, x64, norm, what, floor=EPS_FLOOR, s=0.0):
    """r32 = max |x32 - x64| / norm over all elements: what ATen's fp32 evaluation shows against its fp64 one in the
    normalisation of the bound (an element whose norm is 0 has no terms: both references must be 0 there).  -> (r32, eps_case),
    eps_case = max(floor, 8 * r32); the floor is the kernel's own count of roundings (EPS_FLOOR for the matrix-core heads); s is
    the absolute slack of the bound (check_gradient's s)."""
    x32, x64, norm = x32.detach().double(), x64.detach().double(), norm.detach().double()
    diff = ((x32 - x64).abs() - s).clamp(min=0)
    dead = norm == 0
    assert not bool((diff[dead] != 0).any()), f"{what}: the fp32 and fp64 references differ where the bound's norm is 0"
    r32 = float((diff[~dead] / norm[~dead]).max()) if bool((~dead).any()) else 0.0
    return r32, max(floor, 8.0 * r32)


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


# ------------------------------------------------------------------------------- the loss kernels and the Adam step
# Inputs, fp64 references and checkers of tests/test_gpu_losses.py (csrc/loss.hip, the Adam kernels of csrc/optim.hip).
# tests/test_loss_util.py runs all of them on the CPU: the exact inputs meet their premises, ATen's fp32 results pass the bounds,
# and every checker rejects the fault it is there for.  Tensors of a case are [n, c, S] (S = the voxels of a sample).
LOSS_BLOCK_VOX = 2048          # voxels per workgroup of loss.hip; one fp32 partial row per workgroup, the rows are added in fp64
U32 = 2.0 ** -24               # one fp32 rounding
LOSS_SUM_BOUND = 2.0 ** -18    # a sum of loss.hip: p a few ulp off (expf, reciprocal), 8 additions per lane, 8 levels of the
#                                workgroup sum, fp64 from there: under 24 roundings of 2^-24, doubled
LOSS_EPS_FLOOR = 2.0 ** -20    # a logit gradient of loss.hip / an Adam update: sixteen fp32 roundings
F32_TINY = 2.0 ** -126         # fp32's smallest normal number: below it a result has no relative precision (a saturated softmax gives
#                                logit gradients of 1e-48), so a logit gradient is admitted this absolute error on top of its bound


def _np_rng(tag):
    return O._rng("in:" + tag)


def block_abs_sums(terms):
    """terms [..., S] -> the fp64 sum of |terms| over every block of LOSS_BLOCK_VOX voxels [..., blocks]: what a workgroup adds."""
    t = terms.detach().double().abs()
    S = t.shape[-1]
    nb = -(-S // LOSS_BLOCK_VOX)
    t = torch.nn.functional.pad(t, (0, nb * LOSS_BLOCK_VOX - S))
    return t.reshape(t.shape[:-1] + (nb, LOSS_BLOCK_VOX)).sum(-1)


def f32_scalar(t):
    """A 0-dim fp32 tensor (device or CPU) as numpy float32, bits kept."""
    return np.float32(t.detach().float().cpu().numpy())


def assert_same_f32(got, want, what):
    """Bit-for-bit equality of two fp32 scalars (+0 == -0); a NaN is expected exactly where `want` is NaN."""
    got, want = np.float32(got), np.float32(want)
    if np.isnan(want):
        assert np.isnan(got), f"{what}: got {got!r}, want NaN"
    else:
        assert got == want, f"{what}: got {got!r} want {want!r} (difference {float(got) - float(want):.3e})"


# ---- A.1 heat-map regression on integers
def hm_exact_case(tag, n, c, shape, tgt="u8"):
    """Targets: channels [:-1] of an n x (c + 1) x shape volume of integers 0..255 (uint8, or fp32 holding them); out = target + delta,
    delta an integer in [-64, 64] (a tenth of them 0); channel weights and dloss powers of two."""
    g = _np_rng(tag)
    S = int(np.prod(shape))
    vol = g.integers(0, 256, size=(n, c + 1, S))
    delta = g.integers(-64, 65, size=(n, c, S))
    delta[g.random(delta.shape) < 0.1] = 0
    volume = torch.from_numpy(vol.astype(np.uint8 if tgt == "u8" else np.float32)).reshape((n, c + 1) + tuple(shape))
    out = torch.from_numpy((vol[:, :-1] + delta).astype(np.float32)).reshape((n, c) + tuple(shape))
    w = torch.from_numpy((2.0 ** g.integers(-3, 2, size=c)).astype(np.float32))
    return types.SimpleNamespace(n=n, c=c, shape=tuple(shape), spatial=S, volume=volume, target=volume[:, :-1], out=out, w=w, dloss=0.5,
                                 count=n * S, tgt=tgt)


def hm_reference(case, kind):
    """fp64 sums S_c (exact integers), the loss as the finalize kernel forms it -- tot = f32(tot + f32(w_c) * f32(S_c / count)), c
    ascending, S_c / count in fp64 -- and the gradient: fp64 for L2, the exact fp32 numbers sign(d) * f32(dloss * w_c) * f32(1 / count)
    for L1.  Asserts the premise: the sum of |terms| of every workgroup is below 2^24, so its fp32 partial is exact in any order."""
    n, c, S = case.n, case.c, case.spatial
    d = (case.out.double() - case.target.double()).reshape(n, c, S)
    assert float(d.abs().max()) <= 64 and bool((d == d.round()).all())
    f = d * d if kind == "L2" else d.abs()
    assert_sums_exact(block_abs_sums(f), f"heat-map {kind} block sums")
    Sc = f.sum((0, 2))
    w = case.w.numpy()
    assert bool((np.log2(w) == np.round(np.log2(w))).all()), "channel weights must be powers of two"
    tot = np.float32(0)
    for k in range(c):
        tot = np.float32(tot + np.float32(w[k]) * np.float32(float(Sc[k]) / case.count))
    loss64 = float((case.w.double() * Sc / case.count).sum())
    sgn = 2.0 * d if kind == "L2" else torch.sign(d)
    grad64 = (case.dloss * case.w.double()[None, :, None] / case.count) * sgn
    scale32 = (np.float32(case.dloss) * w) * np.float32(1.0 / case.count)
    assert scale32.dtype == np.float32
    grad_l1 = torch.sign(d).float() * torch.from_numpy(scale32)[None, :, None]
    return types.SimpleNamespace(d=d, Sc=Sc, loss32=tot, loss64=loss64, grad64=grad64, grad_l1=grad_l1, kind=kind)


def check_hm(case, ref, loss, dout, what):
    """loss: the very bits of ref.loss32.  dout [n, c, S]: L1 equals +-scale exactly and is exactly 0 where d = 0; L2 is within
    4 * 2^-24 * |ref64| per element (float(1 / count), the product with the weight and the final product round once each).
    -> the worst observed |dout - ref64| / |ref64| (L2; 0 for L1)."""
    assert_same_f32(loss, ref.loss32, what + ": loss")
    dout = dout.detach().cpu().reshape(case.n, case.c, case.spatial)
    if ref.kind == "L1":
        assert_exact(dout, ref.grad_l1, what + ": dout")
        return 0.0
    return check_gradient(dout, ref.grad64, ref.grad64.abs(), 4.0 * U32, what + ": dout")


# ---- A.2 cross-entropy with terms of w_y * 200 or 0
CE_WEIGHTS = (0.25, 0.5, 1.0, 2.0, 4.0)


def ce_exact_case(tag, n, c, shape, ignore=-100, ignored="some"):
    """Logits -200 everywhere except one 0 per voxel at a random class (fp32 exp(-200) is exactly 0, so a voxel's term is
    w_y * 200, or 0 where the label is that class); labels independent of that class; weights from CE_WEIGHTS; ignored: "some"
    (a tenth of the voxels carry ignore_index), "sample" (also all of sample 0) or "all"."""
    g = _np_rng(tag)
    S = int(np.prod(shape))
    hot = g.integers(0, c, size=(n, S))
    lg = np.full((n, c, S), -200.0, dtype=np.float32)
    np.put_along_axis(lg, hot[:, None, :], 0.0, axis=1)
    lab = g.integers(0, c, size=(n, S)).astype(np.int64)
    lab[g.random((n, S)) < 0.1] = ignore
    if ignored == "sample":
        lab[0] = ignore
    elif ignored == "all":
        lab[:] = ignore
    w = torch.from_numpy(g.choice(np.asarray(CE_WEIGHTS), size=c).astype(np.float32))
    return types.SimpleNamespace(n=n, c=c, shape=tuple(shape), spatial=S, lg=torch.from_numpy(lg), hot=torch.from_numpy(hot),
                                 lab=torch.from_numpy(lab), w=w, ignore=ignore)


def ce_exact_reference(case):
    """num64 = sum w_y * 200 [y != the voxel's 0 class], den64 = sum w_y over the live voxels, both exact in fp64; the finalize kernel
    divides in fp64 and rounds once: loss32 = f32(num64 / den64) (NaN when every voxel is ignored, as in ATen), saved32 = f32(den64).
    Asserts the premise: every workgroup's sums are below 2^24 steps of 50 (num) and of 1/4 (den)."""
    live = case.lab != case.ignore
    wy = torch.where(live, case.w.double()[case.lab.clamp(0, case.c - 1)], torch.zeros((), dtype=torch.float64))
    term = wy * 200.0 * (case.lab != case.hot)
    assert_sums_exact(block_abs_sums(term), "CE numerator block sums", unit=50.0)
    assert_sums_exact(block_abs_sums(wy), "CE denominator block sums", unit=0.25)
    num64, den64 = float(term.sum()), float(wy.sum())
    loss32 = np.float32(num64 / den64) if den64 != 0.0 else np.float32("nan")
    return types.SimpleNamespace(num64=num64, den64=den64, loss32=loss32, saved32=np.float32(den64))


def check_ce_exact(ref, loss, saved0, what):
    assert_same_f32(saved0, ref.saved32, what + ": saved[0] against sum w_y")
    assert_same_f32(loss, ref.loss32, what + ": loss against f32(num64 / den64)")


# ---- A.3 Dice with probabilities in {0, 1/4, 1/2, 1}
def dice_exact_case(tag, n, c, shape, sigmoid):
    """softmax: logits in {0, -200} with 1, 2 or 4 zeros per voxel (as many as c allows): p in {0, 1/4, 1/2, 1} exactly (exp(-200) is
    0 in fp32, the reciprocal of 1, 2, 4 is exact); sigmoid: logits in {-200, 0, 200}: p in {0, 1/2, 1}.  -> lg, the exact p (fp64),
    labels, weights in [0.05, 1.05)."""
    g = _np_rng(tag)
    S = int(np.prod(shape))
    if sigmoid:
        lg = g.choice(np.asarray([-200.0, 0.0, 200.0]), size=(n, c, S))
        p = (lg + 200.0) / 400.0
    else:
        k = g.choice(np.asarray([k for k in (1, 2, 4) if k <= c]), size=(n, 1, S))
        rank = np.argsort(np.argsort(g.random((n, c, S)), axis=1), axis=1)
        zero = rank < k
        lg = np.where(zero, 0.0, -200.0)
        p = zero / k
    lab = g.integers(0, c, size=(n, S)).astype(np.int64)
    w = torch.from_numpy((0.05 + g.random(c)).astype(np.float32))
    return types.SimpleNamespace(n=n, c=c, shape=tuple(shape), spatial=S, lg=torch.from_numpy(lg.astype(np.float32)),
                                 p=torch.from_numpy(p.astype(np.float64)), lab=torch.from_numpy(lab), w=w, sigmoid=sigmoid, eps=1e-5)


def dice_sums(p, lab, ignore):
    """One-hot target t, mask m (the reference masks where the ONE-HOT target equals ignore_index) and the Dice sums
    I_c = sum p t m, D_c = sum (p + t) m over samples and voxels, in p's precision.  p [n, c, S], lab [n, S] in [0, c)."""
    t = torch.nn.functional.one_hot(lab, p.shape[1]).permute(0, 2, 1).to(p.dtype)
    m = torch.ones_like(t) if ignore is None else (t != ignore).to(p.dtype)
    return t, m, (p * t * m).sum((0, 2)), ((p + t) * m).sum((0, 2))


def dice_from_sums(I, D, w, eps):
    dice = 2.0 * (w * I) / D.clamp(min=eps)
    return dice, (1.0 - dice).mean()


def dice_exact_reference(case, ignore):
    """saved64 [c, 2] = {I_c, D_c}, dice64, loss64 from the exact probabilities.  Asserts the premise: the sums of a workgroup and
    the totals are below 2^24 steps of 1/4 (fp32 partials and the fp32 `saved` hold them exactly)."""
    t, m, I, D = dice_sums(case.p, case.lab, ignore)
    assert_sums_exact(block_abs_sums((case.p + t) * m), "Dice block sums", unit=0.25)
    assert_sums_exact(D, "Dice totals", unit=0.25)
    dice, loss = dice_from_sums(I, D, case.w.double(), case.eps)
    return types.SimpleNamespace(saved64=torch.stack((I, D), -1), dice64=dice, loss64=float(loss))


def check_dice_exact(case, ref, saved, dice_out, loss, what):
    """saved: every entry equals the fp64 sum.  dice_out: within 2 * 2^-24 * |dice64| (the product with the weight and the division
    round once each).  loss: within (C + 4) * 2^-24 * (1 + max |dice64|) (product, division, 1 - dice, C - 1 additions, the division
    by C).  -> the observed |loss - loss64| / ((1 + max |dice64|) * 2^-24), to be read against C + 4."""
    assert_exact(saved.detach().cpu().reshape(case.c, 2), ref.saved64, what + ": saved")
    if dice_out is not None:
        check_gradient(dice_out.detach().cpu(), ref.dice64, ref.dice64.abs(), 2.0 * U32, what + ": dice_out")
    got = float(loss)
    unit = U32 * (1.0 + float(ref.dice64.abs().max()))
    assert not np.isnan(got), what + ": loss is NaN"
    err = abs(got - ref.loss64)
    assert err <= (case.c + 4) * unit, f"{what}: |loss - loss64| = {err:.3e} > (C + 4) 2^-24 (1 + max |dice|) = {(case.c + 4) * unit:.3e}"
    return err / unit


# ---- B. random logits against fp64
def loss_random_case(tag, n, c, shape, edge=False):
    """Logits N(0, 2^2); 2% of the voxels have one channel pushed to +-30, 2% an exact tie of channels 0 and 1; weights in
    [0.05, 1.05); a tenth of the voxels are marked for cross-entropy's ignore_index (case.ign).  edge: dloss = -2.5, eps = 1e-2, the
    weight of class 1 is 0, and the last channel is dead -- logit -40 everywhere, never a label -- so its D is below eps (the zero
    branch of the D gradient)."""
    g = _np_rng(tag)
    S = int(np.prod(shape))
    lg = (2.0 * g.standard_normal((n, c, S))).astype(np.float32)
    push = g.random((n, S)) < 0.02
    ch = g.integers(0, c, size=(n, S))
    val = np.where(g.random((n, S)) < 0.5, 30.0, -30.0).astype(np.float32)
    cur = np.take_along_axis(lg, ch[:, None, :], axis=1)[:, 0]
    np.put_along_axis(lg, ch[:, None, :], np.where(push, val, cur)[:, None, :], axis=1)
    if c > 1:
        tie = g.random((n, S)) < 0.02
        lg[:, 1] = np.where(tie, lg[:, 0], lg[:, 1])
    lab = g.integers(0, c, size=(n, S)).astype(np.int64)
    w = (0.05 + g.random(c)).astype(np.float32)
    ign = g.random((n, S)) < 0.1
    eps, dloss = 1e-5, 1.0
    if edge:
        eps, dloss = 1e-2, -2.5
        if c > 1:
            w[1] = 0.0
        if c > 2:
            lg[:, c - 1] = -40.0
            lab[lab == c - 1] = 0
    return types.SimpleNamespace(n=n, c=c, shape=tuple(shape), spatial=S, lg=torch.from_numpy(lg), lab=torch.from_numpy(lab),
                                 w=torch.from_numpy(w), ign=torch.from_numpy(ign), eps=eps, dloss=dloss, edge=edge)


def dice_chain(case, sigmoid, ignore, dtype):
    """The Dice loss as plain torch expressions in `dtype` on the CPU, autograd for the logit gradient."""
    lg = case.lg.to(dtype).clone().requires_grad_(True)
    p = torch.sigmoid(lg) if sigmoid else torch.softmax(lg, 1)
    t, m, I, D = dice_sums(p, case.lab, ignore)
    dice, loss = dice_from_sums(I, D, case.w.to(dtype), case.eps)
    (loss * case.dloss).backward()
    return types.SimpleNamespace(loss=float(loss.detach()), saved=torch.stack((I, D), -1).detach(), dice=dice.detach(), dlg=lg.grad, p=p.detach(),
                                 t=t, m=m)


def dice_grad_norm(case, r64, sigmoid):
    """The sum of the absolute terms of a Dice logit gradient, in fp64: with g = dL/dp = m (gI t m + gD),
    softmax: A[k, v] = p_k (|g_k| + sum_j p_j |g_j|); sigmoid: A[k, v] = |g_k| p_k (1 + p_k) (g p - g p^2: 1 - p cancels where the
    sigmoid saturates)."""
    I, D = r64.saved[:, 0], r64.saved[:, 1]
    w, c = case.w.double(), case.c
    Dc = D.clamp(min=case.eps)
    gI = (-2.0 * w / (c * Dc) * case.dloss)[None, :, None]
    gD = (torch.where(D >= case.eps, 2.0 * w * I / (c * Dc * Dc), torch.zeros_like(D)) * case.dloss)[None, :, None]
    g = (r64.m * (gI * r64.t * r64.m + gD)).abs()
    if sigmoid:
        return g * r64.p * (1.0 + r64.p)
    return r64.p * (g + (r64.p * g).sum(1, keepdim=True))


def ce_labels(case, ignore):
    lab = case.lab.clone()
    lab[case.ign] = ignore
    return lab


def ce_chain(case, ignore, dtype):
    """F.cross_entropy(weight, ignore_index) in `dtype` on the CPU with autograd; in addition den = sum w_y over the live voxels, the
    sum of |terms| of the loss (sum w_y |nll| / den) and the sum of absolute terms of the gradient |dloss| w_y / den (p_k + t_k)."""
    lab = ce_labels(case, ignore)
    lg = case.lg.to(dtype).clone().requires_grad_(True)
    w = case.w.to(dtype)
    loss = torch.nn.functional.cross_entropy(lg, lab, weight=w, ignore_index=ignore)
    (loss * case.dloss).backward()
    live = lab != ignore
    safe = lab.clamp(0, case.c - 1)
    wy = torch.where(live, w[safe], torch.zeros((), dtype=dtype))
    den = wy.sum()
    logp = torch.log_softmax(lg.detach(), 1)
    nll = -logp.gather(1, safe[:, None, :])[:, 0]
    t = torch.nn.functional.one_hot(safe, case.c).permute(0, 2, 1).to(dtype)
    norm = abs(case.dloss) * (wy / den)[:, None, :] * (logp.exp() + t)
    return types.SimpleNamespace(loss=float(loss.detach()), den=float(den), loss_terms=float((wy * nll.abs()).sum() / den), dlg=lg.grad, norm=norm)


def check_loss_scalar(got, want64, terms, what, bound=LOSS_SUM_BOUND):
    """|got - want64| <= bound * terms (the sum of the absolute terms).  -> the observed ratio |got - want64| / terms."""
    got = float(got)
    assert not np.isnan(got), what + ": NaN"
    err = abs(got - want64)
    assert err <= bound * terms, f"{what}: |got - ref64| = {err:.3e} > {bound:.3e} * sum |terms| = {bound * terms:.3e} (got {got!r} want {want64!r})"
    return err / terms if terms > 0 else 0.0


def loss_grad_eps(x32, x64, norm, what):
    """(r32, eps_case) of a logit gradient: eps_case = max(2^-20, 8 * r32), r32 from ATen's fp32 autograd against its fp64 one."""
    return ref_error(x32, x64, norm, what, floor=LOSS_EPS_FLOOR, s=F32_TINY)


def check_dice_random(case, r64, norm, eps_case, saved, loss, dlg, what):
    """saved [c, 2] and the loss within 2^-18 * sum |terms| (the sums: of themselves, their terms are positive; the loss:
    mean_c (1 + |dice64_c|)); dlogits [n, c, S] through check_gradient with the case's eps.  -> observed ratios."""
    s64 = r64.saved
    return dict(saved=check_gradient(saved.detach().cpu().reshape(case.c, 2), s64, s64.abs(), LOSS_SUM_BOUND, what + ": saved"),
                loss=check_loss_scalar(loss, r64.loss, float((1.0 + r64.dice.abs()).mean()), what + ": loss"),
                dlg=check_gradient(dlg.detach().cpu().reshape(case.n, case.c, case.spatial), r64.dlg, norm, eps_case, what + ": dlogits",
                                   s=F32_TINY))


def check_ce_random(case, r64, eps_case, saved0, loss, dlg, what):
    return dict(saved=check_loss_scalar(saved0, r64.den, r64.den, what + ": saved[0]"),
                loss=check_loss_scalar(loss, r64.loss, r64.loss_terms, what + ": loss"),
                dlg=check_gradient(dlg.detach().cpu().reshape(case.n, case.c, case.spatial), r64.dlg, r64.norm, eps_case, what + ": dlogits",
                                   s=F32_TINY))


# ---- C. Adam
ADAM_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def adam_case(tag, count):
    """One step from a given state: random p, m, g, v >= 0; every 16th element has g = 0 and v = 0 (the denominator is eps)."""
    g = _np_rng(tag)
    f = lambda a: torch.from_numpy(a.astype(np.float32))
    p, m, gr = f(g.standard_normal(count)), f(0.1 * g.standard_normal(count)), f(g.standard_normal(count))
    v = f(0.01 * g.standard_normal(count) ** 2)
    gr[::16] = 0.0
    v[::16] = 0.0
    return types.SimpleNamespace(count=count, p=p, g=gr, m=m, v=v)


def adam_lines(p, g, m, v, lr, b1, b2, eps, wd, step, gscale, dtype, bias_correction=True):
    """torch.optim.Adam's step (weight decay added to the gradient, eps added after the bias correction of the denominator) restated:
    every operand, the hyper-parameters included, is a tensor of `dtype`, so float32 evaluates each line in fp32.  The
    hyper-parameters are the fp32 numbers the C ABI receives.  -> p', m', v', the update delta = p - p'."""
    s = lambda x: torch.tensor(float(np.float32(x)), dtype=dtype)
    p, g, m, v = (t.to(dtype) for t in (p, g, m, v))
    lr, b1, b2, eps, wd, gscale, one = s(lr), s(b1), s(b2), s(eps), s(wd), s(gscale), s(1.0)
    gr = g * gscale + wd * p
    m1 = b1 * m + (one - b1) * gr
    v1 = b2 * v + (one - b2) * gr * gr
    t = s(step)
    bc1, bc2 = (one - b1 ** t, one - b2 ** t) if bias_correction else (one, one)
    denom = v1.sqrt() / bc2.sqrt() + eps
    delta = (lr / bc1) * (m1 / denom)
    terms_m = (b1 * m).abs() + (one - b1) * ((g * gscale).abs() + (wd * p).abs())
    terms_v = b2 * v + (one - b2) * gr * gr
    terms_d = (lr / bc1) * (terms_m / denom)     # (= |delta| wherever b1 m and (1 - b1) g do not cancel)
    return types.SimpleNamespace(p=p - delta, m=m1, v=v1, delta=delta, terms_m=terms_m, terms_v=terms_v, terms_d=terms_d)


def adam_reference(case, wd, step, gscale):
    """fp64 and fp32 evaluations of adam_lines and eps_case per tensor: max(2^-20, 8 * r32), r32 the fp32 lines' error in the norm
    of the bound (m, v: the sum of |terms|; p: the update's own size |delta64|).  Where b1 m and (1 - b1) g cancel, delta inherits m's
    absolute error, which is large against |delta64| itself: that one element inflates r32 of p (1e-3 at 10 007 elements) and with it
    the bound of every element.  So p is ALSO held to eps_case of the update's sum of absolute terms (lr / bc1) terms_m / denom
    ("pt"), whose r32 stays at a few 1e-6; check_adam asserts both."""
    r64 = adam_lines(case.p, case.g, case.m, case.v, wd=wd, step=step, gscale=gscale, dtype=torch.float64, **ADAM_HP)
    r32 = adam_lines(case.p, case.g, case.m, case.v, wd=wd, step=step, gscale=gscale, dtype=torch.float32, **ADAM_HP)
    out = types.SimpleNamespace(r64=r64, r32=r32, r32s={}, eps={})
    for name, x32, x64, norm in (("m", r32.m, r64.m, r64.terms_m), ("v", r32.v, r64.v, r64.terms_v), ("p", r32.delta, r64.delta, r64.delta.abs()),
                                 ("pt", r32.delta, r64.delta, r64.terms_d)):
        out.r32s[name], out.eps[name] = ref_error(x32, x64, norm, "Adam " + name, floor=LOSS_EPS_FLOOR)
    return out


def check_adam(ref, p, m, v, what):
    """m, v: |got - ref64| <= eps_case * sum |terms|; p: |p - p64| <= 2^-24 |p64| + eps_case * |delta64| and, with its own eps_case,
    <= 2^-24 |p64| + eps_case * (the update's sum of |terms|).  Every element, no NaN.  -> observed ratios."""
    r = ref.r64
    return dict(m=check_gradient(m, r.m, r.terms_m, ref.eps["m"], what + ": m"),
                v=check_gradient(v, r.v, r.terms_v, ref.eps["v"], what + ": v"),
                p=check_gradient(p, r.p, r.delta.abs(), ref.eps["p"], what + ": p", u=U32),
                pt=check_gradient(p, r.p, r.terms_d, ref.eps["pt"], what + ": p against the update's terms", u=U32))


# ------------------------------------------------------------------------------- the data path: augmentation
# Inputs, the fp64 restatement and the checkers of tests/test_gpu_data_path.py (csrc/augment.hip).  tests/test_data_path_util.py
# runs them on the CPU against a numpy model of the kernels' block decomposition with injectable faults.  Arrays of a case are
# numpy [b, c, S] (S = the voxels of one channel); profiles/data_path_bounds.md derives the bound.
AUG_BLOCK_VOX = 2048           # AUG_BLOCK of augment.hip: one partial (min/max pair, then sum) per workgroup
AUG_FINALIZE_STRIDE = 64       # both finalize kernels walk the partials with i += 64
AUG_EPS_FLOOR = 2.0 ** -20     # sixteen fp32 roundings
AUG_SURE = 2.0 ** -16          # an element this far (in the bound's own terms) beyond lo / hi is clipped in any evaluation held to
#                                eps <= 2^-16: its error is that of lo / hi alone


def aug_blocks(spatial):
    return -(-int(spatial) // AUG_BLOCK_VOX)


def augment_ref64(data, params):
    """The three transforms of oracle/ref_augment.apply with the brightness add, the sample's minimum and its range in fp32 (what
    numpy does on the reference's float32 patches, and what the kernels do bit for bit) and everything after that in fp64.
    data [b, c, ...] fp32, params [b, c, 3] fp32 {add, gamma, factor} (gamma of each channel as given: the reference draws one per
    sample).  -> out and its parts, all [b, c, S] / [b, c, 1] fp64, and the per-element norm of the bound:
      e_g  = (g - minm) + |g|                                   the terms of g = p * rnge + minm
      e_m  = mean(e_g) + mean(|g|)                              the mean's
      unc  = |f| (e_g + e_m + |g - mean|) + e_m + |unclipped|   the contrast line's
      norm = e_g at the channel's end where the element is clipped beyond doubt, else max(unc, e_g at both ends)."""
    data = np.asarray(data, dtype=np.float32)
    params = np.asarray(params, dtype=np.float32)
    b, c = data.shape[:2]
    s = data.reshape(b, c, -1) + params[:, :, 0:1]
    assert s.dtype == np.float32
    minm = s.min(axis=(1, 2))
    rnge = s.max(axis=(1, 2)) - minm
    assert minm.dtype == np.float32 and rnge.dtype == np.float32
    m64, r64 = minm.astype(np.float64)[:, None, None], rnge.astype(np.float64)[:, None, None]
    gamma, f = params[:, :, 1:2].astype(np.float64), params[:, :, 2:3].astype(np.float64)
    t = (s.astype(np.float64) - m64) / (r64 + 1e-7)
    g = np.power(t, gamma) * r64 + m64
    mean, lo, hi = g.mean(-1, keepdims=True), g.min(-1, keepdims=True), g.max(-1, keepdims=True)
    unclipped = (g - mean) * f + mean
    out = np.clip(unclipped, lo, hi)
    e_g = (g - m64) + np.abs(g)
    e_m = e_g.mean(-1, keepdims=True) + np.abs(g).mean(-1, keepdims=True)
    e_lo = np.take_along_axis(e_g, g.argmin(-1)[..., None], -1)
    e_hi = np.take_along_axis(e_g, g.argmax(-1)[..., None], -1)
    unc = np.abs(f) * (e_g + e_m + np.abs(g - mean)) + e_m + np.abs(unclipped)
    sure_hi = unclipped - hi > AUG_SURE * (unc + e_hi)
    sure_lo = lo - unclipped > AUG_SURE * (unc + e_lo)
    norm = np.where(sure_hi, e_hi, np.where(sure_lo, e_lo, np.maximum(unc, np.maximum(e_lo, e_hi))))
    return types.SimpleNamespace(out=out, s=s, minm=minm, rnge=rnge, t=t, g=g, mean=mean, lo=lo, hi=hi, unclipped=unclipped, norm=norm,
                                 sure_lo=sure_lo, sure_hi=sure_hi)


def aug_eps(data, params, ref, what):
    """(r32, eps_case): r32 = the error of oracle/ref_augment.apply (numpy fp32 on the CPU) against augment_ref64 in the norm of
    the bound; eps_case = max(2^-20, 8 * r32), which must stay below AUG_SURE (the norm's clip decision relies on it)."""
    from oracle import ref_augment as A
    x32 = A.apply(np.asarray(data, dtype=np.float32), params).reshape(ref.out.shape)
    r32, eps = ref_error(torch.from_numpy(x32), torch.from_numpy(ref.out), torch.from_numpy(ref.norm), what, floor=AUG_EPS_FLOOR)
    assert eps < AUG_SURE, f"{what}: eps_case {eps:.3e} reaches the clip decision's margin 2^-16 (r32 {r32:.3e})"
    return r32, eps


def check_augment(got, ref, eps, what):
    """Every element, none excluded: |got - ref64| <= eps * norm, no NaN.  -> the worst observed |got - ref64| / norm."""
    got = torch.from_numpy(np.asarray(got, dtype=np.float32).reshape(ref.out.shape))
    return check_gradient(got, torch.from_numpy(ref.out), torch.from_numpy(ref.norm), eps, what)


def aug_random_case(tag, b, c, shape, kind="positive", params="drawn"):
    """standard_normal * 40 + 100 like the suite's whole-tensor test; kind "negative": * 40 - 100; "scaled": channel 1 is 1000 times
    channel 0's scale.  With more than AUG_FINALIZE_STRIDE partials the sample's maximum sits in the LAST voxel of channel 0 and its
    minimum in the last voxel of channel c - 1 (the block behind partial 64).  params: "drawn" (oracle.ref_augment.draw_parameters,
    seeded by the tag) or a (shift, gamma, factor) corner given to every sample, the shift's sign alternating by channel."""
    from oracle import ref_augment as A
    g = _np_rng(tag)
    S = int(np.prod(shape))
    x = g.standard_normal((b, c, S)) * 40 + (-100 if kind == "negative" else 100)
    if kind == "scaled" and c > 1:
        x[:, 1] *= 1000.0
    if aug_blocks(S) > AUG_FINALIZE_STRIDE:
        x[:, 0, -1] = x.max(axis=(1, 2)) + 50.0
        x[:, c - 1, -1 if c > 1 else -2] = x.min(axis=(1, 2)) - 50.0
    if isinstance(params, str):
        state = np.random.get_state()
        np.random.seed(int(g.integers(0, 2 ** 31)))
        prm = A.draw_parameters(b, c)
        np.random.set_state(state)
    else:
        prm = np.zeros((b, c, 3), dtype=np.float32)
        prm[:, :, 0] = params[0] * np.where(np.arange(c) % 2, -1.0, 1.0)[None]
        prm[:, :, 1], prm[:, :, 2] = params[1], params[2]
    return types.SimpleNamespace(b=b, c=c, shape=tuple(shape), spatial=S, x=x.astype(np.float32), params=prm)


# ---- the two-valued lattice
def aug_lattice_case(tag, b, c, shape, lh=None, shifted=True):
    """After the brightness shift every channel of sample i holds only L_i and H_i: integers, |.| <= 4096, H - L >= 2 (lh: the (L, H)
    pairs to use).  The shifts are integers, different for every channel of a sample (all 0 with shifted=False); x = {L, H} - add.  The number of H voxels
    differs for every (sample, channel); voxel k * 2048 of every block k and the last voxel hold H, voxel 1 holds L, the rest are
    placed at random.  Then grange = H - L = fl(grange + 1e-7f), t is exactly 0 or 1, powf gives 0 and 1 for any gamma, g is L or H,
    every fp32 block partial is an integer below 2^24 in any order and the fp64 total is exact."""
    g = _np_rng(tag)
    S = int(np.prod(shape))
    nb = aug_blocks(S)
    assert S >= 8 and c <= 64
    forced = np.unique(np.concatenate([np.arange(nb) * AUG_BLOCK_VOX, [S - 1]]))
    free = np.setdiff1d(np.arange(S), np.concatenate([forced, [1]]))
    room = len(free) - 1
    assert room >= b * c, "too few voxels for a different count per (sample, channel)"
    step = max(1, (room * 3 // 4) // (b * c))
    if lh is None:
        lo = g.integers(-4096, 4000, size=b)
        lh = [(int(v), int(v) + int(g.integers(2, 4097 - v))) for v in lo]
    low = np.asarray([p[0] for p in lh], dtype=np.int64)
    high = np.asarray([p[1] for p in lh], dtype=np.int64)
    add = np.stack([g.permutation(np.arange(-40, 41))[:c] for _ in range(b)]).astype(np.int64) * int(shifted)
    mask = np.zeros((b, c, S), dtype=bool)
    mask[:, :, forced] = True
    order = g.permutation(b * c)
    for i in range(b):
        for ch in range(c):
            extra = 1 + int(order[i * c + ch]) * step
            mask[i, ch, g.permutation(free)[:extra]] = True
    lat = np.where(mask, high[:, None, None], low[:, None, None])
    x = (lat - add[:, :, None]).astype(np.float32)
    case = types.SimpleNamespace(b=b, c=c, shape=tuple(shape), spatial=S, x=x, add=add.astype(np.float32), mask=mask, low=low, high=high,
                                 lat=lat.astype(np.float32), nhigh=mask.sum(-1), shifted=shifted)
    aug_lattice_premises(case)
    return case


def aug_lattice_premises(case):
    """The premises of the exact part, in fp32 on the CPU.  -> the exact sums [b, c] (Python integers in an object array)."""
    low, high = case.low, case.high
    assert bool((np.abs(low) <= 4096).all() and (np.abs(high) <= 4096).all() and (high - low >= 2).all())
    assert len(set(case.nhigh.reshape(-1).tolist())) == case.b * case.c, "the H counts must differ per (sample, channel)"
    for i in range(case.b):
        assert not case.shifted or len(set(case.add[i].tolist())) == case.c, "the shifts must differ per channel"
    s = case.x + case.add[:, :, None]
    assert s.dtype == np.float32 and np.array_equal(s, case.lat)                       # the shifted values are L and H exactly
    gmin, gmax = s.min(axis=(1, 2)), s.max(axis=(1, 2))
    assert np.array_equal(gmin, low.astype(np.float32)) and np.array_equal(gmax, high.astype(np.float32))
    grange = gmax - gmin
    assert grange.dtype == np.float32 and np.array_equal(grange + np.float32(1e-7), grange)      # fl(grange + 1e-7f) = grange
    t = (s - gmin[:, None, None]) / (grange + np.float32(1e-7))[:, None, None]
    assert t.dtype == np.float32 and set(np.unique(t).tolist()) <= {0.0, 1.0} and np.array_equal(t == 1.0, case.mask)
    for gamma in (0.7, 1.0, 1.3):
        assert set(np.unique(np.power(t, np.float32(gamma))).tolist()) <= {0.0, 1.0}
    nb = aug_blocks(case.spatial)
    pad = np.zeros((case.b, case.c, nb * AUG_BLOCK_VOX))
    pad[:, :, :case.spatial] = np.abs(case.lat)
    part = pad.reshape(case.b, case.c, nb, AUG_BLOCK_VOX).sum(-1)
    assert float(part.max()) < FP32_EXACT, "a block's sum of |g| reaches 2^24"
    assert bool((case.mask.reshape(case.b, case.c, -1)[:, :, np.arange(nb) * AUG_BLOCK_VOX]).all()) and bool(case.mask[:, :, -1].all())
    sums = np.empty((case.b, case.c), dtype=object)
    for i in range(case.b):
        for ch in range(case.c):
            k = int(case.nhigh[i, ch])
            sums[i, ch] = k * int(high[i]) + (case.spatial - k) * int(low[i])
    return sums


def aug_lattice_mean32(case):
    """What aug_finalize2_kernel stores: (float)(sum / count), both exact in fp64.  [b, c] fp32, strictly between L and H."""
    sums = aug_lattice_premises(case)
    mean = np.empty((case.b, case.c), dtype=np.float32)
    for i in range(case.b):
        for ch in range(case.c):
            mean[i, ch] = np.float32(np.float64(sums[i, ch]) / np.float64(case.spatial))
    assert bool((mean > case.low[:, None]).all() and (mean < case.high[:, None]).all())
    return mean


def aug_lattice_params(case, gamma, factor, shift=True):
    prm = np.zeros((case.b, case.c, 3), dtype=np.float32)
    if shift:
        prm[:, :, 0] = case.add
    prm[:, :, 1], prm[:, :, 2] = gamma, factor
    return prm


def _as5(a, case):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).reshape((case.b, case.c, 1) + case.shape)))


def check_aug_lattice_mean(got, case, what):
    """Contrast factor 0: clip(fma(g - mean, 0, mean), lo, hi) is the channel's mean in every voxel, bit for bit."""
    want = np.broadcast_to(aug_lattice_mean32(case)[:, :, None], (case.b, case.c, case.spatial))
    return assert_exact(_as5(got, case), _as5(want, case), what + ": factor 0 -> f32(S / count)")


def check_aug_lattice_extremes(got, case, what):
    """Contrast factor 2^40: a voxel that held L becomes lo = L, one that held H becomes hi = H, bit for bit."""
    return assert_exact(_as5(got, case), _as5(case.lat, case), what + ": factor 2^40 -> L / H")


def check_aug_lattice_factor(got, case, factor, what):
    """A factor of few bits: |got - ref64| <= 2^-24 (|f| |g - mean| + |out|) against the fp64 evaluation of
    clip(fma(fl32(g - mean), f, mean), L, H) with the exact fp32 mean.  -> the number of voxels that are not bit-equal to the
    reference rounded to fp32."""
    mean = aug_lattice_mean32(case)[:, :, None]
    d32 = case.lat - mean
    assert d32.dtype == np.float32
    lo, hi = case.low.astype(np.float64)[:, None, None], case.high.astype(np.float64)[:, None, None]
    ref = np.clip(d32.astype(np.float64) * float(factor) + mean.astype(np.float64), lo, hi)
    norm = abs(float(factor)) * np.abs(case.lat.astype(np.float64) - mean.astype(np.float64)) + np.abs(ref)
    got = np.asarray(got, dtype=np.float32).reshape(ref.shape)
    check_gradient(torch.from_numpy(got), torch.from_numpy(ref), torch.from_numpy(norm), U32, what + f": factor {factor}")
    return int((got != ref.astype(np.float32)).sum())


def aug_two_channel_case(tag, b, shape):
    """Samples of two channels after the shift: channel 0 holds L and M, channel 1 holds M and H, M = (L + H) / 2, H - L a multiple
    of 4: the sample's minimum lies in channel 0 and its maximum in channel 1, t is 0, 1/2 or 1 exactly.  lo / hi of channel 0 are
    L and g(1/2), of channel 1 g(1/2) and H, while gmin and grange are the sample's."""
    g = _np_rng(tag)
    S = int(np.prod(shape))
    low = g.integers(-2000, 1000, size=b)
    high = low + 4 * g.integers(1, 500, size=b)
    mid = (low + high) // 2
    add = np.stack([g.permutation(np.arange(-9, 10))[:2] for _ in range(b)]).astype(np.int64)
    upper = g.random((b, 2, S)) < 0.4
    upper[:, :, 0], upper[:, :, 1], upper[:, :, -1] = True, False, True
    lat = np.empty((b, 2, S), dtype=np.int64)
    lat[:, 0] = np.where(upper[:, 0], mid[:, None], low[:, None])
    lat[:, 1] = np.where(upper[:, 1], high[:, None], mid[:, None])
    x = (lat - add[:, :, None]).astype(np.float32)
    half = lat == mid[:, None, None]
    s = x + add.astype(np.float32)[:, :, None]
    t = (s - s.min(axis=(1, 2), keepdims=True)) / ((s.max(axis=(1, 2)) - s.min(axis=(1, 2))) + np.float32(1e-7))[:, None, None]
    assert t.dtype == np.float32 and set(np.unique(t).tolist()) == {0.0, 0.5, 1.0} and np.array_equal(t == 0.5, half)
    return types.SimpleNamespace(b=b, c=2, shape=tuple(shape), spatial=S, x=x, add=add.astype(np.float32), lat=lat.astype(np.float32),
                                 half=half, low=low, high=high)


def check_aug_two_channel(got, case, ref, eps, what):
    """Contrast factor 2^40 on aug_two_channel_case: the voxels that held L and H come back as L and H bit for bit (each channel is
    clipped to ITS OWN ends, the gamma map runs on the SAMPLE's range); the voxels at t = 1/2 are an end of their channel, g(1/2), held
    to the random part's bound."""
    got = np.asarray(got, dtype=np.float32).reshape(case.b, 2, case.spatial)
    bad = (got != case.lat) & ~case.half
    assert not bad.any(), f"{what}: {int(bad.sum())} of {int((~case.half).sum())} L / H voxels differ; first at {tuple(np.argwhere(bad)[0])}"
    assert bool((ref.sure_lo | ref.sure_hi).all()), what + ": a voxel is not clipped beyond doubt at factor 2^40"
    return check_augment(got, ref, eps, what)


# ------------------------------------------------------------------------------- the rounding lattice
# Inputs of tests/test_gpu_rounding.py keep "every fp32 partial sum is exact" and DROP "the result is a number of the output
# type": the accumulator holds the exact result, the kernel rounds once, and ref64.to(dtype) is the one correct answer.  The
# helpers below count, on the reference alone, what such a case needs in order to tell the roundings apart.
def neighbours(v, dtype):
    """v (fp64) -> (towards, away): the `dtype` numbers next to v on the side of zero and on the far side, both v itself where
    v is a number of the type; fp64 tensors, the sign of a zero kept, `away` +-inf beyond the largest finite number."""
    v = v.detach().double()
    r = v.to(dtype)
    bits = r.view(torch.int16)       # sign-magnitude patterns: one less is the next number towards zero, for both signs
    t_bits = bits - (r.double().abs() > v.abs()).to(torch.int16)
    towards = t_bits.view(dtype).double()
    away = (t_bits + (towards != v).to(torch.int16)).view(dtype).double()
    return towards, away


def rounding_census(v, dtype):
    """What a reference holds: .rne = v.to(dtype) (fp64), the neighbours, and masks .nonrep (no number of the type), .tie_zero /
    .tie_away (exactly half way; round-to-nearest-even goes towards / away from zero), .sub (stored as a nonzero subnormal),
    .zeroed (nonzero, stored as a signed zero), .inf (stored as +-inf)."""
    v = v.detach().double()
    rne = v.to(dtype).double()
    towards, away = neighbours(v, dtype)
    top = 2.0 * 2.0 ** float(np.floor(np.log2(torch.finfo(dtype).max)))       # the number after the largest finite one
    far = torch.where(torch.isinf(away), torch.sign(away) * top, away)
    nonrep = towards != v
    tie = nonrep & ((v - towards).abs() == (far - v).abs())
    tiny = torch.finfo(dtype).smallest_normal
    return types.SimpleNamespace(v=v, rne=rne, towards=towards, away=away, nonrep=nonrep, tie_zero=tie & (rne == towards),
                                 tie_away=tie & (rne == away), sub=(rne != 0) & (rne.abs() < tiny), zeroed=(v != 0) & (rne == 0),
                                 inf=torch.isinf(rne))


def census_counts(cen):
    n = lambda m: int(m.sum())
    return dict(elements=cen.v.numel(), nonrep=n(cen.nonrep), tie_zero=n(cen.tie_zero), tie_away=n(cen.tie_away), sub=n(cen.sub),
                zeroed=n(cen.zeroed), inf=n(cen.inf))


def assert_rounding_premises(v, dtype, what, nonrep=0.25, ties=100, sub=0, sub_ties=0, zeroed=0, inf=None):
    """Conditions under which equality with v.to(dtype) tells the roundings apart -- on the reference alone: at least `nonrep` of
    the elements are no numbers of the type, at least `ties` exact ties resolve towards zero and as many away from it; at least
    `sub` elements are stored as nonzero subnormals with `sub_ties` ties among them in each direction; at least `zeroed` nonzero
    elements lie below half the smallest subnormal (or on that tie) and are stored as a signed zero; inf = None: every element
    is finite, inf = (lo, hi): the share of +-inf lies in [lo, hi], both signs occur, and the rest is finite.  -> the census."""
    v = v.detach().double()
    assert bool(torch.isfinite(v).all()), f"{what}: the fp64 reference is not finite"
    cen = rounding_census(v, dtype)
    k = census_counts(cen)
    assert k["nonrep"] >= nonrep * k["elements"], f"{what}: only {k['nonrep']} of {k['elements']} reference elements are no {dtype} numbers"
    assert k["tie_zero"] >= ties and k["tie_away"] >= ties, f"{what}: {k['tie_zero']} ties towards zero, {k['tie_away']} away, {ties} wanted of each"
    assert k["sub"] >= sub, f"{what}: {k['sub']} subnormal results, {sub} wanted"
    assert k["zeroed"] >= zeroed, f"{what}: {k['zeroed']} nonzero results are stored as a zero, {zeroed} wanted"
    if sub_ties:
        tz, ta = int((cen.tie_zero & (cen.sub | cen.zeroed)).sum()), int((cen.tie_away & cen.sub).sum())
        assert tz >= sub_ties and ta >= sub_ties, f"{what}: {tz} / {ta} subnormal ties towards zero / away, {sub_ties} wanted of each"
    if inf is None:
        assert k["inf"] == 0, f"{what}: {k['inf']} reference elements overflow {dtype}"
    else:
        share = k["inf"] / k["elements"]
        assert inf[0] <= share <= inf[1], f"{what}: {share:.3%} of the reference elements overflow, wanted {inf[0]:.0%} .. {inf[1]:.0%}"
        assert bool((cen.rne == float("inf")).any()) and bool((cen.rne == float("-inf")).any()), f"{what}: one sign of infinity is missing"
    return cen


def assert_rounded(got, v, dtype, what):
    """Every element of `got` equals v.to(dtype): ONE round-to-nearest-even of the exact value -- subnormals kept, +-inf from
    65520 on, no NaN -- and a nonzero value that rounds to zero comes out as the zero of ITS sign.  -> elements compared."""
    v = v.detach().double().cpu()
    want = v.to(dtype)
    total = assert_exact(got, want, what)
    g = got.detach().cpu()
    flipped = (want == 0) & (v != 0) & (torch.signbit(g.double()) != torch.signbit(want.double()))
    if bool(flipped.any()):
        i = tuple(flipped.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(flipped.sum())} zeros carry the wrong sign; first at {i}: exact value {v[i].item()!r}")
    return total


def report_rounding(item, what, kernel, elements, counts):
    """The `[exact]` line of a rounding comparison: what was compared and what the reference held."""
    print(f"[exact] item={item} {what} kernel={kernel} elements={elements} nonrep={counts['nonrep']} ties={counts['tie_zero']}/{counts['tie_away']} "
          f"subnormal={counts['sub']} zeroed={counts['zeroed']} inf={counts['inf']}")


def add_counts(total, k):
    for name, val in k.items():
        total[name] = total.get(name, 0) + val
    return total
