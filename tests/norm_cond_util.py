"""Inputs, fp64 references, bounds and a NumPy restatement for the conditioning tests of the normalisation kernels
(csrc/norm_act.hip; tests/test_gpu_norm_conditioning.py asserts with them, tests/test_norm_cond_util.py runs all of it on the CPU).

INPUTS.  x = m + sigma * g per (sample, channel), g a fixed-seed Gaussian, sigma = 1, m_c = R * (1 + j_c) with a per-channel jitter
|j_c| <= 2^-13 (the channels of a group get different offsets, but the spread R * j stays below sigma: the group's mean / std stays
~R).  Where a tensor has at least four units (a unit: a GroupNorm group of sample 0, a BatchNorm channel), unit 1 is CONSTANT
(sigma = 0, value 1000.5 -- not a power of two) and unit 2 NEAR-CONSTANT (sigma = 2^-10 * m, m = R or 1000.5 when R = 0: mean / std
= 1024 whatever R is).  GroupNorm: the last sample (of two or more) has the offsets negated.  BatchNorm: the last quarter of the
channels.  The tensor is rounded to the storage type before anything is derived from it.

REFERENCE.  Two passes in fp64 on the CPU, written out: mean, biased variance, rstd = 1 / sqrt(var + eps), xhat, the affine,
ReLU, and the closed-form backward  dx = rstd * (gamma * du - m1 - xhat * m2),  m1 = mean(gamma * du),  m2 = mean(gamma * du *
xhat) over the unit,  dgamma = sum du * xhat,  dbeta = sum du; BatchNorm's running statistics with the unbiased variance.  eps is the
fp32 value the entry points receive.

BOUNDS.  u = 2^-24 (half an fp32 ulp, relative).  Per unit, s = sqrt(var + eps) and R = |mean| / s from the reference (so the
constant unit has R = 1000.5 / sqrt(eps) ~ 3e5, the near-constant one 1024).  Every bound has the form
        MARGIN * u * (a + b * R) * max(1, |xhat|) * scale          (+ half an ulp of the output in 16-bit storage)
with a, b the count of roundings a correct fp32 implementation cannot avoid.  There is NO R^2 term: that is what a variance taken
as sum x^2 / N - mean^2 from fp32 sums has, and what these tests exist to see.  The counts (scale in brackets):

  mean    [s]          a = A_SUM (1 + P)    the fp32 sums of the shifted data, counted as A_SUM = 2 roundings (a thread's chain,
                                            the sum across threads; the totals of the rows are fp64), of terms of size (1 + P) s
                       b = 1                mean is stored as fp32: u * |mean| = u * R * s
  rstd    [rstd]       a = 2 + A_SUM (1 + P^2)   var, var + eps, the square root and the fp32 store: 2; the sum of squares of the
                                            shifted data, which is (1 + P^2) times the variance
                       b = 1/2              a one-pass fp32 variance (Welford's, ATen's) rounds its running mean at every step:
                                            u R s in each deviation, 2 u R |xhat| in each square, signs mixed -- counted as a half
                       a CONSTANT unit (var = 0): a = 2, b = 0 -- every deviation from a shift or a running mean taken from the
                                            data is exactly 0, only var + eps, the root and the store round: rstd = 1 / sqrt(eps)
  coef a  [|a|]        rstd's, a + 1        the product gamma * rstd
  coef b  [|gamma|]    a = a(mean) + 2 |beta / gamma|,  b = 3: mean's rounding, the product mean * a, the final rounding -- against
                       beta - mean * a with the fp64 mean and the coef a THAT WAS RETURNED: a's own error times the mean is R times
                       rstd's error, an R^2 term that cancels in z when b is formed from the rounded a, as it must be
  z       [|gamma|]    a = a(coef a) + 1 + a(coef b),  b = b(rstd) + 3     a's error acts on x - mean only: (a + b R)(rstd) |xhat|;
                                            the fma: 1; coef b's
  dx      [rstd * (|gamma du| + rms(gamma du))]
                       a = 3 a(rstd) + 2 A_SUM + 4       rstd enters three times; the two sums; k1, k2, k3 and the final fma
                       b = 3 b(rstd) + 4    mean's rounding in k3 and in xhat, the rounding of k2 (times x) and of k3: both ~ R
  dgamma  [sum |du| (1 + |xhat|)]   a = a(rstd) + A_SUM + 1,  b = b(rstd) + 1 (mean's rounding moves every xhat by u * R)
  dbeta   [sum |du|]   a = A_SUM + 1, b = 0
  running_mean / running_var: momentum times the bounds of mean and of var (= 2 * rstd's, relative to var + eps) plus one rounding of
  the blend.

P: a pass that shifts the data before it sums takes the shift from the data -- the contract of mednet_gn_stats / mednet_bn_stats is
the first channel of the unit at voxel 0 (of sample 0 for BatchNorm) --, so the shifted data has a ratio of its own,
P = |x_shift - mean| / s <= max |xhat|; it is read from the reference.  A pass that does not shift (ATen's) is inside the same bound.

MARGIN = 4, over those counts: the fp32 sums of the tested shapes are chains of at most 8-24 additions per thread and a sum over at
most 256 threads; rounding errors of a chain of L additions grow as sqrt(L / 3) * 0.6 u in the mean and as L * u at worst, and
A_SUM * MARGIN = 8 >= 0.6 * sqrt(280 / 3) = 5.8.  test_norm_cond_util.py shows that ATen's own fp32 group_norm / batch_norm stays
inside these bounds at every R used (the bound is no tighter than the reference the project is held to), and that the restated
sum-of-squares formula leaves them at R = 4096.
"""
import types
import zlib

import numpy as np
import torch

U32 = 2.0 ** -24
MARGIN = 4.0
A_SUM = 2.0
B_RSTD = 0.5
EPS = float(np.float32(1e-5))
CONSTANT = 1000.5
RATIOS = {"fp32": (0, 16, 256, 4096), "fp16": (0, 16, 64), "bf16": (0, 4, 16)}
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
MANT = {"bf16": 8, "fp16": 11, "fp32": 24}          # significant bits
EMIN = {"bf16": -126, "fp16": -14, "fp32": -126}

# (n, C, groups, shape): the smallest shapes that reach each path of the statistics pass
GN_SHAPES = {"small": (2, 32, 8, (8, 8, 8)),        # one or two chunks: the per-thread chain dominates
             "ragged": (2, 32, 8, (16, 16, 24)),    # many chunks, a ragged last one
             "first": (1, 1, 1, (8, 16, 16)),       # the 'gcr' first layer: one channel, vector width 1, 256 rows
             "wide": (2, 64, 8, (8, 8, 8))}         # 16-bit modes: vector width 8
BN_SHAPE = (3, 32, (8, 8, 8))
MOMENTUM = 0.1
MOMENTUM_F32 = float(np.float32(MOMENTUM))


def _rng(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


def to_storage(t, mode):
    return t.to(DT[mode]).double()


def half_ulp(ref, mode):
    """Half the spacing of the storage type at |ref| (0 for fp32 storage: the fp32 roundings are in the counts)."""
    if mode == "fp32":
        return torch.zeros_like(ref)
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** EMIN[mode]))).clamp_min(EMIN[mode])
    return 0.5 * torch.pow(2.0, e - (MANT[mode] - 1))


# ------------------------------------------------------------------------------------------------ inputs
def make_case(tag, n, c, groups, shape, R, mode, batch=False):
    """x, dz, gamma, beta (fp64 CPU, x and dz rounded to the storage type) of one case.  groups is ignored for BatchNorm."""
    g = _rng(f"cond:{tag}:{n}:{c}:{groups}:{shape}:{batch}")
    noise = torch.from_numpy(g.standard_normal((n, c, *shape)))
    jitter = torch.from_numpy(g.uniform(-1.0, 1.0, c)) * 2.0 ** -13
    m = (float(R) * (1.0 + jitter))[None].repeat(n, 1)
    sigma = torch.ones(n, c, dtype=torch.float64)
    units = c if batch else groups
    cg = 1 if batch else c // groups
    special = {}
    if batch:
        m[:, c - c // 4:] *= -1.0
    elif n > 1:
        m[n - 1] *= -1.0
    if units >= 4:
        rows = slice(None) if batch else slice(0, 1)
        m[rows, cg:2 * cg], sigma[rows, cg:2 * cg] = CONSTANT, 0.0
        mn = float(R) if R else CONSTANT
        m[rows, 2 * cg:3 * cg], sigma[rows, 2 * cg:3 * cg] = mn, mn * 2.0 ** -10
        special = {"constant": 1, "near-constant": 2}
    bc = (n, c) + (1,) * len(shape)
    x = to_storage(m.reshape(bc) + sigma.reshape(bc) * noise, mode)
    # du with a mean and a component along xhat: m1 and m2 of the backward are O(1), so k2 * x + k3 matters
    dz = to_storage(torch.from_numpy(g.standard_normal((n, c, *shape))) + 0.5 + 0.5 * noise, mode)
    gamma = torch.from_numpy(g.uniform(0.5, 1.5, c)).float().double()
    beta = torch.from_numpy(g.uniform(-0.5, 0.5, c)).float().double()
    return types.SimpleNamespace(tag=tag, n=n, c=c, groups=units, cg=cg, shape=tuple(shape), spatial=int(np.prod(shape)), R=R, mode=mode,
                                 batch=batch, x=x, dz=dz, gamma=gamma, beta=beta, special=special, eps=EPS)


# ------------------------------------------------------------------------------------------------ reference (fp64, two passes)
def _units(case, t):
    """[n, c, *shape] -> [units, elements]: a row per statistics unit (GroupNorm: (sample, group); BatchNorm: channel)."""
    n, c = case.n, case.c
    t = t.reshape(n, c, -1)
    if case.batch:
        return t.permute(1, 0, 2).reshape(c, -1)
    return t.reshape(n * case.groups, -1)


def _from_units(case, r):
    n, c = case.n, case.c
    if case.batch:
        return r.reshape(c, n, -1).permute(1, 0, 2).reshape(n, c, *case.shape)
    return r.reshape(n, c, *case.shape)


def _per_channel(case, v):
    """A per-unit vector -> [n, c]."""
    if case.batch:
        return v[None].expand(case.n, -1)
    return v.reshape(case.n, case.groups).repeat_interleave(case.cg, dim=1)


def reference(case, act="relu", rm0=None, rv0=None):
    """Everything the tests compare, in fp64.  z = act(gamma * xhat + beta); the backward takes act' from the stored z."""
    xs = _units(case, case.x)
    count = xs.shape[1]
    mean = xs.sum(1) / count
    var = ((xs - mean[:, None]) ** 2).sum(1) / count
    rstd = 1.0 / torch.sqrt(var + case.eps)
    xhat = _from_units(case, (xs - mean[:, None]) * rstd[:, None])
    bc = (1, case.c) + (1,) * len(case.shape)
    gam, bet = case.gamma.reshape(bc), case.beta.reshape(bc)
    y = gam * xhat + bet
    z = torch.relu(y) if act == "relu" else y
    zs = to_storage(z, case.mode)
    du = case.dz * (zs > 0) if act == "relu" else case.dz
    gd = gam * du
    m1 = _units(case, gd).sum(1) / count
    m2 = _units(case, gd * xhat).sum(1) / count
    rms = torch.sqrt((_units(case, gd) ** 2).sum(1) / count)
    full = lambda v: _from_units(case, v[:, None].expand(-1, count))
    dx = full(rstd) * (gd - full(m1) - xhat * full(m2))
    red = (0,) + tuple(range(2, 2 + len(case.shape)))
    a = case.gamma[None] * _per_channel(case, rstd)
    r = types.SimpleNamespace(count=count, mean=mean, var=var, rstd=rstd, s=torch.sqrt(var + case.eps), xhat=xhat, y=y, z=z, z_stored=zs, du=du,
                              dx=dx, dgamma=(du * xhat).sum(red), dbeta=du.sum(red), m1=m1, m2=m2, rms=rms, coef_a=a,
                              coef_b=case.beta[None] - _per_channel(case, mean) * a,
                              abs_du=du.abs().sum(red), abs_du_xhat=(du.abs() * (1 + xhat.abs())).sum(red))
    r.R = mean.abs() / r.s
    r.P = (xs[:, 0] - mean).abs() / r.s
    if rm0 is not None:
        unbiased = var * (count / (count - 1.0))
        r.running_mean = (1.0 - MOMENTUM_F32) * rm0 + MOMENTUM_F32 * mean
        r.running_var = (1.0 - MOMENTUM_F32) * rv0 + MOMENTUM_F32 * unbiased
    return r


# ------------------------------------------------------------------------------------------------ bounds
def bounds(case, r):
    """The bound of every compared quantity, shaped like the quantity (see the module docstring for the counts)."""
    u, M = U32, MARGIN
    R, s, rstd = r.R, r.s, r.rstd
    Rc, rc = _per_channel(case, R), _per_channel(case, rstd)
    g, b = case.gamma.abs()[None], case.beta.abs()[None]
    full = lambda v: _from_units(case, v[:, None].expand(-1, r.count))
    bc = (1, case.c) + (1,) * len(case.shape)
    xh = r.xhat.abs().clamp_min(1.0)
    a_mean, a_rstd = A_SUM * (1.0 + r.P), 2.0 + A_SUM * (1.0 + r.P ** 2)
    rel_rstd = a_rstd + B_RSTD * R                                  # rstd's (a + b R), per unit
    rel_rstd = torch.where(r.var == 0, torch.full_like(R, 2.0), rel_rstd)   # a constant unit: every deviation is exactly 0
    a_coef_b = _per_channel(case, a_mean) + 2.0 * b / g             # [n, c]
    B = types.SimpleNamespace()
    B.mean = M * u * (a_mean + R) * s
    B.rstd = M * u * rel_rstd * rstd
    B.coef_a = M * u * (_per_channel(case, rel_rstd) + 1.0) * r.coef_a.abs()
    B.coef_b = M * u * (a_coef_b + 3.0 * Rc) * g
    per_elem = lambda t: t.reshape(case.n, case.c, *(1,) * len(case.shape))
    B.z = M * u * (per_elem(_per_channel(case, rel_rstd) + 2.0 + a_coef_b) + 3.0 * full(R)) * xh * case.gamma.abs().reshape(bc)
    B.z = B.z + half_ulp(r.z.abs() + B.z, case.mode)
    scale = full(rstd) * ((case.gamma.reshape(bc) * r.du).abs() + full(r.rms))
    B.dx = M * u * (3.0 * full(rel_rstd) + 2.0 * A_SUM + 4.0 + 4.0 * full(R)) * xh * scale
    B.dx = B.dx + half_ulp(r.dx.abs() + B.dx, case.mode)
    B.dgamma = M * u * (_per_channel(case, rel_rstd + A_SUM + 1.0 + R).max(0).values) * r.abs_du_xhat
    B.dbeta = M * u * (A_SUM + 1.0) * r.abs_du
    if hasattr(r, "running_mean"):
        B.running_mean = MOMENTUM_F32 * B.mean + u * r.running_mean.abs()
        B.running_var = MOMENTUM_F32 * 2.0 * M * u * rel_rstd * (r.var + case.eps) * (r.count / (r.count - 1.0)) + u * r.running_var.abs()
    return B


def _ratio(err, bound):
    """err / bound; where the bound is 0 (a channel whose every du is masked: sums of zeros) only an exact result passes."""
    return torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))


def worst_ratio(got, ref, bound, what):
    """max |got - ref| / bound over EVERY element; a NaN, an Inf or a shape mismatch is a failure."""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} of {got.numel()} elements are NaN / Inf / unwritten"
    assert bool((bound >= 0).all()) and bool(torch.isfinite(bound).all()), f"{what}: the bound is not finite"
    return float(_ratio((got - ref).abs(), bound).max())


def unit_ratios(case, got, ref, bound):
    """Per statistics unit, the worst |got - ref| / bound of a per-unit vector (mean, rstd): {"plain": ..., "constant": ..., ...}."""
    q = _ratio((got.detach().double().cpu().reshape(ref.shape) - ref).abs(), bound).reshape(-1)
    out = {k: float(q[i]) for k, i in case.special.items()}
    keep = torch.ones_like(q, dtype=torch.bool)
    for i in case.special.values():
        keep[i] = False
    out["plain"] = float(q[keep].max())
    return out


# ------------------------------------------------------------------------------------------------ NumPy restatement (fp32 storage)
def pick_vec(c, mode):
    if mode == "fp32" and c % 4 == 0 and c // 4 <= 256:
        return 4
    return 8 if c % 8 == 0 and c // 8 <= 256 else 1


def chunk_plan(spatial, c, vec):
    rows = 256 // (c // vec)
    cv = max((spatial + 1023) // 1024, rows * 8)
    cv = (cv + rows - 1) // rows * rows
    return cv, (spatial + cv - 1) // cv


def partial_rows_model(x, vec, pivot=None):
    """gn_partial_kernel on x[S][C] (float32): rows[chunks][C][2] = {sum (x - p), sum (x - p)^2}: a thread's chain over its voxels
    v0 + row, v0 + row + rows, ... in fp32 (the square through an fma: one rounding), then the sum over the rows of a column in
    order, fp32.  pivot: [C] float32 or None (the sums of x itself)."""
    S, C = x.shape
    rows = 256 // (C // vec)
    cv, chunks = chunk_plan(S, C, vec)
    p = np.zeros(C, np.float32) if pivot is None else pivot.astype(np.float32)
    out = np.zeros((chunks, C, 2), np.float32)
    for ch in range(chunks):
        v0, v1 = ch * cv, min((ch + 1) * cv, S)
        acc_s, acc_q = np.zeros((rows, C), np.float32), np.zeros((rows, C), np.float32)
        for v in range(v0, v1, rows):
            k = min(rows, v1 - v)
            d = (x[v:v + k] - p[None]).astype(np.float32)
            acc_s[:k] = acc_s[:k] + d
            acc_q[:k] = (d.astype(np.float64) * d.astype(np.float64) + acc_q[:k].astype(np.float64)).astype(np.float32)
        s, q = np.zeros(C, np.float32), np.zeros(C, np.float32)
        for r in range(rows):
            s, q = s + acc_s[r], q + acc_q[r]
        out[ch, :, 0], out[ch, :, 1] = s, q
    return out


def gn_stats_model(case, pivoted):
    """mean, rstd [n * groups] (float32 values as float64) of the statistics pass in fp32 storage: pivoted = False restates
    var = sum x^2 / N - mean^2 from the fp32 rows; True the pivoted pass (the group's first channel of voxel 0 is subtracted first)."""
    n, c, G, cg = case.n, case.c, case.groups, case.cg
    vec = pick_vec(c, "fp32")
    x = case.x.reshape(n, c, -1).permute(0, 2, 1).contiguous().numpy().astype(np.float32)      # [n][S][C]
    count = float(case.spatial * cg)
    mean, rstd = np.zeros(n * G), np.zeros(n * G)
    for i in range(n):
        piv = np.repeat(x[i, 0, ::cg], cg) if pivoted else None
        rows = partial_rows_model(x[i], vec, piv).astype(np.float64).sum(0)                     # fp64 totals of the rows
        for k in range(G):
            s, q = rows[k * cg:(k + 1) * cg, 0].sum(), rows[k * cg:(k + 1) * cg, 1].sum()
            ms = s / count
            var = max(q / count - ms * ms, 0.0)
            mean[i * G + k] = np.float32(ms + (float(piv[k * cg]) if pivoted else 0.0))
            rstd[i * G + k] = np.float32(1.0 / np.sqrt(var + float(np.float32(case.eps))))
    return torch.from_numpy(mean), torch.from_numpy(rstd)


def coef_b_reference(case, r, coef_a_got):
    """beta - mean * a with the reference's mean and the coefficient a that was returned (see the docstring: coef b)."""
    return case.beta[None] - _per_channel(case, r.mean) * coef_a_got.detach().double().cpu().reshape(case.n, case.c)
