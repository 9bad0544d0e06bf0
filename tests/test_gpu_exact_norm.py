"""Exact-arithmetic tests of the normalisation family (csrc/norm_act.hip): GroupNorm statistics, coefficients and backward,
BatchNorm, the stand-alone activations -- against ATen (fp64, CPU) with EQUALITY in every element.

gpu_util.norm_lattice builds x = m + sigma * s and du = e + p + q * s per (sample, group) such that mean, rstd, the forward
coefficients, {k1, k2, k3}, dx, dres, dgamma and dbeta are dyadic numbers of the output types and every fp32 partial sum is
exact in any order; eps is an argument of every entry point and is 0 or 3 here (rstd = 1 / sigma or 1 / 2).  The references
are ATen's fp64 group_norm / batch_norm and their autograd, relu / elu and their backward, snapped to the 2^-12 grid
(gpu_util.snap: ATen's fp64 rstd is not exactly 1 / sigma; no element may move by more than 1e-9).  Every test asserts, on the
reference alone, representability of ALL output elements and that the sums of |terms| of the partial rows stay below 2^24,
then equality.  Outputs and the whole workspace start as NaN: a row nobody wrote shows.  tests/test_exact_norm_util.py holds
the CPU side: the conditions for every case, and the proof that equality on these inputs sees a dropped tail voxel, a wrong
group, a missing k2 / k3, a row counted twice, a dres that is not du and a wrong coef row.

EQUAL in every element: stats, coef, bcoef, y, dx, dres, dgamma, dbeta of every GroupNorm / BatchNorm entry point,
running_mean for momentum 0.5 and 0.125, num_batches_tracked, activation none / ReLU forward and backward, ELU backward from
a dyadic z, ELU forward for positive inputs.
ONE ULP, the only two tolerances of this module, both derived and not measured:
  * running_var (every momentum) and running_mean for momentum 0.1f: count / (count - 1) and 0.1f are not dyadic; the kernel
    forms the blend in fp64 and rounds once, so the limit is 1 fp32 ulp of the fp64 reference (which gets the same fp32
    momentum value);
  * ELU forward for negative inputs in 16-bit storage, inputs from {-8, ..., -1/4}: half an ulp of the store plus the fp32
    error of __expf(u) - 1, below 2^-20 relative for |u| >= 1/4 -- 1 ulp of the storage type at the reference.
LEFT to the norm tests (test_gpu_ops.py, test_gpu_batchnorm.py): the fp32 negative side of ELU, ELU recomputed from the
pre-activation (an __expf), and LeakyReLU anywhere (its slope 0.1f is not dyadic).

No plan query exists for these launchers: the tests restate their rules (pick_vec, lds_free_rows_per_wg, 256 % cg,
chunks >= 4096) and assert that the case list reaches every value.  Lines `[exact] item=<h..l> ... elements=<count>`.
"""
import contextlib
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mednet_hip import _lib as L
from oracle import ref_cpu as O

from gpu_util import CL, DEV, DT, assert_exact, assert_representable, assert_sums_exact, lattice, norm_lattice, report, snap

pytestmark = pytest.mark.gpu
MODES = ["bf16", "fp16", "fp32"]
EPS = [0.0, 3.0]
E_UNSUPPORTED = -5
NONE, RELU, ELU = L.ACT_NONE, L.ACT_RELU, L.ACT_ELU

# (n, C, groups, shape): the smallest shapes that reach each path of the launchers (see path_of)
GN_CASES = [(2, 32, 8, (5, 6, 7)),      # 16-bit: vec 8, 4 columns, LDS-free rows, one chunk, one-launch finalize
            (2, 32, 8, (9, 10, 12)),    # three chunks of 512 voxels, the last 56: idle rows
            (1, 256, 8, (3, 5, 9)),     # 32 columns, 8 rows, chunks of 64, the last 7 voxels; cg = 32; odd size: paired channels
            (2, 24, 8, (4, 6, 5)),      # 3 columns: an idle thread, column_reduce through LDS; cg = 3: the four-launch form
            (2, 24, 8, (8, 9, 10)),     # ... two chunks
            (2, 8, 8, (6, 7, 9)),       # cg = 1, one column, 256 rows
            (2, 8, 8, (12, 14, 16)),    # ... two chunks of 2048
            (2, 6, 3, (3, 4, 5)),       # vec 1, 6 columns (42 rows, LDS)
            (2, 4, 1, (3, 4, 5)),       # vec 1 (16-bit), 4 columns, a single group
            (1, 1024, 8, (2, 3, 4))]    # 128 columns: 2 LDS-free rows per workgroup (16-bit storage only)
OPTION_CASES = [GN_CASES[0], GN_CASES[2]]
OPTION_RUNS = [("gn_lds_free", m) for m in MODES] + [("gn_bwd_one_launch", m) for m in MODES] + [("gn_f32_vec4", "fp32")]
POOL_CASES = [(2, 32, 8, (4, 6, 8)), (1, 256, 8, (2, 4, 6)), (2, 8, 8, (6, 8, 10)), (2, 24, 8, (4, 6, 4))]   # even extents, C % 8 == 0
BN_CASES = [(2, 32, (5, 6, 7)), (2, 24, (4, 6, 5)), (2, 6, (3, 4, 5)), (2, 8, (3, 5, 7))]   # (n, C, shape); the last: odd S, even n * S
ACT_COUNTS = [5, 8, 2048 * 3 + 5, 8192 * 2048 + 2048 * 3 + 5]   # the last enters the second trip of the grid-stride loop


def dcode_of(mode):
    return L.dt_of(DT[mode])


def case_id(c):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c)


def gn_modes(case):
    return ["bf16", "fp16"] if case[1] == 1024 else MODES   # (in fp32 C = 1024 is 256 columns, another path: a 16-bit case)


def gn_params():
    return [pytest.param(c, e, m, id=f"{case_id(c)}-{e}-{m}") for c in GN_CASES for e in EPS for m in gn_modes(c)]


# ------------------------------------------------------------------------------------------------ the launchers' rules, restated
def pick_vec(c, mode, f32_vec4=1):
    if mode == "fp32" and c % 4 == 0 and c // 4 <= 256 and f32_vec4:
        return 4
    return 8 if c % 8 == 0 and c // 8 <= 256 else 1


def lds_free_rows_per_wg(cols):
    if cols <= 64:
        return 4 if cols & (cols - 1) == 0 else 0
    return 256 // cols if cols % 64 == 0 and 256 % cols == 0 else 0


def chunk_plan(spatial, c, vec):
    rows = 256 // (c // vec)
    cv = max((spatial + 1023) // 1024, rows * 8)
    cv = (cv + rows - 1) // rows * rows
    return cv, (spatial + cv - 1) // cv


def partial_rows_max(c):
    best = 1
    for mode in ("fp32", "bf16"):
        cols = c // pick_vec(c, mode)
        best = max(best, lds_free_rows_per_wg(cols) if cols <= 256 else 0)
    return 1024 * best


def path_of(case, mode, opts=()):
    """What the launchers choose for a case: vector width, LDS-free rows per workgroup (0: column_reduce through LDS), whether a
    thread idles (256 % cols), whether the last chunk is shorter than the rows of a workgroup, one-launch finalize."""
    n, c, groups, shape = case
    vec = pick_vec(c, mode, 0 if "gn_f32_vec4" in opts else 1)
    cols = c // vec
    cv, chunks = chunk_plan(int(np.prod(shape)), c, vec)
    tail = int(np.prod(shape)) - (chunks - 1) * cv
    return dict(vec=vec, rpw=0 if "gn_lds_free" in opts else lds_free_rows_per_wg(cols), idle=256 % cols != 0, chunks=chunks,
                short_tail=tail < 256 // cols, one_launch=256 % (c // groups) == 0 and "gn_bwd_one_launch" not in opts)


def assert_case_list_reaches_every_path():
    seen = [path_of(c, m) for c in GN_CASES for m in gn_modes(c)] + [path_of(c, m, (o,)) for c in OPTION_CASES for o, m in OPTION_RUNS]
    assert {p["vec"] for p in seen} == {1, 4, 8}
    assert {p["rpw"] for p in seen} == {0, 2, 4}
    assert {p["idle"] for p in seen} == {True, False} and {p["one_launch"] for p in seen} == {True, False}
    assert any(p["short_tail"] for p in seen) and any(p["chunks"] > 1 for p in seen) and any(p["chunks"] == 1 for p in seen)
    assert any(p["vec"] == 8 for p in (path_of(c, "fp32", ("gn_f32_vec4",)) for c in OPTION_CASES))


@contextlib.contextmanager
def options(*names):
    """Kernel-form knobs of norm_act.hip set to 0 for a block, restored to their default 1 afterwards."""
    lib = L.lib()
    try:
        for k in names:
            assert lib.mednet_set_option(k.encode(), 0) == 0
        yield
    finally:
        for k in names:
            lib.mednet_set_option(k.encode(), 1)


# ------------------------------------------------------------------------------------------------ references (ATen, fp64, CPU)
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def lat(n, c, groups, shape, eps, batch=False, nonneg=False):
    key = ("lat", n, c, groups, tuple(shape), eps, batch, nonneg)
    return cached(key, lambda: norm_lattice(f"exn{key[1:]}", n, c, groups, shape, eps, batch=batch, nonneg=nonneg))


def act_backward(dz, z, act):
    """du = dz * act'(.) from the activation OUTPUT, as ATen's autograd of relu_ / elu_ computes it."""
    if act == RELU:
        return torch.ops.aten.threshold_backward(dz, z, 0.0)
    if act == ELU:
        return torch.ops.aten.elu_backward(dz, 1.0, 1.0, 1.0, True, z)
    return dz


def per_channel(t, cg):
    return t.repeat_interleave(cg, dim=1)


def forward_ref(lt, beta):
    """y, stats[n][g] = {mean, rstd}, coef[n][c] = {gamma * rstd, beta - mean * gamma * rstd} (BatchNorm: g = c, rows replicated)."""
    x, g, b = lt.x.double(), lt.gamma.double(), beta.double()
    if lt.batch:
        y, mean, rstd = torch.ops.aten.native_batch_norm(x, g, b, None, None, True, 0.0, lt.eps)
        mean, rstd = mean[None].expand(lt.n, -1), rstd[None].expand(lt.n, -1)
    else:
        y, mean, rstd = torch.ops.aten.native_group_norm(x.contiguous(), g, b, lt.n, lt.c, lt.spatial, lt.groups, lt.eps)
    mean, rstd = snap(mean.reshape(lt.n, lt.groups)), snap(rstd.reshape(lt.n, lt.groups))
    a = g[None] * per_channel(rstd, lt.cg)
    coef = torch.stack((a, b[None] - per_channel(mean, lt.cg) * a), -1)
    return snap(y), torch.stack((mean, rstd), -1), coef


def backward_ref(lt, beta, du, frozen=False):
    """dx, dgamma, dbeta of ATen's autograd for the gradient du of the normalisation's output."""
    x, g, b = (t.double().clone().requires_grad_(True) for t in (lt.x, lt.gamma, beta))
    if lt.batch and frozen:
        y = torch.batch_norm(x, g, b, lt.m[0].clone(), (lt.sigma[0] ** 2).clone(), False, 0.0, lt.eps, False)
    elif lt.batch:
        y = torch.batch_norm(x, g, b, None, None, True, 0.0, lt.eps, False)   # (F.batch_norm refuses eps = 0)
    else:
        y = F.group_norm(x, lt.groups, g, b, lt.eps)
    y.backward(du.double())
    return snap(x.grad), snap(g.grad), snap(b.grad)


def channel_sums(t):
    return t.double().flatten(2).sum(-1)    # [n, c]


def bcoef_ref(lt, stats, du, frozen=False):
    """{k1, k2, k3} with dx = k1 * du + k2 * x + k3, from the exact channel sums {sum du, sum du * x} in fp64 (the closed form of
    the GroupNorm backward; test_exact_norm_util.py asserts that it reproduces ATen's dx), and the rows' totals A, B."""
    x, gam = lt.x.double(), lt.gamma.double()[None]
    A, B = channel_sums(du), channel_sums(du.double() * x)
    if lt.batch:
        A, B = A.sum(0, keepdim=True).expand(lt.n, -1), B.sum(0, keepdim=True).expand(lt.n, -1)
    mean, rstd = stats[..., 0], stats[..., 1]
    mc, rc = per_channel(mean, lt.cg), per_channel(rstd, lt.cg)
    bh = rc * (B - mc * A)
    grp = lambda t: t.reshape(lt.n, lt.groups, lt.cg).sum(-1)
    s1, s2 = grp(gam * A), grp(gam * bh)
    count = float(lt.spatial * lt.cg * (lt.n if lt.batch else 1))
    k2 = -rstd * rstd * s2 / count
    k3 = (rstd * rstd * s2 * mean - rstd * s1) / count
    if frozen:
        k2, k3 = torch.zeros_like(k2), torch.zeros_like(k3)
    bc = torch.stack((rc * gam, per_channel(k2, lt.cg), per_channel(k3, lt.cg)), -1)
    return bc, (bh[0] if lt.batch else bh.sum(0)), (A[0] if lt.batch else A.sum(0))


def make_variant(name, lt, beta, act, dz, du, z=None, dz2=None, dres=False, in_act=NONE, frozen=False, null_z=False):
    """One backward call and its reference.  dz (+ dz2): the gradient handed to the kernel; du = (dz + dz2) * act': what the
    normalisation's backward sees; z: the activated tensor whose act' is taken (null_z: handed to ATen only, the kernel
    recomputes it from x and coef)."""
    dx, dgamma, dbeta = backward_ref(lt, beta, du, frozen)
    if in_act == RELU:
        dx = torch.ops.aten.threshold_backward(dx, lt.x.double(), 0.0)
    return types.SimpleNamespace(name=name, lt=lt, beta=beta, act=act, dz=dz, dz2=dz2, z=None if null_z else z, dres=dres, in_act=in_act,
                                 frozen=frozen, du=du, dx=dx, dgamma=dgamma, dbeta=dbeta)


def relu_pair(lt):
    """The ReLU forms: z = relu(y) with beta_act (no pre-activation is 0), du = dz masked."""
    y, _, coef = forward_ref(lt, lt.beta_act)
    u = coef[..., 0].reshape(lt.n, lt.c, 1, 1, 1) * lt.x.double() + coef[..., 1].reshape(lt.n, lt.c, 1, 1, 1)
    assert bool((y != 0).all()) and bool((u == y).all()), "relu: a pre-activation of 0, or ca * x + cb is not the reference's y"
    z = F.relu(y)
    return z, act_backward(lt.du.double(), z, RELU)


def gn_variants(case, eps):
    """Item i's calls for one case (shared by the storage types)."""
    def make():
        n, c, groups, shape = case
        lt, ln = lat(n, c, groups, shape, eps), lat(n, c, groups, shape, eps, nonneg=True)
        du, tag = lt.du.double(), f"exnv{case, eps}"
        out = [make_variant("none", lt, lt.beta, NONE, du, du)]
        z, dur = relu_pair(lt)
        out.append(make_variant("relu z", lt, lt.beta_act, RELU, du, dur, z=z, dres=True))
        out.append(make_variant("relu recomputed", lt, lt.beta_act, RELU, du, dur, z=z, null_z=True))
        ze = lattice(tag + "z", n, c, *shape, values=(-0.5, -0.75, 1, 2, 3), density=1.0).double()
        dze = du / torch.where(ze > 0, torch.ones_like(ze), ze + 1)
        due = act_backward(dze, ze, ELU)
        assert torch.equal(due, du)
        out.append(make_variant("elu z", lt, lt.beta, ELU, dze, due, z=ze, dres=True))
        d1 = lattice(tag + "d", n, c, *shape, density=0.7).double()
        out.append(make_variant("dz + dz2", lt, lt.beta, NONE, d1, du, dz2=du - d1, dres=True))
        assert bool((ln.x == 0).any()) and bool((ln.x > 0).any()) and bool((ln.x >= 0).all())
        out.append(make_variant("in_act relu", ln, ln.beta, NONE, ln.du.double(), ln.du.double(), in_act=RELU))
        return out
    return cached(("gnv", case, eps), make)


def check_variant(v, dt):
    """The exactness conditions of one backward call, on the reference alone."""
    lt, what = v.lt, f"{v.name} {dt}"
    for name, t in (("x", lt.x), ("dz", v.dz), ("dz2", v.dz2), ("z", v.z), ("dx", v.dx), ("dres", v.du)):
        if t is not None:
            assert_representable(t, dt, f"{what}: {name}")
    for name, t in (("dgamma", v.dgamma), ("dbeta", v.dbeta)):
        assert_representable(t, torch.float32, f"{what}: {name}")
    x, du = lt.x.double(), v.du.double()
    assert_sums_exact(channel_sums(x.abs()), what + ": sum |x|")
    assert_sums_exact(channel_sums(x * x), what + ": sum x^2")
    assert_sums_exact(channel_sums(du.abs()), what + ": sum |du|")
    assert_sums_exact(channel_sums((du * x).abs()), what + ": sum |du * x|", unit=0.5)   # (du * xhat: steps of 1/2 when eps = 3)


def check_forward(lt, beta, dt):
    y, stats, coef = forward_ref(lt, beta)
    assert_representable(y, dt, "y")
    assert_representable(stats, torch.float32, "stats")
    assert_representable(coef, torch.float32, "coef")
    assert torch.equal(stats[..., 0], lt.m) and torch.equal(stats[..., 1], 1.0 / torch.sqrt(lt.sigma ** 2 + lt.eps))
    return y, stats, coef


def split_rows(tag, totals, rows):
    """[n, rows, c] small integers whose sum over the rows is `totals` [n, c]."""
    g = O._rng("in:" + tag)
    n, c = totals.shape
    r = torch.from_numpy(g.integers(-4, 5, size=(n, rows, c)).astype(np.float64))
    r[:, -1] = totals - r[:, :-1].sum(1)
    return r


def foreign_rows(tag, lt, du, rows):
    """partial[n][rows][c][2] = {sum du, sum du * x} as a data-gradient epilogue would have written it, and the conditions."""
    A, B = channel_sums(du), channel_sums(du.double() * lt.x.double())
    part = torch.stack((split_rows(tag + "a", A, rows), split_rows(tag + "b", B, rows)), -1)
    assert_representable(part, torch.float32, "partial rows")
    assert_sums_exact(part.abs().sum(1), "sum of |partial rows|")
    return part.float()


# ------------------------------------------------------------------------------------------------ device side
def vol(t, dt):
    return None if t is None else t.to(DEV).to(dt).contiguous(memory_format=CL)


def nan_vol(lt, dt):
    return torch.full((lt.n, lt.c, *lt.shape), float("nan"), device=DEV).to(dt).contiguous(memory_format=CL)


def nan_f32(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


def f32(t):
    return t.to(torch.float32).contiguous().to(DEV)


def workspace(n, c, spatial):
    nbytes = L.lib().mednet_gn_ws_bytes(n, c, spatial)
    ws = nan_f32((nbytes + 3) // 4)
    return ws, ws.numel() * 4


def launched(rc, what, c, item):
    """A declined case is reported, never passed silently; only C = 1024 may be declined."""
    if rc == E_UNSUPPORTED:
        assert c == 1024, f"{what}: declined ({L.lib().mednet_last_error().decode()})"
        report(item, what, "DECLINED (MEDNET_E_UNSUPPORTED)", 0)
        pytest.skip(f"{what}: the library declines C = {c}")
    assert rc == 0, f"{what}: {rc} {L.lib().mednet_last_error().decode()}"
    torch.cuda.synchronize()


def run_stats(lt, beta, mode, item="h"):
    """mednet_gn_stats / mednet_bn_stats (no running buffers) and the apply pass with their coefficients: stats, coef, y equal."""
    dt, lib = DT[mode], L.lib()
    y_ref, stats_ref, coef_ref = check_forward(lt, beta, dt)
    assert_representable(lt.x, dt, "x")
    assert_sums_exact(channel_sums(lt.x.abs()), "sum |x|")
    assert_sums_exact(channel_sums(lt.x.double() ** 2), "sum x^2")
    # the statistics pass sums x - p, p the first channel of the unit at voxel 0 (of sample 0 for BatchNorm): exact as well
    p = (lt.x[:1] if lt.batch else lt.x)[:, ::lt.cg, :1, :1, :1].double().repeat_interleave(lt.cg, dim=1)
    assert_sums_exact(channel_sums((lt.x.double() - p).abs()), "sum |x - pivot|")
    assert_sums_exact(channel_sums((lt.x.double() - p) ** 2), "sum (x - pivot)^2")
    xg, gam, bet = vol(lt.x, dt), f32(lt.gamma), f32(beta)
    stats, coef, y = nan_f32(lt.n, lt.groups, 2), nan_f32(lt.n, lt.c, 2), nan_vol(lt, dt)
    ws, wsb = workspace(lt.n, lt.c, lt.spatial)
    if lt.batch:
        rc = lib.mednet_bn_stats(xg.data_ptr(), gam.data_ptr(), bet.data_ptr(), None, None, None, 0.1, stats.data_ptr(), coef.data_ptr(),
                                 lt.n, lt.spatial, lt.c, lt.eps, dcode_of(mode), ws.data_ptr(), wsb, L.stream())
    else:
        rc = lib.mednet_gn_stats(xg.data_ptr(), gam.data_ptr(), bet.data_ptr(), stats.data_ptr(), coef.data_ptr(), lt.n, lt.spatial, lt.c,
                                 lt.groups, lt.eps, dcode_of(mode), ws.data_ptr(), wsb, L.stream())
    launched(rc, f"stats {mode} C={lt.c}", lt.c, item)
    total = assert_exact(stats, stats_ref, f"stats {mode}") + assert_exact(coef, coef_ref, f"coef {mode}")
    rc = lib.mednet_gn_act_fwd(xg.data_ptr(), coef.data_ptr(), None, y.data_ptr(), lt.n, lt.spatial, lt.c, NONE, dcode_of(mode), dcode_of(mode), L.stream())
    launched(rc, "gn_act_fwd", lt.c, item)
    return stats, coef, total + assert_exact(y, y_ref, f"y {mode}")


def compare_backward(v, what, dx, dres, dgamma, dbeta):
    total = assert_exact(dx, v.dx, what + ": dx") + assert_exact(dgamma, v.dgamma, what + ": dgamma") + assert_exact(dbeta, v.dbeta, what + ": dbeta")
    if dres is not None:
        total += assert_exact(dres, v.du, what + ": dres")
    return total


def run_backward(v, mode, stats, coef, item="i"):
    """mednet_gn_act_bwd / mednet_bn_act_bwd with the statistics and coefficients the library computed itself."""
    lt, dt, lib = v.lt, DT[mode], L.lib()
    check_variant(v, dt)
    xg, dzg, dz2g, zg, gam = vol(lt.x, dt), vol(v.dz, dt), vol(v.dz2, dt), vol(v.z, dt), f32(lt.gamma)
    dx, dres = nan_vol(lt, dt), nan_vol(lt, dt) if v.dres else None
    dgamma, dbeta = nan_f32(lt.c), nan_f32(lt.c)
    ws, wsb = workspace(lt.n, lt.c, lt.spatial)
    if lt.batch:
        assert dz2g is None
        rc = lib.mednet_bn_act_bwd(dzg.data_ptr(), xg.data_ptr(), L.ptr(zg), coef.data_ptr(), stats.data_ptr(), gam.data_ptr(), dx.data_ptr(),
                                   L.ptr(dres), dgamma.data_ptr(), dbeta.data_ptr(), lt.n, lt.spatial, lt.c, v.act, v.in_act, int(v.frozen),
                                   dcode_of(mode), ws.data_ptr(), wsb, L.stream())
    else:
        rc = lib.mednet_gn_act_bwd(dzg.data_ptr(), L.ptr(dz2g), xg.data_ptr(), L.ptr(zg), coef.data_ptr(), stats.data_ptr(), gam.data_ptr(),
                                   dx.data_ptr(), L.ptr(dres), dgamma.data_ptr(), dbeta.data_ptr(), lt.n, lt.spatial, lt.c, lt.groups, v.act,
                                   v.in_act, dcode_of(mode), ws.data_ptr(), wsb, L.stream())
    what = f"act_bwd[{v.name}] {mode}"
    launched(rc, what, lt.c, item)
    return compare_backward(v, what, dx, dres, dgamma, dbeta)


def gn_statistics_and_backward(case, eps, mode, opts=()):
    n, c, groups, shape = case
    lt, ln = lat(n, c, groups, shape, eps), lat(n, c, groups, shape, eps, nonneg=True)
    fwd, th, ti = {}, 0, 0
    with options(*opts):
        for l, beta in ((lt, lt.beta), (lt, lt.beta_act), (ln, ln.beta)):
            st, cf, k = run_stats(l, beta, mode)
            fwd[id(l), id(beta)] = (st, cf)
            th += k
        for v in gn_variants(case, eps):
            ti += run_backward(v, mode, *fwd[id(v.lt), id(v.beta)])
    p = path_of(case, mode, opts)
    kernel = f"vec {p['vec']} rpw {p['rpw']} chunks {p['chunks']} one_launch {int(p['one_launch'])} opts {list(opts)}"
    report("h", f"gn_stats {case} eps={eps} {mode}", kernel, th)
    report("i", f"gn_act_bwd {case} eps={eps} {mode}", kernel, ti)


# ------------------------------------------------------------------------------------------------ items h, i
@pytest.mark.parametrize("case,eps,mode", gn_params())
def test_groupnorm_statistics_and_backward(case, eps, mode):
    """Items h and i: mednet_gn_stats, then mednet_gn_act_bwd with ITS stats / coef: activation none, ReLU from z, ReLU
    recomputed, ELU from a dyadic z, dz + dz2, dres, in_act = ReLU."""
    assert_case_list_reaches_every_path()
    gn_statistics_and_backward(case, eps, mode)


@pytest.mark.parametrize("opt,mode", OPTION_RUNS)
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("case", OPTION_CASES, ids=case_id)
def test_groupnorm_other_kernel_forms(case, eps, opt, mode):
    """... again with column_reduce through LDS, with the reduce / finalize / params launches, and fp32 with 8-wide vectors."""
    gn_statistics_and_backward(case, eps, mode, (opt,))


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("c,groups", [(16, 8), (8, 8)])
@pytest.mark.parametrize("chunks", [5, 4096 + 3])
def test_groupnorm_finalize_alone(chunks, c, groups, eps):
    """mednet_gn_finalize on rows the test writes: 256 threads, and 1024 at chunks >= 4096; cg % 2 == 0 and the scalar branch."""
    n, spatial, cg = 2, 1000, c // groups
    g = O._rng(f"in:exnf{chunks, c, eps}")
    sigma = torch.from_numpy(g.choice(np.asarray([1.0, 2.0, 4.0]), size=(n, groups)) if eps == 0 else np.ones((n, groups)))
    m = torch.from_numpy(g.integers(-3, 4, size=(n, groups)).astype(np.float64))
    gamma = lattice(f"exnf{chunks, c}g", c, values=(0.5, 1, 2), density=1.0)
    beta = lattice(f"exnf{chunks, c}b", c, values=(-3, -1, 1, 2), density=1.0)
    tot = torch.stack((per_channel(m, cg) * spatial, per_channel(m * m + sigma * sigma, cg) * spatial), -1)     # [n, c, 2]
    part = torch.stack((split_rows(f"f{chunks, c}a", tot[..., 0], chunks), split_rows(f"f{chunks, c}b", tot[..., 1], chunks)), -1)
    assert_representable(part, torch.float32, "rows")
    assert_sums_exact(part.abs().sum(1), "sum of |rows|")
    rstd = 1.0 / torch.sqrt(sigma * sigma + eps)
    a = gamma.double()[None] * per_channel(rstd, cg)
    stats_ref, coef_ref = torch.stack((m, rstd), -1), torch.stack((a, beta.double()[None] - per_channel(m, cg) * a), -1)
    assert_representable(stats_ref, torch.float32, "stats")
    assert_representable(coef_ref, torch.float32, "coef")
    stats, coef, ws = nan_f32(n, groups, 2), nan_f32(n, c, 2), nan_f32(n * c * 2)
    pg, gam, bet = f32(part), f32(gamma), f32(beta)
    rc = L.lib().mednet_gn_finalize(pg.data_ptr(), chunks, gam.data_ptr(), bet.data_ptr(), stats.data_ptr(), coef.data_ptr(), n, spatial, c,
                                    groups, eps, ws.data_ptr(), ws.numel() * 4, L.stream())
    launched(rc, "gn_finalize", c, "h")
    total = assert_exact(stats, stats_ref, "gn_finalize stats") + assert_exact(coef, coef_ref, "gn_finalize coef")
    report("h", f"gn_finalize chunks={chunks} C={c} groups={groups} eps={eps}", f"{1024 if chunks >= 4096 else 256} threads, cg {cg}", total)


# ------------------------------------------------------------------------------------------------ item j
def big_rows(cg):
    return 16 * 256 // cg + 37     # the 16-deep loop of the one-launch form runs, then its remainder, over all 256 / cg row classes


@pytest.mark.parametrize("case,eps,mode", gn_params())
def test_groupnorm_backward_from_foreign_rows(case, eps, mode):
    """Item j: mednet_gn_bwd_coefficients, mednet_gn_act_bwd_fused (activation none and ReLU recomputed, in_act ReLU) and
    mednet_gn_act_bwd_fused_res (ReLU / ELU from z, dres) on rows {sum du, sum du * x} that the test writes."""
    n, c, groups, shape = case
    dt, dc, lib = DT[mode], dcode_of(mode), L.lib()
    total, cg = 0, c // groups
    for v in gn_variants(case, eps):
        if v.dz2 is not None:
            continue
        lt = v.lt
        check_variant(v, dt)
        _, stats_ref, coef_ref = check_forward(lt, v.beta, dt)
        bc_ref, dgamma_ref, dbeta_ref = bcoef_ref(lt, stats_ref, v.du)
        assert_representable(bc_ref, torch.float32, "bcoef")
        assert torch.equal(dgamma_ref, v.dgamma) and torch.equal(dbeta_ref, v.dbeta)
        xg, dzg, gam, stats, coef = vol(lt.x, dt), vol(v.dz, dt), f32(lt.gamma), f32(stats_ref), f32(coef_ref)
        for rows in (1, 5, big_rows(cg)):
            part = foreign_rows(f"exnj{case, eps, v.name, rows}", lt, v.du, rows).to(DEV)
            what = f"[{v.name}] rows={rows} {mode}"
            if v.name == "none":
                bcoef, dgamma, dbeta = nan_f32(n, c, 3), nan_f32(c), nan_f32(c)
                ws, wsb = workspace(n, c, lt.spatial)
                rc = lib.mednet_gn_bwd_coefficients(stats.data_ptr(), gam.data_ptr(), part.data_ptr(), rows, bcoef.data_ptr(), dgamma.data_ptr(),
                                                    dbeta.data_ptr(), n, lt.spatial, c, groups, ws.data_ptr(), wsb, L.stream())
                launched(rc, "gn_bwd_coefficients " + what, c, "j")
                total += (assert_exact(bcoef, bc_ref, "bcoef " + what) + assert_exact(dgamma, v.dgamma, "coefficients dgamma " + what)
                          + assert_exact(dbeta, v.dbeta, "coefficients dbeta " + what))
            dx, dgamma, dbeta = nan_vol(lt, dt), nan_f32(c), nan_f32(c)
            ws, wsb = workspace(n, c, lt.spatial)
            if v.z is None:    # none, ReLU recomputed, in_act
                dres = None
                rc = lib.mednet_gn_act_bwd_fused(dzg.data_ptr(), xg.data_ptr(), coef.data_ptr(), stats.data_ptr(), gam.data_ptr(), part.data_ptr(),
                                                 rows, dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), n, lt.spatial, c, groups, v.act, v.in_act,
                                                 dc, ws.data_ptr(), wsb, L.stream())
            else:
                dres, zg = nan_vol(lt, dt), vol(v.z, dt)
                rc = lib.mednet_gn_act_bwd_fused_res(dzg.data_ptr(), xg.data_ptr(), zg.data_ptr(), coef.data_ptr(), stats.data_ptr(), gam.data_ptr(),
                                                     part.data_ptr(), rows, dx.data_ptr(), dres.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), n,
                                                     lt.spatial, c, groups, v.act, dc, ws.data_ptr(), wsb, L.stream())
            launched(rc, "gn_act_bwd_fused " + what, c, "j")
            total += compare_backward(v, "fused " + what, dx, dres, dgamma, dbeta)
    report("j", f"gn_act_bwd_fused / _res / coefficients {case} eps={eps} {mode}", f"one_launch {int(256 % cg == 0)} rows 1, 5, {big_rows(cg)}", total)


def pool_inputs(case, eps, pool):
    """The encoder form: du = (pooling backward of dy_pool + skip gradient) * relu'(z) IS the constructed du.  z has a unique
    maximum per window and is negative only where du is 0 (and the joined gradient never is there); dy_pool sits at the arg-max voxels
    (max) or is spread in eighths (avg); the skip gradient carries the rest."""
    def make():
        n, c, groups, (d, h, w) = case
        lt = lat(n, c, groups, (d, h, w), eps)
        du, tag = lt.du.double(), f"exnp{case, eps, pool}"
        g = O._rng("in:" + tag)
        perm = torch.from_numpy(g.random((n, c, d // 2, h // 2, w // 2, 8)).argsort(-1).astype(np.float64) + 1.0)
        z = perm.reshape(n, c, d // 2, h // 2, w // 2, 2, 2, 2).permute(0, 1, 2, 5, 3, 6, 4, 7).reshape(n, c, d, h, w).contiguous()
        neg = (du == 0) & (z != 8)
        z = torch.where(neg, -z, z)
        dyp = lattice(tag + "g", n, c, d // 2, h // 2, w // 2, values=(-2, -1, 1, 2), density=1.0).double() * (8 if pool == "avg" else 1)
        zr = z.clone().requires_grad_(True)
        (F.max_pool3d if pool == "max" else F.avg_pool3d)(zr, 2).backward(dyp)
        free = lattice(tag + "s", n, c, d, h, w, values=(-2, -1, 1, 2), density=1.0).double()
        free = torch.where(free + zr.grad == 0, zr.grad, free)      # (avg: the pooling share is +-1, +-2 too and could cancel)
        skip = torch.where(neg, free, du - zr.grad)
        joined = zr.grad + skip
        due = act_backward(joined, z, RELU)
        assert torch.equal(due, du) and bool((F.max_pool3d(z, 2) == 8).all())
        assert bool((joined[neg] != 0).all()), "a masked voxel with a joined gradient of 0: relu' would not show there"
        v = make_variant(f"pool {pool}", lt, lt.beta, RELU, joined, due, z=z, dres=True)
        return v, dyp, skip
    return cached(("pool", case, eps, pool), make)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pool", ["max", "avg"])
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("case", POOL_CASES, ids=case_id)
def test_groupnorm_backward_rebuilding_the_pooling_join(case, eps, pool, mode):
    """Item j: mednet_gn_act_bwd_fused_res_pool."""
    n, c, groups, (d, h, w) = case
    dt, lib = DT[mode], L.lib()
    v, dyp, skip = pool_inputs(case, eps, pool)
    lt = v.lt
    check_variant(v, dt)
    for name, t in (("dy_pool", dyp), ("skip", skip)):
        assert_representable(t, dt, name)
    _, stats_ref, _ = check_forward(lt, v.beta, dt)
    total = 0
    for rows in (1, 5, big_rows(c // groups)):
        part = foreign_rows(f"exnjp{case, eps, pool, rows}", lt, v.du, rows).to(DEV)
        dx, dres, dgamma, dbeta = nan_vol(lt, dt), nan_vol(lt, dt), nan_f32(c), nan_f32(c)
        ws, wsb = workspace(n, c, lt.spatial)
        dypg, skg, xg, zg, stats, gam = vol(dyp, dt), vol(skip, dt), vol(lt.x, dt), vol(v.z, dt), f32(stats_ref), f32(lt.gamma)
        rc = lib.mednet_gn_act_bwd_fused_res_pool(dypg.data_ptr(), skg.data_ptr(), xg.data_ptr(), zg.data_ptr(), stats.data_ptr(), gam.data_ptr(),
                                                  part.data_ptr(), rows, dx.data_ptr(), dres.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), n, d, h, w,
                                                  c, groups, RELU, L.POOL_MAX if pool == "max" else L.POOL_AVG, dcode_of(mode), ws.data_ptr(), wsb,
                                                  L.stream())
        launched(rc, "gn_act_bwd_fused_res_pool", c, "j")
        total += compare_backward(v, f"fused_res_pool {pool} rows={rows} {mode}", dx, dres, dgamma, dbeta)
    report("j", f"gn_act_bwd_fused_res_pool {case} eps={eps} {pool} {mode}", "gn_bwd_apply_pool", total)


# ------------------------------------------------------------------------------------------------ item k
def ulp32(ref):
    r = ref.double().abs().float()
    return (torch.nextafter(r, torch.full_like(r, float("inf"))) - r).double()


def assert_within_one_ulp(got, ref, what):
    got, ref = got.detach().double().cpu(), ref.double()
    err = (got - ref).abs() / ulp32(ref)
    print(f"{what}: max error {float(err.max()):.3f} fp32 ulp")
    assert bool((err <= 1.0).all()), f"{what}: {float(err.max()):.3f} ulp > 1"
    return got.numel()


def bn_variants(case, eps):
    def make():
        n, c, shape = case
        lt = lat(n, c, c, shape, eps, batch=True)
        du = lt.du.double()
        z, dur = relu_pair(lt)
        return [make_variant("none", lt, lt.beta, NONE, du, du), make_variant("frozen", lt, lt.beta, NONE, du, du, frozen=True),
                make_variant("relu z", lt, lt.beta_act, RELU, du, dur, z=z, dres=True),
                make_variant("relu recomputed", lt, lt.beta_act, RELU, du, dur, z=z, null_z=True)]
    return cached(("bnv", case, eps), make)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("case", BN_CASES, ids=case_id)
def test_batchnorm(case, eps, mode):
    """Item k: mednet_bn_stats without and with running buffers, mednet_bn_act_bwd (frozen 0 / 1), mednet_bn_act_bwd_fused."""
    n, c, shape = case
    dt, dc, lib = DT[mode], dcode_of(mode), L.lib()
    lt = lat(n, c, c, shape, eps, batch=True)
    fwd, total = {}, 0
    for beta in (lt.beta, lt.beta_act):
        st, cf, k = run_stats(lt, beta, mode, item="k")
        fwd[id(beta)] = (st, cf)
        total += k
    # running statistics: the reference gets the fp32 value of the momentum argument
    _, stats_ref, coef_ref = check_forward(lt, lt.beta, dt)
    xg, gam, bet = vol(lt.x, dt), f32(lt.gamma), f32(lt.beta)
    rm0 = lattice(f"exnk{case}m", c, values=(-2, -1, 1, 2), density=0.8).double()
    rv0 = lattice(f"exnk{case}v", c, values=(1, 2, 4), density=1.0).double()
    for momentum in (0.5, 0.125, 0.1):
        rm_ref, rv_ref = rm0.clone(), rv0.clone()
        torch.ops.aten.native_batch_norm(lt.x.double(), lt.gamma.double(), lt.beta.double(), rm_ref, rv_ref, True, float(np.float32(momentum)), eps)
        rm, rv, nbt = f32(rm0), f32(rv0), torch.tensor([7], dtype=torch.int64, device=DEV)
        stats, coef = nan_f32(n, c, 2), nan_f32(n, c, 2)
        ws, wsb = workspace(n, c, lt.spatial)
        rc = lib.mednet_bn_stats(xg.data_ptr(), gam.data_ptr(), bet.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), momentum,
                                 stats.data_ptr(), coef.data_ptr(), n, lt.spatial, c, eps, dc, ws.data_ptr(), wsb, L.stream())
        launched(rc, "bn_stats", c, "k")
        assert int(nbt.item()) == 8
        total += assert_exact(stats, stats_ref, f"bn_stats stats {mode}") + assert_exact(coef, coef_ref, f"bn_stats coef {mode}")
        if momentum == 0.1:
            total += assert_within_one_ulp(rm, rm_ref, f"running_mean momentum 0.1 {mode}")
        else:
            assert_representable(rm_ref, torch.float32, "running_mean")
            total += assert_exact(rm, rm_ref, f"running_mean momentum {momentum} {mode}")
        total += assert_within_one_ulp(rv, rv_ref, f"running_var momentum {momentum} {mode}")
        if momentum == 0.5:     # a second call: the counter again + 1, the mean blended again (still dyadic)
            torch.ops.aten.native_batch_norm(lt.x.double(), lt.gamma.double(), lt.beta.double(), rm_ref, rv_ref, True, momentum, eps)
            rc = lib.mednet_bn_stats(xg.data_ptr(), gam.data_ptr(), bet.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), momentum,
                                     stats.data_ptr(), coef.data_ptr(), n, lt.spatial, c, eps, dc, ws.data_ptr(), wsb, L.stream())
            launched(rc, "bn_stats", c, "k")
            assert int(nbt.item()) == 9
            assert_representable(rm_ref, torch.float32, "running_mean")
            total += assert_exact(rm, rm_ref, f"running_mean after two calls {mode}")
    # backward
    off = n * partial_rows_max(c) * c * 2      # bcoef[n][c][3] sits behind the partial region of the workspace
    cw = 4 if c % 4 == 0 else 1
    for v in bn_variants(case, eps):
        total += run_backward(v, mode, *fwd[id(v.beta)], item="k")
        if v.z is not None:
            continue
        check_variant(v, dt)
        _, st_ref, cf_ref = check_forward(lt, v.beta, dt)
        bc_ref, dgamma_ref, dbeta_ref = bcoef_ref(lt, st_ref, v.du, v.frozen)
        assert_representable(bc_ref, torch.float32, "bcoef")
        assert torch.equal(dgamma_ref, v.dgamma) and torch.equal(dbeta_ref, v.dbeta)
        dzg, stats, coef = vol(v.dz, dt), f32(st_ref), f32(cf_ref)
        A, B = channel_sums(v.du).sum(0, keepdim=True), channel_sums(v.du.double() * lt.x.double()).sum(0, keepdim=True)
        for rows in (1, 5, 8 * 1024 // cw // n + 37):     # bn_column_sums: 8 rows in flight over 1024 / cw row classes, then the remainder
            tag = f"exnkr{case, eps, v.name, rows}"
            part = torch.stack((split_rows(tag + "a", A, n * rows), split_rows(tag + "b", B, n * rows)), -1)     # [1][n * rows][c][2]
            assert_representable(part, torch.float32, "rows")
            assert_sums_exact(part.abs().sum(1), "sum of |rows|")
            pg, dx, dgamma, dbeta = f32(part), nan_vol(lt, dt), nan_f32(c), nan_f32(c)
            ws, wsb = workspace(n, c, lt.spatial)
            rc = lib.mednet_bn_act_bwd_fused(dzg.data_ptr(), xg.data_ptr(), coef.data_ptr(), stats.data_ptr(), gam.data_ptr(), pg.data_ptr(), rows,
                                             dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), n, lt.spatial, c, v.act, v.in_act, int(v.frozen), dc,
                                             ws.data_ptr(), wsb, L.stream())
            what = f"bn_act_bwd_fused[{v.name}] rows={rows} {mode}"
            launched(rc, what, c, "k")
            total += compare_backward(v, what, dx, None, dgamma, dbeta)
            total += assert_exact(ws[off:off + n * c * 3].reshape(n, c, 3), bc_ref, what + ": bcoef rows")
    report("k", f"batchnorm {case} eps={eps} {mode}", f"vec {pick_vec(c, mode)} cw {cw}", total)


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("n,c", [(2, 6), (3, 200)])
def test_batchnorm_eval_coefficients(n, c, eps):
    """mednet_bn_eval_coef with running_var + eps in {1, 4, 16}: stats and coef equal in all n rows."""
    rm = lattice(f"exne{n, c}m", c, values=(-3, -2, -1, 1, 2, 3), density=0.9)
    rv = lattice(f"exne{n, c}v", c, values=(1, 4, 16) if eps == 0 else (1, 13), density=1.0)
    gamma = lattice(f"exne{n, c}g", c, values=(0.5, 1, 2), density=1.0)
    beta = lattice(f"exne{n, c}b", c, values=(-3, -1, 1, 2), density=0.8)
    assert set((rv.double() + eps).tolist()) <= {1.0, 4.0, 16.0}
    x = lattice(f"exne{n, c}x", n, c, 2, 2, 2, density=0.8).double()
    rstd = 1.0 / torch.sqrt(rv.double() + eps)      # (1, 1/2, 1/4: exact)
    a = gamma.double() * rstd
    stats_ref = torch.stack((rm.double(), rstd), -1)[None].expand(n, -1, -1)
    coef_ref = torch.stack((a, beta.double() - rm.double() * a), -1)[None].expand(n, -1, -1)
    # ... and the coefficients reproduce ATen's evaluation-mode output
    y = torch.batch_norm(x, gamma.double(), beta.double(), rm.double(), rv.double(), False, 0.0, eps, False)
    assert torch.equal(snap(y), coef_ref[0, :, 0].reshape(1, c, 1, 1, 1) * x + coef_ref[0, :, 1].reshape(1, c, 1, 1, 1))
    assert_representable(stats_ref, torch.float32, "stats")
    assert_representable(coef_ref, torch.float32, "coef")
    stats, coef = nan_f32(n, c, 2), nan_f32(n, c, 2)
    rmg, rvg, gam, bet = f32(rm), f32(rv), f32(gamma), f32(beta)     # (named: a temporary's memory is reused by the next one)
    rc = L.lib().mednet_bn_eval_coef(rmg.data_ptr(), rvg.data_ptr(), gam.data_ptr(), bet.data_ptr(), stats.data_ptr(),
                                     coef.data_ptr(), n, c, eps, L.stream())
    launched(rc, "bn_eval_coef", c, "k")
    report("k", f"bn_eval_coef n={n} C={c} eps={eps}", "bn_eval_coef", assert_exact(stats, stats_ref, "eval stats") + assert_exact(coef, coef_ref, "eval coef"))


# ------------------------------------------------------------------------------------------------ item l
def act_inputs(count):
    """x: non-zero small integers; z: dyadic negatives and positive integers; dz: small integers; u: ELU's negative side -- and
    ATen's fp64 results, computed once for the three storage types and kept in fp32 (asserted to hold them exactly; only
    ELU's negative side, which carries the 1-ulp limit, stays in fp64)."""
    def make():
        g = O._rng(f"in:exnl{count}")
        pick = lambda vals: torch.from_numpy(g.choice(np.asarray(vals, dtype=np.float32), size=count))
        t = types.SimpleNamespace(x=pick([-3, -2, -1, 1, 2, 3]), z=pick([-0.5, -0.75, 1, 2, 3]), dz=pick([-2, -1, 1, 2, 4]),
                                  u=pick([-8, -4, -2, -1, -0.5, -0.25, 1, 2]))

        def keep(ref):
            assert torch.equal(ref.float().double(), ref)
            return ref.float()

        x64, dz64 = t.x.double(), t.dz.double()
        t.relu, t.elu_pos = keep(F.relu(x64)), keep(F.elu(x64.abs()))
        t.bwd_relu, t.bwd_elu = keep(act_backward(dz64, F.relu(x64), RELU)), keep(act_backward(dz64, t.z.double(), ELU))
        t.neg = t.u < 0
        t.elu_neg, t.elu_rest = F.elu(t.u[t.neg].double()), keep(F.elu(t.u[~t.neg].double()))
        return t
    return cached(("act", count), make)


def equal_flat(got, ref, dt, what):
    """assert_exact for flat tensors; compared on the device first (the largest count is 16.8 M elements)."""
    assert_representable(ref, dt, what)
    if bool((got == ref.to(DEV).to(dt)).all()):
        return got.numel()
    return assert_exact(got, ref, what)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("count", ACT_COUNTS)
def test_standalone_activation(count, mode):
    """Item l: mednet_act_fwd / mednet_act_bwd; the vector body, the scalar tail and the second trip of the grid-stride loop."""
    dt, dc, lib = DT[mode], dcode_of(mode), L.lib()
    assert (min(-(-count // 2048), 8192) * 2048 < count) == (count == ACT_COUNTS[-1])     # flat_grid: only the largest count strides
    t = act_inputs(count)
    total = 0

    def fwd(x, act):
        xg, out = x.to(DEV).to(dt), torch.full((count,), float("nan"), device=DEV).to(dt)
        rc = lib.mednet_act_fwd(xg.data_ptr(), out.data_ptr(), count, act, dc, L.stream())
        launched(rc, "act_fwd", 0, "l")
        return out

    def bwd(dz, z, act):
        dg, zg, out = dz.to(DEV).to(dt), z.to(DEV).to(dt), torch.full((count,), float("nan"), device=DEV).to(dt)
        rc = lib.mednet_act_bwd(dg.data_ptr(), zg.data_ptr(), out.data_ptr(), count, act, dc, L.stream())
        launched(rc, "act_bwd", 0, "l")
        return out

    total += equal_flat(fwd(t.x, NONE), t.x, dt, f"act_fwd none {mode}")
    total += equal_flat(fwd(t.x, RELU), t.relu, dt, f"act_fwd relu {mode}")
    total += equal_flat(fwd(t.x.abs(), ELU), t.elu_pos, dt, f"act_fwd elu, positive side {mode}")
    total += equal_flat(bwd(t.dz, t.x, NONE), t.dz, dt, f"act_bwd none {mode}")
    total += equal_flat(bwd(t.dz, t.relu, RELU), t.bwd_relu, dt, f"act_bwd relu {mode}")
    total += equal_flat(bwd(t.dz, t.z, ELU), t.bwd_elu, dt, f"act_bwd elu {mode}")
    if mode != "fp32":    # ELU's negative side: 1 ulp of the storage type at the reference (see the module docstring)
        got, ref = fwd(t.u, ELU).cpu(), t.elu_neg
        assert torch.equal(got[~t.neg].float(), t.elu_rest)
        mant = 7 if mode == "bf16" else 10
        ulp = torch.exp2(torch.floor(torch.log2(ref.abs())) - mant)
        err = (got[t.neg].double() - ref).abs() / ulp
        print(f"act_fwd elu, negative side {mode} count={count}: max error {float(err.max()):.3f} ulp")
        assert bool((err <= 1.0).all()), f"act_fwd elu, negative side {mode}: {float(err.max()):.3f} ulp > 1"
        total += count
    report("l", f"act_fwd / act_bwd count={count} {mode}", "act_fwd, act_bwd", total)
    if mode == MODES[-1]:
        _CACHE.pop(("act", count), None)    # (the largest count holds 0.6 GB of inputs and references)
