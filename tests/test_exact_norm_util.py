"""CPU side of tests/test_gpu_exact_norm.py, no GPU and no library: (1) the exactness conditions -- the snap distance of ATen's
fp64 result, every output element a number of bf16, fp16 (tensors) or fp32 (statistics, coefficients, parameter gradients), every
sum of |terms| below 2^24 -- hold for every case of the GPU module; (2) discrimination: a model of the kernels' arithmetic in
fp64 (partial rows -> statistics -> coefficients -> k1 * du + k2 * x + k3) reproduces ATen's result on these inputs, and with ONE
fault at a time it differs from it in at least one element of the output the fault belongs to.  Equality on these inputs
therefore fails for each of those faults."""
import pytest
import torch

import test_gpu_exact_norm as N
from gpu_util import norm_lattice, snap

DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def test_norm_lattice_is_seeded_and_balanced():
    a, b = norm_lattice("t", 2, 24, 8, (4, 6, 5), 0.0), norm_lattice("t", 2, 24, 8, (4, 6, 5), 0.0)
    assert torch.equal(a.x, b.x) and torch.equal(a.du, b.du) and torch.equal(a.gamma, b.gamma)
    x = a.x.double().reshape(2, 8, -1)
    assert torch.equal(x.mean(-1), a.m) and torch.equal(((x - a.m[..., None]) ** 2).mean(-1), a.sigma ** 2)
    assert set(a.sigma.unique().tolist()) <= {1.0, 2.0, 4.0} and set(norm_lattice("t", 2, 24, 8, (4, 6, 5), 3.0).sigma.unique().tolist()) == {1.0}
    with pytest.raises(ValueError, match="odd"):
        norm_lattice("t", 2, 24, 8, (3, 5, 7), 0.0)            # odd size, cg = 3
    with pytest.raises(ValueError):
        norm_lattice("t", 1, 8, 8, (3, 5, 7), 0.0, batch=True)  # BatchNorm: n * S odd
    odd = norm_lattice("t", 1, 32, 8, (3, 5, 9), 0.0)           # odd size: channel pairs carry opposite signs and one gamma
    s = (odd.x.double().reshape(1, 8, 4, -1) - odd.m[..., None, None]) / odd.sigma[..., None, None]
    assert torch.equal(s[:, :, 0::2], -s[:, :, 1::2]) and torch.equal(odd.gamma[0::2], odd.gamma[1::2])
    bn = norm_lattice("t", 2, 8, 8, (3, 5, 7), 0.0, batch=True)  # BatchNorm: balanced over the samples of a channel
    assert torch.equal(bn.x.double().transpose(0, 1).reshape(8, -1).mean(-1), bn.m[0]) and torch.equal(bn.m[0], bn.m[1])
    nn = norm_lattice("t", 2, 8, 8, (6, 7, 9), 0.0, nonneg=True)
    assert bool((nn.x >= 0).all()) and bool((nn.x == 0).any())


def test_snap_keeps_the_grid_and_refuses_a_real_difference():
    t = torch.tensor([0.5, -1.75, 3.0], dtype=torch.float64)
    assert torch.equal(snap(t + 2e-13), t)
    with pytest.raises(AssertionError, match="moved"):
        snap(t + 1e-6)


def test_the_case_list_reaches_every_path_of_the_launchers():
    N.assert_case_list_reaches_every_path()
    assert N.path_of(N.GN_CASES[1], "bf16")["chunks"] == 3 and N.path_of(N.GN_CASES[1], "bf16")["short_tail"]
    assert N.path_of(N.GN_CASES[2], "bf16") == dict(vec=8, rpw=4, idle=False, chunks=3, short_tail=True, one_launch=True)
    assert N.path_of(N.GN_CASES[3], "bf16")["idle"] and not N.path_of(N.GN_CASES[3], "bf16")["one_launch"]
    assert N.path_of(N.GN_CASES[9], "bf16")["rpw"] == 2
    assert N.big_rows(1) > 16 * 256 and N.big_rows(32) > 16 * 8


# ------------------------------------------------------------------------------------------------ conditions
@pytest.mark.parametrize("eps", N.EPS)
@pytest.mark.parametrize("case", N.GN_CASES, ids=N.case_id)
def test_conditions_of_the_groupnorm_cases(case, eps):
    for v in N.gn_variants(case, eps):
        for dt in DTYPES:
            N.check_variant(v, dt)
            _, stats, _ = N.check_forward(v.lt, v.beta, dt)
        if v.dz2 is None:    # the closed form the kernels apply reproduces ATen's dx and parameter gradients, with fp32 coefficients
            bc, dgamma, dbeta = N.bcoef_ref(v.lt, stats, v.du)
            N.assert_representable(bc, torch.float32, "bcoef")
            r = lambda k: bc[..., k].reshape(v.lt.n, v.lt.c, 1, 1, 1)
            dx = r(0) * v.du + r(1) * v.lt.x.double() + r(2)
            if v.in_act == N.RELU:
                dx = dx * (v.lt.x > 0)
            assert torch.equal(dx, v.dx) and torch.equal(dgamma, v.dgamma) and torch.equal(dbeta, v.dbeta)
            for rows in (1, 5, N.big_rows(v.lt.cg)):
                N.foreign_rows(f"t{rows}", v.lt, v.du, rows)
        if v.name == "none":
            nz = float((v.dx != 0).double().mean())
            print(f"{case} eps={eps}: dx is non-zero in {100 * nz:.1f} % of the elements")
            assert nz >= 0.9, "dx is zero in more than a tenth of the elements: a dropped term could hide"
        if v.name == "relu z":   # the mask is neither empty nor full
            assert 0.05 < float((v.z > 0).double().mean()) < 0.95


@pytest.mark.parametrize("pool", ["max", "avg"])
@pytest.mark.parametrize("eps", N.EPS)
@pytest.mark.parametrize("case", N.POOL_CASES, ids=N.case_id)
def test_conditions_of_the_pooling_join_cases(case, eps, pool):
    v, dyp, skip = N.pool_inputs(case, eps, pool)
    for dt in DTYPES:
        N.check_variant(v, dt)
        N.check_forward(v.lt, v.beta, dt)
        N.assert_representable(dyp, dt, "dy_pool")
        N.assert_representable(skip, dt, "skip")
    assert bool((v.z < 0).any()), "no masked voxel: relu' is not exercised"


@pytest.mark.parametrize("eps", N.EPS)
@pytest.mark.parametrize("case", N.BN_CASES, ids=N.case_id)
def test_conditions_of_the_batchnorm_cases(case, eps):
    for v in N.bn_variants(case, eps):
        for dt in DTYPES:
            N.check_variant(v, dt)
            _, stats, _ = N.check_forward(v.lt, v.beta, dt)
        bc, dgamma, dbeta = N.bcoef_ref(v.lt, stats, v.du, v.frozen)
        N.assert_representable(bc, torch.float32, "bcoef")
        r = lambda k: bc[..., k].reshape(v.lt.n, v.lt.c, 1, 1, 1)
        assert torch.equal(r(0) * v.du + r(1) * v.lt.x.double() + r(2), v.dx) and torch.equal(dgamma, v.dgamma) and torch.equal(dbeta, v.dbeta)
        assert torch.equal(bc[0], bc[-1])


# ------------------------------------------------------------------------------------------------ discrimination
FAULTS = ["neighbour group", "k2 dropped", "k3 dropped", "tail voxel", "row twice", "dres before act'", "coef row"]


def model(lt, beta, dz, relu, fault=None, mask=None):
    """The kernels' arithmetic in fp64: sums over the voxels (weights w: 1, 0 for a dropped voxel, 2 for a chunk counted twice) ->
    statistics and coefficients; the backward, with the true statistics (the forward is checked on its own): du = dz * relu'(ca *
    x + cb) (or dz * mask, where the activated tensor is handed in), the sums {sum du, sum du * xhat}, {k1, k2, k3}, dx, dres,
    the parameter gradients.  BatchNorm (lt.batch): the sums run over the samples too.
    The faults are models, one place each: "neighbour group" puts the next group's mean / rstd into the xhat of the sum
    du * xhat only (it shows in dgamma, and through k2 / k3 in dx), not into the apply coefficients; "coef row" swaps the forward
    coefficient row (it shows in y, and in a recomputed mask)."""
    n, c, G, cg, S = lt.n, lt.c, lt.groups, lt.cg, lt.spatial
    x, dz, gam, b = lt.x.double().flatten(2), dz.double().flatten(2), lt.gamma.double()[None], beta.double()[None]
    pc = lambda t: N.per_channel(t, cg)
    tot = (lambda t: t.sum(0, keepdim=True).expand(n, -1)) if lt.batch else (lambda t: t)
    grp = lambda t: tot(t).reshape(n, G, cg).sum(-1)
    w = torch.ones(n, 1, S, dtype=torch.float64)
    if fault == "tail voxel":
        w[n - 1, 0, S - 1] = 0.0
    if fault == "row twice":
        w[0, 0, :N.chunk_plan(S, c, N.pick_vec(c, "bf16"))[0]] = 2.0
    count = float(S * cg * (n if lt.batch else 1))
    mean = grp((x * w).sum(-1)) / count
    rstd = 1.0 / torch.sqrt(grp((x * x * w).sum(-1)) / count - mean * mean + lt.eps)
    a = gam * pc(rstd)
    out = dict(stats=torch.stack((mean, rstd), -1), coef=torch.stack((a, b - pc(mean) * a), -1))
    mean, rstd = lt.m, 1.0 / torch.sqrt(lt.sigma ** 2 + lt.eps)
    mc, rc = pc(mean).clone(), pc(rstd).clone()
    ua = gam * rc
    ub = b - mc * ua
    if fault == "neighbour group":     # the first channel of a group takes the next group's statistics
        for g in range(G):
            mc[:, g * cg], rc[:, g * cg] = mean[:, (g + 1) % G], rstd[:, (g + 1) % G]
    if fault == "coef row":            # the first sample is applied, and its mask recomputed, with the second sample's row
        ua, ub = ua.clone(), ub.clone()
        ua[0], ub[0] = ua[1], ub[1]
    out["y"] = (ua[..., None] * x + ub[..., None]).reshape(n, c, *lt.shape)
    if mask is not None:
        du = dz * mask.double().flatten(2)
    else:
        du = dz * (ua[..., None] * x + ub[..., None] > 0) if relu else dz
    A, B = tot((du * w).sum(-1)), tot((du * (x - mc[..., None]) * rc[..., None] * w).sum(-1))
    s1, s2 = grp(gam * A) / (n if lt.batch else 1), grp(gam * B) / (n if lt.batch else 1)    # (A, B are totals already)
    k2 = -rstd * rstd * s2 / count
    k3 = (rstd * rstd * s2 * mean - rstd * s1) / count
    if fault == "k2 dropped":
        k2 = torch.zeros_like(k2)
    if fault == "k3 dropped":
        k3 = torch.zeros_like(k3)
    dx = (pc(rstd) * gam)[..., None] * du + pc(k2)[..., None] * x + pc(k3)[..., None]
    shape = (n, c, *lt.shape)
    out.update(dx=dx.reshape(shape), dres=(dz if fault == "dres before act'" else du).reshape(shape),
               dgamma=B[0] if lt.batch else B.sum(0), dbeta=A[0] if lt.batch else A.sum(0))
    return out


NAMED = {"neighbour group": ["dgamma", "dx"], "k2 dropped": ["dx"], "k3 dropped": ["dx"], "tail voxel": ["stats", "coef", "dbeta", "dx"],
         "row twice": ["stats", "coef", "dbeta", "dx"], "dres before act'": ["dres"], "coef row": ["y"]}


def each_fault_changes_its_output(v, dz, relu, mask=None, skip=()):
    """Without a fault the model IS the reference (after the same snap), element by element; with each fault that exists for
    the call, every output named for it differs from the model without it."""
    lt = v.lt
    y, stats, coef = N.forward_ref(lt, v.beta)
    ref = dict(y=y, stats=stats, coef=coef, dx=v.dx, dres=v.du, dgamma=v.dgamma, dbeta=v.dbeta)
    good = model(lt, v.beta, dz, relu, mask=mask)
    for k in ref:
        assert torch.equal(snap(good[k]), ref[k]), f"model without a fault: {k} differs from ATen ({v.name})"
    for fault in FAULTS:
        if fault in skip:
            continue
        bad = model(lt, v.beta, dz, relu, fault, mask=mask)
        for k in NAMED[fault]:
            assert not torch.equal(bad[k], good[k]), f"{fault}: {k} is unchanged ({v.name}, {lt.c} channels, {lt.shape}, eps {lt.eps})"


def absent(lt, act):
    """The faults that do not exist for a call: no neighbouring group, no second sample, no activation."""
    return ([] if lt.groups > 1 else ["neighbour group"]) + ([] if lt.n > 1 else ["coef row"]) + ([] if act else ["dres before act'"])


@pytest.mark.parametrize("eps", N.EPS)
@pytest.mark.parametrize("case", N.GN_CASES, ids=N.case_id)
def test_each_fault_changes_its_output(case, eps):
    vs = {v.name: v for v in N.gn_variants(case, eps)}
    for relu, v in ((False, vs["none"]), (True, vs["relu recomputed"])):
        each_fault_changes_its_output(v, v.lt.du, relu, skip=absent(v.lt, relu))


@pytest.mark.parametrize("pool", ["max", "avg"])
@pytest.mark.parametrize("eps", N.EPS)
@pytest.mark.parametrize("case", N.POOL_CASES, ids=N.case_id)
def test_each_fault_changes_its_output_in_the_pooling_join(case, eps, pool):
    """The kernel's dz is the joined gradient (pooling backward + skip), its mask the sign of the z handed in."""
    v, _, _ = N.pool_inputs(case, eps, pool)
    each_fault_changes_its_output(v, v.dz, True, mask=v.z > 0, skip=absent(v.lt, True))


@pytest.mark.parametrize("eps", N.EPS)
@pytest.mark.parametrize("case", N.BN_CASES, ids=N.case_id)
def test_each_fault_changes_its_output_in_batchnorm(case, eps):
    """BatchNorm: a group is a channel, the sums run over the samples.  Its stats / coef / bcoef rows are replicated, so "the
    second sample's row for the first" changes nothing BY CONSTRUCTION: that fault does not exist here (the one that does, a
    replica nobody wrote, shows as NaN in the GPU test, which compares all n rows)."""
    vs = {v.name: v for v in N.bn_variants(case, eps)}
    for relu, v in ((False, vs["none"]), (True, vs["relu recomputed"])):
        lt = v.lt
        assert torch.equal(lt.m[0], lt.m[-1]) and torch.equal(lt.sigma[0], lt.sigma[-1])
        each_fault_changes_its_output(v, lt.du, relu, skip=absent(lt, relu) + ["coef row"])
