"""CPU side of tests/test_gpu_rounding.py: (1) the premises -- every sum exact, enough elements that are no numbers of the output
type, exact ties in both directions, the subnormal / overflow / candidate-difference counts -- hold for every case of the GPU
module whose fp64 reference is small enough to build here (the large shapes assert them inside their GPU test), and (2) the
comparison rejects each fault it is there for: the fault is applied to the reference with torch, fed to the same checker, and
the failure names the first coordinates."""
import pytest
import torch

import test_gpu_rounding as R
from gpu_util import assert_rounded, assert_rounding_premises, census_counts, check_gn_sums, neighbours, rounding_census

X = R.X
SMALL = 300000   # voxels x widest channel count up to which a case's fp64 reference is built in the CPU suite (test_exact_util's)
FIRST_AT = r"first at \(\d+, \d+, \d+, \d+, \d+\)"


def _small(n, cin, cout, shape, up=1):
    return n * shape[0] * shape[1] * shape[2] * up * max(cin, cout) <= SMALL


def _small_kernel(name):
    kind, n, cin, cout, shape = R.KERNELS[name][:5]
    return _small(n, cin, cout, shape, 8 if kind == "convt" else 1)


# ------------------------------------------------------------------------------------------------ the census itself
def test_the_census_counts_ties_subnormals_zeros_and_infinities():
    h = torch.float16
    v = torch.tensor([2049.0, 2051.0, 2050.0, -2049.0, 4097.0, 3 * 2.0 ** -25, 2.0 ** -25, -2.0 ** -26, 65519.0, 65520.0, -70000.0, 0.0, 1.0],
                     dtype=torch.float64)
    cen = rounding_census(v, h)
    towards, away = neighbours(v, h)
    assert towards.tolist()[:5] == [2048.0, 2050.0, 2050.0, -2048.0, 4096.0] and away.tolist()[:5] == [2050.0, 2052.0, 2050.0, -2050.0, 4100.0]
    assert cen.nonrep.tolist() == [True, True, False, True, True, True, True, True, True, True, True, False, False]
    assert cen.tie_zero.tolist() == [True, False, False, True, False, False, True, False, False, False, False, False, False]
    assert cen.tie_away.tolist() == [False, True, False, False, False, True, False, False, False, True, False, False, False]
    assert cen.sub.tolist()[5:8] == [True, False, False] and cen.zeroed.tolist()[5:8] == [False, True, True]
    assert cen.inf.tolist()[8:11] == [False, True, True] and float(cen.rne[8]) == 65504.0
    b = rounding_census(torch.tensor([257.0, 259.0, 258.0, -515.0], dtype=torch.float64), torch.bfloat16)
    assert b.tie_zero.tolist() == [True, False, False, False] and b.tie_away.tolist() == [False, True, False, False] and b.nonrep.tolist() == [True, True, False, True]
    with pytest.raises(AssertionError, match="ties towards zero"):
        assert_rounding_premises(torch.arange(2049.0, 4096.0, 4.0, dtype=torch.float64).repeat(4), h, "one direction only")
    with pytest.raises(AssertionError, match="are no torch.float16 numbers"):
        assert_rounding_premises(torch.arange(0.0, 2048.0, dtype=torch.float64), h, "representable")
    assert assert_rounded(torch.tensor([-0.0, 2048.0]).half(), torch.tensor([-2.0 ** -26, 2049.0], dtype=torch.float64), h, "signed zero") == 2
    with pytest.raises(AssertionError, match=r"zeros carry the wrong sign; first at \(0,\)"):
        assert_rounded(torch.tensor([0.0, 2048.0]).half(), torch.tensor([-2.0 ** -26, 2049.0], dtype=torch.float64), h, "signed zero")


# ------------------------------------------------------------------------------------------------ premises
@pytest.mark.parametrize("name,mode", [p for p in R.STORE_PARAMS if _small_kernel(p[0])])
def test_premises_of_the_store_rounding_cases(name, mode):
    c = R.kernel_case(name, mode)
    c.premises(mode)
    with X.options(**R.KERNELS[name][7]):
        R.check_plan(name, mode)      # (the plan queries need no device)


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp16x2"])
@pytest.mark.parametrize("cin", [1, 4])
def test_premises_of_the_first_layer_cases(mode, cin):
    R.rcase("conv", 2, cin, 32, (9, 11, 21), R.M_FEW[mode], amp=3).premises(mode, keys=("y",))


@pytest.mark.parametrize("mode", X.MODES16)
@pytest.mark.parametrize("name", ["convt", "convt-direct"])
def test_premises_of_the_conv_transpose_join(name, mode):
    c = R.kernel_case(name, mode, bias=True, skip=True)
    c.premises(mode)
    one, two, differ = R.convt_join(c, mode)
    assert differ >= 0.01 * one.numel()


@pytest.mark.parametrize("mode", X.MODES16)
def test_premises_of_the_data_gradient_join_and_of_the_statistics(mode):
    key = R.JOIN_CASES[0][2]
    assert _small(*key)
    t = R.dgrad_join_inputs(key, mode)
    assert t["differ"] >= 0.01 * t["one"].numel() and not torch.equal(t["plain"], t["two"])
    n, cin, cout, shape, _, _ = R.DGRAD_STATS_CASES[0]
    assert _small(n, cin, cout, shape)
    R.dgrad_stats_premises(n, cin, cout, shape, mode)
    s = R.sparse_case(2, 32, 32, (9, 11, 21), mode)      # (the forward cases are too large for this suite: the same recipe at the small shape)
    R.fwd_stats_premises(s["y"], R.DT[mode], "fwd sums")


@pytest.mark.parametrize("edge", R.EDGES)
@pytest.mark.parametrize("name,mode", [p for p in R.EDGE_KERNELS if _small_kernel(p[0])])
def test_premises_of_the_fp16_edges(name, mode, edge):
    base = R.kernel_case(name, mode)
    base.premises(mode)
    c, minima = R.edge_variant(base, edge)
    R.assert_subnormal_operands(c, edge)
    cens = c.premises(mode, **minima)
    for k, cen in cens.items():
        n = census_counts(cen)
        if edge == "subnormal-out":
            assert n["sub"] >= 1000
        elif edge == "tiny-out":
            assert n["zeroed"] >= 100
        elif edge == "overflow":
            assert 0.01 * n["elements"] <= n["inf"] <= 0.5 * n["elements"]
        else:
            assert n["sub"] == 0 and n["inf"] == 0


@pytest.mark.parametrize("mode", X.MODES16)
def test_premises_of_the_small_joins(mode):
    for c, shape, kind in R.POOL_CASES:
        R.pool_case(mode, c, shape, kind)
    for args in R.UPCAT_CASES:
        R.upcat_case(mode, *args)


# ------------------------------------------------------------------------------------------------ injected faults
def _general(mode="fp16"):
    c = R.kernel_case("general", mode)
    c.premises(mode)
    return c


@pytest.mark.parametrize("mode", X.MODES16)
def test_truncation_and_round_half_away_are_rejected(mode):
    c, dt = _general(mode), R.DT[mode]
    for k in ("y", "dx"):
        v = c.ref()[0][k]
        cen = rounding_census(v, dt)
        assert assert_rounded(cen.rne.to(dt), v, dt, k) == v.numel()
        with pytest.raises(AssertionError, match=r"\d+ of 133056 elements differ.*" + FIRST_AT):
            assert_rounded(cen.towards.to(dt), v, dt, k)                                       # truncation
        half_away = torch.where(cen.tie_zero, cen.away, cen.rne)
        with pytest.raises(AssertionError, match=rf"{int(cen.tie_zero.sum())} of 133056 elements differ.*" + FIRST_AT):
            assert_rounded(half_away.to(dt), v, dt, k)                                         # round half away from zero
        half_down = torch.where(cen.tie_away, cen.towards, cen.rne)
        with pytest.raises(AssertionError, match=rf"{int(cen.tie_away.sum())} of 133056 elements differ"):
            assert_rounded(half_down.to(dt), v, dt, k)                                         # ... and half towards zero


def test_flushed_subnormal_results_are_rejected():
    h = torch.float16
    c, _ = R.edge_variant(_general(), "subnormal-out")
    v = c.ref()[0]["dx"]
    cen = rounding_census(v, h)
    flushed = torch.where(cen.sub, torch.zeros_like(cen.rne), cen.rne)
    with pytest.raises(AssertionError, match=rf"{int(cen.sub.sum())} of 133056 elements differ.*" + FIRST_AT):
        assert_rounded(flushed.to(h), v, h, "dx")
    # a result below half the smallest subnormal must carry its sign
    c, _ = R.edge_variant(_general(), "tiny-out")
    v = c.ref()[0]["y"]
    cen = rounding_census(v, h)
    assert bool((cen.zeroed & (v < 0)).any())
    with pytest.raises(AssertionError, match="zeros carry the wrong sign"):
        assert_rounded(cen.rne.abs().to(h) * torch.where(cen.rne == 0, 1.0, torch.sign(cen.rne)).to(h), v, h, "y")


@pytest.mark.parametrize("edge", ["subnormal-x", "subnormal-w"])
def test_subnormal_inputs_flushed_before_the_product_are_rejected(edge):
    h = torch.float16
    c, _ = R.edge_variant(_general(), edge)
    flush = lambda t: torch.where(t.abs() < R.F16_TINY, torch.zeros_like(t), t)
    got = c.base._run(flush(c.x), flush(c.w), None, flush(c.g), None)
    for k in ("y", "dx"):
        with pytest.raises(AssertionError, match=r"elements differ.*" + FIRST_AT):
            assert_rounded(got[k].to(h), c.ref()[0][k], h, k)


def test_a_saturating_store_is_rejected():
    h = torch.float16
    c, minima = R.edge_variant(_general(), "overflow")
    cens = c.premises("fp16", **minima)
    v = c.ref()[0]["y"]
    n_inf = int(cens["y"].inf.sum())
    with pytest.raises(AssertionError, match=rf"{n_inf} of 133056 elements differ.*" + FIRST_AT):
        assert_rounded(cens["y"].rne.clamp(-65504.0, 65504.0).to(h), v, h, "y")
    with pytest.raises(AssertionError, match=r"elements differ \(\d+ NaN\)"):
        assert_rounded(torch.where(cens["y"].inf, torch.full_like(v, float("nan")), cens["y"].rne).to(h), v, h, "y")   # inf - inf


@pytest.mark.parametrize("mode", X.MODES16)
def test_the_wrong_number_of_roundings_in_a_join_is_rejected(mode):
    dt = R.DT[mode]
    c = R.kernel_case("convt", mode, bias=True, skip=True)
    one, two, _ = R.convt_join(c, mode)
    with pytest.raises(AssertionError, match=r"elements differ.*" + FIRST_AT):
        assert_rounded(two.to(dt), c.ref()[0]["y"], dt, "ConvTranspose3d join rounded twice")
    t = R.dgrad_join_inputs(R.JOIN_CASES[0][2], mode)
    with pytest.raises(AssertionError, match=r"elements differ.*" + FIRST_AT):
        R.assert_exact(t["one"].to(dt), t["two"], "data-gradient join rounded once")
    assert R.assert_exact(t["two"].to(dt), t["two"], "two") == t["two"].numel()


@pytest.mark.parametrize("mode", X.MODES16)
def test_statistics_summed_before_the_rounding_are_rejected(mode):
    dt = R.DT[mode]
    s = R.sparse_case(2, 32, 32, (9, 11, 21), mode)
    stored, want = R.fwd_stats_premises(s["y"], dt, "fwd sums")[R.L.ACT_NONE]
    rows = lambda t: torch.stack((t.sum((2, 3, 4)), (t * t).sum((2, 3, 4))), -1).reshape(2, 16, 2, 2).sum(2).repeat_interleave(2, 1)[:, None] \
        * torch.tensor([1.0, 0.0]).repeat(16)[None, None, :, None]
    assert R.compare_stored_sums(rows(stored), want, "sums of the stored values") > 0
    with pytest.raises(AssertionError, match=r"sum of the STORED values.*first at \(\d+, \d+\)"):
        R.compare_stored_sums(rows(s["y"]), want, "sums of the accumulators")
    # the GroupNorm backward's rows: exact against the stored gradient, rejected when taken from the unrounded one
    n, cin, cout, shape, _, _ = R.DGRAD_STATS_CASES[0]
    s, add, gy, coef, pre, variants = R.dgrad_stats_premises(n, cin, cout, shape, mode)
    stored, du = variants[(True, R.L.ACT_RELU)]
    part = lambda d: torch.stack((d.sum((2, 3, 4)), (d * gy.double()).sum((2, 3, 4))), -1)[:, None]
    check_gn_sums(part(du), stored, pre, gy, R.L.ACT_RELU, "stored")
    assert X.compare_channel_sums(part(du), du, gy.double(), "stored") > 0
    early = X.gn_reference(s["dx"] + add.double(), pre, R.L.ACT_RELU)
    with pytest.raises(AssertionError, match=r"elements differ.*first at \(\d+, \d+, \d+\)"):
        X.compare_channel_sums(part(early), du, gy.double(), "from the accumulators")
