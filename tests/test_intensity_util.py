"""The numpy model of tests/intensity_util.py on the CPU: it equals np.sort(members)[rank] on the hostile inputs the GPU tests use,
the percentile chain equals its fp64 restatement, and every injectable fault is rejected by the check that is there for it."""
import math

import numpy as np
import pytest

import intensity_util as U

SHAPE = (17, 19, 13)


def ranks_and_pairs(n):
    ranks = set(U.check_ranks(n))
    for q in (0, 0.5, 50, 99.5, 100):
        a, b, _ = U.percentile_ranks(q, n)
        ranks.update((a, b))
    return sorted(ranks)


def select_ok(x, mask, **fault):
    want = U.sorted_members(x, mask)
    ranks = ranks_and_pairs(len(want))
    for k in range(0, len(ranks), U.MAX_RANKS):
        rk = ranks[k:k + U.MAX_RANKS]
        got = U.order_statistics(x, rk, mask, **fault)
        if not U.same_values(got, want[rk] if len(want) else np.full(len(rk), np.nan, np.float32)):
            return False
    return True


# ---------------------------------------------------------------------------------------------- the model is right
@pytest.mark.parametrize("dt", list(U.NP_DT))
@pytest.mark.parametrize("name", U.HOSTILE)
def test_model_select_equals_sort(name, dt):
    x = U.hostile(name, SHAPE, dt, seed=1)
    assert select_ok(x, None) and select_ok(x, U.random_mask(SHAPE, 2))


def test_keys_are_monotone_and_invert():
    v = np.array([-np.inf, -65504.0, -1.0, -2.0 ** -126, -2.0 ** -149, -0.0, 0.0, 2.0 ** -149, 2.0 ** -126, 1.0, 1.0 + 2.0 ** -23, np.inf],
                 dtype=np.float32)
    k = U.key_of(v)
    assert (np.diff(k.astype(np.int64)) >= 0).all() and k[5] == k[6] and (np.diff(k.astype(np.int64))[[0, 1, 2, 3, 4, 6, 7, 8, 9, 10]] > 0).all()
    assert U.same_values(U.value_of(k), v)


def test_small_member_counts_and_out_of_range_ranks():
    x = np.array([3.0, np.nan, -2.0, 5.0], dtype=np.float32)
    one = np.array([0, 0, 1, 0], dtype=np.uint8)
    assert U.same_values(U.order_statistics(x, [0, 1, 2], one), [-2.0, np.nan, np.nan])
    two = np.array([1, 1, 1, 0], dtype=np.uint8)
    assert U.same_values(U.order_statistics(x, [0, 1, 2, -1], two), [-2.0, 3.0, np.nan, np.nan])
    assert U.same_values(U.order_statistics(x, [0, 7], np.zeros(4, np.uint8)), [np.nan, np.nan])
    assert U.count_nan(x, two) == 1 and U.count_nan(x, one) == 0 and len(U.members(x, two)) == 2


def test_pooled_cases_equal_the_concatenation():
    cases = [(U.hostile("air60", s, "f32", seed=k), U.random_mask(s, k)) for k, s in enumerate([(5, 6, 7), (17, 19, 13), (3, 4, 50)])]
    want = U.sorted_members(cases)
    ranks = U.check_ranks(len(want))
    assert U.same_values(U.order_statistics(cases, ranks), want[ranks])


# ---------------------------------------------------------------------------------------------- percentiles
def test_percentile_chain_equals_its_fp64_restatement_and_numpy():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 10, 201, 4199):
        s = np.sort(rng.normal(0, 100, n).astype(np.float32))
        for q in (0, 0.5, 2.5, 50, 97.5, 99.5, 100):
            a, b, t = U.percentile_ranks(q, n)
            assert 0 <= a <= b <= n - 1 and 0.0 <= t < 1.0
            v = U.percentile_value(s[a], s[b], t)
            assert v == U.percentile_restated(s[a], s[b], t)
            assert abs(v - np.percentile(s.astype(np.float64), q)) <= 4 * U.U64 * max(abs(float(s[a])), abs(float(s[b])))
    assert U.percentile_ranks(50, 0) == (0, 0, 0.0)
    assert U.percentile_value(np.float32(3.0), np.float32(np.inf), 0.0) == 3.0          # exactly a: no inf * 0


def test_fused_interpolation_is_rejected():
    """A chain with the product and the sum fused differs from the pinned one on some (a, b, t): the restatement sees it."""
    rng = np.random.default_rng(6)
    differs = 0
    for _ in range(400):
        a, b = np.sort(rng.normal(0, 100, 2).astype(np.float32))
        t = float(rng.random())
        assert U.percentile_value(a, b, t) == U.percentile_restated(a, b, t)
        differs += U.percentile_value(a, b, t, fault="fma") != U.percentile_restated(a, b, t)
    assert differs > 0


# ---------------------------------------------------------------------------------------------- every fault is rejected
def test_sign_magnitude_key_order_is_rejected():
    x = U.hostile("mixed", SHAPE, "f32", seed=1)
    assert select_ok(x, None) and not select_ok(x, None, key_fault="sign_magnitude")


def test_negative_zero_below_positive_zero_is_rejected():
    """With a key of its own, -0.0 sorts below +0.0 and next to the negative subnormals: the value at a rank is still +-0 (== cannot
    tell), so the check is on the keys -- equal values must have equal keys -- and on the count below zero."""
    z = np.array([0.0, -0.0], dtype=np.float32)
    assert U.key_of(z)[0] == U.key_of(z)[1]
    assert U.key_of(z, fault="neg_zero")[0] != U.key_of(z, fault="neg_zero")[1]
    x = np.array([-0.0, -2.0 ** -149, 0.0, -0.0, 2.0 ** -149], dtype=np.float32)
    k = U.key_of(x, fault="neg_zero")
    assert not (k[0] == k[2] == k[3])


def test_prefix_one_bit_short_is_rejected():
    """Values 1 + k 2^-23 with k < 4096 differ in key bits 0 .. 11: a last-level prefix that ignores bit 10 pools two bins' worth."""
    k = np.random.default_rng(8).integers(0, 4096, 4199)
    x = (1.0 + k * 2.0 ** -23).astype(np.float32)
    assert select_ok(x, None) and not select_ok(x, None, select_fault="short_prefix")


def test_rank_off_by_one_at_a_bin_boundary_is_rejected():
    x = np.repeat(np.array([1.0, 2.0, 4.0, 8.0], dtype=np.float32), 5)      # ranks 5, 10, 15 sit exactly on bin boundaries
    assert U.same_values(U.order_statistics(x, [4, 5, 9, 10, 15]), [1, 2, 2, 4, 8])
    assert not U.same_values(U.order_statistics(x, [4, 5, 9, 10, 15], select_fault="boundary_rank"), [1, 2, 2, 4, 8])


def test_nan_counted_as_a_member_is_rejected():
    x = U.hostile("nans", SHAPE, "f32", seed=1)
    n_ok, n_bad = len(U.members(x)), len(U.members(x, fault="nan_member"))
    assert n_bad == n_ok + U.count_nan(x) and U.count_nan(x) > 0
    want = U.sorted_members(x)
    ranks = U.check_ranks(len(want))
    assert U.same_values(U.order_statistics(x, ranks), want[ranks])
    # a counted NaN is a valid rank past the members (its key is above +inf's) ...
    keys = U.key_of(U.members(x, fault="nan_member"))
    assert U.radix_select(keys, [n_ok])[1][0] and not U.radix_select(U.key_of(U.members(x)), [n_ok])[1][0]
    # ... and one with the sign bit set sorts below -inf: rank 0 is no longer the minimum
    y = x.copy()
    y[np.isnan(y)] = np.float32(-np.nan)
    y.reshape(-1)[:2] = np.array([0xFFC00000, 0xFF800001], dtype=np.uint32).view(np.float32)
    want = U.sorted_members(y)
    ranks = U.check_ranks(len(want))
    assert U.same_values(U.order_statistics(y, ranks), want[ranks])
    assert not U.same_values(U.order_statistics(y, ranks, member_fault="nan_member"), want[ranks])


def test_sum_of_squares_variance_on_offset_data_is_rejected():
    rng = np.random.default_rng(7)
    for mean, sd in ((1e4, 1.0), (-1000.0, 0.25)):
        m = (mean + sd * rng.standard_normal(4199)).astype(np.float32)
        ref, bad = U.moments(m), U.moments(m, fault="sumsq")
        bound = U.moments_bound(m, U.sum_depth([SHAPE]))
        assert abs(ref["std"] - np.std(m.astype(np.float64))) <= bound["std"]
        assert abs(bad["std"] - ref["std"]) > bound["std"], (mean, bad["std"], ref["std"], bound)


def test_nan_coming_through_the_clip_is_rejected():
    x = U.hostile("nans", (1,) + SHAPE, "f32", seed=3)
    table = np.array([[-10.0, 10.0, 1.0, 0.5]], dtype=np.float32)
    good, bad = U.apply(x, table, np.float32, fill=7.0), U.apply(x, table, np.float32, fill=7.0, fault="nan_through")
    nan = np.isnan(x)
    assert nan.any() and (good[nan] == 7.0).all() and np.isfinite(good).all()
    assert (bad[nan] == np.float32((-10.0 - 1.0) * 0.5)).all() and not np.array_equal(good, bad)


# ---------------------------------------------------------------------------------------------- table, apply, bounds
def test_table_rows():
    assert list(U.apply_table("zscore", 2.0, 4.0, 0, 0, 1e-8)) == [-math.inf, math.inf, 2.0, 0.25]
    assert list(U.apply_table("zscore", 2.0, 0.0, 0, 0, 0.5)) == [-math.inf, math.inf, 2.0, 2.0]
    assert list(U.apply_table("ct", 2.0, 4.0, -1.0, 3.0, 1e-8)) == [-1.0, 3.0, 2.0, 0.25]
    assert list(U.apply_table("rescale", 2.0, 4.0, -1.0, 3.0, 1e-8)) == [-1.0, 3.0, -1.0, 0.25]
    assert U.apply_table("rescale", 0, 0, 5.0, 5.0, 1e-8)[3] == np.float32(1e8)
    assert U.apply_table("zscore", np.nan, np.nan, 0, 0, 1e-8)[3] == np.float32(1e8)


def test_apply_restatement():
    x = np.array([[[[-5.0, -1.0, 0.0, 3.0, 9.0, np.nan, np.inf, -np.inf]]]], dtype=np.float32)
    table = np.array([[-1.0, 3.0, 1.0, 2.0]], dtype=np.float32)
    mask = np.array([[[1, 1, 0, 1, 1, 1, 1, 1]]], dtype=np.uint8)
    assert list(U.apply(x, table, np.float32, mask, fill=-9.0)[0, 0, 0]) == [-4.0, -4.0, -9.0, 4.0, 4.0, -9.0, 4.0, -4.0]
    wide = np.array([[-np.inf, np.inf, 0.0, 1e-6]], dtype=np.float32)
    y = U.apply(np.array([[[[1.0, 65504.0 * 1e6 * 2, 1e-2]]]], dtype=np.float32), wide, np.float16)
    assert y.dtype == np.float16 and y[0, 0, 0, 0] > 0 and y[0, 0, 0, 0] < 2.0 ** -14 and np.isinf(y[0, 0, 0, 1])


def test_row_plan_and_depth():
    assert U.row_plan(5 * 6 * 7) == (1, 256) and U.row_plan(4199) == (2, 2304)
    rows, share = U.row_plan(208 * 208 * 200)
    assert rows == 2048 and share > 4096 and share % 256 == 0 and rows * share >= 208 * 208 * 200
    assert U.sum_depth([(5, 6, 7)]) < U.sum_depth([(208, 208, 200)]) < 100


def test_moments_on_a_lattice_are_exact():
    m = np.tile(np.array([1.0, 3.0, 5.0, 7.0], dtype=np.float32), 1024)
    r = U.moments(m)
    assert (r["n"], r["min"], r["max"], r["mean"], r["m2"]) == (4096, 1.0, 7.0, 4.0, 4096 * 5.0)
