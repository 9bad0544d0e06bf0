"""Intensity normalisation on the GPU (csrc/intensity.hip, mednet_hip.intensity) against the numpy model of tests/intensity_util.py:
order statistics equal np.sort of the members value for value, moments are bit-equal on integer lattices and within the derived
bound of profiles/intensity_bounds.md elsewhere (the observed fractions are printed, pytest -s shows them), the parameter table and
the apply pass are bit-equal to their restatements, the schemes end to end, the mask and its box, guard bands, the predictor.

Shapes (row_plan of csrc/volume.h): 5 x 6 x 7 is one workgroup; 17 x 19 x 13 = 4199 voxels has a second row with a ragged last
block, an odd w and so a vector-load head and tail in every channel after the first; 208 x 208 x 200 is just over 2048 x 4096
voxels, where a row's share exceeds 4096 (one test only)."""
import math

import numpy as np
import pytest
import torch

import intensity_util as U
import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import intensity as M
from mednet_hip import predict as HP
from mednet_hip.unet import model as HM
from oracle import ref_cpu as O

from fence import Fence
from gpu_util import DEV

pytestmark = pytest.mark.gpu

ONE, TWO_ROWS, ROW_LIMIT = (5, 6, 7), (17, 19, 13), (208, 208, 200)
TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "i16": torch.int16, "u8": torch.uint8}
QS = (0, 0.5, 50, 99.5, 100)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def odd_view(mask):
    """The mask as a view at an odd byte offset that ends where its allocation's payload ends."""
    buf = torch.empty(mask.size + 3, dtype=torch.uint8, device=DEV)
    buf[3:].copy_(dev(mask).reshape(-1))
    return buf[3:].view(mask.shape)


def volume(name, c, shape, dt, seed):
    return np.stack([U.hostile(name, shape, dt, seed=seed + 10 * k) for k in range(c)])


def wanted_ranks(n):
    ranks = set(U.check_ranks(n))
    for q in QS:
        ranks.update(U.percentile_ranks(q, n)[:2])
    return sorted(ranks)


def check_select(vols, masks, put=dev, put_mask=None):
    """vols: one C x D x H x W array or a list of them (pooled), masks alike (None: no mask).  Every channel, every wanted rank."""
    pooled = isinstance(vols, list)
    vols, masks = (vols, masks) if pooled else ([vols], [masks])
    c = vols[0].shape[0]
    want = [U.sorted_members([(v[k], m) for v, m in zip(vols, masks)]) for k in range(c)]
    per = [wanted_ranks(len(w)) for w in want]
    tv = [put(v) for v in vols]
    tm = [None if m is None else (put_mask or odd_view)(m) for m in masks]
    for at in range(0, max(len(p) for p in per), U.MAX_RANKS):
        rows = [(p[at:at + U.MAX_RANKS] + [0] * U.MAX_RANKS)[:U.MAX_RANKS] for p in per]
        got = host(M.order_statistics(tv if pooled else tv[0], dev(np.array(rows, dtype=np.int64)), tm if pooled else tm[0]))
        assert got.dtype == np.float32 and got.shape == (c, U.MAX_RANKS)
        for k in range(c):
            exp = want[k][rows[k]] if len(want[k]) else np.full(U.MAX_RANKS, np.nan, np.float32)
            assert U.same_values(got[k], exp), (k, rows[k], got[k], exp)
    return tv, tm


# ---------------------------------------------------------------------------------------------- 1. select is exact
@pytest.mark.parametrize("dt", list(TORCH_DT))
@pytest.mark.parametrize("name", U.HOSTILE)
def test_select_equals_sort(name, dt):
    for c, shape in ((1, ONE), (3, TWO_ROWS)):
        vol = volume(name, c, shape, dt, seed=3)
        check_select(vol, None)
        check_select(vol, U.random_mask(shape, seed=4))


def test_select_with_a_list_of_ranks_and_a_volume_without_channels():
    vol = U.hostile("air60", TWO_ROWS, "i16", seed=5)
    want = U.sorted_members(vol)
    ranks = U.check_ranks(len(want))
    got = M.order_statistics(dev(vol), ranks)
    assert tuple(got.shape) == (1, len(ranks)) and got.device.type == "cuda" and U.same_values(host(got)[0], want[ranks])


def test_small_member_counts_and_the_empty_mask():
    vol = volume("nans", 2, ONE, "f32", seed=6)
    vol[0, 0, 0, :3] = [np.nan, 3.0, -2.0]
    for keep, n in ((((0, 0, 1),), 1), (((0, 0, 1), (0, 0, 2)), 2), (((0, 0, 0),), 0), ((), 0)):
        mask = np.zeros(ONE, np.uint8)
        for p in keep:
            mask[p] = 1
        stats = M.intensity_stats(dev(vol), dev(mask), percentiles=QS[:4]).to_host()
        got = host(M.order_statistics(dev(vol), [0, 1, 2, -1], dev(mask)))
        m0 = U.sorted_members(vol[0], mask)
        assert len(m0) == n and int(stats.n[0]) == n and int(stats.n_nan[0]) == U.count_nan(vol[0], mask)
        exp = np.full(4, np.nan, np.float32)
        exp[:n] = m0
        assert U.same_values(got[0], exp)
        if n == 0:
            for f in ("min", "max", "mean", "std"):
                assert bool(torch.isnan(getattr(stats, f)[0])), f
            assert bool(torch.isnan(stats.percentiles[0]).all()) and bool(torch.isnan(stats.order[0]).all())
        else:
            assert float(stats.min[0]) == m0[0] and float(stats.max[0]) == m0[-1]
            assert same_bits(host(stats.percentiles[0]), U.percentiles_of(m0, QS[:4])[0])


def test_channels_are_independent():
    vol = volume("air60", 3, TWO_ROWS, "f32", seed=7)
    mask = U.random_mask(TWO_ROWS, seed=8)
    ranks = [0, 5, 700, 1500, 1600]
    a = host(M.order_statistics(dev(vol), ranks, dev(mask)))
    b = host(M.order_statistics(dev(vol[[2, 0, 1]]), ranks, dev(mask)))
    assert same_bits(a[[2, 0, 1]], b) and not same_bits(a, b)


def test_pooled_cases_equal_their_concatenation():
    shapes = [ONE, TWO_ROWS, (3, 4, 50)]
    vols = [volume("air60" if k else "nans", 2, s, "f32", seed=20 + k) for k, s in enumerate(shapes)]
    masks = [U.random_mask(s, seed=30 + k) for k, s in enumerate(shapes)]
    check_select(vols, masks)
    check_select(vols, [None] * 3)
    stats = M.intensity_stats([dev(v) for v in vols], [dev(m) for m in masks], percentiles=(0.5, 50, 99.5)).to_host()
    for k in range(2):
        m = U.sorted_members([(v[k], mk) for v, mk in zip(vols, masks)])
        assert int(stats.n[k]) == len(m) and int(stats.n_nan[k]) == sum(U.count_nan(v[k], mk) for v, mk in zip(vols, masks))
        pct, order, frac = U.percentiles_of(m, (0.5, 50, 99.5))
        assert same_bits(host(stats.percentiles[k]), pct) and same_bits(host(stats.frac[k]), frac)
        assert U.same_values(host(stats.order[k]), order)
        assert float(stats.min[k]) == m[0] and float(stats.max[k]) == m[-1]


def test_row_limit():
    """Just over 2048 x 4096 voxels: 2048 rows whose share exceeds 4096.  int16, 60 % air, a mask: select, counts and moments."""
    vol = U.hostile("air60", ROW_LIMIT, "i16", seed=9)
    mask = U.random_mask(ROW_LIMIT, seed=10, keep=0.7)
    assert U.row_plan(vol.size)[0] == 2048 and U.row_plan(vol.size)[1] > 4096
    stats = M.intensity_stats(dev(vol), dev(mask), percentiles=(0.5, 50, 99.5)).to_host()
    m = U.sorted_members(vol, mask)
    pct, order, _ = U.percentiles_of(m, (0.5, 50, 99.5))
    assert int(stats.n[0]) == len(m) and int(stats.n_nan[0]) == 0
    assert U.same_values(host(stats.order[0]), order) and same_bits(host(stats.percentiles[0]), pct)
    ref = U.moments(m)
    bound = U.moments_bound(m, U.sum_depth([ROW_LIMIT]))
    assert float(stats.min[0]) == ref["min"] and float(stats.max[0]) == ref["max"]
    print(f"row limit: mean {abs(float(stats.mean[0]) - ref['mean']) / bound['mean']:.3f} std {abs(float(stats.std[0]) - ref['std']) / bound['std']:.3f} of the bound")
    assert abs(float(stats.mean[0]) - ref["mean"]) <= bound["mean"] and abs(float(stats.std[0]) - ref["std"]) <= bound["std"]


# ---------------------------------------------------------------------------------------------- 2. moments
def table_of(vols, masks=None):
    cases = M._cases(vols, masks, "test")
    return M._table_fields(M._moments(cases))


@pytest.mark.parametrize("dt", ["f32", "i16", "f16", "u8"])
def test_moments_on_integer_lattices_equal_numpy_bit_for_bit(dt):
    """n a power of two and an integer mean: every partial sum of x and of (x - mean)^2 is an integer below 2^53, exact in any order."""
    shape, mean = (16, 16, 32), 37
    rng = np.random.default_rng(11)
    half = rng.integers(0, 75, (2, 8, 16, 32)) if dt == "u8" else rng.integers(-400, 475, (2, 8, 16, 32))
    vol = np.concatenate([half, 2 * mean - half], axis=1).astype(U.NP_DT[dt])
    assert vol.shape == (2,) + shape and U.row_plan(vol[0].size)[0] == 2
    got = {k: host(v) for k, v in table_of(dev(vol)).items()}
    for k in range(2):
        x = vol[k].astype(np.float64).reshape(-1)
        m2 = np.sum((x - x.mean()) ** 2)
        assert x.mean() == mean and got["n"][k] == x.size and got["n_nan"][k] == 0
        assert got["min"][k] == x.min() and got["max"][k] == x.max() and got["mean"][k] == np.float64(mean)
        assert same_bits(got["std"][k], np.sqrt(m2 / x.size)) and got["std"][k] == np.std(x)
        assert got["std"][k] ** 2 * x.size == pytest.approx(m2, rel=4 * U.U64)


@pytest.mark.parametrize("case", ["random", "offset_1e4", "offset_-1000"])
def test_moments_within_the_derived_bound(case):
    rng = np.random.default_rng(12)
    shape = TWO_ROWS
    base = rng.standard_normal((2,) + shape)
    vol = {"random": 100.0 * base, "offset_1e4": 1e4 + base, "offset_-1000": -1000.0 + 0.25 * base}[case].astype(np.float32)
    vol[1, 3, 4, :5] = np.nan
    mask = U.random_mask(shape, seed=13, keep=0.8)
    depth = U.sum_depth([shape])
    worst = {}
    for m in (None, mask):
        got = {k: host(v) for k, v in table_of(dev(vol), None if m is None else dev(m)).items()}
        for k in range(2):
            mem = U.members(vol[k], m)
            ref, bound = U.moments(mem), U.moments_bound(mem, depth)
            assert got["n"][k] == ref["n"] and got["n_nan"][k] == U.count_nan(vol[k], m)
            assert got["min"][k] == ref["min"] and got["max"][k] == ref["max"]
            for f in ("mean", "std"):
                err = abs(float(got[f][k]) - ref[f])
                worst[f] = max(worst.get(f, 0.0), err / bound[f])
                assert err <= bound[f], (case, f, err, bound[f])
    print(f"moments[{case}]: largest fraction of the bound: mean {worst['mean']:.3f}, std {worst['std']:.3f} (depth {depth})")


def test_results_are_bit_identical_across_runs():
    vol, mask = dev(volume("air60", 3, TWO_ROWS, "f32", seed=14)), dev(U.random_mask(TWO_ROWS, seed=15))
    runs = []
    for _ in range(2):
        s = M.intensity_stats(vol, mask)
        runs.append([host(getattr(s, f)) for f in s.FIELDS] + [host(M.ZScore(mask=mask)(vol)), host(M.Rescale()(vol))])
    for a, b in zip(*runs):
        assert same_bits(a, b)


# ---------------------------------------------------------------------------------------------- 3. parameters and apply
def test_ranks_percentiles_and_tables_equal_their_fp64_restatement():
    qs, eps = (0.5, 99.5, 50.0, 37.25), 1e-8
    for name, shape in (("air60", TWO_ROWS), ("nans", ONE), ("constant", ONE)):
        vol = volume(name, 2, shape, "f32", seed=16)
        mask = U.random_mask(shape, seed=17)
        cases = M._cases(dev(vol), dev(mask), "test")
        table = M._moments(cases)
        ranks, frac = M._ranks(table, qs)
        order, counts = M._select(cases, ranks)
        f = {k: host(v) for k, v in M._table_fields(table).items()}
        for scheme, code in (("zscore", L.INTENSITY_ZSCORE), ("ct", L.INTENSITY_CT), ("rescale", L.INTENSITY_RESCALE)):
            params, pct = M._params(code, table, order, frac, len(qs), 2, eps, DEV, want_pct=True)
            for k in range(2):
                m = U.sorted_members(vol[k], mask)
                exp_rank = [r for q in qs for r in U.percentile_ranks(q, len(m))[:2]]
                assert list(host(ranks)[k]) == exp_rank and list(host(counts)[k]) == [len(m), U.count_nan(vol[k], mask)]
                assert same_bits(host(frac)[k], np.array([U.percentile_ranks(q, len(m))[2] for q in qs]))
                want_pct, want_order, _ = U.percentiles_of(m, qs)
                assert U.same_values(host(order)[k].reshape(-1, 2), want_order) and same_bits(host(pct)[k], want_pct)
                want = U.apply_table(scheme, float(f["mean"][k]), float(f["std"][k]), want_pct[0], want_pct[1], eps)
                assert same_bits(host(params)[k], want), (name, scheme, host(params)[k], want)
    # eps takes over where std (or the span) is below it
    flat = M._cases(dev(np.full((1,) + ONE, 5.0, np.float32)), None, "test")
    t = M._moments(flat)
    rk, fr = M._ranks(t, (0.5, 99.5))
    od, _ = M._select(flat, rk)
    assert same_bits(host(M._params(L.INTENSITY_ZSCORE, t, None, None, 0, 1, 0.5, DEV)[0]), U.apply_table("zscore", 5.0, 0.0, 0, 0, 0.5)[None])
    assert same_bits(host(M._params(L.INTENSITY_RESCALE, None, od, fr, 2, 1, 0.25, DEV)[0]), U.apply_table("rescale", 0, 0, 5.0, 5.0, 0.25)[None])


APPLY_TABLES = {
    # (lo, hi, sub, mul) per channel: clipping that lands exactly on values of the data; an infinite lo / hi; f16 results that are
    # subnormal (mul 2^-20) or overflow to inf (mul 2^12)
    "window": [[-3.5, 3.5, 0.25, 1.5], [1.0, 65504.0, -2.0, 0.125]],
    "open": [[-math.inf, 1.0, 0.5, 3.0], [-1.0, math.inf, 7.0, -0.75]],
    "tiny": [[-100.0, 100.0, 1.0, 2.0 ** -20], [-math.inf, math.inf, 3.0, 2.0 ** -22]],
    "huge": [[-1000.0, 1000.0, -1.0, 2.0 ** 12], [-2.0, 2.0, 1.0, 1e5]],
}


@pytest.mark.parametrize("dt", list(TORCH_DT))
@pytest.mark.parametrize("shape", [ONE, TWO_ROWS])
def test_apply_equals_the_fp32_restatement_bit_for_bit(dt, shape):
    mask = U.random_mask(shape, seed=18, keep=0.7)
    seen = set()
    for name in ("mixed", "full_range", "nans"):
        vol = volume(name, 2, shape, dt, seed=19)
        for tname, rows in APPLY_TABLES.items():
            table = np.array(rows, dtype=np.float32)
            for out_dt, np_dt in ((torch.float32, np.float32), (torch.float16, np.float16)):
                for m, fill in ((None, 0.0), (mask, -7.5)):
                    want = U.apply(vol, table, np_dt, m, fill)
                    got = M.apply_table(dev(vol), dev(table), None if m is None else odd_view(m), fill, out_dt)
                    assert same_bits(host(got), want), (name, tname, out_dt, m is not None)
                    if TORCH_DT[dt] == out_dt:             # in place
                        src = dev(vol)
                        back = M.apply_table(src, dev(table), None if m is None else dev(m), fill, out=src)
                        assert back.data_ptr() == src.data_ptr() and same_bits(host(src), want)
                    if m is not None:
                        outside = np.broadcast_to((m == 0)[None], vol.shape) | np.isnan(vol.astype(np.float32))
                        assert (host(got)[outside] == np_dt(fill)).all()
                    if np_dt == np.float16:
                        a = np.abs(want.astype(np.float32))
                        seen.update(["subnormal"] if ((a > 0) & (a < 2.0 ** -14)).any() else [])
                        seen.update(["inf"] if np.isinf(want[np.isfinite(vol.astype(np.float32))]).any() else [])
    assert seen == {"subnormal", "inf"}, seen


def test_clipping_lands_exactly_on_lo_and_hi():
    x = np.array([-5.0, -3.5, np.nextafter(np.float32(-3.5), np.float32(0)), 0.0, 3.5, np.nextafter(np.float32(3.5), np.float32(9)), np.inf,
                  -np.inf, np.nan, 1.0], dtype=np.float32).reshape(1, 1, 2, 5)
    table = np.array([[-3.5, 3.5, -3.5, 1.0]], dtype=np.float32)
    got = host(M.apply_table(dev(x), dev(table), None, 9.0, torch.float32)).reshape(-1)
    assert list(got) == [0.0, 0.0, float(np.float32(np.nextafter(np.float32(-3.5), np.float32(0))) + np.float32(3.5)), 3.5, 7.0, 7.0, 7.0, 0.0, 9.0, 4.5]


# ---------------------------------------------------------------------------------------------- 4. schemes end to end
def test_zscore_over_the_nonzero_mask():
    vol = volume("air60", 2, TWO_ROWS, "f32", seed=21)
    vol[vol == -1024.0] = 0.0
    vol[1, 2, 3, 4] = np.nan                       # non-zero for the mask, no member, filled
    nz = (vol != 0).any(axis=0).astype(np.uint8)
    stats = M.intensity_stats(dev(vol), "nonzero").to_host()
    table = np.stack([U.apply_table("zscore", float(stats.mean[k]), float(stats.std[k]), 0, 0, 1e-8) for k in range(2)])
    for k in range(2):
        ref = U.moments(U.members(vol[k], nz))
        assert int(stats.n[k]) == ref["n"] and abs(float(stats.mean[k]) - ref["mean"]) <= 1e-9 * abs(ref["mean"])
    for dtype, np_dt in ((torch.float16, np.float16), (torch.float32, np.float32)):
        got = M.ZScore(mask="nonzero", fill=-1.0, dtype=dtype)(dev(vol))
        assert same_bits(host(got), U.apply(vol, table, np_dt, nz, -1.0)) and bool(torch.isfinite(got).all())
    plain = M.normalize(dev(vol[0]), M.ZScore(dtype=torch.float32))         # D x H x W in, D x H x W out, every voxel
    s0 = M.intensity_stats(dev(vol[0])).to_host()
    t0 = U.apply_table("zscore", float(s0.mean[0]), float(s0.std[0]), 0, 0, 1e-8)[None]
    assert tuple(plain.shape) == TWO_ROWS and same_bits(host(plain), U.apply(vol[:1], t0, np.float32)[0])


def test_ct_window_from_a_pooled_fingerprint():
    shapes = [TWO_ROWS, (9, 10, 11), ONE]
    vols = [U.hostile("air60", s, "i16", seed=22 + k)[None] for k, s in enumerate(shapes)]
    labels = [U.random_mask(s, seed=25 + k, keep=0.3) * 2 for k, s in enumerate(shapes)]
    stats = M.intensity_stats([dev(v) for v in vols], masks=[dev(lab) > 0 for lab in labels])
    m = U.sorted_members([(v[0], lab) for v, lab in zip(vols, labels)])
    pct, _, _ = U.percentiles_of(m, (0.5, 99.5))
    s = stats.to_host()
    assert int(s.n[0]) == len(m) and same_bits(host(s.percentiles[0]), pct)
    ct = M.CTWindow.from_stats(stats, channel=0)
    table = U.apply_table("ct", float(s.mean[0]), float(s.std[0]), pct[0], pct[1], 1e-8)[None]
    assert same_bits(ct.table().numpy(), table)
    for v in vols:
        assert same_bits(host(ct(dev(v))), U.apply(v, table, np.float16))
    out = torch.empty(vols[0].shape, dtype=torch.float32, device=DEV)
    assert M.normalize(dev(vols[0]), ct, out=out) is out and same_bits(host(out), U.apply(vols[0], table, np.float32))


def test_rescale():
    vol = volume("air60", 2, TWO_ROWS, "f32", seed=28)
    vol[vol == -1024.0] = 0.0
    nz = (vol != 0).any(axis=0).astype(np.uint8)
    for mask, m_np in ((None, None), ("nonzero", nz)):
        rows = []
        for k in range(2):
            pct, _, _ = U.percentiles_of(U.sorted_members(vol[k], m_np), (0.5, 99.5))
            rows.append(U.apply_table("rescale", 0, 0, pct[0], pct[1], 1e-8))
        got = M.Rescale(mask=mask, dtype=torch.float32)(dev(vol))
        want = U.apply(vol, np.stack(rows), np.float32, m_np, 0.0)
        assert same_bits(host(got), want) and float(got.min()) == 0.0 and float(got.max()) <= 1.0 + 1e-6


# ---------------------------------------------------------------------------------------------- 5. mask and box
@pytest.mark.parametrize("dt", list(TORCH_DT))
@pytest.mark.parametrize("shape", [TWO_ROWS, (18, 20, 14)])       # scalar; d h w % 4 == 0: four voxels per thread, one 32-bit store
def test_nonzero_mask_and_box(dt, shape):
    vol = np.zeros((2,) + shape, U.NP_DT[dt])
    cases = [("all zero", [], (0, 0, 0, -1, -1, -1)), ("one voxel", [(1, 16, 0, 12)], (16, 0, 12, 16, 0, 12)),
             ("two channels", [(0, 2, 5, 3), (1, 9, 18, 0), (0, 4, 4, 4)], (2, 4, 0, 9, 18, 4))]
    for what, points, box in cases:
        v = vol.copy()
        for p in points:
            v[p] = 3
        mask, got = M.nonzero_mask(dev(v), return_box=True)
        want = (v != 0).any(axis=0)
        assert mask.dtype == torch.uint8 and np.array_equal(host(mask), want.astype(np.uint8)), what
        assert got.dtype == torch.int32 and tuple(host(got)) == box, what
        if points:
            idx = np.argwhere(want)
            assert tuple(idx.min(0)) + tuple(idx.max(0)) == box
    if dt in ("f32", "f16"):
        v = vol.copy()
        v[0, 1, 2, 3], v[1, 3, 2, 1] = np.nan, -0.0
        mask, got = M.nonzero_mask(dev(v), return_box=True)
        assert int(mask.sum()) == 1 and tuple(host(got)) == (1, 2, 3, 1, 2, 3)        # NaN is non-zero, -0.0 is zero
    big = U.hostile("air60", shape, dt, seed=29)
    values, counts = np.unique(big, return_counts=True)
    big[big == values[np.argmax(counts)]] = 0                   # the air becomes the background
    assert np.array_equal(host(M.nonzero_mask(dev(big))), (big != 0).astype(np.uint8))


def test_crop_to_nonzero():
    shape = (9, 10, 11)
    vol = np.zeros((2,) + shape, np.float32)
    vol[0, 2:5, 3:9, 1:4] = 1.0
    vol[1, 6, 3, 9] = -2.0
    t, lab = dev(vol), dev(np.arange(np.prod(shape), dtype=np.int64).reshape(shape))
    cv, cl, box = M.crop_to_nonzero(t, lab)
    assert box == (2, 3, 1, 6, 8, 9) and tuple(cv.shape) == (2, 5, 6, 9) and tuple(cl.shape) == (5, 6, 9)
    assert cv.data_ptr() == t[:, 2:, 3:, 1:].data_ptr() and torch.equal(cl, lab[2:7, 3:9, 1:10])          # views
    cv, box = M.crop_to_nonzero(t, margin=3)
    assert box == (0, 0, 0, 8, 9, 10) and tuple(cv.shape) == (2,) + shape                                # clamped at the border
    cv, box = M.crop_to_nonzero(t, margin=1)
    assert box == (1, 2, 0, 7, 9, 10)
    cv, box = M.crop_to_nonzero(torch.zeros_like(t))
    assert box == (0, 0, 0, 8, 9, 10) and tuple(cv.shape) == (2,) + shape                                # all zero: the whole volume


# ---------------------------------------------------------------------------------------------- 6. footprint
@pytest.mark.parametrize("dt", list(TORCH_DT))
def test_in_guard_bands(dt):
    """Every source (with a uint8 mask that ends at the guard), every output, the tables and the workspaces (exactly as large as the
    queries answer) in guarded slabs: the exact checks still pass and no guard byte changes."""
    for shape in (ONE, TWO_ROWS):
        vol = volume("nans" if dt in ("f32", "f16") else "air60", 3, shape, dt, seed=31)
        mask = U.random_mask(shape, seed=32)
        with Fence() as fence:
            tv, tm = check_select(vol, mask, put=lambda a: fence.put(dev(a)), put_mask=lambda a: fence.put(dev(a)))
            src, m = tv[0], tm[0]
            stats = M.intensity_stats(src, m)
            nz, box = M.nonzero_mask(src, return_box=True)
            z = M.ZScore(mask=m, fill=2.0)(src)
            r = M.Rescale(dtype=torch.float32)(src)
            table = fence.put(dev(np.array(APPLY_TABLES["window"] + [[-1.0, 1.0, 0.0, 2.0]], dtype=np.float32)))
            a = M.apply_table(src, table, m, 1.0, torch.float32)
            quad = fence.put(dev(volume("air60", 2, (6, 6, 7), dt, seed=33)))            # 252 voxels: the four-wide mask kernel
            nz4, box4 = M.nonzero_mask(quad, return_box=True)
            for t in (stats.n, stats.mean, stats.percentiles, stats.order, stats.frac, nz, box, z, r, a, nz4, box4):
                assert fence.owns(t)
            lib = L.lib()
            assert {rq[0] for rq in fence.ws_requests} <= {lib.mednet_intensity_select_ws_bytes(3, k) for k in (4, 8)} | \
                {lib.mednet_intensity_moments_ws_bytes(3, *shape)}
            assert all(rq[0] == rq[1] for rq in fence.ws_requests) and len(fence.ws_requests) >= 5
            fence.check()
        s = stats.to_host()
        for k in range(3):
            mem = U.sorted_members(vol[k], mask)
            assert int(s.n[k]) == len(mem) and same_bits(host(s.percentiles[k]), U.percentiles_of(mem, (0.5, 99.5))[0])
        assert np.array_equal(host(nz), (np.nan_to_num(vol.astype(np.float32), nan=1.0) != 0).any(axis=0).astype(np.uint8))
        want4 = (host(quad) != 0).any(axis=0)
        idx = np.argwhere(want4)
        assert np.array_equal(host(nz4), want4.astype(np.uint8)) and tuple(host(box4)) == tuple(idx.min(0)) + tuple(idx.max(0))
        zt = np.stack([U.apply_table("zscore", float(s.mean[k]), float(s.std[k]), 0, 0, 1e-8) for k in range(3)])
        assert same_bits(host(z), U.apply(vol, zt, np.float16, mask, 2.0))
        assert same_bits(host(a), U.apply(vol, host(table), np.float32, mask, 1.0))
        rt = np.stack([U.apply_table("rescale", 0, 0, *U.percentiles_of(U.sorted_members(vol[k]), (0.5, 99.5))[0], 1e-8) for k in range(3)])
        assert same_bits(host(r), U.apply(vol, rt, np.float32))


# ---------------------------------------------------------------------------------------------- 7. the predictor
def test_predictor_normalises_at_the_native_grid_first():
    shape, patch, ov, nh, ncls = (40, 36, 44), (32, 32, 32), (4, 4, 4), 1, 3
    rng = np.random.default_rng(41)
    ct_vol = np.where(rng.random((1,) + shape) < 0.55, -1024, rng.normal(60, 200, (1,) + shape)).astype(np.int16)
    mr_vol = (rng.standard_normal((1,) + shape) * 50 + 300).astype(np.float32)
    with mednet_hip.precision("fp32"):
        net = O.keyed_init_(HM.ResidualUNet3D(in_channels=1, out_channels=nh + ncls, final_sigmoid=False, f_maps=[8])).to(DEV).eval()
        kw = dict(num_heatmaps=nh, pad_mode="symmetric", batch_size=3, blend="gaussian")
        for vol, scheme in ((ct_vol, M.CTWindow(-900.0, 400.0, 50.0, 180.0)), (ct_vol, M.Rescale()), (mr_vol, M.ZScore(mask="nonzero"))):
            for extra, call in ((dict(), dict()), (dict(target_spacing=(1, 1, 1)), dict(spacing=(2, 1, 1)))):
                with_scheme = HP.GridPredictor(net, patch, ov, normalize=scheme, **extra, **kw).predict(vol, **call)
                by_hand = HP.GridPredictor(net, patch, ov, **extra, **kw).predict(scheme(dev(vol)), **call)
                assert type(with_scheme) is type(by_hand) and same_bits(host(with_scheme.acc), host(by_hand.acc))
                res = with_scheme.result()
                assert tuple(res.shape) == (nh + 1,) + shape and torch.equal(res, by_hand.result())
        # normalize=None: the predictor of today
        a = HP.GridPredictor(net, patch, ov, normalize=None, **kw).predict(mr_vol)
        b = HP.GridPredictor(net, patch, ov, **kw).predict(mr_vol)
        assert same_bits(host(a.acc), host(b.acc)) and torch.equal(a.result(), b.result())
        # the crop-stitch path takes the scheme too
        s = M.ZScore()
        assert torch.equal(HP.GridPredictor(net, patch, ov, num_heatmaps=nh, normalize=s)(mr_vol),
                           HP.GridPredictor(net, patch, ov, num_heatmaps=nh)(s(dev(mr_vol))))
