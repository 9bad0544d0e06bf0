"""tests/degrade_util.py on the CPU: the model of csrc/degrade.hip meets its known answers and scipy, and every checker rejects the
fault it is there for."""
import numpy as np
import pytest
from scipy import ndimage

import degrade_util as D
import resample_util as R

MOMENT_SEED = 0x5EEDC0FFEE123457      # chosen here on the CPU: the model alone passes check_moments with it
MOMENT_VOXELS = 1 << 18


def test_philox_known_answers():
    for counter, key, want in D.KNOWN_ANSWERS:
        got = tuple(int(v) for v in D.philox4x32(counter, key))
        assert got == want, (counter, key, [hex(v) for v in got])
    # an array of counters equals the scalar calls
    r = D.philox4x32((np.arange(5, dtype=np.uint64), 3, 0, 0), (7, 9))
    for j in range(5):
        assert tuple(int(v[j]) for v in r) == tuple(int(v) for v in D.philox4x32((j, 3, 0, 0), (7, 9)))


@pytest.mark.parametrize("shape", [(5, 6, 7), (9, 10, 33)])
@pytest.mark.parametrize("sigma", [0.5, 1.0, 1.5])
def test_fp64_blur_equals_scipy(shape, sigma):
    """To 1e-12 of the volume's largest magnitude; (5, 6, 7) with sigma 1.5 has n = 5 <= r = 6 and n = 6 <= r on two axes."""
    x = np.random.default_rng(3).standard_normal(shape)
    tables = [D.model_blur_table(n, sigma, exact=True) for n in shape]
    if shape == (5, 6, 7) and sigma == 1.5:
        assert shape[0] <= (tables[0][3] - 1) // 2 and shape[1] <= (tables[1][3] - 1) // 2
    want = ndimage.gaussian_filter(x, sigma, mode="reflect", truncate=4.0)
    assert np.abs(D.filter64(x, tables) - want).max() <= 1e-12 * np.abs(x).max()
    # the library's weights are these rounded once to fp32: three passes, one rounding of a weight each
    rounded = [D.model_blur_table(n, sigma) for n in shape]
    assert all(np.array_equal(r[2], t[2].astype(np.float32)) for r, t in zip(rounded, tables))
    assert np.abs(D.filter64(x, rounded) - want).max() <= 3 * 2.0 ** -24 * np.abs(x).max()


def test_reflect_is_scipys_and_the_library_tables_equal_the_model():
    from mednet_hip import sampler as HS
    for n in (1, 2, 5, 33):
        x = np.arange(n, dtype=np.float64)
        padded = np.pad(x, 3 * n, mode="symmetric")
        for j in range(-3 * n, 4 * n):
            assert D.reflect(j, n) == int(padded[j + 3 * n]) == int(HS._reflect(np.asarray(j), n))
    for n, sigma in ((5, 1.5), (33, 0.5), (7, 1.0), (64, 0.73)):
        a, b = HS.blur_table(n, sigma), D.model_blur_table(n, sigma)
        assert a[3] == b[3] and all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3])), (n, sigma)
    for n, zoom in ((9, 0.5), (10, 0.73), (33, 0.99), (33, 0.5), (128, 0.61)):
        a, b = HS.low_resolution_table(n, zoom), D.model_low_resolution_table(n, zoom)
        if D.low_resolution_size(n, zoom) == n:
            assert a is None
            continue
        assert a[3] == b[3] and all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3])), (n, zoom)
    assert HS.blur_table(9, 0.0) is None and HS.low_resolution_table(9, 1.0) is None and HS.low_resolution_table(9, 1.7) is None


@pytest.mark.parametrize("zoom", [0.5, 0.73, 0.99])
def test_composite_table_equals_nearest_then_cubic_bit_for_bit(zoom):
    shape = (9, 10, 33)
    x = R.random_volume(5, shape)
    for axis, n in enumerate(shape):
        m = D.low_resolution_size(n, zoom)
        two = R.pass32(R.pass32(x, axis, R.model_table(n, m, "nearest")), axis, R.model_table(m, n, "cubic"))
        one = D.pass32(x, axis, D.model_low_resolution_table(n, zoom))
        assert np.array_equal(D.bits(one), D.bits(two)), (axis, zoom)
    # ... and the three composite passes equal "down-sample nearest on every axis, then three cubic passes"
    size = tuple(D.low_resolution_size(n, zoom) for n in shape)
    low = R.resample32(x, R.tables_for(shape, size, "nearest"))
    want = R.resample32(low, R.tables_for(size, shape, "cubic"))
    got = D.filter32(x, [D.model_low_resolution_table(n, zoom) for n in shape])
    assert np.array_equal(D.bits(got), D.bits(want))


def test_model_normals_are_normal():
    z, rad = D.normals64(MOMENT_SEED, 0, MOMENT_VOXELS)
    mean, var, p = D.check_moments(z, "model")
    print(f"[measure] mean={mean:.3e} var={var:.6f} ks_p={p:.3f}")
    assert np.isfinite(rad).all()


@pytest.mark.parametrize("fault", [f for f in D.NOISE_FAULTS if f])
def test_noise_checker_rejects(fault):
    z, rad = D.normals64(MOMENT_SEED, 2, 1 << 14)
    D.check_noise(z.astype(np.float32), z, rad, "model")
    bad, _ = D.normals64(MOMENT_SEED, 2, 1 << 14, fault=fault)
    with pytest.raises(AssertionError):
        D.check_noise(np.nan_to_num(bad, posinf=3e38).astype(np.float32), z, rad, fault)
    if fault == "u1_zero":      # the range itself: a word below 2^8 gives u1 = 0
        D.check_uniforms(*D.uniforms([0, 0xFFFFFFFF], [0, 0xFFFFFFFF]), "model")
        with pytest.raises(AssertionError):
            D.check_uniforms(*D.uniforms([0, 0xFFFFFFFF], [0, 0xFFFFFFFF], fault=fault), fault)


@pytest.mark.parametrize("fault", [f for f in D.TABLE_FAULTS if f])
def test_blur_checker_rejects(fault):
    shape, sigma = (5, 6, 7), 1.0
    x = R.random_volume(7, shape) + 2.0
    tables = [D.model_blur_table(n, sigma) for n in shape]
    ref, bound = D.filter64(x, tables), D.error_bound(x, tables)
    D.check_bounded(D.filter32(x, tables), ref, bound, "model")
    with pytest.raises(AssertionError):
        D.check_bounded(D.filter32(x, [D.model_blur_table(n, sigma, fault=fault) for n in shape]), ref, bound, fault)


def test_low_resolution_checker_rejects_a_shifted_table():
    shape, zoom = (9, 10, 33), 0.73
    x = R.random_volume(8, shape)
    want = D.filter32(x, [D.model_low_resolution_table(n, zoom) for n in shape])
    D.check_exact(want, want.copy(), "model")
    with pytest.raises(AssertionError):
        D.check_exact(D.filter32(x, [D.model_low_resolution_table(n, zoom, fault="shift") for n in shape]), want, "shift")


def test_dyadic_tables_are_exact_and_show_a_read_past_count():
    n, taps = 12, 13
    t = D.dyadic_table(1, n, taps, descending=True)
    assert (np.diff(t[1][0]) <= 0).all() and t[0].min() == 1 and t[0].max() == taps
    live = np.arange(taps)[None, :] < t[0][:, None]
    assert np.array_equal(np.where(live, t[2], 0).sum(1), np.ones(n)) and (t[2][~live] == 1000).all()
    x = R.integer_volume(2, (3, n, 5))
    assert np.array_equal(D.pass32(x, 1, t).astype(np.float64), D.pass64(x, 1, t))
    loose = (np.minimum(t[0] + 1, taps).astype(np.int32), t[1], t[2], taps)
    with pytest.raises(AssertionError):
        D.check_exact(D.pass32(x, 1, loose), D.pass64(x, 1, t), "count + 1")
