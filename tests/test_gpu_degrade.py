"""mednet_noise_patches and mednet_filter_rows (csrc/degrade.hip), the stand-alone transforms of mednet_hip/sampler.py and
DevicePatchSampler(degrade=...) on the GPU.  Models, tables and checkers are those of tests/degrade_util.py, which
tests/test_degrade_util.py runs on the CPU with their fault models; bounds and measured values: profiles/degrade_bounds.md.

Shapes are the smallest at which each path exists: (5, 6, 7) nothing divides by 4 and 210 voxels leave a noise tail of 2; (8, 12, 64)
the four-wide path; (3, 4, 260) a line past 256 threads with w % 4 == 0.  rows = 3: one identity row and two rows with different
tables."""
import numpy as np
import pytest
import torch

from mednet_hip import _lib as L
from mednet_hip import resample as HR
from mednet_hip import sampler as HS

import degrade_index_sweep as DS
import degrade_util as D
import resample_util as R
import warp_index_sweep as S
from fence import Fence
from gpu_util import DEV

pytestmark = pytest.mark.gpu

SHAPES = [(5, 6, 7), (8, 12, 64), (3, 4, 260)]
TAPS = (1, 4, 13, 64)
NOISE_VOXELS = (210, 4 * 256 * 3 + 4, 1)
SEED = 0x0123456789ABCDEF


def dev(a, put=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return put(t) if put else t


def run_filter(x, axis, row_table, tables, put=None, fill=np.nan):
    """x [rows, D, H, W] -> the pass's output as numpy; dst starts as `fill`, so an element nobody wrote shows."""
    src = dev(x[:, None], put)
    dst = dev(np.full(src.shape, fill, dtype=np.float32), put)
    count, index, weight = (dev(a, put) for a in D.stack(tables))
    HS.filter_rows(src, dst, axis, dev(np.asarray(row_table, dtype=np.int32), put), (count, index, weight))
    torch.cuda.synchronize()
    return dst.cpu().numpy()[:, 0]


# ------------------------------------------------------------------------------------------------ the filter
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_filter_exact_on_dyadic_tables(shape, axis):
    """Integers in +-512 and weights in multiples of 2^-6 that sum to 1: every step is exact, so every element equals numpy's.
    Ragged counts, repeated and descending indices; slots past count hold a weight of 1000."""
    n = shape[axis]
    x = R.integer_volume(10 + axis, (3,) + shape)
    for taps in TAPS:
        tables = [D.dyadic_table(100 + taps, n, taps), D.dyadic_table(200 + taps, n, taps, descending=True)]
        row_table = [1, -1, 0]
        got = run_filter(x, axis, row_table, tables)
        D.check_exact(got, D.rows_pass64(x, axis, row_table, tables), f"{shape} axis {axis} taps {taps}")


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_filter_equals_resample_axis_on_a_contiguous_table(shape, axis):
    """Device against device with the same chain: random data, index = start + k, n_out = n."""
    n, taps = shape[axis], 5
    g = np.random.default_rng(40 + axis)
    start = np.clip(np.arange(n) - 2 + g.integers(-1, 2, size=n), 0, n - 1).astype(np.int32)
    count = g.integers(1, taps + 1, size=n).astype(np.int32)
    weight = g.standard_normal((n, taps)).astype(np.float32)
    x = R.random_volume(41, (3,) + shape)
    want = HR.resample_axis(dev(x), axis, (dev(start), dev(count), dev(weight), taps))
    torch.cuda.synchronize()
    got = run_filter(x, axis, [0, -1, 0], [D.contiguous_table((start, count, weight, taps), n)])
    want = want.cpu().numpy()
    for r in (0, 2):
        assert np.array_equal(D.bits(got[r]), D.bits(want[r])), (shape, axis, r)
    assert np.array_equal(D.bits(got[1]), D.bits(x[1]))


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_filter_identity_rows_come_back_bit_for_bit(shape, axis):
    x = D.nan_pattern((3,) + shape)
    x[1] = R.integer_volume(3, shape)
    got = run_filter(x, axis, [-1, 0, -1], [D.dyadic_table(7, shape[axis], 4)], fill=0.0)
    for r in (0, 2):
        assert np.array_equal(D.bits(got[r]), D.bits(x[r])), (shape, axis, r)
    D.check_exact(got[1], D.rows_pass64(x[1:2], axis, [0], [D.dyadic_table(7, shape[axis], 4)])[0], "the row between them")


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_filter_nan_next_to_the_support_does_not_leak(shape, axis):
    """Two live taps (i, reflect(i + 1)) of four slots; the dead slots point AT the NaN plane with a weight of 1000."""
    n = shape[axis]
    p = n // 2
    index = np.array([[i, D.reflect(i + 1, n), p, p] for i in range(n)], dtype=np.int32)
    table = (np.full(n, 2, dtype=np.int32), index, np.tile(np.float32([0.5, 0.5, 1000.0, 1000.0]), (n, 1)), 4)
    x = R.integer_volume(50, (3,) + shape)
    sl = [slice(None)] * 4
    sl[1 + axis] = p
    x[tuple(sl)] = np.nan
    got = np.moveaxis(run_filter(x, axis, [0, 0, -1], [table]), 1 + axis, -1)
    want = np.moveaxis(D.rows_pass64(x, axis, [0, 0, -1], [table]), 1 + axis, -1)
    touched = np.array([p in (index[i, 0], index[i, 1]) for i in range(n)])
    assert np.isnan(got[:2][..., touched]).all() and not np.isnan(got[:2][..., ~touched]).any()
    assert np.array_equal(got[:2][..., ~touched].astype(np.float64), want[:2][..., ~touched])


# ------------------------------------------------------------------------------------------------ blur and low resolution
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gaussian_blur_against_the_fp64_model(shape):
    sigma = np.array([[0.0], [0.7], [1.5]])
    x = R.random_volume(60, (3, 1) + shape) * 40 + 100
    data = dev(x)
    out = HS.gaussian_blur(data, sigma)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(D.bits(got[0]), D.bits(x[0]))                      # sigma 0: no table, the row is copied
    for r in (1, 2):
        tables = [D.model_blur_table(n, float(sigma[r, 0])) for n in shape]
        ratio = D.check_bounded(got[r, 0], D.filter64(x[r, 0], tables), D.error_bound(x[r, 0], tables), f"{shape} sigma {sigma[r, 0]}")
        print(f"[measure] blur shape={shape} sigma={sigma[r, 0]} taps={tables[0][3]} worst fraction of the bound {ratio:.3f}")
    const = np.full((1, 1) + shape, 3.25, dtype=np.float32)
    out = HS.gaussian_blur(dev(const), 1.0)
    torch.cuda.synchronize()
    tables = [D.model_blur_table(n, 1.0) for n in shape]
    D.check_bounded(out.cpu().numpy()[0, 0], D.filter64(const[0, 0], tables), D.error_bound(const[0, 0], tables), "constant volume")


def test_gaussian_blur_without_a_drawn_row_launches_nothing_and_returns_data():
    data = dev(R.random_volume(61, (2, 2, 5, 6, 7)))
    assert HS.gaussian_blur(data, 0.0) is data and HS.simulate_low_resolution(data, 1.0) is data
    assert HS.gaussian_noise_(data, np.zeros((2, 2)), 1) is data


@pytest.mark.parametrize("zoom", [0.5, 0.73, 0.99])
def test_simulate_low_resolution_equals_nearest_then_cubic_resampling(zoom):
    shape = (9, 10, 33)
    x = R.random_volume(70, (1, 1) + shape)
    out = HS.simulate_low_resolution(dev(x), zoom)
    m = tuple(D.low_resolution_size(n, zoom) for n in shape)
    want = HR.resample(HR.resample(dev(x[0]), size=m, kind="nearest"), size=shape, kind="cubic")
    torch.cuda.synchronize()
    assert np.array_equal(D.bits(out.cpu().numpy()[0]), D.bits(want.cpu().numpy())), zoom
    model = D.filter32(x[0, 0], [None if mm == n else D.model_low_resolution_table(n, zoom) for n, mm in zip(shape, m)])
    assert np.array_equal(D.bits(out.cpu().numpy()[0, 0]), D.bits(model))


# ------------------------------------------------------------------------------------------------ noise
def run_noise(x, std, seed, put=None):
    """x [rows, nvox] -> x + std * z as numpy."""
    data, sd = dev(x, put), dev(np.asarray(std, dtype=np.float32), put)
    L.check(L.lib().mednet_noise_patches(data.data_ptr(), sd.data_ptr(), seed, x.shape[0], x.shape[1], L.stream()), "noise_patches")
    torch.cuda.synchronize()
    return data.cpu().numpy()


@pytest.mark.parametrize("nvox", NOISE_VOXELS)
def test_noise_against_the_fp64_model_and_the_join(nvox):
    zero = np.zeros((3, nvox), dtype=np.float32)
    z = run_noise(zero, [1.0, 1.0, 1.0], SEED)
    worst = 0.0
    for r in range(3):
        z64, rad = D.normals64(SEED, r, nvox)
        worst = max(worst, D.check_noise(z[r], z64, rad, f"{nvox} voxels row {r}"))
    print(f"[measure] noise nvox={nvox} worst |z - z64| / (2^-24 rad) = {worst:.3f} (K = {D.NOISE_K})")
    assert np.array_equal(D.bits(run_noise(zero, [1.0, 1.0, 1.0], SEED)), D.bits(z))            # two launches, equal bits
    # the join: out == fmaf(std, z_observed, x), and the determinism with it
    x = (np.random.default_rng(80).standard_normal((3, nvox)) * 3).astype(np.float32)
    std = np.float32([0.37, 2.0, 1e-3])
    got = run_noise(x, std, SEED)
    want = (std[:, None].astype(np.float64) * z.astype(np.float64) + x.astype(np.float64)).astype(np.float32)
    assert np.array_equal(D.bits(got), D.bits(want))
    # a row's values do not depend on another row's std; a std == 0 row is neither read nor written
    mixed = D.nan_pattern((3, nvox)).copy()
    mixed[1] = 0.0
    got = run_noise(mixed, [0.0, 1.0, 0.0], SEED)
    assert np.array_equal(D.bits(got[1]), D.bits(z[1]))
    assert np.array_equal(D.bits(got[0]), D.bits(mixed[0])) and np.array_equal(D.bits(got[2]), D.bits(mixed[2]))
    # the key's high word counts
    other = run_noise(zero, [1.0, 1.0, 1.0], SEED ^ (1 << 40))
    assert not np.array_equal(D.bits(other), D.bits(z)) and (other != z).mean() > 0.99 if nvox > 1 else (other != z).all()


def test_gaussian_noise_wrapper_and_the_moments_of_the_kernel():
    nvox = 1 << 16
    data = torch.zeros((2, 2, 16, 64, 64), device=DEV)
    HS.gaussian_noise_(data, np.array([[1.0, 0.0], [0.5, 2.0]]), SEED)
    torch.cuda.synchronize()
    got = data.cpu().numpy().reshape(4, nvox)
    assert (got[1] == 0).all()
    for r, s in ((0, 1.0), (2, 0.5), (3, 2.0)):
        z64, rad = D.normals64(SEED, r, nvox)
        D.check_noise(got[r] / s, z64, rad, f"row {r}")
    D.check_moments(got[0], "kernel")
    assert HS.gaussian_noise_(torch.zeros((1, 3, 4, 4, 4), device=DEV), 0.25, 5).std() > 0      # a scalar std goes to every row


# ------------------------------------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_footprint_of_both_entries_between_guard_bands(shape):
    nvox = int(np.prod(shape))
    x = R.random_volume(90, (3, nvox))
    plain = run_noise(x, [1.0, 0.0, 0.5], SEED)
    with Fence() as fence:
        got = run_noise(x, [1.0, 0.0, 0.5], SEED, fence.put)
        fence.check()
    assert np.array_equal(D.bits(got), D.bits(plain)) and not np.isnan(got).any()
    x = R.integer_volume(91, (3,) + shape)
    for axis in (0, 1, 2):
        tables = [D.dyadic_table(300 + axis, shape[axis], 13), D.dyadic_table(400 + axis, shape[axis], 4)]
        plain = run_filter(x, axis, [0, -1, 1], tables)
        with Fence() as fence:
            got = run_filter(x, axis, [0, -1, 1], tables, fence.put)
            fence.check()
        assert np.array_equal(D.bits(got), D.bits(plain)) and not np.isnan(got).any(), (shape, axis)
        D.check_exact(got, D.rows_pass64(x, axis, [0, -1, 1], tables), f"fenced {shape} axis {axis}")


@pytest.fixture(scope="module")
def clamp_sweep_green(tmp_path_factory):
    """The host sweep of csrc/degrade_index.h (tests/degrade_index_sweep.py) in a PLAIN build, once per module.  A failure here fails
    the hostile-table cases BEFORE they launch anything; the build under the sanitizers belongs to the CPU suite alone."""
    plain = S.plain_compiler()
    assert plain is not None, "no host C++ compiler: the clamp header cannot be swept"
    DS.sweep(str(tmp_path_factory.mktemp("degrade_index")), plain, sanitize=False)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_footprint_with_hostile_tables(shape, clamp_sweep_green):
    """Indices -5 and 2^30, counts 0 and 1000, row_table 99: the output is the clamped table's, and no guard byte changes."""
    x = R.integer_volume(92, (3,) + shape)
    for axis in (0, 1, 2):
        n, taps = shape[axis], 4
        count, index, weight, _ = D.dyadic_table(500 + axis, n, taps)
        weight = np.where(np.arange(taps)[None, :] < count[:, None], weight, 0).astype(np.float32)
        weight[0], weight[-1] = [0.25] * 4, [1, 0, 0, 0]
        hostile_count, hostile_index = count.copy(), index.copy()
        hostile_count[0], hostile_count[-1] = 1000, 0                       # -> taps, 1
        hostile_index[0] = [-5, 1 << 30, 0, n - 1]                          # -> 0, n - 1, 0, n - 1
        clamped_count, clamped_index = hostile_count.copy(), hostile_index.copy()
        clamped_count[0], clamped_count[-1] = taps, 1
        clamped_index[0] = [0, n - 1, 0, n - 1]
        with Fence() as fence:
            got = run_filter(x, axis, [0, 99, -7], [(hostile_count, hostile_index, weight, taps)], fence.put)
            fence.check()
        D.check_exact(got, D.rows_pass64(x, axis, [0, -1, -1], [(clamped_count, clamped_index, weight, taps)]), f"hostile {shape} axis {axis}")


# ------------------------------------------------------------------------------------------------ the sampler
def sampler_volumes():
    rng = np.random.default_rng(31)
    shape = (20, 18, 22)
    images = [(rng.standard_normal((2,) + shape) * 40 + 100).astype(np.float16) for _ in range(2)]
    labels = [rng.integers(0, 3, (1,) + shape).astype(np.uint8) for _ in range(2)]
    return images, labels


KW = dict(samples_per_subject=2, class_probabilities=[0.2, 0.4, 0.4], device=DEV)
PATCH, INDICES = [8, 9, 12], [0, 1, 2, 3]


def replay(images, labels, batch):
    """The plain sampler's crop at the positions `batch` drew."""
    plain = HS.DevicePatchSampler(images, labels, PATCH, **KW)
    drawn = iter(zip([i % len(images) for i in INDICES], batch["patch_position"], batch["selected_class"]))
    plain.position = lambda idx: next(drawn)
    return plain.batch(INDICES)


def test_sampler_with_every_probability_one_equals_the_stand_alone_functions():
    images, labels = sampler_volumes()
    deg = HS.ImageDegradation(p_noise=1, p_blur=1, p_blur_channel=1, p_low_resolution=1, p_low_resolution_channel=1)
    ds = HS.DevicePatchSampler(images, labels, PATCH, degrade=deg, **KW)
    np.random.seed(6)
    b = ds.batch(INDICES)
    last = ds.last_degradation
    assert last["params"].shape == (4, 2, 3) and last["seed"] is not None and 0 <= last["seed"] < 2 ** 64
    assert (last["params"][:, :, 0] > 0).all() and (last["params"][:, :, 1] >= 0.5).all() and (last["params"][:, :, 2] < 1).all()
    assert set(b) == {"subject_key", "patch_position", "selected_class", "data", "label"}
    r = replay(images, labels, b)
    want = r["data"].clone()
    HS.gaussian_noise_(want, last["params"][:, :, 0], last["seed"])
    want = HS.gaussian_blur(want, last["params"][:, :, 1])
    want = HS.simulate_low_resolution(want, last["params"][:, :, 2])
    torch.cuda.synchronize()
    assert np.array_equal(D.bits(b["data"].cpu().numpy()), D.bits(want.cpu().numpy()))
    assert not torch.equal(b["data"], r["data"]) and torch.equal(b["label"], r["label"])
    assert b["data"].is_contiguous() and bool(torch.isfinite(b["data"]).all())


def test_sampler_without_degradation_is_the_parent_path():
    images, labels = sampler_volumes()
    np.random.seed(9)
    a = HS.DevicePatchSampler(images, labels, PATCH, augment=True, **KW).batch(INDICES)
    state_a = np.random.get_state()
    np.random.seed(9)
    ds = HS.DevicePatchSampler(images, labels, PATCH, augment=True, degrade=None, **KW)
    b = ds.batch(INDICES)
    state_b = np.random.get_state()
    assert torch.equal(a["data"], b["data"]) and torch.equal(a["label"], b["label"]) and ds.last_degradation is None
    assert np.array_equal(state_a[1], state_b[1]) and state_a[2:] == state_b[2:]


def test_sampler_with_probabilities_zero_changes_nothing_but_the_generator():
    images, labels = sampler_volumes()
    deg = HS.ImageDegradation(p_noise=0, p_blur=0, p_blur_channel=0, p_low_resolution=0, p_low_resolution_channel=0)
    ds = HS.DevicePatchSampler(images, labels, PATCH, degrade=deg, **KW)
    np.random.seed(12)
    b = ds.batch(INDICES)
    state = np.random.get_state()
    assert ds.last_degradation["seed"] is None
    assert np.array_equal(ds.last_degradation["params"], np.tile([0.0, 0.0, 1.0], (4, 2, 1)))
    r = replay(images, labels, b)
    assert torch.equal(b["data"], r["data"]) and torch.equal(b["label"], r["label"])
    # the generator: per sample the position's calls, then exactly calls_per_sample uniform draws; no seed draw
    plain = HS.DevicePatchSampler(images, labels, PATCH, **KW)
    np.random.seed(12)
    for k, i in enumerate(INDICES):
        _, ini, cls = plain.position(i)
        assert np.array_equal(ini, b["patch_position"][k]) and int(cls) == int(b["selected_class"][k])
        for _ in range(deg.calls_per_sample(2)):
            np.random.uniform()
    again = np.random.get_state()
    assert np.array_equal(state[1], again[1]) and state[2:] == again[2:]
