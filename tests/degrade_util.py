"""A numpy model of csrc/degrade.hip and of the degradation half of mednet_hip/sampler.py: philox4x32-10 in uint64 arithmetic, the
Box-Muller normals in fp64 from the same integers, the blur and low-resolution tables restated independently of sampler.py, a pass
in fp64 and one in the kernels' fp32 association (the emulation of tests/resample_util.py, with an explicit index per tap), and the
checkers of tests/test_gpu_degrade.py.  tests/test_degrade_util.py runs all of it on the CPU and shows that every checker rejects the
fault it is there for (`fault=`).

A table of one axis of extent n is (count int32 [n], index int32 [n][taps], weight fp32 [n][taps], taps)."""
import math

import numpy as np

import resample_util as R

U32 = R.U32
MASK = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
NOISE_FAULTS = (None, "rounds", "key_swap", "lane_order", "u1_zero")
TABLE_FAULTS = (None, "edge", "unnormalised", "shift")
NOISE_K = 8             # profiles/degrade_bounds.md: the bound of a normal is NOISE_K * 2^-24 * rad (measured ratio 3.21, doubled, next power of two)

# the three known answers of philox4x32-10: (counter, key, output)
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


# ---------------------------------------------------------------------------------------------- noise
def philox4x32(counter, key, rounds=10):
    """counter: four arrays (or ints) of 32-bit values, key: two ints -> four uint64 arrays of 32-bit values.  Every product of two
    32-bit numbers fits uint64."""
    c = [np.asarray(v, dtype=np.uint64) for v in np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in counter])]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(rounds):
        p0, p1 = PHILOX_M0 * c[0], PHILOX_M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + PHILOX_W0) & MASK, (k1 + PHILOX_W1) & MASK
    return c


def uniforms(a, b, fault=None):
    """(u1, u2) in fp64 from two words; both are fp32 numbers.  fault "u1_zero": u1 without the + 1."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    top = (a >> np.uint64(8)).astype(np.float64)
    return (top + (0.0 if fault == "u1_zero" else 1.0)) * 2.0 ** -24, (b >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def normals64(seed, row, nvox, fault=None):
    """The normals of voxels 0 .. nvox - 1 of one row in fp64 -> (z [nvox], rad [nvox]).  Faults: "rounds" (nine), "key_swap" (the
    seed's words exchanged), "lane_order" (sine on the even lane), "u1_zero"."""
    assert fault in NOISE_FAULTS
    seed = int(seed)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    if fault == "key_swap":
        key = key[::-1]
    nblk = (nvox + 3) // 4
    r = philox4x32((np.arange(nblk, dtype=np.uint64), int(row), 0, 0), key, rounds=9 if fault == "rounds" else 10)
    z, rad = np.empty((nblk, 4)), np.empty((nblk, 4))
    for pair in (0, 1):
        u1, u2 = uniforms(r[2 * pair], r[2 * pair + 1], fault)
        with np.errstate(divide="ignore"):
            rd = np.sqrt(-2.0 * np.log(u1))
        even, odd = rd * np.cos(2.0 * np.pi * u2), rd * np.sin(2.0 * np.pi * u2)
        if fault == "lane_order":
            even, odd = odd, even
        z[:, 2 * pair], z[:, 2 * pair + 1] = even, odd
        rad[:, 2 * pair] = rad[:, 2 * pair + 1] = rd
    return z.reshape(-1)[:nvox], rad.reshape(-1)[:nvox]


def check_uniforms(u1, u2, what):
    """u1 in (0, 1] (the logarithm is finite), u2 in [0, 1)."""
    u1, u2 = np.asarray(u1), np.asarray(u2)
    assert (u1 > 0).all() and (u1 <= 1).all(), f"{what}: u1 outside (0, 1]: min {u1.min()!r} max {u1.max()!r}"
    assert (u2 >= 0).all() and (u2 < 1).all(), f"{what}: u2 outside [0, 1)"


def check_noise(got, z64, rad64, what, k=NOISE_K):
    """Every element, no NaN: |got - z64| <= k * 2^-24 * rad.  -> the largest observed |got - z64| / (2^-24 * rad)."""
    got, z64, rad64 = np.asarray(got, dtype=np.float64), np.asarray(z64), np.asarray(rad64)
    assert got.shape == z64.shape == rad64.shape, f"{what}: shapes {got.shape} / {z64.shape}"
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} non-finite elements"
    assert np.isfinite(z64).all(), f"{what}: the model is not finite"
    diff, unit = np.abs(got - z64), U32 * rad64
    bad = diff > k * unit
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {got.size} normals outside {k} * 2^-24 * rad; first at {int(np.flatnonzero(bad)[0])}: "
                           f"got {got[bad][0]!r} want {z64[bad][0]!r}")
    live = unit > 0
    return float((diff[live] / unit[live]).max()) if live.any() else 0.0


def check_moments(z, what):
    """Mean within 5 / sqrt(N) of 0, variance within 5 sqrt(2 / N) of 1, Kolmogorov-Smirnov p-value above 1e-3."""
    from scipy import stats
    z = np.asarray(z, dtype=np.float64)
    n = z.size
    mean, var = float(z.mean()), float(z.var())
    assert abs(mean) <= 5.0 / math.sqrt(n), f"{what}: mean {mean:.3e}"
    assert abs(var - 1.0) <= 5.0 * math.sqrt(2.0 / n), f"{what}: variance {var:.6f}"
    p = float(stats.kstest(z, "norm").pvalue)
    assert p > 1e-3, f"{what}: Kolmogorov-Smirnov p-value {p:.3e}"
    return mean, var, p


# ---------------------------------------------------------------------------------------------- tables
def reflect(j, n):
    """d c b a | a b c d | d c b a, by folding until the index is inside."""
    while j < 0 or j >= n:
        j = -j - 1 if j < 0 else 2 * n - 1 - j
    return j


def model_blur_table(n, sigma, fault=None, exact=False):
    """Tap by tap in Python floats.  Faults: "edge" (the index is clamped instead of reflected), "unnormalised" (the weights are not
    divided by their sum), "shift" (every index one too far).  exact: the weights stay fp64 (the comparison with scipy); otherwise
    they are rounded once to fp32, as the library's are."""
    assert fault in TABLE_FAULTS
    r = int(4.0 * sigma + 0.5)
    taps = 2 * r + 1
    w = [math.exp(-(k * k) / (2.0 * sigma * sigma)) for k in range(-r, r + 1)]
    total = math.fsum(w) if fault != "unnormalised" else 1.0
    weight = np.asarray([[v / total for v in w]] * n, dtype=np.float64)
    weight = weight if exact else weight.astype(np.float32)
    index = np.zeros((n, taps), dtype=np.int32)
    for i in range(n):
        for k in range(taps):
            j = i - r + k + (1 if fault == "shift" else 0)
            index[i, k] = min(max(j, 0), n - 1) if fault == "edge" else reflect(j, n)
    return np.full(n, taps, dtype=np.int32), index, weight, taps


def low_resolution_size(n, zoom):
    return max(1, int(round(n * zoom)))


def model_low_resolution_table(n, zoom, fault=None):
    """The composite of S = nearest n -> m and U = cubic m -> n from tests/resample_util.py's own tables.  Fault "shift": U's rows read
    one row of S too far."""
    assert fault in (None, "shift")
    m = low_resolution_size(n, zoom)
    s_start = R.model_table(n, m, "nearest")[0]
    u_start, u_count, u_weight, taps = R.model_table(m, n, "cubic")
    index = np.zeros((n, taps), dtype=np.int32)
    for i in range(n):
        for k in range(taps):
            index[i, k] = s_start[min(int(u_start[i]) + k + (1 if fault == "shift" else 0), m - 1)]
    return u_count.copy(), index, u_weight.copy(), taps


def contiguous_table(table, n_in):
    """A (start, count, weight, taps) table of tests/resample_util.py with its indices written out."""
    start, count, weight, taps = table
    index = np.minimum(start[:, None].astype(np.int64) + np.arange(taps)[None, :], n_in - 1).astype(np.int32)
    return count.copy(), index, weight.copy(), taps


def stack(tables):
    """Tables of one axis -> (count [T][n], index [T][n][taps], weight [T][n][taps]) padded to the longest."""
    taps = max(t[3] for t in tables)
    n = len(tables[0][0])
    count = np.stack([t[0] for t in tables]).astype(np.int32)
    index = np.zeros((len(tables), n, taps), dtype=np.int32)
    weight = np.zeros((len(tables), n, taps), dtype=np.float32)
    for k, t in enumerate(tables):
        index[k, :, :t[3]], weight[k, :, :t[3]] = t[1], t[2]
    return count, index, weight


# ---------------------------------------------------------------------------------------------- the passes
def _taps(table):
    count, index, weight, taps = table
    for k in range(taps):
        yield index[:, k].astype(np.int64), weight[:, k].astype(np.float64), k < count


def pass64(vol, axis, table, absolute=False):
    """One pass in fp64 with the fp32 table values; vol [..., D, H, W], axis within the last three.  A slot at or above count is not
    read."""
    v = np.moveaxis(np.asarray(vol, dtype=np.float64), axis - 3, -1)
    v = np.abs(v) if absolute else v
    out = np.zeros(v.shape)
    for idx, w, live in _taps(table):
        out += np.where(live, (np.abs(w) if absolute else w) * np.where(live, v[..., idx], 0.0), 0.0)
    return np.moveaxis(out, -1, axis - 3)


def pass32(vol, axis, table):
    """The kernels' association: acc = w[0] * v[0], then acc = fmaf(w[k], v[k], acc), fp32 (tests/resample_util.py's emulation)."""
    v = np.moveaxis(np.asarray(vol, dtype=np.float32), axis - 3, -1).astype(np.float64)
    acc = None
    for k, (idx, w, live) in enumerate(_taps(table)):
        with np.errstate(invalid="ignore"):
            term = w * v[..., idx]
            nxt = (term if k == 0 else term + acc.astype(np.float64)).astype(np.float32)
        acc = nxt if k == 0 else np.where(live, nxt, acc)
    return np.moveaxis(acc, -1, axis - 3)


def filter64(vol, tables, absolute=False):
    """Axis 2, then 1, then 0; tables[axis] may be None (no pass)."""
    out = np.asarray(vol, dtype=np.float64)
    for axis in (2, 1, 0):
        if tables[axis] is not None:
            out = pass64(out, axis, tables[axis], absolute)
    return np.abs(out) if absolute else out


def filter32(vol, tables):
    out = np.asarray(vol, dtype=np.float32)
    for axis in (2, 1, 0):
        if tables[axis] is not None:
            out = pass32(out, axis, tables[axis])
    return out


def error_bound(vol, tables):
    """The chain bound of resample_util.error_bound for tables with explicit indices."""
    g = 1.0
    for t in tables:
        if t is not None:
            n = int(t[3])
            g *= 1.0 + n * U32 / (1.0 - n * U32)
    return (g - 1.0) * filter64(vol, tables, absolute=True)


def rows_pass64(x, axis, row_table, tables):
    """A batch pass in fp64: x [rows, D, H, W]; a row without a table is returned as it is.  Exact on the dyadic cases."""
    out = np.array(x, dtype=np.float64)
    for r, t in enumerate(row_table):
        if 0 <= t < len(tables):
            out[r] = pass64(x[r], axis, tables[t])
    return out


# ---------------------------------------------------------------------------------------------- inputs
def dyadic_table(seed, n, taps, descending=False):
    """Ragged counts in 1 .. taps, weights multiples of 2^-6 that sum to 1 over a row's count, indices anywhere in the axis with
    repeats (descending: sorted downwards).  Slots at and above count hold a weight of 1000 and index 0: reading them shows."""
    g = np.random.default_rng(seed)
    count = g.integers(1, taps + 1, size=n).astype(np.int32)
    count[0], count[-1] = taps, 1
    index = g.integers(0, n, size=(n, taps)).astype(np.int32)
    if descending:
        index = -np.sort(-index, axis=1)
    weight = np.full((n, taps), 1000.0, dtype=np.float32)
    for i in range(n):
        units = np.bincount(g.integers(0, count[i], size=64), minlength=count[i])
        weight[i, :count[i]] = units / 64.0
        index[i, count[i]:] = 0
    return count, index, weight, taps


def nan_pattern(shape):
    """NaN payloads, -0.0, infinities and subnormals as fp32."""
    words = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x3F800000, 0x7FBFFFFF],
                     dtype=np.uint32)
    return np.resize(words, int(np.prod(shape))).reshape(shape).view(np.float32)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


check_exact, check_bounded = R.check_exact, R.check_bounded
