"""A numpy model of mednet_hip.intensity (csrc/intensity.hip): the order-preserving key of fp32, the level-by-level refinement of
several ranks at once over integer histograms, the membership rule, the percentile chain, the moments, the apply table and the
apply arithmetic, the error bound of profiles/intensity_bounds.md, and the hostile inputs the CPU and GPU tests share.
tests/test_intensity_util.py runs all of it on the CPU and shows that every checker rejects the fault it is there for (`fault=`)."""
import math
from fractions import Fraction

import numpy as np

U64 = 2.0 ** -53
LEVEL_BITS = (11, 11, 10)
MAX_RANKS = 8
SCHEMES = ("zscore", "ct", "rescale")
NP_DT = {"f32": np.float32, "f16": np.float16, "i16": np.int16, "u8": np.uint8}

KEY_FAULTS = (None, "sign_magnitude", "neg_zero")
SELECT_FAULTS = (None, "short_prefix", "boundary_rank")


# ---------------------------------------------------------------------------------------------- keys and members
def key_of(x, fault=None):
    """fp32 -> uint32 whose unsigned order is the order of the values; -0.0 has +0.0's key.  fault: "sign_magnitude" (the raw bits
    with the sign bit flipped: negatives in reverse), "neg_zero" (-0.0 keeps a key of its own, below +0.0)."""
    assert fault in KEY_FAULTS
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).copy()
    if fault != "neg_zero":
        u[x == 0] = 0
    if fault == "sign_magnitude":
        return u ^ np.uint32(0x80000000)
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def value_of(key):
    key = np.asarray(key, dtype=np.uint32)
    pos = (key & np.uint32(0x80000000)) != 0
    return np.where(pos, key & np.uint32(0x7FFFFFFF), ~key).astype(np.uint32).view(np.float32)


def members(x, mask=None, fault=None):
    """The member values of ONE channel as a flat fp32 array: inside the mask and not NaN.  fault: "nan_member"."""
    v = np.asarray(x).astype(np.float32).reshape(-1)
    keep = np.ones(v.shape, bool) if mask is None else (np.asarray(mask).reshape(-1) != 0)
    if fault != "nan_member":
        keep = keep & ~np.isnan(v)
    return v[keep]


def count_nan(x, mask=None):
    v = np.asarray(x).astype(np.float32).reshape(-1)
    keep = np.ones(v.shape, bool) if mask is None else (np.asarray(mask).reshape(-1) != 0)
    return int((np.isnan(v) & keep).sum())


# ---------------------------------------------------------------------------------------------- the radix select
def radix_select(keys, ranks, fault=None):
    """uint32 keys (one or several arrays, pooled), zero-based ranks -> (keys with those ranks as uint32, valid flags), all ranks
    refined together level by level, from histograms only, as the kernels do.  fault: "short_prefix" (a level compares the
    prefix one bit short), "boundary_rank" (the walk stays in a bin whose cumulative count EQUALS the remaining rank)."""
    assert fault in SELECT_FAULTS
    pools = [np.asarray(k, dtype=np.uint32).reshape(-1) for k in (keys if isinstance(keys, (list, tuple)) else [keys])]
    n = sum(len(k) for k in pools)
    prefix = [0] * len(ranks)
    rem = [int(r) for r in ranks]
    valid = [0 <= r < n for r in rem]
    shift = 32
    for level, bits in enumerate(LEVEL_BITS):
        hs, shift = shift, shift - bits
        hists = []
        for r in range(len(ranks)):
            h = np.zeros(1 << bits, dtype=np.int64)
            for k in pools:                                     # the accumulate form: one level over every case
                if level == 0:
                    sel = k
                else:
                    cut = hs + (1 if fault == "short_prefix" else 0)
                    sel = k[(k.astype(np.uint64) >> np.uint64(cut)) == (prefix[r] >> (cut - hs))]
                h += np.bincount((sel >> np.uint32(shift)) & np.uint32((1 << bits) - 1), minlength=1 << bits)
            hists.append(h)
        for r in range(len(ranks)):
            if not valid[r]:
                continue
            cum, b = 0, 0
            while b < (1 << bits) - 1 and (cum + hists[r][b] < rem[r] if fault == "boundary_rank" else cum + hists[r][b] <= rem[r]):
                cum += int(hists[r][b])
                b += 1
            prefix[r] = (prefix[r] << bits) | b
            rem[r] -= cum
    return np.array(prefix, dtype=np.uint32), np.array(valid)


def order_statistics(x, ranks, mask=None, key_fault=None, select_fault=None, member_fault=None):
    """ONE channel (or a list of (x, mask) cases pooled) -> fp32 values with the given ranks among the members; NaN where a rank
    is outside [0, n)."""
    cases = x if isinstance(x, list) else [(x, mask)]
    keys = [key_of(members(v, m, member_fault), key_fault) for v, m in cases]
    if key_fault == "sign_magnitude":        # (its inverse)
        k, ok = radix_select(keys, ranks, select_fault)
        vals = (k ^ np.uint32(0x80000000)).view(np.float32)
    else:
        k, ok = radix_select(keys, ranks, select_fault)
        vals = value_of(k)
    return np.where(ok, vals, np.float32(np.nan)).astype(np.float32)


def sorted_members(x, mask=None):
    cases = x if isinstance(x, list) else [(x, mask)]
    return np.sort(np.concatenate([members(v, m) for v, m in cases]))


def same_values(got, want):
    """== on the values (so -0.0 equals +0.0), NaN slots in the same places."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return got.shape == want.shape and bool(np.array_equal(np.isnan(got), np.isnan(want))) and bool((got[~np.isnan(got)] == want[~np.isnan(want)]).all())


def check_ranks(n):
    """The ranks the tests ask for: {0, 1, n/2, n-2, n-1} clipped to [0, n), at most 8."""
    return sorted({min(max(r, 0), max(n - 1, 0)) for r in (0, 1, n // 2, n - 2, n - 1)})


# ---------------------------------------------------------------------------------------------- percentiles
def percentile_ranks(q, n):
    """-> (rank a, rank b, t) of percentile q among n members; n == 0: (0, 0, 0)."""
    if n <= 0:
        return 0, 0, 0.0
    pos = (np.float64(q) / np.float64(100.0)) * np.float64(n - 1)
    fl = math.floor(pos)
    lo = min(int(fl), n - 1)
    return lo, min(lo + 1, n - 1), float(pos - np.float64(fl))


def percentile_value(a, b, t, fault=None):
    """The chain of the kernels: fp64, one rounding per operation, exactly a when t == 0.  fault: "fma" (the product and the sum
    fused: one rounding)."""
    a, b, t = np.float64(np.float32(a)), np.float64(np.float32(b)), np.float64(t)
    if t == 0:
        return float(a)
    if fault == "fma":
        d = b - a
        if not (np.isfinite(a) and np.isfinite(d)):
            return float(a + d * t)
        return float(Fraction(float(a)) + Fraction(float(d)) * Fraction(float(t)))
    return float(a + (b - a) * t)


def percentile_restated(a, b, t):
    """The same in Python floats (IEEE fp64, no contraction)."""
    a, b, t = float(np.float32(a)), float(np.float32(b)), float(t)
    return a if t == 0.0 else a + (b - a) * t


def percentiles_of(sorted_vals, qs):
    """-> (fp64 values, fp32 order statistics [P][2], t [P]) from the sorted members"""
    n = len(sorted_vals)
    vals, order, fr = [], [], []
    for q in qs:
        a, b, t = percentile_ranks(q, n)
        pa, pb = (np.float32(np.nan), np.float32(np.nan)) if n == 0 else (sorted_vals[a], sorted_vals[b])
        order.append((pa, pb)), fr.append(t), vals.append(percentile_value(pa, pb, t))
    return np.array(vals, dtype=np.float64), np.array(order, dtype=np.float32).reshape(len(qs), 2), np.array(fr, dtype=np.float64)


# ---------------------------------------------------------------------------------------------- moments
def moments(m, fault=None):
    """Member values (fp32, one channel, pooled) -> dict(n, min, max, mean, std, m2) by the two-pass form with exactly rounded sums
    (math.fsum): the reference.  fault: "sumsq" (E[x^2] - mean^2 with fp64 sums)."""
    m = np.asarray(m, dtype=np.float32).astype(np.float64)
    n = len(m)
    if n == 0:
        return dict(n=0, min=np.nan, max=np.nan, mean=np.nan, std=np.nan, m2=np.nan)
    mean = math.fsum(m) / n
    if fault == "sumsq":
        m2 = float(np.sum(m * m)) - n * mean * mean
        return dict(n=n, min=m.min(), max=m.max(), mean=mean, std=math.sqrt(max(m2, 0.0) / n), m2=m2)
    m2 = math.fsum((m - mean) ** 2)
    return dict(n=n, min=m.min(), max=m.max(), mean=mean, std=math.sqrt(m2 / n), m2=m2)


def row_plan(vox):
    """volume.h: (rows, share)"""
    rows = max(1, min(2048, -(-vox // 4096)))
    return rows, -(-(-(-vox // rows)) // 256) * 256


def sum_depth(shapes):
    """An upper bound of the number of fp64 additions any one term of a moment sum goes through, for the cases `shapes` (D, H, W):
    a thread's chain over its share of a row (the 256 threads stride over head, body and tail: at most share / 256 + 8 + 2 terms),
    the workgroup tree (8), a thread's chain over the rows (at most 8), the tree over those (8), one addition per case onto the
    running sum, and the first addition onto 0."""
    worst = 0
    for s in shapes:
        rows, share = row_plan(int(np.prod(s)))
        worst = max(worst, share // 256 + 10 + 8 + -(-rows // 256) + 8)
    return worst + len(shapes) + 1


def gamma(k):
    return k * U64 / (1.0 - k * U64)


def moments_bound(m, depth):
    """Bounds on |mean^ - mean|, |m2^ - m2| and |std^ - std| of the kernels against `moments` (profiles/intensity_bounds.md), from
    the depth of the summation, the fp64 unit roundoff and the sums of |terms|.  The reference's own error (two roundings for the
    mean, a handful for std) is inside the `+ 2` / `+ 4`."""
    m = np.asarray(m, dtype=np.float32).astype(np.float64)
    n = len(m)
    ref = moments(m)
    sabs = math.fsum(np.abs(m))
    e_mean = gamma(depth + 2) * sabs / n
    grow = n * e_mean ** 2                                # sum (x - mean^)^2 = m2 + n (mean^ - mean)^2
    e_m2 = gamma(depth + 4) * (ref["m2"] + grow) + grow
    if ref["m2"] > 0:
        rel = e_m2 / ref["m2"]
        e_std = ref["std"] * (0.5 * rel * (1.0 + rel) + 4 * U64)
    else:
        e_std = math.sqrt(e_m2 / n) * (1 + 4 * U64)
    return dict(mean=e_mean, m2=e_m2, std=e_std)


# ---------------------------------------------------------------------------------------------- the table and the apply pass
def apply_table(scheme, mean, std, p_lo, p_hi, eps):
    """(lo, hi, sub, mul) as fp32, each computed in fp64 (Python floats) and rounded once."""
    assert scheme in SCHEMES
    mx = lambda v: v if v > eps else eps           # (a NaN takes eps)
    if scheme == "zscore":
        row = (-math.inf, math.inf, mean, 1.0 / mx(std))
    elif scheme == "ct":
        row = (p_lo, p_hi, mean, 1.0 / mx(std))
    else:
        row = (p_lo, p_hi, p_lo, 1.0 / mx(p_hi - p_lo))
    return np.array(row, dtype=np.float64).astype(np.float32)


def apply(x, table, dtype, mask=None, fill=0.0, fault=None):
    """x C x D x H x W (any source dtype), table fp32 C x 4 -> ((np.clip(x, lo, hi) - sub) * mul).astype(dtype) in fp32, `fill`
    outside the mask and at NaN voxels.  fault: "nan_through" (fmaxf / fminf semantics without the NaN test: a NaN comes out as lo)."""
    x = np.asarray(x).astype(np.float32)
    t = np.asarray(table, dtype=np.float32)
    lo, hi, sub, mul = (t[:, k].reshape(-1, 1, 1, 1) for k in range(4))
    with np.errstate(all="ignore"):
        if fault == "nan_through":
            clipped = np.fmin(np.fmax(x, lo), hi)
        else:
            clipped = np.minimum(np.maximum(x, lo), hi)
        y = ((clipped - sub).astype(np.float32) * mul).astype(np.float32)
        out = np.isnan(x) if fault != "nan_through" else np.zeros(x.shape, bool)
        if mask is not None:
            out = out | (np.asarray(mask) == 0)[None]
        y = np.where(out, np.float32(fill), y)
        return y.astype(dtype)


# ---------------------------------------------------------------------------------------------- hostile inputs
HOSTILE = ("constant", "air60", "last_level", "top_level", "mixed", "full_range", "nans")


def hostile(name, shape, dt="f32", seed=0):
    """A volume of `shape` in dtype `dt` ("f32", "f16", "i16", "u8").  constant: one value; air60: 60 % one value plus noise;
    last_level: values that only the last level of the select separates (f32: 1 + k 2^-23, k < 1024; f16: adjacent halves; the
    integer types: adjacent integers); top_level: values that differ in the top 11 key bits only (signed powers of 2^8 apart);
    mixed: both signs, +-0, +-inf, fp32 and f16 subnormals; full_range: the whole range of the type (int16 with -32768);
    nans: noise with NaNs sprinkled in (float types; the integer types have none and get noise)."""
    assert name in HOSTILE and dt in NP_DT
    rng = np.random.default_rng([seed, HOSTILE.index(name), list(NP_DT).index(dt)])
    n = int(np.prod(shape))
    flt = dt in ("f32", "f16")
    info = None if flt else np.iinfo(NP_DT[dt])
    if name == "constant":
        v = np.full(n, -1024.0 if dt != "u8" else 7.0)
    elif name == "air60":
        air = -1024.0 if dt != "u8" else 0.0
        noise = rng.normal(40.0, 300.0, n) if flt else rng.integers(max(info.min, -1000), min(info.max, 3000), n)
        v = np.where(rng.random(n) < 0.6, air, noise)
    elif name == "last_level":
        k = rng.integers(0, 1024, n)
        v = 1.0 + k * 2.0 ** -23 if dt == "f32" else 1.0 + (k % 64) * 2.0 ** -10 if dt == "f16" else (k % 200).astype(np.float64)
    elif name == "top_level":
        if flt:
            e = rng.integers(-1, 2, n) * 8 if dt == "f16" else rng.integers(-12, 13, n) * 8
            v = np.where(rng.random(n) < 0.5, -1.0, 1.0) * 2.0 ** e
        else:
            v = np.where(rng.random(n) < 0.5, 1.0, 0.0) * 2.0 ** rng.integers(0, 7, n)
    elif name == "mixed":
        if flt:
            pool = np.array([0.0, -0.0, np.inf, -np.inf, 2.0 ** -149, -2.0 ** -149, 2.0 ** -130, 2.0 ** -24, -2.0 ** -24, 2.0 ** -20, 1.0, -1.0,
                             65504.0, -65504.0, 3.5, -3.5, 2.0 ** -14, -2.0 ** -14])
            v =np.where(rng.random(n) < 0.5, pool[rng.integers(0, len(pool), n)], rng.normal(0, 2, n))
        else:
            v = rng.integers(max(info.min, -5), 6, n).astype(np.float64)
    elif name == "full_range":
        if flt:
            v = rng.normal(0, 1, n) * 10.0 ** rng.integers(-4, 5, n)
        else:
            v = rng.integers(info.min, info.max + 1, n).astype(np.float64)
            v[: min(n, 4)] = [info.min, info.max, info.min, 0][: min(n, 4)]
    else:
        v = rng.normal(0, 50, n)
        if flt:
            v[rng.random(n) < 0.07] = np.nan
    with np.errstate(all="ignore"):
        return v.astype(NP_DT[dt]).reshape(shape)


def random_mask(shape, seed=0, keep=0.4):
    return (np.random.default_rng([seed, 99]).random(shape) < keep).astype(np.uint8)
