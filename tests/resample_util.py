"""A numpy model of mednet_hip.resample (csrc/resample.hip): the axis tables restated independently, the passes in fp64 and in the
kernels' fp32 association, the error bound of profiles/resample_bounds.md and the checkers of tests/test_gpu_resample.py.
tests/test_resample_util.py runs all of it on the CPU and shows that every checker rejects the fault it is there for (`fault=`).

fp32 chains are emulated as float32(float64(w) * float64(v) + float64(acc)): the product of two fp32 numbers is exact in fp64, the
sum is rounded to fp64 and then to fp32.  That equals one fmaf except where the fp64 sum lands on an fp32 rounding boundary (about
one step in 2^29); on the dyadic lattices every step is exact and the emulation is too."""
import math

import numpy as np

U32 = 2.0 ** -24        # unit roundoff of fp32
U16 = 2.0 ** -11        # of fp16
F16_TINY = 2.0 ** -25   # half the spacing of fp16's subnormals: the absolute error of a store below 2^-14

TABLE_FAULTS = (None, "align_corners", "renormalise", "no_stretch")


def _filter(kind, x):
    x = abs(x)
    if kind == "linear":
        return 1.0 - x if x < 1.0 else 0.0
    if x <= 1.0:
        return 1.5 * x ** 3 - 2.5 * x ** 2 + 1.0
    if x < 2.0:
        return -0.5 * x ** 3 + 2.5 * x ** 2 - 4.0 * x + 2.0
    return 0.0


def model_table(n_in, n_out, kind="linear", antialias=True, fault=None):
    """The table of one axis, tap by tap in Python floats (fp64): (start int32, count int32, weight fp32 [n_out][taps], taps).
    fault: "align_corners" (corner-aligned centres), "renormalise" (outside taps dropped, the rest renormalised), "no_stretch" (the
    anti-alias flag ignored)."""
    assert fault in TABLE_FAULTS
    scale = n_in / n_out
    rows = []
    for i in range(n_out):
        s = (i + 0.5) * scale - 0.5
        if fault == "align_corners":
            s = i * (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        if kind == "nearest":
            rows.append((min(max(math.floor(s + 0.5), 0), n_in - 1), [1.0]))
            continue
        stretch = scale if (antialias and n_in > n_out and fault != "no_stretch") else 1.0
        radius = (1.0 if kind == "linear" else 2.0) * stretch
        acc = {}
        for j in range(math.floor(s - radius), math.ceil(s + radius) + 1):
            wj = _filter(kind, (j - s) / stretch)
            if fault == "renormalise" and not 0 <= j < n_in:
                continue
            t = min(max(j, 0), n_in - 1)
            acc[t] = acc.get(t, 0.0) + wj
        idx = sorted(t for t in acc if acc[t] != 0.0)
        first, last = idx[0], idx[-1]
        w = [acc.get(t, 0.0) for t in range(first, last + 1)]
        total = math.fsum(w)
        rows.append((first, [v / total for v in w]))
    taps = max(len(w) for _, w in rows)
    start = np.array([r[0] for r in rows], dtype=np.int32)
    count = np.array([len(r[1]) for r in rows], dtype=np.int32)
    weight = np.zeros((n_out, taps), dtype=np.float32)
    for i, (_, w) in enumerate(rows):
        weight[i, :len(w)] = np.asarray(w, dtype=np.float64).astype(np.float32)
    return start, count, weight, taps


def tables_for(shape, size, kind="linear", antialias=True, fault=None):
    return [model_table(n, m, kind, antialias, fault) for n, m in zip(shape, size)]


# ---------------------------------------------------------------------------------------------- the passes
def _taps(table, n_in):
    """Per tap slot k: (source index [n_out], weight [n_out] as fp64 of the fp32 value, live [n_out])."""
    start, count, weight, taps = table
    for k in range(taps):
        yield np.minimum(start.astype(np.int64) + k, n_in - 1), weight[:, k].astype(np.float64), k < count


def pass64(vol, axis, table, absolute=False):
    """One pass in fp64 with the fp32 table values; vol [..., D, H, W], axis counts within the last three.  absolute: |w| and |v|
    (the bound's sum of absolute terms).  A voxel outside a row's count is not read."""
    v = np.moveaxis(np.asarray(vol, dtype=np.float64), axis - 3, -1)
    v = np.abs(v) if absolute else v
    out = np.zeros(v.shape[:-1] + (len(table[0]),))
    for idx, w, live in _taps(table, v.shape[-1]):
        out += np.where(live, (np.abs(w) if absolute else w) * np.where(live, v[..., idx], 0.0), 0.0)
    return np.moveaxis(out, -1, axis - 3)


def pass32(vol, axis, table):
    """One pass in the kernels' association: acc = w[0] * v[0], then acc = fmaf(w[k], v[k], acc), fp32 (see the module docstring)."""
    v = np.moveaxis(np.asarray(vol, dtype=np.float32), axis - 3, -1).astype(np.float64)
    acc = None
    for k, (idx, w, live) in enumerate(_taps(table, v.shape[-1])):
        with np.errstate(invalid="ignore"):
            term = w * v[..., idx]
            nxt = (term if k == 0 else term + acc.astype(np.float64)).astype(np.float32)
        acc = nxt if k == 0 else np.where(live, nxt, acc)
    return np.moveaxis(acc, -1, axis - 3)


def resample64(vol, tables, absolute=False):
    out = np.asarray(vol, dtype=np.float64)
    for axis in (2, 1, 0):
        out = pass64(out, axis, tables[axis], absolute)
    return out


def resample32(vol, tables, order=(2, 1, 0)):
    """order (2, 1, 0) is the kernels' (x, then y, then z); another order is the association fault."""
    out = np.asarray(vol, dtype=np.float32)
    for axis in order:
        out = pass32(out, axis, tables[axis])
    return out


def error_bound(vol, tables):
    """|fp32 result - fp64 result| <= (prod over the three axes of (1 + gamma_n) - 1) * A per element, n the axis's longest chain,
    gamma_n = n u / (1 - n u), u = 2^-24, A the three passes run on |v| with |w| (profiles/resample_bounds.md)."""
    g = 1.0
    for t in tables:
        n = int(t[3])
        g *= 1.0 + n * U32 / (1.0 - n * U32)
    return (g - 1.0) * resample64(vol, tables, absolute=True)


# ---------------------------------------------------------------------------------------------- stores
def store_u8(x):
    """fminf(fmaxf(x, 0), 255), rintf (nearest-even; np.rint is)."""
    return np.rint(np.clip(np.asarray(x, dtype=np.float32), 0.0, 255.0)).astype(np.uint8)


def store_f16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16)


# ---------------------------------------------------------------------------------------------- arg-max
def argmax_first(scores, fault=None):
    """First maximum over axis 0 (the lowest class on ties); fault "highest": the last one."""
    s = np.asarray(scores)
    if fault == "highest":
        return (s.shape[0] - 1 - np.argmax(s[::-1], axis=0)).astype(np.uint8)
    return np.argmax(s, axis=0).astype(np.uint8)


def one_hot(labels, ncls, dtype=np.float32):
    """[ncls, D, H, W]: label == c ? 1 : 0 (a label >= ncls scores for nobody)."""
    return (np.asarray(labels)[None] == np.arange(ncls).reshape(-1, 1, 1, 1)).astype(dtype)


# ---------------------------------------------------------------------------------------------- checkers
def check_bounded(got, ref64, bound, what, rel=0.0, absolute=0.0):
    """Every element, no NaN: |got - ref64| <= bound + rel * (|ref64| + bound) + absolute (rel / absolute: the store's own
    rounding).  -> the largest observed fraction of the allowance."""
    got, ref64, bound = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert got.shape == ref64.shape == bound.shape, f"{what}: shapes {got.shape} / {ref64.shape} / {bound.shape}"
    assert not np.isnan(got).any(), f"{what}: {int(np.isnan(got).sum())} NaN"
    allow = bound + rel * (np.abs(ref64) + bound) + absolute
    diff = np.abs(got - ref64)
    bad = diff > allow
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {got.size} elements outside the bound; first at {tuple(np.argwhere(bad)[0])}: "
                           f"got {got[bad][0]!r} want {ref64[bad][0]!r} allowed {allow[bad][0]:.3e}")
    live = allow > 0
    return float((diff[live] / allow[live]).max()) if live.any() else 0.0


def check_exact(got, want, what):
    """Bit-for-bit numeric equality of every element, no NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = ~(got.astype(np.float64) == want.astype(np.float64))
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {got.size} elements differ; first at {tuple(np.argwhere(bad)[0])}: "
                           f"got {got[bad][0]!r} want {want[bad][0]!r}")


def check_argmax(got, scores64, bounds, what, max_excluded=0.05):
    """got uint8 [D, H, W] against the fp64 scores [ncls, D, H, W]: equal wherever the fp64 margin between the two best classes
    exceeds the sum of their error bounds (`bounds` like scores64, or 0 for the dyadic cases: then every voxel is compared and a tie
    goes to the lowest class).  The share of voxels left out is asserted to be at most max_excluded BEFORE anything is compared.
    -> that share."""
    s = np.asarray(scores64, dtype=np.float64)
    b = np.broadcast_to(np.asarray(bounds, dtype=np.float64), s.shape)
    want = argmax_first(s)
    if s.shape[0] == 1:
        decided = np.ones(want.shape, dtype=bool)
    else:
        order = np.argsort(-s, axis=0, kind="stable")[:2]
        top = np.take_along_axis(s, order, axis=0)
        tb = np.take_along_axis(b, order, axis=0)
        decided = (top[0] - top[1] > tb[0] + tb[1]) | ((tb[0] + tb[1]) == 0)
    share = 1.0 - float(decided.mean())
    assert share <= max_excluded, f"{what}: {share:.2%} of the voxels lie within the bound of a tie (at most {max_excluded:.0%})"
    bad = decided & (np.asarray(got) != want)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {int(decided.sum())} decided voxels differ; first at {tuple(np.argwhere(bad)[0])}: "
                           f"got {np.asarray(got)[bad][0]} want {want[bad][0]}")
    return share


# ---------------------------------------------------------------------------------------------- inputs
def integer_volume(seed, shape, lo=-512, hi=512):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=shape).astype(np.float32)


def random_volume(seed, shape, dtype="f32"):
    g = np.random.default_rng(seed)
    if dtype == "u8":
        return g.integers(0, 256, size=shape).astype(np.uint8)
    v = g.standard_normal(shape).astype(np.float32)
    return v.astype(np.float16) if dtype == "f16" else v


def softmax_planes(seed, ncls, shape):
    g = np.random.default_rng(seed)
    z = 2.0 * g.standard_normal((ncls,) + tuple(shape))
    e = np.exp(z - z.max(0, keepdims=True))
    return (e / e.sum(0, keepdims=True)).astype(np.float32)


def blob_labels(seed, ncls, shape, special=()):
    """A label volume of smooth blobs (the arg-max of low-pass noise planes), values 0 .. ncls - 1; `special`: label values written
    over a few single voxels (255, a label >= ncls)."""
    g = np.random.default_rng(seed)
    n = min(ncls, 8)
    z = g.standard_normal((n,) + tuple(shape))
    for axis in (1, 2, 3):
        for _ in range(2):
            z = z + np.roll(z, 1, axis) + np.roll(z, -1, axis)
    lab = (np.argmax(z, 0) * max(1, ncls // n)).astype(np.uint8)
    for k, v in enumerate(special):
        lab.reshape(-1)[(7 + 13 * k) % lab.size] = v
    return lab
