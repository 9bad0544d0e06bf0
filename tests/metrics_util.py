"""The numpy restatement of case-level evaluation (mednet_hip.metrics, csrc/metrics.hip) and the checkers of
tests/test_gpu_metrics.py.  Nothing here imports the code under test.  tests/test_metrics_util.py holds the restatement to scipy and
to known answers and shows that every checker rejects the fault it is there for; profiles/case_metrics_bounds.md derives the bounds.

  confusion_ref            numpy.bincount
  surface_ref              pad and shift: the voxels of the class with a face neighbour that differs or lies outside
  edt_sq_ref               brute force over all seed points in fp64, with the fp32-rounded spacing
  surface_distances_ref    the metrics from the two explicit point sets

`fault=` injects the mistakes the checkers must catch (None: the restatement itself)."""
import types

import numpy as np

U32 = 2.0 ** -24                         # one fp32 rounding
EDT_REL = (1.0 + U32) ** 4 - 1.0         # general spacing: the transform against fp64, per element, relative
PCT_REL = 5.0 * U32 + 2.0 ** -40         # the interpolated percentile against fp64, relative to the larger order statistic
FAULTS = ("skip_axis", "cityblock", "conn26", "border", "transpose", "nearest")


def f32_spacing(spacing):
    """The spacing as the kernels receive it: fp32 numbers, here as Python floats."""
    return tuple(float(np.float32(s)) for s in spacing)


# ------------------------------------------------------------------------------------------------------- confusion, overlap
def confusion_ref(pred, label, ncls, ignore_index=None, fault=None):
    """-> (int64 [ncls, ncls] with [l, p] = voxels of label l predicted as p, voxels left out because either is >= ncls).  Voxels whose
    label equals ignore_index are counted nowhere."""
    p, l = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(label).reshape(-1).astype(np.int64)
    if ignore_index is not None:
        keep = l != ignore_index
        p, l = p[keep], l[keep]
    ok = (l >= 0) & (l < ncls) & (p >= 0) & (p < ncls)
    cm = np.bincount(l[ok] * ncls + p[ok], minlength=ncls * ncls).reshape(ncls, ncls).astype(np.int64)
    if fault == "transpose":
        cm = cm.T.copy()
    return cm, int((~ok).sum())


def overlap_ref(cm):
    """fp64 from the integer counts -> dict of dice, iou, sensitivity, precision (NaN for a zero denominator), volume_pred,
    volume_label."""
    cm = np.asarray(cm, dtype=np.int64)
    tp, vl, vp = np.diag(cm).astype(np.float64), cm.sum(1), cm.sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(dice=2.0 * tp / (vp + vl), iou=tp / (vp + vl - tp), sensitivity=tp / vl, precision=tp / vp, volume_pred=vp,
                    volume_label=vl)


# ------------------------------------------------------------------------------------------------------- surface mask
FACES = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))


def surface_ref(vol, cls, fault=None):
    """uint8: 1 where vol == cls and one of the six face neighbours is != cls or outside the volume."""
    m = np.asarray(vol) == cls
    pad = np.pad(m, 1, constant_values=(fault == "border"))     # (the fault: the outside counts as the class)
    d, h, w = m.shape
    if fault == "conn26":
        offs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
    else:
        offs = FACES
    inner = np.ones_like(m)
    for a, b, c in offs:
        inner &= pad[1 + a:1 + a + d, 1 + b:1 + b + h, 1 + c:1 + c + w]
    return (m & ~inner).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------- distances
def points(mask):
    """int64 [n, 3]: the (z, y, x) of the nonzero voxels, in memory order."""
    return np.argwhere(np.asarray(mask) != 0).astype(np.int64)


def sq_dist_to_set(at, seeds, spacing, fault=None, chunk=2048):
    """fp64 [len(at)]: min over the seed points of sum_a (spacing_a * (at_a - seed_a))^2, +inf without a seed.  Integer index
    differences, the fp32-rounded spacing, everything else in fp64."""
    sp = np.asarray(f32_spacing(spacing), dtype=np.float64)
    at, seeds = np.asarray(at, dtype=np.int64).reshape(-1, 3), np.asarray(seeds, dtype=np.int64).reshape(-1, 3)
    out = np.full(len(at), np.inf)
    if len(seeds) == 0:
        return out
    axes = (0, 1) if fault == "skip_axis" else (0, 1, 2)
    for a0 in range(0, len(at), chunk):
        blk = at[a0:a0 + chunk]
        terms = [np.abs((blk[:, None, a] - seeds[None, :, a]).astype(np.float64) * sp[a]) for a in axes]
        tot = sum(terms) ** 2 if fault == "cityblock" else sum(t * t for t in terms)
        out[a0:a0 + chunk] = tot.min(1)
    return out


def edt_sq_ref(seed, spacing=(1, 1, 1), fault=None):
    """fp64 D x H x W: the squared distance of every voxel to the nearest voxel with seed != 0."""
    seed = np.asarray(seed)
    at = np.argwhere(np.ones(seed.shape, dtype=bool))
    return sq_dist_to_set(at, points(seed), spacing, fault).reshape(seed.shape)


def surface_distances_ref(pred, label, cls, spacing=(1, 1, 1), percentile=95.0, tolerance=1.0, fault=None):
    """One class from the two explicit surface point sets, fp64.  d2_pred / d2_label: the squared distances of the prediction's
    surface voxels to the label's surface and back, in memory order; per direction the count, the count with d2 <= fp32(tol)^2, max
    d2 (-inf for none); hd, hd_percentile, assd, nsd (NaN when either surface is empty)."""
    sp = points(surface_ref(pred, cls, fault))
    sg = points(surface_ref(label, cls, fault))
    d2p, d2g = sq_dist_to_set(sp, sg, spacing, fault), sq_dist_to_set(sg, sp, spacing, fault)
    tol_sq = float(np.float32(tolerance) * np.float32(tolerance))
    n_p, n_g = len(sp), len(sg)
    within_p, within_g = int((d2p <= tol_sq).sum()), int((d2g <= tol_sq).sum())
    max_p = float(d2p.max()) if n_p else -np.inf
    max_g = float(d2g.max()) if n_g else -np.inf
    r = types.SimpleNamespace(n_pred=n_p, n_label=n_g, d2_pred=d2p, d2_label=d2g, within_pred=within_p, within_label=within_g,
                              max_d2_pred=max_p, max_d2_label=max_g, pct_pair=(np.nan, np.nan))
    if n_p == 0 or n_g == 0:
        r.hd = r.hd_percentile = r.assd = r.nsd = np.nan
        return r
    method = "nearest" if fault == "nearest" else "linear"
    r.pct_pair = (float(np.percentile(np.sqrt(d2p), percentile, method=method)), float(np.percentile(np.sqrt(d2g), percentile, method=method)))
    r.hd = float(np.sqrt(max(max_p, max_g)))
    r.hd_percentile = max(r.pct_pair)
    r.assd = float((np.sqrt(d2p).sum() + np.sqrt(d2g).sum()) / (n_p + n_g))
    r.nsd = (within_p + within_g) / (n_p + n_g)
    return r


def order_statistics(d2, percentile):
    """The two order statistics numpy's linear interpolation reads -> (sqrt of the lower, sqrt of the upper), fp64."""
    v = np.sort(np.asarray(d2, dtype=np.float64))
    pos = percentile / 100.0 * (len(v) - 1)
    lo = min(int(np.floor(pos)), len(v) - 1)
    return float(np.sqrt(v[lo])), float(np.sqrt(v[min(lo + 1, len(v) - 1)]))


# ------------------------------------------------------------------------------------------------------- scipy's path
def scipy_surface(vol, cls):
    from scipy import ndimage
    m = np.asarray(vol) == cls
    return (m & ~ndimage.binary_erosion(m, ndimage.generate_binary_structure(3, 1), border_value=0)).astype(np.uint8)


def scipy_edt_sq(seed, spacing=(1, 1, 1)):
    """distance_transform_edt measures to the nearest ZERO: the seeds go in inverted.  Without a seed scipy's answer is not +inf; the
    callers do not ask."""
    from scipy import ndimage
    return ndimage.distance_transform_edt(np.asarray(seed) == 0, sampling=f32_spacing(spacing)) ** 2


def scipy_surface_distances(pred, label, cls, spacing=(1, 1, 1), percentile=95.0, tolerance=1.0):
    """The metrics of one class the way a host evaluation takes them: two erosions, two whole-volume transforms."""
    from scipy import ndimage
    sp, sg = scipy_surface(pred, cls).astype(bool), scipy_surface(label, cls).astype(bool)
    if not sp.any() or not sg.any():
        return dict(hd=np.nan, hd_percentile=np.nan, assd=np.nan, nsd=np.nan)
    dp = ndimage.distance_transform_edt(~sg, sampling=f32_spacing(spacing))[sp]
    dg = ndimage.distance_transform_edt(~sp, sampling=f32_spacing(spacing))[sg]
    n = len(dp) + len(dg)
    tol = float(np.float32(tolerance))
    return dict(hd=float(max(dp.max(), dg.max())), hd_percentile=float(max(np.percentile(dp, percentile), np.percentile(dg, percentile))),
                assd=float((dp.sum() + dg.sum()) / n), nsd=float(((dp <= tol).sum() + (dg <= tol).sum()) / n))


# ------------------------------------------------------------------------------------------------------- inputs
def rng(tag):
    return np.random.default_rng(abs(hash_tag(tag)))


def hash_tag(tag):
    """A seed from a string, the same in every process (Python's hash() is salted)."""
    h = 2166136261
    for ch in tag.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


def random_labels(tag, shape, ncls, stray=0.0):
    """uint8 volume of classes 0 .. ncls - 1; a fraction `stray` of the voxels holds a value >= ncls."""
    g = rng(tag)
    v = g.integers(0, ncls, size=shape).astype(np.uint8)
    if stray:
        hit = g.random(shape) < stray
        v[hit] = g.integers(ncls, 256, size=shape).astype(np.uint8)[hit]
    return v


def blobs(tag, shape, ncls, shift=(0, 0, 0), jitter=0.0):
    """A label volume of ncls - 1 ellipsoids (class k centred in the k-th slab along z, so that every class has an interior and a
    surface), moved by `shift`; jitter: the fraction of voxels re-drawn at random, which roughens the surfaces."""
    g = rng(tag)
    d, h, w = shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    vol = np.zeros(shape, dtype=np.uint8)
    for k in range(1, ncls):
        c = (d * (k - 0.5) / (ncls - 1) + shift[0], h / 2 + shift[1], w / 2 + shift[2])
        r = (max(d / (2.6 * (ncls - 1)), 1.5), h / 3.2, w / 3.2)
        vol[((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 <= 1.0] = k
    if jitter:
        hit = g.random(shape) < jitter
        vol[hit] = g.integers(0, ncls, size=shape).astype(np.uint8)[hit]
    return vol


def box(shape, lo, size, cls=1):
    v = np.zeros(shape, dtype=np.uint8)
    v[lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]] = cls
    return v


# ------------------------------------------------------------------------------------------------------- checkers
def _first(bad, got, want, n=6):
    idx = np.argwhere(bad)[:n]
    return " | ".join(f"{tuple(int(k) for k in i)}: got {got[tuple(i)]!r} want {want[tuple(i)]!r}" for i in idx)


def check_equal(got, want, what):
    """Every element equal, shapes equal; NaN only where `want` has it (an unwritten fp32 element reads as NaN under the fence)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    g, w = np.atleast_1d(got), np.atleast_1d(want)
    if g.dtype.kind == "f" or w.dtype.kind == "f":
        g, w = g.astype(np.float64), w.astype(np.float64)
        bad = ~((g == w) | (np.isnan(g) & np.isnan(w)))
    else:
        bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ; first at " + _first(bad, g, w)
    return int(bad.size)


def check_edt_exact(got, ref64, what):
    """Bit equality with the fp64 restatement rounded once to fp32 -- which must not move it: the case has to be exact."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    r32 = ref64.astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), ref64), f"{what}: the reference is not exact in fp32; this is no exact case"
    got = np.asarray(got)
    assert got.dtype == np.float32, f"{what}: dtype {got.dtype}"
    return check_equal(got, r32, what)


def check_edt_bound(got, ref64, what, rel=EDT_REL):
    """|got - ref64| <= rel * ref64 in every element, inf where the reference is inf, no NaN.  -> the worst observed ratio, in
    units of 2^-24."""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    assert got.shape == ref64.shape, f"{what}: shape {got.shape} != {ref64.shape}"
    assert not np.isnan(got).any(), f"{what}: {int(np.isnan(got).sum())} NaN"
    fin = np.isfinite(ref64)
    assert np.array_equal(np.isfinite(got), fin), f"{what}: infinities differ"
    err = np.abs(got[fin] - ref64[fin])
    bad = err > rel * ref64[fin]
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements outside {rel:.3e} * ref; worst ratio " \
                          f"{float((err[bad] / ref64[fin][bad]).max()) / U32:.2f} u"
    nz = ref64[fin] > 0
    return float((err[nz] / ref64[fin][nz]).max() / U32) if nz.any() else 0.0


def check_hd(got, max_d2, what):
    """hd is the correctly rounded fp32 root of the exact max d2 (NaN for NaN)."""
    if np.isnan(max_d2):
        assert np.isnan(got), f"{what}: got {got!r}, want NaN"
        return
    want = np.float32(np.sqrt(np.float64(np.float32(max_d2))))
    assert np.float32(max_d2) == max_d2, f"{what}: max d2 {max_d2!r} is not exact in fp32"
    assert np.float32(got) == want, f"{what}: got {got!r} want {want!r}"


def check_assd(got, ref, what):
    """fp64 sum of correctly rounded fp32 roots: each term within 2^-24 of its value, (n + 2) fp64 roundings on top, and as many
    in the reference."""
    if np.isnan(ref.assd):
        assert np.isnan(got), f"{what}: got {got!r}, want NaN"
        return 0.0
    n = ref.n_pred + ref.n_label
    bound = (U32 + 2.0 * (n + 2) * 2.0 ** -53) * ref.assd
    err = abs(float(got) - ref.assd)
    assert err <= bound, f"{what}: |got - ref| = {err:.3e} > {bound:.3e} (got {got!r} want {ref.assd!r})"
    return err / (U32 * ref.assd) if ref.assd else 0.0


def check_percentile(got, ref, percentile, what):
    """The larger of the two directed percentiles.  Per direction the fp32 value is within PCT_REL * (the upper order statistic) of
    numpy's fp64 one; the maximum of two values each within its bound is within the larger bound."""
    if np.isnan(ref.hd_percentile):
        assert np.isnan(got), f"{what}: got {got!r}, want NaN"
        return 0.0
    assert not np.isnan(got), f"{what}: NaN"
    upper = max(order_statistics(ref.d2_pred, percentile)[1], order_statistics(ref.d2_label, percentile)[1])
    err = abs(float(got) - ref.hd_percentile)
    assert err <= PCT_REL * upper, f"{what}: |got - ref| = {err:.3e} > {PCT_REL * upper:.3e} (got {got!r} want {ref.hd_percentile!r})"
    return err / (U32 * upper) if upper else 0.0
