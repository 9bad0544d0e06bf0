"""A numpy restatement of mednet_hip.components and metrics.lesion_detection that imports nothing of the code under test.

Components: a union-find over the explicit list of neighbour pairs, each pair formed from COORDINATES (a neighbour exists only where
z + dz, y + dy, x + dx all lie inside the volume), hooked larger root under smaller root and compressed until no pair disagrees.  The
root of a component is then its smallest linear index = its first voxel in raster order (z, y, x; x fastest), and the components
are numbered in the order of their roots.  That is scipy.ndimage.label's numbering (tests/test_components_util.py checks it).

`fault=` injects one mistake, so that a test can show its comparison rejects it:
    xwrap        neighbours along x are taken on the linear index: (z, y, w - 1) touches (z, y + 1, 0)
    ywrap        the same across y to z
    18as26       connectivity 18 treated as 26
    26as6        connectivity 26 treated as 6
    rootindex    components numbered by root index + 1, without compaction
    tie_larger   keep_largest: a tie goes to the larger id
    strict       remove_small: > instead of >=
    border_hole  fill_holes: a hole that touches the border is filled too
    all_joins    the all-values labelling joins neighbours of different values
"""
import itertools

import numpy as np

FAULTS = ("xwrap", "ywrap", "18as26", "26as6", "rootindex", "tie_larger", "strict", "border_hole", "all_joins")
COLUMNS = 11  # count, zmin, zmax, ymin, ymax, xmin, xmax, sum z, sum y, sum x, value


def foreground_key(vol, cls=None, invert=False):
    """0 on background, else what two connected voxels must agree in: the value for cls=None, 1 for (vol == cls) != invert."""
    vol = np.asarray(vol, dtype=np.uint8)
    if cls is None:
        assert not invert
        return vol.astype(np.int64)
    return ((vol == cls) != bool(invert)).astype(np.int64)


def earlier_offsets(connectivity):
    """The neighbours that come first in raster order: 3 / 9 / 13 of them."""
    axes = {6: 1, 18: 2, 26: 3}[connectivity]
    offs = [o for o in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(c != 0 for c in o) <= axes and o < (0, 0, 0)]
    assert len(offs) == {6: 3, 18: 9, 26: 13}[connectivity]
    return offs


def label(vol, cls=None, connectivity=26, invert=False, fault=None):
    """-> (int32 labels of vol's shape, K)."""
    assert fault is None or fault in FAULTS
    if fault == "18as26" and connectivity == 18:
        connectivity = 26
    if fault == "26as6" and connectivity == 26:
        connectivity = 6
    key = foreground_key(vol, cls, invert)
    if fault == "all_joins" and cls is None:
        key = (key != 0).astype(np.int64)
    d, h, w = key.shape
    n = d * h * w
    flat = key.reshape(-1)
    z, y, x = (a.reshape(-1) for a in np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij"))
    v = np.arange(n)
    ea, eb = [], []
    for dz, dy, dx in earlier_offsets(connectivity):
        ok = (z + dz >= 0) & (z + dz < d)
        if fault != "ywrap":
            ok &= (y + dy >= 0) & (y + dy < h)
        if fault != "xwrap":
            ok &= (x + dx >= 0) & (x + dx < w)
        nb = v + (dz * h + dy) * w + dx
        ok &= (nb >= 0) & (nb < n)
        a, b = v[ok], nb[ok]
        same = (flat[a] != 0) & (flat[a] == flat[b])
        ea.append(a[same])
        eb.append(b[same])
    a, b = np.concatenate(ea), np.concatenate(eb)
    parent = np.arange(n)
    while True:
        pa, pb = parent[a], parent[b]
        differ = pa != pb
        if not differ.any():
            break
        np.minimum.at(parent, np.maximum(pa, pb)[differ], np.minimum(pa, pb)[differ])
        while True:
            nxt = parent[parent]
            if (nxt == parent).all():
                break
            parent = nxt
    fg = flat != 0
    roots = fg & (parent == v)
    k = int(roots.sum())
    if fault == "rootindex":
        out = np.where(fg, parent + 1, 0)
    else:
        rank = np.cumsum(roots) - 1
        out = np.where(fg, rank[parent] + 1, 0)
    return out.astype(np.int32).reshape(d, h, w), k


def stats(vol, labels, k):
    """int64 [k, 11]: count, zmin, zmax, ymin, ymax, xmin, xmax, sum z, sum y, sum x, value."""
    vol, labels = np.asarray(vol), np.asarray(labels)
    table = np.zeros((k, COLUMNS), dtype=np.int64)
    zz, yy, xx = np.nonzero(labels)
    ids = labels[zz, yy, xx].astype(np.int64) - 1
    table[:, 0] = np.bincount(ids, minlength=k)
    for c, coord in ((1, zz), (3, yy), (5, xx)):
        lo = np.full(k, np.iinfo(np.int64).max)
        hi = np.full(k, -1, dtype=np.int64)
        np.minimum.at(lo, ids, coord)
        np.maximum.at(hi, ids, coord)
        table[:, c], table[:, c + 1] = lo, hi
    for c, coord in ((7, zz), (8, yy), (9, xx)):
        table[:, c] = np.bincount(ids, weights=coord, minlength=k).astype(np.int64)
    table[ids, 10] = vol[zz, yy, xx]
    return table


def select(vol, labels, keep, fill):
    vol, labels = np.asarray(vol), np.asarray(labels)
    return np.where((labels > 0) & ~np.asarray(keep, dtype=bool)[labels], np.uint8(fill), vol).astype(np.uint8)


def keep_largest(vol, classes, connectivity=26, fault=None):
    labels, k = label(vol, None, connectivity, fault=fault)
    table = stats(vol, labels, k)
    keep = np.ones(k + 1, dtype=bool)
    for c in classes:
        ids = np.nonzero(table[:, 10] == c)[0]
        if ids.size == 0:
            continue
        counts = table[ids, 0]
        order = ids[::-1] if fault == "tie_larger" else ids
        best = order[np.argmax(table[order, 0])]     # argmax returns the first maximum
        assert table[best, 0] == counts.max()
        keep[ids + 1] = False
        keep[best + 1] = True
    return select(vol, labels, keep, 0)


def remove_small(vol, classes, min_voxels=None, min_volume=None, spacing=(1, 1, 1), connectivity=26, fault=None):
    assert (min_voxels is None) != (min_volume is None)
    labels, k = label(vol, None, connectivity, fault=fault)
    table = stats(vol, labels, k)
    size = table[:, 0] if min_voxels is not None else table[:, 0].astype(np.float64) * (float(spacing[0]) * float(spacing[1]) * float(spacing[2]))
    threshold = min_voxels if min_voxels is not None else float(min_volume)
    big = size > threshold if fault == "strict" else size >= threshold
    keep = np.ones(k + 1, dtype=bool)
    keep[1:] = ~np.isin(table[:, 10], list(classes)) | big
    return select(vol, labels, keep, 0)


def fill_holes(vol, cls, fault=None):
    labels, k = label(vol, cls, 6, invert=True, fault=fault)
    t = stats(vol, labels, k)
    d, h, w = np.asarray(vol).shape
    border = (t[:, 1] == 0) | (t[:, 2] == d - 1) | (t[:, 3] == 0) | (t[:, 4] == h - 1) | (t[:, 5] == 0) | (t[:, 6] == w - 1)
    keep = np.ones(k + 1, dtype=bool)
    keep[1:] = False if fault == "border_hole" else border
    return select(vol, labels, keep, cls)


def postprocess(vol, keep_largest_classes=(), min_voxels=None, fill_holes_classes=(), connectivity=26):
    """remove-small, then keep-largest, then fill-holes."""
    out = np.asarray(vol, dtype=np.uint8).copy()
    for c, nmin in (min_voxels or {}).items():
        out = remove_small(out, (c,), min_voxels=nmin, connectivity=connectivity)
    if keep_largest_classes:
        out = keep_largest(out, keep_largest_classes, connectivity)
    for c in fill_holes_classes:
        out = fill_holes(out, c)
    return out


def lesion_detection(pred, label_vol, cls, connectivity=26, min_overlap=1):
    """-> dict of the six counts and three ratios (NaN for a zero denominator)."""
    lp, kp = label(pred, cls, connectivity)
    lg, kg = label(label_vol, cls, connectivity)
    both = (lp > 0) & (lg > 0)
    pairs, shared = np.unique(np.stack((lp[both], lg[both]), axis=1), axis=0, return_counts=True) if both.any() else \
        (np.zeros((0, 2), dtype=np.int64), np.zeros((0,), dtype=np.int64))
    pairs = pairs[shared >= min_overlap]
    tp_label, tp_pred = len(set(pairs[:, 1].tolist())), len(set(pairs[:, 0].tolist()))
    with np.errstate(invalid="ignore", divide="ignore"):
        sens = np.float64(tp_label) / np.float64(kg)
        prec = np.float64(tp_pred) / np.float64(kp)
        f1 = 2.0 * sens * prec / (sens + prec)
    return dict(n_label=kg, n_pred=kp, tp_label=tp_label, fn=kg - tp_label, fp=kp - tp_pred, tp_pred=tp_pred, sensitivity=float(sens),
                precision=float(prec), f1=float(f1))


# ------------------------------------------------------------------------------------------------------- shapes the tests share
def serpentine(shape):
    """Alternate full x-rows of every z-plane joined at alternating ends, planes joined at alternating corners: ONE component under
    every connectivity that visits every part of the volume; its root is voxel 0."""
    d, h, w = shape
    vol = np.zeros(shape, dtype=np.uint8)
    for z in range(d):
        vol[z, 0::2, :] = 1
        for i, y in enumerate(range(1, h, 2)):
            vol[z, y, (w - 1) if i % 2 == 0 else 0] = 1
    return vol


def spiral(shape):
    """(1, h, w): a one-voxel-wide rectangular spiral with a one-voxel gap between its arms, walked inwards from the LAST voxel of
    the volume: one component under every connectivity, whose rows are joined only through the arms' far ends."""
    _, h, w = shape
    plane = np.zeros((h, w), dtype=np.uint8)
    inside = lambda p, q: 0 <= p < h and 0 <= q < w
    y, x, dy, dx = 0, 0, 0, 1
    plane[y, x] = 1
    while True:
        for _ in range(2):
            ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(ny, nx) and not plane[ny, nx] and not (inside(fy, fx) and plane[fy, fx]):
                break
            dy, dx = dx, -dy
        else:
            break
        y, x = ny, nx
        plane[y, x] = 1
    return plane[::-1, ::-1].copy().reshape(1, h, w)


def checkerboard(shape):
    z, y, x = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")
    return ((z + y + x) % 2 == 0).astype(np.uint8)


def random_volume(shape, density, seed, classes=1):
    rng = np.random.default_rng(seed)
    vol = (rng.random(shape) < density).astype(np.uint8)
    if classes > 1:
        vol *= rng.integers(1, classes + 1, size=shape, dtype=np.uint8)
    return vol


def blobs(shape, seed, classes=3, count=12, radius=(1, 4)):
    """A volume of `count` random boxes with values 1 .. classes on background 0: components of several sizes per class."""
    rng = np.random.default_rng(seed)
    vol = np.zeros(shape, dtype=np.uint8)
    for _ in range(count):
        c = [int(rng.integers(0, s)) for s in shape]
        r = [int(rng.integers(radius[0], radius[1] + 1)) for _ in shape]
        sl = tuple(slice(max(ci - ri, 0), ci + ri + 1) for ci, ri in zip(c, r))
        vol[sl] = int(rng.integers(1, classes + 1))
    return vol
