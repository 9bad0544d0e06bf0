"""The numpy restatement of tests/components_util.py, on the CPU: it equals scipy.ndimage (label, binary_fill_holes, sum /
find_objects / center_of_mass) on random volumes, it gives known answers without scipy, and every fault it can inject is rejected
by the comparison tests/test_gpu_components.py uses (equality of the whole integer array)."""
import numpy as np
import pytest

import components_util as U

CONN = (6, 18, 26)
SHAPE = (33, 34, 65)


def two(shape, a, b):
    vol = np.zeros(shape, dtype=np.uint8)
    vol[a] = vol[b] = 1
    return vol


# ---------------------------------------------------------------------------------------------- against scipy
@pytest.mark.parametrize("conn", CONN)
def test_labels_equal_scipy(conn):
    ndi = pytest.importorskip("scipy.ndimage")
    st = ndi.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn])
    for density in (0.05, 0.31, 0.9):
        vol = U.random_volume(SHAPE, density, seed=conn)
        got, k = U.label(vol, 1, conn)
        want, kw = ndi.label(vol == 1, st)
        assert k == kw and np.array_equal(got, want), (conn, density)
        got, k = U.label(vol, 1, conn, invert=True)
        want, kw = ndi.label(vol != 1, st)
        assert k == kw and np.array_equal(got, want), (conn, density, "invert")
    multi = U.random_volume((9, 17, 70), 0.6, seed=3, classes=5)
    got, k = U.label(multi, None, conn)
    # every value on its own, then renumbered by first voxel
    parts = [ndi.label(multi == c, st)[0] for c in range(1, 6)]
    first = {}
    for c, lab in enumerate(parts):
        for i in range(1, lab.max() + 1):
            first[(c, i)] = np.flatnonzero(lab.reshape(-1) == i)[0]
    order = sorted(first, key=first.get)
    want = np.zeros_like(got)
    for new, (c, i) in enumerate(order, 1):
        want[parts[c] == i] = new
    assert k == len(order) and np.array_equal(got, want)


def test_table_and_fill_holes_equal_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    vol = U.random_volume((9, 17, 70), 0.2, seed=5, classes=3)
    lab, k = U.label(vol, None, 26)
    t = U.stats(vol, lab, k)
    idx = np.arange(1, k + 1)
    assert np.array_equal(t[:, 0], ndi.sum(np.ones_like(lab), lab, idx).astype(np.int64))
    for i, sl in enumerate(ndi.find_objects(lab)):
        assert [t[i, 1], t[i, 2] + 1, t[i, 3], t[i, 4] + 1, t[i, 5], t[i, 6] + 1] == [sl[0].start, sl[0].stop, sl[1].start, sl[1].stop,
                                                                                    sl[2].start, sl[2].stop]
    com = np.asarray(ndi.center_of_mass(np.ones_like(lab), lab, idx))
    assert np.allclose(t[:, 7:10] / t[:, :1], com, rtol=1e-12, atol=0)
    assert np.array_equal(t[:, 10], ndi.maximum(vol, lab, idx).astype(np.int64))
    for seed in range(4):
        v = U.random_volume((7, 9, 11), 0.55, seed=seed)
        want = np.where(ndi.binary_fill_holes(v == 1), 1, v).astype(np.uint8)
        assert np.array_equal(U.fill_holes(v, 1), want), seed


# ---------------------------------------------------------------------------------------------- known answers
def test_known_answers():
    shape = (3, 4, 5)
    face, edge, corner = two(shape, (1, 1, 1), (1, 1, 2)), two(shape, (1, 1, 1), (1, 2, 2)), two(shape, (1, 1, 1), (2, 2, 2))
    for vol, counts in ((face, (1, 1, 1)), (edge, (2, 1, 1)), (corner, (2, 2, 1))):
        assert tuple(U.label(vol, 1, c)[1] for c in CONN) == counts
    cb = U.checkerboard((6, 7, 9))
    assert U.label(cb, 1, 6)[1] == int(cb.sum()) and U.label(cb, 1, 26)[1] == 1
    for a, b in (((0, 0, 4), (0, 1, 0)), ((0, 3, 2), (1, 0, 2)), ((0, 3, 4), (1, 0, 0)), ((1, 3, 4), (2, 0, 0)), ((0, 1, 4), (0, 2, 0))):
        for c in CONN:
            assert U.label(two(shape, a, b), 1, c)[1] == 2, (a, b, c)
    for shape in ((1, 33, 70), (9, 17, 70)):
        s = U.serpentine(shape)
        for c in CONN:
            lab, k = U.label(s, 1, c)
            assert k == 1 and np.array_equal(lab, s.astype(np.int32))
    sp = U.spiral((1, 21, 37))
    assert sp[0, -1, -1] == 1 and all(U.label(sp, 1, c)[1] == 1 for c in CONN) and 0.4 < sp.mean() < 0.6
    lab, k = U.label(np.array([[[0, 2, 2, 1, 0, 1]]], dtype=np.uint8), None, 6)
    assert k == 3 and lab.tolist() == [[[0, 1, 1, 2, 0, 3]]]
    t = U.stats(np.array([[[0, 2, 2, 1, 0, 1]]], dtype=np.uint8), lab, k)
    assert t.tolist() == [[2, 0, 0, 0, 0, 1, 2, 0, 0, 3, 2], [1, 0, 0, 0, 0, 3, 3, 0, 0, 3, 1], [1, 0, 0, 0, 0, 5, 5, 0, 0, 5, 1]]


def filter_cases():
    tie = np.zeros((3, 5, 9), dtype=np.uint8)
    tie[0, 0, 0:3] = 1
    tie[2, 4, 5:8] = 1          # two components of 3 voxels: the first one stays
    tie[1, 2, 2:4] = 1
    tie[0, 4, :] = 2
    tie[2, 0, 0] = 2
    hole = np.zeros((7, 7, 9), dtype=np.uint8)
    hole[1:6, 1:6, 1:8] = 1
    hole[3, 3, 2:4] = 0          # a closed hole
    hole[3, 3, 5] = 3            # another class inside
    hole[2, 2, 6] = 0
    hole[1, 1, 7] = 0            # (2, 2, 6) touches the outside only through the corner (1, 1, 7): it is a hole under 6
    hole[4, 4, 1:4] = 0          # open to the outside through x = 1 .. 0
    hole[4, 4, 0] = 0
    opened = np.zeros((5, 5, 5), dtype=np.uint8)
    opened[0:4, 1:4, 1:4] = 1
    opened[0:2, 2, 2] = 0        # a cavity that reaches the face z = 0 through one voxel
    return tie, hole, opened


def test_filters_known_answers():
    tie, hole, opened = filter_cases()
    kept = U.keep_largest(tie, (1, 2, 7), 26)
    want = tie.copy()
    want[2, 4, 5:8] = 0
    want[1, 2, 2:4] = 0
    want[2, 0, 0] = 0
    assert np.array_equal(kept, want)
    assert np.array_equal(U.remove_small(tie, (1,), min_voxels=3), np.where((tie == 1) & (np.arange(9) >= 2)[None, None] & (np.arange(5) == 2)[None, :, None], 0, tie))
    assert np.array_equal(U.remove_small(tie, (1,), min_voxels=4), np.where(tie == 1, 0, tie))
    vv = 3.0 * 0.7 * 0.7
    assert np.array_equal(U.remove_small(tie, (1,), min_volume=3 * vv, spacing=(3.0, 0.7, 0.7)), U.remove_small(tie, (1,), min_voxels=3))
    filled = U.fill_holes(hole, 1)
    want = hole.copy()
    want[3, 3, 2:4] = 1
    want[3, 3, 5] = 1
    want[2, 2, 6] = 1
    assert np.array_equal(filled, want)
    assert np.array_equal(U.fill_holes(opened, 1), opened)
    pp = U.postprocess(tie, keep_largest_classes=(2,), min_voxels={1: 3}, fill_holes_classes=())
    want = tie.copy()
    want[1, 2, 2:4] = 0
    want[2, 0, 0] = 0
    assert np.array_equal(pp, want)


def test_detection_known_answers():
    nan = float("nan")
    shape = (4, 6, 12)
    lab = np.zeros(shape, dtype=np.uint8)
    lab[1, 1, 1:3] = 1
    lab[1, 1, 5:7] = 1
    pred = np.zeros(shape, dtype=np.uint8)
    pred[1, 1, 1:7] = 1                                # one blob over two lesions
    r = U.lesion_detection(pred, lab, 1)
    assert (r["n_label"], r["n_pred"], r["tp_label"], r["fn"], r["fp"], r["tp_pred"]) == (2, 1, 2, 0, 0, 1) and r["f1"] == 1.0
    pred = np.zeros(shape, dtype=np.uint8)
    lab = np.zeros(shape, dtype=np.uint8)
    lab[2, 2, 2:9] = 1
    pred[2, 2, 2:4] = 1
    pred[2, 2, 6:8] = 1                                # two blobs on one lesion
    pred[0, 5, 10] = 1                                 # and a false positive
    r = U.lesion_detection(pred, lab, 1)
    assert (r["n_label"], r["n_pred"], r["tp_label"], r["fn"], r["fp"], r["tp_pred"]) == (1, 3, 1, 0, 1, 2)
    assert r["sensitivity"] == 1.0 and r["precision"] == 2 / 3 and abs(r["f1"] - 0.8) < 1e-15
    r = U.lesion_detection(pred, lab, 1, min_overlap=3)   # each blob shares 2 voxels: below the overlap
    assert (r["tp_label"], r["fn"], r["fp"], r["tp_pred"]) == (0, 1, 3, 0) and r["sensitivity"] == 0.0 and np.isnan(r["f1"])
    r = U.lesion_detection(np.zeros(shape, np.uint8), np.zeros(shape, np.uint8), 1)
    assert r["n_label"] == r["n_pred"] == 0 and all(np.isnan(r[k]) for k in ("sensitivity", "precision", "f1")) and nan != r["f1"]


# ---------------------------------------------------------------------------------------------- every fault is seen
def test_each_injected_fault_is_rejected():
    shape = (3, 4, 5)
    eq = np.array_equal
    xw, yw = two(shape, (0, 0, 4), (0, 1, 0)), two(shape, (0, 3, 2), (1, 0, 2))
    for c in CONN:
        assert not eq(U.label(xw, 1, c, fault="xwrap")[0], U.label(xw, 1, c)[0]), c
        assert not eq(U.label(yw, 1, c, fault="ywrap")[0], U.label(yw, 1, c)[0]), c
    corner, edge = two(shape, (1, 1, 1), (2, 2, 2)), two(shape, (1, 1, 1), (1, 2, 2))
    assert not eq(U.label(corner, 1, 18, fault="18as26")[0], U.label(corner, 1, 18)[0])
    assert not eq(U.label(edge, 1, 26, fault="26as6")[0], U.label(edge, 1, 26)[0])
    rnd = U.random_volume((5, 6, 7), 0.3, seed=1)
    assert not eq(U.label(rnd, 1, 6, fault="rootindex")[0], U.label(rnd, 1, 6)[0])
    multi = np.array([[[1, 2, 2, 0, 1]]], dtype=np.uint8)
    assert not eq(U.label(multi, None, 6, fault="all_joins")[0], U.label(multi, None, 6)[0])
    tie, hole, opened = filter_cases()
    assert not eq(U.keep_largest(tie, (1,), fault="tie_larger"), U.keep_largest(tie, (1,)))
    assert not eq(U.remove_small(tie, (1,), min_voxels=3, fault="strict"), U.remove_small(tie, (1,), min_voxels=3))
    assert not eq(U.fill_holes(opened, 1, fault="border_hole"), U.fill_holes(opened, 1))
    assert not eq(U.fill_holes(hole, 1, fault="border_hole"), U.fill_holes(hole, 1))
    # the random volumes of the GPU test see the labelling faults too
    dense = U.random_volume(SHAPE, 0.31, seed=6)
    for c, fault in ((6, "xwrap"), (6, "ywrap"), (18, "18as26"), (26, "26as6"), (26, "rootindex")):
        assert not eq(U.label(dense, 1, c, fault=fault)[0], U.label(dense, 1, c)[0]), fault
