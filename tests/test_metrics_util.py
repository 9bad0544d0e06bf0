"""The yardstick of tests/test_gpu_metrics.py on the CPU: the numpy restatement of tests/metrics_util.py agrees with scipy where scipy
has the operation, gives the known answers, and its checkers reject the faults they are there for -- a transform that skips an axis,
city-block distances, a 26-connected surface, volume-border voxels that are no surface, a transposed confusion matrix, a percentile
taken with method="nearest"."""
import numpy as np
import pytest

import metrics_util as M

SPACINGS = [(1, 1, 1), (2, 1, 0.5), (3.0, 0.7, 0.7)]


# ------------------------------------------------------------------------------------------------------- against scipy
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 5), (3, 4, 5), (9, 11, 13)])
def test_surface_equals_mask_minus_scipy_erosion(shape):
    pytest.importorskip("scipy")
    vol = M.random_labels(f"surf{shape}", shape, 3)
    full = np.ones(shape, dtype=np.uint8)
    for v, cls in ((vol, 0), (vol, 1), (vol, 2), (vol, 7), (full, 1), (M.blobs("b", (9, 11, 13), 3), 1)):
        assert np.array_equal(M.surface_ref(v, cls), M.scipy_surface(v, cls)), (shape, cls)


@pytest.mark.parametrize("spacing", SPACINGS)
def test_brute_force_distance_equals_scipy_edt(spacing):
    pytest.importorskip("scipy")
    g = M.rng(f"edt{spacing}")
    for shape in ((1, 1, 1), (1, 1, 9), (7, 9, 13), (9, 11, 13)):
        seed = (g.random(shape) < 0.05).astype(np.uint8)
        seed[tuple(g.integers(0, s) for s in shape)] = 1
        ref, sci = M.edt_sq_ref(seed, spacing), M.scipy_edt_sq(seed, spacing)
        assert np.allclose(ref, sci, rtol=1e-12, atol=0), (shape, float(np.abs(ref - sci).max()))


def test_surface_distances_equal_the_scipy_path():
    pytest.importorskip("scipy")
    pred, label = M.blobs("p", (12, 14, 16), 3, shift=(1, -1, 2), jitter=0.02), M.blobs("l", (12, 14, 16), 3)
    for spacing in SPACINGS:
        for cls in (1, 2):
            ref = M.surface_distances_ref(pred, label, cls, spacing, 95.0, 1.0)
            sci = M.scipy_surface_distances(pred, label, cls, spacing, 95.0, 1.0)
            for k, v in sci.items():
                assert np.isclose(getattr(ref, k), v, rtol=1e-12, atol=0), (spacing, cls, k, getattr(ref, k), v)


# ------------------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("shift", [(0, 0, 3), (2, 0, 0), (1, 2, 2), (3, 4, 0)])
@pytest.mark.parametrize("spacing", SPACINGS)
def test_shifted_boxes_have_the_shift_as_hausdorff_distance(shift, spacing):
    shape, lo, size = (16, 18, 20), (3, 4, 5), (6, 7, 8)
    a, b = M.box(shape, lo, size), M.box(shape, tuple(l + s for l, s in zip(lo, shift)), size)
    ref = M.surface_distances_ref(a, b, 1, spacing, 100.0, 0.0)
    want = float(np.sqrt(sum((s * k) ** 2 for s, k in zip(M.f32_spacing(spacing), shift))))
    assert np.isclose(ref.hd, want, rtol=1e-14) and np.isclose(ref.hd_percentile, want, rtol=1e-14), (ref.hd, want)
    assert ref.n_pred == ref.n_label == 6 * 7 * 8 - 4 * 5 * 6


def test_a_mask_against_itself_and_a_single_voxel():
    vol = M.blobs("self", (10, 12, 14), 3, jitter=0.05)
    for cls in (1, 2):
        ref = M.surface_distances_ref(vol, vol, cls, (3.0, 0.7, 0.7))
        assert ref.hd == 0 and ref.hd_percentile == 0 and ref.assd == 0 and ref.nsd == 1 and ref.n_pred == ref.n_label > 0
    cm, oor = M.confusion_ref(vol, vol, 3)
    assert oor == 0 and np.array_equal(cm, np.diag(np.bincount(vol.reshape(-1), minlength=3)))
    assert np.array_equal(M.overlap_ref(cm)["dice"], np.ones(3))
    one = M.box((5, 6, 7), (2, 3, 4), (1, 1, 1))
    assert np.array_equal(M.surface_ref(one, 1), one)
    assert M.edt_sq_ref(one, (2, 1, 0.5))[0, 0, 0] == 4.0 ** 2 + 3.0 ** 2 + 2.0 ** 2
    assert np.isinf(M.edt_sq_ref(np.zeros((2, 3, 4), dtype=np.uint8))).all()


def test_overlap_of_absent_classes_is_nan():
    cm = np.array([[5, 1, 0], [2, 3, 0], [0, 0, 0]])
    o = M.overlap_ref(cm)
    assert np.isnan(o["dice"][2]) and np.isnan(o["iou"][2]) and np.isnan(o["sensitivity"][2]) and np.isnan(o["precision"][2])
    assert o["dice"][1] == 2 * 3 / (4 + 5) and o["iou"][1] == 3 / 6 and o["sensitivity"][1] == 3 / 5 and o["precision"][1] == 3 / 4
    cm2, oor = M.confusion_ref([0, 1, 9, 1, 2], [0, 1, 1, 7, 2], 3, ignore_index=2)
    assert oor == 2 and cm2.sum() == 2 and cm2[0, 0] == 1 and cm2[1, 1] == 1


# ------------------------------------------------------------------------------------------------------- the checkers reject faults
def _case():
    pred = M.blobs("fp", (12, 14, 16), 3, shift=(1, -2, 2), jitter=0.03)
    label = M.blobs("fl", (12, 14, 16), 3, jitter=0.01)
    return pred, label


def test_exact_checker_rejects_a_skipped_axis_and_cityblock_distances():
    seed = (M.rng("faults").random((6, 7, 9)) < 0.04).astype(np.uint8)
    seed[1, 2, 3] = 1
    for spacing in ((1, 1, 1), (2, 1, 0.5)):
        ref = M.edt_sq_ref(seed, spacing)
        assert M.check_edt_exact(ref.astype(np.float32), ref, "clean") == seed.size
        for fault in ("skip_axis", "cityblock"):
            with pytest.raises(AssertionError, match="elements differ"):
                M.check_edt_exact(M.edt_sq_ref(seed, spacing, fault).astype(np.float32), ref, fault)
    with pytest.raises(AssertionError, match="not exact"):
        M.check_edt_exact(ref.astype(np.float32), M.edt_sq_ref(seed, (3.0, 0.7, 0.7)), "inexact reference")


def test_bound_checker_passes_fp32_evaluation_and_rejects_faults():
    """The contract evaluated in fp32 on the CPU stays inside the derived bound; one fp32 ulp more than the bound allows, a skipped
    axis and city-block distances do not."""
    spacing, shape = (3.0, 0.7, 0.7), (9, 11, 13)
    seed = (M.rng("bound").random(shape) < 0.03).astype(np.uint8)
    seed[4, 5, 6] = 1
    ref = M.edt_sq_ref(seed, spacing)
    sp = np.asarray(M.f32_spacing(spacing), dtype=np.float32)
    g = np.where(seed != 0, np.float32(0), np.float32(np.inf))
    for axis in (2, 1, 0):                              # x, y, z: g + fl(fl(s k) fl(s k)) in fp32, the minimum over the line
        n = shape[axis]
        k = np.arange(n, dtype=np.float32)
        t = sp[axis] * np.abs(k[:, None] - k[None, :])
        t = (t * t).astype(np.float32)
        gm = np.moveaxis(g, axis, -1)
        g = np.moveaxis((gm[..., None, :] + t).astype(np.float32).min(-1), -1, axis)
    worst = M.check_edt_bound(g, ref, "fp32 contract")
    assert 0 < worst <= 4.0, worst
    with pytest.raises(AssertionError, match="outside"):
        M.check_edt_bound(g * np.float32(1 + 2 ** -21), ref, "five ulp off")
    for fault in ("skip_axis", "cityblock"):
        with pytest.raises(AssertionError, match="outside"):
            M.check_edt_bound(M.edt_sq_ref(seed, spacing, fault), ref, fault)
    bad = g.copy()
    bad[0, 0, 0] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        M.check_edt_bound(bad, ref, "unwritten")


def test_surface_checker_rejects_26_connectivity_and_an_open_border():
    pred, _ = _case()
    full = np.ones((3, 4, 5), dtype=np.uint8)
    for vol, fault in ((pred, "conn26"), (full, "border"), (M.box((6, 6, 6), (0, 1, 1), (4, 4, 4)), "border")):
        want = M.surface_ref(vol, 1)
        M.check_equal(want.copy(), want, "clean")
        with pytest.raises(AssertionError, match="elements differ"):
            M.check_equal(M.surface_ref(vol, 1, fault), want, fault)


def test_confusion_checker_rejects_a_transposed_matrix():
    pred, label = _case()
    cm, _ = M.confusion_ref(pred, label, 3)
    with pytest.raises(AssertionError, match="elements differ"):
        M.check_equal(M.confusion_ref(pred, label, 3, fault="transpose")[0], cm, "transposed")
    o, ot = M.overlap_ref(cm), M.overlap_ref(cm.T)
    with pytest.raises(AssertionError, match="elements differ"):
        M.check_equal(ot["sensitivity"], o["sensitivity"], "sensitivity from the transpose")


def test_metric_checkers_reject_faulty_distances_and_the_nearest_percentile():
    pred, label = _case()
    for cls in (1, 2):
        ref = M.surface_distances_ref(pred, label, cls, (1, 1, 1), 95.0, 2.0)
        assert ref.n_pred > 0 and ref.n_label > 0
        M.check_hd(np.float32(ref.hd), max(ref.max_d2_pred, ref.max_d2_label), "clean hd")
        M.check_assd(float(np.sqrt(ref.d2_pred).astype(np.float32).astype(np.float64).sum() + np.sqrt(ref.d2_label).astype(np.float32).astype(np.float64).sum())
                     / (ref.n_pred + ref.n_label), ref, "clean assd")
        M.check_percentile(np.float32(ref.hd_percentile), ref, 95.0, "clean percentile")
        for fault in ("cityblock", "skip_axis", "conn26"):
            f = M.surface_distances_ref(pred, label, cls, (1, 1, 1), 95.0, 2.0, fault=fault)
            with pytest.raises(AssertionError):
                M.check_assd(f.assd, ref, fault)
        with pytest.raises(AssertionError):
            M.check_hd(np.nextafter(np.float32(ref.hd), np.float32(np.inf)), max(ref.max_d2_pred, ref.max_d2_label), "one ulp off")
    # the percentile: a line of 39 prediction voxels at distances 1 .. 39 from a single label voxel (on a lattice the neighbouring
    # order statistics of a real case are mostly equal, and then every interpolation method agrees)
    line_p, line_g = np.zeros((1, 1, 40), dtype=np.uint8), np.zeros((1, 1, 40), dtype=np.uint8)
    line_p[0, 0, 1:] = 1
    line_p[0, 0, 2:39:2] = 2           # (class 1 keeps isolated voxels: each is its own surface)
    line_g[0, 0, 0] = 1
    for q in (95.0, 50.0, 12.5):
        lin = M.surface_distances_ref(line_p, line_g, 1, (1, 1, 0.7), q, 2.0)
        near = M.surface_distances_ref(line_p, line_g, 1, (1, 1, 0.7), q, 2.0, fault="nearest")
        assert lin.n_pred == 20 and lin.n_label == 1 and near.hd_percentile != lin.hd_percentile
        M.check_percentile(np.float32(lin.hd_percentile), lin, q, "clean percentile")
        with pytest.raises(AssertionError):
            M.check_percentile(np.float32(near.hd_percentile), lin, q, "nearest")
    empty = M.surface_distances_ref(pred, np.zeros_like(label), 1)
    assert empty.n_label == 0 and empty.n_pred > 0 and np.isnan(empty.hd) and np.isnan(empty.assd) and np.isnan(empty.nsd)
    assert np.isinf(empty.max_d2_pred) and empty.max_d2_label == -np.inf
