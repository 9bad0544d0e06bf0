"""Case-level evaluation on the GPU (csrc/metrics.hip, mednet_hip.metrics) against the numpy restatement of tests/metrics_util.py:
confusion counts, surface masks and the distance transform bit for bit where the arithmetic is exact, the transform with general
spacing and the composed metrics inside bounds derived from the number formats (profiles/case_metrics_bounds.md), bit-identical
between runs, and with every kernel's reads and writes inside its tensors (tests/fence.py)."""
import functools

import numpy as np
import pytest
import torch

import metrics_util as M
import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import metrics as H
from mednet_hip import predict as HP
from mednet_hip.unet import model as HM
from oracle import ref_cpu as O

from fence import Fence
from gpu_util import DEV

pytestmark = pytest.mark.gpu

UNIT, DYADIC, GENERAL = (1, 1, 1), (2, 1, 0.5), (3.0, 0.7, 0.7)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------- confusion, overlap
def check_overlap(cm_dev, cm_ref, what):
    """Ratios: each side rounds a sum or product and a quotient once in fp64, so they agree within 4 * 2^-53; NaN where numpy has
    NaN.  Volumes: equal."""
    got = dict(zip(("dice", "iou", "sensitivity", "precision", "volume_pred", "volume_label"), (host(t) for t in H.overlap(cm_dev))))
    want = M.overlap_ref(cm_ref)
    for k in ("volume_pred", "volume_label"):
        M.check_equal(got[k], want[k], f"{what}: {k}")
    for k in ("dice", "iou", "sensitivity", "precision"):
        g, w = got[k], want[k]
        assert g.dtype == np.float64 and np.array_equal(np.isnan(g), np.isnan(w)), f"{what}: {k} NaNs {g} / {w}"
        live = ~np.isnan(w)
        assert (np.abs(g[live] - w[live]) <= 4 * 2.0 ** -53 * np.abs(w[live])).all(), f"{what}: {k} {g} / {w}"


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 17, 241), (17, 9, 70)], ids=["1", "4097", "10710"])
def test_confusion_equals_bincount(shape):
    """One voxel, one workgroup's share plus one, a ragged count reaching a third workgroup; 1, 2, 5, 32 classes; values >= ncls in
    both volumes; with and without ignore_index; the label read in place as the last channel of a uint8 C x D x H x W volume."""
    for ncls in (1, 2, 5, 32):
        pred = M.random_labels(f"cp{shape}{ncls}", shape, ncls, stray=0.05)
        label = M.random_labels(f"cl{shape}{ncls}", shape, ncls, stray=0.05)
        vol4 = dev(np.stack([M.random_labels("other", shape, 7), label]))
        for ignore in (None, 0, ncls - 1, 200):
            for lab_dev in (dev(label), vol4[-1]):
                cm, oor = H.confusion(dev(pred), lab_dev, ncls, ignore_index=ignore)
                want, want_oor = M.confusion_ref(pred, label, ncls, ignore)
                assert cm.dtype == torch.int64 and tuple(cm.shape) == (ncls, ncls)
                M.check_equal(host(cm), want, f"confusion {shape} ncls {ncls} ignore {ignore}")
                assert int(oor) == want_oor, (shape, ncls, ignore, int(oor), want_oor)
                check_overlap(cm, want, f"overlap {shape} ncls {ncls} ignore {ignore}")
    clean = M.random_labels("clean", shape, 3)
    cm, oor = H.confusion(dev(clean), dev(clean), 5)
    assert int(oor) == 0 and np.array_equal(host(cm), np.diag(np.bincount(clean.reshape(-1), minlength=5)))
    check_overlap(cm, host(cm), "classes 3 and 4 absent from both: NaN")


def test_confusion_takes_converted_labels_and_refuses_too_many_classes():
    shape = (5, 6, 7)
    pred = M.random_labels("ip", shape, 4)
    label = M.random_labels("il", shape, 4).astype(np.int64)
    label[0, 0, :3] = -100
    label[1, 1, :2] = 300
    cm, oor = H.confusion(dev(pred), dev(label), 4, ignore_index=-100)
    want, want_oor = M.confusion_ref(pred, label, 4, -100)
    M.check_equal(host(cm), want, "int64 label with ignore_index -100")
    assert int(oor) == want_oor == 2
    with pytest.raises(RuntimeError, match="confusion: ncls 33"):
        H.confusion(dev(pred), dev(pred), 33)
    with pytest.raises(ValueError):
        H.confusion(dev(pred), dev(pred)[:-1], 4)


# ---------------------------------------------------------------------------------------------- surface mask
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 5), (3, 4, 5), (17, 9, 70)])
def test_surface_mask_equals_the_restatement(shape):
    """Random classes, the full volume (its shell), a single interior voxel, an absent class, a mask touching every face."""
    vols = [(M.random_labels(f"sm{shape}", shape, 3), 1), (M.random_labels(f"sm{shape}", shape, 3), 0), (np.ones(shape, dtype=np.uint8), 1),
            (np.ones(shape, dtype=np.uint8), 5), (M.box(shape, tuple(s // 2 for s in shape), (1, 1, 1), cls=9), 9)]
    touching = np.full(shape, 4, dtype=np.uint8)
    if min(shape) >= 3:
        touching[1:-1, 1:-1, 1:-1][M.rng("hole").random(tuple(s - 2 for s in shape)) < 0.2] = 0
    vols.append((touching, 4))
    for vol, cls in vols:
        got = H.surface_mask(dev(vol), cls)
        assert got.dtype == torch.uint8
        M.check_equal(host(got), M.surface_ref(vol, cls), f"surface {shape} class {cls}")
    a, b = vols[0][0], vols[5][0]
    sa, sb = H._surface_masks(dev(a), dev(b), 1)          # (prediction and label in one launch)
    M.check_equal(host(sa), M.surface_ref(a, 1), "pair: first")
    M.check_equal(host(sb), M.surface_ref(b, 1), "pair: second")


# ---------------------------------------------------------------------------------------------- transform, exact cases
def run_edt(seed, spacing):
    out = H.edt_squared(dev(seed), spacing)
    assert out.dtype == torch.float32 and tuple(out.shape) == seed.shape
    return host(out)


def sparse_seeds(tag, shape, p=0.02, at_least=1):
    g = M.rng(tag)
    seed = (g.random(shape) < p).astype(np.uint8)
    for _ in range(at_least):
        seed[tuple(int(g.integers(0, s)) for s in shape)] = 1
    return seed


@pytest.mark.parametrize("spacing", [UNIT, DYADIC], ids=["unit", "dyadic"])
def test_transform_is_exact_for_unit_and_dyadic_spacing(spacing):
    """Bit equality with the fp64 brute force: random sparse seeds, one seed in a corner, every voxel a seed, no seed, one voxel."""
    for shape in ((7, 9, 70), (20, 20, 20)):
        seed = sparse_seeds(f"ex{shape}", shape)
        M.check_edt_exact(run_edt(seed, spacing), M.edt_sq_ref(seed, spacing), f"sparse {shape}")
    corner = np.zeros((6, 7, 9), dtype=np.uint8)
    corner[-1, 0, -1] = 1
    M.check_edt_exact(run_edt(corner, spacing), M.edt_sq_ref(corner, spacing), "corner seed")
    full = np.ones((5, 6, 7), dtype=np.uint8)
    assert not run_edt(full, spacing).any()
    none = run_edt(np.zeros((5, 6, 7), dtype=np.uint8), spacing)
    assert np.isposinf(none).all()
    for one in (0, 1):
        got = run_edt(np.full((1, 1, 1), one, dtype=np.uint8), spacing)
        assert got[0, 0, 0] == (0.0 if one else np.inf)


# extents at the boundaries of a wavefront (63, 64, 65), of the 8 outputs a thread keeps (7, 8, 9), of the bundle tiers (padded
# extent 240 | 248 and 464 | 472) and of the 64 KiB of LDS a launch gets without asking (padded extent 856 | 864)
EXTENTS = (1, 2, 7, 8, 9, 63, 64, 65, 130, 240, 241, 464, 465, 856, 857)


@pytest.mark.parametrize("axis", [0, 1, 2], ids=["z", "y", "x"])
def test_transform_is_exact_at_every_extent_boundary(axis):
    for n in EXTENTS:
        shape = [3, 5, 2]
        shape[axis] = n
        shape = tuple(shape)
        seed = sparse_seeds(f"b{axis}{n}", shape, p=0.01, at_least=2)
        for spacing in (UNIT, DYADIC):
            M.check_edt_exact(run_edt(seed, spacing), M.edt_sq_ref(seed, spacing), f"extent {n} along axis {axis}, spacing {spacing}")


@pytest.mark.parametrize("shape", [(5, 7, 500), (5, 14, 300), (3, 500, 40), (3, 300, 70), (500, 5, 7), (300, 5, 14)],
                         ids=["x16", "x32", "y16", "y32", "z16", "z32"])
def test_transform_is_exact_over_several_ragged_bundles(shape):
    """Bundles of 16 and of 32 lines (extents 500 and 300) with three workgroups per plane, the last one ragged, along every axis;
    bundles of 64 get theirs from 7 x 9 x 70 and 20 x 20 x 20 above."""
    seed = sparse_seeds(f"rb{shape}", shape, p=0.002, at_least=2)
    for spacing in (UNIT, DYADIC):
        M.check_edt_exact(run_edt(seed, spacing), M.edt_sq_ref(seed, spacing), f"{shape} {spacing}")


@pytest.mark.parametrize("shape", [(2048, 1, 1), (1, 2048, 1), (1, 1, 2048)], ids=["z", "y", "x"])
def test_transform_is_exact_on_the_longest_lines(shape):
    seed = np.zeros(shape, dtype=np.uint8).reshape(-1)
    seed[[0, 700, 2040]] = 1
    seed = seed.reshape(shape)
    for spacing in (UNIT, DYADIC):
        M.check_edt_exact(run_edt(seed, spacing), M.edt_sq_ref(seed, spacing), f"{shape} {spacing}")
    far = np.zeros(shape, dtype=np.uint8).reshape(-1)
    far[2047] = 1
    far = far.reshape(shape)
    got = run_edt(far, UNIT).reshape(-1)
    assert got[0] == 2047.0 ** 2 and got[2047] == 0.0


# ---------------------------------------------------------------------------------------------- transform, general spacing
@pytest.mark.parametrize("shape", [(7, 9, 70), (20, 20, 20), (9, 11, 13)])
def test_transform_with_general_spacing_stays_inside_the_derived_bound(shape):
    """Spacing (3.0, 0.7, 0.7): every element within (1 + 2^-24)^4 - 1 of the fp64 brute force, relative (all terms are non-negative;
    profiles/case_metrics_bounds.md).  The kernels' own contract rounds less and is derived there to (1 + 2^-24)^3 - 1."""
    seed = sparse_seeds(f"gen{shape}", shape)
    worst = M.check_edt_bound(run_edt(seed, GENERAL), M.edt_sq_ref(seed, GENERAL), f"general spacing {shape}")
    print(f"[metrics] edt general spacing {shape}: worst relative error {worst:.2f} u (bound {M.EDT_REL / M.U32:.2f} u)")
    none = run_edt(np.zeros(shape, dtype=np.uint8), GENERAL)
    assert np.isposinf(none).all()


# ---------------------------------------------------------------------------------------------- statistics and composed metrics
@functools.lru_cache(maxsize=None)
def blob_case():
    shape = (24, 20, 28)
    pred = M.blobs("pred", shape, 3, shift=(1, -2, 3), jitter=0.01)
    label = M.blobs("label", shape, 3, jitter=0.004)
    return pred, label


def check_class(pred, label, cls, percentile, tolerance, what):
    """The four kernels one after the other, then the composed metrics, for one class with unit spacing."""
    ref = M.surface_distances_ref(pred, label, cls, UNIT, percentile, tolerance)
    p, g = dev(pred), dev(label)
    sp, sg = H._surface_masks(p, g, cls)
    tol_sq = float(np.float32(tolerance) ** 2)
    for seed, surf, n, within, mx, d2ref, name in ((sg, sp, ref.n_pred, ref.within_pred, ref.max_d2_pred, ref.d2_pred, "pred -> label"),
                                                   (sp, sg, ref.n_label, ref.within_label, ref.max_d2_label, ref.d2_label, "label -> pred")):
        d2 = H.edt_squared(seed, UNIT)
        counts, mx_dev, sum_dev = H.surface_stats(surf, d2, tol_sq)
        assert [int(counts[0]), int(counts[1])] == [n, within], (what, name, host(counts), n, within)
        assert float(mx_dev) == mx and mx_dev.dtype == torch.float32, (what, name, float(mx_dev), mx)
        want_sum = float(np.sqrt(d2ref).sum())
        assert sum_dev.dtype == torch.float64
        if np.isfinite(want_sum):
            assert abs(float(sum_dev) - want_sum) <= (M.U32 + 2.0 * (n + 2) * 2.0 ** -53) * want_sum, (what, name, float(sum_dev), want_sum)
        else:                                            # (the other surface is empty: every distance is +inf)
            assert float(sum_dev) == want_sum, (what, name, float(sum_dev), want_sum)
    hd, hdp, assd, nsd, n_pred, n_label = (host(t)[0] for t in H.surface_distances(p, g, [cls], UNIT, percentile, tolerance))
    assert (int(n_pred), int(n_label)) == (ref.n_pred, ref.n_label), (what, n_pred, n_label)
    M.check_hd(hd, max(ref.max_d2_pred, ref.max_d2_label) if not np.isnan(ref.hd) else np.nan, what + ": hd")
    a = M.check_assd(assd, ref, what + ": assd")
    q = M.check_percentile(hdp, ref, percentile, what + ": hd_percentile")
    if np.isnan(ref.nsd):
        assert np.isnan(nsd), (what, nsd)
    else:
        assert nsd == ref.nsd, (what, nsd, ref.nsd)
    hd100 = host(H.surface_distances(p, g, [cls], UNIT, 100.0, tolerance)[1])[0]
    assert (np.isnan(hd) and np.isnan(hd100)) or hd100 == hd, (what, hd100, hd)
    print(f"[metrics] {what}: n {ref.n_pred} / {ref.n_label} hd {hd} assd error {a:.3f} u percentile error {q:.3f} u")
    return ref


@pytest.mark.parametrize("shift", [(0, 0, 3), (1, 2, 2), (3, 4, 0)])
def test_shifted_boxes(shift):
    shape, lo, size = (16, 18, 20), (3, 4, 5), (6, 7, 8)
    a, b = M.box(shape, lo, size), M.box(shape, tuple(l + s for l, s in zip(lo, shift)), size)
    ref = check_class(a, b, 1, 95.0, 2.0, f"boxes shifted by {shift}")
    assert ref.hd == float(np.sqrt(sum(k * k for k in shift)))
    for spacing in (DYADIC, GENERAL):
        hd = float(H.surface_distances(dev(a), dev(b), [1], spacing)[0][0])
        want = np.sqrt(sum((s * k) ** 2 for s, k in zip(M.f32_spacing(spacing), shift)))
        assert abs(hd - want) <= 4 * M.U32 * want, (spacing, hd, want)


@pytest.mark.parametrize("cls", [1, 2])
def test_overlapping_blobs(cls):
    pred, label = blob_case()
    ref = check_class(pred, label, cls, 95.0, 2.0, f"blobs class {cls}")
    assert ref.n_pred > 100 and ref.n_label > 100 and ref.hd > 2.0
    check_class(pred, label, cls, 37.5, 1.0, f"blobs class {cls}, percentile 37.5")


def test_a_class_present_in_one_volume_only_gives_nan_and_the_counts():
    pred, label = blob_case()
    only_pred = np.where(label == 2, 0, label).astype(np.uint8)
    ref = check_class(pred, only_pred, 2, 95.0, 1.0, "class 2 missing from the label")
    assert ref.n_pred > 0 and ref.n_label == 0 and np.isnan(ref.hd)
    ref = check_class(only_pred, pred, 2, 95.0, 1.0, "class 2 missing from the prediction")
    assert ref.n_pred == 0 and ref.n_label > 0
    hd, hdp, assd, nsd, n_pred, n_label = H.surface_distances(dev(pred), dev(label), [7, 1], UNIT)
    assert host(n_pred)[0] == 0 and host(n_label)[0] == 0 and np.isnan(host(hd)[0]) and np.isnan(host(nsd)[0]) and not np.isnan(host(hd)[1])
    with pytest.raises(ValueError):
        H.surface_distances(dev(pred), dev(label), [1], UNIT, tolerance=-1.0)


# ---------------------------------------------------------------------------------------------- evaluate_case
def table_ref(pred, label, ncls, classes, spacing, percentile, tolerance, ignore=None):
    cm, oor = M.confusion_ref(pred, label, ncls, ignore)
    return cm, oor, M.overlap_ref(cm), [M.surface_distances_ref(pred, label, c, spacing, percentile, tolerance) for c in classes]


def check_table(t, pred, label, ncls, what, classes=None, percentile=95.0, tolerance=1.0):
    """A to_host() table against the restatement, field by field (unit spacing)."""
    classes = tuple(range(1, ncls)) if classes is None else classes
    cm, oor, ov, refs = table_ref(pred, label, ncls, classes, UNIT, percentile, tolerance)
    assert t["classes"] == classes and t["out_of_range"] == oor
    M.check_equal(t["confusion"], cm, what + ": confusion")
    for k in ("volume_pred", "volume_label"):
        M.check_equal(t[k], ov[k], f"{what}: {k}")
    for k in ("dice", "iou", "sensitivity", "precision"):
        assert np.array_equal(np.isnan(t[k]), np.isnan(ov[k])), (what, k)
        live = ~np.isnan(ov[k])
        assert (np.abs(t[k][live] - ov[k][live]) <= 4 * 2.0 ** -53 * np.abs(ov[k][live])).all(), (what, k, t[k], ov[k])
    for i, (c, ref) in enumerate(zip(classes, refs)):
        assert (t["n_pred"][i], t["n_label"][i]) == (ref.n_pred, ref.n_label), (what, c)
        M.check_hd(t["hd"][i], max(ref.max_d2_pred, ref.max_d2_label) if not np.isnan(ref.hd) else np.nan, f"{what}: hd of class {c}")
        M.check_assd(t["assd"][i], ref, f"{what}: assd of class {c}")
        M.check_percentile(t["hd_percentile"][i], ref, percentile, f"{what}: hd_percentile of class {c}")
        assert (np.isnan(ref.nsd) and np.isnan(t["nsd"][i])) or t["nsd"][i] == ref.nsd, (what, c, t["nsd"][i], ref.nsd)


def same_tables(a, b):
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert v.dtype == b[k].dtype and np.array_equal(v.view(np.int64), b[k].view(np.int64)), k
        else:
            assert v == b[k], k


def test_evaluate_case_equals_the_restatement_and_repeats_bit_for_bit():
    pred, label = blob_case()
    p, g = dev(pred), dev(label)
    first = H.evaluate_case(p, g, 3, tolerance=2.0)
    assert first.dice.is_cuda and first.hd.is_cuda and first.confusion.is_cuda
    t = first.to_host()
    check_table(t, pred, label, 3, "blobs", tolerance=2.0)
    same_tables(t, H.evaluate_case(p, g, 3, tolerance=2.0).to_host())
    four = H.evaluate_case(p, g, 4, classes=(2, 3), percentile=50.0).to_host()
    check_table(four, pred, label, 4, "blobs, 4 classes, classes (2, 3)", classes=(2, 3), percentile=50.0)
    assert np.isnan(four["dice"][3]) and np.isnan(four["hd"][1]) and four["n_pred"][1] == 0


def test_blended_prediction_evaluate():
    """ResidualUNet3D(1, 3) with random weights, 32^3 patches on 40 x 36 x 44, blend="gaussian": .evaluate(label) is evaluate_case on
    .result()[-1], and both equal the restatement on that uint8 volume copied to the host."""
    shape, patch, ov = (40, 36, 44), (32, 32, 32), (4, 4, 4)
    img = (O._rng("metrics:e2e").standard_normal((1,) + shape) * 2).astype(np.float16)
    label = M.blobs("e2e", shape, 3)
    with mednet_hip.precision("fp32"):
        net = O.keyed_init_(HM.ResidualUNet3D(in_channels=1, out_channels=3, final_sigmoid=False, f_maps=[8, 16])).to(DEV).eval()
        bp = HP.GridPredictor(net, patch, ov, num_heatmaps=0, pad_mode="symmetric", batch_size=2, blend="gaussian").predict(img)
        t = bp.evaluate(dev(label)).to_host()
        result = bp.result()
    assert result.dtype == torch.uint8 and tuple(result.shape) == (1,) + shape
    same_tables(t, H.evaluate_case(result[-1], dev(label), 3).to_host())
    check_table(t, host(result[-1]), label, 3, "blended prediction")


# ---------------------------------------------------------------------------------------------- footprint
def test_every_entry_stays_inside_its_tensors():
    """Inputs, outputs and workspaces in slabs of their own between guard bands, the workspaces at exactly the size the queries
    answer: the outputs equal the unfenced ones bit for bit and no guard byte changes."""
    pred, label = blob_case()
    shape, ncls, cls = pred.shape, 3, 1
    p, g = dev(pred), dev(label)
    cm0, oor0 = H.confusion(p, g, ncls)
    sp0, sg0 = H._surface_masks(p, g, cls)
    d20 = H.edt_squared(sg0, GENERAL)
    st0 = H.surface_stats(sp0, d20, 4.0)
    with Fence() as fence:
        fp, fg = fence.put(p), fence.put(g)
        cm, oor = H.confusion(fp, fg, ncls)
        sp, sg = H._surface_masks(fp, fg, cls)
        d2 = H.edt_squared(sg, GENERAL)
        st = H.surface_stats(sp, d2, 4.0)
        fence.check()
        for t in (cm, oor, sp, sg, d2) + tuple(st):
            assert fence.owns(t)
        lib = L.lib()
        asked = [r[0] for r in fence.ws_requests]
        assert asked == [lib.mednet_confusion_ws_bytes(*shape, ncls), lib.mednet_surface_stats_ws_bytes(*shape)] == [r[1] for r in fence.ws_requests]
        assert torch.equal(cm, cm0) and torch.equal(oor, oor0) and torch.equal(sp, sp0) and torch.equal(sg, sg0)
        assert torch.equal(d2.view(torch.int32), d20.view(torch.int32))
        assert torch.equal(st[0], st0[0]) and torch.equal(st[1].view(torch.int32), st0[1].view(torch.int32))
        assert torch.equal(st[2].view(torch.int64), st0[2].view(torch.int64))
    # the ragged shape of the other suites, every bundle edge open: 10710 voxels, three workgroups, x beyond one wavefront
    vol = M.random_labels("fence", (17, 9, 70), 3, stray=0.02)
    seed = sparse_seeds("fence", (17, 9, 70))
    want = H.edt_squared(dev(seed), DYADIC)
    with Fence() as fence:
        fv, fs = fence.put(dev(vol)), fence.put(dev(seed))
        cm, _ = H.confusion(fv, fv, 32, ignore_index=1)
        mask = H.surface_mask(fv, 2)
        d2 = H.edt_squared(fs, DYADIC)
        st = H.surface_stats(mask, d2, 1.0)
        fence.check()
        assert fence.owns(d2) and fence.owns(mask) and fence.owns(cm)
        assert torch.equal(d2.view(torch.int32), want.view(torch.int32))
        M.check_equal(host(cm), M.confusion_ref(vol, vol, 32, 1)[0], "fenced confusion")
        M.check_equal(host(mask), M.surface_ref(vol, 2), "fenced surface mask")
        assert int(st[0][0]) == int(M.surface_ref(vol, 2).sum())


# ---------------------------------------------------------------------------------------------- landmarks
def test_landmark_errors():
    pos = np.array([[3, 4, 5], [0, 0, 0], [10, 2, 7], [6, 6, 6], [1, 9, 2]], dtype=np.int64)
    tgt = np.array([[3, 4, 5], [1, 2, 2], [8.5, 2.25, 9], [0, 0, 0], [1, 9, 40]])
    spacing = (3.0, 0.7, 0.7)
    got = H.landmark_errors(dev(pos), dev(tgt), spacing)
    want = np.sqrt((((pos - tgt) * np.asarray(spacing)) ** 2).sum(1))
    assert got.is_cuda and got.dtype == torch.float64 and np.allclose(host(got), want, rtol=1e-14, atol=0)
    assert np.allclose(host(H.landmark_errors(dev(pos), tgt.tolist())), np.sqrt(((pos - tgt) ** 2).sum(1)), rtol=1e-14, atol=0)
