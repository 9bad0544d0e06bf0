"""Connected components on the GPU (csrc/components.hip, mednet_hip.components, metrics.lesion_detection) against the numpy
restatement of tests/components_util.py.  Every comparison is equality of integer arrays: the whole int32 label volume, K, the whole
statistics table, the whole filtered volume, the detection counts.  Every labelling also asserts the kernels' error word info[1] == 0
(a parent walk that reached its step cap).  Shapes are the smallest at which the kernels take another path: one voxel, lines along
each axis longer than a wave's 256-voxel chunk, volumes at byte offsets 1 .. 3 (the 4-byte loads' alignment head), voxel counts above
two numbering rows of 4096 that are no multiple of it, an extent of 2048."""
import functools

import numpy as np
import pytest
import torch

import components_util as U
import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import components as C
from mednet_hip import metrics as H
from mednet_hip import predict as HP
from mednet_hip.unet import model as HM
from oracle import ref_cpu as O

from fence import Fence
from gpu_util import DEV

pytestmark = pytest.mark.gpu

CONN = (6, 18, 26)
RANDOM_SHAPE = (33, 34, 65)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)      # (a copy: the shared cases are read-only)


def host(t):
    return t.detach().cpu().numpy()


def raw_label(vol_dev, cls, conn, invert=False, labels=None, info=None, ws=None):
    """mednet_cc_label through the C ABI -> (labels tensor, K, error word)."""
    d, h, w = vol_dev.shape
    labels = torch.empty((d, h, w), dtype=torch.int32, device=DEV) if labels is None else labels
    info = torch.empty((2,), dtype=torch.int64, device=DEV) if info is None else info
    need = L.lib().mednet_cc_ws_bytes(d, h, w)
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV) if ws is None else ws
    assert ws.numel() == need
    L.check(L.lib().mednet_cc_label(vol_dev.data_ptr(), L.CC_ALL if cls is None else cls, int(invert), conn, d, h, w, labels.data_ptr(),
                                    info.data_ptr(), ws.data_ptr(), need, L.stream()), "cc_label")
    k, err = info.tolist()
    return labels, k, err


def check_label(vol, cls=1, conn=26, invert=False, what="", offset=0):
    """The whole label volume and K equal the restatement's; the error word is 0.  offset: the volume's byte offset in its allocation."""
    vol = np.ascontiguousarray(vol, dtype=np.uint8)
    buf = torch.zeros((vol.size + 8,), dtype=torch.uint8, device=DEV)
    v = buf[offset:offset + vol.size].view(vol.shape)
    v.copy_(dev(vol))
    assert v.data_ptr() % 4 == offset % 4
    labels, k, err = raw_label(v, cls, conn, invert)
    want, kw = U.label(vol, cls, conn, invert)
    assert err == 0, f"{what}: error word {err}"
    assert k == kw, f"{what} {vol.shape} cls {cls} conn {conn} invert {invert} offset {offset}: K {k}, expected {kw}"
    got = host(labels)
    assert got.dtype == np.int32 and np.array_equal(got, want), \
        f"{what} {vol.shape} cls {cls} conn {conn} invert {invert} offset {offset}: {int((got != want).sum())} voxels differ"
    return labels, k


def two(shape, a, b):
    vol = np.zeros(shape, dtype=np.uint8)
    vol[a] = vol[b] = 1
    return vol


@functools.lru_cache(maxsize=None)
def random_case(density, classes=1):
    vol = U.random_volume(RANDOM_SHAPE, density, seed=int(density * 100) + classes, classes=classes)
    vol.setflags(write=False)
    return vol


# ---------------------------------------------------------------------------------------------- degenerate volumes
def test_degenerate_volumes():
    for conn in CONN:
        check_label(np.ones((1, 1, 1)), 1, conn, what="one foreground voxel")
        check_label(np.zeros((1, 1, 1)), 1, conn, what="one background voxel")
        check_label(np.zeros((3, 5, 7)), 1, conn, what="empty")
        check_label(np.ones((3, 5, 7)), 1, conn, what="full")
        for shape in ((1, 1, 130), (1, 130, 1), (130, 1, 1), (1, 1, 600)):
            check_label(np.ones(shape), 1, conn, what="a full line")
            line = U.random_volume(shape, 0.7, seed=sum(shape))
            check_label(line, 1, conn, what="a broken line")


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_volume_at_an_odd_address(offset):
    for shape in ((1, 1, 1), (1, 1, 2), (1, 1, 130), (3, 5, 7), (2, 3, 301)):
        for conn in CONN:
            check_label(np.ones(shape), 1, conn, what="full", offset=offset)
            check_label(U.random_volume(shape, 0.5, seed=offset, classes=3), None, conn, what="random", offset=offset)


# ---------------------------------------------------------------------------------------------- connectivity, wrap-around
def test_face_edge_corner_and_checkerboard():
    shape = (3, 4, 5)
    for vol, counts in ((two(shape, (1, 1, 1), (1, 1, 2)), (1, 1, 1)), (two(shape, (1, 1, 1), (1, 2, 1)), (1, 1, 1)),
                        (two(shape, (1, 1, 1), (2, 1, 1)), (1, 1, 1)), (two(shape, (1, 1, 1), (1, 2, 2)), (2, 1, 1)),
                        (two(shape, (1, 1, 1), (2, 1, 2)), (2, 1, 1)), (two(shape, (1, 1, 1), (2, 2, 1)), (2, 1, 1)),
                        (two(shape, (1, 1, 2), (2, 2, 1)), (2, 2, 1)), (two(shape, (1, 1, 1), (2, 2, 2)), (2, 2, 1)),
                        (two(shape, (1, 2, 1), (2, 1, 2)), (2, 2, 1))):
        for conn, n in zip(CONN, counts):
            _, k = check_label(vol, 1, conn, what="two voxels")
            assert k == n
    cb = U.checkerboard((6, 7, 9))
    assert check_label(cb, 1, 6, what="checkerboard")[1] == int(cb.sum())
    assert check_label(cb, 1, 18, what="checkerboard")[1] == 1
    assert check_label(cb, 1, 26, what="checkerboard")[1] == 1


def test_no_wrap_around():
    """Neighbours in memory that are no neighbours in the volume: the end of a row and the start of the next, the end of a plane and
    the start of the next, and their diagonal variants.  Two components under every connectivity."""
    shape = (3, 4, 5)
    pairs = [((0, 0, 4), (0, 1, 0)), ((1, 2, 4), (1, 3, 0)), ((0, 3, 2), (1, 0, 2)), ((0, 3, 4), (1, 0, 0)), ((1, 3, 4), (2, 0, 0)),
             ((0, 3, 3), (1, 0, 4)), ((0, 3, 1), (1, 0, 0)), ((0, 1, 4), (0, 2, 1)), ((0, 1, 4), (1, 2, 0)), ((0, 0, 4), (1, 1, 0)),
             ((0, 2, 0), (0, 1, 4)), ((0, 3, 0), (1, 0, 1))]
    for a, b in pairs:
        for conn in CONN:
            _, k = check_label(two(shape, a, b), 1, conn, what=f"wrap {a} {b}")
            assert k == 2, (a, b, conn)


# ---------------------------------------------------------------------------------------------- long chains
@pytest.mark.parametrize("conn", CONN)
def test_long_chains_across_every_workgroup(conn):
    """One component that visits every part of the volume, joined only at far ends.  (9, 17, 70) = 10 710 voxels: three numbering
    rows, the last ragged; (1, 45, 301): rows longer than a wave's chunk."""
    for shape in ((1, 33, 70), (9, 17, 70), (1, 45, 301)):
        s = U.serpentine(shape)
        assert check_label(s, 1, conn, what="serpentine")[1] == 1
        assert check_label(s[:, :, ::-1], 1, conn, what="mirrored serpentine")[1] == 1
        check_label(s, 1, conn, invert=True, what="the serpentine's complement")
    for shape in ((1, 33, 70), (1, 61, 135)):
        sp = U.spiral(shape)
        assert check_label(sp, 1, conn, what="spiral")[1] == 1
        assert check_label(sp[:, ::-1, ::-1], 1, conn, what="spiral from the first voxel")[1] == 1
        check_label(sp, 1, conn, invert=True, what="the spiral's complement")


# ---------------------------------------------------------------------------------------------- random volumes
@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("density", [0.05, 0.31, 0.9])
def test_random_volumes(density, conn):
    vol = random_case(density)
    check_label(vol, 1, conn, what="random")
    check_label(vol, 1, conn, invert=True, what="random, inverted")
    check_label(vol, 0, conn, what="random, class 0")


@pytest.mark.parametrize("conn", CONN)
def test_all_classes_in_one_labelling(conn):
    for density in (0.31, 0.9):
        vol = random_case(density, classes=5)
        check_label(vol, None, conn, what="five classes")
        check_label(vol, 3, conn, what="one of five classes")
        check_label(vol, 3, conn, invert=True, what="all but one of five classes")


@pytest.mark.parametrize("shape", [(2, 3, 2048), (2048, 2, 3), (3, 2048, 2)], ids=str)
def test_an_extent_of_2048(shape):
    vol = U.random_volume(shape, 0.6, seed=7, classes=2)
    for conn in CONN:
        check_label(vol, None, conn, what="extent 2048")
    check_label(np.ones(shape), 1, 6, what="extent 2048, full")


# ---------------------------------------------------------------------------------------------- statistics
def check_stats(vol, cls, conn, what):
    comps = C.label_components(dev(vol), cls, conn)
    lab, k = U.label(vol, cls, conn)
    assert comps.count == k and np.array_equal(host(comps.labels), lab), what
    t = comps.stats()
    assert t.dtype == torch.int64 and tuple(t.shape) == (k, 11)
    want = U.stats(vol, lab, k)
    assert np.array_equal(host(t), want), f"{what}: rows {np.flatnonzero((host(t) != want).any(1))[:5]} differ"
    if k:
        assert np.array_equal(host(comps.volumes((3.0, 0.7, 0.7))), want[:, 0].astype(np.float64) * (3.0 * 0.7 * 0.7))
        assert np.array_equal(host(comps.centroids()), want[:, 7:10].astype(np.float64) / want[:, :1].astype(np.float64))
    return comps


@pytest.mark.parametrize("conn", CONN)
def test_statistics_table(conn):
    for density in (0.05, 0.31, 0.9):
        check_stats(random_case(density), 1, conn, f"random {density}")
    check_stats(random_case(0.31, classes=5), None, conn, "five classes")


def test_statistics_of_one_component_and_of_none():
    comps = check_stats(np.full((9, 17, 70), 4, dtype=np.uint8), None, 26, "one component: the whole volume")
    assert host(comps.stats()).tolist() == [[10710, 0, 8, 0, 16, 0, 69, 10710 * 4, 10710 * 8, 10710 * 69 // 2, 4]]
    check_stats(U.serpentine((9, 17, 70)), 1, 6, "serpentine")
    empty = check_stats(np.zeros((3, 5, 7), dtype=np.uint8), 1, 26, "no component")
    assert empty.count == 0 and tuple(empty.stats().shape) == (0, 11)
    v = dev(np.zeros((3, 5, 7), dtype=np.uint8))
    assert L.lib().mednet_cc_stats(v.data_ptr(), empty.labels.data_ptr(), 3, 5, 7, 0, None, L.stream()) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- filters
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
    hole[1, 1, 7] = 0            # (2, 2, 6) reaches the outside only through the corner (1, 1, 7): a hole, the complement is 6-connected
    hole[4, 4, 0:4] = 0          # open to the outside along x
    opened = np.zeros((5, 5, 5), dtype=np.uint8)
    opened[0:4, 1:4, 1:4] = 1
    opened[0:2, 2, 2] = 0        # a cavity that reaches the face z = 0 through one voxel
    return tie, hole, opened


def test_keep_largest():
    tie, _, _ = filter_cases()
    want = tie.copy()
    want[2, 4, 5:8] = 0
    want[1, 2, 2:4] = 0
    assert np.array_equal(U.keep_largest(tie, (1,)), want)
    assert np.array_equal(host(C.keep_largest(dev(tie), (1,))), want), "a tie goes to the smaller id"
    assert np.array_equal(host(C.keep_largest(dev(tie), (7,))), tie), "an absent class"
    assert np.array_equal(host(C.keep_largest(dev(tie), (1, 2, 7))), U.keep_largest(tie, (1, 2, 7)))
    for conn in CONN:
        vol = U.blobs((17, 18, 33), seed=conn, classes=4, count=25)
        v = dev(vol)
        out = C.keep_largest(v, (1, 2, 4), conn)
        assert np.array_equal(host(out), U.keep_largest(vol, (1, 2, 4), conn)) and np.array_equal(host(v), vol)
        same = C.keep_largest(v, (1, 2, 4), conn, out=v)
        assert same is v and np.array_equal(host(v), U.keep_largest(vol, (1, 2, 4), conn)), "in place"
    empty = dev(np.zeros((3, 5, 7), dtype=np.uint8))
    assert not bool(C.keep_largest(empty, (1,)).any())


def test_remove_small():
    tie, _, _ = filter_cases()
    for n in (2, 3, 4):                  # components of 2, 3 and 3 voxels: below, at and above the threshold
        assert np.array_equal(host(C.remove_small(dev(tie), (1,), min_voxels=n)), U.remove_small(tie, (1,), min_voxels=n)), n
    at = host(C.remove_small(dev(tie), (1,), min_voxels=3))
    assert at[0, 0, 0] == 1 and at[2, 4, 5] == 1 and at[1, 2, 2] == 0 and (at == 2).sum() == 10
    sp = (3.0, 0.7, 0.7)
    vv = 3.0 * 0.7 * 0.7
    for mv in (3 * vv, np.nextafter(3 * vv, 10.0), 2 * vv):
        got = host(C.remove_small(dev(tie), (1, 2), min_volume=mv, spacing=sp))
        assert np.array_equal(got, U.remove_small(tie, (1, 2), min_volume=mv, spacing=sp)), mv
    assert host(C.remove_small(dev(tie), (1,), min_volume=3 * vv, spacing=sp))[0, 0, 0] == 1, "count * volume == threshold is kept"
    vol = U.blobs((17, 18, 33), seed=2, classes=3, count=30, radius=(0, 2))
    assert np.array_equal(host(C.remove_small(dev(vol), (1, 3), min_voxels=20, connectivity=6)),
                          U.remove_small(vol, (1, 3), min_voxels=20, connectivity=6))
    with pytest.raises(ValueError):
        C.remove_small(dev(tie), (1,))
    with pytest.raises(ValueError):
        C.remove_small(dev(tie), (1,), min_voxels=1, min_volume=1.0)


def test_fill_holes():
    _, hole, opened = filter_cases()
    want = hole.copy()
    want[3, 3, 2:4] = 1
    want[3, 3, 5] = 1          # another class inside the hole is overwritten
    want[2, 2, 6] = 1          # connected to the outside only diagonally: filled
    assert np.array_equal(U.fill_holes(hole, 1), want)
    assert np.array_equal(host(C.fill_holes(dev(hole), 1)), want)
    assert np.array_equal(host(C.fill_holes(dev(opened), 1)), opened), "a cavity open to the border through one face voxel stays"
    for seed in range(3):
        v = U.random_volume((7, 9, 11), 0.55, seed=seed, classes=2)
        assert np.array_equal(host(C.fill_holes(dev(v), 1)), U.fill_holes(v, 1)), seed
    full = dev(np.ones((3, 5, 7), dtype=np.uint8))
    assert bool((C.fill_holes(full, 1) == 1).all())


def test_postprocess_order():
    """remove-small, keep-largest, fill-holes, in that order: a small component of class 1 that is the only thing inside a class-2
    shell is removed first, and the hole it leaves is then filled with 2."""
    vol = np.zeros((9, 9, 11), dtype=np.uint8)
    vol[1:8, 1:8, 1:8] = 2
    vol[3:6, 3:6, 3:6] = 0
    vol[4, 4, 4] = 1
    vol[0, 0, 9:11] = 1
    vol[8, 8, 9] = 2
    pp = C.Postprocess(keep_largest=(2,), min_voxels={1: 2}, fill_holes=(2,), connectivity=6)
    want = U.postprocess(vol, (2,), {1: 2}, (2,), 6)
    assert want[4, 4, 4] == 2 and want[3, 3, 3] == 2 and want[8, 8, 9] == 0 and want[0, 0, 9] == 1
    v = dev(vol)
    assert np.array_equal(host(pp(v)), want) and np.array_equal(host(v), vol)
    rnd = U.blobs((17, 18, 33), seed=9, classes=3, count=30)
    pp = C.Postprocess(keep_largest=(1, 3), min_voxels={2: 30, 3: 5}, fill_holes=(1,))
    assert np.array_equal(host(pp(dev(rnd))), U.postprocess(rnd, (1, 3), {2: 30, 3: 5}, (1,), 26))


# ---------------------------------------------------------------------------------------------- footprint
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 7), (9, 17, 70)], ids=str)
def test_footprint(shape):
    """Label, statistics and selection with every tensor in a slab of its own: the uint8 volume ENDS at its back guard (a vector load
    past it would bring an impossible value into the labels), the workspace has exactly the queried size, and no guard byte changes."""
    vol = U.random_volume(shape, 0.6, seed=11, classes=3)
    want, kw = U.label(vol, None, 26)
    d, h, w = shape
    with Fence() as fence:
        v = fence.put(dev(vol))
        labels, info = fence.alloc(shape, torch.int32), fence.alloc(2, torch.int64)
        ws = fence.workspace(L.lib().mednet_cc_ws_bytes(d, h, w))
        _, k, err = raw_label(v, None, 26, labels=labels, info=info, ws=ws)
        assert err == 0 and k == kw
        table = fence.alloc((max(k, 1), 11), torch.int64)
        L.check(L.lib().mednet_cc_stats(v.data_ptr(), labels.data_ptr(), d, h, w, k, table.data_ptr(), L.stream()), "cc_stats")
        keep_np = (np.arange(k + 1) % 2).astype(np.uint8)
        keep, out = fence.put(dev(keep_np)), fence.alloc(shape, torch.uint8)
        L.check(L.lib().mednet_cc_select(v.data_ptr(), labels.data_ptr(), keep.data_ptr(), 9, out.data_ptr(), d, h, w, L.stream()), "cc_select")
        fence.check()
        assert all(fence.owns(t) for t in (v, labels, info, ws, table, keep, out))
    assert np.array_equal(host(labels), want)
    assert np.array_equal(host(table)[:k], U.stats(vol, want, kw))
    assert np.array_equal(host(out), U.select(vol, want, keep_np, 9))


def test_footprint_through_the_python_layer():
    vol = U.blobs((9, 17, 70), seed=4, classes=3, count=20)
    with Fence() as fence:
        v = fence.put(dev(vol))
        out = C.keep_largest(v, (1, 2, 3))
        filled = C.fill_holes(v, 1)
        fence.check()
        assert fence.owns(out) and fence.owns(filled)
        assert any(asked == 12 for asked, _, _ in fence.ws_requests), fence.ws_requests
    assert np.array_equal(host(out), U.keep_largest(vol, (1, 2, 3))) and np.array_equal(host(filled), U.fill_holes(vol, 1))


# ---------------------------------------------------------------------------------------------- repeatability
def test_two_runs_are_bit_identical():
    vol = dev(random_case(0.31, classes=5))
    a, b = C.label_components(vol, None, 26), C.label_components(vol, None, 26)
    assert a.count == b.count and torch.equal(a.labels, b.labels) and torch.equal(a.stats(), b.stats())


# ---------------------------------------------------------------------------------------------- detection counts
def counts_of(r):
    return tuple(int(r[k]) for k in ("n_label", "n_pred", "tp_label", "fn", "fp", "tp_pred"))


def check_detection(pred, lab, cls, conn=26, min_overlap=1):
    got = H.lesion_detection(dev(pred), dev(lab), cls, conn, min_overlap)
    for name in ("n_label", "n_pred", "tp_label", "fn", "fp", "tp_pred"):
        t = getattr(got, name)
        assert t.dtype == torch.int64 and t.dim() == 0 and t.is_cuda, name
    g, want = got.to_host(), U.lesion_detection(pred, lab, cls, conn, min_overlap)
    assert counts_of(g) == counts_of(want), (counts_of(g), counts_of(want))
    for name in ("sensitivity", "precision", "f1"):
        assert got.__dict__[name].dtype == torch.float64
        assert (np.isnan(g[name]) and np.isnan(want[name])) or abs(g[name] - want[name]) <= 4 * 2.0 ** -53 * abs(want[name]), name
    return g


def test_detection_counts_hand_built():
    shape = (4, 6, 12)
    lab = np.zeros(shape, dtype=np.uint8)
    lab[1, 1, 1:3] = 1
    lab[1, 1, 5:7] = 1
    pred = np.zeros(shape, dtype=np.uint8)
    pred[1, 1, 1:7] = 1
    g = check_detection(pred, lab, 1)
    assert counts_of(g) == (2, 1, 2, 0, 0, 1) and g["sensitivity"] == 1.0 and g["precision"] == 1.0 and g["f1"] == 1.0
    lab = np.zeros(shape, dtype=np.uint8)
    pred = np.zeros(shape, dtype=np.uint8)
    lab[2, 2, 2:9] = 1
    pred[2, 2, 2:4] = 1
    pred[2, 2, 6:8] = 1
    pred[0, 5, 10] = 1
    g = check_detection(pred, lab, 1)
    assert counts_of(g) == (1, 3, 1, 0, 1, 2) and g["sensitivity"] == 1.0 and g["precision"] == 2 / 3
    g = check_detection(pred, lab, 1, min_overlap=2)
    assert counts_of(g) == (1, 3, 1, 0, 1, 2)
    g = check_detection(pred, lab, 1, min_overlap=3)          # each blob shares two voxels with the lesion: fewer than min_overlap
    assert counts_of(g) == (1, 3, 0, 1, 3, 0) and g["sensitivity"] == 0.0 and g["precision"] == 0.0 and np.isnan(g["f1"])
    zero = np.zeros(shape, dtype=np.uint8)
    g = check_detection(zero, zero, 1)
    assert counts_of(g) == (0, 0, 0, 0, 0, 0) and all(np.isnan(g[k]) for k in ("sensitivity", "precision", "f1"))
    g = check_detection(pred, zero, 1)
    assert counts_of(g) == (0, 3, 0, 0, 3, 0) and np.isnan(g["sensitivity"]) and g["precision"] == 0.0


def test_detection_counts_random():
    for seed in range(3):
        pred = U.blobs((17, 18, 33), seed=seed, classes=2, count=20, radius=(0, 2))
        lab = U.blobs((17, 18, 33), seed=100 + seed, classes=2, count=20, radius=(0, 2))
        for conn in (6, 26):
            for cls in (1, 2):
                check_detection(pred, lab, cls, conn, 1)
            check_detection(pred, lab, 1, conn, 4)


# ---------------------------------------------------------------------------------------------- integration
TODAY = {"confusion", "out_of_range", "dice", "iou", "sensitivity", "precision", "volume_pred", "volume_label", "hd", "hd_percentile",
         "assd", "nsd", "n_pred", "n_label", "classes", "spacing", "percentile", "tolerance"}


def test_evaluate_case_with_lesion_classes():
    pred = U.blobs((17, 18, 33), seed=1, classes=2, count=14, radius=(0, 2))
    lab = U.blobs((17, 18, 33), seed=2, classes=2, count=14, radius=(0, 2))
    p, g = dev(pred), dev(lab)
    plain = H.evaluate_case(p, g, 3)
    assert type(plain) is H.CaseMetrics and set(plain.to_host()) == TODAY
    m = H.evaluate_case(p, g, 3, lesion_classes=(1, 2))
    out = m.to_host()
    assert set(out) - TODAY == {"lesion_classes"} | {"lesion_" + k for k in ("n_label", "n_pred", "tp_label", "fn", "fp", "tp_pred",
                                                                             "sensitivity", "precision", "f1")}
    assert out["lesion_classes"] == (1, 2)
    for i, c in enumerate((1, 2)):
        alone = H.lesion_detection(p, g, c).to_host()
        mine = m.lesions[c].to_host()
        assert all(mine[k] == alone[k] or (np.isnan(mine[k]) and np.isnan(alone[k])) for k in alone), (mine, alone)
        assert counts_of(alone) == tuple(int(out["lesion_" + k][i]) for k in ("n_label", "n_pred", "tp_label", "fn", "fp", "tp_pred"))
        assert counts_of(alone) == counts_of(U.lesion_detection(pred, lab, c))
    for k in TODAY - {"classes", "spacing", "percentile", "tolerance"}:
        assert np.array_equal(np.asarray(out[k]), np.asarray(plain.to_host()[k]), equal_nan=True), k


def test_predictor_hooks():
    """The smallest real network of the blend tests.  result(postprocess=pp) and GridPredictor(..., postprocess=pp), blended and
    crop-stitched, equal pp applied by hand to the class channel of the unprocessed result; with None the result is today's."""
    ctor = dict(in_channels=1, out_channels=5, final_sigmoid=False, f_maps=[8, 16])
    nh, patch, ov, shape = 2, (16, 16, 16), (2, 3, 4), (21, 30, 19)
    img = (O._rng("predict:e2e").standard_normal((1,) + shape) * 2).astype(np.float16)
    pp = C.Postprocess(keep_largest=(1,), min_voxels={2: 3}, fill_holes=(0,), connectivity=6)
    with mednet_hip.precision("fp32"):
        net = O.keyed_init_(HM.ResidualUNet3D(**ctor)).to(DEV).eval()
        for blend in ("gaussian", None):
            kw = dict(num_heatmaps=nh, pad_mode="symmetric", batch_size=3, blend=blend)
            base = HP.GridPredictor(net, patch, ov, **kw)(img)
            again = HP.GridPredictor(net, patch, ov, postprocess=None, **kw)(img)
            assert torch.equal(base, again) and base.dtype == torch.uint8 and tuple(base.shape) == (nh + 1,) + shape
            want = base.clone()
            want[-1] = pp(base[-1])
            assert np.array_equal(host(want[-1]), U.postprocess(host(base[-1]), (1,), {2: 3}, (0,), 6))
            got = HP.GridPredictor(net, patch, ov, postprocess=pp, **kw)(img)
            assert torch.equal(got, want), blend
            if blend is not None:
                pred = HP.GridPredictor(net, patch, ov, **kw).predict(img)
                assert torch.equal(pred.result(), base) and torch.equal(pred.result(postprocess=None), base)
                assert torch.equal(pred.result(postprocess=pp), want)
