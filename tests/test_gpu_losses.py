"""The kernels at the end of every step at operator level (-m gpu): csrc/loss.hip (Dice, cross-entropy, heat-map regression: forward,
finalize, backward) and the Adam kernels of csrc/optim.hip, through the C ABI with every output pre-filled with NaN and a
workspace of exactly mednet_loss_ws_bytes (itself filled with NaN), at shapes that reach a second workgroup, a block boundary, a
ragged last block, more than 256 partial rows (the stride of the finalize kernels) and the unrolled loop of hm_finalize_kernel.

A. Exact inputs (gpu_util.hm_exact_case / ce_exact_case / dice_exact_case): every fp32 partial sum is exact in any order, so a
   dropped or doubled voxel, block or partial row changes bits.
     heat map   loss == tot = f32(tot + f32(w_c) * f32(S_c / count)) bit for bit; L1 gradient == +-scale and 0 where d = 0; L2
                gradient within 4 * 2^-24 |ref64|.
     CE         saved[0] == sum w_y, loss == f32(num64 / den64) bit for bit; NaN when every voxel is ignored, as in ATen.
     Dice       saved == the fp64 sums in every entry; dice_out within 2 * 2^-24 |dice64|; loss within (C + 4) 2^-24 (1 + max |dice64|).
B. Random logits against plain torch expressions / ATen in fp64 on the CPU: `saved` and the loss within 2^-18 * sum |terms|, the
   logit gradient per element within eps_case * (sum of its absolute terms) + 2^-126, eps_case = max(2^-20, 8 * r32) with r32 from
   ATen's own fp32 autograd against its fp64 one.
C. mednet_adam_step / mednet_adam_step_scaled: one step from a given state against gpu_util.adam_lines in fp64, bounds from the
   same lines in fp32; the scaler's state machine exactly.
D. Labels outside [0, C): what the kernels do is pinned.  E. int64 labels that do not fit an int count as out of range.
Every case prints one `[exact] item=loss ...` line with r32, the bound and the worst observed ratio; the worst per kernel are
recorded in profiles/loss_bounds.md.  tests/test_loss_util.py runs builders, references and checkers on the CPU."""
import functools

import numpy as np
import pytest
import torch

import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import ops

import gpu_util as U
from gpu_util import DEV, DT

pytestmark = pytest.mark.gpu
NAN = float("nan")
E_UNSUPPORTED = -5
SHAPES = {"tiny": (3, 7, 11),      # 231 voxels: under one trip of the voxel loop
          "block": (8, 16, 16),    # 2048: exactly one workgroup
          "plus1": (1, 3, 683),    # 2049: one voxel in the second workgroup
          "three": (5, 21, 41),    # 4305: three workgroups, the last holds 209 voxels and ends inside a trip
          "large": (65, 95, 97)}   # 598 975: 293 workgroups, ragged; n = 2 gives 586 partial rows
CLASSES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)
LABEL_LAYOUTS = ("i64", "u8", "u8vol")


def test_shapes_sit_where_the_plan_says():
    v = {k: int(np.prod(s)) for k, s in SHAPES.items()}
    B = U.LOSS_BLOCK_VOX
    assert v["tiny"] < 256 and v["block"] == B and v["plus1"] == B + 1
    assert 2 * B < v["three"] < 3 * B and (v["three"] - 2 * B) % 256 != 0
    nb = -(-v["large"] // B)
    assert nb == 293 and v["large"] % B != 0 and nb > 256 and 2 * nb > 512 and nb > 192 + 64
    for n, c, s in ((1, 1, v["tiny"]), (2, 4, v["large"]), (3, 300, v["block"])):
        assert L.lib().mednet_loss_ws_bytes(n, c, s) == (n * (-(-s // B)) * c * 2 + 64) * 4


# ------------------------------------------------------------------------------------------------ device side
def nan_dev(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def exact_ws(n, c, spatial):
    """A workspace of exactly mednet_loss_ws_bytes, every byte 0xFF (fp32 NaN): a partial row that is read but not written shows."""
    return torch.full((L.lib().mednet_loss_ws_bytes(n, c, spatial),), 255, dtype=torch.uint8, device=DEV)


class Placed:
    """Logits [n, c, S] on the device, contiguous or as channels 1 .. c of an n x (c + 2) x S tensor (stride_n = (c + 2) S), and a
    gradient buffer of the same layout filled with NaN."""

    def __init__(self, x, layout):
        n, c, S = x.shape
        self.lo, wide = (0, c) if layout == "contig" else (1, c + 2)
        self.full = torch.randn(n, wide, S, device=DEV)
        self.full[:, self.lo:self.lo + c] = x.to(DEV)
        self.gfull = nan_dev(n, wide, S)
        self.x, self.g = self.full[:, self.lo:self.lo + c], self.gfull[:, self.lo:self.lo + c]
        self.sn, self.sc, self.c = wide * S, S, c

    def outside_is_untouched(self):
        keep = torch.ones(self.gfull.shape[1], dtype=torch.bool, device=DEV)
        keep[self.lo:self.lo + self.c] = False
        return bool(torch.isnan(self.gfull[:, keep]).all())


def place_labels(lab, layout, tag):
    """int64 / uint8 labels [n, S], or uint8 labels as the last channel of an n x 3 x S volume.  -> (view, dtype code, stride_n)"""
    n, S = lab.shape
    if layout == "i64":
        return lab.to(DEV), L.I64, S
    if layout == "u8":
        return lab.to(torch.uint8).to(DEV), L.U8, S
    vol = torch.from_numpy(U._np_rng(tag + "vol").integers(0, 256, size=(n, 3, S)).astype(np.uint8))
    vol[:, 2] = lab.to(torch.uint8)
    vol = vol.to(DEV)
    return vol[:, 2], L.U8, 3 * S


def run_dice(P, lab, lab_dt, lab_sn, w, eps, sigmoid, ignore, dloss, bwd=True):
    n, c, S = P.x.shape
    lib = L.lib()
    loss, saved, dice, ws = nan_dev(), nan_dev(c, 2), nan_dev(c), exact_ws(n, c, S)
    ii = L.NO_IGNORE if ignore is None else int(ignore)
    wd = None if w is None else w.to(DEV)
    L.check(lib.mednet_dice_fwd_lt(P.x.data_ptr(), lab.data_ptr(), lab_dt, lab_sn, L.ptr(wd), loss.data_ptr(), saved.data_ptr(),
                                   dice.data_ptr(), n, c, S, P.sn, P.sc, eps, int(sigmoid), ii, ws.data_ptr(), ws.numel(), L.stream()),
            "dice_fwd_lt")
    if bwd:
        dl = torch.tensor(dloss, dtype=torch.float32, device=DEV)
        L.check(lib.mednet_dice_bwd_lt(P.x.data_ptr(), lab.data_ptr(), lab_dt, lab_sn, L.ptr(wd), saved.data_ptr(), dl.data_ptr(),
                                       P.g.data_ptr(), n, c, S, P.sn, P.sc, eps, int(sigmoid), ii, L.stream()), "dice_bwd_lt")
    torch.cuda.synchronize()
    return loss.cpu(), saved.cpu(), dice.cpu(), P.g.cpu()


def run_ce(P, lab, w, ignore, dloss, bwd=True):
    n, c, S = P.x.shape
    lib = L.lib()
    loss, saved, ws = nan_dev(), nan_dev(2), exact_ws(n, c, S)
    labd, wd = lab.to(DEV), None if w is None else w.to(DEV)
    assert wd is None or wd.numel() == c
    L.check(lib.mednet_ce_fwd(P.x.data_ptr(), labd.data_ptr(), L.ptr(wd), loss.data_ptr(), saved.data_ptr(), n, c, S, P.sn, P.sc,
                              int(ignore), ws.data_ptr(), ws.numel(), L.stream()), "ce_fwd")
    if bwd:
        dl = torch.tensor(dloss, dtype=torch.float32, device=DEV)
        L.check(lib.mednet_ce_bwd(P.x.data_ptr(), labd.data_ptr(), L.ptr(wd), saved.data_ptr(), dl.data_ptr(), P.g.data_ptr(), n, c, S,
                                  P.sn, P.sc, int(ignore), L.stream()), "ce_bwd")
    torch.cuda.synchronize()
    return loss.cpu(), saved.cpu(), P.g.cpu()


def run_hm(P, case, kind):
    n, c, S = P.x.shape
    lib = L.lib()
    vol = case.volume.to(DEV)
    tgt = vol[:, :-1]
    loss, ws = nan_dev(), exact_ws(n, c, S)
    w, dl = case.w.to(DEV), torch.tensor(case.dloss, dtype=torch.float32, device=DEV)
    k, u8 = (L.REG_L2 if kind == "L2" else L.REG_L1), int(case.tgt == "u8")
    L.check(lib.mednet_heatmap_loss_fwd_strided(P.x.data_ptr(), tgt.data_ptr(), (c + 1) * S, w.data_ptr(), loss.data_ptr(), n, c, S, P.sn,
                                                P.sc, k, u8, ws.data_ptr(), ws.numel(), L.stream()), "heatmap_loss_fwd")
    L.check(lib.mednet_heatmap_loss_bwd_strided(P.x.data_ptr(), tgt.data_ptr(), (c + 1) * S, w.data_ptr(), dl.data_ptr(), P.g.data_ptr(),
                                                n, c, S, P.sn, P.sc, k, u8, L.stream()), "heatmap_loss_bwd")
    torch.cuda.synchronize()
    return loss.cpu(), P.g.cpu()


def layouts_for(key):
    return ("contig",) if key == "large" else ("contig", "slice")   # (the large shape stays at 19 MB per tensor)


# ================================================================================================ A.1 heat map
HM_CASES = [(k, 1 + i % 3, c, ("u8", "f32")[(i + j) % 2]) for j, k in enumerate(("tiny", "block")) for i, c in enumerate((1, 3, 16, 17, 300))] \
    + [("plus1", 2, 3, "u8"), ("three", 3, 3, "f32"), ("three", 2, 3, "u8"), ("large", 2, 3, "u8"), ("large", 1, 3, "f32")]


@functools.lru_cache(maxsize=2)
def hm_case(key, n, c, tgt):
    case = U.hm_exact_case(f"hm{key}{n}{c}{tgt}", n, c, SHAPES[key], tgt)
    return case, {kind: U.hm_reference(case, kind) for kind in ("L2", "L1")}


@pytest.mark.parametrize("key,n,c,tgt", HM_CASES)
def test_heatmap_loss_on_integers_is_exact(key, n, c, tgt):
    case, refs = hm_case(key, n, c, tgt)
    x = case.out.reshape(n, c, -1)
    worst = 0.0
    for layout in layouts_for(key):
        for kind in ("L2", "L1"):
            P = Placed(x, layout)
            loss, dout = run_hm(P, case, kind)
            what = f"heat map {kind} {key} n={n} c={c} target={tgt} {layout}"
            worst = max(worst, U.check_hm(case, refs[kind], loss, dout, what))
            assert P.outside_is_untouched(), what + ": the gradient buffer was written outside the channel slice"
    print(f"[exact] item=loss heat map {key} n={n} c={c} target={tgt} kernel=hm_fwd_kernel,hm_finalize_kernel,hm_bwd_kernel loss: bit-exact "
          f"L1: bit-exact L2 dout: bound {4 * U.U32:.2e} seen {worst:.2e}")


# ================================================================================================ A.2 cross-entropy
CE_CASES = [("three", 1 + i % 3, c, (-100, 1)[i % 2] if c > 1 else -100, "some") for i, c in enumerate(CLASSES)] \
    + [(k, 1 + i % 3, 5, -100, "some") for i, k in enumerate(("tiny", "block", "plus1"))] \
    + [("large", 2, 2, -100, "some"), ("large", 2, 4, 3, "some"), ("three", 2, 5, -100, "sample"), ("three", 2, 5, 2, "all"),
       ("large", 2, 4, -100, "sample")]


@pytest.mark.parametrize("key,n,c,ignore,ignored", CE_CASES)
def test_cross_entropy_on_exact_terms_is_exact(key, n, c, ignore, ignored):
    case = U.ce_exact_case(f"ce{key}{n}{c}{ignored}", n, c, SHAPES[key], ignore, ignored)
    ref = U.ce_exact_reference(case)
    assert np.isnan(ref.loss32) == (ignored == "all")
    for layout in layouts_for(key):
        P = Placed(case.lg, layout)
        loss, saved, _ = run_ce(P, case.lab, case.w, ignore, 1.0, bwd=False)
        U.check_ce_exact(ref, loss, saved[0], f"CE {key} n={n} C={c} ignore={ignore} ({ignored}) {layout}")
    print(f"[exact] item=loss CE exact {key} n={n} C={c} ignore={ignore} ({ignored}) kernel=class_loss_fwd_kernel<CE>,ce_finalize_kernel "
          f"saved[0]: bit-exact loss: bit-exact ({ref.loss32!r})")


# ================================================================================================ A.3 Dice
DICE_CASES = [("three", 1 + i % 3, c) for i, c in enumerate(CLASSES)] + [(k, 1 + i % 3, 4) for i, k in enumerate(("tiny", "block", "plus1"))] \
    + [("large", 2, 2), ("large", 2, 4)]


@pytest.mark.parametrize("sigmoid", [False, True])
@pytest.mark.parametrize("key,n,c", DICE_CASES)
def test_dice_on_dyadic_probabilities_is_exact(key, n, c, sigmoid):
    case = U.dice_exact_case(f"dx{key}{n}{c}{int(sigmoid)}", n, c, SHAPES[key], sigmoid)
    assert n * case.spatial <= 1.2e6
    worst, i = 0.0, 0
    for ignore in (None, 0, 1):
        ref = U.dice_exact_reference(case, ignore)
        for layout in layouts_for(key):
            lab, lab_dt, lab_sn = place_labels(case.lab, LABEL_LAYOUTS[i % 3], f"dx{key}{c}")
            i += 1
            P = Placed(case.lg, layout)
            loss, saved, dice, _ = run_dice(P, lab, lab_dt, lab_sn, case.w, case.eps, sigmoid, ignore, 1.0, bwd=False)
            what = f"Dice exact {key} n={n} C={c} sigmoid={int(sigmoid)} ignore={ignore} {layout} labels={LABEL_LAYOUTS[(i - 1) % 3]}"
            worst = max(worst, U.check_dice_exact(case, ref, saved, dice, loss, what))
    print(f"[exact] item=loss Dice exact {key} n={n} C={c} sigmoid={int(sigmoid)} kernel=class_loss_fwd_kernel<DICE>,dice_finalize_kernel saved: bit-exact "
          f"loss: bound {c + 4} roundings seen {worst:.2f}")


# ================================================================================================ B. random logits
RANDOM_CASES = [("three", 1 + i % 3, c, c in (4, 17)) for i, c in enumerate(CLASSES)] \
    + [(k, 1 + i % 3, 3, False) for i, k in enumerate(("tiny", "block", "plus1"))] + [("large", 2, 2, False), ("large", 2, 4, True)]


@functools.lru_cache(maxsize=2)
def random_case(key, n, c, edge):
    return U.loss_random_case(f"rnd{key}{n}{c}", n, c, SHAPES[key], edge)


def dice_variants(key, c):
    """(sigmoid, ignore_index): all six at the small shapes, two at the large one (the fp64 reference costs a second there)."""
    if key == "large":
        return [(False, None), (True, 1)] if c == 2 else [(False, 0), (True, None)]
    return [(s, ig) for s in (False, True) for ig in (None, 0, 1)]


@pytest.mark.parametrize("key,n,c,edge", RANDOM_CASES)
def test_dice_against_fp64_per_element(key, n, c, edge):
    case = random_case(key, n, c, edge)
    i = 0
    for sigmoid, ignore in dice_variants(key, c):
        r64, r32 = U.dice_chain(case, sigmoid, ignore, torch.float64), U.dice_chain(case, sigmoid, ignore, torch.float32)
        if edge and c > 2:
            assert float(r64.saved[c - 1, 1]) < case.eps, "the dead channel's D must lie below eps"
        norm = U.dice_grad_norm(case, r64, sigmoid)
        what = f"Dice {key} n={n} C={c} sigmoid={int(sigmoid)} ignore={ignore} edge={int(edge)}"
        e32, eps_case = U.loss_grad_eps(r32.dlg, r64.dlg, norm, what)
        layout = layouts_for(key)[i % len(layouts_for(key))]
        lab, lab_dt, lab_sn = place_labels(case.lab, LABEL_LAYOUTS[i % 3], f"rnd{key}{c}")
        i += 1
        P = Placed(case.lg, layout)
        loss, saved, _, dlg = run_dice(P, lab, lab_dt, lab_sn, case.w, case.eps, sigmoid, ignore, case.dloss)
        seen = U.check_dice_random(case, r64, norm, eps_case, saved, loss, dlg, what + " " + layout)
        assert P.outside_is_untouched(), what + ": the gradient buffer was written outside the channel slice"
        print(f"[exact] item=loss {what} {layout} kernel=class_loss_fwd_kernel<DICE>,dice_finalize_kernel,class_loss_bwd_kernel<DICE> saved: bound {U.LOSS_SUM_BOUND:.2e} "
              f"seen {seen['saved']:.2e} loss: seen {seen['loss']:.2e} dlogits: r32 {e32:.2e} eps {eps_case:.2e} seen {seen['dlg']:.2e}")


@pytest.mark.parametrize("key,n,c,edge", [t for t in RANDOM_CASES if t[2] > 1])
def test_cross_entropy_against_fp64_per_element(key, n, c, edge):
    case = random_case(key, n, c, edge)
    ignores = (-100,) if key == "large" else (-100, c - 1)
    for i, ignore in enumerate(ignores):
        r64, r32 = U.ce_chain(case, ignore, torch.float64), U.ce_chain(case, ignore, torch.float32)
        what = f"CE {key} n={n} C={c} ignore={ignore} edge={int(edge)}"
        e32, eps_case = U.loss_grad_eps(r32.dlg, r64.dlg, r64.norm, what)
        layout = layouts_for(key)[i % len(layouts_for(key))]
        P = Placed(case.lg, layout)
        loss, saved, dlg = run_ce(P, U.ce_labels(case, ignore), case.w, ignore, case.dloss)
        seen = U.check_ce_random(case, r64, eps_case, saved[0], loss, dlg, what + " " + layout)
        assert P.outside_is_untouched(), what + ": the gradient buffer was written outside the channel slice"
        print(f"[exact] item=loss {what} {layout} kernel=class_loss_fwd_kernel<CE>,ce_finalize_kernel,class_loss_bwd_kernel<CE> saved: bound {U.LOSS_SUM_BOUND:.2e} "
              f"seen {seen['saved']:.2e} loss: seen {seen['loss']:.2e} dlogits: r32 {e32:.2e} eps {eps_case:.2e} seen {seen['dlg']:.2e}")


def test_more_than_32_classes_are_refused_and_nothing_is_written():
    n, c, S = 1, 33, 231
    lib = L.lib()
    x, lab = torch.zeros(n, c, S, device=DEV), torch.zeros(n, S, dtype=torch.int64, device=DEV)
    loss, saved, g, ws = nan_dev(), nan_dev(c, 2), nan_dev(n, c, S), exact_ws(n, c, S)
    dl = torch.ones((), device=DEV)
    rcs = [lib.mednet_dice_fwd_lt(x.data_ptr(), lab.data_ptr(), L.I64, S, None, loss.data_ptr(), saved.data_ptr(), None, n, c, S, c * S, S,
                                  1e-5, 0, L.NO_IGNORE, ws.data_ptr(), ws.numel(), L.stream()),
           lib.mednet_dice_bwd_lt(x.data_ptr(), lab.data_ptr(), L.I64, S, None, saved.data_ptr(), dl.data_ptr(), g.data_ptr(), n, c, S, c * S, S,
                                  1e-5, 0, L.NO_IGNORE, L.stream()),
           lib.mednet_ce_fwd(x.data_ptr(), lab.data_ptr(), None, loss.data_ptr(), saved.data_ptr(), n, c, S, c * S, S, -100, ws.data_ptr(),
                             ws.numel(), L.stream()),
           lib.mednet_ce_bwd(x.data_ptr(), lab.data_ptr(), None, saved.data_ptr(), dl.data_ptr(), g.data_ptr(), n, c, S, c * S, S, -100,
                             L.stream())]
    torch.cuda.synchronize()
    assert rcs == [E_UNSUPPORTED] * 4
    for t in (loss, saved, g):
        assert bool(torch.isnan(t).all())
    assert bool((ws == 255).all())


# ---------------------------------------------------------------------------------------------- once through the wrappers
def test_ops_wrappers_pass_the_strides_of_slices_and_label_volumes():
    """ops.heatmap_loss / ops.dice_loss / ops.cross_entropy on a channel slice of a wider 5-d tensor, heat-map targets as [:, :-1] and
    uint8 labels as the last channel of a label volume: the same exact references as the ABI calls."""
    key, n = "three", 2
    shape = SHAPES[key]
    # heat map: out is channels 1 .. c of a wider tensor
    case, refs = hm_case(key, n, 3, "u8")
    for kind in ("L2", "L1"):
        wide = torch.randn(n, 5, *shape, device=DEV)
        wide[:, 1:4] = case.out.to(DEV)
        wide.requires_grad_(True)
        loss = ops.heatmap_loss(wide[:, 1:4], case.volume.to(DEV)[:, :-1], case.w.to(DEV), kind)
        (loss * case.dloss).backward()
        U.check_hm(case, refs[kind], loss.detach().cpu(), wide.grad[:, 1:4].cpu(), f"ops.heatmap_loss {kind}")
        assert int(torch.count_nonzero(wide.grad[:, 0])) == 0 and int(torch.count_nonzero(wide.grad[:, 4])) == 0
    # Dice: exact sums, uint8 labels where they lie in a volume; random logits for the gradient
    dc = U.dice_exact_case("opsdice", n, 4, shape, False)
    vol = torch.zeros(n, 2, *shape, dtype=torch.uint8)
    vol[:, 1] = dc.lab.reshape(n, *shape).to(torch.uint8)
    wide = torch.randn(n, 6, *shape, device=DEV)
    wide[:, 2:] = dc.lg.reshape(n, 4, *shape).to(DEV)
    loss = ops.dice_loss(wide[:, 2:], vol.to(DEV)[:, 1], dc.w.to(DEV), dc.eps, False, 1)
    ref = U.dice_exact_reference(dc, 1)
    unit = U.U32 * (1.0 + float(ref.dice64.abs().max()))
    assert abs(float(loss) - ref.loss64) <= (4 + 4) * unit
    rc = random_case(key, n, 4, True)
    r64, r32 = U.dice_chain(rc, False, 1, torch.float64), U.dice_chain(rc, False, 1, torch.float32)
    norm = U.dice_grad_norm(rc, r64, False)
    _, eps_case = U.loss_grad_eps(r32.dlg, r64.dlg, norm, "ops.dice_loss")
    vol[:, 1] = rc.lab.reshape(n, *shape).to(torch.uint8)
    wide = torch.randn(n, 6, *shape, device=DEV)
    wide[:, 2:] = rc.lg.reshape(n, 4, *shape).to(DEV)
    wide.requires_grad_(True)
    loss = ops.dice_loss(wide[:, 2:], vol.to(DEV)[:, 1], rc.w.to(DEV), rc.eps, False, 1)
    (loss * rc.dloss).backward()
    U.check_loss_scalar(loss.detach().cpu(), r64.loss, float((1.0 + r64.dice.abs()).mean()), "ops.dice_loss: loss")
    U.check_gradient(wide.grad[:, 2:].cpu().reshape(n, 4, -1), r64.dlg, norm, eps_case, "ops.dice_loss: dlogits", s=U.F32_TINY)
    assert int(torch.count_nonzero(wide.grad[:, :2])) == 0
    # cross-entropy: exact terms on a slice
    cc = U.ce_exact_case("opsce", n, 5, shape, 1, "sample")
    wide = torch.randn(n, 7, *shape, device=DEV)
    wide[:, 1:6] = cc.lg.reshape(n, 5, *shape).to(DEV)
    loss = ops.cross_entropy(wide[:, 1:6], cc.lab.reshape(n, *shape).to(DEV), cc.w.to(DEV), 1)
    U.assert_same_f32(U.f32_scalar(loss), U.ce_exact_reference(cc).loss32, "ops.cross_entropy: loss")
    r64, r32 = U.ce_chain(rc, -100, torch.float64), U.ce_chain(rc, -100, torch.float32)
    _, eps_case = U.loss_grad_eps(r32.dlg, r64.dlg, r64.norm, "ops.cross_entropy")
    wide = torch.randn(n, 6, *shape, device=DEV)
    wide[:, 2:] = rc.lg.reshape(n, 4, *shape).to(DEV)
    wide.requires_grad_(True)
    loss = ops.cross_entropy(wide[:, 2:], U.ce_labels(rc, -100).reshape(n, *shape).to(DEV), rc.w.to(DEV), -100)
    (loss * rc.dloss).backward()
    U.check_loss_scalar(loss.detach().cpu(), r64.loss, r64.loss_terms, "ops.cross_entropy: loss")
    U.check_gradient(wide.grad[:, 2:].cpu().reshape(n, 4, -1), r64.dlg, r64.norm, eps_case, "ops.cross_entropy: dlogits", s=U.F32_TINY)


# ================================================================================================ C. Adam
ADAM_LARGE = 2 * 2097152 + 1027
ADAM_COUNTS = (1, 255, 257, 10007, ADAM_LARGE)
ADAM_ALL = [(step, wd, gs) for step in (1, 2, 5, 1000) for wd in (0.0, 0.01) for gs in (1.0, 0.125, 1.0 / 3.0)]
ADAM_FEW = [(2, 0.01, 0.125), (5, 0.0, 1.0 / 3.0), (1000, 0.01, 1.0)]   # at the large count: a second of fp64 each


@functools.lru_cache(maxsize=1)
def adam_state(count):
    return U.adam_case(f"adam{count}", count)


def dev_state(case):
    return tuple(t.to(DEV).clone() for t in (case.p, case.g, case.m, case.v))


def report_adam(what, kernel, ref, seen):
    print(f"[exact] item=loss Adam {what} kernel={kernel} "
          + " ".join(f"{k}: r32 {ref.r32s[k]:.2e} eps {ref.eps[k]:.2e} seen {seen[k]:.2e}" for k in ("m", "v", "p", "pt")))


@pytest.mark.parametrize("count", ADAM_COUNTS)
def test_adam_step_against_fp64_per_element(count):
    case = adam_state(count)
    hp = U.ADAM_HP
    for step, wd, gs in (ADAM_FEW if count == ADAM_LARGE else ADAM_ALL):
        ref = U.adam_reference(case, wd, step, gs)
        p, g, m, v = dev_state(case)
        if (step, wd) == (2, 0.01):     # once through the wrapper
            ops.adam_step_(p, g, m, v, hp["lr"], hp["b1"], hp["b2"], hp["eps"], wd, step, gs)
        else:
            L.check(L.lib().mednet_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), count, hp["lr"], hp["b1"], hp["b2"],
                                             hp["eps"], wd, step, gs, L.stream()), "adam_step")
        torch.cuda.synchronize()
        assert torch.equal(g.cpu(), case.g), "the gradient was written"
        what = f"count={count} step={step} wd={wd} grad_scale={gs:.4f}"
        report_adam(what, "adam_kernel", ref, U.check_adam(ref, p.cpu(), m.cpu(), v.cpu(), "Adam " + what))


def scaled_step(p, g, m, v, state, wd, inv_world, growth=2.0, backoff=0.5, interval=3):
    hp = U.ADAM_HP
    L.check(L.lib().mednet_adam_step_scaled(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), hp["lr"], hp["b1"], hp["b2"],
                                            hp["eps"], wd, inv_world, state.data_ptr(), growth, backoff, interval, L.stream()),
            "adam_step_scaled")
    torch.cuda.synchronize()


def scaler_state(scale, good, steps, skipped):
    return torch.tensor([scale, good, steps, 0.0, skipped, 0.0, 0.0, 0.0], dtype=torch.float32, device=DEV)


def test_scaled_adam_clean_step_meets_the_same_bounds():
    case = adam_state(ADAM_LARGE)
    scale, inv_world, wd, steps = 1024.0, 0.125, 0.01, 4
    ref = U.adam_reference(case, wd, steps + 1, inv_world / scale)
    p, g, m, v = dev_state(case)
    state = scaler_state(scale, 1.0, float(steps), 7.0)
    scaled_step(p, g, m, v, state, wd, inv_world)
    assert state.cpu().tolist() == [scale, 2.0, steps + 1.0, 0.0, 7.0, 0.0, 0.0, 0.0]
    what = f"scaled count={ADAM_LARGE} step={steps + 1} wd={wd} scale={scale} inv_world={inv_world}"
    report_adam(what, "grad_check_kernel,adam_scaled_kernel,scaler_update_kernel", ref, U.check_adam(ref, p.cpu(), m.cpu(), v.cpu(), what))


@pytest.mark.parametrize("where", ["first", "last"])
def test_scaled_adam_overflow_step_leaves_the_state_untouched(where):
    """One +-inf or NaN in the first element or in the last one (inside the tail of the grid-stride loop): p, m, v keep their bits,
    the scale backs off, the good-step count returns to 0, the step count stays and one more step counts as skipped."""
    case = adam_state(ADAM_LARGE)
    for bad in (float("inf"), float("-inf"), NAN):
        p, g, m, v = dev_state(case)
        g[0 if where == "first" else ADAM_LARGE - 1] = bad
        state = scaler_state(1024.0, 2.0, 4.0, 7.0)
        scaled_step(p, g, m, v, state, 0.01, 0.125)
        for got, want, name in ((p, case.p, "p"), (m, case.m, "m"), (v, case.v, "v")):
            assert torch.equal(got.cpu(), want), f"{name} changed in a step with g[{where}] = {bad}"
        assert state.cpu().tolist() == [512.0, 0.0, 4.0, 0.0, 8.0, 0.0, 0.0, 0.0], (where, bad)


def test_scaler_grows_after_the_interval_and_never_falls_below_one():
    case = adam_state(257)
    p, g, m, v = dev_state(case)
    state = scaler_state(1024.0, 0.0, 0.0, 0.0)
    want = [[1024.0, 1.0, 1.0], [1024.0, 2.0, 2.0], [2048.0, 0.0, 3.0], [2048.0, 1.0, 4.0]]   # growth after exactly 3 good steps
    for w3 in want:
        scaled_step(p, g, m, v, state, 0.0, 1.0, interval=3)
        assert state.cpu().tolist() == w3 + [0.0, 0.0, 0.0, 0.0, 0.0]
    g[5] = float("inf")
    for start, after in ((1.5, 1.0), (1.0, 1.0), (4.0, 2.0)):
        state = scaler_state(start, 2.0, 9.0, 0.0)
        scaled_step(p, g, m, v, state, 0.0, 1.0)
        assert state.cpu().tolist() == [after, 0.0, 9.0, 0.0, 1.0, 0.0, 0.0, 0.0]


# ================================================================================================ D, E. labels outside [0, C)
BIG = 2 ** 32
BAD_I64 = (4, -1, BIG + 1, -BIG + 1)     # 2^32 + 1 and -2^32 + 1 narrow to class 1: they are out of range like 4 and -1


def bad_label_case():
    """Three workgroups; the bad voxel sits in the last, ragged one, in sample 1, behind a voxel that cross-entropy does not ignore."""
    case = random_case("three", 2, 4, False)
    bn = 1
    ok = ~case.ign[bn] & (case.lab[bn] != 3)
    bv = max(v for v in range(2 * U.LOSS_BLOCK_VOX + 1, case.spatial) if bool(ok[v]) and bool(ok[v - 1]))
    return case, (bn, bv)


@pytest.mark.parametrize("sigmoid", [False, True])
def test_dice_out_of_range_label_poisons_loss_and_gradient(sigmoid):
    """The reference raises on a label outside [0, C); a kernel cannot without a host synchronisation per step, so the Dice loss turns
    NaN, and with it the gradient: every element for softmax, all of channel 0 -- the channel that carries the poison -- for sigmoid,
    whose other channels stay finite.  (The docstring of test_gpu_ops.test_out_of_range_labels_poison_the_loss says "loss and every
    gradient"; for the sigmoid form and for cross-entropy that is not what the kernels do, see the next test.)"""
    case, (bn, bv) = bad_label_case()
    for layout, values in (("i64", BAD_I64), ("u8", (4, 255))):
        for bad in values:
            lab = case.lab.clone()
            lab[bn, bv] = bad
            labd, lab_dt, lab_sn = place_labels(lab, layout, "bad")
            P = Placed(case.lg, "contig")
            loss, saved, dice, dlg = run_dice(P, labd, lab_dt, lab_sn, case.w, case.eps, sigmoid, None, 1.0)
            what = f"Dice sigmoid={int(sigmoid)} label {bad} ({layout})"
            assert bool(torch.isnan(loss)), what + ": the loss is not NaN"
            if sigmoid:
                assert bool(torch.isnan(dlg[:, 0]).all()) and bool(torch.isfinite(dlg[:, 1:]).all()), what
            else:
                assert bool(torch.isnan(dlg).all()), what + ": a gradient element is not NaN"


def test_cross_entropy_out_of_range_label_poisons_the_loss_only():
    """Cross-entropy: the loss is NaN; the gradient stays finite and the rows of the bad voxel are 0 (in training the NaN loss reaches
    every gradient through the loss scalar).  weight[] has exactly C elements and is not indexed with the bad value.  A label of
    2^32 - 100 is not ignore_index -100."""
    case, (bn, bv) = bad_label_case()
    for ignore, values in ((-100, BAD_I64 + (BIG - 100,)), (3, BAD_I64)):
        for bad in values:
            lab = U.ce_labels(case, ignore)
            lab[bn, bv] = bad
            P = Placed(case.lg, "contig")
            loss, saved, dlg = run_ce(P, lab, case.w, ignore, 1.0)
            what = f"CE ignore={ignore} label {bad}"
            assert bool(torch.isnan(loss)), what + ": the loss is not NaN"
            assert bool(torch.isfinite(saved[0])) and bool(torch.isfinite(dlg).all()), what
            assert int(torch.count_nonzero(dlg[bn, :, bv])) == 0, what + ": the bad voxel has a gradient"
            assert int(torch.count_nonzero(dlg[bn, :, bv - 1])) > 0


@pytest.mark.parametrize("kind", ["DICE", "CE"])
def test_fused_small_heads_treat_a_wide_int64_label_as_out_of_range(kind):
    """mednet_head_dice_fwd / mednet_head_ce_fwd (head_loss.hip label_at): finite with good labels, NaN with 2^32 + 1 or -2^32 + 1."""
    import test_gpu_head_backward as H
    mode, cin, cout, n, shape = "bf16", 16, 4, 2, (5, 7, 33)
    dt, dcode, lib = DT[mode], L.dt_of(DT[mode]), L.lib()
    S = int(np.prod(shape))
    z = H.act_output(U.rnd("wide64u", n, cin, *shape), L.ACT_ELU, mode)
    zg, gyg = H.to_dev_cl(z, dt), H.to_dev_cl(U.half_round(U.rnd("wide64y", n, cin, *shape), mode), dt)
    dl = torch.tensor(1.0, dtype=torch.float32, device=DEV)
    good = torch.from_numpy(np.random.Generator(np.random.PCG64(4)).integers(0, cout, size=(n,) + shape))
    with mednet_hip.precision(mode):
        pk = ops.pack_conv_weight(U.rnd("wide64w", cout, cin, 1, 1, 1, scale=0.3).to(DEV), 1, False)
        b, wt = U.rnd("wide64b", cout).to(DEV), torch.tensor(H.A_WEIGHT[:cout], device=DEV)
        ii = L.NO_IGNORE if kind == "DICE" else -100
        for bad in (None, BIG + 1, -BIG + 1):
            lab = good.clone()
            if bad is not None:
                lab[1, 4, 6, 30] = bad
            out = H._fused(lib, kind, zg, pk, b, lab.to(DEV), L.I64, S, wt, gyg, L.ACT_ELU, n, shape, cin, cout, dcode, dl, 1e-5, False, ii, dt)
            torch.cuda.synchronize()
            assert bool(torch.isnan(out[1])) == (bad is not None), f"{kind} head, label {bad}: loss {float(out[1])}"
