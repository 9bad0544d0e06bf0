"""Resampling on the GPU (csrc/resample.hip, mednet_hip.resample) against the numpy model of tests/resample_util.py: bit-equal
where the arithmetic is exact, within the derived bound of profiles/resample_bounds.md elsewhere (the bound comes from the chain
lengths, the unit roundoff and the sum of |w| |v| per element; the observed fractions are printed, pytest -s shows them), the fused
arg-max bit-equal to the three passes, guard bands around hostile tables, and the predictor's way to the network's grid and back.

Largest observed fractions of the bound (MI355X): see profiles/resample_bounds.md."""
import numpy as np
import pytest
import torch

import mednet_hip
import resample_util as R
from mednet_hip import predict as HP
from mednet_hip import resample as M
from mednet_hip.unet import model as HM
from oracle import ref_cpu as O

from fence import Fence
from gpu_util import DEV

pytestmark = pytest.mark.gpu

TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "u8": torch.uint8}


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def tables(shape, size, kind, aa):
    return [M.axis_table(n, m, kind, aa) for n, m in zip(shape, size)]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---------------------------------------------------------------------------------------------- 1. exact cases
@pytest.mark.parametrize("size", [(16, 24, 32), (4, 6, 8), (16, 6, 32)])
def test_integer_lattice_equals_fp64_bit_for_bit(size):
    """Integers in [-512, 512], x2 up and / 2 anti-aliased down (dyadic weights): every product and partial sum is an fp32 number."""
    shape = (8, 12, 16)
    vol = R.integer_volume(11, (2,) + shape)
    want = R.resample64(vol, tables(shape, size, "linear", True))
    got = M.resample(dev(vol), size=size)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2,) + size
    R.check_exact(host(got), want, f"{shape} -> {size}")
    R.check_exact(host(M.resample(dev(vol)[1], size=size)), want[1], f"D x H x W {shape} -> {size}")
    R.check_exact(host(M.resample(dev(vol).half(), size=size, dtype=torch.float32)), want, f"f16 source {shape} -> {size}")


@pytest.mark.parametrize("dt", ["f32", "f16", "u8"])
def test_identity_sizes_return_the_input_bits(dt):
    shape = (5, 6, 7)
    vol = dev(R.random_volume(12, (2,) + shape, dt))
    for kind in ("nearest", "linear", "cubic"):
        got = M.resample(vol, size=shape, kind=kind)
        assert same_bits(got, vol) and got.data_ptr() != vol.data_ptr()
        assert same_bits(M.resample(vol, spacing=(2, 1, 0.5), target_spacing=(2, 1, 0.5), kind=kind), vol)
    if dt == "f32":     # another dtype: the store's one rounding
        assert same_bits(M.resample(vol, size=shape, dtype=torch.float16), vol.half())
        assert np.array_equal(host(M.resample(vol * 100, size=shape, dtype=torch.uint8)), R.store_u8(host(vol * 100)))


@pytest.mark.parametrize("shape,size", [((12, 10, 14), (19, 23, 17)), ((33, 35, 130), (16, 18, 65)), ((5, 6, 7), (7, 5, 3)), ((1, 5, 1), (3, 1, 4))])
def test_nearest_equals_numpy_indexing(shape, size):
    for dt in ("u8", "f32", "f16"):
        vol = R.random_volume(13, (2,) + shape, dt)
        iz, iy, ix = (np.minimum(np.floor((np.arange(m) + 0.5) * (n / m)).astype(np.int64), n - 1) for n, m in zip(shape, size))
        want = vol[:, iz][:, :, iy][:, :, :, ix]
        got = M.resample(dev(vol), size=size, kind="nearest")
        assert np.array_equal(host(got), want), (dt, shape, size)
    lab = R.blob_labels(14, 5, shape, special=(255,))
    assert np.array_equal(host(M.resample_labels(dev(lab), size=size, kind="nearest")), lab[iz][:, iy][:, :, ix])


# ---------------------------------------------------------------------------------------------- 2. bounded cases
SHAPES = {"up": ((12, 10, 14), (19, 23, 17), 3), "down-ragged": ((33, 35, 130), (16, 18, 65), 1), "cubic-7x": ((29, 9, 9), (4, 9, 9), 1),
          "ones-in": ((1, 5, 1), (3, 1, 4), 3), "ones-out": ((6, 1, 7), (1, 4, 2), 1), "narrow": ((5, 6, 7), (7, 5, 3), 3),
          "thick": ((20, 11, 13), (9, 17, 30), 2)}      # z shrinks (the tap loop), x grows (its 4-wide loads)
KINDS = [("linear", True), ("linear", False), ("cubic", True), ("cubic", False)]


@pytest.mark.parametrize("kind,aa", KINDS, ids=[f"{k}-{'aa' if a else 'point'}" for k, a in KINDS])
@pytest.mark.parametrize("case", list(SHAPES))
def test_random_volumes_within_the_derived_bound(case, kind, aa):
    """Every element against the fp64 model run with the fp32 table values; f16 and u8 stores add exactly one rounding."""
    shape, size, c = SHAPES[case]
    tabs = tables(shape, size, kind, aa)
    if case == "cubic-7x" and kind == "cubic" and aa:
        assert tabs[0][3] >= 24          # a 7.25-fold stretch of the 4-wide Keys kernel, cut by the 29 voxels there are
    for dt in ("f32", "f16", "u8"):
        vol = R.random_volume(21, (c,) + shape, dt)
        ref = R.resample64(vol, tabs)
        bound = R.error_bound(vol, tabs)
        out32 = M.resample(dev(vol), size=size, kind=kind, antialias=aa, dtype=torch.float32)
        frac = R.check_bounded(host(out32), ref, bound, f"{case} {kind} aa={aa} {dt}")
        print(f"[resample] {case} {kind} aa={aa} {dt}: largest observed fraction of the bound {frac:.3f}")
        out16 = M.resample(dev(vol), size=size, kind=kind, antialias=aa, dtype=torch.float16)
        assert same_bits(out16, out32.half()), f"{case} {kind} {dt}: the f16 store is not one round-to-nearest-even of the fp32 result"
        R.check_bounded(host(out16), ref, bound, f"{case} {kind} aa={aa} {dt} -> f16", rel=R.U16, absolute=R.F16_TINY)
        scale = 1.0 if dt == "u8" else 60.0
        src = dev(vol) if dt == "u8" else (dev(vol).float() * scale + 100.0).to(TORCH_DT[dt])
        out8 = M.resample(src, size=size, kind=kind, antialias=aa, dtype=torch.uint8)
        ref8 = M.resample(src, size=size, kind=kind, antialias=aa, dtype=torch.float32)
        assert np.array_equal(host(out8), R.store_u8(host(ref8))), f"{case} {kind} {dt}: the u8 store is not clamp + rint of the fp32 result"
        if dt == "u8":
            R.check_bounded(host(out8), np.clip(ref, 0, 255), bound, f"{case} {kind} aa={aa} u8 -> u8", absolute=0.5)
        default = M.resample(dev(vol), size=size, kind=kind, antialias=aa)
        assert default.dtype == TORCH_DT[dt] and same_bits(default, {"f32": out32, "f16": out16, "u8": out8}[dt])


# ---------------------------------------------------------------------------------------------- 3. fused against the passes
def first_argmax(planes):
    """argmax_first of volume.h on the device: a later class wins only with a strictly larger score."""
    best, arg = planes[0].clone(), torch.zeros(planes.shape[1:], dtype=torch.uint8, device=planes.device)
    for c in range(1, planes.shape[0]):
        m = planes[c] > best
        arg = torch.where(m, torch.full_like(arg, c), arg)
        best = torch.where(m, planes[c], best)
    return arg, best


def three_passes(planes, size, kind, aa):
    return M.resample(planes, size=size, kind=kind, antialias=aa, dtype=torch.float32)


FUSED_KINDS = [("linear", True), ("cubic", True), ("linear", False)]


@pytest.mark.parametrize("kind,aa", FUSED_KINDS, ids=[f"{k}-{'aa' if a else 'point'}" for k, a in FUSED_KINDS])
@pytest.mark.parametrize("case", list(SHAPES))
def test_fused_argmax_equals_the_three_passes_bit_for_bit(case, kind, aa):
    """out and out_max against argmax_first over the three-pass fp32 results: every voxel, both source forms."""
    shape, size, _ = SHAPES[case]
    g = torch.Generator(device=DEV).manual_seed(31)
    for ncls in (1, 2, 4, 17, 256):
        planes = torch.softmax(2.0 * torch.randn((ncls,) + shape, device=DEV, generator=g), 0)
        if ncls >= 4:
            planes[1] = planes[0]                      # exact ties of the two lowest classes
        for src in (planes, planes.half()):
            want, want_max = first_argmax(three_passes(src, size, kind, aa))
            got, got_max = M.resample_argmax(src, size=size, kind=kind, antialias=aa, return_max=True)
            assert got.dtype == torch.uint8 and tuple(got.shape) == size
            assert torch.equal(got, want), f"{case} {kind} {ncls} classes {src.dtype}: {int((got != want).sum())} voxels differ"
            assert same_bits(got_max, want_max), f"{case} {kind} {ncls} classes {src.dtype}: out_max"
            assert torch.equal(M.resample_argmax(src, size=size, kind=kind, antialias=aa), got)
        if kind != "linear":
            continue
        # the u8 form against one-hot float planes; a label of 255 is present, a label >= ncls scores for nobody
        lab = dev(R.blob_labels(32, ncls, shape, special=(255, min(ncls, 255))))
        hot = (lab[None] == torch.arange(ncls, device=DEV).view(-1, 1, 1, 1)).float()
        want, _ = first_argmax(three_passes(hot, size, "linear", aa))
        got = M.resample_labels(lab, size=size, num_classes=ncls, kind="linear", antialias=aa)
        assert torch.equal(got, want), f"{case} labels {ncls} classes: {int((got != want).sum())} voxels differ"
        assert int(got.max()) < ncls


# ---------------------------------------------------------------------------------------------- 4. fused against fp64
@pytest.mark.parametrize("size", [(16, 24, 32), (4, 6, 8), (16, 6, 32)])
def test_fused_argmax_on_dyadic_cases_equals_fp64_everywhere(size):
    """One-hot labels and dyadic score planes under dyadic tables: exact scores, exact ties included -- the lowest class wins."""
    shape = (8, 12, 16)
    tabs = tables(shape, size, "linear", True)
    lab = R.blob_labels(41, 4, shape, special=(255, 4))
    s64 = R.resample64(R.one_hot(lab, 4, np.float64), tabs)
    if size == (16, 24, 32):
        top = np.sort(s64, axis=0)
        assert (top[-1] == top[-2]).any(), "the case holds no exact tie"
    got = M.resample_labels(dev(lab), size=size, num_classes=4)
    assert R.check_argmax(host(got), s64, 0.0, f"labels {shape} -> {size}") == 0.0
    planes = (np.random.default_rng(42).integers(0, 9, size=(5,) + shape) / 8.0).astype(np.float32)
    s64 = R.resample64(planes, tabs)
    got, best = M.resample_argmax(dev(planes), size=size, return_max=True)
    assert R.check_argmax(host(got), s64, 0.0, f"dyadic planes {shape} -> {size}") == 0.0
    R.check_exact(host(best), s64.max(0), "out_max")


@pytest.mark.parametrize("size", [(19, 23, 17), (7, 6, 9), (24, 20, 28)])
def test_fused_argmax_against_fp64_outside_the_margin(size):
    """Equality wherever the fp64 margin between the two best classes exceeds the derived bound; at most 5 % of the voxels may be
    left out, asserted before anything is compared."""
    shape = (12, 10, 14)
    tabs = tables(shape, size, "linear", True)
    lab = R.blob_labels(43, 4, shape)
    hot = R.one_hot(lab, 4)
    share = R.check_argmax(host(M.resample_labels(dev(lab), size=size, num_classes=4)), R.resample64(hot, tabs), R.error_bound(hot, tabs),
                           f"labels {shape} -> {size}")
    print(f"[resample] one-hot labels {shape} -> {size}: {share:.2%} of the voxels within the bound of a tie")
    planes = R.softmax_planes(44, 14, shape)
    share = R.check_argmax(host(M.resample_argmax(dev(planes), size=size)), R.resample64(planes, tabs), R.error_bound(planes, tabs),
                           f"softmax planes {shape} -> {size}")
    print(f"[resample] softmax planes {shape} -> {size}: {share:.2%} of the voxels within the bound of a tie")


# ---------------------------------------------------------------------------------------------- 5. safety
def hand_table(rows, taps):
    """rows: (start, count, weights of all `taps` slots) per output."""
    start = torch.tensor([r[0] for r in rows], dtype=torch.int32)
    count = torch.tensor([r[1] for r in rows], dtype=torch.int32)
    weight = torch.tensor([list(r[2]) for r in rows], dtype=torch.float32).reshape(len(rows), taps)
    return start, count, weight, taps


def on_device(table, put=lambda t: t.to(DEV)):
    return tuple(put(t) for t in table[:3]) + (table[3], False)


def argmax_call(src, ncls, size, tz, ty, tx, return_max=True):
    """mednet_resample_argmax with the caller's tables (the module's wrapper builds its own)."""
    d, h, w = src.shape[-3:]
    out = torch.empty(size, dtype=torch.uint8, device=src.device)
    best = torch.empty(size, dtype=torch.float32, device=src.device) if return_max else None
    args = [a for t in (tz, ty, tx) for a in (t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3])]
    M.L.check(M.L.lib().mednet_resample_argmax(src.data_ptr(), M._DTYPES[src.dtype], ncls, d, h, w, out.data_ptr(), M.L.ptr(best), *size,
                                               *args, M.L.stream()), "resample_argmax")
    return out, best


@pytest.mark.parametrize("taps", [2, 3])
def test_nan_next_to_the_support_does_not_leak(taps):
    """Rows of count = taps - 1 whose unused slot holds a WEIGHT, and a NaN in the voxel just behind every row's support: a kernel
    that read the slot would bring the NaN out.  taps = 2 takes the unrolled path of the fused kernel, 3 the tap loop."""
    cnt, n_out = taps - 1, 4
    n_in = n_out * taps
    rows = [(i * taps, cnt, [1.0 / cnt] * cnt + [0.5]) for i in range(n_out)]
    table = on_device(hand_table(rows, taps))
    vol = torch.rand((2, n_in, n_in, n_in), device=DEV)
    live = torch.zeros(n_in, dtype=torch.bool, device=DEV)
    for i in range(n_out):
        live[i * taps:i * taps + cnt] = True
    vol[:, ~live] = float("nan")
    vol[:, :, ~live] = float("nan")
    vol[:, :, :, ~live] = float("nan")
    out = vol
    for axis in (2, 1, 0):
        out = M.resample_axis(out, axis, table)
    assert tuple(out.shape) == (2, n_out, n_out, n_out) and bool(torch.isfinite(out).all())
    want = vol[:, live][:, :, live][:, :, :, live].reshape(2, n_out, cnt, n_out, cnt, n_out, cnt).double().mean((2, 4, 6))
    assert float((out.double() - want).abs().max()) <= 1e-6
    got, best = argmax_call(vol, 2, (n_out,) * 3, table, table, table)
    want_arg, want_best = first_argmax(out)
    assert bool(torch.isfinite(best).all()) and torch.equal(got, want_arg) and same_bits(best, want_best)


def test_hostile_tables_stay_inside_the_tensors():
    """count far above taps and start values far outside the extent, in guard bands: the kernels clamp both, no guard byte changes
    and the result is what the clamped table gives."""
    big = 2 ** 31 - 1
    rows = [(-5, 1000, [0.5, 0.25, 0.25]), (big, 3, [1.0, 0.0, 0.0]), (-big - 1, -7, [1.0, 9.0, 9.0]), (6, big, [0.25, 0.5, 0.25]),
            (2, 0, [2.0, 9.0, 9.0])]
    n = 8
    clamped = [(0, 3), (n - 1, 3), (0, 1), (6, 3), (2, 1)]
    with Fence() as fence:
        table = on_device(hand_table(rows, 3), fence.put)
        for dt in ("f32", "f16", "u8"):
            src = fence.put(dev(R.random_volume(51, (2, n, n, n), dt)))
            for axis in (0, 1, 2):
                out = M.resample_axis(src, axis, table, torch.float32)
                assert fence.owns(out)
                v = np.moveaxis(host(src).astype(np.float64), 1 + axis, -1)
                want = np.stack([sum(rows[i][2][k] * v[..., min(s + k, n - 1)] for k in range(c)) for i, (s, c) in enumerate(clamped)], -1)
                assert np.abs(np.moveaxis(host(out), 1 + axis, -1) - want).max() <= 1e-3 * max(1.0, np.abs(want).max())
            ncls = 2 if dt != "u8" else 256
            out, best = argmax_call(src if dt != "u8" else src[0], ncls, (5, 5, 5), table, table, table)
            assert fence.owns(out) and fence.owns(best) and bool(torch.isfinite(best).all())
        fence.check()


def test_normal_cases_in_guard_bands():
    """One ordinary call of each entry with the volume, the tables and the outputs fenced: the vector loads of the axis pass
    (w % 4 == 0), the 32-bit store of the fused kernel and both scalar tails."""
    for shape, size in (((8, 12, 16), (16, 24, 32)), ((9, 7, 13), (5, 11, 6)), ((33, 35, 130), (16, 18, 65))):
        vol = R.random_volume(52, (2,) + shape)
        with Fence() as fence:
            tabs = [on_device(tuple(torch.from_numpy(a) for a in t[:3]) + (t[3],), fence.put) for t in tables(shape, size, "linear", True)]
            src = fence.put(dev(vol))
            out = src
            for axis in (2, 1, 0):
                out = M.resample_axis(out, axis, tabs[axis], torch.float32)
                assert fence.owns(out)
            got, best = argmax_call(src, 2, size, *tabs)
            lab, _ = argmax_call(fence.put(dev(R.blob_labels(53, 3, shape))), 3, size, *tabs, return_max=False)
            assert fence.owns(got) and fence.owns(best) and fence.owns(lab)
            fence.check()
        assert same_bits(out, M.resample(dev(vol), size=size))
        want, want_best = first_argmax(out)
        assert torch.equal(got, want) and same_bits(best, want_best)


def test_results_are_bit_identical_across_runs():
    shape, size = (33, 35, 130), (40, 18, 65)
    vol = dev(R.random_volume(54, (4,) + shape))
    lab = dev(R.blob_labels(55, 4, shape))
    first = (M.resample(vol, size=size, kind="cubic"), *M.resample_argmax(vol, size=size, return_max=True), M.resample_labels(lab, size=size, num_classes=4))
    again = (M.resample(vol, size=size, kind="cubic"), *M.resample_argmax(vol, size=size, return_max=True), M.resample_labels(lab, size=size, num_classes=4))
    for a, b in zip(first, again):
        assert same_bits(a, b)


def test_tables_are_cached_per_device():
    M.resample(torch.zeros((1, 4, 4, 4), device=DEV), size=(8, 4, 2))
    t = M.device_table(4, 8, "linear", True, torch.device(DEV))
    assert M.device_table(4, 8, "linear", True, torch.device(DEV)) is t and t[0].device == torch.device(DEV)


# ---------------------------------------------------------------------------------------------- 6. the predictor
def test_predictor_resamples_to_the_networks_grid_and_back():
    """spacing (2, 1, 1) at target spacing (1, 1, 1): the network runs on 80 x 36 x 44, result() has the native shape and equals the
    composition of the public pieces bit for bit; peaks map by the stated formula; evaluate runs on the native grid; without
    spacings the result is today's predict."""
    shape, patch, ov, nh, ncls = (40, 36, 44), (32, 32, 32), (4, 4, 4), 2, 3
    img = (O._rng("resample:predictor").standard_normal((1,) + shape) * 2).astype(np.float32)
    with mednet_hip.precision("fp32"):
        net = O.keyed_init_(HM.ResidualUNet3D(in_channels=1, out_channels=nh + ncls, final_sigmoid=False, f_maps=[8])).to(DEV).eval()
        kw = dict(num_heatmaps=nh, pad_mode="symmetric", batch_size=3, blend="gaussian")
        plain = HP.GridPredictor(net, patch, ov, **kw)
        pr = HP.GridPredictor(net, patch, ov, target_spacing=(1, 1, 1), **kw)
        pred = pr.predict(img, spacing=(2, 1, 1))
        assert isinstance(pred, HP.ResampledPrediction) and pred.native_shape == shape and tuple(pred.acc.shape) == (nh + ncls, 80, 36, 44)
        # the composition of the public pieces
        net_vol = M.resample(dev(img), spacing=(2, 1, 1), target_spacing=(1, 1, 1))
        assert tuple(net_vol.shape) == (1, 80, 36, 44)
        base = plain.predict(net_vol)
        assert type(base) is HP.BlendedPrediction and same_bits(base.acc, pred.acc) and same_bits(base.wsum, pred.wsum)
        res = pred.result()
        assert res.dtype == torch.uint8 and tuple(res.shape) == (nh + 1,) + shape
        assert torch.equal(res[-1], M.resample_argmax(base.probabilities(), size=shape))
        heat = M.resample(base.heatmaps(), size=shape)
        assert torch.equal(res[:-1], heat.clamp(0, 255).to(torch.uint8))
        assert same_bits(pred.heatmaps(), heat) and same_bits(pred.probabilities(), M.resample(base.probabilities(), size=shape))
        assert same_bits(pred.probabilities(torch.float16), M.resample(base.probabilities(), size=shape, dtype=torch.float16))
        flipped = pred.result(postprocess=lambda v: 2 - v)
        assert torch.equal(flipped[-1], 2 - res[-1]) and torch.equal(flipped[:-1], res[:-1])
        # peaks: p = (q + 0.5) * n_native / n_net - 0.5
        q, qv = base.peaks()
        p, pv = pred.peaks()
        assert p.dtype == torch.float64 and torch.equal(pv, qv)
        assert torch.equal(p, (q.double() + 0.5) * torch.tensor([0.5, 1.0, 1.0], dtype=torch.float64, device=DEV) - 0.5)
        # evaluate on the native grid
        label = dev(R.blob_labels(61, ncls, shape))
        from mednet_hip.metrics import evaluate_case
        got, want = pred.evaluate(label, spacing=(2, 1, 1)).to_host(), evaluate_case(res[-1], label, ncls, spacing=(2, 1, 1)).to_host()
        assert str(got) == str(want)
        # without spacings: today's predict, bit for bit
        for other in (pr.predict(img), plain.predict(img, spacing=(2, 1, 1))):
            ref = plain.predict(img)
            assert type(other) is HP.BlendedPrediction and same_bits(other.acc, ref.acc) and torch.equal(other.result(), ref.result())
