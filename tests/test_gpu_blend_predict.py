"""Blended sliding-window inference on the GPU (csrc/blend.hip, mednet_hip.predict): Gaussian windows, test-time mirroring, soft
outputs and heat-map peaks against the numpy fp64 restatement of tests/blend_util.py -- exact where the arithmetic is exact, bit-equal
across batch sizes, and within bounds taken from the number formats and ATen's own fp32 error (profiles/blend_bounds.md) elsewhere."""
import functools

import numpy as np
import pytest
import torch

import blend_util as B
import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import predict as HP
from mednet_hip.unet import model as HM
from oracle import ref_cpu as O

from fence import Fence
from gpu_util import DEV

pytestmark = pytest.mark.gpu

PATCH, OV, VOL = B.PATCH, B.OVERLAP, B.VOLUME
POS = B.grid_positions(VOL, PATCH, OV)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def run_accumulate(logits, windows, nh, of="probabilities", mirror=0, batch=80, pos=POS, vol=VOL, ov=OV):
    """Upload once, accumulate in launches of `batch` rows -> (acc, wsum) on the device."""
    lg = logits if torch.is_tensor(logits) else dev(logits)
    win = tuple(dev(w) for w in windows)
    p = dev(pos)
    acc = torch.zeros((lg.shape[1],) + tuple(vol), dtype=torch.float32, device=DEV)
    wsum = torch.zeros(tuple(vol), dtype=torch.float32, device=DEV)
    for b0 in range(0, len(pos), batch):
        HP.accumulate(lg[b0:b0 + batch], p[b0:b0 + batch].contiguous(), acc, wsum, win, nh, ov, mirror, of)
    return acc, wsum


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------- 1. exact geometry
EXACT = [("h0c1", 0, 1, "probabilities", 1.0), ("h2c2", 2, 2, "probabilities", 0.5), ("h0c4", 0, 4, "probabilities", 0.25),
         ("h2c4", 2, 4, "probabilities", 0.25), ("h2c5-logits", 2, 5, "logits", 1.0)]


@pytest.mark.parametrize("case", EXACT, ids=[c[0] for c in EXACT])
def test_exact_geometry_every_batch_size_and_mirror(case):
    """Power-of-two windows, integer heat maps encoding (row, z, y, x), a softmax of exactly 1 / ncls (or integer logits): every
    product and partial sum is an fp32 number in any order, so acc and wsum equal the fp64 restatement bit for bit -- for launches of
    1, 3, 5 and 80 rows and every mirror mask, the mirrored input built with numpy flips."""
    _, nh, ncls, of, unit = case
    lg = B.exact_logits(80, nh, ncls, PATCH, of)
    win = B.pow2_windows(PATCH)
    ref = B.Blend64(nh + ncls, nh, VOL, PATCH, OV, win, of).add(lg, POS)
    B.assert_exact_premise(ref.norm, unit, "acc")
    B.assert_exact_premise(ref.wsum, 1.0, "wsum")
    for mirror in range(8):
        on_dev = dev(B.flip(lg, mirror, 2))
        for batch in (1, 3, 5, 80):
            acc, wsum = run_accumulate(on_dev, win, nh, of, mirror, batch)
            B.check_exact(acc.cpu().numpy(), ref.acc, f"acc (mirror {mirror}, batch {batch})")
            B.check_exact(wsum.cpu().numpy(), ref.wsum, f"wsum (mirror {mirror}, batch {batch})")


# ---------------------------------------------------------------------------------------------- 2. batch size, determinism
@pytest.mark.parametrize("of", ["probabilities", "logits"])
def test_bits_do_not_depend_on_batch_size_or_run(of):
    lg = dev(B.random_logits(80, 6, PATCH, seed=21))
    win = B.gaussian_windows(PATCH)
    for mirror in (0, 5):
        first = run_accumulate(lg, win, 2, of, mirror, 1)
        for batch in (1, 4, 80, 80):
            acc, wsum = run_accumulate(lg, win, 2, of, mirror, batch)
            assert same_bits(acc, first[0]) and same_bits(wsum, first[1]), (of, mirror, batch)


# ---------------------------------------------------------------------------------------------- 3. values
@functools.lru_cache(maxsize=None)
def value_case(of):
    """Gaussian windows, random logits (scale 3): the fp64 restatement, ATen's fp32 composition and the bounds, computed once."""
    lg = B.random_logits(80, 7, PATCH, seed=11)
    win = B.gaussian_windows(PATCH)
    ref = B.Blend64(7, 2, VOL, PATCH, OV, win, of).add(lg, POS)
    a32 = B.Blend32(7, 2, VOL, PATCH, OV, win, of).add(lg, POS)
    r_a, r_w = B.r32_of(a32.acc.numpy(), ref.acc, ref.norm), B.r32_of(a32.wsum.numpy(), ref.wsum, ref.wsum)
    eps_a, eps_w = B.eps_of(r_a, ref.cnt), B.eps_of(r_w, ref.cnt)
    heat, prob, result = B.finalize64(ref.acc, ref.wsum, 2, of)
    r_sm = 0.0
    if of == "logits":
        mean = (ref.acc[2:] / ref.wsum).astype(np.float32)
        r_sm = B.r32_of(torch.softmax(torch.from_numpy(mean), 0).numpy(), B.softmax64(mean.astype(np.float64)), prob)
    return dict(lg=lg, win=win, ref=ref, r_a=r_a, r_w=r_w, eps_a=eps_a, eps_w=eps_w, heat=heat, prob=prob, result=result, r_sm=r_sm)


def prob_bound(c, half):
    ref = c["ref"]
    if ref.blend_of == "probabilities":
        return B.quotient_bound(c["prob"], ref.norm[2:], ref.wsum, c["eps_a"], c["eps_w"], half)
    delta = B.quotient_bound(ref.acc[2:] / ref.wsum, ref.norm[2:], ref.wsum, c["eps_a"], c["eps_w"])
    return B.softmax_bound(c["prob"], delta, c["r_sm"], half)


@pytest.mark.parametrize("of", ["probabilities", "logits"])
def test_values_against_fp64_within_format_and_aten_bounds(of):
    """acc, wsum, probabilities() and heatmaps() per element: |got - ref64| <= (4 r32 + cnt 2^-24) * sum |terms| and what follows from
    it for the quotient; r32 is the error of the same composition in fp32 ATen ops on the CPU, cnt the number of terms of the voxel."""
    c = value_case(of)
    ref = c["ref"]
    acc, wsum = run_accumulate(c["lg"], c["win"], 2, of, 0, 7)
    worst = dict(r32_acc=c["r_a"], r32_wsum=c["r_w"], r32_softmax=c["r_sm"])
    worst["acc"] = B.check_values(acc.cpu().numpy(), ref.acc, c["eps_a"] * ref.norm, "acc")
    worst["wsum"] = B.check_values(wsum.cpu().numpy(), ref.wsum, c["eps_w"] * ref.wsum, "wsum")
    pred = HP.BlendedPrediction(acc, wsum, 2, of)
    p32, p16, heat = pred.probabilities(), pred.probabilities(torch.float16), pred.heatmaps()
    assert p32.dtype == torch.float32 and p16.dtype == torch.float16 and heat.dtype == torch.float32
    worst["heat"] = B.check_values(heat.cpu().numpy(), c["heat"], B.quotient_bound(c["heat"], ref.norm[:2], ref.wsum, c["eps_a"], c["eps_w"]),
                                   "heatmaps()")
    worst["prob"] = B.check_values(p32.cpu().numpy(), c["prob"], prob_bound(c, False), "probabilities()")
    worst["prob16"] = B.check_values(p16.cpu().numpy(), c["prob"], prob_bound(c, True), "probabilities(float16)")
    print(f"[blend] {of}: " + " ".join(f"{k}={v:.3e}" for k, v in worst.items()))
    # the division itself: within one fp32 ulp of the fp64 quotient of the DEVICE's accumulators; fp16 is that value rounded once
    a64, w64 = acc.cpu().numpy().astype(np.float64), wsum.cpu().numpy().astype(np.float64)
    B.check_one_ulp(heat.cpu().numpy(), a64[:2] / w64, "heat = acc / wsum")
    if of == "probabilities":
        B.check_one_ulp(p32.cpu().numpy(), a64[2:] / w64, "prob = acc / wsum")
    assert np.array_equal(p16.cpu().numpy(), p32.cpu().numpy().astype(np.float16))
    # result(): the reference's layout from the device's own numbers
    res = pred.result().cpu().numpy()
    assert res.dtype == np.uint8 and res.shape == (3,) + VOL
    assert np.array_equal(res[:2], np.clip(heat.cpu().numpy(), 0, 255).astype(np.uint8))
    assert np.array_equal(res[2], acc.cpu().numpy()[2:].argmax(0))


def test_finalize_ties_clip_edges_and_an_uncovered_voxel():
    """First maximum on ties, truncation after the clip to 0..255, and wsum == 0 reads 0 everywhere instead of NaN."""
    acc = torch.zeros((3, 1, 2, 4), dtype=torch.float32)
    wsum = torch.full((1, 2, 4), 0.5)
    acc[0, 0, 0] = torch.tensor([-3.0, 0.4, 127.9, 200.0]) * 0.5
    acc[0, 0, 1] = torch.tensor([255.9, 1.0, 1.999, 64.5]) * 0.5
    acc[1] = 0.25
    acc[2] = 0.25
    acc[2, 0, 1, 2:] = 0.2500001
    wsum[0, 1, 3] = 0.0
    for of in ("probabilities", "logits"):
        res, prob, heat = HP.finalize(acc.to(DEV), wsum.to(DEV), 1, of, result=True, probabilities=torch.float32, heatmaps=True)
        assert res[0].cpu().flatten().tolist() == [0, 0, 127, 200, 255, 1, 1, 0]
        assert res[1].cpu().flatten().tolist() == [0, 0, 0, 0, 0, 0, 1, 0]
        assert float(heat[0, 0, 1, 3]) == 0.0 and prob[:, 0, 1, 3].cpu().tolist() == [0.0, 0.0]
        assert not bool(torch.isnan(prob).any()) and not bool(torch.isnan(heat).any())
        assert prob[:, 0, 0, 0].cpu().tolist() == [0.5, 0.5]


# ---------------------------------------------------------------------------------------------- 4. grid_gather_mirror
@pytest.mark.parametrize("pad_mode", ["constant", "symmetric"])
def test_gather_mirror_mask_zero_is_the_old_gather_and_the_others_are_flips(pad_mode):
    g = np.random.Generator(np.random.PCG64(2))
    vol = dev(g.standard_normal((2,) + VOL).astype(np.float32))
    pos = dev(POS)
    old = HP.gather_patches(vol, pos, PATCH, OV, pad_mode)
    out = torch.full_like(old, float("nan"))
    L.check(L.lib().mednet_grid_gather_mirror(vol.data_ptr(), pos.data_ptr(), out.data_ptr(), 80, 2, *VOL, *PATCH, *OV, HP._PAD[pad_mode], 0,
                                              L.stream()), "grid_gather_mirror")
    assert same_bits(out, old)
    base = old.cpu().numpy()
    for mirror in range(1, 8):
        got = HP.gather_patches(vol, pos, PATCH, OV, pad_mode, mirror=mirror).cpu().numpy()
        assert np.array_equal(got, B.flip(base, mirror, 2)), mirror


# ---------------------------------------------------------------------------------------------- 5. pointwise model end to end
class Stub(torch.nn.Module):
    """logits_c = a_c x + b_c per voxel behind num_heatmaps heat maps (k + 1) x: exact in fp32 on the lattice volume."""

    def __init__(self, num_heatmaps=2):
        super().__init__()
        self.nh = num_heatmaps
        self.a = torch.nn.Parameter(torch.tensor(B.STUB_A).reshape(1, 5, 1, 1, 1))
        self.b = torch.nn.Parameter(torch.tensor(B.STUB_B).reshape(1, 5, 1, 1, 1))

    def forward(self, x):
        heat = [(k + 1) * x for k in range(self.nh)]
        return torch.cat(heat + [self.a * x + self.b], dim=1)


@functools.lru_cache(maxsize=None)
def stub_case():
    vol = B.lattice_volume(VOL, 5)
    want = B.stub_logits64(vol[0], 2)
    return vol, want, B.softmax64(want[2:])


@pytest.mark.parametrize("blend,axes", [("gaussian", ()), ("constant", ()), ("gaussian", (0, 1, 2)), ("constant", (1,)), ("gaussian", (2, 0))])
def test_pointwise_model_end_to_end(blend, axes):
    """Every patch gives a voxel the same logits, so probabilities() is the softmax of the pointwise logits and heatmaps() the
    pointwise values, whatever the window and the mirror axes; the top-2 probability gap over the lattice is 6.5e-3
    (tests/test_blend_util.py), so the class plane of result() equals the fp64 arg-max in EVERY voxel."""
    vol, want, prob = stub_case()
    stub = Stub().to(DEV)
    pr = HP.GridPredictor(stub, PATCH, OV, num_heatmaps=2, pad_mode="constant", batch_size=7, blend=blend, mirror_axes=axes)
    pred = pr.predict(vol)
    win = B.gaussian_windows(PATCH) if blend == "gaussian" else tuple(np.ones(p, dtype=np.float32) for p in PATCH)
    # the restatement on the stub's own (exact) logits: the patches of every mirror pass in the predictor's order
    padded = np.pad(vol[0].astype(np.float64), [(o, p) for o, p in zip(OV, PATCH)])
    rows = np.stack([padded[z:z + PATCH[0], y:y + PATCH[1], x:x + PATCH[2]] for z, y, x in POS])
    ref = B.Blend64(7, 2, VOL, PATCH, OV, win)
    a32 = B.Blend32(7, 2, VOL, PATCH, OV, win)
    passes = [m for m in range(8) if m & ~HP.mirror_mask(axes) == 0]
    assert pr.mirror_passes == passes and len(passes) == 2 ** len(axes)
    for m in passes:
        lg = np.stack([B.stub_logits64(B.flip(r, m, 0), 2) for r in rows])
        ref.add(lg, POS, mirror=m)
        a32.add(lg.astype(np.float32), POS, mirror=m)
    eps_a = B.eps_of(B.r32_of(a32.acc.numpy(), ref.acc, ref.norm), ref.cnt)
    eps_w = B.eps_of(B.r32_of(a32.wsum.numpy(), ref.wsum, ref.wsum), ref.cnt)
    B.check_values(pred.acc.cpu().numpy(), ref.acc, eps_a * ref.norm, "acc")
    B.check_values(pred.wsum.cpu().numpy(), ref.wsum, eps_w * ref.wsum, "wsum")
    h64, p64, r64 = B.finalize64(ref.acc, ref.wsum, 2)
    assert np.abs(p64 - prob).max() < 1e-13 and np.abs(h64 - want[:2]).max() < 1e-13     # (the restatement gives the pointwise values)
    B.check_values(pred.probabilities().cpu().numpy(), prob, B.quotient_bound(prob, ref.norm[2:], ref.wsum, eps_a, eps_w), "probabilities()")
    B.check_values(pred.heatmaps().cpu().numpy(), want[:2], B.quotient_bound(want[:2], ref.norm[:2], ref.wsum, eps_a, eps_w), "heatmaps()")
    res = pred.result()
    assert res.dtype == torch.uint8 and tuple(res.shape) == (3,) + VOL and res.device.type == "cuda"
    assert np.array_equal(res[2].cpu().numpy(), want[2:].argmax(0))
    assert np.array_equal(res.cpu().numpy(), pr(vol).cpu().numpy())                     # __call__ with blend set returns result()
    zyx, val = pred.peaks()
    assert tuple(zyx.shape) == (2, 3) and zyx.dtype == torch.int64
    heat = pred.heatmaps().cpu().numpy()
    for k in range(2):
        assert tuple(zyx[k].tolist()) == np.unravel_index(heat[k].argmax(), VOL) and float(val[k]) == heat[k].max()


def test_without_blend_the_predictor_is_the_parents():
    """blend=None runs the crop-stitch lines: the result equals stitching the same logits with `assemble` by hand, and the new keyword
    arguments are refused where they make no sense."""
    vol, _, _ = stub_case()
    stub = Stub().to(DEV)
    got = HP.GridPredictor(stub, PATCH, OV, num_heatmaps=2, pad_mode="constant", batch_size=7)(vol)
    v = dev(vol, torch.float32)
    pos = dev(POS)
    want = torch.zeros((3,) + VOL, dtype=torch.uint8, device=DEV)
    with torch.no_grad():
        for b0 in range(0, 80, 7):
            p = pos[b0:b0 + 7].contiguous()
            HP.assemble(stub(HP.gather_patches(v, p, PATCH, OV, "constant")), p, want, 2, OV)
    assert torch.equal(got, want) and got.dtype == torch.uint8
    with pytest.raises(ValueError):
        HP.GridPredictor(stub, PATCH, OV, mirror_axes=(0,))
    with pytest.raises(ValueError):
        HP.GridPredictor(stub, PATCH, OV).predict(vol)
    with pytest.raises(ValueError):
        HP.GridPredictor(stub, PATCH, OV, blend="gaussian", blend_of="votes")


# ---------------------------------------------------------------------------------------------- 6. real network
def test_real_network_with_mirroring_follows_the_restated_loop():
    """ResidualUNet3D(1, 5, f_maps=[8, 16]) in fp32 mode, the existing end-to-end test's shapes, mirror_axes=(2,): the predictor against
    the same device model called on the same batches with an explicit torch.flip, blended by the fp64 restatement.  This pins the loop,
    not the network: the model's own run-to-run difference is measured and must be zero."""
    ctor = dict(in_channels=1, out_channels=5, final_sigmoid=False, f_maps=[8, 16])
    nh, patch, ov, shape = 2, (16, 16, 16), (2, 3, 4), (21, 30, 19)
    img = (O._rng("predict:e2e").standard_normal((1,) + shape) * 2).astype(np.float16)
    pos_np = B.grid_positions(shape, patch, ov)
    win = B.gaussian_windows(patch)
    with mednet_hip.precision("fp32"):
        net = O.keyed_init_(HM.ResidualUNet3D(**ctor)).to(DEV).eval()
        pred = HP.GridPredictor(net, patch, ov, num_heatmaps=nh, pad_mode="symmetric", batch_size=3, blend="gaussian",
                                mirror_axes=(2,)).predict(img)
        v, pos = dev(img, torch.float32), dev(pos_np)
        ref = B.Blend64(5, nh, shape, patch, ov, win)
        a32 = B.Blend32(5, nh, shape, patch, ov, win)
        with torch.no_grad():
            for m, dims in ((0, ()), (4, (4,))):
                for b0 in range(0, len(pos_np), 3):
                    x = HP.gather_patches(v, pos[b0:b0 + 3].contiguous(), patch, ov, "symmetric")
                    x = torch.flip(x, dims).contiguous() if dims else x
                    lg, again = net(x), net(x)
                    assert torch.equal(lg, again), "the model differs between two runs on the same input"
                    lg = lg.float().cpu().numpy()
                    ref.add(lg, pos_np[b0:b0 + 3], mirror=m)
                    a32.add(lg, pos_np[b0:b0 + 3], mirror=m)
    assert ref.cnt.max() == 16 and ref.cnt.min() >= 2
    eps_a = B.eps_of(B.r32_of(a32.acc.numpy(), ref.acc, ref.norm), ref.cnt)
    eps_w = B.eps_of(B.r32_of(a32.wsum.numpy(), ref.wsum, ref.wsum), ref.cnt)
    B.check_values(pred.acc.cpu().numpy(), ref.acc, eps_a * ref.norm, "acc")
    B.check_values(pred.wsum.cpu().numpy(), ref.wsum, eps_w * ref.wsum, "wsum")
    h64, p64, _ = B.finalize64(ref.acc, ref.wsum, nh)
    B.check_values(pred.probabilities().cpu().numpy(), p64, B.quotient_bound(p64, ref.norm[nh:], ref.wsum, eps_a, eps_w), "probabilities()")
    B.check_values(pred.heatmaps().cpu().numpy(), h64, B.quotient_bound(h64, ref.norm[:nh], ref.wsum, eps_a, eps_w), "heatmaps()")


# ---------------------------------------------------------------------------------------------- 7. overlap 0
def test_overlap_zero_gives_the_single_covering_patch():
    """Patch 8^3 on (13, 19, 9) without overlap: every voxel lies in exactly one patch, and the blended result is that patch's arg-max
    (and its heat maps).  The crop-stitch path's empty result is not changed."""
    patch, ov, shape = (8, 8, 8), (0, 0, 0), (13, 19, 9)
    pos = B.grid_positions(shape, patch, ov)
    assert len(pos) == 2 * 3 * 2
    lg = B.random_logits(len(pos), 6, patch, seed=4, scale=40.0)
    want = np.zeros((6,) + shape)
    for b, (z, y, x) in enumerate(pos):
        ps, vs = B._window((z, y, x), patch, shape)
        want[(slice(None),) + vs] = lg[b][(slice(None),) + ps]
    ones = tuple(np.ones(8, dtype=np.float32) for _ in range(3))
    acc, wsum = run_accumulate(lg, ones, 2, "logits", 0, 5, pos=pos, vol=shape, ov=ov)
    assert bool((wsum == 1).all())
    res = HP.finalize(acc, wsum, 2, "logits", result=True)[0].cpu().numpy()
    assert np.array_equal(res[2], want[2:].argmax(0)) and np.array_equal(res[:2], np.clip(want[:2], 0, 255).astype(np.uint8))
    vol = B.lattice_volume(shape, 9)
    stub = Stub().to(DEV)
    got = HP.GridPredictor(stub, patch, ov, num_heatmaps=2, batch_size=5, blend="constant")(vol).cpu().numpy()
    assert np.array_equal(got[2], B.stub_logits64(vol[0], 2)[2:].argmax(0))
    empty = HP.GridPredictor(stub, patch, ov, num_heatmaps=2, batch_size=5)(vol)
    assert tuple(empty.shape) == (3,) + shape and not bool(empty.any())


# ---------------------------------------------------------------------------------------------- 8. footprint
def test_footprint_inside_guard_bands():
    """Logits, positions, windows, accumulators, every finalize output and the peaks workspace (exactly _ws_bytes) in guard bands, for
    the shape whose patches hang over the volume: bit-equal to the unfenced run, every guard byte intact."""
    lg = B.random_logits(80, 6, PATCH, seed=8)
    win = B.gaussian_windows(PATCH)

    def run(put, ws_check=None):
        logits, pos = put(dev(lg)), put(dev(POS))
        w = tuple(put(dev(v)) for v in win)
        acc = put(torch.zeros((6,) + VOL, dtype=torch.float32, device=DEV))
        wsum = put(torch.zeros(VOL, dtype=torch.float32, device=DEV))
        for mirror in (0, 3):
            for b0 in range(0, 80, 32):
                HP.accumulate(logits[b0:b0 + 32], pos[b0:b0 + 32], acc, wsum, w, 2, OV, mirror)
        res, prob, heat = HP.finalize(acc, wsum, 2, result=True, probabilities=torch.float16, heatmaps=True)
        zyx, val = HP.heatmap_peaks(heat)
        return dict(acc=acc, wsum=wsum, res=res, prob=prob, heat=heat, zyx=zyx, val=val)

    plain = run(lambda t: t)
    with Fence() as fence:
        fenced = run(fence.put)
        fence.check()
        for k in ("acc", "wsum", "res", "prob", "heat", "val"):
            assert fence.owns(fenced[k]), k
        need = L.lib().mednet_heatmap_peaks_ws_bytes(2, int(np.prod(VOL)))
        assert [r[:2] for r in fence.ws_requests] == [(need, need)]
    for k, t in plain.items():
        assert t.cpu().numpy().tobytes() == fenced[k].cpu().numpy().tobytes(), k
    assert not bool(torch.isnan(fenced["heat"]).any()) and not bool(torch.isnan(fenced["prob"]).any())


# ---------------------------------------------------------------------------------------------- 9. peaks
def test_heatmap_peaks_planted_maximum_tie_nan_and_negative_channel():
    """Two channels of 70 001 voxels (18 workgroups, a ragged tail): a planted maximum twice (the lowest index wins) next to NaNs, and
    an all-negative channel whose maximum is the very last voxel; index and value exact."""
    n = 70001
    g = np.random.Generator(np.random.PCG64(6))
    h = np.empty((2, n), dtype=np.float32)
    h[0] = g.random(n)
    h[0, [69999, 4100, 30000]] = 5.0
    h[0, [10, 4099, n - 1]] = np.nan
    h[1] = -0.1 - g.random(n)
    h[1, n - 1] = -0.05
    h[1, 123] = np.nan
    idx, val = B.peaks64(h)
    assert idx.tolist() == [4100, n - 1]
    zyx, got = HP.heatmap_peaks(dev(h).reshape(2, 1, 1, n))
    assert zyx.cpu().tolist() == [[0, 0, 4100], [0, 0, n - 1]] and got.cpu().tolist() == [5.0, float(np.float32(-0.05))]
    # positions as (z, y, x), several maxima per line, a channel of NaNs only
    small = g.integers(0, 4, size=(3, 5, 7, 11)).astype(np.float32)
    small[2] = np.nan
    zyx, got = HP.heatmap_peaks(dev(small))
    idx, val = B.peaks64(small)
    for k in range(2):
        assert tuple(zyx[k].tolist()) == np.unravel_index(idx[k], (5, 7, 11)) and float(got[k]) == val[k]
    assert float(got[2]) == -np.inf and bool((zyx[2] < 0).any())
