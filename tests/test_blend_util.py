"""The numpy restatement of blended inference (tests/blend_util.py) on the CPU: its own invariants hold, ATen's fp32 composition
passes the bounds the GPU tests use, and the checkers reject every injected fault."""
import numpy as np
import pytest

import blend_util as B
from mednet_hip import predict as HP

PATCH, OV, VOL = B.PATCH, B.OVERLAP, B.VOLUME
POS = B.grid_positions(VOL, PATCH, OV)


def test_windows_follow_the_formula_and_are_symmetric():
    for patch in (PATCH, (128, 128, 128), (16, 16, 16)):
        win = HP.blend_window(patch)
        for v, r, p in zip(win, B.gaussian_windows(patch), patch):
            assert v.dtype == np.float32 and v.shape == (p,) and np.array_equal(v, r)
            assert np.array_equal(v, v[::-1]) and v.max() <= 1.0 and v.argmax() in ((p - 1) // 2, p // 2)
            i = np.arange(p)
            assert np.array_equal(v, np.exp(-0.5 * ((i - (p - 1) / 2) / (0.125 * p)) ** 2).astype(np.float32))
        for v, p in zip(HP.blend_window(patch, "constant"), patch):
            assert v.dtype == np.float32 and np.array_equal(v, np.ones(p, dtype=np.float32))
    w = B.weight32(HP.blend_window((128, 128, 128)))
    assert 5e-11 < float(w.min()) < 6e-11          # far inside fp32's normal range: no clamp
    assert len({len(np.unique(v)) for v in B.pow2_windows(PATCH)}) >= 1 and all((v >= 1).all() for v in B.pow2_windows(PATCH))
    with pytest.raises(ValueError):
        HP.blend_window(PATCH, "cosine")


def test_grid_and_coverage_of_the_test_shape():
    assert np.array_equal(POS, HP.grid_positions(VOL, PATCH, OV)) and len(POS) == 80
    blend = B.Blend64(1, 0, VOL, PATCH, OV, B.gaussian_windows(PATCH)).add(np.zeros((80, 1) + PATCH), POS)
    assert blend.cnt.min() == 1 and blend.cnt.max() == 8
    assert 0.0175 <= blend.wsum.min() and blend.wsum.max() < 0.815      # (0.017507 .. 0.81290)
    step = np.asarray(PATCH) - 2 * np.asarray(OV)
    far = POS - np.asarray(OV) + np.asarray(PATCH)
    assert [len(np.unique(POS[(far > np.asarray(VOL))[:, k], k])) for k in range(3)] == [2, 2, 1]   # grid rows hanging over the far end
    assert (POS % step == 0).all()


def test_constant_logits_give_softmax_back_and_heat_maps_their_value():
    g = np.random.Generator(np.random.PCG64(3))
    one = (g.standard_normal(7) * 3).astype(np.float32)
    lg = np.broadcast_to(one[None, :, None, None, None], (80, 7) + PATCH)
    for of in ("probabilities", "logits"):
        blend = B.Blend64(7, 2, VOL, PATCH, OV, B.gaussian_windows(PATCH), of).add(lg, POS)
        heat, prob, result = B.finalize64(blend.acc, blend.wsum, 2, of)
        assert np.abs(prob - B.softmax64(one[2:].astype(np.float64))[:, None, None, None]).max() < 1e-14
        assert np.abs(heat - one[:2].astype(np.float64)[:, None, None, None]).max() < 1e-13
        assert (result[2] == one[2:].argmax()).all() and result.dtype == np.uint8 and result.shape == (3,) + VOL


def _stub_rows(volume, mask, nh=2):
    """The pointwise stub on the (mirrored) constant-padded patches of `volume`."""
    padded = np.pad(volume[0].astype(np.float64), [(o, p) for o, p in zip(OV, PATCH)])
    rows = []
    for z, y, x in POS:
        patch = padded[z:z + PATCH[0], y:y + PATCH[1], x:x + PATCH[2]]
        rows.append(B.stub_logits64(B.flip(patch, mask, 0), nh))
    return np.stack(rows)


def test_mirroring_leaves_a_pointwise_model_unchanged():
    vol = B.lattice_volume(VOL, 5)
    win = B.gaussian_windows(PATCH)
    base = B.Blend64(7, 2, VOL, PATCH, OV, win).add(_stub_rows(vol, 0), POS)
    want = B.stub_logits64(vol[0], 2)
    for mask in (1, 2, 4, 7):
        m = B.Blend64(7, 2, VOL, PATCH, OV, win).add(_stub_rows(vol, mask), POS, mirror=mask)
        assert np.abs(m.acc - base.acc).max() < 1e-13 and np.array_equal(m.wsum, base.wsum)
    heat, prob, result = B.finalize64(base.acc, base.wsum, 2)
    assert np.abs(prob - B.softmax64(want[2:])).max() < 1e-13 and np.abs(heat - want[:2]).max() < 1e-13
    assert np.array_equal(result[2], want[2:].argmax(0))


def test_the_stub_models_top_two_gap_over_the_lattice():
    """The class plane of .result() is compared in EVERY voxel: the two largest probabilities are never closer than 6.5e-3."""
    x = np.arange(-16, 17) / 8.0
    p = np.sort(B.softmax64(B.stub_logits64(x, 0)), axis=0)
    gap = float((p[-1] - p[-2]).min())
    assert 6.5e-3 <= gap < 7e-3, gap


def test_peaks_restated():
    h = np.array([[1.0, np.nan, 5.0, 5.0, -1.0], [-3.0, -2.0, -2.0, np.nan, -7.0], [np.nan] * 5])
    idx, val = B.peaks64(h)
    assert idx.tolist() == [2, 1, -1] and val.tolist() == [5.0, -2.0, -np.inf]


# ---------------------------------------------------------------------------------------------- the checkers
def _exact_pair(fault, mirror=5, batch=3, of="probabilities", ncls=4):
    lg = B.exact_logits(80, 2, ncls, PATCH, of)
    win = B.pow2_windows(PATCH)
    ref = B.Blend64(2 + ncls, 2, VOL, PATCH, OV, win, of).add(lg, POS)
    got = B.Blend64(2 + ncls, 2, VOL, PATCH, OV, win, of, fault=fault).add(B.flip(lg, mirror, 2), POS, mirror=mirror, batch=batch)
    return ref, got


def test_exact_inputs_meet_their_premise_and_mirrored_input_gives_the_same_sums():
    for of, ncls, unit in (("probabilities", 1, 1.0), ("probabilities", 2, 0.5), ("probabilities", 4, 0.25), ("logits", 5, 1.0)):
        ref, got = _exact_pair(None, of=of, ncls=ncls)
        B.assert_exact_premise(ref.norm, unit, f"{of} {ncls}")
        B.assert_exact_premise(ref.wsum, 1.0, "wsum")
        B.check_exact(got.acc.astype(np.float32), ref.acc, "acc")      # (every sum is an fp32 number)
        B.check_exact(got.wsum.astype(np.float32), ref.wsum, "wsum")
    assert len({tuple(w.tolist()) for w in B.pow2_windows(PATCH)}) == 3


@pytest.mark.parametrize("fault", [f for f in B.FAULTS if f != "unnormalised"])
def test_exact_checker_rejects_each_fault(fault):
    ref, got = _exact_pair(fault)
    with pytest.raises(AssertionError):
        B.check_exact(got.acc, ref.acc, "acc")
        B.check_exact(got.wsum, ref.wsum, "wsum")


def _random_case(of):
    lg = B.random_logits(80, 7, PATCH, seed=11)
    win = B.gaussian_windows(PATCH)
    ref = B.Blend64(7, 2, VOL, PATCH, OV, win, of).add(lg, POS)
    a32 = B.Blend32(7, 2, VOL, PATCH, OV, win, of).add(lg, POS)
    return lg, win, ref, a32


@pytest.mark.parametrize("of", ["probabilities", "logits"])
def test_atens_fp32_composition_passes_the_bounds_and_every_fault_is_outside_them(of):
    lg, win, ref, a32 = _random_case(of)
    r_a, r_w = B.r32_of(a32.acc.numpy(), ref.acc, ref.norm), B.r32_of(a32.wsum.numpy(), ref.wsum, ref.wsum)
    assert 0 < r_a < 2e-6 and r_w < 2e-6, (r_a, r_w)
    eps_a, eps_w = B.eps_of(r_a, ref.cnt), B.eps_of(r_w, ref.cnt)
    assert B.check_values(a32.acc.numpy(), ref.acc, eps_a * ref.norm, "acc") <= 0.25 + 1e-9
    assert B.check_values(a32.wsum.numpy(), ref.wsum, eps_w * ref.wsum, "wsum") <= 0.25 + 1e-9
    heat, prob, result = B.finalize64(ref.acc, ref.wsum, 2, of)
    hb = B.quotient_bound(heat, ref.norm[:2], ref.wsum, eps_a, eps_w)
    h32 = (a32.acc[:2] / a32.wsum).numpy()
    B.check_values(h32, heat, hb, "heat")
    if of == "probabilities":
        pb = B.quotient_bound(prob, ref.norm[2:], ref.wsum, eps_a, eps_w)
        B.check_values((a32.acc[2:] / a32.wsum).numpy(), prob, pb, "prob")
    else:
        import torch
        mean = ref.acc[2:] / ref.wsum
        sm32 = torch.softmax(torch.from_numpy(mean.astype(np.float32)), 0).numpy()
        r_sm = B.r32_of(sm32, B.softmax64(mean.astype(np.float32).astype(np.float64)), prob)
        pb = B.softmax_bound(prob, B.quotient_bound(mean, ref.norm[2:], ref.wsum, eps_a, eps_w), r_sm)
        B.check_values(torch.softmax(a32.acc[2:] / a32.wsum, 0).numpy(), prob, pb, "prob")
    for fault in B.FAULTS:
        mirror = 6 if fault == "no_flip_back" else 0
        bad = B.Blend64(7, 2, VOL, PATCH, OV, win, of, fault=fault).add(B.flip(lg, mirror, 2), POS, mirror=mirror, batch=4)
        with pytest.raises(AssertionError):
            if fault == "unnormalised":
                bh, bp, _ = B.finalize64(bad.acc, bad.wsum, 2, of, fault=fault)
                B.check_values(bh, heat, hb, "heat")
            else:
                B.check_values(bad.acc, ref.acc, eps_a * ref.norm, "acc")
                B.check_values(bad.wsum, ref.wsum, eps_w * ref.wsum, "wsum")


def test_one_ulp_and_fp16_helpers():
    q = np.array([1 / 3, 2 / 3, 1e-8, 0.0])
    B.check_one_ulp(q.astype(np.float32), q, "division")
    with pytest.raises(AssertionError):
        B.check_one_ulp((q * (1 + 3e-7)).astype(np.float32), q, "division")
    b = B.quotient_bound(q, q, np.ones(4), 0.0, 0.0, half=True)
    B.check_values(q.astype(np.float32).astype(np.float16), q, b, "fp16")
