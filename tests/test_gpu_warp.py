"""mednet_warp_patches (csrc/warp.hip) and DevicePatchSampler(spatial=...) on the GPU.  Cases, references and checkers are those of
tests/warp_util.py, which tests/test_warp_util.py runs on the CPU model and its fault models; bounds and measured values:
profiles/spatial_augment_bounds.md.

A. exact cases, bit equality: identity = mednet_crop_patches, the 48 cube symmetries, dyadic coordinates, outside / cval / ties.
B. random rotations, scales and lattices against fp64: linear within eps * norm at every element, nearest equal away from
   half-integers (left-out share <= 1 %), heat maps within one grey level and equal away from ties.
C. footprint: every operand between guard bands (tests/fence.py), also with matrices that hold 2^30, NaN and -inf.
D. the sampler: a seeded batch equals the model applied to its own last_spatial; identity ranges = the plain crop; one training step."""
import numpy as np
import pytest
import torch

from mednet_hip import _lib as L
from mednet_hip import sampler as HS

import warp_index_sweep as S
import warp_util as W
from fence import Fence
from gpu_util import DEV

pytestmark = pytest.mark.gpu

_DT = {np.dtype(np.float16): L.F16, np.dtype(np.float32): L.F32, np.dtype(np.uint8): L.U8}


def gpu_run(case, put=None):
    """The library on one case -> the whole batch tensor as numpy.  `put`: where the operands go (a fence's put)."""
    put = put or (lambda t: t)
    dev = lambda a: put(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    vol, out = dev(case["vol"]), dev(W.blank_output(case))
    aff, slot = dev(case["affine"]), dev(np.asarray(case["slots"], dtype=np.int32))
    disp = None if case["disp"] is None else dev(case["disp"])
    HS.warp_patches(vol, aff, slot, out, 1, case["interp"], case["border"], case["cval"], disp)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_group(cases):
    report = []
    for case in cases:
        W.check_case(case, gpu_run(case), report)
    return report


# ------------------------------------------------------------------------------------------------ A. exact
def test_identity_equals_crop_patches_at_every_face():
    cases = W.identity_cases()
    run_group(cases)
    lib = L.lib()
    for case in cases:        # ... and the crop kernel's own output, bit for bit
        vol = torch.from_numpy(case["vol"]).to(DEV)
        want = torch.from_numpy(W.blank_output(case)).to(DEV)
        pos = torch.tensor(np.asarray(case["positions"], dtype=np.int32), device=DEV)
        slot = torch.tensor(case["slots"], dtype=torch.int32, device=DEV)
        c, d, h, w = vol.shape
        pd, ph, pw = case["patch"]
        L.check(lib.mednet_crop_patches(vol.data_ptr(), _DT[case["vol"].dtype], pos.data_ptr(), slot.data_ptr(), 3, want.data_ptr(),
                                        _DT[W.out_dtype(case)], c, d, h, w, c + 2, 1, pd, ph, pw, L.stream()), "crop_patches")
        torch.cuda.synchronize()
        assert np.array_equal(W.bits(gpu_run(case)), W.bits(want.cpu().numpy())), case["name"]


def test_cube_symmetries_equal_numpy_indexing():
    cases = W.symmetry_cases()
    assert len({tuple(m.ravel()) for c in cases for m in c["matrices"]}) == 48
    run_group(cases)


def test_dyadic_coordinates_equal_fp64_rounded_once():
    run_group(W.dyadic_cases())


def test_outside_the_volume_cval_and_heat_map_ties():
    cases = W.outside_cases()
    run_group(cases)
    tie = [c for c in cases if c["name"] == "outside-ties-u8"][0]
    ref = W.reference(tie)[0][1]
    assert (np.abs(ref - np.floor(ref) - 0.5) == 0).mean() > 0.3      # the case does hold ties
    got = gpu_run(tie)[tie["slots"][0], 1:2]
    assert np.all(got[np.abs(ref - np.floor(ref) - 0.5) == 0] % 2 == 0)


# ------------------------------------------------------------------------------------------------ B. bounds
@pytest.mark.parametrize("case", W.bound_cases(), ids=lambda c: c["name"])
def test_random_rotations_scales_and_lattices_against_fp64(case):
    report = []
    W.check_case(case, gpu_run(case), report)
    for r in report:
        print("[measure] " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in r.items()))


# ------------------------------------------------------------------------------------------------ C. footprint
def fenced_equals_unfenced(case):
    plain = gpu_run(case)
    with Fence() as fence:
        got = gpu_run(case, fence.put)
        fence.check()
    assert np.array_equal(W.bits(got), W.bits(plain)), case["name"] + ": the fenced result differs"
    if got.dtype == np.float32:
        assert not np.isnan(got).any(), case["name"] + ": a guard's NaN reached the output"
    return got


@pytest.mark.parametrize("case", W.footprint_cases(), ids=lambda c: c["name"])
def test_footprint_rotations_and_zoom_out_between_guard_bands(case):
    W.check_case(case, fenced_equals_unfenced(case))


def test_every_workgroup_mapping_gives_the_same_bits():
    """Option warp_brick is an A/B knob of tools/run_sampler.py: results never depend on it.  The ragged patch, lattice on."""
    lib = L.lib()
    cases = [c for c in W.footprint_cases() if c["border"] == "constant"]
    try:
        want = [gpu_run(c) for c in cases]
        for variant in range(len(W.BRICKS)):
            lib.mednet_set_option(b"warp_brick", variant)
            for c, w in zip(cases, want):
                got = gpu_run(c)
                W.check_case(c, got)
                assert np.array_equal(W.bits(got), W.bits(w)), (variant, c["name"])
    finally:
        lib.mednet_set_option(b"warp_brick", W.BRICKS.index(W.BRICK))


@pytest.fixture(scope="module")
def index_sweep_green(tmp_path_factory):
    """The host sweep of csrc/warp_index.h (tests/warp_index_sweep.py) in a PLAIN build, once per module: every tap index inside
    [0, n) for NaN, +-inf and |s| >= 2^31.  A failure here fails the non-finite cases BEFORE they launch anything.  The build under
    the sanitizers belongs to the CPU suite alone (tests/test_warp_index_host.py) and is never made here."""
    plain = S.plain_compiler()
    assert plain is not None, "no host C++ compiler: the index header cannot be swept"
    S.sweep(str(tmp_path_factory.mktemp("warp_index")), plain, sanitize=False)


@pytest.mark.parametrize("border", ["constant", "edge"])
def test_footprint_with_matrices_holding_2_to_30_nan_and_inf(border, index_sweep_green):
    """Runs only with the host sweep of the index header green: the conversion of such coordinates is clamped in float first."""
    with np.errstate(invalid="ignore"):
        case = W.nonfinite_case(border)
        got = fenced_equals_unfenced(case)
        W.check_case(case, got)
    rows = [got[s, 1:4] for s in case["slots"]]
    if border == "constant":
        assert np.all(rows[1] == -2.0) and np.all(rows[2] == -2.0)
    else:
        assert all(np.isin(r, case["vol"]).all() for r in rows)


# ------------------------------------------------------------------------------------------------ D. sampler
SPATIAL = dict(rotation=((-0.4, 0.4), (-0.3, 0.3), (-0.5, 0.5)), scale=(0.8, 1.25), mirror_axes=(0, 1, 2), elastic=(4, 1.5))
SAMPLER_SEED = 4      # chosen on the CPU: every label patch leaves out under 1 % of its voxels


def sampler_volumes(n_hm):
    rng = np.random.default_rng(31)
    shape = (20, 18, 22)
    images = [(rng.standard_normal((2,) + shape) * 40 + 100).astype(np.float16) for _ in range(2)]
    labels = [rng.integers(0, 3, (1,) + shape).astype(np.uint8) for _ in range(2)]
    heatmaps = [rng.integers(0, 256, (n_hm,) + shape).astype(np.uint8) for _ in range(2)] if n_hm else None
    return images, labels, heatmaps


def sampler_cases(ds, batch, images, labels, heatmaps, patch, indices):
    """One single-row case per sample and source volume, with the sampler's own matrices and lattices."""
    sp, last = ds.spatial, ds.last_spatial
    n_hm = 0 if heatmaps is None else heatmaps[0].shape[0]
    out = []
    for k, i in enumerate(indices):
        subj = i % len(images)
        disp = None if last["lattice"] is None else last["lattice"][k][None]
        aff = last["affine"][k].reshape(1, 12)
        jobs = [("data", images[subj], batch["data"][k], "linear", sp.border_data, sp.data_cval),
                ("label", labels[subj], batch["label"][k, n_hm:], "nearest", sp.border_label, sp.label_cval)]
        if n_hm:
            jobs.append(("heat", heatmaps[subj], batch["label"][k, :n_hm], "linear", sp.border_label, sp.label_cval))
        for what, vol, got, interp, border, cval in jobs:
            case = W.make_case(f"sampler-{what}-{k}", "bound", vol, patch, aff, interp, border, cval, disp)
            full = W.blank_output(case)
            full[case["slots"][0], 1:1 + vol.shape[0]] = got.cpu().numpy()
            out.append((case, full))
    return out


def test_seeded_sampler_batch_equals_the_model_on_its_own_last_spatial():
    images, labels, heatmaps = sampler_volumes(2)
    patch, indices = [8, 9, 10], [0, 1, 2, 3]
    ds = HS.DevicePatchSampler(images, labels, patch, samples_per_subject=2, heatmaps=heatmaps, class_probabilities=[0.2, 0.4, 0.4],
                               device=DEV, spatial=HS.SpatialAugmentation(**SPATIAL))
    np.random.seed(SAMPLER_SEED)
    b = ds.batch(indices)
    torch.cuda.synchronize()
    assert tuple(b["data"].shape) == (4, 2, 8, 9, 10) and b["data"].dtype == torch.float32
    assert tuple(b["label"].shape) == (4, 3, 8, 9, 10) and b["label"].dtype == torch.uint8        # heat maps first, the class map last
    assert b["spatial"].shape == (4, 3, 4) and b["spatial"].dtype == np.float32
    assert np.array_equal(b["spatial"][:, :, 3], b["patch_position"] + (np.asarray(patch) - 1) / 2)
    for case, full in sampler_cases(ds, b, images, labels, heatmaps, patch, indices):
        W.check_case(case, full)


def test_identity_ranges_give_exactly_the_plain_batch():
    images, labels, heatmaps = sampler_volumes(1)
    kw = dict(samples_per_subject=2, heatmaps=heatmaps, class_probabilities=[0.2, 0.4, 0.4], device=DEV)
    np.random.seed(9)
    plain = HS.DevicePatchSampler(images, labels, [8, 9, 10], **kw).batch([0, 1, 2, 3])
    np.random.seed(9)
    same = HS.DevicePatchSampler(images, labels, [8, 9, 10], spatial=HS.SpatialAugmentation(), **kw).batch([0, 1, 2, 3])
    assert np.array_equal(plain["patch_position"], same["patch_position"])
    assert torch.equal(plain["data"], same["data"]) and torch.equal(plain["label"], same["label"])
    # identity RANGES consume draws, so under one seed the positions move.  The spatial=None sampler is therefore replayed with the
    # spatial draws skipped: its position() hands back the positions the identity-range batch drew, everything else is its own path
    np.random.seed(9)
    ident = HS.SpatialAugmentation(rotation=((0, 0),) * 3, scale=(1, 1), border_data="constant", data_cval=5.0)
    b = HS.DevicePatchSampler(images, labels, [8, 9, 10], spatial=ident, **kw).batch([0, 1, 2, 3])
    assert ident.calls_per_sample() == 6
    assert np.array_equal(b["spatial"][:, :, :3], np.stack([np.eye(3, dtype=np.float32)] * 4))
    replay = HS.DevicePatchSampler(images, labels, [8, 9, 10], **kw)
    drawn = iter(zip([0, 1, 0, 1], b["patch_position"], b["selected_class"]))
    replay.position = lambda idx: next(drawn)
    r = replay.batch([0, 1, 2, 3])
    assert np.array_equal(r["patch_position"], b["patch_position"]) and "spatial" not in r
    assert torch.equal(r["data"], b["data"]) and torch.equal(r["label"], b["label"])
    for k, (p, subj) in enumerate(zip(b["patch_position"], [0, 1, 0, 1])):     # ... and numpy's slicing, independently of the crop
        sl = (slice(None), slice(p[0], p[0] + 8), slice(p[1], p[1] + 9), slice(p[2], p[2] + 10))
        assert np.array_equal(b["data"][k].cpu().numpy(), images[subj][sl].astype(np.float32))
        assert np.array_equal(b["label"][k].cpu().numpy(), np.concatenate([heatmaps[subj][sl], labels[subj][sl]]))


def test_one_training_step_on_a_warped_batch_gives_a_finite_loss():
    import mednet_hip
    from mednet_hip.train import SegmentationStep
    from mednet_hip.unet import model as HM
    from oracle import ref_cpu as O
    rng = np.random.default_rng(32)
    images = [(rng.standard_normal((1, 24, 24, 24)) * 2).astype(np.float16) for _ in range(2)]
    labels = [rng.integers(0, 4, (1, 24, 24, 24)).astype(np.uint8) for _ in range(2)]
    ds = HS.DevicePatchSampler(images, labels, [16, 16, 16], samples_per_subject=2, device=DEV, augment=True,
                               spatial=HS.SpatialAugmentation(**SPATIAL))
    np.random.seed(3)
    batch = ds.batch([0, 1, 2, 3])
    assert bool(torch.isfinite(batch["data"]).all()) and int(batch["label"].max()) <= 3
    with mednet_hip.precision("bf16"):
        net = O.keyed_init_(HM.ResidualUNet3D(in_channels=1, out_channels=4, final_sigmoid=False, f_maps=[32, 64])).to(DEV)
        step = SegmentationStep(net, loss_weight=[0.05, 1, 1, 1.0], lr=1e-3)
        loss = float(step(batch))
        step.flat.release()
    assert np.isfinite(loss)
