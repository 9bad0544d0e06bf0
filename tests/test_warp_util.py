"""The CPU side of the mednet_warp_patches tests (tests/warp_util.py): the fp64 restatement against scipy and against numpy indexing,
the fp32 model through every check the GPU run goes through, and the fault models -- each must be refused wherever it changes a result."""
import numpy as np
import pytest

import warp_util as W


def test_fp64_restatement_against_scipy_map_coordinates():
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    shape, patch = (2, 9, 11, 13), (4, 5, 7)
    vol = rng.standard_normal(shape)
    worst = 0.0
    for trial in range(12):
        aff = W.random_affines(rng, 1, patch, shape, zoom=(0.5, 2.0), spread=2.0)[0]
        disp = rng.normal(0, 1.0, (3, 2, 3, 3)) if trial % 2 else None
        s = W.source_coordinates(aff, patch, disp, "f64")
        for border, mode in (("constant", "grid-constant"), ("edge", "nearest")):
            got = W.sample(vol, s, "linear", border, -1.25, "f64")
            want = np.stack([nd.map_coordinates(vol[c], s, order=1, mode=mode, cval=-1.25) for c in range(shape[0])])
            worst = max(worst, float(np.abs(got - want).max()))
    assert worst < 1e-13, worst


def test_fp64_restatement_of_identity_and_cube_symmetries_is_numpy_indexing():
    for case in W.identity_cases():
        for i, pos in enumerate(case["positions"]):
            sl = tuple(slice(p, p + n) for p, n in zip(pos, case["patch"]))
            assert np.array_equal(W.reference(case)[i][1], case["vol"][(slice(None),) + sl].astype(np.float64)), case["name"]
    seen = set()
    for case in W.symmetry_cases():
        for i, (pos, m) in enumerate(zip(case["positions"], case["matrices"])):
            seen.add(tuple(m.astype(int).ravel()))
            idx = np.stack(np.meshgrid(*(np.arange(8),) * 3, indexing="ij")).reshape(3, -1)
            # u = idx - 3.5, so 2u is odd and so is every entry of m @ 2u: + 7 makes it even
            src = ((m.astype(int) @ (2 * idx - 7)) + 7) // 2 + np.asarray(pos)[:, None]
            want = case["vol"][:, src[0], src[1], src[2]].reshape((-1, 8, 8, 8)).astype(np.float64)
            assert np.array_equal(W.reference(case)[i][1], want), case["name"]
            if np.array_equal(m, np.diag(np.diag(m))):   # flips alone: numpy's own flip of the crop
                crop = case["vol"][:, pos[0]:pos[0] + 8, pos[1]:pos[1] + 8, pos[2]:pos[2] + 8]
                axes = [1 + k for k in range(3) if m[k, k] < 0]
                assert np.array_equal(want, np.flip(crop, axes).astype(np.float64))
    assert len(seen) == 48


def test_the_fp32_model_passes_every_check_of_the_gpu_run():
    run = W.model_run()
    report = []
    for case in W.all_cases():
        W.check_case(case, run(case), report)
    with np.errstate(invalid="ignore"):
        for border in ("constant", "edge"):
            case = W.nonfinite_case(border)
            W.check_case(case, run(case))
    ratios = [r for r in report if "ratio" in r]
    assert ratios and max(r["ratio"] for r in ratios) <= 1 / 8 + 1e-12     # eps >= 8 r32 by construction
    assert all(r["r32"] < W.EPS_FLOOR / 8 for r in ratios), "the fp32 model leaves the floor: re-derive it"


def test_nearest_cases_leave_out_at_most_one_percent_and_the_margin_covers_the_fp32_coordinate_error():
    seen = 0
    for case in W.all_cases():
        if case["kind"] != "bound":
            continue
        for i in range(len(case["slots"])):
            # the coordinate's rounding budget in voxels, an upper bound: outside the margin fp32 and fp64 take the same index.
            # Without a lattice it is at most 2^-16.3 at these extents, with the lattice (sigma 1.5, up to 6 points) 2^-13.6.
            delta = 16 * W.U * W.coordinate_budget(case, i).max()
            assert delta < W.HALF_MARGIN / (2 if case["disp"] is not None else 8), (case["name"], delta)
            if case["interp"] == "nearest":
                assert W.left_out(case)[i].mean() <= W.LEFT_OUT_CAP, case["name"]
                seen += 1
    assert seen >= 12


def test_nonfinite_matrices_give_cval_or_a_volume_voxel():
    with np.errstate(invalid="ignore"):
        for border in ("constant", "edge"):
            case = W.nonfinite_case(border)
            out = W.model_run()(case)
            rows = [out[s, 1:4] for s in case["slots"]]
            assert all(np.isfinite(r).all() for r in rows)
            if border == "constant":
                assert np.all(rows[1] == -2.0) and np.all(rows[2] == -2.0)
                assert np.all((rows[0] == -2.0) | np.isin(rows[0], case["vol"]))
            else:
                assert all(np.isin(r, case["vol"]).all() for r in rows)


@pytest.mark.parametrize("fault", W.FAULTS)
def test_every_fault_is_refused_wherever_it_changes_a_result(fault):
    good, bad = W.model_run(), W.model_run(fault)
    exists = 0
    for case in W.all_cases():
        a, b = good(case), bad(case)
        if np.array_equal(W.bits(a), W.bits(b)):
            continue
        exists += 1
        assert W.rejected(case, b), f"{fault} changes {int((a != b).sum())} voxels of {case['name']} and passes its check"
    assert exists, f"{fault}: no case shows it"


@pytest.mark.parametrize("brick", W.BRICKS, ids=lambda b: "x".join(map(str, b)))
def test_a_dropped_partial_brick_is_refused_under_every_workgroup_mapping(brick):
    """The library has four mappings (option warp_brick); each leaves other voxels unwritten when its last partial brick is dropped."""
    good, bad = W.model_run(), W.model_run("drop_brick", brick)
    exists = 0
    for case in W.all_cases():
        if any(p % b for p, b in zip(case["patch"], brick)):
            exists += 1
            assert not np.array_equal(W.bits(good(case)), W.bits(bad(case))), case["name"]
            assert W.rejected(case, bad(case)), f"brick {brick}: {case['name']} passes with its partial bricks dropped"
    assert exists
