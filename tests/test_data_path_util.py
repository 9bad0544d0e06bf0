"""CPU side of tests/test_gpu_data_path.py: (1) the lattice builders meet their premises -- fl(grange + 1e-7f) = grange, t in {0, 1}
(or {0, 1/2, 1}), every block's sum below 2^24; (2) the fp64 restatement of the augmentation agrees with oracle/ref_augment.apply
within a few fp32 roundings in the norm of the bound; (3) every checker of parts A and B passes a numpy model of augment.hip's block
decomposition -- partials per 2048 voxels, the finalize loops of stride 64, the per-(sample, channel) indexing of parameters and
statistics, fp32 arithmetic -- and refuses the model with a fault injected; (4) what the suite's older whole-tensor bound makes of
the same faults; (5) the geometry of overlapping stitch windows (o0 > o1) and the oracle's rule for them."""
import numpy as np
import pytest

import gpu_util as U
import test_gpu_data_path as T
from oracle import ref_augment as A
from oracle import ref_predict as P

F32 = np.float32
FAULTS = ("ragged", "first64", "channel0", "sample_range")


# ------------------------------------------------------------------------------------------------ a model of augment.hip
def _fma32(a, b, c):
    """fl32(a * b + c) with one rounding (the product of two fp32 numbers is exact in fp64; the fp64 sum rounds far below fp32)."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F32)


def _gamma_map(x, add, gmin, grange, gamma):
    t = (x + F32(add) - gmin) / (grange + F32(1e-7))
    assert t.dtype == F32
    return _fma32(np.power(np.maximum(t, F32(0)), F32(gamma)), grange, gmin)


def aug_model(x, params, fault=None):
    """x [b, c, S] fp32, params [b, c, 3] -> the output of the five kernels, fp32 throughout.  Faults: "ragged": the last block is
    skipped by all three passes over the data when it is ragged and not the only one; "first64": both finalize kernels stop after
    64 partials; "channel0": aug_apply reads the parameters of the sample's channel 0; "sample_range": every channel is clipped to
    the sample's ends instead of its own."""
    x = np.asarray(x, dtype=F32)
    params = np.asarray(params, dtype=F32)
    b, c, S = x.shape
    nb = U.aug_blocks(S)
    live = (nb - 1) * U.AUG_BLOCK_VOX if fault == "ragged" and S % U.AUG_BLOCK_VOX and nb > 1 else S
    nbl = U.aug_blocks(live)
    nfin = min(nbl, U.AUG_FINALIZE_STRIDE) if fault == "first64" else nbl
    edges = [(k * U.AUG_BLOCK_VOX, min((k + 1) * U.AUG_BLOCK_VOX, live)) for k in range(nbl)]
    out = x.copy()
    for i in range(b):
        pmn = np.asarray([[x[i, ch, a:e].min() for a, e in edges] for ch in range(c)], dtype=F32)      # aug_minmax_kernel
        pmx = np.asarray([[x[i, ch, a:e].max() for a, e in edges] for ch in range(c)], dtype=F32)
        cmn, cmx = pmn[:, :nfin].min(1), pmx[:, :nfin].max(1)                                          # aug_finalize1_kernel
        gmin, gmax = (cmn + params[i, :, 0]).min(), (cmx + params[i, :, 0]).max()
        grange = F32(gmax - gmin)
        lo = np.asarray([_gamma_map(cmn[ch], params[i, ch, 0], gmin, grange, params[i, ch, 1]) for ch in range(c)], dtype=F32)
        hi = np.asarray([_gamma_map(cmx[ch], params[i, ch, 0], gmin, grange, params[i, ch, 1]) for ch in range(c)], dtype=F32)
        if fault == "sample_range":
            lo[:], hi[:] = lo.min(), hi.max()
        for ch in range(c):
            g = _gamma_map(x[i, ch, :live], params[i, ch, 0], gmin, grange, params[i, ch, 1])
            part = np.asarray([g[a:e].sum(dtype=F32) for a, e in edges], dtype=F32)                    # aug_sum_kernel
            mean = F32(part[:nfin].astype(np.float64).sum() / np.float64(S))                           # aug_finalize2_kernel
            add, gamma, factor = params[i, 0 if fault == "channel0" else ch]                           # aug_apply_kernel
            g = _gamma_map(x[i, ch, :live], add, gmin, grange, gamma)
            d = g - mean
            assert d.dtype == F32
            out[i, ch, :live] = np.minimum(np.maximum(_fma32(d, factor, mean), lo[ch]), hi[ch])
    return out


def a_checkers_refusing(case, fn):
    """The names of part A's checkers on the shifted lattice that refuse `fn(x, params)`."""
    refused = set()
    for name, factor, check in (("mean", 0.0, U.check_aug_lattice_mean), ("extremes", 2.0 ** 40, U.check_aug_lattice_extremes),
                                ("factor", 0.5, lambda got, cs, what: U.check_aug_lattice_factor(got, cs, 0.5, what)),
                                ("factor", 1.5, lambda got, cs, what: U.check_aug_lattice_factor(got, cs, 1.5, what))):
        for gamma in T.GAMMAS:
            try:
                check(fn(case.x, U.aug_lattice_params(case, gamma, factor)), case, "model")
            except AssertionError:
                refused.add(name)
    return refused


# ------------------------------------------------------------------------------------------------ (1) premises
def test_shapes_and_lattice_premises():
    v = {k: int(np.prod(s)) for k, s in T.SHAPES.items()}
    assert [v[k] for k in ("tiny", "block", "plus1", "three", "trip2")] == [231, 2048, 2049, 4305, 131073]
    assert U.aug_blocks(v["trip2"]) == 65
    assert float(F32(2.0) + F32(1e-7)) == 2.0 and float(F32(1.0) + F32(1e-7)) != 1.0          # why H - L >= 2
    for key, b, c in T.LATTICE_CASES:
        case = T.lattice_case(key, b, c)                     # (the builder asserts the premises; once more, and the means)
        U.aug_lattice_premises(case)
        mean = U.aug_lattice_mean32(case)
        assert len(np.unique(case.nhigh)) == b * c and mean.shape == (b, c)
        nb = U.aug_blocks(case.spatial)
        assert bool(case.mask[:, :, (nb - 1) * U.AUG_BLOCK_VOX:].any(-1).all())               # the last (ragged) block holds an H
    for key in T.SHAPES:
        U.aug_two_channel_case(f"dp:two:{key}", 2, T.SHAPES[key])                             # asserts t in {0, 1/2, 1}


# ------------------------------------------------------------------------------------------------ (2) the fp64 restatement
@pytest.mark.parametrize("cs", T.RANDOM_CASES, ids=[f"{k}-{b}x{c}-{kind}-{p}" for k, b, c, kind, p in T.RANDOM_CASES])
def test_fp64_restatement_agrees_with_the_fp32_oracle_and_the_model_passes(cs):
    case = T.random_case(*cs)
    ref = U.augment_ref64(case.x, case.params)
    r32, eps = U.aug_eps(case.x, case.params, ref, str(cs))
    assert r32 <= 2.0 ** -22, f"oracle fp32 against fp64: {r32:.3e} of the norm -- the norm does not fit the operation"
    assert eps == U.AUG_EPS_FLOOR
    U.check_augment(A.apply(case.x, case.params), ref, eps, "the fp32 oracle")
    if cs[0] != "trip2" or cs[1] == 1:
        U.check_augment(aug_model(case.x, case.params), ref, eps, "the model")
    if U.aug_blocks(case.spatial) > U.AUG_FINALIZE_STRIDE:       # the sample's extremes sit behind partial 64
        s = case.x + case.params[:, :, 0:1]
        assert bool((s.reshape(case.b, -1).argmax(1) % case.spatial >= 64 * U.AUG_BLOCK_VOX).all())
        assert bool((s.reshape(case.b, -1).argmin(1) % case.spatial >= 64 * U.AUG_BLOCK_VOX - 1).all())


# ------------------------------------------------------------------------------------------------ (3) faults
@pytest.mark.parametrize("key,b,c", [t for t in T.LATTICE_CASES if t[2] <= 3], ids=lambda v: str(v))
def test_part_a_passes_the_model_and_refuses_each_fault(key, b, c):
    case = T.lattice_case(key, b, c)
    S = case.spatial
    assert a_checkers_refusing(case, aug_model) == set()
    if S % U.AUG_BLOCK_VOX and U.aug_blocks(S) > 1:
        assert {"mean", "extremes"} <= a_checkers_refusing(case, lambda x, p: aug_model(x, p, "ragged"))
    if U.aug_blocks(S) > U.AUG_FINALIZE_STRIDE:
        assert "mean" in a_checkers_refusing(case, lambda x, p: aug_model(x, p, "first64"))
    if c > 1:
        assert "factor" in a_checkers_refusing(case, lambda x, p: aug_model(x, p, "channel0"))


@pytest.mark.parametrize("key", list(T.SHAPES))
def test_identity_constant_and_two_channel_checks_on_the_model(key):
    shape = T.SHAPES[key]
    ident = U.aug_lattice_case(f"dp:ident:{key}", 3, 2, shape, lh=[(0, 2), (0, 64), (0, 4096)], shifted=False)
    assert np.array_equal(aug_model(ident.x, U.aug_lattice_params(ident, 1.0, 1.0, shift=False)), ident.x)
    const = np.empty((3, 1, ident.spatial), dtype=F32)
    const[0], const[1], const[2] = -5.0, 0.0, 4096.0
    for gamma, factor in ((0.7, 0.0), (1.3, 1.7), (0.7, 2.0 ** 40)):
        prm = np.zeros((3, 1, 3), dtype=F32)
        prm[:, :, 1], prm[:, :, 2] = gamma, factor
        assert np.array_equal(aug_model(const, prm), const)
    two = U.aug_two_channel_case(f"dp:two:{key}", 2, shape)
    for gamma in (0.7, 1.3):
        prm = np.zeros((2, 2, 3), dtype=F32)
        prm[:, :, 0], prm[:, :, 1], prm[:, :, 2] = two.add, gamma, 2.0 ** 40
        ref = U.augment_ref64(two.x, prm)
        _, eps = U.aug_eps(two.x, prm, ref, "two-channel")
        U.check_aug_two_channel(aug_model(two.x, prm), two, ref, eps, "model")
        with pytest.raises(AssertionError):     # channel 0's voxels at t = 1/2 go to H, channel 1's to L
            U.check_aug_two_channel(aug_model(two.x, prm, "sample_range"), two, ref, eps, "sample_range")


@pytest.mark.parametrize("cs", [c for c in T.RANDOM_CASES if c[2] in (2, 3) and (c[0] != "trip2" or c[1] == 1)],
                         ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-{c[3]}-{c[4]}")
def test_part_b_refuses_each_fault(cs):
    case = T.random_case(*cs)
    ref = U.augment_ref64(case.x, case.params)
    _, eps = U.aug_eps(case.x, case.params, ref, str(cs))
    S, nb = case.spatial, U.aug_blocks(case.spatial)
    faults = ["channel0"]
    if bool(ref.sure_lo.any() or ref.sure_hi.any()):
        faults.append("sample_range")           # (a factor below 1 clips nothing: the channel's ends are not used)
    if S % U.AUG_BLOCK_VOX and nb > 1:
        faults.append("ragged")
    if nb > U.AUG_FINALIZE_STRIDE:
        faults.append("first64")
    for fault in faults:
        with pytest.raises(AssertionError):
            U.check_augment(aug_model(case.x, case.params, fault), ref, eps, fault)


# ------------------------------------------------------------------------------------------------ (4) the older whole-tensor bound
def whole_tensor_error(fault):
    """tests/test_gpu_predict.py::test_device_augmentation_matches_the_numpy_restatement's data, parameters and metric."""
    g = np.random.Generator(np.random.PCG64(11))
    data = (g.standard_normal((3, 2, 9, 17, 23)) * 40 + 100).astype(F32)
    state = np.random.get_state()
    np.random.seed(5)
    params = A.draw_parameters(3, 2)
    np.random.set_state(state)
    want = A.apply(data, params).reshape(3, 2, -1)
    got = aug_model(data.reshape(3, 2, -1), params, fault)
    ref = U.augment_ref64(data, params)
    _, eps = U.aug_eps(data, params, ref, "whole tensor")
    try:
        U.check_augment(got, ref, eps, str(fault))
        new_ok = True
    except AssertionError:
        new_ok = False
    return float(np.abs(got - want).max() / np.abs(want).max()), new_ok


def test_what_the_whole_tensor_bound_makes_of_the_faults():
    """The model passes 2e-5 * max |want|.  The issue expected the bound to ACCEPT wrong per-channel parameters and statistics on that
    test's data; it does not -- the drawn contrast factors of a sample's two channels differ by tenths, the clipped voxels move by
    tens of grey values -- so both faults are seen there (recorded in profiles/data_path_bounds.md).  What it cannot see is the
    second trip of the finalize loops and anything below 2e-5 of the largest voxel: "first64" and "ragged" do not exist at 3519 voxels
    (two blocks, the last ragged one IS reached by "ragged"), and the per-element bound of part B refuses all of them."""
    err, new_ok = whole_tensor_error(None)
    assert err <= 2e-5 and new_ok
    for fault in ("channel0", "sample_range"):
        err, new_ok = whole_tensor_error(fault)
        assert err > 2e-5 and not new_ok, (fault, err)
    err, new_ok = whole_tensor_error("first64")
    assert err <= 2e-5 and new_ok              # two partials per channel: the fault does not exist at this shape


def test_a_mean_off_by_one_voxel_of_131073_passes_the_old_bound_and_fails_the_exact_check():
    case = T.lattice_case("trip2", 2, 3)
    prm = U.aug_lattice_params(case, 1.0, 0.0)
    good, bad = aug_model(case.x, prm), aug_model(case.x, prm, "first64")
    assert np.abs(bad - good).max() <= 2e-5 * np.abs(good).max()
    U.check_aug_lattice_mean(good, case, "model")
    with pytest.raises(AssertionError):
        U.check_aug_lattice_mean(bad, case, "first64")


# ------------------------------------------------------------------------------------------------ (5) the stitch windows
def writers(dims, patch, ov):
    """-> pos, and per voxel of the volume the list of grid rows whose cropped window covers it."""
    from mednet_hip import predict as HP
    pos = HP.grid_positions(dims, patch, ov)
    _, shape = P.crop_window(patch, ov)
    who = {}
    for i, p in enumerate(pos):
        for z in range(p[0], min(p[0] + shape[0], dims[0])):
            for y in range(p[1], min(p[1] + shape[1], dims[1])):
                for x in range(p[2], min(p[2] + shape[2], dims[2])):
                    who.setdefault((z, y, x), []).append(i)
    return pos, who


def test_deep_pad_geometry_two_patches_write_plane_4_and_the_later_wins():
    tag, shape, patch, ov, mode, nh, ncls, bs = [c for c in P.PREDICT_CASES if c[0] == "deep_pad"][0]
    dims = shape[1:]
    pos, who = writers(dims, patch, ov)
    assert ov[0] > ov[1] and len(pos) == 4
    shared = {v: w for v, w in who.items() if len(w) > 1}
    assert shared and {v[0] for v in shared} == {4} and {tuple(w) for w in shared.values()} == {(0, 2), (1, 3)}
    assert len(shared) == dims[1] * dims[2]                                    # the whole plane z = 4
    assert all(w[0] // bs != w[1] // bs for w in shared.values())              # batch size 2: different launches (the golden case)
    assert all(w[0] // 4 == w[1] // 4 for w in shared.values())                # GridPredictor's default 4: one launch
    data = np.stack([np.full((1,) + tuple(patch), i + 1, dtype=np.uint8) for i in range(4)])
    res = np.zeros((1,) + tuple(dims), dtype=np.uint8)
    P.add_processed_batch(res, data, pos, ov)
    for v, w in who.items():
        assert res[(0,) + v] == max(w) + 1                                     # the later row
    rev = np.zeros_like(res)
    P.add_processed_batch(rev, data[::-1], pos[::-1], ov)
    for v, w in who.items():
        assert rev[(0,) + v] == min(w) + 1                                     # rows reversed: the later ROW is the earlier patch


def test_overlap_cases_of_the_gpu_module_share_whole_planes():
    for tag, dims, patch, ov in T.OVERLAP_CASES:
        assert ov[0] > ov[1]
        pos, who = writers(dims, patch, ov)
        shared = [v for v, w in who.items() if len(w) > 1]
        planes = {v[0] for v in shared}
        assert len(who) == int(np.prod(dims)) and len(shared) == len(planes) * dims[1] * dims[2] and dims[1] * dims[2] >= 1024
