"""The axis tables of mednet_hip.resample and the numpy model / checkers of tests/resample_util.py, on the CPU: the table facts of
DESIGN.md section 29 bit for bit, the module's tables against the model's independent restatement, the torch trilinear cross-check,
and every checker of tests/test_gpu_resample.py rejecting the fault it is there for."""
import numpy as np
import pytest
import torch

import resample_util as R
from mednet_hip import resample as M

CASES = [((12, 10, 14), (19, 23, 17)), ((33, 35, 130), (16, 18, 65)), ((29, 9, 9), (4, 9, 9)), ((1, 5, 1), (3, 1, 4)), ((8, 12, 16), (16, 6, 32))]


def _rows(table):
    start, count, weight, _ = table
    return [(int(s), weight[i, :c].tolist()) for i, (s, c) in enumerate(zip(start, count))]


@pytest.mark.parametrize("kind", ["nearest", "linear", "cubic"])
@pytest.mark.parametrize("n", [1, 2, 7, 64])
def test_identity_table(kind, n):
    for aa in (False, True):
        start, count, weight, taps = M.axis_table(n, n, kind, aa)
        assert taps == 1 and (count == 1).all() and (start == np.arange(n)).all() and (weight == np.float32(1.0)).all()
        assert M.is_identity((start, count, weight, taps))
    assert not M.is_identity(M.axis_table(4, 5, "linear", True))


@pytest.mark.parametrize("kind", ["nearest", "linear", "cubic"])
def test_one_source_voxel_folds_onto_index_zero(kind):
    for n_out in (1, 3, 8):
        start, count, weight, taps = M.axis_table(1, n_out, kind, True)
        assert taps == 1 and (start == 0).all() and (count == 1).all() and (weight == np.float32(1.0)).all()


def test_times_two_upsampling_rows():
    rows = _rows(M.axis_table(6, 12, "linear", True))
    assert rows[0] == (0, [1.0]) and rows[-1] == (5, [1.0])
    for i in range(1, 11):
        assert rows[i] == ((i - 1) // 2, [0.75, 0.25] if i % 2 else [0.25, 0.75]), (i, rows[i])
    w = M.axis_table(6, 12, "linear", True)[2]
    assert w[0].tolist() == [1.0, 0.0] and w[-1].tolist() == [1.0, 0.0]          # [1, 0] at the ends: the unused slot is 0


def test_half_antialiased_rows_are_dyadic():
    rows = _rows(M.axis_table(12, 6, "linear", True))
    assert rows[0] == (0, [0.5, 0.375, 0.125]) and rows[-1] == (9, [0.125, 0.375, 0.5])
    for i in range(1, 5):
        assert rows[i] == (2 * i - 1, [0.125, 0.375, 0.375, 0.125]), (i, rows[i])
    # without the stretch the filter falls between the voxels: 1/2, 1/2
    assert _rows(M.axis_table(12, 6, "linear", False))[2] == (4, [0.5, 0.5])


def test_rows_stay_inside_the_source_and_sum_to_one():
    for kind in ("nearest", "linear", "cubic"):
        for aa in (False, True):
            for n_in, n_out in ((7, 13), (13, 7), (29, 4), (130, 65), (9, 9), (2, 64), (64, 2), (1, 5), (5, 1), (35, 18)):
                start, count, weight, taps = M.axis_table(n_in, n_out, kind, aa)
                assert start.dtype == np.int32 and count.dtype == np.int32 and weight.dtype == np.float32 and weight.shape == (n_out, taps)
                assert (start >= 0).all() and (count >= 1).all() and (start + count <= n_in).all() and count.max() == taps
                assert abs(weight.astype(np.float64).sum(1) - 1.0).max() <= taps * 2.0 ** -24
                for i in range(n_out):
                    assert (weight[i, count[i]:] == 0).all()


def test_module_tables_equal_the_models_restatement():
    for kind in ("nearest", "linear", "cubic"):
        for aa in (False, True):
            for n_in, n_out in ((7, 13), (13, 7), (29, 4), (130, 65), (12, 19), (10, 23), (14, 17), (8, 16), (16, 8), (1, 4), (5, 1)):
                a, b = M.axis_table(n_in, n_out, kind, aa), R.model_table(n_in, n_out, kind, aa)
                assert a[3] == b[3] and (a[0] == b[0]).all() and (a[1] == b[1]).all(), (kind, aa, n_in, n_out)
                # both round fp64 weights to fp32 once; their fp64 values may differ in the last place (Horner form, order of the sum)
                assert np.abs(a[2].astype(np.float64) - b[2]).max() <= 2.0 ** -23, (kind, aa, n_in, n_out)
    for n_in, n_out in ((8, 16), (16, 8), (12, 24), (12, 6), (9, 9)):      # dyadic rows: bit for bit
        assert (M.axis_table(n_in, n_out, "linear", True)[2] == R.model_table(n_in, n_out, "linear", True)[2]).all()


def test_taps_limit_and_arguments():
    assert M.axis_table(60 * 4, 8, "linear", True)[3] <= 64
    with pytest.raises(ValueError, match="taps"):
        M.axis_table(2048, 16, "linear", True)
    with pytest.raises(ValueError, match="taps"):
        M.axis_table(2048, 64, "cubic", True)
    assert M.axis_table(2048, 16, "linear", False)[3] == 2
    with pytest.raises(ValueError, match="kind"):
        M.axis_table(4, 4, "lanczos", True)
    with pytest.raises(ValueError, match="extents"):
        M.axis_table(0, 4, "linear", True)


@pytest.mark.parametrize("shape,size", [((7, 9, 11), (13, 9, 20)), ((12, 10, 14), (19, 23, 17)), ((9, 8, 7), (4, 5, 3))])
def test_linear_without_antialiasing_is_torch_trilinear(shape, size):
    vol = np.random.default_rng(5).standard_normal((2,) + shape)
    want = torch.nn.functional.interpolate(torch.from_numpy(vol)[None], size=size, mode="trilinear", align_corners=False)[0].numpy()
    tables = [M.axis_table(n, m, "linear", False) for n, m in zip(shape, size)]
    got = R.resample64(vol, tables)
    err = float(np.abs(got - want).max())
    print(f"trilinear cross-check {shape} -> {size}: max abs difference {err:.3e}")
    assert err <= 1e-5
    # a convention error shows up at >= 1e-2
    for fault in ("align_corners",):
        bad = R.resample64(vol, R.tables_for(shape, size, "linear", False, fault))
        assert float(np.abs(bad - want).max()) >= 1e-2


# ---------------------------------------------------------------------------------------------- the checkers reject their faults
def _checked(vol, shape, size, kind, aa, tables):
    """What the GPU tests do with a kernel's result, here with the fp32 model of `tables` in the kernel's place."""
    good = [M.axis_table(n, m, kind, aa) for n, m in zip(shape, size)]
    return R.check_bounded(R.resample32(vol, tables), R.resample64(vol, good), R.error_bound(vol, good), f"{kind} {shape} -> {size}")


@pytest.mark.parametrize("shape,size,kind,aa", [((12, 10, 14), (19, 23, 17), "linear", True), ((33, 35, 130), (16, 18, 65), "linear", True),
                                                ((29, 9, 9), (4, 9, 9), "cubic", True), ((12, 10, 14), (19, 23, 17), "cubic", False)])
def test_fp32_model_passes_the_bound_and_table_faults_do_not(shape, size, kind, aa):
    vol = R.random_volume(3, (2,) + shape)
    frac = _checked(vol, shape, size, kind, aa, R.tables_for(shape, size, kind, aa))
    print(f"fp32 model, {kind} aa={aa} {shape} -> {size}: largest observed fraction of the bound {frac:.3f}")
    assert frac <= 1.0
    # (two-tap linear rows give the edge voxel the whole weight under either border rule: folding and renormalising part ways
    #  only with more than two taps)
    shrinks = aa and any(n > m for n, m in zip(shape, size))
    faults = ["align_corners"] + (["renormalise"] if kind == "cubic" or shrinks else []) + (["no_stretch"] if shrinks else [])
    for fault in faults:
        with pytest.raises(AssertionError, match="outside the bound"):
            _checked(vol, shape, size, kind, aa, R.tables_for(shape, size, kind, aa, fault))


@pytest.mark.parametrize("shape,size", [((8, 12, 16), (16, 24, 32)), ((8, 12, 16), (4, 6, 8)), ((8, 12, 16), (16, 6, 32))])
def test_integer_lattice_is_exact_in_fp32(shape, size):
    """Integers in [-512, 512] under the dyadic tables: every product and partial sum is an fp32 number, so the fp32 chains equal
    the fp64 model bit for bit -- in ANY association, which is why the association fault is shown on a non-dyadic case below."""
    vol = R.integer_volume(1, (2,) + shape)
    tables = [M.axis_table(n, m, "linear", True) for n, m in zip(shape, size)]
    want = R.resample64(vol, tables)
    R.check_exact(R.resample32(vol, tables), want, "fp32 model")
    assert (want.astype(np.float32).astype(np.float64) == want).all()
    R.check_exact(R.resample32(vol, tables, order=(1, 2, 0)), want, "fp32 model, y before x")
    with pytest.raises(AssertionError, match="differ"):
        R.check_exact(R.resample32(vol, R.tables_for(shape, size, "linear", True, "align_corners")), want, "align_corners")


def test_association_fault_changes_bits():
    """The fused kernel is held to the three passes bit for bit; a y-before-x association does not survive that."""
    shape, size = (12, 10, 14), (19, 23, 17)
    vol = R.random_volume(4, (4,) + shape)
    tables = [M.axis_table(n, m, "linear", True) for n, m in zip(shape, size)]
    want = R.resample32(vol, tables)
    with pytest.raises(AssertionError, match="differ"):
        R.check_exact(R.resample32(vol, tables, order=(1, 2, 0)), want, "y before x")


def test_tie_rule_fault_is_rejected():
    """One-hot labels under x2 up-sampling tie exactly (1/2 : 1/2 between two blobs): the lowest class must win."""
    shape, size = (8, 12, 16), (16, 24, 32)
    lab = R.blob_labels(2, 4, shape)
    tables = [M.axis_table(n, m, "linear", True) for n, m in zip(shape, size)]
    scores = R.resample64(R.one_hot(lab, 4), tables)
    top = np.sort(scores, axis=0)
    assert (top[-1] == top[-2]).any(), "the case holds no exact tie"
    assert R.check_argmax(R.argmax_first(scores), scores, 0.0, "first maximum") == 0.0
    with pytest.raises(AssertionError, match="decided voxels differ"):
        R.check_argmax(R.argmax_first(scores, fault="highest"), scores, 0.0, "last maximum")


def test_argmax_checker_asserts_the_excluded_share_first():
    scores = np.zeros((2, 2, 2, 2))
    scores[0] = 1e-9
    with pytest.raises(AssertionError, match="within the bound of a tie"):
        R.check_argmax(np.zeros((2, 2, 2), dtype=np.uint8), scores, 1e-6, "all within the bound")
    lab = R.blob_labels(3, 4, (12, 10, 14), special=(255, 9))
    tables = [M.axis_table(n, m, "linear", True) for n, m in zip((12, 10, 14), (19, 23, 17))]
    planes = R.one_hot(lab, 4)
    s64 = R.resample64(planes, tables)
    share = R.check_argmax(R.argmax_first(R.resample32(planes, tables)), s64, R.error_bound(planes, tables), "one-hot labels")
    print(f"one-hot labels (12, 10, 14) -> (19, 23, 17): {share:.2%} of the voxels within the bound of a tie")


def test_nan_outside_the_support_does_not_leak():
    vol = R.random_volume(6, (1, 6, 6, 8))
    tables = [M.axis_table(n, m, "linear", True) for n, m in zip((6, 6, 8), (6, 6, 16))]
    start, count = tables[2][0], tables[2][1]
    assert count[0] == 1 and start[0] == 0          # output 0 reads x = 0 alone
    vol[..., 1] = np.nan
    assert not np.isnan(R.resample32(vol, tables)[..., 0]).any() and not np.isnan(R.resample64(vol, tables)[..., 0]).any()
    assert np.isnan(R.resample32(vol, tables)[..., 1]).all()


def test_stores():
    x = np.array([-3.0, 0.5, 1.5, 2.5, 254.5, 255.5, 300.0, 17.49], dtype=np.float32)
    assert R.store_u8(x).tolist() == [0, 0, 2, 2, 254, 255, 255, 17]
    assert R.store_f16(np.float32(1.0 + 2.0 ** -11)) == np.float16(1.0)
