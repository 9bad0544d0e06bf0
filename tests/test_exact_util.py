"""CPU side of tests/test_gpu_exact.py: (1) the exact comparison sees the local faults that the suite's norm comparison
(gpu_util.assert_close: ||a - b||2 / ||b||2 <= tol) cannot, (2) the exactness conditions -- every reference element is a number
of the kernel's output type, every sum of |terms| stays below 2^24 -- hold for every small parametrised case of the GPU module
(the large shapes assert them inside their GPU test), (3) the inputs and checkers of
tests/test_gpu_head_backward.py: the references pass their own bounds, and each fault the checkers are there for is rejected."""
import pytest
import torch
import torch.nn.functional as F

import test_gpu_exact as X
import test_gpu_head_backward as H
from gpu_util import (ELU_Z, TOL, act_grad_from_out, assert_exact, assert_representable, check_gn_sums, elu_lattice, half_round, lattice,
                      rel, rnd, split_weight)

SMALL = 300000   # voxels x widest channel count up to which a case's fp64 reference is built in the CPU suite


def _small(n, cin, cout, shape, up=1):
    return n * shape[0] * shape[1] * shape[2] * up * max(cin, cout) <= SMALL


def test_lattice_is_seeded_and_sparse():
    a, b = lattice("t", 4, 8, 16, density=0.25), lattice("t", 4, 8, 16, density=0.25)
    assert torch.equal(a, b) and set(a.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert 0.15 < float((a != 0).float().mean()) < 0.35
    assert set(lattice("u", 64, values=(-1.5, 0.5), density=1.0).unique().tolist()) == {-1.5, 0.5}


def _ragged_case():
    c = X.case("conv", 2, 32, 32, (9, 11, 21))    # test_conv3d_mfma_fwd_dgrad_wgrad's ragged case: 133 056 outputs, tol 6e-3
    c.check_conditions("bf16")
    return c, c.ref()[0]["y"]


def test_one_wrong_voxel_passes_the_norm_and_fails_the_exact_comparison():
    c, y = _ragged_case()
    bad = y.clone()
    bad[1, 17, 8, 10, 20] += 1.0            # ONE element, one lattice step, at the far corner of the ragged volume
    assert rel(bad, y) <= 6e-3              # the existing test's tolerance for this shape: the fault is invisible
    bad[1, 17, 8, 10, 20] += 2.0 * float(y.std())   # ... and so is an error of two standard deviations
    assert rel(bad, y) <= 6e-3
    with pytest.raises(AssertionError) as e:
        assert_exact(bad, y, "y")
    msg = str(e.value)
    assert "1 of 133056" in msg and "(1, 17, 8, 10, 20)" in msg and "x%16 in [4]" in msg and "z%4 in [0]" in msg and "c%16 in [1]" in msg
    assert assert_exact(y.clone(), y, "y") == y.numel()
    assert assert_exact(-0.0 * torch.ones(3), torch.zeros(3), "signed zero") == 3
    with pytest.raises(AssertionError, match="1 NaN"):
        assert_exact(torch.tensor([1.0, float("nan")]), torch.tensor([1.0, 2.0]), "unwritten")


def test_a_missing_border_row_and_a_missing_tap_are_named():
    c, y = _ragged_case()
    # a whole border row of one channel not written (the last row of the last, ragged, brick in y): under test_conv3d_k3's bf16
    # tolerance for the norm
    bad = y.clone()
    bad[0, 5, 3, 10, :] = 0.0
    assert 0 < rel(bad, y) <= TOL["bf16"]
    with pytest.raises(AssertionError) as e:
        assert_exact(bad, y, "y")
    assert "y%8 in [2]" in str(e.value) and "z%4 in [3]" in str(e.value) and "c%32 in [5]" in str(e.value)
    # one tap (the corner tap 0, 0, 0) dropped at ONE output voxel, all input channels
    x, w = c.x.double(), c.w.double()
    tap = torch.einsum("nczyx,oc->nozyx", F.pad(x, (1, 1, 1, 1, 1, 1))[:, :, 0:9, 0:11, 0:21], w[:, :, 0, 0, 0])
    idx = tuple((tap != 0).nonzero()[-1].tolist())
    bad = y.clone()
    bad[idx] -= tap[idx]
    assert 0 < rel(bad, y) <= 6e-3
    with pytest.raises(AssertionError, match=r"1 of 133056 elements differ.*" + str(idx).replace("(", r"\(").replace(")", r"\)")):
        assert_exact(bad, y, "y")


def _conv_params():
    out = []
    for n, cin, cout, shape, bias in X.DIRECT_CASES:
        out += [("conv", n, cin, cout, shape, dict(bias=bias), m) for m in X.ALL_MODES]
    for n, cin, cout, shape in X.GENERAL_CASES:
        out += [("conv", n, cin, cout, shape, {}, m) for m in ("bf16", "fp16")]
    for n, cout, shape in X.FIRST_CASES:
        out += [("conv", n, 1, cout, shape, {}, m) for m in ("bf16", "fp16")]
    for n, cin, cout, shape in X.X3_CASES:
        out.append(("conv", n, cin, cout, shape, {}, "fp32"))
    for n, cin, cout, shape, _ in X.WGRAD_CASES:
        out += [("conv", n, cin, cout, shape, {}, m) for m in ("bf16", "fp16")]
    for n, cin, cout, shape in X.CONVT_MFMA_CASES:
        out += [("convt", n, cin, cout, shape, dict(bias=True, skip=True), m) for m in ("bf16", "fp16")]
    for n, cin, cout, shape in X.CONVT_DIRECT_CASES:
        out += [("convt", n, cin, cout, shape, dict(bias=True, skip=True), m) for m in X.ALL_MODES]
    for n, cin, cout, shape in X.CONVT_X3_CASES:
        out.append(("convt", n, cin, cout, shape, dict(bias=True, skip=True), "fp32"))
    return [p for p in out if _small(p[1], p[2], p[3], p[4], 8 if p[0] == "convt" else 1)]


@pytest.mark.parametrize("kind,n,cin,cout,shape,kw,mode", _conv_params())
def test_exactness_conditions_of_the_small_cases(kind, n, cin, cout, shape, kw, mode):
    X.case(kind, n, cin, cout, shape, **kw).check_conditions(mode)


@pytest.mark.parametrize("split", ["w", "x", "g"])
def test_exactness_conditions_of_the_split_bf16_cases(split):
    for kind, n, cin, cout, shape in (("conv", 2, 32, 32, (9, 11, 21)), ("conv", 2, 1, 32, (9, 11, 21)), ("convt", 2, 32, 16, (3, 5, 9))):
        c = X.case(kind, n, cin, cout, shape, split=split, big=256, bias=kind == "convt", skip=kind == "convt")
        c.check_conditions("fp32")
        t = {"w": c.w, "x": c.x, "g": c.g}[split]
        others = [v for k, v in (("w", c.w), ("x", c.x), ("g", c.g)) if k != split]
        assert bool((t.bfloat16().float() != t).any()) and all(bool((v.bfloat16().float() == v).all()) for v in others)


def test_exactness_conditions_of_the_split_weight_cases():
    """fp16x2: the weights need their low image (2049 is no fp16 number), yet every output is one -- the high parts telescope."""
    for kind, n, cin, cout, shape in (("conv", 2, 32, 32, (9, 11, 21)), ("conv", 1, 32, 64, (8, 8, 8)), ("convt", 2, 64, 32, (8, 16, 16))):
        c = X.case(kind, n, cin, cout, shape, split="wpair", big=2048, bias=kind == "convt", skip=kind == "convt")
        c.check_conditions("fp16x2")
        assert bool((c.w.half().float() != c.w).any())
        # without the low image the result is another one: the case depends on it
        hi = c.w.half().double()
        y_hi = (F.conv_transpose3d(c.x.double(), hi, c.b.double(), stride=2, padding=1, output_padding=1) + c.skip.double()
                if kind == "convt" else F.conv3d(c.x.double(), hi, None, padding=1))
        assert not torch.equal(y_hi, c.ref()[0]["y"])


def test_conditions_of_the_fused_sum_cases_that_fit_the_cpu_suite():
    n, cin, cout, shape, px, pw, _, _ = X.ACT_FWD_CASES[0]
    for dt in (torch.bfloat16, torch.float16):
        X.act_fwd_conditions(n, cin, cout, shape, px, pw, dt)
    X.act_fwd_conditions(2, 32, 32, (9, 11, 21), 0.25, 0.125, torch.float32)


# ------------------------------------------------------------------------------- the fused heads' backward: the checkers can fail
@pytest.mark.parametrize("mode,bits", [("bf16", 17), ("fp16", 23)])
def test_split_weights_are_reproduced_by_the_storage_type_split(mode, bits):
    """gpu_util.split_weight: fp32 numbers whose split hi = round(w), lo = round(w - hi) in the
    storage type -- the matrix-core heads' own -- gives them back exactly, with a low image that is not empty."""
    w0 = rnd("split" + mode, 21, 32, scale=0.3)
    w = split_weight(w0, mode)
    assert w.dtype == torch.float32
    hi = half_round(w, mode)
    lo = half_round(w - hi, mode)
    assert torch.equal((hi.double() + lo.double()), w.double()), "hi + lo does not reproduce the weight"
    assert torch.equal(hi + lo, w) and bool((lo != 0).any()) and bool((hi != w).any())
    # the two images together keep about `bits` bits of w0 (fp16: the low image of a weight below 1 is a subnormal, step 2^-24)
    assert bool(((w - w0).abs() <= w0.abs() * 2.0 ** (-bits + 1) + (2.0 ** -25 if mode == "fp16" else 0.0)).all())


def _fp32_results(c):
    """What ATen's fp32 evaluation gives for a case of part B: the stored dz (rounded to the mode's storage type), dW, db, and the
    GroupNorm sums of every activation of the case's block output, summed in fp32 from that stored dz (one row)."""
    dz = half_round(c.ref32.dz, c.mode)
    parts = {}
    for act in H.RUN_ACTS[c.zkind]:
        du = dz * act_grad_from_out(c.z, act)
        parts[act] = torch.stack((du.sum((2, 3, 4)), (du * c.gy).sum((2, 3, 4))), -1)[:, None].contiguous()
    return dz, c.ref32.dW, c.ref32.db, parts


@pytest.mark.parametrize("mode", H.B_MODES)
@pytest.mark.parametrize("n,shape", H.B_SHAPES)
@pytest.mark.parametrize("head", ["seg", "lm"])
def test_the_fp32_references_pass_the_head_backward_checkers(head, mode, n, shape):
    """Every case of part B of tests/test_gpu_head_backward.py: ATen's own fp32 results lie within the bounds the kernels are held
    to (eps_case = max(2^-15, 8 * r32), 2^-16 * sum |terms| for the sums), and the L1 cases meet their input condition."""
    for variant in H.variants_of(head):
        for zkind in H.Z_KINDS:
            c = H.head_case(head, mode, n, shape, variant, zkind)
            dz, dW, db, parts = _fp32_results(c)
            seen = H.check_case_gradients(c, dz, dW, db)
            assert all(seen[k] <= c.eps[k] and c.eps[k] >= 2.0 ** -15 and c.eps[k] >= 8 * c.r32[k] for k in seen), (seen, c.eps)
            for act, part in parts.items():
                assert part.shape == (n, 1, 32, 2)
                check_gn_sums(part, dz, c.z, c.gy, act, H.case_name(c))


MUTATION_CASES = [("seg", (5, "DICE", False, 2)), ("seg", (16, "CE", False, 3)), ("lm", (16, 2, "DICE", "L1", False, None)),
                  ("lm", (5, 3, "CE", "L2", False, 2))]


@pytest.mark.parametrize("mode", H.B_MODES)
@pytest.mark.parametrize("head,variant", MUTATION_CASES)
def test_the_head_backward_checkers_reject_the_faults_they_are_there_for(head, variant, mode):
    """Mutations of ATen's fp32 results at (2, (16, 16, 36)) -- 9216 voxels, 72 runs of 128, two workgroups per sample: each is
    refused, and the unmutated results pass."""
    n, shape = 2, (16, 16, 36)
    c = H.head_case(head, mode, n, shape, variant, "elu")
    dz, dW, db, parts = _fp32_results(c)
    name = H.case_name(c)
    H.check_case_gradients(c, dz, dW, db)
    check_gn_sums(parts[H.L.ACT_ELU], dz, c.z, c.gy, H.L.ACT_ELU, name)
    spatial = 16 * 16 * 36
    flat = lambda t: t.reshape(t.shape[0], t.shape[1], spatial)
    # the sums without the last 4 voxels of the last sample (one lane's last trip)
    du = flat(dz * act_grad_from_out(c.z, H.L.ACT_ELU)).clone()
    du[-1, :, -4:] = 0
    short = torch.stack((du.sum(2), (du * flat(c.gy)).sum(2)), -1)[:, None]
    with pytest.raises(AssertionError, match="GroupNorm sums outside"):
        check_gn_sums(short, dz, c.z, c.gy, H.L.ACT_ELU, name)
    # the sums with ELU's factor z + 1 replaced by ReLU's mask
    with pytest.raises(AssertionError, match="GroupNorm sums outside"):
        check_gn_sums(parts[H.L.ACT_ELU], dz, c.z, c.gy, H.L.ACT_RELU, name)
    du = dz * act_grad_from_out(c.z, H.L.ACT_RELU)
    masked = torch.stack((du.sum((2, 3, 4)), (du * c.gy).sum((2, 3, 4))), -1)[:, None]
    with pytest.raises(AssertionError, match="GroupNorm sums outside"):
        check_gn_sums(masked, dz, c.z, c.gy, H.L.ACT_ELU, name)
    # a row of NaN (not written)
    holed = torch.cat((parts[H.L.ACT_ELU], torch.full((n, 1, 32, 2), float("nan"))), 1)
    with pytest.raises(AssertionError, match="not written"):
        check_gn_sums(holed, dz, c.z, c.gy, H.L.ACT_ELU, name)
    # dz without the contribution of the last class in the voxels of the last run of a sample
    k = c.m - 1
    part_k = torch.einsum("c,nv->ncv", c.W[k], flat(c.ref32.dl.float())[:, k])
    bad = flat(c.ref32.dz.float()).clone()
    bad[:, :, -128:] -= part_k[:, :, -128:]
    with pytest.raises(AssertionError, match=r"dz: \d+ of 589824 elements outside"):
        H.check_case_gradients(c, half_round(bad.reshape(dz.shape), mode), dW, db)
    # dW with the row of one class taken from its neighbour
    bad = dW.clone()
    bad[k] = dW[k - 1]
    with pytest.raises(AssertionError, match="dW: 32 of"):
        H.check_case_gradients(c, dz, bad, db)
    # a gradient stored with bf16's 8 bits where the mode keeps fp16's 11
    if mode == "fp16":
        with pytest.raises(AssertionError, match="dz: "):
            H.check_case_gradients(c, c.ref32.dz.bfloat16().float(), dW, db)
    # one element never written
    bad = dz.clone()
    bad[1, 31, 15, 15, 35] = float("nan")
    with pytest.raises(AssertionError, match="1 of 589824 elements are NaN"):
        H.check_case_gradients(c, bad, dW, db)


def test_the_elu_lattice_is_dyadic_seeded_and_keeps_one_maximum_per_window():
    a, b = elu_lattice("t", 2, 4, 4, 6, 8), elu_lattice("t", 2, 4, 4, 6, 8)
    assert torch.equal(a, b) and set(a.unique().tolist()) == set(ELU_Z)
    for dt in (torch.bfloat16, torch.float16):
        assert_representable(a, dt, "ELU lattice")
    assert float(a.min()) > -1 and set((4 * (a + 1)[a <= 0]).unique().tolist()) == {1.0, 2.0, 3.0, 4.0}
    m = elu_lattice("t", 2, 4, 4, 6, 8, window_max=True)
    assert set(m.unique().tolist()) == set(ELU_Z)
    win = m.reshape(2, 4, 2, 2, 3, 2, 4, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(2, 4, 2, 3, 4, 8)
    top = win.max(-1, keepdim=True).values
    assert bool(((win == top).sum(-1) == 1).all()) and set(top.unique().tolist()) == set(ELU_Z[1:])


def test_conditions_of_the_elu_cases_of_the_groupnorm_sum_tests():
    """Conditions 1 to 3 of the ELU branch (du = dx * (z + 1) in steps of 1/4) for the shapes the four tests use; the inputs
    functions assert them (the large ConvTranspose3d and convolution cases do so inside their GPU test)."""
    for n, c, shape, pool, with_add in X.POOL_GN_CASES:
        for dt in (torch.bfloat16, torch.float16, torch.float32):
            refs = X.pool_gn_inputs(n, c, shape, pool, with_add, dt)[3]
            out, dx, du = refs[X.L.ACT_ELU]
            assert bool((du != dx).any()) and bool((du * 4 == torch.round(du * 4)).all())   # (a negative maximum scales its gradient)
    for n, cin, cout, shape in X.HEAD_GN_CASES:
        for dt in (torch.bfloat16, torch.float16, torch.float32):
            gz, du = X.head_gn_inputs(n, cin, cout, shape, dt)[4][X.L.ACT_ELU]
            assert set(gz.unique().tolist()) == set(ELU_Z) and bool((du != torch.round(du)).any())
    for n, cin, cout, shape, _ in X.CONVT_GN_CASES:
        if _small(n, cin, cout, shape, 8):
            for mode in X.MODES16:
                gz, du = X.convt_gn_inputs(n, cin, cout, shape, mode)[3][X.L.ACT_ELU]
                assert bool((du != torch.round(du)).any())
    for mode, n, cin, cout, shape, _, _ in X.DGRAD_CASES[:2]:
        _, _, variants = X.dgrad_conditions((n, cin, cout, shape), X.DT[mode])
        for with_add in (False, True):
            dx, du = variants[(with_add, X.L.ACT_ELU)]
            relu = variants[(with_add, X.L.ACT_RELU)][1]
            assert bool((du != dx).any()) and bool((du != 0).any()) and not torch.equal(du, relu)
