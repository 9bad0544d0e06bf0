"""CPU side of tests/test_gpu_exact.py: (1) the exact comparison sees the local faults that the suite's norm comparison
(gpu_util.assert_close: ||a - b||2 / ||b||2 <= tol) cannot, (2) the exactness conditions -- every reference element is a number
of the kernel's output type, every sum of |terms| stays below 2^24 -- hold for every small parametrised case of the GPU module
(the large shapes assert them inside their GPU test)."""
import pytest
import torch
import torch.nn.functional as F

import test_gpu_exact as X
from gpu_util import TOL, assert_exact, lattice, rel

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
