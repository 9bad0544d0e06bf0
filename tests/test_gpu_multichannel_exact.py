"""Exact-arithmetic tests of the multi-channel first layer (2-4 fp32 input channels, 16-bit storage): conv_first_mfma_kernel<2..4, .>
with its fused GroupNorm pair sums and wgrad_first_mfma_kernel<2..4, ., .>, against ATen (fp64, CPU) with EQUALITY in every element.

Same method as tests/test_gpu_exact.py (lattice inputs: the exact result is a number of the output type and every fp32 partial
sum is exact in any order), same first-layer shapes -- the brick is still 4 x 8 x 16.  Because two correct kernels give the same
bits, which kernel ran is taken from the library's own queries (mednet_conv3d_cm_supported, mednet_conv3d_fused_stats_chunks,
mednet_conv3d_wgrad_cm_plan), never from outputs.
"""
import contextlib
import ctypes

import pytest
import torch
import torch.nn.functional as F

import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import nn as hnn

from gpu_util import DEV, assert_exact, assert_representable, assert_sums_exact, lattice
from test_gpu_exact import DT, case, check_sum_conditions, compare_pair_sums, report

pytestmark = pytest.mark.gpu
CL = torch.channels_last_3d
MODES = ["bf16", "fp16", "fp16x2"]
SHAPES = [(2, 32, (9, 11, 21)),    # ragged in every dimension, two samples
          (1, 64, (5, 6, 7)),      # smaller than a brick, two channel blocks
          (2, 16, (9, 11, 21)),    # half a block
          (1, 48, (4, 8, 16))]     # exactly one brick, 1 1/2 blocks
Case = type(case("conv", 1, 2, 48, (4, 8, 16)))   # (base class of the local cases with an fp32 input below; the case is used anyway)
_DEFAULTS = dict(conv_cm=1, wgrad_c1_mfma=1, assume_cus=0, conv_c1_persist=1)


@contextlib.contextmanager
def options(**kw):
    """A/B knobs of the library for the duration of a block (test_gpu_exact.options knows no conv_cm)."""
    lib = L.lib()
    try:
        for k, v in kw.items():
            assert lib.mednet_set_option(k.encode(), int(v)) == 0
        yield
    finally:
        for k in kw:
            lib.mednet_set_option(k.encode(), _DEFAULTS[k])


def algo_of(mode):
    return L.ALGO_AUTO | (L.ALGO_SPLITW_BIT if mode == "fp16x2" else 0)


def wgrad_plan(n, shape, cin, cout, dcode, gn=0):
    out = (ctypes.c_int * 4)()
    rc = L.lib().mednet_conv3d_wgrad_cm_plan(n, *shape, cin, cout, dcode, gn, ctypes.addressof(out))
    assert rc == 0, L.lib().mednet_last_error().decode()
    return list(out)   # [workgroups, NB, workgroups per CU, LDS bytes]


def run_first_layer(x, w, g, mode, cout, rows):
    """x (fp32, any memory format) through hnn.Conv3d with fused statistics, backward with g -> (y, partial, dw)."""
    n, cin = x.shape[:2]
    with mednet_hip.precision(mode):
        conv = hnn.Conv3d(cin, cout, 3, bias=False).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(w)
        y, partial = conv.forward_with_stats(x)
        assert partial is not None and tuple(partial.shape) == (n, rows, cout, 2), "no fused statistics"
        y.backward(g.to(DEV).to(DT[mode]))
        torch.cuda.synchronize()
    return y.detach(), partial.detach(), conv.weight.grad.detach()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin", [2, 3, 4])
@pytest.mark.parametrize("n,cout,shape", SHAPES)
def test_multichannel_first_layer_kernels(mode, cin, n, cout, shape):
    """y, the fused pair sums and dw (matrix-core form and, with wgrad_c1_mfma = 0, the direct form), the input given planar and
    channels_last_3d with identical bits."""
    c = case("conv", n, cin, cout, shape)
    c.check_conditions(mode)
    ref = c.ref()[0]
    lib, dt = L.lib(), DT[mode]
    assert lib.mednet_conv3d_cm_supported(cin, cout, 3, L.F32, L.dt_of(dt), algo_of(mode)) == 1
    rows = lib.mednet_conv3d_fused_stats_chunks(n, *shape, cin, cout, 3, L.F32, L.dt_of(dt), algo_of(mode))
    assert rows > 0, "the multi-channel first-layer kernel does not take this call"
    check_sum_conditions(ref["y"], f"{c}")
    total = 0
    for c1 in (1, 0):
        with options(wgrad_c1_mfma=c1):
            assert lib.mednet_conv3d_wgrad_cm_gn_supported(cin, cout, L.F32, L.dt_of(dt)) == c1   # (the plain dispatch's predicate)
            if c1 and cout == 64:
                assert wgrad_plan(n, shape, cin, cout, L.dt_of(dt))[1] == 2, "two channel blocks per workgroup expected"
            got = {}
            for layout in ("planar", "channels_last"):
                xg = c.x.to(DEV)
                if layout == "channels_last":
                    xg = xg.contiguous(memory_format=CL)
                    assert not xg.is_contiguous()
                y, partial, dw = run_first_layer(xg, c.w, c.g, mode, cout, rows)
                total += assert_exact(y, ref["y"], f"{layout} {mode} {c}: y") + assert_exact(dw, ref["dw"], f"{layout} wgrad mfma={c1} {c}: dw")
                total += compare_pair_sums(partial, ref["y"], f"{layout} {mode} {c}")
                got[layout] = (y, partial, dw)
            for a, b, name in zip(got["planar"], got["channels_last"], ("y", "partial", "dw")):
                assert torch.equal(a, b), f"{c} {mode}: {name} differs between the two input layouts"
    report("a", f"{c} {mode}", "conv_first_mfma_kernel+wgrad_cm(mfma,direct)", total)


# ------------------------------------------------------------------------------------------------ persistent walk
WALK_SHAPE = (3, 32, (40, 72, 80))   # 1350 (brick, channel block) items: more than 4 workgroups per CU


@pytest.mark.parametrize("mode,cin", [("bf16", 2), ("bf16", 4), ("fp16x2", 4)])
def test_multichannel_persistent_walk(mode, cin):
    """More items than workgroups: a workgroup walks several bricks, the sample changes inside its list, a skipped sample
    yields zero rows."""
    n, cout, shape = WALK_SHAPE
    c = case("conv", n, cin, cout, shape)
    c.check_conditions(mode)
    ref = c.ref()[0]
    lib, dt = L.lib(), DT[mode]
    rows = lib.mednet_conv3d_fused_stats_chunks(n, *shape, cin, cout, 3, L.F32, L.dt_of(dt), algo_of(mode))
    ncb = (cout + 31) // 32
    grid = rows // 4 * ncb                      # (rows = 4 * workgroups / channel blocks)
    per_sample = ((shape[0] + 3) // 4) * ((shape[1] + 7) // 8) * ((shape[2] + 15) // 16) * ncb
    items = n * per_sample
    assert items > grid > 0, f"{items} items on {grid} workgroups: no walk"
    jumps = [b for b in range(grid) if b + grid < items and (b + grid) // per_sample - b // per_sample == 2]
    assert jumps, "no workgroup skips a sample"
    check_sum_conditions(ref["y"], f"{c}")
    y, partial, dw = run_first_layer(c.x.to(DEV), c.w, c.g, mode, cout, rows)
    total = assert_exact(y, ref["y"], f"walk {mode} {c}: y") + assert_exact(dw, ref["dw"], f"walk {mode} {c}: dw")
    total += compare_pair_sums(partial, ref["y"], f"walk {mode} {c}")
    b = jumps[0]
    mid = b // per_sample + 1
    assert float(partial[mid, 4 * (b // ncb):4 * (b // ncb) + 4].abs().max()) == 0.0, "rows of a skipped sample are not zero"
    report("a", f"{c} {mode}", f"conv_first_mfma_kernel walk {items} items / {grid} workgroups", total)


# ------------------------------------------------------------------------------------------------ low parts of the input
class Fp32InputCase(Case):
    """A first layer whose fp32 input is NOT a number of the storage type (Case insists on that when cin != 1): only the listed
    outputs are held to the conditions."""

    def check_outputs(self, mode, keys):
        ref, mag = self.ref()
        for k in keys:
            assert_representable(ref[k], torch.float32 if k == "dw" else DT[mode], f"{self} {mode} {k}")
            assert_sums_exact(mag[k], f"{self} {mode} {k}")
            assert float(ref[k].abs().max()) > 0
        assert_representable(self.g, DT[mode], f"{self} {mode} gradient")
        assert bool((self.x.to(DT[mode]).float() != self.x).any()), "the input has no low part"


class PairedLowCase(Fp32InputCase):
    """Channels 0 and 1 carry (big + 1) m and big m with weights s and -s (cin = 4: channels 2 and 3 the same with their own m, s;
    cin = 3: channel 2 plain lattice values): the high parts cancel and every output is the small integer sum s m, which only the
    low image of x produces."""

    def __init__(self, n, cin, cout, shape, big):
        Case.__init__(self, "conv", n, cin, cout, shape, big=big)
        tag = f"mcpl{n}_{cin}_{cout}_{shape}{big}"
        x, w = self.x.clone(), self.w.clone()
        for p in range(cin // 2):
            m = lattice(f"{tag}m{p}", n, *shape, density=0.5)
            s = lattice(f"{tag}s{p}", cout, 3, 3, 3, values=(-1, 1), density=0.5)
            x[:, 2 * p], x[:, 2 * p + 1] = (big + 1) * m, big * m
            w[:, 2 * p], w[:, 2 * p + 1] = s, -s
        self.x, self.w = x.contiguous(), w.contiguous()
        self._ref = None


_LOW = {}


def low_case(kind, *args):
    if (kind, args) not in _LOW:
        if kind == "dw":
            n, cin, cout, shape, big = args
            _LOW[(kind, args)] = Fp32InputCase("conv", n, cin, cout, shape, split="x", big=big)
        else:
            _LOW[(kind, args)] = PairedLowCase(*args)
    return _LOW[(kind, args)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin", [2, 3, 4])
def test_low_part_of_the_input_in_the_weight_gradient(mode, cin):
    """x = +-(big + 1): dw = (big + 1) k is exact in fp32 and off by whole steps if the low image of x is dropped."""
    n, cout, shape = 2, 32, (9, 11, 21)
    big = 256 if mode == "bf16" else 2048
    c = low_case("dw", n, cin, cout, shape, big)
    c.check_outputs(mode, ("dw",))
    ref = c.ref()[0]
    rows = L.lib().mednet_conv3d_fused_stats_chunks(n, *shape, cin, cout, 3, L.F32, L.dt_of(DT[mode]), algo_of(mode))
    assert rows > 0 and L.lib().mednet_conv3d_wgrad_cm_gn_supported(cin, cout, L.F32, L.dt_of(DT[mode])) == 1
    _, _, dw = run_first_layer(c.x.to(DEV), c.w, c.g, mode, cout, rows)
    report("b", f"{c} {mode}", "wgrad_first_mfma_kernel low part of x", assert_exact(dw, ref["dw"], f"low part {mode} {c}: dw"))
    hi_only = F.conv3d(c.x.to(DT[mode]).double(), c.w.double(), padding=1)   # (the case depends on the low part)
    assert not torch.equal(hi_only, ref["y"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin", [2, 3, 4])
def test_low_part_of_the_input_in_the_forward(mode, cin):
    """16-bit output: paired channels whose high parts cancel; a dropped low image gives 0 where the reference has sum s m."""
    n, cout, shape = 2, 32, (9, 11, 21)
    big = 256 if mode == "bf16" else 2048
    c = low_case("y", n, cin, cout, shape, big)
    c.check_outputs(mode, ("y", "dw"))
    ref = c.ref()[0]
    hi_only = F.conv3d(c.x.to(DT[mode]).double(), c.w.double(), padding=1)
    assert int((hi_only != ref["y"]).sum()) > ref["y"].numel() // 4, "the case does not exercise the low image"
    check_sum_conditions(ref["y"], f"{c}")
    rows = L.lib().mednet_conv3d_fused_stats_chunks(n, *shape, cin, cout, 3, L.F32, L.dt_of(DT[mode]), algo_of(mode))
    assert rows > 0
    y, partial, dw = run_first_layer(c.x.to(DEV), c.w, c.g, mode, cout, rows)
    total = assert_exact(y, ref["y"], f"low part {mode} {c}: y") + assert_exact(dw, ref["dw"], f"low part {mode} {c}: dw")
    total += compare_pair_sums(partial, ref["y"], f"low part {mode} {c}")
    report("b", f"{c} {mode}", "conv_first_mfma_kernel low part of x", total)


# ------------------------------------------------------------------------------------------------ the dispatch
def test_statistics_are_fused_and_the_mfma_request_succeeds():
    """What fails without the path: fused rows for a 4-channel first layer, and set_conv_algo('mfma') taking it."""
    n, shape = 2, (9, 11, 21)
    lib = L.lib()
    assert lib.mednet_conv3d_fused_stats_chunks(n, *shape, 4, 32, 3, L.F32, L.BF16, L.ALGO_AUTO) > 0
    c = case("conv", n, 4, 32, shape)
    mednet_hip.set_conv_algo("mfma")
    try:
        with mednet_hip.precision("bf16"):
            conv = hnn.Conv3d(4, 32, 3, bias=False).to(DEV)
            with torch.no_grad():
                conv.weight.copy_(c.w)
            y = conv(c.x.to(DEV))
            torch.cuda.synchronize()
    finally:
        mednet_hip.set_conv_algo("auto")
    assert_exact(y, c.ref()[0]["y"], "mfma request: y")


def test_option_conv_cm_0_restores_the_dispatch():
    n, shape = 2, (9, 11, 21)
    lib = L.lib()
    with options(conv_cm=0):
        assert lib.mednet_conv3d_cm_supported(4, 32, 3, L.F32, L.BF16, L.ALGO_AUTO) == 0
        assert lib.mednet_conv3d_fused_stats_chunks(n, *shape, 4, 32, 3, L.F32, L.BF16, L.ALGO_AUTO) == 0
        assert lib.mednet_conv3d_wgrad_cm_gn_supported(4, 32, L.F32, L.BF16) == 0
        c = case("conv", n, 4, 32, shape)
        with mednet_hip.precision("bf16"):     # the direct kernels on a channels-last copy, as before
            conv = hnn.Conv3d(4, 32, 3, bias=False).to(DEV)
            with torch.no_grad():
                conv.weight.copy_(c.w)
            y, partial = conv.forward_with_stats(c.x.to(DEV))
            assert partial is None
            y.backward(c.g.to(DEV).bfloat16())
            assert_exact(y, c.ref()[0]["y"], "conv_cm=0: y")
            assert_exact(conv.weight.grad, c.ref()[0]["dw"], "conv_cm=0: dw")
        mednet_hip.set_conv_algo("mfma")
        try:
            with mednet_hip.precision("bf16"), pytest.raises(RuntimeError):
                hnn.Conv3d(4, 32, 3, bias=False).to(DEV)(c.x.to(DEV))
        finally:
            mednet_hip.set_conv_algo("auto")
    assert lib.mednet_conv3d_cm_supported(4, 32, 3, L.F32, L.BF16, L.ALGO_AUTO) == 1
