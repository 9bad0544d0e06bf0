"""Exact-arithmetic tests: every conv-family kernel against ATen (fp64, CPU) with EQUALITY in every element.

The inputs lie on a lattice (small integers, or a big power of two plus a small integer where a split operand is wanted) such
that the mathematically exact result is a number of the kernel's output type and every fp32 partial sum is exact in any
summation order.  Accumulation order, MFMA blocking, split products and the output rounding then drop out: a correct kernel
and the reference agree in every element, and one wrong voxel, tap, channel or row fails the test (gpu_util.assert_exact says
where).  Every test first asserts, on the reference alone and for ALL elements, the conditions that make equality the right
expectation (gpu_util.assert_representable / assert_sums_exact); tests/test_exact_util.py asserts them on the CPU for the
small cases.  Because two correct kernels give the same bits here, "the outputs differ" cannot show which kernel ran: the
library's own plan queries do.

Every test prints one line `[exact] item=<a..g> ...  elements=<count>` per comparison group (pytest -s / -rP shows them).
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import nn as hnn
from mednet_hip import ops

from gpu_util import DEV, FP32_EXACT, assert_exact, assert_representable, assert_sums_exact, elu_lattice, lattice

pytestmark = pytest.mark.gpu
CL = torch.channels_last_3d
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp16x2": torch.float16, "fp32": torch.float32}
MODES16 = ["bf16", "fp16"]
ALL_MODES = ["bf16", "fp16", "fp16x2", "fp32"]

_DEFAULTS = dict(conv32=1, conv2b=1, conv2b_min_fill=80, conv2b_min_cin=64, conv2b_split=1, wgrad_v4=1, x3=1, x3_stats=1,
                 wgrad_c1_mfma=1, convt_dgrad32=1, conv32_gnb=1, assume_cus=0)


@contextlib.contextmanager
def options(**kw):
    """A/B knobs of the library for the duration of a block; restored to the defaults afterwards."""
    lib = L.lib()
    try:
        for k, v in kw.items():
            assert lib.mednet_set_option(k.encode(), int(v)) == 0
        yield
    finally:
        for k in kw:
            lib.mednet_set_option(k.encode(), _DEFAULTS[k])


def _cus():
    """Plan queries without a device assume the MI355X's 256 CUs (as tests/test_plan_audit.py does)."""
    return options() if torch.cuda.is_available() else options(assume_cus=256)


def stats_plan(n, shape, cin, cout, dcode, gnb=0, stride=1, split=False):
    """mednet_conv3d_stats_plan: [kind, grid, items, channel blocks, bricks, bricks per sample, accumulate, rows, ...]."""
    out = (ctypes.c_int * 13)()
    with _cus():
        rc = L.lib().mednet_conv3d_stats_plan(n, *shape, cin, cout, dcode, int(gnb) | (2 if split else 0), stride, ctypes.addressof(out))
    assert rc == 0, L.lib().mednet_last_error().decode()
    return list(out)


def wgrad_plan(n, shape, cin, cout, dcode, wgs=0):
    out = (ctypes.c_int * 10)()
    with _cus():
        rc = L.lib().mednet_conv3d_wgrad_plan(n, *shape, cin, cout, dcode, wgs, ctypes.addressof(out))
    assert rc == 0, L.lib().mednet_last_error().decode()
    return list(out)


def dcode_of(mode):
    return L.dt_of(DT[mode])


def report(item, what, kernel, elements):
    print(f"[exact] item={item} {what} kernel={kernel} elements={elements}")


# ------------------------------------------------------------------------------------------------ cases and references
class Case:
    """Lattice inputs of one convolution layer and its fp64 reference (forward, data / weight / bias gradient), with the sums of
    the absolute values of every output's terms (the same convolution of |x| with |w|)."""

    def __init__(self, kind, n, cin, cout, shape, bias=False, split=None, big=256, skip=False):
        self.kind, self.n, self.cin, self.cout, self.shape, self.split, self.big = kind, n, cin, cout, tuple(shape), split, big
        tag = f"ex{kind}{n}_{cin}_{cout}_{shape}{split}{big}"
        cmax = max(cin, cout)
        # densities: the output's standard deviation stays near 28 lattice steps at the widest layers (bf16 holds every integer up
        # to 256): var = 27 * C * p_x * E[x^2] * p_w with x in {+-1, +-2} (E = 2.5), w in {+-1}
        px = 0.5 if cmax <= 8 else 0.25
        pw = min(px, 800.0 / (27 * cmax * 2.5 * px))
        self.oshape = tuple(2 * s for s in shape) if kind == "convt" else tuple(shape)
        wshape = (cin, cout, 3, 3, 3) if kind == "convt" else (cout, cin, 3, 3, 3)
        x = lattice(tag + "x", n, cin, *shape, density=px)
        w = lattice(tag + "w", *wshape, values=(-1, 1), density=pw)
        g = lattice(tag + "g", n, cout, *self.oshape, density=px)
        if split == "w":     # exactly ONE operand of every product needs its low part: big + 1 = hi + lo in the 16-bit type
            w = w * (big + 1)
        elif split == "x":
            x = torch.sign(x) * (big + 1) * (x.abs() > 0)
        elif split == "g":
            g = torch.sign(g) * (big + 1) * (g.abs() > 0)
        elif split == "wpair":
            # 16-bit OUTPUT with split weights: an output k * (big + 1) would not be a 16-bit number.  Channels come in equal pairs
            # (x[2j+1] = x[2j], g[2j+1] = g[2j]) and every 2 x 2 weight block is s * [[big + 1, -big], [-big, big + 1]]: the high
            # parts telescope, every output is the small sum of s * x, and a dropped or misplaced low image is off by whole steps
            assert cin % 2 == 0 and cout % 2 == 0
            x = x[:, 0::2].repeat_interleave(2, dim=1)
            g = g[:, 0::2].repeat_interleave(2, dim=1)
            s = w[0::2, 0::2].clone()      # one sign per (channel pair, channel pair, tap)
            blk = torch.tensor([[big + 1.0, -float(big)], [-float(big), big + 1.0]])
            w = (s[:, None, :, None] * blk[None, :, None, :, None, None, None]).reshape(wshape)
        self.x, self.w, self.g = x.contiguous(), w.contiguous(), g.contiguous()
        self.b = lattice(tag + "b", cout, values=(-3, -1, 1, 2), density=0.75) if bias else None
        self.skip = lattice(tag + "s", n, cout, *self.oshape, density=0.5) if skip else None
        self._ref = None

    def _run(self, x, w, b, g, skip):
        x, w = x.double().requires_grad_(True), w.double().requires_grad_(True)
        b = None if b is None else b.double().requires_grad_(True)
        if self.kind == "convt":
            y = F.conv_transpose3d(x, w, b, stride=2, padding=1, output_padding=1)
        else:
            y = F.conv3d(x, w, b, padding=1)
        if skip is not None:
            y = y + skip.double()
        y.backward(g.double())
        return dict(y=y.detach(), dx=x.grad, dw=w.grad, db=None if b is None else b.grad)

    def ref(self):
        """(reference, sums of |terms|), computed once per case and shared by all storage modes and kernel options."""
        if self._ref is None:
            a = lambda t: None if t is None else t.abs()
            self._ref = (self._run(self.x, self.w, self.b, self.g, self.skip),
                         self._run(a(self.x), a(self.w), a(self.b), a(self.g), a(self.skip)))
        return self._ref

    def check_conditions(self, mode):
        """The conditions under which equality is the right expectation -- on the reference alone, every element."""
        ref, mag = self.ref()
        dt = DT[mode]
        for k in ("y", "dx", "dw", "db"):
            if ref[k] is None:
                continue
            assert_representable(ref[k], torch.float32 if k in ("dw", "db") else dt, f"{self} {mode} {k}")
            assert_sums_exact(mag[k], f"{self} {mode} {k}")
        for t in (self.x, self.g, self.skip):   # the operands are numbers of the storage type
            if t is not None and not (t is self.x and self.cin == 1):
                assert_representable(t, dt, f"{self} {mode} operand")
        assert float(ref["y"].abs().max()) > 0 and float(ref["dx"].abs().max()) > 0 and float(ref["dw"].abs().max()) > 0
        if self.kind == "convt":
            self.check_parity_classes()

    def check_parity_classes(self):
        """All eight output-parity classes and the far faces (2d-1, 2h-1, 2w-1: where output_padding matters) carry values."""
        y = self.ref()[0]["y"]
        for pz in (0, 1):
            for py in (0, 1):
                for px in (0, 1):
                    assert float(y[:, :, pz::2, py::2, px::2].abs().max()) > 0, f"{self}: parity class {(pz, py, px)} is all zero"
        assert float(y[:, :, -1].abs().max()) > 0 and float(y[:, :, :, -1].abs().max()) > 0 and float(y[..., -1].abs().max()) > 0

    def __repr__(self):
        return f"{self.kind}(n={self.n}, {self.cin}->{self.cout}, {self.shape}, split={self.split})"


_CASES = {}


def case(kind, n, cin, cout, shape, **kw):
    key = (kind, n, cin, cout, tuple(shape), tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = Case(kind, n, cin, cout, shape, **kw)
    return _CASES[key]


def run_layer(c, mode, algo="auto", put=None):
    """The case through hnn.Conv3d / hnn.ConvTranspose3d in a storage mode -> {y, dx, dw, db} on the CPU.  `put`: where every
    device tensor the layer is given goes first, as put(tensor, cl); cl: an activation, which the library wants channels-last, not
    a parameter (tests/test_gpu_footprint.py: fence.put)."""
    dt = DT[mode]
    put = put or (lambda t, cl: t)
    mednet_hip.set_conv_algo(algo)
    try:
        with mednet_hip.precision(mode):
            if c.kind == "convt":
                mod = hnn.ConvTranspose3d(c.cin, c.cout).to(DEV)
            else:
                mod = hnn.Conv3d(c.cin, c.cout, 3, bias=c.b is not None).to(DEV)
            with torch.no_grad():
                mod.weight.copy_(c.w)
                if c.b is not None:
                    mod.bias.copy_(c.b)
                elif c.kind == "convt":
                    mod.bias.zero_()
                for p in mod.parameters():
                    p.data = put(p.data, False)
            # (the network input of a first layer arrives in fp32; every other tensor in the mode's storage type, so that the
            #  matrix-core kernels take the call)
            xg = put(c.x.to(DEV) if c.cin == 1 else c.x.to(DEV).to(dt), True).requires_grad_(True)
            if c.kind == "convt":
                y = mod(xg, skip=None if c.skip is None else put(c.skip.to(DEV).to(dt), True))
            else:
                y = mod(xg)
            assert y.dtype == dt and tuple(y.shape) == (c.n, c.cout, *c.oshape)
            y.backward(put(c.g.to(DEV).to(dt), True))
            torch.cuda.synchronize()
            has_b = c.b is not None
            return dict(y=y.detach().cpu(), dx=xg.grad.cpu(), dw=mod.weight.grad.cpu(), db=mod.bias.grad.cpu() if has_b else None)
    finally:
        mednet_hip.set_conv_algo("auto")


def compare_layer(c, got, what):
    ref = c.ref()[0]
    total = 0
    for k in ("y", "dx", "dw", "db"):
        if ref[k] is not None:
            total += assert_exact(got[k], ref[k], f"{what}: {k}")
    return total


# ------------------------------------------------------------------------------------------------ (a) 3x3x3 convolution
DIRECT_CASES = [(2, 1, 8, (6, 10, 12), False), (1, 8, 16, (5, 7, 9), True), (1, 32, 32, (8, 8, 16), False),
                (2, 3, 5, (4, 6, 7), True), (1, 16, 64, (4, 4, 4), False), (1, 64, 32, (3, 5, 8), False)]   # test_conv3d_k3's
GENERAL_CASES = [(1, 32, 32, (4, 8, 16)), (2, 32, 32, (9, 11, 21)), (1, 64, 32, (8, 16, 16)), (1, 32, 64, (6, 8, 32)),
                 (1, 128, 128, (5, 6, 7)), (1, 256, 256, (4, 4, 4)), (2, 64, 64, (16, 16, 16)), (2, 16, 32, (9, 11, 21)),
                 (1, 32, 16, (8, 8, 16)), (1, 16, 16, (5, 9, 17)), (1, 48, 80, (4, 8, 16)), (2, 64, 96, (10, 10, 6)),
                 (1, 32, 64, (12, 20, 24)), (2, 32, 32, (7, 9, 40))]      # test_conv3d_mfma_fwd_dgrad_wgrad's 14 shapes
FIRST_CASES = [(2, 32, (9, 11, 21)), (1, 64, (5, 6, 7)), (2, 16, (9, 11, 21)), (1, 48, (4, 8, 16)), (3, 32, (40, 72, 80))]
CONV32_CASES = [(1, (66, 60, 50)),     # 544 bricks, ragged in z, y and x
                (3, (32, 64, 48)),     # 576 bricks, the sample changes inside a workgroup's brick list
                (2, (32, 60, 62))]     # 512 bricks, 2 z-layers of bricks per XCD
CONV2B_CASES = [(1, 64, 64, (30, 60, 50)),     # 256 brick slots x 1 block pair, ragged in z, y and x
                (2, 32, 128, (24, 40, 48)),    # 180 bricks x 2 pairs: padding items, two rounds, the sample changes
                (1, 128, 128, (36, 40, 48))]   # 135 bricks (not a multiple of 8), 8 K chunks
X3_CASES = [(2, 32, 32, (9, 11, 21)), (1, 48, 16, (5, 6, 7)), (3, 16, 48, (4, 9, 17)), (1, 64, 96, (8, 8, 16))]
WGRAD_CASES = [(1, 32, 32, (8, 8, 16), 0), (2, 32, 32, (9, 11, 21), 0), (1, 32, 32, (40, 16, 32), 0), (1, 16, 48, (12, 9, 17), 0),
               (2, 64, 32, (24, 24, 48), 24), (1, 128, 96, (8, 8, 16), 0)]


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("n,cin,cout,shape,bias", DIRECT_CASES)
def test_direct_kernels(mode, n, cin, cout, shape, bias):
    """The direct (VALU) forward / data-gradient / weight-gradient / bias-gradient kernels (set_conv_algo('direct')), Cin = 1,
    Cin = 3, Cout = 5 and odd sizes included."""
    c = case("conv", n, cin, cout, shape, bias=bias)
    c.check_conditions(mode)
    assert L.lib().mednet_conv3d_act_supported(n, *shape, cin, cout, L.ALGO_DIRECT) == 0
    assert L.lib().mednet_conv3d_fused_stats_chunks(n, *shape, cin, cout, 3, dcode_of(mode), dcode_of(mode), L.ALGO_DIRECT) == 0
    report("a", f"{c} {mode}", "direct", compare_layer(c, run_layer(c, mode, "direct"), f"direct {mode} {c}"))


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp16x2"])
@pytest.mark.parametrize("n,cin,cout,shape", GENERAL_CASES)
def test_general_matrix_core_kernel(mode, n, cin, cout, shape):
    """conv_mfma_kernel<1> / <3> (options conv32 = 0, conv2b = 0), the root of the suite's bit-identity chain, and the weight
    gradient the shape selects: one brick, ragged everywhere, volumes smaller than a brick, half-full channel blocks, 8-wide
    bricks."""
    c = case("conv", n, cin, cout, shape)
    c.check_conditions(mode)
    with options(conv32=0, conv2b=0, conv2b_split=0):   # (conv2b_split: the two-block kernel's (high, low) form takes fp16x2 calls)
        for a, b in ((cin, cout), (cout, cin)):   # forward and data-gradient form
            assert stats_plan(n, shape, a, b, dcode_of(mode), split=mode == "fp16x2")[0] in (2, 3)
        assert L.lib().mednet_conv3d_act_supported(n, *shape, cin, cout, L.ALGO_MFMA) == 1
        got = run_layer(c, mode, "mfma")
    kind = wgrad_plan(n, shape, cin, cout, dcode_of(mode))[0]
    report("a", f"{c} {mode}", f"conv_mfma_kernel+wgrad_mfma{kind}", compare_layer(c, got, f"general {mode} {c}"))


@pytest.mark.parametrize("mode", MODES16)
@pytest.mark.parametrize("n,shape", CONV32_CASES)
def test_conv32_specialisation(mode, n, shape):
    """conv32_mfma_kernel (32 -> 32 channels on >= 512 bricks), forward and data gradient."""
    cin = cout = 32
    c = case("conv", n, cin, cout, shape)
    c.check_conditions(mode)
    assert stats_plan(n, shape, cin, cout, dcode_of(mode))[0] == 4
    report("a", f"{c} {mode}", "conv32_mfma_kernel", compare_layer(c, run_layer(c, mode, "mfma"), f"conv32 {mode} {c}"))


@pytest.mark.parametrize("mode", MODES16)
@pytest.mark.parametrize("n,cin,cout,shape", CONV2B_CASES)
def test_two_block_kernel(mode, n, cin, cout, shape):
    """conv2b_mfma_kernel (two channel blocks per wave): the forward, and the data gradient where the layer's Cin comes in pairs
    of blocks."""
    c = case("conv", n, cin, cout, shape)
    c.check_conditions(mode)
    with options(conv2b_min_fill=0, conv2b_min_cin=16):
        assert stats_plan(n, shape, cin, cout, dcode_of(mode))[0] in (5, 6)
        if cin % 64 == 0:
            assert stats_plan(n, shape, cout, cin, dcode_of(mode))[0] in (5, 6)    # the data gradient: the kernel's Cin / Cout swapped
        got = run_layer(c, mode, "mfma")
    report("a", f"{c} {mode}", "conv2b_mfma_kernel", compare_layer(c, got, f"conv2b {mode} {c}"))


@pytest.mark.parametrize("mode", MODES16)
@pytest.mark.parametrize("v4", [1, 0])
@pytest.mark.parametrize("n,cin,cout,shape,wgs", WGRAD_CASES)
def test_weight_gradient_kernels(mode, v4, n, cin, cout, shape, wgs):
    """wgrad_mfma4_kernel (z-columns, where d >= 8, h >= 8, w >= 16) and wgrad_mfma2_kernel (bricks; option wgrad_v4 = 0) through
    the C ABI with a workspace and an output filled with NaN patterns, a workgroup count that does not divide the items
    included."""
    c = case("conv", n, cin, cout, shape)
    c.check_conditions(mode)
    lib, dt, code = L.lib(), DT[mode], dcode_of(mode)
    d, h, w = shape
    xg = c.x.to(DEV).to(dt).contiguous(memory_format=CL)
    dyg = c.g.to(DEV).to(dt).contiguous(memory_format=CL)
    with options(wgrad_v4=v4):
        want = 4 if (v4 and d >= 8 and h >= 8 and w >= 16) else 2
        assert wgrad_plan(n, shape, cin, cout, code, wgs)[0] == want
        assert lib.mednet_conv3d_wgrad_coresident(n, d, h, w, cin, cout, 3, code, code, L.ALGO_MFMA) == int(want == 4)
        ws = torch.empty(lib.mednet_conv3d_wgrad_ws_bytes(n, d, h, w, cin, cout, 3, wgs), dtype=torch.uint8, device=DEV)
        ws.fill_(0xFF)
        dw = torch.full((cout, cin, 3, 3, 3), float("nan"), device=DEV)
        db = torch.full((cout,), float("nan"), device=DEV)
        L.check(lib.mednet_conv3d_wgrad(xg.data_ptr(), dyg.data_ptr(), dw.data_ptr(), db.data_ptr(), n, d, h, w, cin, cout, 3, code,
                                        L.NDHWC, code, L.NDHWC, L.ALGO_MFMA, wgs, ws.data_ptr(), ws.numel(), L.stream()), "conv3d_wgrad")
        torch.cuda.synchronize()
    ref = c.ref()[0]
    db_ref = c.g.double().sum((0, 2, 3, 4))
    assert_sums_exact(c.g.abs().double().sum((0, 2, 3, 4)), "db")
    total = assert_exact(dw, ref["dw"], f"wgrad_mfma{want} {mode} {c} wgs={wgs}: dw") + assert_exact(db, db_ref, "db")
    report("a", f"{c} {mode} wgs={wgs}", f"wgrad_mfma{want}_kernel", total)


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp16x2"])
@pytest.mark.parametrize("n,cout,shape", FIRST_CASES)
def test_first_layer_kernels(mode, n, cout, shape):
    """Cin = 1: conv_first_mfma_kernel<1, .> (persistent walk for the big volume) with its fused GroupNorm sums, and the weight
    gradient in its matrix-core form (wgrad_first_mfma_kernel<1, ., .>, wgrad_c1_mfma = 1) and its VALU form."""
    c = case("conv", n, 1, cout, shape)
    c.check_conditions(mode)
    ref = c.ref()[0]
    lib, dt = L.lib(), DT[mode]
    rows = lib.mednet_conv3d_fused_stats_chunks(n, *shape, 1, cout, 3, L.F32, L.dt_of(dt), L.ALGO_AUTO | (L.ALGO_SPLITW_BIT if mode == "fp16x2" else 0))
    assert rows > 0, "the first-layer matrix-core kernel does not take this call"
    check_sum_conditions(ref["y"], f"{c}")
    total = 0
    for c1 in (1, 0):
        with options(wgrad_c1_mfma=c1), mednet_hip.precision(mode):
            conv = hnn.Conv3d(1, cout, 3, bias=False).to(DEV)
            with torch.no_grad():
                conv.weight.copy_(c.w)
            poison = torch.full((n, rows, cout, 2), float("nan"), device=DEV)   # (the partial buffer comes from torch.empty)
            del poison
            y, partial = conv.forward_with_stats(c.x.to(DEV))
            assert partial is not None and tuple(partial.shape) == (n, rows, cout, 2)
            y.backward(c.g.to(DEV).to(dt))
            torch.cuda.synchronize()
            total += assert_exact(y, ref["y"], f"first layer {mode} {c}: y") + assert_exact(conv.weight.grad, ref["dw"], f"wgrad_c1 mfma={c1}: dw")
            total += compare_pair_sums(partial, ref["y"], f"first layer {mode} {c}")
    report("a", f"{c} {mode}", "conv_first_mfma_kernel<1>+wgrad_c1(mfma,valu)", total)


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp16x2"])
@pytest.mark.parametrize("n,cout,shape", FIRST_CASES[:4])
def test_first_layer_kernels_16bit_input(mode, n, cout, shape):
    """Cin = 1 with the input already in the 16-bit storage type (the one-channel output of a GroupNorm in the 'gcr' orders): the
    16-bit-load form of conv_first_mfma_kernel<1, .> with its fused GroupNorm sums, and of the weight gradient in its matrix-core
    and its VALU form.  The lattice input converts exactly, so the fp64 reference is the one of the fp32-input test."""
    c = case("conv", n, 1, cout, shape)
    c.check_conditions(mode)
    ref = c.ref()[0]
    lib, dt = L.lib(), DT[mode]
    x16 = c.x.to(dt)
    assert bool((x16.double() == c.x.double()).all()), "the lattice input is not a number of the storage type"
    rows = lib.mednet_conv3d_fused_stats_chunks(n, *shape, 1, cout, 3, L.dt_of(dt), L.dt_of(dt), L.ALGO_AUTO | (L.ALGO_SPLITW_BIT if mode == "fp16x2" else 0))
    assert rows > 0, "the first-layer matrix-core kernel does not take 16-bit input"
    check_sum_conditions(ref["y"], f"{c}")
    total = 0
    for c1 in (1, 0):
        with options(wgrad_c1_mfma=c1), mednet_hip.precision(mode):
            conv = hnn.Conv3d(1, cout, 3, bias=False).to(DEV)
            with torch.no_grad():
                conv.weight.copy_(c.w)
            y, partial = conv.forward_with_stats(x16.to(DEV))
            assert partial is not None and tuple(partial.shape) == (n, rows, cout, 2)
            y.backward(c.g.to(DEV).to(dt))
            torch.cuda.synchronize()
            total += assert_exact(y, ref["y"], f"first layer, 16-bit x, {mode} {c}: y")
            total += assert_exact(conv.weight.grad, ref["dw"], f"wgrad_c1 mfma={c1}, 16-bit x: dw")
            total += compare_pair_sums(partial, ref["y"], f"first layer, 16-bit x, {mode} {c}")
    report("a", f"{c} {mode} x16", "conv_first_mfma_kernel<1>+wgrad_c1(mfma,valu)", total)


def x3_family_takes(n, cin, cout, shape):
    """Does the split-bf16 family take this fp32-storage layer?  (First layer: its fused-sum rows; otherwise the query of the
    data gradient with a summed second gradient, which only the split-bf16 kernel offers in fp32 storage.)"""
    lib = L.lib()
    if cin == 1:
        return lib.mednet_conv3d_fused_stats_chunks(n, *shape, cin, cout, 3, L.F32, L.F32, L.ALGO_AUTO) > 0
    return lib.mednet_conv3d_dgrad_add_supported(n, *shape, cin, cout, L.ALGO_AUTO, L.F32) == 1


@pytest.mark.parametrize("x3", [1, 0])
@pytest.mark.parametrize("n,cin,cout,shape", X3_CASES + [(2, 1, 32, (9, 11, 21)), (1, 1, 32, (8, 16, 32))])
def test_fp32_mode_families(x3, n, cin, cout, shape):
    """fp32 storage: the split-bf16 family (x3 = 1: conv_x3 / wgrad_x3 / conv_c1_x3 / wgrad_c1_x3) and the exact-product family
    (x3 = 0: v_mfma_f32_32x32x2_f32)."""
    c = case("conv", n, cin, cout, shape)
    c.check_conditions("fp32")
    with options(x3=x3):
        assert x3_family_takes(n, cin, cout, shape) == bool(x3), "option x3 selects no other family"
        got = run_layer(c, "fp32")
    report("a", f"{c} fp32", "split-bf16" if x3 else "fp32-mfma", compare_layer(c, got, f"fp32 x3={x3} {c}"))


# ------------------------------------------------------------------------------------------------ (b) low parts
@pytest.mark.parametrize("split", ["w", "x", "g"])
@pytest.mark.parametrize("kind,n,cin,cout,shape", [("conv", 2, 32, 32, (9, 11, 21)), ("conv", 1, 64, 96, (8, 8, 16)),
                                                   ("conv", 2, 1, 32, (9, 11, 21)), ("convt", 2, 32, 16, (3, 5, 9)),
                                                   ("convt", 1, 64, 32, (4, 4, 8))])
def test_split_bf16_low_parts(split, kind, n, cin, cout, shape):
    """fp32 mode, x3 = 1: hi*hi + hi*lo + lo*hi (lo*lo is dropped by design, conv_x3_mfma.hip:4-6), so exactly ONE operand of
    every product carries a low part: weights 257 = 256 + 1 (bf16 keeps 8 bits), or such activations, or such gradients, against
    small integers.  A kernel that drops or misplaces a low-image product is off by whole lattice steps."""
    c = case(kind, n, cin, cout, shape, split=split, big=256, bias=kind == "convt", skip=kind == "convt")
    c.check_conditions("fp32")
    for t in {"w": (c.w,), "x": (c.x,), "g": (c.g,)}[split]:
        assert bool((t.bfloat16().float() != t).any()), "the operand has no low part"
    if kind == "conv":
        assert x3_family_takes(n, cin, cout, shape)
    report("b", f"{c} fp32", "split-bf16", compare_layer(c, run_layer(c, "fp32"), f"split-bf16 low parts ({split}) {c}"))


@pytest.mark.parametrize("kind,n,cin,cout,shape,want,opts", [
    ("conv", 2, 32, 32, (9, 11, 21), (2, 3), dict(conv2b_split=0)),   # general kernel: the low image as further K chunks
    ("conv", 2, 32, 32, (9, 11, 21), (5, 6), {}),      # conv2b's (high, low) form, ragged bricks
    ("conv", 1, 32, 64, (8, 8, 8), (2, 3), {}),        # narrow volume: conv_mfma_kernel<3>
    ("conv", 1, 32, 32, (32, 64, 64), (5, 6), {}),     # conv2b's (high, low) form in place of the 32 -> 32 specialisation
    ("convt", 2, 64, 32, (8, 16, 16), None, {})])
def test_split_weight_low_images(kind, n, cin, cout, shape, want, opts):
    """fp16x2: the WEIGHTS' low images (FwdArgs::lo_delta).  Outputs are stored in fp16, where k * 2049 is no number: channels come
    in equal pairs and the weights in blocks s * [[2049, -2048], [-2048, 2049]] (Case, 'wpair'), so that the high parts cancel
    and every output is a small integer that only the low image produces."""
    c = case(kind, n, cin, cout, shape, split="wpair", big=2048, bias=kind == "convt", skip=kind == "convt")
    c.check_conditions("fp16x2")
    assert bool((c.w.half().float() != c.w).any())
    with options(**opts):
        if want is not None:
            assert stats_plan(n, shape, cin, cout, L.F16, split=True)[0] in want
        got = run_layer(c, "fp16x2", "mfma")
    report("b", f"{c} fp16x2", f"plan kinds {want}", compare_layer(c, got, f"split weights {c}"))
    # the same layer WITHOUT the low images must miss: the case really depends on them
    plain = run_layer(c, "fp16", "mfma")
    assert not torch.equal(plain["y"].double(), c.ref()[0]["y"]), "the case does not exercise the low image"


# ------------------------------------------------------------------------------------------------ (c) ConvTranspose3d
def _fuzz_cases_ct(k, seed):   # (test_conv_transpose_mfma_dgrad_wgrad's)
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(1, 3)), int(rng.choice([32, 64, 96])), int(rng.choice([32, 64])),
             tuple(int(v) for v in rng.integers(1, 21, 3))) for _ in range(k)]


CONVT_MFMA_CASES = [(1, 64, 32, (2, 4, 16)), (2, 64, 32, (3, 5, 9)), (1, 256, 128, (4, 4, 4)), (1, 32, 32, (5, 9, 17))] + _fuzz_cases_ct(10, 77)
CONVT_DIRECT_CASES = [(2, 16, 8, (3, 5, 4)), (1, 8, 8, (4, 4, 4)), (1, 64, 32, (2, 3, 5))]
CONVT_X3_CASES = [(2, 32, 16, (3, 5, 9)), (1, 64, 32, (4, 4, 8)), (1, 16, 48, (5, 3, 17)), (2, 128, 64, (3, 6, 16))]
CONVT32_CASE = (2, 64, 32, (16, 32, 32))     # 2 x 8 x 8 x 2 = 256 bricks of 2 x 4 x 16: convt_dgrad32_mfma_kernel (plan kind 7)


@pytest.mark.parametrize("mode", MODES16)
@pytest.mark.parametrize("n,cin,cout,shape", CONVT_MFMA_CASES)
def test_conv_transpose_matrix_core(mode, n, cin, cout, shape):
    c = case("convt", n, cin, cout, shape, bias=True, skip=True)
    c.check_conditions(mode)
    assert L.lib().mednet_convt3d_dgrad_gn_rows(n, *shape, cin, cout, dcode_of(mode), L.ALGO_MFMA) > 0   # matrix-core data gradient
    report("c", f"{c} {mode}", "convt mfma", compare_layer(c, run_layer(c, mode, "mfma"), f"convT mfma {mode} {c}"))


@pytest.mark.parametrize("mode", MODES16)
def test_conv_transpose_dgrad32(mode):
    n, cin, cout, shape = CONVT32_CASE
    c = case("convt", n, cin, cout, shape, bias=True, skip=True)
    c.check_conditions(mode)
    assert stats_plan(n, shape, cin, cout, dcode_of(mode), gnb=1, stride=2)[0] == 7
    report("c", f"{c} {mode}", "convt_dgrad32_mfma_kernel", compare_layer(c, run_layer(c, mode, "mfma"), f"convt_dgrad32 {mode} {c}"))


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("n,cin,cout,shape", CONVT_DIRECT_CASES)
def test_conv_transpose_direct(mode, n, cin, cout, shape):
    c = case("convt", n, cin, cout, shape, bias=True, skip=True)
    c.check_conditions(mode)
    report("c", f"{c} {mode}", "convt direct", compare_layer(c, run_layer(c, mode, "direct"), f"convT direct {mode} {c}"))


@pytest.mark.parametrize("x3", [1, 0])
@pytest.mark.parametrize("n,cin,cout,shape", CONVT_X3_CASES)
def test_conv_transpose_fp32_mode(x3, n, cin, cout, shape):
    c = case("convt", n, cin, cout, shape, bias=True, skip=True)
    c.check_conditions("fp32")
    with options(x3=x3):
        got = run_layer(c, "fp32")
    report("c", f"{c} fp32", "split-bf16" if x3 else "fp32-mfma", compare_layer(c, got, f"convT fp32 x3={x3} {c}"))


# ------------------------------------------------------------------------------------------------ fused sums
def check_sum_conditions(y, what, other=None, unit=1.0):
    """Condition 3: per sample and channel the totals of |y| and y^2 (resp. |du| and |du * gn_y|) over the WHOLE sample, counted
    in lattice steps of `unit` (1/4 for the ELU cases: du = dx * (z + 1)), stay below 2^24 (per channel PAIR: twice the worst
    channel bounds it) -- the accumulate-mode kernels keep one fp32 sum per wave over many bricks.  Every term must lie on the
    lattice."""
    y = y.double()
    second = y * y if other is None else (y * other.double()).abs()
    for t, name in ((y.abs(), "sum |.|"), (second, "sum of the second moment")):
        assert bool((t / unit == torch.round(t / unit)).all()), f"{what}: {name} has terms off the lattice of step {unit}"
        m = 2.0 * float(t.sum((2, 3, 4)).max()) / unit
        assert m < FP32_EXACT, f"{what}: {name} reaches {m:.4g} lattice steps >= 2^24 per channel pair"


def compare_pair_sums(partial, y, what, per_channel=False):
    """The returned rows, summed in fp64, EQUAL sum y and sum y^2 of the reference per sample and channel pair (entry 2j = channels
    2j and 2j + 1 together, entry 2j + 1 = 0), or per channel where the kernel keeps single channels."""
    p = partial.detach().double().cpu()
    assert not bool(torch.isnan(p).any()), f"{what}: {int(torch.isnan(p).any(-1).any(-1).sum())} rows of the partial buffer hold a NaN (not written)"
    tot = p.sum(1)                               # [n][c][2]
    y = y.double()
    n, ch = y.shape[:2]
    s, q = y.sum((2, 3, 4)), (y * y).sum((2, 3, 4))
    want = torch.stack((s, q), -1)
    if not per_channel:
        want = want.reshape(n, ch // 2, 2, 2).sum(2)
        odd = tot[:, 1::2]
        if bool((odd != 0).any()):    # a kernel that keeps single channels: fold to pairs, the totals must still be the pair totals
            tot = tot.reshape(n, ch // 2, 2, 2).sum(2)
        else:
            tot = tot[:, 0::2]
    return assert_exact(tot, want, f"{what}: fused sums {{sum y, sum y^2}}")


def _sparse_inputs(tag, n, cin, cout, shape, px, pw):
    x = lattice(tag + "x", n, cin, *shape, values=(-1, 1), density=px)
    w = lattice(tag + "w", cout, cin, 3, 3, 3, values=(-1, 1), density=pw)
    return x, w


_FWD_REF = {}


def fwd_ref(n, cin, cout, shape, px, pw):
    key = (n, cin, cout, shape, px, pw)
    if key not in _FWD_REF:
        x, w = _sparse_inputs(f"exs{key}", n, cin, cout, shape, px, pw)
        _FWD_REF[key] = (x, w, F.conv3d(x.double(), w.double(), None, padding=1), F.conv3d(x.abs().double(), w.abs().double(), None, padding=1))
    return _FWD_REF[key]


# (n, cin, cout, shape, p_x, p_w, plan kinds wanted, options): sparser inputs for the big shapes, so that the sums of a whole
# sample stay below 2^24
ACT_FWD_CASES = [
    (2, 32, 32, (20, 24, 36), 0.25, 0.125, (2,), {}),                      # ragged bricks: one row per wave and brick
    (1, 16, 128, (32, 64, 64), 0.125, 0.125, (3,), {}),                    # general kernel, accumulate mode, four channel blocks
    (3, 32, 32, (32, 64, 48), 0.125, 0.0625, (4,), {}),                    # conv32: 576 bricks, the sample changes inside a workgroup's list
    (1, 64, 64, (30, 60, 50), 0.125, 0.0625, (5, 6), dict(conv2b_min_fill=0)),   # conv2b, ragged
    (2, 32, 128, (24, 40, 48), 0.125, 0.125, (5, 6), dict(conv2b_min_fill=0, conv2b_min_cin=16)),   # padding items, the sample changes
]


def act_fwd_conditions(n, cin, cout, shape, px, pw, dt):
    x, w, yr, ay = fwd_ref(n, cin, cout, shape, px, pw)
    assert_sums_exact(ay, "act_fwd y")
    for ref in (yr, F.relu(yr)):
        assert_representable(ref, dt, "act_fwd y")
        check_sum_conditions(ref, f"act_fwd {n, cin, cout, shape}")
    assert float(yr.abs().max()) > 0
    return x, w, yr


@pytest.mark.parametrize("mode", MODES16)
@pytest.mark.parametrize("n,cin,cout,shape,px,pw,kinds,opts", ACT_FWD_CASES)
def test_fused_forward_epilogues(mode, n, cin, cout, shape, px, pw, kinds, opts):
    """mednet_conv3d_act_fwd, activation none and ReLU (exact on the lattice), with gn_partial pre-filled with NaN: y exact, and
    the rows add up EXACTLY to sum y and sum y^2 of the reference per sample and channel pair, odd entries zero -- in
    row-per-brick mode and in accumulate mode, for the general kernel, conv32 and conv2b."""
    dt, dcode = DT[mode], dcode_of(mode)
    x, w, yr = act_fwd_conditions(n, cin, cout, shape, px, pw, dt)
    lib = L.lib()
    d, h, wd = shape
    xg = x.to(DEV).to(dt).contiguous(memory_format=CL)
    total = 0
    with options(**opts):
        plan = stats_plan(n, shape, cin, cout, dcode)
        assert plan[0] in kinds, plan
        with mednet_hip.precision(mode):
            pk = ops.pack_conv_weight(w.to(DEV), 3, False)
        rows = lib.mednet_conv3d_fused_stats_chunks(n, d, h, wd, cin, cout, 3, dcode, dcode, L.ALGO_MFMA)
        assert rows > 0
        for act, fn in ((L.ACT_NONE, lambda t: t), (L.ACT_RELU, F.relu)):
            for stats in (True, False):
                y = torch.full((n, cout, *shape), float("nan"), device=DEV).to(dt).contiguous(memory_format=CL)
                part = torch.full((n, rows, cout, 2), float("nan"), device=DEV) if stats else None
                L.check(lib.mednet_conv3d_act_fwd(xg.data_ptr(), pk.data_ptr(), y.data_ptr(), n, d, h, wd, cin, cout, act, L.ALGO_MFMA,
                                                  L.ptr(part), dcode, L.stream()), "act_fwd")
                torch.cuda.synchronize()
                total += assert_exact(y, fn(yr), f"act_fwd act={act} stats={stats} {mode}: y")
                if stats:
                    p = part.cpu()
                    assert not bool(torch.isnan(p).any()) and bool((p[:, :, 1::2] == 0).all()), "odd entries of the pair format must be zero"
                    total += compare_pair_sums(part, fn(yr), f"act_fwd act={act} {mode} kind {plan[0]}")
    report("d", f"{n, cin, cout, shape} {mode}", f"plan kind {plan[0]} accumulate={plan[6]}", total)


@pytest.mark.parametrize("n,c,shape,px,pw", [(2, 32, (30, 60, 50), 0.125, 0.0625), (1, 32, (32, 64, 64), 0.125, 0.0625), (2, 64, (16, 32, 64), 0.125, 0.0625),
                                          (2, 256, (16, 32, 32), 0.0625, 0.03125)])
def test_fused_forward_sums_in_the_fp32_mode(n, c, shape, px, pw):
    """The split-bf16 forward kernel's GroupNorm sums (option x3_stats; one row per wave of a group of bricks, per CHANNEL)."""
    x, w, yr = act_fwd_conditions(n, c, c, shape, px, pw, torch.float32)
    assert L.lib().mednet_conv3d_fused_stats_chunks(n, *shape, c, c, 3, L.F32, L.F32, L.ALGO_AUTO) > 0
    with mednet_hip.precision("fp32"):
        conv = hnn.Conv3d(c, c, 3, bias=False).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(w)
        y, partial = conv.forward_with_stats(x.to(DEV))
        torch.cuda.synchronize()
    assert partial is not None
    total = assert_exact(y, yr, "x3 forward: y") + compare_pair_sums(partial, yr, "x3_stats", per_channel=True)
    report("d", f"{n, c, c, shape} fp32", "conv_x3 + x3_stats", total)


# ------------------------------------------------------------------------------------------------ (e) data-gradient epilogues
GN_ACTS = (L.ACT_NONE, L.ACT_RELU, L.ACT_ELU)   # (LeakyReLU's 0.1 is no dyadic number: tests/test_gpu_head_backward.py covers it)
SUM_UNIT = {L.ACT_NONE: 1.0, L.ACT_RELU: 1.0, L.ACT_ELU: 0.25}   # the lattice step of du


def gn_reference(dx, gn_z, act):
    """du = dx * act'(.) for the per-channel {sum du, sum du * gn_y}; act in (none, ReLU, ELU).  gn_z is the block OUTPUT for the
    kernels that read it (act_grad_n: ELU' = z + 1 for z <= 0, ATen's elu_backward(is_result=true)); for none and ReLU a
    pre-activation serves as well (only its sign is used)."""
    if act == L.ACT_NONE:
        return dx
    if act == L.ACT_RELU:
        return dx * (gn_z > 0)
    assert act == L.ACT_ELU and float(gn_z.min()) > -1
    return dx * torch.where(gn_z > 0, torch.ones_like(gn_z), gn_z + 1)


def compare_channel_sums(partial, du, gy, what):
    p = partial.detach().double().cpu()
    assert not bool(torch.isnan(p).any()), f"{what}: a row of the partial buffer was not written"
    want = torch.stack((du.sum((2, 3, 4)), (du * gy).sum((2, 3, 4))), -1)
    return assert_exact(p.sum(1), want, f"{what}: {{sum du, sum du * gn_y}}")


DGRAD_CASES = [
    ("bf16", 2, 32, 32, (9, 11, 21), (2, 3), dict(conv32=0)),                         # general kernel, ragged
    ("fp16", 1, 32, 64, (6, 8, 32), (2, 3), dict(conv32=0, conv2b=0)),                # two channel blocks of dy
    ("bf16", 2, 32, 32, (32, 60, 62), (4,), {}),                                      # conv32 (conv32_gnb)
    ("fp16", 2, 32, 32, (32, 60, 62), (4,), {}),
    ("bf16", 1, 64, 64, (30, 60, 50), (5, 6), dict(conv2b_min_fill=0)),               # conv2b
    ("fp16", 1, 64, 64, (30, 60, 50), (5, 6), dict(conv2b_min_fill=0)),
    ("fp32", 2, 32, 32, (30, 60, 50), None, {}),                                      # the fp32 mode's split-bf16 data gradient, ragged
    ("fp32", 2, 64, 64, (15, 30, 62), None, {}),
]


def dgrad_inputs(n, cin, cout, shape):
    """dy (Cout channels), weights, add and gn_y (Cin channels) sparse enough that the sums of a whole sample stay exact."""
    big = n * shape[0] * shape[1] * shape[2] > 20000
    tag = f"exd{n, cin, cout, shape}"
    dy = lattice(tag + "g", n, cout, *shape, values=(-1, 1), density=0.125 if big else 0.25)
    w = lattice(tag + "w", cout, cin, 3, 3, 3, values=(-1, 1), density=0.0625 if big else 0.125)
    add = lattice(tag + "a", n, cin, *shape, values=(-2, -1, 1, 2), density=0.25)
    gy = lattice(tag + "y", n, cin, *shape, values=(-4, -2, 2, 4), density=0.5)
    # ca in {0.5, 1, 2} (and their negatives) times an even gn_y is an integer, cb a half-integer: ca * gn_y + cb is never zero and
    # its sign is exact
    ca = lattice(tag + "ca", n, cin, values=(-2, -1, -0.5, 0.5, 1, 2), density=1.0)
    cb = lattice(tag + "cb", n, cin, values=(-1.5, -0.5, 0.5, 1.5), density=1.0)
    # ELU: this kernel has no block output to read, it forms act' = exp(ca * gn_y + cb) from the recomputed PRE-activation
    # (act_grad_pre_n), which is a dyadic number only at its ends.  ca * gn_y in {0, +-128, +-256, +-512} and cb in {0, +-256}: every
    # pre-activation is a multiple of 128, so act' is exactly 1 (positive, or exp(0)) or exactly 0 (exp(-128) = 2.6e-56 is below
    # the smallest fp32 number).  ReLU' differs from it at 0 and LeakyReLU' below 0.
    ea = lattice(tag + "ea", n, cin, values=(-128, -64, 64, 128), density=1.0)
    eb = lattice(tag + "eb", n, cin, values=(-256, 0, 0, 256), density=1.0)
    xr = torch.zeros(n, cin, *shape, dtype=torch.float64, requires_grad=True)
    F.conv3d(xr, w.double(), None, padding=1).backward(dy.double())
    xa = torch.zeros(n, cin, *shape, dtype=torch.float64, requires_grad=True)
    F.conv3d(xa, w.abs().double(), None, padding=1).backward(dy.abs().double())
    return dict(dy=dy, w=w, add=add, gy=gy, coef=torch.stack((ca, cb), -1).contiguous(), coef_elu=torch.stack((ea, eb), -1).contiguous(),
                dx=xr.grad, mag=xa.grad + add.abs().double())


_DGRAD = {}


def dgrad_conditions(key, dt):
    """Inputs, and per (add, activation) variant the reference (dx, du), after the exactness conditions have been asserted."""
    if key not in _DGRAD:
        _DGRAD[key] = dgrad_inputs(*key)
    t = _DGRAD[key]
    gy64 = t["gy"].double()
    affine = lambda coef: coef[..., 0].double()[:, :, None, None, None] * gy64 + coef[..., 1].double()[:, :, None, None, None]
    pre, pre_elu = affine(t["coef"]), affine(t["coef_elu"])
    assert float(pre.abs().min()) > 0
    assert bool((pre_elu % 128 == 0).all()) and bool((pre_elu == 0).any()) and bool((pre_elu < 0).any()) and bool((pre_elu > 0).any())
    elu_grad = (pre_elu >= 0).double()      # exp(0) = 1; exp(u) = 0 in fp32 for u <= -128
    assert_sums_exact(t["mag"], "dgrad dx")
    variants = {}
    for with_add in (False, True):
        dx = t["dx"] + (t["add"].double() if with_add else 0)
        assert_representable(dx, dt, "dx")
        for act in GN_ACTS:
            du = dx * elu_grad if act == L.ACT_ELU else gn_reference(dx, pre, act)
            check_sum_conditions(du, f"dgrad_gn {key}", other=gy64)
            variants[(with_add, act)] = (dx, du)
    return t, gy64, variants


@pytest.mark.parametrize("mode,n,cin,cout,shape,kinds,opts", DGRAD_CASES)
def test_fused_data_gradient_epilogues(mode, n, cin, cout, shape, kinds, opts):
    """mednet_conv3d_dgrad_add (dx = dgrad(dy) + add) and mednet_conv3d_dgrad_gn with gn_act none / ReLU / ELU, add present / absent
    and power-of-two gn_coef: dx exact and the summed rows EQUAL {sum du, sum du * gn_y} computed in fp64 from the reference dx.
    ELU has coefficients of its own (dgrad_inputs): this kernel's ELU' is exp(pre-activation), pinned where it is exactly 0 or 1."""
    key = (n, cin, cout, shape)
    dt, dcode = DT[mode], dcode_of(mode)
    t, gy64, variants = dgrad_conditions(key, dt)
    lib = L.lib()
    d, h, wd = shape
    algo = L.ALGO_AUTO if mode == "fp32" else L.ALGO_MFMA
    dev = lambda a: a.to(DEV).to(dt).contiguous(memory_format=CL)
    dyg, addg, gyg, coef, coef_elu = dev(t["dy"]), dev(t["add"]), dev(t["gy"]), t["coef"].to(DEV), t["coef_elu"].to(DEV)
    total = 0
    with options(**opts):
        if kinds is not None:
            plan = stats_plan(n, shape, cout, cin, dcode, gnb=1)     # (the kernel's Cin / Cout = the layer's Cout / Cin)
            assert plan[0] in kinds, plan
        assert lib.mednet_conv3d_dgrad_add_supported(n, d, h, wd, cin, cout, algo, dcode) == 1
        rows = lib.mednet_conv3d_dgrad_gn_rows_dt(n, d, h, wd, cin, cout, algo, dcode)
        assert rows > 0
        with mednet_hip.precision(mode):
            pk = ops.pack_conv_weight(t["w"].to(DEV), 3, False)
        dx = torch.full((n, cin, *shape), float("nan"), device=DEV).to(dt).contiguous(memory_format=CL)
        L.check(lib.mednet_conv3d_dgrad_add(dyg.data_ptr(), pk.data_ptr(), addg.data_ptr(), dx.data_ptr(), n, d, h, wd, cin, cout, algo,
                                            dcode, L.stream()), "dgrad_add")
        torch.cuda.synchronize()
        total += assert_exact(dx, variants[(True, 0)][0], f"dgrad_add {mode} {key}: dx")
        for (with_add, act), (dx_ref, du_ref) in variants.items():
            dx = torch.full((n, cin, *shape), float("nan"), device=DEV).to(dt).contiguous(memory_format=CL)
            part = torch.full((n, rows, cin, 2), float("nan"), device=DEV)
            L.check(lib.mednet_conv3d_dgrad_gn(dyg.data_ptr(), pk.data_ptr(), addg.data_ptr() if with_add else None, dx.data_ptr(),
                                               gyg.data_ptr(), (coef_elu if act == L.ACT_ELU else coef).data_ptr(), act, part.data_ptr(), n, d, h, wd, cin, cout, algo,
                                               dcode, L.stream()), "dgrad_gn")
            torch.cuda.synchronize()
            what = f"dgrad_gn {mode} {key} add={with_add} act={act}"
            total += assert_exact(dx, dx_ref, what + ": dx") + compare_channel_sums(part, du_ref, gy64, what)
    report("e", f"{key} {mode}", f"plan kinds {kinds}", total)


POOL_GN_CASES = [(2, 32, (8, 12, 16), "max", True), (1, 64, (6, 4, 10), "avg", True), (2, 16, (4, 8, 6), "max", False)]


def pool_gn_inputs(n, c, shape, pool, with_add, dt):
    """-> dy of the pooling, add, gn_y and per activation (block output, reference dx, du), the exactness conditions asserted.
    none / ReLU: a block output with ties inside the windows; ELU: the dyadic lattice gpu_util.ELU_Z with a unique maximum per
    window (the pooling backward selects by this tensor, so dx is another one)."""
    d, h, w = shape
    tag = f"expg{n, c, shape, pool}"
    dyp = lattice(tag + "g", n, c, d // 2, h // 2, w // 2, values=(-16, -8, 8, 16), density=0.6)   # multiples of 8: avg divides by 8
    add = lattice(tag + "a", n, c, *shape, density=0.5) if with_add else None
    gy = lattice(tag + "y", n, c, *shape, density=0.5)
    outs = {False: lattice(tag + "o", n, c, *shape, values=(-2, -1, 1, 2, 3), density=0.7),      # block output: ties inside the windows
            True: elu_lattice(tag + "e", n, c, *shape, window_max=True)}
    refs = {}
    for act in GN_ACTS:
        out = outs[act == L.ACT_ELU]
        xr = out.double().requires_grad_(True)
        (F.max_pool3d if pool == "max" else F.avg_pool3d)(xr, 2).backward(dyp.double())
        dx_ref = xr.grad + (add.double() if with_add else 0)
        assert_representable(dx_ref, dt, "pool2_bwd_gn dx")
        assert_representable(out, dt, "pool2_bwd_gn block output")
        du = gn_reference(dx_ref, out.double(), act)
        check_sum_conditions(du, tag, other=gy.double(), unit=SUM_UNIT[act])
        refs[act] = (out, dx_ref, du)
    return dyp, add, gy, refs


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("n,c,shape,pool,with_add", POOL_GN_CASES)
def test_pooling_backward_with_groupnorm_sums(mode, n, c, shape, pool, with_add):
    """mednet_pool2_bwd_gn: dx = pooling backward (+ add), du = dx * act'(block output), rows = {sum du, sum du * gn_y}."""
    dt, dcode = DT[mode], dcode_of(mode)
    lib = L.lib()
    d, h, w = shape
    rows = lib.mednet_pool2_bwd_gn_rows(n, d, h, w, c, dcode)
    assert rows > 0
    tag = f"expg{n, c, shape, pool}"
    dyp, add, gy, refs = pool_gn_inputs(n, c, shape, pool, with_add, dt)
    dev = lambda a: None if a is None else a.to(DEV).to(dt).contiguous(memory_format=CL)
    total = 0
    for act in GN_ACTS:
        out, dx_ref, du = refs[act]
        dx = torch.full((n, c, *shape), float("nan"), device=DEV).to(dt).contiguous(memory_format=CL)
        part = torch.full((n, rows, c, 2), float("nan"), device=DEV)
        outg, dypg, addg, gyg = dev(out), dev(dyp), dev(add), dev(gy)
        L.check(lib.mednet_pool2_bwd_gn(dypg.data_ptr(), outg.data_ptr(), L.ptr(addg), dx.data_ptr(), gyg.data_ptr(), act, part.data_ptr(),
                                        n, d, h, w, c, L.POOL_MAX if pool == "max" else L.POOL_AVG, dcode, L.stream()), "pool2_bwd_gn")
        torch.cuda.synchronize()
        total += assert_exact(dx, dx_ref, f"pool2_bwd_gn {mode} act={act}: dx") + compare_channel_sums(part, du, gy.double(), f"pool2_bwd_gn {mode} act={act}")
    report("e", f"pool2_bwd_gn {n, c, shape, pool} {mode}", "pool2_bwd_gn", total)


HEAD_GN_CASES = [(2, 32, 4, (6, 8, 10)), (1, 64, 2, (9, 11, 21)), (2, 16, 3, (5, 6, 7))]


def head_gn_inputs(n, cin, cout, shape, dt):
    """-> weights, dy, gn_y, the reference dx and per activation (block output, du), the exactness conditions asserted."""
    tag = f"exhg{n, cin, cout, shape}"
    wt = lattice(tag + "w", cout, cin, 1, 1, 1, values=(-3, -2, -1, 1, 2, 3), density=0.75)
    dy = lattice(tag + "g", n, cout, *shape, density=0.5)
    gy = lattice(tag + "y", n, cin, *shape, density=0.5)
    gzs = {False: lattice(tag + "z", n, cin, *shape, values=(-1, 1, 2), density=0.7),      # the block output
           True: elu_lattice(tag + "e", n, cin, *shape)}
    dx_ref = torch.einsum("nozyx,oc->nczyx", dy.double(), wt.double()[:, :, 0, 0, 0])
    assert_representable(dx_ref, dt, "head_dgrad_gn dx")
    refs = {}
    for act in GN_ACTS:
        gz = gzs[act == L.ACT_ELU]
        assert_representable(gz, dt, "head_dgrad_gn block output")
        du = gn_reference(dx_ref, gz.double(), act)
        check_sum_conditions(du, tag, other=gy.double(), unit=SUM_UNIT[act])
        refs[act] = (gz, du)
    return wt, dy, gy, dx_ref, refs


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("n,cin,cout,shape", HEAD_GN_CASES)
def test_head_data_gradient_with_groupnorm_sums(mode, n, cin, cout, shape):
    """mednet_head_dgrad_gn: dx = W^T dlogits (planar fp32 logit gradients), du = dx * act'(block output), rows = {sum du,
    sum du * gn_y}."""
    dt, dcode = DT[mode], dcode_of(mode)
    lib = L.lib()
    d, h, w = shape
    rows = lib.mednet_head_dgrad_gn_rows(n, d, h, w, cin, dcode)
    assert rows > 0
    wt, dy, gy, dx_ref, refs = head_gn_inputs(n, cin, cout, shape, dt)
    with mednet_hip.precision(mode):
        pk = ops.pack_conv_weight(wt.to(DEV), 1, False)
    dev = lambda a: a.to(DEV).to(dt).contiguous(memory_format=CL)
    dyg, gyg = dy.to(DEV).contiguous(), dev(gy)
    total = 0
    for act in GN_ACTS:
        gz, du = refs[act]
        gzg = dev(gz)
        dx = torch.full((n, cin, *shape), float("nan"), device=DEV).to(dt).contiguous(memory_format=CL)
        part = torch.full((n, rows, cin, 2), float("nan"), device=DEV)
        L.check(lib.mednet_head_dgrad_gn(dyg.data_ptr(), pk.data_ptr(), dx.data_ptr(), gyg.data_ptr(), gzg.data_ptr(), act, part.data_ptr(),
                                         n, d, h, w, cin, cout, dcode, L.stream()), "head_dgrad_gn")
        torch.cuda.synchronize()
        total += assert_exact(dx, dx_ref, f"head_dgrad_gn {mode} act={act}: dx") + compare_channel_sums(part, du, gy.double(), f"head_dgrad_gn {mode} act={act}")
    report("e", f"head_dgrad_gn {n, cin, cout, shape} {mode}", "head_dgrad_gn", total)


CONVT_GN_CASES = [(2, 64, 32, (3, 5, 9), 2), (1, 32, 32, (5, 9, 17), 2), (2, 64, 32, (16, 32, 32), 7)]


def convt_gn_inputs(n, cin, cout, shape, mode):
    """-> the ConvTranspose3d case, gn_y, the reference dx and per activation (block output, du), the conditions asserted."""
    c = case("convt", n, cin, cout, shape, bias=True, skip=True)
    c.check_conditions(mode)
    dx_ref = c.ref()[0]["dx"]
    tag = f"exct{n, cin, cout, shape}"
    gy = lattice(tag + "y", n, cin, *shape, values=(-1, 1), density=0.25)
    gzs = {False: lattice(tag + "z", n, cin, *shape, values=(-1, 1, 2), density=0.7), True: elu_lattice(tag + "e", n, cin, *shape)}
    refs = {}
    for act in GN_ACTS:
        gz = gzs[act == L.ACT_ELU]
        assert_representable(gz, DT[mode], "convt3d_dgrad_gn block output")
        du = gn_reference(dx_ref, gz.double(), act)
        check_sum_conditions(du, tag, other=gy.double(), unit=SUM_UNIT[act])
        refs[act] = (gz, du)
    return c, gy, dx_ref, refs


@pytest.mark.parametrize("mode", MODES16)
@pytest.mark.parametrize("n,cin,cout,shape,kind", CONVT_GN_CASES)
def test_conv_transpose_data_gradient_with_groupnorm_sums(mode, n, cin, cout, shape, kind):
    """mednet_convt3d_dgrad_gn (conv_mfma_kernel<2> and convt_dgrad32_mfma_kernel): dx of the ConvTranspose3d, du = dx * act'(block
    output), rows = {sum du, sum du * gn_y}."""
    dt, dcode = DT[mode], dcode_of(mode)
    lib = L.lib()
    d, h, w = shape
    c, gy, dx_ref, refs = convt_gn_inputs(n, cin, cout, shape, mode)
    assert stats_plan(n, shape, cin, cout, dcode, gnb=1, stride=2)[0] == kind
    rows = lib.mednet_convt3d_dgrad_gn_rows(n, d, h, w, cin, cout, dcode, L.ALGO_MFMA)
    assert rows > 0
    with mednet_hip.precision(mode):
        pk = ops.pack_conv_weight(c.w.to(DEV), 3, True)
    dev = lambda a: a.to(DEV).to(dt).contiguous(memory_format=CL)
    dyg, gyg = dev(c.g), dev(gy)
    total = 0
    for act in GN_ACTS:
        gz, du = refs[act]
        gzg = dev(gz)
        dx = torch.full((n, cin, *shape), float("nan"), device=DEV).to(dt).contiguous(memory_format=CL)
        part = torch.full((n, rows, cin, 2), float("nan"), device=DEV)
        L.check(lib.mednet_convt3d_dgrad_gn(dyg.data_ptr(), pk.data_ptr(), dx.data_ptr(), gyg.data_ptr(), gzg.data_ptr(), act, part.data_ptr(),
                                            n, d, h, w, cin, cout, dcode, L.ALGO_MFMA, L.stream()), "convt3d_dgrad_gn")
        torch.cuda.synchronize()
        total += assert_exact(dx, dx_ref, f"convt3d_dgrad_gn {mode} act={act}: dx") + compare_channel_sums(part, du, gy.double(), f"convt3d_dgrad_gn {mode} act={act}")
    report("e", f"convt3d_dgrad_gn {n, cin, cout, shape} {mode}", f"plan kind {kind}", total)


# ------------------------------------------------------------------------------------------------ (f) 1x1x1 head
@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("n,cin,cout,shape", [(2, 32, 4, (6, 8, 10)), (1, 8, 18, (5, 6, 7)), (1, 8, 3, (4, 4, 5)), (1, 8, 2, (8, 8, 8)),
                                              (2, 64, 2, (6, 8, 10))])
def test_head_planar_logits(mode, n, cin, cout, shape):
    """hnn.Conv3d(cin, cout, 1, planar_output=True): fp32 planar logits, dx, dw and db."""
    dt = DT[mode]
    tag = f"exh{n, cin, cout, shape}"
    x = lattice(tag + "x", n, cin, *shape, density=0.5)
    w = lattice(tag + "w", cout, cin, 1, 1, 1, values=(-3, -2, -1, 1, 2, 3), density=0.75)
    b = lattice(tag + "b", cout, values=(-3, -1, 1, 2), density=0.75)
    g = lattice(tag + "g", n, cout, *shape, density=0.5)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    yr = F.conv3d(xr, wr, br)
    yr.backward(g.double())
    assert_representable(xr.grad, dt, "head dx")
    assert_sums_exact(F.conv3d(x.abs().double(), w.abs().double(), b.abs().double()), "head y")
    assert_sums_exact(x.abs().double().sum() * g.abs().double().max(), "head dw")
    with mednet_hip.precision(mode):
        conv = hnn.Conv3d(cin, cout, 1, planar_output=True).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(w)
            conv.bias.copy_(b)
        xg = x.to(DEV).to(dt).requires_grad_(True)
        y = conv(xg)
        assert y.dtype == torch.float32 and y.is_contiguous()
        y.backward(g.to(DEV))
        torch.cuda.synchronize()
    total = (assert_exact(y, yr, f"head {mode}: logits") + assert_exact(xg.grad, xr.grad, f"head {mode}: dx")
             + assert_exact(conv.weight.grad, wr.grad, f"head {mode}: dw") + assert_exact(conv.bias.grad, br.grad, f"head {mode}: db"))
    report("f", f"head {n, cin, cout, shape} {mode}", "1x1x1 head", total)


# ------------------------------------------------------------------------------------------------ (g) selection / averaging
@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("c,shape,kind", [(8, (8, 12, 10), "max"), (32, (4, 4, 4), "max"), (8, (7, 9, 11), "max"), (3, (6, 5, 4), "max"),
                                          (16, (6, 6, 6), "avg"), (5, (5, 7, 6), "avg")])
def test_pool2(mode, c, shape, kind):
    """2x2x2 max / average pooling, forward and backward, odd sizes and ties included; inputs are multiples of 8 for the
    average (it divides by 8), gradients multiples of 8 likewise."""
    n, dt = 2, DT[mode]
    x = lattice(f"exp{c}{shape}", n, c, *shape, values=(-16, -8, 8, 16, 24), density=0.7)
    oshape = tuple(s // 2 for s in shape)
    g = lattice(f"expg{c}{shape}", n, c, *oshape, values=(-16, -8, 8, 16), density=0.8)
    xr = x.double().requires_grad_(True)
    yr = (F.max_pool3d if kind == "max" else F.avg_pool3d)(xr, 2)
    yr.backward(g.double())
    assert_representable(yr, dt, "pool y")
    assert_representable(xr.grad, dt, "pool dx")
    with mednet_hip.precision(mode):
        xg = x.to(DEV).to(dt).requires_grad_(True)
        y = ops.pool2(xg, L.POOL_MAX if kind == "max" else L.POOL_AVG)
        y.backward(g.to(DEV).to(dt))
    total = assert_exact(y, yr, f"pool2 {kind} {mode}: y") + assert_exact(xg.grad, xr.grad, f"pool2 {kind} {mode}: dx")
    # ... and the backward with a second gradient summed in (the decoder's skip join)
    lib, dcode = L.lib(), dcode_of(mode)
    add = lattice(f"expa{c}{shape}", n, c, *shape, density=0.5)
    dev = lambda a: a.to(DEV).to(dt).contiguous(memory_format=CL)
    dx = torch.full((n, c, *shape), float("nan"), device=DEV).to(dt).contiguous(memory_format=CL)
    gg, xx, aa = dev(g), dev(x), dev(add)
    L.check(lib.mednet_pool2_bwd(gg.data_ptr(), xx.data_ptr(), aa.data_ptr(), dx.data_ptr(), n, *shape, c,
                                 L.POOL_MAX if kind == "max" else L.POOL_AVG, dcode, L.stream()), "pool2_bwd")
    torch.cuda.synchronize()
    assert_representable(xr.grad + add.double(), dt, "pool dx + add")
    total += assert_exact(dx, xr.grad + add.double(), f"pool2_bwd + add {kind} {mode}")
    report("g", f"pool2 {kind} {c, shape} {mode}", "pool2_fwd/bwd(+add)", total)


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("ce,cx,eshape,xshape", [(8, 16, (8, 12, 10), (4, 6, 5)), (8, 16, (7, 9, 10), (3, 4, 5)), (3, 5, (5, 5, 5), (2, 2, 2)),
                                                 (16, 32, (9, 7, 11), (4, 3, 5))])
def test_upsample_concat(mode, ce, cx, eshape, xshape):
    """Nearest-neighbour upsampling + concatenation, forward / backward (odd `eshape` included) and the GroupNorm sums of
    mednet_upcat_fwd_stats."""
    n, dt = 2, DT[mode]
    e = lattice(f"exue{ce}{eshape}", n, ce, *eshape, density=0.6)
    x = lattice(f"exux{cx}{xshape}", n, cx, *xshape, density=0.6)
    g = lattice(f"exug{ce}{cx}{eshape}", n, ce + cx, *eshape, density=0.6)
    er, xr = e.double().requires_grad_(True), x.double().requires_grad_(True)
    yr = torch.cat((er, F.interpolate(xr, size=eshape, mode="nearest")), dim=1)
    yr.backward(g.double())
    assert_representable(xr.grad, dt, "upcat dx")
    with mednet_hip.precision(mode):
        eg, xg = e.to(DEV).to(dt).requires_grad_(True), x.to(DEV).to(dt).requires_grad_(True)
        y = ops.upsample_concat(eg, xg)
        y.backward(g.to(DEV).to(dt))
    total = (assert_exact(y, yr, f"upcat {mode}: y") + assert_exact(eg.grad, er.grad, f"upcat {mode}: denc")
             + assert_exact(xg.grad, xr.grad, f"upcat {mode}: dx"))
    lib, dcode = L.lib(), dcode_of(mode)
    chunks = lib.mednet_upcat_stats_chunks(n, *eshape, ce, cx, dcode)
    if chunks > 0:
        check_sum_conditions(yr.detach(), "upcat stats")
        out = ops.empty_cl(n, ce + cx, *eshape, dt, DEV)
        part = torch.full((n, chunks, ce + cx, 2), float("nan"), device=DEV)
        ecl, xcl = ops.to_cl(e.to(DEV).to(dt)), ops.to_cl(x.to(DEV).to(dt))
        L.check(lib.mednet_upcat_fwd_stats(ecl.data_ptr(), xcl.data_ptr(), out.data_ptr(), part.data_ptr(), n, *eshape, ce, *xshape, cx,
                                           dcode, L.stream()), "upcat_stats")
        torch.cuda.synchronize()
        total += assert_exact(out, yr, f"upcat_fwd_stats {mode}: out") + compare_pair_sums(part, yr.detach(), f"upcat_fwd_stats {mode}", per_channel=True)
    report("g", f"upcat {ce, cx, eshape} {mode}", f"upcat fwd/bwd, stats rows {chunks}", total)


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("n,c,shape,pool,residual", [(2, 32, (8, 12, 16), "max", True), (1, 64, (6, 4, 10), "avg", True),
                                                     (2, 16, (4, 8, 6), "max", False), (1, 8, (5, 7, 9), None, True)])
def test_add_and_groupnorm_apply(mode, n, c, shape, pool, residual):
    """mednet_add, and mednet_gn_act_fwd / mednet_gn_act_pool_fwd driven directly with power-of-two coefficients, a lattice
    residual and activation none / ReLU: z and the pooled tensor exact."""
    dt, dcode = DT[mode], dcode_of(mode)
    lib = L.lib()
    d, h, w = shape
    tag = f"exga{n, c, shape}"
    y = lattice(tag + "y", n, c, *shape, values=(-4, -2, 2, 4), density=0.7)
    r = lattice(tag + "r", n, c, *shape, values=(-8, 8, 16), density=0.5) if residual else None
    ca = lattice(tag + "ca", n, c, values=(-4, -2, 2, 4, 8), density=1.0)       # (even y times ca >= 2: multiples of 4, + cb, + r)
    cb = lattice(tag + "cb", n, c, values=(-8, -4, 4, 8), density=1.0)
    coef = torch.stack((ca, cb), -1).contiguous().to(DEV)
    dev = lambda a: None if a is None else a.to(DEV).to(dt).contiguous(memory_format=CL)
    yg, rg = dev(y), dev(r)
    u = ca.double()[:, :, None, None, None] * y.double() + cb.double()[:, :, None, None, None] + (r.double() if residual else 0)
    total = 0
    for act, fn in ((L.ACT_NONE, lambda t: t), (L.ACT_RELU, F.relu)):
        zr = fn(u)
        assert_representable(zr, dt, "gn_act z")
        z = torch.full((n, c, *shape), float("nan"), device=DEV).to(dt).contiguous(memory_format=CL)
        L.check(lib.mednet_gn_act_fwd(yg.data_ptr(), coef.data_ptr(), L.ptr(rg), z.data_ptr(), n, d * h * w, c, act, dcode, dcode, L.stream()), "gn_act_fwd")
        torch.cuda.synchronize()
        total += assert_exact(z, zr, f"gn_act_fwd {mode} act={act}")
        if pool is not None:
            assert lib.mednet_gn_act_pool_supported(d, h, w, c, dcode)
            pr = (F.max_pool3d if pool == "max" else F.avg_pool3d)(zr, 2)    # (z: multiples of 4 below 64, the average of 8: halves)
            z1 = torch.full_like(z, float("nan"))
            p1 = torch.full((n, c, d // 2, h // 2, w // 2), float("nan"), device=DEV).to(dt).contiguous(memory_format=CL)
            L.check(lib.mednet_gn_act_pool_fwd(yg.data_ptr(), coef.data_ptr(), L.ptr(rg), z1.data_ptr(), p1.data_ptr(), n, d, h, w, c, act,
                                               L.POOL_MAX if pool == "max" else L.POOL_AVG, dcode, L.stream()), "gn_act_pool_fwd")
            torch.cuda.synchronize()
            assert_representable(pr, dt, "gn_act_pool pooled")
            total += assert_exact(z1, zr, f"gn_act_pool_fwd {mode} act={act}: z") + assert_exact(p1, pr, f"gn_act_pool_fwd {mode} act={act}: pooled")
    a, b = dev(y), dev(lattice(tag + "b", n, c, *shape, density=0.6))
    out = torch.full_like(a, float("nan"))
    L.check(lib.mednet_add(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), dcode, L.stream()), "add")
    torch.cuda.synchronize()
    total += assert_exact(out, a.double().cpu() + b.double().cpu(), f"mednet_add {mode}")
    report("g", f"gn_act / add {n, c, shape} {mode}", "gn_act_fwd, gn_act_pool_fwd, add", total)
