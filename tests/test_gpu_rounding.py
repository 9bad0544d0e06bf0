"""Rounding tests of the conv family: every 16-bit store against ONE round-to-nearest-even of the exact result.

tests/test_gpu_exact.py feeds lattice inputs whose exact result is a number of the output type, so truncation, round-half-away,
flushed subnormals, a saturating store, a second rounding and statistics taken before the store all give the same bits there.
The cases here keep that suite's other premise -- every fp32 partial sum is exact (gpu_util.assert_sums_exact) -- and drop
representability: the weights of even output channels are multiplied by 2^m + 1 and those of odd ones by 2^m - 1 (m = 7 for
bf16, 9 for fp16, 10 where an output has few terms; both multipliers are numbers of the storage type).  The accumulator then holds the exact result, the kernel
rounds exactly once, and `ref64.to(dtype)` of ATen's fp64 result is the unique correct answer: equality in every element
(gpu_util.assert_rounded) stays the demand and needs no bound.  With two multipliers the exact ties resolve in both directions,
so round-half-away fails as well.  Powers of two on x, w and g keep every sum exact and move the results into fp16's subnormal
range or beyond 65504.

Every test first asserts, on the reference alone, what makes the comparison telling (gpu_util.assert_rounding_premises: the
share of elements that are no numbers of the type, ties in both directions, subnormals, infinities, the difference between the
one- and two-rounding candidates of a join, between the sums of rounded and of unrounded values); tests/test_rounding_util.py
asserts the same on the CPU and shows that the comparison rejects each fault it is there for.

(a) store rounding of every forward / data-gradient kernel, (b) the joins -- ConvTranspose3d forward adds bias and skip in fp32
and rounds ONCE, the stride-1 data gradient with `add` stores the gradient and adds to the STORED value, two roundings, equal to
the two-launch form --, (c) the fused GroupNorm sums are sums of the stored values: first moments EXACT, second moments only
BOUNDED by gpu_util's summation bound (squares of these values do not keep fp32 sums exact), (d) fp16 subnormal outputs,
subnormal inputs and overflow to +-inf, (e) the joins of csrc/norm_act.hip.

bf16 subnormals and bf16 overflow are left out on purpose: their accumulators would be fp32 subnormals or infinities, where
"every partial sum is exact" no longer holds.  The fp32 storage mode stores the exact sum; weight gradients are fp32.

Every comparison prints `[exact] item=.. kernel=.. elements=.. nonrep=.. ties=towards/away subnormal=.. zeroed=.. inf=..`.
"""
import pytest
import torch
import torch.nn.functional as F

import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import nn as hnn
from mednet_hip import ops

import test_gpu_exact as X
from gpu_util import (DEV, SUM_BOUND, add_counts, assert_exact, assert_representable, assert_rounded, assert_rounding_premises,
                      assert_sums_exact, census_counts, check_gn_sums, lattice, report_rounding, rounding_census)

pytestmark = pytest.mark.gpu
CL = torch.channels_last_3d
DT = X.DT
M = {"bf16": 7, "fp16": 9, "fp16x2": 9}     # multipliers 2^m +- 1: 8 significant bits for bf16, 10 of fp16's 11
M_FEW = {"bf16": 7, "fp16": 10, "fp16x2": 10}   # outputs of few terms: fp16 takes all 11 bits
FEW = dict(m=M_FEW, amp=3)
F16_TINY = 2.0 ** -14                       # fp16's smallest normal number


# ------------------------------------------------------------------------------------------------ cases and references
class RCase(X.Case):
    """test_gpu_exact.Case on the rounding lattice: the same x, w, g (same seeds and densities), the weights of even OUTPUT channels
    times 2^m + 1 and of odd ones times 2^m - 1; x and g times `amp` (3 where an output has few terms -- a first layer, the 27 / 8
    taps of a ConvTranspose3d output --, so that a single product is already no number of the type).  The reference holds y, the
    bare convolution `conv` (y without bias and skip) and dx; no weight gradient (fp32, out of scope)."""

    def __init__(self, kind, n, cin, cout, shape, m, bias=False, skip=False, amp=1):
        super().__init__(kind, n, cin, cout, shape, bias=bias, skip=skip)
        self.m = m
        self.x, self.g = self.x * amp, self.g * amp
        mult = torch.where(torch.arange(cout) % 2 == 0, 2.0 ** m + 1, 2.0 ** m - 1).float()
        self.w = (self.w * mult.view((1, cout, 1, 1, 1) if kind == "convt" else (cout, 1, 1, 1, 1))).contiguous()
        self.unit = dict(y=1.0, conv=1.0, dx=1.0)

    def _run(self, x, w, b, g, skip):
        x = x.double().requires_grad_(True)
        if self.kind == "convt":
            conv = F.conv_transpose3d(x, w.double(), None, stride=2, padding=1, output_padding=1)
        else:
            conv = F.conv3d(x, w.double(), None, padding=1)
        y = conv
        if b is not None:
            y = y + b.double().view(1, -1, 1, 1, 1)
        if skip is not None:
            y = y + skip.double()
        y.backward(g.double())
        return dict(y=y.detach(), conv=conv.detach(), dx=x.grad)

    def scaled(self, ex=0, ew=0, eg=0):
        return self if ex == ew == eg == 0 else Scaled(self, ex, ew, eg)

    def premises(self, mode, keys=("y", "dx"), **minima):
        """Every operand is a number of the storage type, every sum exact, and per output the rounding premises -> {key: census}."""
        dt = DT[mode]
        ref, mag = self.ref()
        for t, name in ((self.x, "x"), (self.w, "w"), (self.g, "g"), (self.skip, "skip")):
            if t is not None and not (name == "x" and self.cin <= 4):      # (a first layer takes its input in fp32)
                assert_representable(t, dt, f"{self} {mode} operand {name}")
        out = {}
        for k in keys:
            assert_sums_exact(mag[k], f"{self} {mode} {k}", unit=self.unit[k])
            out[k] = assert_rounding_premises(ref[k], dt, f"{self} {mode} {k}", **minima)
        return out

    def __repr__(self):
        return f"{self.kind}(n={self.n}, {self.cin}->{self.cout}, {self.shape}, m={self.m})"


class Scaled:
    """A case with x, w, g times 2^ex, 2^ew, 2^eg: every sum stays exact, the references are the base's times a power of two."""
    premises = RCase.premises

    def __init__(self, base, ex, ew, eg):
        self.base, self.e = base, (ex, ew, eg)
        for k in ("kind", "n", "cin", "cout", "shape", "oshape", "m"):
            setattr(self, k, getattr(base, k))
        sy, sd = 2.0 ** (ex + ew), 2.0 ** (eg + ew)
        self.x, self.w, self.g = base.x * 2.0 ** ex, base.w * 2.0 ** ew, base.g * 2.0 ** eg
        self.b = None if base.b is None else base.b * sy
        self.skip = None if base.skip is None else base.skip * sy
        self.unit = dict(y=sy, conv=sy, dx=sd)

    def ref(self):
        ref, mag = self.base.ref()
        return tuple({k: v * self.unit[k] for k, v in r.items()} for r in (ref, mag))

    def __repr__(self):
        return f"{self.base} * 2^{self.e}"


_RCASES = {}


def rcase(kind, n, cin, cout, shape, m, **kw):
    key = (kind, n, cin, cout, tuple(shape), m, tuple(sorted(kw.items())))
    if key not in _RCASES:
        _RCASES[key] = RCase(kind, n, cin, cout, shape, m, **kw)
    return _RCASES[key]


def compare_rounded(c, got, mode, cens, what, keys=("y", "dx")):
    """-> (elements compared, summed census counts)"""
    ref = c.ref()[0]
    total, counts = 0, {}
    for k in keys:
        total += assert_rounded(got[k], ref[k], DT[mode], f"{what}: {k}")
        add_counts(counts, census_counts(cens[k]))
    return total, counts


# ------------------------------------------------------------------------------------------------ the kernels and how each is reached
# name -> (kind, n, cin, cout, shape, storage modes, algorithm, options, arguments of the case): for each kernel the smallest
# shape of test_gpu_exact's case lists that its plan query shows reaching it
KERNELS = {
    "general": ("conv", 2, 32, 32, (9, 11, 21), ("bf16", "fp16", "fp16x2"), "mfma", dict(conv32=0, conv2b=0, conv2b_split=0), {}),
    "general-narrow": ("conv", 2, 64, 96, (10, 10, 6), ("bf16", "fp16", "fp16x2"), "mfma", dict(conv32=0, conv2b=0, conv2b_split=0), {}),
    "general-half-block": ("conv", 1, 16, 16, (5, 9, 17), ("bf16", "fp16", "fp16x2"), "mfma", dict(conv32=0, conv2b=0, conv2b_split=0), {}),
    "conv32": ("conv", 1, 32, 32, (66, 60, 50), ("bf16", "fp16"), "mfma", {}, {}),                      # 544 bricks, ragged
    "conv2b": ("conv", 1, 64, 64, (30, 60, 50), ("bf16", "fp16"), "mfma", dict(conv2b_min_fill=0), {}),   # 256 brick slots
    "conv2b-split": ("conv", 2, 32, 32, (9, 11, 21), ("fp16x2",), "mfma", {}, {}),
    "direct": ("conv", 1, 32, 32, (8, 8, 16), ("bf16", "fp16"), "direct", {}, {}),
    "direct-odd": ("conv", 1, 8, 16, (5, 7, 9), ("bf16", "fp16"), "direct", {}, dict(bias=True)),
    "convt": ("convt", 2, 64, 32, (3, 5, 9), ("bf16", "fp16"), "mfma", {}, dict(m=M_FEW)),
    "convt-wide": ("convt", 1, 256, 128, (4, 4, 4), ("fp16",), "mfma", {}, {}),     # (m = 9: its weights times 2^-24 are subnormals)
    "convt-direct": ("convt", 2, 16, 8, (3, 5, 4), ("bf16", "fp16"), "direct", {}, FEW),
    "convt_dgrad32": ("convt", 2, 64, 32, (16, 32, 32), ("bf16", "fp16"), "mfma", {}, {}),               # 256 bricks of 2 x 4 x 16
}
STORE_PARAMS = [(name, mode) for name, spec in KERNELS.items() for mode in spec[5]]
EDGE_KERNELS = [("general", "fp16"), ("conv32", "fp16"), ("conv2b", "fp16"), ("conv2b-split", "fp16x2"), ("direct", "fp16"), ("convt-wide", "fp16")]


def kernel_case(name, mode, **kw):
    kind, n, cin, cout, shape, _, _, _, args = KERNELS[name]
    args = dict(args, **kw)
    return rcase(kind, n, cin, cout, shape, args.pop("m", M)[mode], **args)


def check_plan(name, mode):
    """The library's own plan queries show which kernel takes the case (inside the case's options) -> its name for the report."""
    kind, n, cin, cout, shape, _, algo, _, _ = KERNELS[name]
    dcode, split = X.dcode_of(mode), mode == "fp16x2"
    if algo == "direct":
        return f"{kind} direct"
    if kind == "convt":
        assert L.lib().mednet_convt3d_dgrad_gn_rows(n, *shape, cin, cout, dcode, L.ALGO_MFMA) > 0
        want = 7 if name == "convt_dgrad32" else 2
        assert X.stats_plan(n, shape, cin, cout, dcode, gnb=1, stride=2)[0] == want
        return "convt forward + " + ("convt_dgrad32_mfma_kernel" if want == 7 else "conv_mfma_kernel<2>")
    kinds = {"conv32": (4,), "conv2b": (5, 6), "conv2b-split": (5, 6)}.get(name, (2, 3))
    for a, b in ((cin, cout), (cout, cin)):     # forward and data-gradient form
        assert X.stats_plan(n, shape, a, b, dcode, split=split)[0] in kinds, (name, mode, a, b)
    assert L.lib().mednet_conv3d_act_supported(n, *shape, cin, cout, L.ALGO_MFMA) == 1
    return {4: "conv32_mfma_kernel", 5: "conv2b_mfma_kernel"}.get(kinds[0], "conv_mfma_kernel") + (" (high, low)" if split else "")


def run_kernel(name, c, mode):
    _, _, _, _, _, _, algo, opts, _ = KERNELS[name]
    with X.options(**opts):
        kernel = check_plan(name, mode)
        got = X.run_layer(c, mode, algo)
    return kernel, got


# ------------------------------------------------------------------------------------------------ (a) store rounding
@pytest.mark.parametrize("name,mode", STORE_PARAMS)
def test_store_rounding(name, mode):
    """The accumulator-to-storage step of the forward and of the data gradient is ONE round-to-nearest-even: the general
    matrix-core kernel (16-wide, narrow and half-filled bricks, ragged edges), conv32_mfma_kernel, conv2b_mfma_kernel and its
    (high, low) form, the direct kernels, ConvTranspose3d on the matrix cores and direct, convt_dgrad32."""
    c = kernel_case(name, mode)
    cens = c.premises(mode)
    kernel, got = run_kernel(name, c, mode)
    total, counts = compare_rounded(c, got, mode, cens, f"{name} {mode} {c}")
    report_rounding("a", f"{c} {mode}", kernel, total, counts)


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp16x2"])
@pytest.mark.parametrize("cin", [1, 4])
def test_store_rounding_of_the_first_layer(mode, cin):
    """conv_first_mfma_kernel with 1 and 4 input channels (fp32 input), under both weight-gradient dispatches."""
    n, cout, shape = 2, 32, (9, 11, 21)
    c = rcase("conv", n, cin, cout, shape, M_FEW[mode], amp=3)
    cens = c.premises(mode, keys=("y",))
    lib, dt = L.lib(), DT[mode]
    algo = L.ALGO_AUTO | (L.ALGO_SPLITW_BIT if mode == "fp16x2" else 0)
    rows = lib.mednet_conv3d_fused_stats_chunks(n, *shape, cin, cout, 3, L.F32, L.dt_of(dt), algo)
    assert rows > 0, "the first-layer matrix-core kernel does not take this call"
    total, counts = 0, {}
    for c1 in (1, 0):
        with X.options(wgrad_c1_mfma=c1), mednet_hip.precision(mode):
            conv = hnn.Conv3d(cin, cout, 3, bias=False).to(DEV)
            with torch.no_grad():
                conv.weight.copy_(c.w)
            y, partial = conv.forward_with_stats(c.x.to(DEV))
            assert partial is not None and tuple(partial.shape) == (n, rows, cout, 2)
            y.backward(c.g.to(DEV).to(dt))
            torch.cuda.synchronize()
        t, k = compare_rounded(c, dict(y=y.detach()), mode, cens, f"first layer cin={cin} {mode} wgrad_c1_mfma={c1}", keys=("y",))
        total += t
        add_counts(counts, k)
    report_rounding("a", f"{c} {mode}", f"conv_first_mfma_kernel<{cin}>", total, counts)


# ------------------------------------------------------------------------------------------------ (b) the joins
def join_candidates(conv, other, dt):
    """one = (conv64 + other).to(dt): fp32 add, one rounding; two = (conv64.to(dt) + other).to(dt): the convolution stored, read
    back and added -- what two launches give.  Both as fp64."""
    one = (conv + other).to(dt).double()
    two = (conv.to(dt).double() + other).to(dt).double()
    return one, two


def assert_candidates_differ(one, two, what, share=0.01):
    d = int((one != two).sum())
    assert d >= share * one.numel(), f"{what}: the one- and two-rounding candidates differ in {d} of {one.numel()} elements only"
    return d


def convt_join(c, mode):
    """ConvTranspose3d forward with bias and skip -> (one, two) after the premise that they differ in >= 1 % of the elements."""
    ref = c.ref()[0]
    one, two = join_candidates(ref["conv"], ref["y"] - ref["conv"], DT[mode])
    assert torch.equal(one, ref["y"].to(DT[mode]).double())
    return one, two, assert_candidates_differ(one, two, f"{c} {mode} bias + skip")


@pytest.mark.parametrize("mode", X.MODES16)
@pytest.mark.parametrize("name", ["convt", "convt-direct", "convt_dgrad32"])
def test_conv_transpose_join_rounds_once(name, mode):
    """mednet_convt3d_fwd adds bias and skip to the fp32 accumulator and rounds ONCE, as it documents; the two-rounding candidate
    differs from that in >= 1 % of the elements."""
    c = kernel_case(name, mode, bias=True, skip=True)
    cens = c.premises(mode)
    one, two, differ = convt_join(c, mode)
    kernel, got = run_kernel(name, c, mode)
    total, counts = compare_rounded(c, got, mode, cens, f"{name} join {mode} {c}")
    assert not torch.equal(got["y"].double().cpu(), two)
    report_rounding("b", f"{c} {mode} bias+skip one-vs-two={differ}", kernel, total, counts)


JOIN_CASES = [   # the data gradient with a summed second gradient: (kernel, storage modes, layer, plan kinds, options)
    ("general", X.MODES16, (2, 32, 32, (9, 11, 21)), (2, 3), dict(conv32=0, conv2b=0)),
    ("conv32", X.MODES16, (1, 32, 32, (66, 60, 50)), (4,), {}),
    ("conv2b", X.MODES16, (1, 64, 64, (30, 60, 50)), (5, 6), dict(conv2b_min_fill=0)),
]
JOIN_PARAMS = [(name, mode) for name, modes, _, _, _ in JOIN_CASES for mode in modes]
_JOIN = {}


def dgrad_join_inputs(key, mode):
    """dy, rounding-lattice weights, `add` (small integers: of the size of the stored gradient's rounding error), gn_y and
    power-of-two coefficients; dx64 = the exact data gradient and the two candidates, the premises asserted."""
    if (key, mode) in _JOIN:
        return _JOIN[(key, mode)]
    n, cin, cout, shape = key
    dt = DT[mode]
    c = rcase("conv", n, cin, cout, shape, M[mode])
    ref, mag = c.ref()
    tag = f"rdj{key}"
    add = lattice(tag + "a", n, cin, *shape, values=(-7, -5, -3, -2, -1, 1, 2, 3, 5, 7), density=0.75)
    gy = lattice(tag + "y", n, cin, *shape, values=(-4, -2, 2, 4), density=0.5)
    ca = lattice(tag + "ca", n, cin, values=(-2, -1, -0.5, 0.5, 1, 2), density=1.0)      # (ca * gn_y + cb is never zero: test_gpu_exact.dgrad_inputs)
    cb = lattice(tag + "cb", n, cin, values=(-1.5, -0.5, 0.5, 1.5), density=1.0)
    for t in (c.g, c.w, add, gy):
        assert_representable(t, dt, f"dgrad join {key} operand")
    assert_sums_exact(mag["dx"] + add.abs().double(), f"dgrad join {key}")
    one, two = join_candidates(ref["dx"], add.double(), dt)
    differ = assert_candidates_differ(one, two, f"dgrad join {key} {mode}")
    cen = assert_rounding_premises(ref["dx"], dt, f"dgrad join {key} {mode} dx")
    pre = ca.double()[:, :, None, None, None] * gy.double() + cb.double()[:, :, None, None, None]
    assert float(pre.abs().min()) > 0
    _JOIN[(key, mode)] = dict(c=c, add=add, gy=gy, coef=torch.stack((ca, cb), -1).contiguous(), pre=pre, one=one, two=two, differ=differ,
                              cen=cen, plain=ref["dx"].to(dt).double())
    return _JOIN[(key, mode)]


@pytest.mark.parametrize("name,mode", JOIN_PARAMS)
def test_data_gradient_join_rounds_twice(name, mode):
    """mednet_conv3d_dgrad_add and mednet_conv3d_dgrad_gn with `add`, in the general, conv32 and conv2b forms: the data gradient is
    rounded to the storage type, `add` is added to the STORED value and the sum rounded again -- exactly what mednet_add after a
    stored data gradient gives, and what the tests that hold fused to unfused bit for bit require.  Without `add` the store is one
    rounding.  The GroupNorm rows come from the stored dx (gpu_util.check_gn_sums: bounded; (c) has the exact cases)."""
    _, _, key, kinds, opts = next(j for j in JOIN_CASES if j[0] == name)
    n, cin, cout, shape = key
    d, h, wd = shape
    dt, dcode = DT[mode], X.dcode_of(mode)
    t = dgrad_join_inputs(key, mode)
    c, lib = t["c"], L.lib()
    dev = lambda a: a.to(DEV).to(dt).contiguous(memory_format=CL)
    dyg, addg, gyg, coef = dev(c.g), dev(t["add"]), dev(t["gy"]), t["coef"].to(DEV)
    total = 0
    with X.options(**opts):
        plan = X.stats_plan(n, shape, cout, cin, dcode, gnb=1)      # (the kernel's Cin / Cout = the layer's Cout / Cin)
        assert plan[0] in kinds, plan
        assert lib.mednet_conv3d_dgrad_add_supported(n, d, h, wd, cin, cout, L.ALGO_MFMA, dcode) == 1
        rows = lib.mednet_conv3d_dgrad_gn_rows_dt(n, d, h, wd, cin, cout, L.ALGO_MFMA, dcode)
        assert rows > 0
        with mednet_hip.precision(mode):
            pk = ops.pack_conv_weight(c.w.to(DEV), 3, False)
        dx = torch.full((n, cin, *shape), float("nan"), device=DEV).to(dt).contiguous(memory_format=CL)
        L.check(lib.mednet_conv3d_dgrad_add(dyg.data_ptr(), pk.data_ptr(), addg.data_ptr(), dx.data_ptr(), n, d, h, wd, cin, cout, L.ALGO_MFMA,
                                            dcode, L.stream()), "dgrad_add")
        torch.cuda.synchronize()
        total += assert_exact(dx, t["two"], f"dgrad_add {name} {mode} {key}: dx against the two-rounding candidate")
        for with_add in (True, False):
            for act in (L.ACT_NONE, L.ACT_RELU):
                dx = torch.full((n, cin, *shape), float("nan"), device=DEV).to(dt).contiguous(memory_format=CL)
                part = torch.full((n, rows, cin, 2), float("nan"), device=DEV)
                L.check(lib.mednet_conv3d_dgrad_gn(dyg.data_ptr(), pk.data_ptr(), addg.data_ptr() if with_add else None, dx.data_ptr(),
                                                   gyg.data_ptr(), coef.data_ptr(), act, part.data_ptr(), n, d, h, wd, cin, cout, L.ALGO_MFMA,
                                                   dcode, L.stream()), "dgrad_gn")
                torch.cuda.synchronize()
                what = f"dgrad_gn {name} {mode} {key} add={with_add} act={act}"
                stored = t["two"] if with_add else t["plain"]
                total += assert_exact(dx, stored, what + ": dx")
                check_gn_sums(part, stored, t["pre"], t["gy"], act, what)
    report_rounding("b", f"dgrad_add/dgrad_gn {key} {mode} one-vs-two={t['differ']}", f"plan kind {plan[0]}", total, census_counts(t["cen"]))


# ------------------------------------------------------------------------------------------------ (c) statistics of the stored values
# Sparse inputs: few outputs are nonzero, each of them a product that is no number of the storage type (bf16: {3, 5} x 129 / 127,
# fp16: {5, 7} x 513 / 511), so that sum |stored value| of a whole sample and channel pair stays below 2^24 lattice steps and the
# fp32 first moments are exact in any order
SPARSE_VALUES = {"bf16": (-5, -3, 3, 5), "fp16": (-7, -5, 5, 7)}
SPARSE_SIZE = {"bf16": 4 * 128.0, "fp16": 6 * 512.0}      # the mean size of one product
_SPARSE = {}


def sparse_case(n, cin, cout, shape, mode, gain=1):
    """The expected number of terms per output, t = 27 * C * p_x * p_w <= 1/2, is what keeps 2 * voxels * t * (size of a product) *
    gain -- the sum of |stored value| of a channel pair, times `gain` for the sums that carry a factor gn_y -- at 2^23; the weights
    are 16 times as dense as x and g, so that every channel pair has several of them."""
    key = (n, cin, cout, tuple(shape), mode, gain)
    if key not in _SPARSE:
        t = min(0.5, 2.0 ** 23 / (2.0 * shape[0] * shape[1] * shape[2] * SPARSE_SIZE[mode] * gain))
        p = (t / (27.0 * max(cin, cout) * 16.0)) ** 0.5
        tag = f"rsp{key}"
        x = lattice(tag + "x", n, cin, *shape, values=SPARSE_VALUES[mode], density=p)
        g = lattice(tag + "g", n, cout, *shape, values=SPARSE_VALUES[mode], density=p)
        w = lattice(tag + "w", cout, cin, 3, 3, 3, values=(-1, 1), density=min(0.5, 16.0 * p))
        mult = torch.where(torch.arange(cout) % 2 == 0, 2.0 ** M[mode] + 1, 2.0 ** M[mode] - 1).float()
        w = (w * mult.view(cout, 1, 1, 1, 1)).contiguous()
        xr = x.double().requires_grad_(True)
        y = F.conv3d(xr, w.double(), None, padding=1)
        y.backward(g.double())
        xa = x.abs().double().requires_grad_(True)
        ya = F.conv3d(xa, w.abs().double(), None, padding=1)
        ya.backward(g.abs().double())
        for t in (x, g, w):
            assert_representable(t, DT[mode], f"sparse {key} operand")
        assert_sums_exact(ya.detach(), f"sparse {key} y")
        assert_sums_exact(xa.grad, f"sparse {key} dx")
        _SPARSE[key] = dict(x=x, g=g, w=w, y=y.detach(), dx=xr.grad)
    return _SPARSE[key]


def pair_sums(t):
    """[n, c, ...] -> per (sample, channel pair) the fp64 sums {sum t, sum t^2} [n, c / 2, 2]."""
    t = t.double()
    n, ch = t.shape[:2]
    return torch.stack((t.sum((2, 3, 4)), (t * t).sum((2, 3, 4))), -1).reshape(n, ch // 2, 2, 2).sum(2)


def assert_sums_tell(stored, exact, what, per_pair=True, share=0.9):
    """The premise of (c): the sum of the rounded values differs from the sum of the unrounded ones in >= 90 % of the entries."""
    fold = (lambda t: pair_sums(t)[..., 0]) if per_pair else (lambda t: t.double().sum((2, 3, 4)))
    a, b = fold(stored), fold(exact)
    d = int((a != b).sum())
    assert d >= share * a.numel(), f"{what}: the sums of rounded and unrounded values differ in {d} of {a.numel()} entries only"
    return d


def fwd_stats_premises(y, dt, what):
    """-> per activation (stored values, their pair sums), after: sum |stored| per (sample, channel pair) < 2^24, the sums tell."""
    out = {}
    for act, fn in ((L.ACT_NONE, lambda t: t), (L.ACT_RELU, F.relu)):
        exact = fn(y)
        stored = exact.to(dt).double()
        assert torch.equal(stored, fn(y.to(dt).double())), "ReLU commutes with the rounding"
        m = float(pair_sums(stored.abs())[..., 0].max())
        assert m < 2.0 ** 24, f"{what}: sum |stored value| reaches {m:.4g} lattice steps >= 2^24 per (sample, channel pair)"
        assert_sums_tell(stored, exact, f"{what} act={act}")
        out[act] = (stored, pair_sums(stored))
    return out


def compare_stored_sums(partial, want, what):
    """The rows, added in fp64: first moments EQUAL to the sum of the stored values per (sample, channel pair); second moments within
    gpu_util.SUM_BOUND * sum y^2 of the fp64 sum of squares of the stored values (this half only bounds)."""
    p = partial.detach().double().cpu()
    assert not bool(torch.isnan(p).any()), f"{what}: a row of the partial buffer was not written"
    assert bool((p[:, :, 1::2] == 0).all()), f"{what}: odd entries of the pair format must be zero"
    tot = p.sum(1)[:, 0::2]
    total = assert_exact(tot[..., 0], want[..., 0], f"{what}: sum of the STORED values")
    bad = (tot[..., 1] - want[..., 1]).abs() > SUM_BOUND * want[..., 1]
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} second moments outside 2^-16 * sum y^2; first at {tuple(bad.nonzero()[0].tolist())}"
    return total + int(bad.numel())


FWD_STATS_CASES = [   # (n, cin, cout, shape, plan kinds, options)
    (2, 32, 32, (20, 24, 36), (2,), {}),                  # ragged bricks: one row per wave and brick
    (1, 16, 128, (32, 64, 64), (3,), {}),                 # general kernel, accumulate mode
    (2, 32, 32, (32, 60, 62), (4,), {}),                  # conv32: always accumulating
]


@pytest.mark.parametrize("mode", X.MODES16)
@pytest.mark.parametrize("n,cin,cout,shape,kinds,opts", FWD_STATS_CASES)
def test_fused_forward_sums_are_sums_of_the_stored_values(mode, n, cin, cout, shape, kinds, opts):
    """mednet_conv3d_act_fwd with gn_partial, activation none and ReLU, in per-brick rows and in accumulate mode: y is one rounding
    of the exact value and the rows add up EXACTLY to the sum of the ROUNDED outputs per sample and channel pair; the second
    moments are held to gpu_util's summation bound against the fp64 sum of squares of the stored values."""
    dt, dcode = DT[mode], X.dcode_of(mode)
    s = sparse_case(n, cin, cout, shape, mode)
    variants = fwd_stats_premises(s["y"], dt, f"fwd stats {n, cin, cout, shape} {mode}")
    cen = rounding_census(s["y"], dt)
    lib = L.lib()
    d, h, wd = shape
    xg = s["x"].to(DEV).to(dt).contiguous(memory_format=CL)
    total = 0
    with X.options(**opts):
        plan = X.stats_plan(n, shape, cin, cout, dcode)
        assert plan[0] in kinds, plan
        with mednet_hip.precision(mode):
            pk = ops.pack_conv_weight(s["w"].to(DEV), 3, False)
        rows = lib.mednet_conv3d_fused_stats_chunks(n, d, h, wd, cin, cout, 3, dcode, dcode, L.ALGO_MFMA)
        assert rows > 0
        for act, (stored, want) in variants.items():
            y = torch.full((n, cout, *shape), float("nan"), device=DEV).to(dt).contiguous(memory_format=CL)
            part = torch.full((n, rows, cout, 2), float("nan"), device=DEV)
            L.check(lib.mednet_conv3d_act_fwd(xg.data_ptr(), pk.data_ptr(), y.data_ptr(), n, d, h, wd, cin, cout, act, L.ALGO_MFMA,
                                              part.data_ptr(), dcode, L.stream()), "act_fwd")
            torch.cuda.synchronize()
            total += assert_exact(y, stored, f"act_fwd act={act} {mode}: y") + compare_stored_sums(part, want, f"act_fwd act={act} {mode} kind {plan[0]}")
    report_rounding("c", f"fwd sums {n, cin, cout, shape} {mode}", f"plan kind {plan[0]} accumulate={plan[6]}", total, census_counts(cen))


DGRAD_STATS_CASES = [(2, 32, 32, (9, 11, 21), (2, 3), dict(conv32=0, conv2b=0)), (2, 32, 32, (32, 60, 62), (4,), {})]


def dgrad_stats_premises(n, cin, cout, shape, mode):
    """-> inputs and per (add, activation) the stored dz, after the premises: sum |du| and sum |du * gn_y| per (sample, channel pair)
    below 2^24, the sums of rounded and unrounded gradients differ in >= 90 % of the (sample, channel) entries."""
    dt = DT[mode]
    s = sparse_case(n, cin, cout, shape, mode, gain=2)
    tag = f"rds{n, cin, cout, shape}"
    add = lattice(tag + "a", n, cin, *shape, values=(-3, -2, -1, 1, 2, 3), density=0.05)
    # |ca * gn_y| >= 2 > |cb|: the sign of the pre-activation follows gn_y, so a ReLU passes about half of every channel
    gy = lattice(tag + "y", n, cin, *shape, values=(-2, 2), density=1.0)
    ca = lattice(tag + "ca", n, cin, values=(-2, -1, 1, 2), density=1.0)
    cb = lattice(tag + "cb", n, cin, values=(-1.5, -0.5, 0.5, 1.5), density=1.0)
    pre = ca.double()[:, :, None, None, None] * gy.double() + cb.double()[:, :, None, None, None]
    assert float(pre.abs().min()) > 0
    variants = {}
    for with_add in (False, True):
        stored = (s["dx"].to(dt).double() + add.double()).to(dt).double() if with_add else s["dx"].to(dt).double()
        exact = s["dx"] + (add.double() if with_add else 0)
        for act in (L.ACT_NONE, L.ACT_RELU):
            du = X.gn_reference(stored, pre, act)
            X.check_sum_conditions(du, f"dgrad_gn sums {n, cin, cout, shape} {mode}", other=gy.double())
            assert_sums_tell(du, X.gn_reference(exact, pre, act), f"dgrad_gn sums {mode} add={with_add} act={act}", per_pair=False)
            variants[(with_add, act)] = (stored, du)
    return s, add, gy, torch.stack((ca, cb), -1).contiguous(), pre, variants


@pytest.mark.parametrize("mode", X.MODES16)
@pytest.mark.parametrize("n,cin,cout,shape,kinds,opts", DGRAD_STATS_CASES)
def test_fused_groupnorm_backward_sums_come_from_the_stored_gradient(mode, n, cin, cout, shape, kinds, opts):
    """mednet_conv3d_dgrad_gn (activation none and ReLU, power-of-two coefficients, add present / absent): dx is the stored
    gradient and the rows are {sum du, sum du * gn_y} of the STORED dx -- through gpu_util.check_gn_sums and, the sums being exact
    on this lattice, with equality in every entry."""
    dt, dcode = DT[mode], X.dcode_of(mode)
    s, add, gy, coef, pre, variants = dgrad_stats_premises(n, cin, cout, shape, mode)
    cen = rounding_census(s["dx"], dt)
    lib = L.lib()
    d, h, wd = shape
    dev = lambda a: a.to(DEV).to(dt).contiguous(memory_format=CL)
    dyg, addg, gyg, coefg = dev(s["g"]), dev(add), dev(gy), coef.to(DEV)
    total = 0
    with X.options(**opts):
        plan = X.stats_plan(n, shape, cout, cin, dcode, gnb=1)
        assert plan[0] in kinds, plan
        rows = lib.mednet_conv3d_dgrad_gn_rows_dt(n, d, h, wd, cin, cout, L.ALGO_MFMA, dcode)
        assert rows > 0
        with mednet_hip.precision(mode):
            pk = ops.pack_conv_weight(s["w"].to(DEV), 3, False)
        for (with_add, act), (stored, du) in variants.items():
            dx = torch.full((n, cin, *shape), float("nan"), device=DEV).to(dt).contiguous(memory_format=CL)
            part = torch.full((n, rows, cin, 2), float("nan"), device=DEV)
            L.check(lib.mednet_conv3d_dgrad_gn(dyg.data_ptr(), pk.data_ptr(), addg.data_ptr() if with_add else None, dx.data_ptr(),
                                               gyg.data_ptr(), coefg.data_ptr(), act, part.data_ptr(), n, d, h, wd, cin, cout, L.ALGO_MFMA,
                                               dcode, L.stream()), "dgrad_gn")
            torch.cuda.synchronize()
            what = f"dgrad_gn sums {mode} {n, cin, cout, shape} add={with_add} act={act}"
            total += assert_exact(dx, stored, what + ": dx")
            check_gn_sums(part, stored, pre, gy, act, what)
            total += X.compare_channel_sums(part, du, gy.double(), what)
    report_rounding("c", f"dgrad_gn sums {n, cin, cout, shape} {mode}", f"plan kind {plan[0]}", total, census_counts(cen))


# ------------------------------------------------------------------------------------------------ (d) fp16 edges
def overflow_exponent(v):
    """The smallest power of two that lifts at least 2 % of |v| to 65520 or beyond (what fp16 stores as +-inf)."""
    a = v.abs()
    for e in range(0, 15):
        if float((a * 2.0 ** e >= 65520).double().mean()) >= 0.02:
            return e
    raise AssertionError("no power of two up to 2^14 overflows 2 % of the reference")


def edge_variant(c, edge):
    """-> (the scaled case, premises of its outputs)."""
    if edge == "subnormal-out":     # x, w and g stay normal numbers; the results are those of the plain case times 2^-26
        return c.scaled(-13, -13, -13), dict(sub=1000, sub_ties=100)
    if edge == "tiny-out":          # ... times 2^-35: a single product lies below half the smallest subnormal, two lie above it
        return c.scaled(-13, -22, -13), dict(nonrep=0, ties=0, sub=1000, zeroed=100)
    if edge == "subnormal-x":       # x and g in {2^-16, 2^-15}; the results are the plain ones times 2^-10
        return c.scaled(-16, 6, -16), {}
    if edge == "subnormal-w":       # w = +-(2^9 +- 1) 2^-24
        return c.scaled(14, -24, 14), {}
    assert edge == "overflow"
    ref = c.ref()[0]
    return c.scaled(overflow_exponent(ref["y"]), 0, overflow_exponent(ref["dx"])), dict(inf=(0.01, 0.5))


def assert_subnormal_operands(v, edge):
    sub = lambda t: bool(((t == 0) | (t.abs() < F16_TINY)).all()) and bool((t != 0).any())
    normal = lambda t: bool(((t == 0) | (t.abs() >= F16_TINY)).all())
    if edge == "subnormal-x":
        assert sub(v.x) and sub(v.g) and normal(v.w)
    elif edge == "subnormal-w":
        assert sub(v.w) and normal(v.x) and normal(v.g)
    else:
        assert normal(v.x) and normal(v.g) and normal(v.w)
    if edge in ("subnormal-x", "subnormal-w"):
        for k, r in v.ref()[0].items():      # the results are normal numbers: >= 90 % of the nonzero ones
            live = r != 0
            assert float((r[live].abs() >= F16_TINY).double().mean()) >= 0.9, k


EDGES = ["subnormal-out", "tiny-out", "subnormal-x", "subnormal-w", "overflow"]


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("name,mode", EDGE_KERNELS)
def test_fp16_edges(name, mode, edge):
    """fp16, forward and data gradient: results below 2^-14 are stored as subnormals (`subnormal-out`: ties to even in both
    directions; `tiny-out`: below half the smallest one a zero of their sign) -- loss-scaled gradients live there; subnormal activations, gradients and weights enter the products with
    their value (the low weight images of fp16x2 are mostly subnormal); a result of 65520 or more is stored as +-inf and never as
    65504 or NaN -- the loss scaler backs off on a non-finite gradient only."""
    base = kernel_case(name, mode)
    base.premises(mode)                       # (the plain case holds no element >= 65520)
    c, minima = edge_variant(base, edge)
    assert_subnormal_operands(c, edge)
    cens = c.premises(mode, **minima)
    kernel, got = run_kernel(name, c, mode)
    for k in ("y", "dx"):
        assert not bool(torch.isnan(got[k]).any()), f"{name} {edge}: NaN in {k}"
    total, counts = compare_rounded(c, got, mode, cens, f"{name} {mode} {edge} {c}")
    report_rounding("d", f"{edge} {c} {mode}", kernel, total, counts)


# ------------------------------------------------------------------------------------------------ (e) joins of csrc/norm_act.hip
TOP = {"bf16": (-255, -201, -131, 130, 203, 251), "fp16": (-2047, -1531, -1025, 1027, 1533, 2045)}   # integers with full significands
BIG = {"bf16": 2.0 ** 8, "fp16": 2.0 ** 11}      # from here on the odd integers are no numbers of the type
SMALL_JOIN = dict(nonrep=0.25, ties=10)          # (a few hundred elements per case: ties in both directions, fewer of them)
# (test_pool2's average-pooling sizes, one even and one odd; a max pooling's backward leaves 7 of 8 voxels equal to `add` alone)
POOL_CASES = [(16, (6, 6, 6), "avg"), (5, (5, 7, 6), "avg")]
UPCAT_CASES = [(8, 16, (8, 12, 10), (4, 6, 5)), (8, 16, (7, 9, 10), (3, 4, 5))]                                  # (test_upsample_concat's)


def pool_case(mode, c, shape, kind):
    """Inputs whose fp32 sums are exact and whose results are no numbers of the storage type -> x, g, add, a and the exact
    results {"pool2_fwd" (the mean of 8; average pooling only), "pool2_bwd+add", "add"} with their censuses, premises asserted."""
    n, dt = 2, DT[mode]
    tag = f"rp{c}{shape}{mode}"
    x = lattice(tag + "x", n, c, *shape, values=TOP[mode], density=0.9)
    g = lattice(tag + "g", n, c, *(s // 2 for s in shape), values=(-24, -16, -8, 8, 16, 24), density=0.9) * BIG[mode]      # g / 8 = k * BIG
    add = lattice(tag + "a", n, c, *shape, values=(-7, -5, -3, -2, -1, 1, 2, 3, 5, 7), density=0.9)
    a = lattice(tag + "b", n, c, *shape, values=(-3, -2, -1, 1, 2, 3), density=0.9) * BIG[mode]
    for t in (x, g, add, a):
        assert_representable(t, dt, "pool operand")
    xr = x.double().requires_grad_(True)
    yr = (F.max_pool3d if kind == "max" else F.avg_pool3d)(xr, 2)
    yr.backward(g.double())
    want = {"pool2_bwd+add": xr.grad + add.double(), "add": a.double() + add.double()}
    if kind == "avg":
        want["pool2_fwd"] = yr.detach()
    cens = {k: assert_rounding_premises(v, dt, f"{k} {kind} {c, shape} {mode}", **SMALL_JOIN) for k, v in want.items()}
    return dict(x=x, g=g, add=add, a=a, want=want, cens=cens)


def upcat_case(mode, ce, cx, eshape, xshape):
    n, dt = 2, DT[mode]
    tag = f"ru{ce}{cx}{eshape}{mode}"
    e = lattice(tag + "e", n, ce, *eshape, density=0.6)
    x = lattice(tag + "x", n, cx, *xshape, density=0.6)
    g = lattice(tag + "g", n, ce + cx, *eshape, values=TOP[mode], density=0.9)
    assert_representable(g, dt, "upcat operand")
    er, xr = e.double().requires_grad_(True), x.double().requires_grad_(True)
    torch.cat((er, F.interpolate(xr, size=eshape, mode="nearest")), dim=1).backward(g.double())
    cen = assert_rounding_premises(xr.grad, dt, f"upcat_bwd {ce, cx, eshape} {mode}", **SMALL_JOIN)
    return dict(e=e, x=x, g=g, dx=xr.grad, denc=er.grad, cen=cen)


@pytest.mark.parametrize("mode", X.MODES16)
@pytest.mark.parametrize("c,shape,kind", POOL_CASES)
def test_pooling_and_add_round_once(mode, c, shape, kind):
    """mednet_add, mednet_pool2_fwd (the mean of 8) and mednet_pool2_bwd with `add`: fp32 arithmetic and ONE rounding at the store,
    on inputs whose fp32 sums are exact and whose results are no numbers of the storage type."""
    n, dt, dcode = 2, DT[mode], X.dcode_of(mode)
    t = pool_case(mode, c, shape, kind)
    lib, got = L.lib(), {}
    dev = lambda a: a.to(DEV).to(dt).contiguous(memory_format=CL)
    if kind == "avg":
        with mednet_hip.precision(mode):
            got["pool2_fwd"] = ops.pool2(dev(t["x"]), L.POOL_AVG)
    dx = torch.full((n, c, *shape), float("nan"), device=DEV).to(dt).contiguous(memory_format=CL)
    gg, xx, aa, ag = dev(t["g"]), dev(t["x"]), dev(t["add"]), dev(t["a"])
    L.check(lib.mednet_pool2_bwd(gg.data_ptr(), xx.data_ptr(), aa.data_ptr(), dx.data_ptr(), n, *shape, c,
                                 L.POOL_MAX if kind == "max" else L.POOL_AVG, dcode, L.stream()), "pool2_bwd")
    out = torch.full_like(aa, float("nan"))
    L.check(lib.mednet_add(ag.data_ptr(), aa.data_ptr(), out.data_ptr(), ag.numel(), dcode, L.stream()), "add")
    torch.cuda.synchronize()
    got["pool2_bwd+add"], got["add"] = dx, out
    total, counts = 0, {}
    for k, v in t["want"].items():
        total += assert_rounded(got[k], v, dt, f"{k} {kind} {mode}")
        add_counts(counts, census_counts(t["cens"][k]))
    report_rounding("e", f"pool2 {kind} {c, shape} {mode}", ", ".join(t["want"]), total, counts)


@pytest.mark.parametrize("mode", X.MODES16)
@pytest.mark.parametrize("ce,cx,eshape,xshape", UPCAT_CASES)
def test_upsample_concat_backward_rounds_once(mode, ce, cx, eshape, xshape):
    """mednet_upcat_bwd: the gradient of the upsampled half is the sum of (up to) 8 gradients, added in fp32 and rounded once."""
    dt = DT[mode]
    t = upcat_case(mode, ce, cx, eshape, xshape)
    with mednet_hip.precision(mode):
        eg, xg = t["e"].to(DEV).to(dt).requires_grad_(True), t["x"].to(DEV).to(dt).requires_grad_(True)
        ops.upsample_concat(eg, xg).backward(t["g"].to(DEV).to(dt))
        torch.cuda.synchronize()
    total = assert_rounded(xg.grad, t["dx"], dt, f"upcat_bwd {mode}: dx") + assert_exact(eg.grad, t["denc"], f"upcat_bwd {mode}: denc")
    report_rounding("e", f"upcat {ce, cx, eshape} {mode}", "upcat_bwd", total, census_counts(t["cen"]))
