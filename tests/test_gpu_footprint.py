"""Footprint tests: where do the kernels read and write?  Every operator runs inside tests/fence.py's Fence -- each input, output,
partial buffer and workspace in a slab of its own between two guard bands, the workspaces EXACTLY as large as the library's
own query says -- then its existing exact result check is made (a NaN or an impossible label that leaked in from outside a
tensor fails by value), then fence.check() compares every guard byte with the pattern.  Where the existing check of an
operator is a bound, the fenced run must equal the same call made outside the fence bit for bit (the kernels are deterministic
and the fence keeps the alignment).  No tolerance of its own anywhere.

The cases, references and checkers are those of test_gpu_exact.py, test_gpu_exact_norm.py, test_gpu_head_backward.py,
test_gpu_losses.py and test_gpu_vis.py, at their smallest shapes that reach the edge in question (a ragged last brick, a count that
is no multiple of the vector width, a second workgroup, a row count above one).  Where those modules allocate through helpers of
their own (vol / nan_vol / nan_f32 / workspace, nan_like / to_dev_cl), the helpers are pointed at the fence and the module's own
runner is called.  Every test ends in `finish`: fence.owns for what the operator returned, a served workspace where the operator
has one, fence.check(), and one line

    [footprint] entry=<what ran> allocations=<fenced slabs> ws_requests=<n> ws_bytes_asked=<sum> ws_bytes_served=<sum> largest_payload=<bytes> result=clean calls=<entry points of the C ABI called inside the fence>

(pytest -s / -rP shows them; profiles/footprint_audit.md keeps those of the MI355X run).
"""
import contextlib
import ctypes
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mednet_hip
from mednet_hip import _lib as L
from mednet_hip import nn as hnn
from mednet_hip import ops, vis
from mednet_hip.unet import model as HM
from oracle import ref_cpu as O

import gpu_util as U
import test_gpu_exact as E
import test_gpu_exact_norm as N
import test_gpu_head_backward as H
import test_gpu_losses as LS
import test_gpu_multichannel_exact as MC
import test_gpu_vis as V
from fence import Fence as _Fence
from gpu_util import DEV, assert_exact, assert_representable, lattice

pytestmark = pytest.mark.gpu
CL = torch.channels_last_3d
DT = E.DT
KIB = 1024


# ------------------------------------------------------------------------------------------------ helpers
class _Recorder:
    """Stands where the ctypes handle stands and notes which entry points of the C ABI were looked up (= called)."""

    def __init__(self, lib):
        self._lib, self.names = lib, set()

    def __getattr__(self, name):
        if name.startswith("mednet_"):
            self.names.add(name)
        return getattr(self._lib, name)


_CALLS = [None]


@pytest.fixture(autouse=True)
def abi_calls(monkeypatch):
    _CALLS[0] = _Recorder(L.lib())
    monkeypatch.setattr(L, "_lib", _CALLS[0])
    yield
    _CALLS[0] = None


class Fence(_Fence):
    """tests/fence.py's Fence; the audit line of a test lists the entry points called while it was open."""

    def __enter__(self):
        _CALLS[0].names.clear()
        return super().__enter__()


def itemsize(dt):
    return torch.empty((), dtype=dt, device="meta").element_size()


def guard_for(*planes):
    """256 KiB, doubled until it exceeds one z-plane (h * w * c * itemsize bytes) of every tensor of the case."""
    g = 256 * KIB
    while g <= max(planes, default=0):
        g *= 2
    return g


def plane(shape, c, dt):
    return shape[-2] * shape[-1] * c * itemsize(dt)


def dev(fence, t, dt=None, cl=True):
    """A CPU tensor as the library wants it (storage type, activations channels-last), in a slab."""
    if t is None:
        return None
    t = t.to(DEV)
    if dt is not None:
        t = t.to(dt)
    if cl and t.dim() == 5:
        t = t.contiguous(memory_format=CL)
    return fence.put(t)


def layer_put(fence):
    def put(t, cl):
        return fence.put(t.contiguous(memory_format=CL) if cl and t.dim() == 5 else t)
    return put


def factories_in(fence, m, made):
    """torch.zeros / torch.full / torch.tensor for the fence's device (the counters, scalars and zeroed buffers the runners of the
    other modules make inline) give fenced tensors too: nothing a kernel writes or reads lies outside a slab."""
    def wrap(orig):
        def factory(*a, **kw):
            r = orig(*a, **kw)
            if torch.is_tensor(r) and r.device.type == fence.device.type and not fence.owns(r):
                r = fence.put(r)
                made.append(r)
            return r
        return factory
    for name in ("zeros", "full", "tensor"):
        m.setattr(torch, name, wrap(getattr(torch, name)))


def finish(fence, entry, outputs=(), ws=None, sites=()):
    """The end of every test: ownership of the outputs, the workspace requests, the guards, the audit line."""
    for t in outputs:
        assert t is None or fence.owns(t), f"{entry}: an output of shape {tuple(t.shape)} was not allocated inside the fence"
    seen = {s.site for s in fence.slabs}
    assert set(sites) <= seen, f"{entry}: no fenced allocation from {sorted(set(sites) - seen)} (sites seen: {sorted(seen)})"
    s = fence.summary()
    if ws is not None:
        assert (s["ws_requests"] > 0) == ws, f"{entry}: {s['ws_requests']} workspace requests went through the fence"
    assert s["ws_asked"] == s["ws_served"], f"{entry}: {s['ws_served']} workspace bytes served for {s['ws_asked']} asked"
    assert s["allocations"] > 0
    fence.check()
    print(f"[footprint] entry={entry} allocations={s['allocations']} ws_requests={s['ws_requests']} ws_bytes_asked={s['ws_asked']} "
          f"ws_bytes_served={s['ws_served']} largest_payload={s['largest_payload']} result=clean calls={','.join(sorted(_CALLS[0].names))}")


def fenced_layer(c, mode, algo, entry, guard=None):
    """A test_gpu_exact case through hnn.Conv3d / hnn.ConvTranspose3d inside a fence: forward, data, weight and bias gradient, the
    weights packed inside the fence too (ops.pack_conv_weight: a buffer of exactly mednet_conv3d_pack_bytes)."""
    c.check_conditions(mode)
    dt = DT[mode]
    g = guard or guard_for(plane(c.oshape, c.cout, dt), plane(c.shape, c.cin, torch.float32 if c.cin == 1 else dt))
    with Fence(guard=g) as fence:
        got = E.run_layer(c, mode, algo, put=layer_put(fence))
        total = E.compare_layer(c, got, entry)
        pack = [s for s in fence.slabs if s.site == "pack_conv_weight"]
        assert len(pack) == 1 and pack[0].nbytes == L.lib().mednet_conv3d_pack_bytes(c.cin, c.cout, 3)
        finish(fence, entry, ws=True, sites=("empty_cl", "pack_conv_weight", "_grad_target", "put"))
    return total


# ================================================================================================ (a) the conv family
@pytest.mark.parametrize("mode", E.ALL_MODES)
@pytest.mark.parametrize("n,cin,cout,shape", [(2, 3, 5, (4, 6, 7)), (1, 8, 16, (5, 7, 9))])
def test_direct_kernels(mode, n, cin, cout, shape):
    c = E.case("conv", n, cin, cout, shape, bias=True)
    assert L.lib().mednet_conv3d_act_supported(n, *shape, cin, cout, L.ALGO_DIRECT) == 0
    fenced_layer(c, mode, "direct", f"conv3d fwd/dgrad/wgrad/bias direct {c} {mode}")


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp16x2"])
@pytest.mark.parametrize("n,cin,cout,shape", [(2, 32, 32, (9, 11, 21)), (1, 16, 16, (5, 9, 17)), (1, 48, 80, (4, 8, 16))])
def test_general_matrix_core_kernel(mode, n, cin, cout, shape):
    c = E.case("conv", n, cin, cout, shape)
    with E.options(conv32=0, conv2b=0, conv2b_split=0):
        for a, b in ((cin, cout), (cout, cin)):
            assert E.stats_plan(n, shape, a, b, E.dcode_of(mode), split=mode == "fp16x2")[0] in (2, 3)
        fenced_layer(c, mode, "mfma", f"conv3d fwd/dgrad/wgrad conv_mfma_kernel {c} {mode}")


@pytest.mark.parametrize("mode", E.MODES16)
def test_conv32_specialisation(mode):
    n, shape = E.CONV32_CASES[0]
    c = E.case("conv", n, 32, 32, shape)
    assert E.stats_plan(n, shape, 32, 32, E.dcode_of(mode))[0] == 4
    fenced_layer(c, mode, "mfma", f"conv3d fwd/dgrad conv32_mfma_kernel {c} {mode}")


@pytest.mark.parametrize("mode", E.MODES16)
def test_two_block_kernel(mode):
    n, cin, cout, shape = E.CONV2B_CASES[0]
    c = E.case("conv", n, cin, cout, shape)
    with E.options(conv2b_min_fill=0, conv2b_min_cin=16):
        assert E.stats_plan(n, shape, cin, cout, E.dcode_of(mode))[0] in (5, 6)
        assert E.stats_plan(n, shape, cout, cin, E.dcode_of(mode))[0] in (5, 6)
        fenced_layer(c, mode, "mfma", f"conv3d fwd/dgrad conv2b_mfma_kernel {c} {mode}")


@pytest.mark.parametrize("x3", [1, 0])
def test_fp32_mode_families(x3):
    n, cin, cout, shape = 1, 48, 16, (5, 6, 7)
    c = E.case("conv", n, cin, cout, shape)
    with E.options(x3=x3):
        assert E.x3_family_takes(n, cin, cout, shape) == bool(x3)
        fenced_layer(c, "fp32", "auto", f"conv3d fwd/dgrad/wgrad {'split-bf16' if x3 else 'fp32-mfma'} {c} fp32")


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp16x2"])
@pytest.mark.parametrize("n,cin,cout,shape,layout", [(2, 1, 32, (9, 11, 21), "planar"), (1, 1, 64, (5, 6, 7), "planar")]
                         + [(n, cin, cout, shape, layout) for n, cin, cout, shape in ((2, 2, 32, (9, 11, 21)), (1, 3, 64, (5, 6, 7)), (2, 4, 32, (9, 11, 21)))
                            for layout in ("planar", "channels_last")])
def test_first_layer_kernels(mode, n, cin, cout, shape, layout):
    """The fp32 network input with 1 to 4 channels, planar and channels-last, where it lies: y, the fused GroupNorm rows (a buffer
    sized by mednet_conv3d_fused_stats_chunks) and the weight gradient in its matrix-core and its VALU form."""
    c = E.case("conv", n, cin, cout, shape)
    c.check_conditions(mode)
    ref = c.ref()[0]
    lib, dt = L.lib(), DT[mode]
    rows = lib.mednet_conv3d_fused_stats_chunks(n, *shape, cin, cout, 3, L.F32, L.dt_of(dt), MC.algo_of(mode))
    assert rows > 0, "the first-layer matrix-core kernel does not take this call"
    if cin > 1:
        assert lib.mednet_conv3d_cm_supported(cin, cout, 3, L.F32, L.dt_of(dt), MC.algo_of(mode)) == 1
    E.check_sum_conditions(ref["y"], f"{c}")
    for c1 in (1, 0):
        with MC.options(wgrad_c1_mfma=c1), mednet_hip.precision(mode), Fence() as fence:
            conv = hnn.Conv3d(cin, cout, 3, bias=False).to(DEV)
            with torch.no_grad():
                conv.weight.copy_(c.w)
                conv.weight.data = fence.put(conv.weight.data)
            xg = c.x.to(DEV)
            if layout == "channels_last":
                xg = xg.contiguous(memory_format=CL)
                assert not xg.is_contiguous()
            y, partial = conv.forward_with_stats(fence.put(xg))
            assert partial is not None and tuple(partial.shape) == (n, rows, cout, 2)
            y.backward(dev(fence, c.g, dt))
            torch.cuda.synchronize()
            assert_exact(y, ref["y"], f"first layer {layout} {mode} {c}: y")
            assert_exact(conv.weight.grad, ref["dw"], f"first layer {layout} wgrad mfma={c1} {c}: dw")
            E.compare_pair_sums(partial, ref["y"], f"first layer {layout} {mode} {c}")
            finish(fence, f"conv3d first layer fwd+stats/wgrad(mfma={c1}) {layout} {c} {mode}", outputs=(y, partial), ws=True,
                   sites=("pack_conv_weight", "_grad_target"))


@pytest.mark.parametrize("mode,algo,kw", [("bf16", "mfma", dict(n=2, cin=64, cout=32, shape=(3, 5, 9))), ("fp16", "mfma", dict(n=2, cin=64, cout=32, shape=(3, 5, 9))),
                                          ("bf16", "mfma", dict(n=1, cin=32, cout=32, shape=(5, 9, 17))),
                                          ("bf16", "direct", dict(n=2, cin=16, cout=8, shape=(3, 5, 4))), ("fp32", "direct", dict(n=2, cin=16, cout=8, shape=(3, 5, 4))),
                                          ("fp32", "auto", dict(n=2, cin=32, cout=16, shape=(3, 5, 9)))])
def test_conv_transpose(mode, algo, kw):
    """ConvTranspose3d with bias and skip: the matrix-core kernels, the direct ones and the fp32 mode's, on the smallest ragged case
    of each list of test_gpu_exact.py."""
    c = E.case("convt", kw["n"], kw["cin"], kw["cout"], kw["shape"], bias=True, skip=True)
    if algo == "mfma":
        assert L.lib().mednet_convt3d_dgrad_gn_rows(c.n, *c.shape, c.cin, c.cout, E.dcode_of(mode), L.ALGO_MFMA) > 0
    fenced_layer(c, mode, algo, f"convt3d fwd+skip/dgrad/wgrad/bias {algo} {c} {mode}")


@pytest.mark.parametrize("mode", E.MODES16)
def test_conv_transpose_dgrad32(mode):
    n, cin, cout, shape = E.CONVT32_CASE
    c = E.case("convt", n, cin, cout, shape, bias=True, skip=True)
    assert E.stats_plan(n, shape, cin, cout, E.dcode_of(mode), gnb=1, stride=2)[0] == 7
    fenced_layer(c, mode, "mfma", f"convt3d convt_dgrad32_mfma_kernel {c} {mode}")


@pytest.mark.parametrize("mode", E.MODES16)
@pytest.mark.parametrize("n,cin,cout,shape,px,pw,kinds,opts", E.ACT_FWD_CASES)
def test_fused_forward_epilogues(mode, n, cin, cout, shape, px, pw, kinds, opts):
    """mednet_conv3d_act_fwd with its GroupNorm rows: the partial buffer has exactly the rows mednet_conv3d_fused_stats_chunks
    answers, in a slab of its own."""
    dt, dcode = DT[mode], E.dcode_of(mode)
    x, w, yr = E.act_fwd_conditions(n, cin, cout, shape, px, pw, dt)
    lib = L.lib()
    d, h, wd = shape
    with E.options(**opts), Fence(guard=guard_for(plane(shape, cout, dt), plane(shape, cin, dt))) as fence:
        plan = E.stats_plan(n, shape, cin, cout, dcode)
        assert plan[0] in kinds, plan
        xg = dev(fence, x, dt)
        with mednet_hip.precision(mode):
            pk = ops.pack_conv_weight(fence.put(w.to(DEV)), 3, False)
        rows = lib.mednet_conv3d_fused_stats_chunks(n, d, h, wd, cin, cout, 3, dcode, dcode, L.ALGO_MFMA)
        assert rows > 0
        for act, fn, stats in ((L.ACT_NONE, lambda t: t, True), (L.ACT_RELU, F.relu, True), (L.ACT_RELU, F.relu, False)):
            y = fence.alloc((n, cout, *shape), dt, memory_format=CL)
            part = fence.alloc((n, rows, cout, 2), torch.float32) if stats else None
            L.check(lib.mednet_conv3d_act_fwd(xg.data_ptr(), pk.data_ptr(), y.data_ptr(), n, d, h, wd, cin, cout, act, L.ALGO_MFMA,
                                              L.ptr(part), dcode, L.stream()), "act_fwd")
            torch.cuda.synchronize()
            assert_exact(y, fn(yr), f"act_fwd act={act} stats={stats} {mode}: y")
            if stats:
                assert bool((part[:, :, 1::2] == 0).all()), "odd entries of the pair format must be zero"
                E.compare_pair_sums(part, fn(yr), f"act_fwd act={act} {mode} kind {plan[0]}")
        finish(fence, f"conv3d_act_fwd+stats plan kind {plan[0]} rows={rows} {n, cin, cout, shape} {mode}", outputs=(pk,), ws=False)


@pytest.mark.parametrize("mode,n,cin,cout,shape,kinds,opts", E.DGRAD_CASES)
def test_fused_data_gradient_epilogues(mode, n, cin, cout, shape, kinds, opts):
    """mednet_conv3d_dgrad_add and mednet_conv3d_dgrad_gn (add present and absent, activation none / ReLU / ELU): the row buffer has
    exactly mednet_conv3d_dgrad_gn_rows_dt rows."""
    key = (n, cin, cout, shape)
    dt, dcode = DT[mode], E.dcode_of(mode)
    t, gy64, variants = E.dgrad_conditions(key, dt)
    lib = L.lib()
    d, h, wd = shape
    algo = L.ALGO_AUTO if mode == "fp32" else L.ALGO_MFMA
    with E.options(**opts), Fence(guard=guard_for(plane(shape, max(cin, cout), dt))) as fence:
        if kinds is not None:
            assert E.stats_plan(n, shape, cout, cin, dcode, gnb=1)[0] in kinds
        assert lib.mednet_conv3d_dgrad_add_supported(n, d, h, wd, cin, cout, algo, dcode) == 1
        rows = lib.mednet_conv3d_dgrad_gn_rows_dt(n, d, h, wd, cin, cout, algo, dcode)
        assert rows > 0
        dyg, addg, gyg = dev(fence, t["dy"], dt), dev(fence, t["add"], dt), dev(fence, t["gy"], dt)
        coef, coef_elu = fence.put(t["coef"].to(DEV)), fence.put(t["coef_elu"].to(DEV))
        with mednet_hip.precision(mode):
            pk = ops.pack_conv_weight(fence.put(t["w"].to(DEV)), 3, False)
        dx = fence.alloc((n, cin, *shape), dt, memory_format=CL)
        L.check(lib.mednet_conv3d_dgrad_add(dyg.data_ptr(), pk.data_ptr(), addg.data_ptr(), dx.data_ptr(), n, d, h, wd, cin, cout, algo,
                                            dcode, L.stream()), "dgrad_add")
        torch.cuda.synchronize()
        assert_exact(dx, variants[(True, 0)][0], f"dgrad_add {mode} {key}: dx")
        for (with_add, act), (dx_ref, du_ref) in variants.items():
            dx = fence.alloc((n, cin, *shape), dt, memory_format=CL)
            part = fence.alloc((n, rows, cin, 2), torch.float32)
            L.check(lib.mednet_conv3d_dgrad_gn(dyg.data_ptr(), pk.data_ptr(), addg.data_ptr() if with_add else None, dx.data_ptr(),
                                               gyg.data_ptr(), (coef_elu if act == L.ACT_ELU else coef).data_ptr(), act, part.data_ptr(), n, d, h, wd,
                                               cin, cout, algo, dcode, L.stream()), "dgrad_gn")
            torch.cuda.synchronize()
            what = f"dgrad_gn {mode} {key} add={with_add} act={act}"
            assert_exact(dx, dx_ref, what + ": dx")
            E.compare_channel_sums(part, du_ref, gy64, what)
        finish(fence, f"conv3d_dgrad_add/_gn rows={rows} {key} {mode}", outputs=(pk,), ws=False)


@pytest.mark.parametrize("mode", E.MODES16)
@pytest.mark.parametrize("n,cin,cout,shape,kind", E.CONVT_GN_CASES)
def test_conv_transpose_data_gradient_with_groupnorm_sums(mode, n, cin, cout, shape, kind):
    """mednet_convt3d_dgrad_gn (conv_mfma_kernel<2> and convt_dgrad32_mfma_kernel): the row buffer has exactly
    mednet_convt3d_dgrad_gn_rows rows."""
    dt, dcode = DT[mode], E.dcode_of(mode)
    lib = L.lib()
    d, h, w = shape
    c, gy, dx_ref, refs = E.convt_gn_inputs(n, cin, cout, shape, mode)
    assert E.stats_plan(n, shape, cin, cout, dcode, gnb=1, stride=2)[0] == kind
    rows = lib.mednet_convt3d_dgrad_gn_rows(n, d, h, w, cin, cout, dcode, L.ALGO_MFMA)
    assert rows > 0
    with Fence(guard=guard_for(plane(c.oshape, cout, dt), plane(shape, cin, dt))) as fence:
        with mednet_hip.precision(mode):
            pk = ops.pack_conv_weight(fence.put(c.w.to(DEV)), 3, True)
        dyg, gyg = dev(fence, c.g, dt), dev(fence, gy, dt)
        outs = [pk]
        for act in E.GN_ACTS:
            gz, du = refs[act]
            gzg = dev(fence, gz, dt)
            dx, part = fence.alloc((n, cin, *shape), dt, memory_format=CL), fence.alloc((n, rows, cin, 2), torch.float32)
            L.check(lib.mednet_convt3d_dgrad_gn(dyg.data_ptr(), pk.data_ptr(), dx.data_ptr(), gyg.data_ptr(), gzg.data_ptr(), act, part.data_ptr(),
                                                n, d, h, w, cin, cout, dcode, L.ALGO_MFMA, L.stream()), "convt3d_dgrad_gn")
            torch.cuda.synchronize()
            assert_exact(dx, dx_ref, f"convt3d_dgrad_gn {mode} act={act}: dx")
            E.compare_channel_sums(part, du, gy.double(), f"convt3d_dgrad_gn {mode} act={act}")
            outs += [dx, part]
        finish(fence, f"convt3d_dgrad_gn plan kind {kind} rows={rows} {n, cin, cout, shape} {mode}", outputs=outs, ws=False)


@pytest.mark.parametrize("mode", E.MODES16)
@pytest.mark.parametrize("v4", [1, 0])
@pytest.mark.parametrize("n,cin,cout,shape,wgs", [E.WGRAD_CASES[4], E.WGRAD_CASES[1]])
def test_weight_gradient_kernels(mode, v4, n, cin, cout, shape, wgs):
    """mednet_conv3d_wgrad through the C ABI with a workspace of exactly mednet_conv3d_wgrad_ws_bytes -- 24 workgroups, which do not
    divide the items, and the library's own count on a ragged volume."""
    c = E.case("conv", n, cin, cout, shape)
    c.check_conditions(mode)
    lib, dt, code = L.lib(), DT[mode], E.dcode_of(mode)
    d, h, w = shape
    with E.options(wgrad_v4=v4), Fence(guard=guard_for(plane(shape, max(cin, cout), dt))) as fence:
        want = 4 if (v4 and d >= 8 and h >= 8 and w >= 16) else 2
        assert E.wgrad_plan(n, shape, cin, cout, code, wgs)[0] == want
        xg, dyg = dev(fence, c.x, dt), dev(fence, c.g, dt)
        ws = fence.workspace(lib.mednet_conv3d_wgrad_ws_bytes(n, d, h, w, cin, cout, 3, wgs))
        dw, db = fence.alloc((cout, cin, 3, 3, 3), torch.float32), fence.alloc((cout,), torch.float32)
        L.check(lib.mednet_conv3d_wgrad(xg.data_ptr(), dyg.data_ptr(), dw.data_ptr(), db.data_ptr(), n, d, h, w, cin, cout, 3, code,
                                        L.NDHWC, code, L.NDHWC, L.ALGO_MFMA, wgs, ws.data_ptr(), ws.numel(), L.stream()), "conv3d_wgrad")
        torch.cuda.synchronize()
        assert_exact(dw, c.ref()[0]["dw"], f"wgrad_mfma{want} {mode} {c} wgs={wgs}: dw")
        U.assert_sums_exact(c.g.abs().double().sum((0, 2, 3, 4)), "db")
        assert_exact(db, c.g.double().sum((0, 2, 3, 4)), "db")
        finish(fence, f"conv3d_wgrad wgrad_mfma{want}_kernel workgroups={wgs} {c} {mode}", outputs=(dw, db, ws), ws=True)


# ================================================================================================ (b) weight packing
PACK_CHANNELS = [(1, 16), (3, 5), (5, 3), (16, 1), (16, 48), (48, 80), (80, 16)]
PACK_LAYERS = [(cin, cout, False) for cin, cout in PACK_CHANNELS] + [(cin, cout, True) for cin, cout in PACK_CHANNELS if 1 not in (cin, cout)]


@pytest.mark.parametrize("mode", E.ALL_MODES)
@pytest.mark.parametrize("cin,cout,transposed", PACK_LAYERS)
def test_packed_weights_3x3x3(cin, cout, transposed, mode):
    """ops.pack_conv_weight (mednet_conv3d_pack_elt with the mode's element type) into a buffer of exactly mednet_conv3d_pack_bytes,
    then the layer's forward and gradients from that buffer, exact."""
    kw = dict(bias=True, skip=True) if transposed else {}
    c = E.case("convt" if transposed else "conv", 1, cin, cout, (3, 4, 5), **kw)
    fenced_layer(c, mode, "auto", f"conv3d_pack_elt + layer {c} {mode}")


@pytest.mark.parametrize("mode", E.ALL_MODES)
@pytest.mark.parametrize("cin,cout", [(1, 3), (5, 16), (48, 5), (80, 80)])
def test_packed_weights_1x1x1(cin, cout, mode):
    dt = DT[mode]
    n, shape = 2, (3, 5, 7)
    tag = f"fp1{cin, cout}"
    x = lattice(tag + "x", n, cin, *shape, density=0.5)
    w = lattice(tag + "w", cout, cin, 1, 1, 1, values=(-2, -1, 1, 2), density=0.5)
    yr = F.conv3d(x.double(), w.double())
    assert_representable(yr, dt, "1x1x1 y")
    U.assert_sums_exact(F.conv3d(x.abs().double(), w.abs().double()), "1x1x1 y")
    with mednet_hip.precision(mode), Fence() as fence:
        conv = hnn.Conv3d(cin, cout, 1, bias=False).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(w)
            conv.weight.data = fence.put(conv.weight.data)
        y = conv(dev(fence, x, torch.float32 if cin == 1 else dt))
        torch.cuda.synchronize()
        assert_exact(y, yr, f"1x1x1 {cin}->{cout} {mode}")
        pack = [s for s in fence.slabs if s.site == "pack_conv_weight"]
        assert len(pack) == 1 and pack[0].nbytes == L.lib().mednet_conv3d_pack_bytes(cin, cout, 1)
        finish(fence, f"conv3d_pack_elt k=1 + forward {cin}->{cout} {mode}", outputs=(y,))


class _PackJob(ctypes.Structure):
    _fields_ = [("w", ctypes.c_void_p), ("packed", ctypes.c_void_p), ("cin", ctypes.c_int), ("cout", ctypes.c_int), ("ksize", ctypes.c_int),
                ("transposed_src", ctypes.c_int)]


@pytest.mark.parametrize("mode", E.ALL_MODES)
def test_pack_many_writes_what_pack_elt_writes(mode):
    """mednet_conv3d_pack_table / _pack_many over four layers (transposed ones included) into buffers of exactly
    mednet_conv3d_pack_bytes: every byte equals the single-layer pack; with MEDNET_PACK_HIGH_ONLY on top of a full pack as well."""
    lib = L.lib()
    layers = [(16, 48, False), (48, 80, False), (80, 16, True), (16, 16, True)]
    with mednet_hip.precision(mode), Fence() as fence:
        elt = mednet_hip.config.pack_elt()
        ws_, singles, many = [], [], []
        for cin, cout, tr in layers:
            w = fence.put(U.rnd(f"fpm{cin, cout, tr}", *((cin, cout) if tr else (cout, cin)), 3, 3, 3).to(DEV))
            ws_.append(w)
            singles.append(ops.pack_conv_weight(w, 3, tr))
            many.append(fence.alloc((lib.mednet_conv3d_pack_bytes(cin, cout, 3),), torch.uint8))
        jobs = (_PackJob * len(layers))()
        for j, (cin, cout, tr), w, buf in zip(jobs, layers, ws_, many):
            j.w, j.packed, j.cin, j.cout, j.ksize, j.transposed_src = w.data_ptr(), buf.data_ptr(), cin, cout, 3, int(tr)
        host = torch.empty(lib.mednet_conv3d_pack_table_bytes(len(layers)), dtype=torch.uint8)
        blocks = ctypes.c_uint(0)
        L.check(lib.mednet_conv3d_pack_table(ctypes.addressof(jobs), len(layers), host.data_ptr(), ctypes.addressof(blocks)), "pack_table")
        table = fence.put(host.to(DEV))
        L.check(lib.mednet_conv3d_pack_many(table.data_ptr(), len(layers), blocks.value, elt, L.stream()), "pack_many")
        torch.cuda.synchronize()
        for (cin, cout, tr), a, b in zip(layers, singles, many):
            assert a.numel() == b.numel() and torch.equal(a, b), f"pack_many {cin}->{cout} transposed={tr} {mode} differs from pack_elt"
        if mode != "fp32":      # the lean rewrite leaves the other images alone: on top of a full pack nothing may change
            L.check(lib.mednet_conv3d_pack_many(table.data_ptr(), len(layers), blocks.value, elt | L.PACK_HIGH_ONLY, L.stream()), "pack_many")
            torch.cuda.synchronize()
            for (cin, cout, tr), a, b in zip(layers, singles, many):
                assert torch.equal(a, b), f"pack_many HIGH_ONLY {cin}->{cout} transposed={tr} {mode} changed a full pack"
        finish(fence, f"conv3d_pack_table/_pack_many(+HIGH_ONLY) {layers} {mode}", outputs=singles + many + [table])


# ================================================================================================ (c) norm_act.hip
@contextlib.contextmanager
def norm_helpers_in(fence, monkeypatch):
    """test_gpu_exact_norm's device-side helpers allocate in the fence; its workspace is EXACTLY mednet_gn_ws_bytes."""
    vol, f32 = N.vol, N.f32

    def workspace(n, c, spatial):
        nbytes = L.lib().mednet_gn_ws_bytes(n, c, spatial)
        return fence.workspace(nbytes, torch.float32), nbytes

    class _Rows:        # foreign_rows(...).to(DEV): the rows a kernel sums, in a slab of their own
        def __init__(self, t):
            self.t = t

        def to(self, device):
            return fence.put(self.t.to(device))

    foreign = N.foreign_rows
    made = []       # every tensor the runners hand to a kernel as an output or a workspace: `finish` asserts fence.owns for them

    def keep(t):
        made.append(t)
        return t

    with monkeypatch.context() as m:
        m.setattr(N, "vol", lambda t, dt: None if t is None else fence.put(vol(t, dt)))
        m.setattr(N, "f32", lambda t: fence.put(f32(t)))
        m.setattr(N, "nan_vol", lambda lt, dt: keep(fence.alloc((lt.n, lt.c, *lt.shape), dt, memory_format=CL)))
        m.setattr(N, "nan_f32", lambda *shape: keep(fence.alloc(shape, torch.float32)))
        m.setattr(N, "workspace", lambda n, c, spatial: (keep(workspace(n, c, spatial)[0]), L.lib().mednet_gn_ws_bytes(n, c, spatial)))
        m.setattr(N, "foreign_rows", lambda *a: _Rows(foreign(*a)))
        factories_in(fence, m, made)
        yield made


# The issue's shapes: c in {4, 5, 32, 64}, (5,6,7) and (9,11,21), n in {1, 3}, on top of the exact module's own cases (which reach
# every path of the launchers, C = 1024 in the 16-bit modes included).  gpu_util.norm_lattice has no case for an odd spatial size with
# an odd channel count per group, so c = 5 runs at (5,6,7) only; BatchNorm wants an even n * S, so with n in {1, 3} it runs at (5,6,7).
GN_EXTRA = [(3, 64, 8, (9, 11, 21)), (1, 32, 8, (9, 11, 21)), (1, 4, 1, (9, 11, 21)), (3, 32, 8, (5, 6, 7)), (1, 64, 8, (5, 6, 7)), (3, 4, 1, (5, 6, 7)),
            (1, 5, 1, (5, 6, 7)), (3, 5, 5, (5, 6, 7))]
BN_EXTRA = [(3, 64, (5, 6, 7)), (1, 32, (5, 6, 7)), (3, 4, (5, 6, 7)), (1, 5, (5, 6, 7))]
GN_PARAMS = [(c, e, m) for c in N.GN_CASES + GN_EXTRA for e in (N.EPS if c in N.OPTION_CASES + GN_EXTRA[:1] else N.EPS[:1]) for m in N.gn_modes(c)]


@pytest.mark.parametrize("case,eps,mode", GN_PARAMS, ids=lambda v: N.case_id(v) if isinstance(v, tuple) else str(v))
def test_groupnorm_statistics_apply_and_backward(case, eps, mode, monkeypatch):
    """mednet_gn_stats, mednet_gn_act_fwd and mednet_gn_act_bwd (every variant of the exact module) with exact workspaces."""
    n, c, groups, shape = case
    with Fence() as fence, norm_helpers_in(fence, monkeypatch) as made:
        N.gn_statistics_and_backward(case, eps, mode)
        finish(fence, f"gn_stats/gn_act_fwd/gn_act_bwd {case} eps={eps} {mode}", ws=True, outputs=made)


@pytest.mark.parametrize("mode", N.MODES)
@pytest.mark.parametrize("case", N.OPTION_CASES, ids=N.case_id)
def test_groupnorm_backward_in_four_launches(case, mode, monkeypatch):
    with Fence() as fence, norm_helpers_in(fence, monkeypatch) as made:
        N.gn_statistics_and_backward(case, 0.0, mode, ("gn_bwd_one_launch",))
        finish(fence, f"gn_act_bwd reduce/finalize/params launches {case} {mode}", ws=True, outputs=made)


@pytest.mark.parametrize("mode", N.MODES)
@pytest.mark.parametrize("case", [N.GN_CASES[0], N.GN_CASES[3], N.GN_CASES[7], GN_EXTRA[0], GN_EXTRA[6]], ids=N.case_id)
def test_groupnorm_backward_from_foreign_rows(case, mode, monkeypatch):
    """mednet_gn_bwd_coefficients, mednet_gn_act_bwd_fused and _fused_res on 1, 5 and many rows: the rows lie in a slab of exactly
    `rows` rows, so a reducer that sums one row too many adds a NaN."""
    with Fence() as fence, norm_helpers_in(fence, monkeypatch) as made:
        N.test_groupnorm_backward_from_foreign_rows(case, 0.0, mode)
        finish(fence, f"gn_bwd_coefficients/gn_act_bwd_fused/_fused_res {case} {mode}", ws=True, outputs=made)


@pytest.mark.parametrize("mode", N.MODES)
@pytest.mark.parametrize("pool", ["max", "avg"])
def test_groupnorm_backward_rebuilding_the_pooling_join(pool, mode, monkeypatch):
    with Fence() as fence, norm_helpers_in(fence, monkeypatch) as made:
        N.test_groupnorm_backward_rebuilding_the_pooling_join(N.POOL_CASES[0], 0.0, pool, mode)
        finish(fence, f"gn_act_bwd_fused_res_pool {N.POOL_CASES[0]} {pool} {mode}", ws=True, outputs=made)


@pytest.mark.parametrize("c,groups", [(16, 8), (8, 8)])
def test_groupnorm_finalize_alone(c, groups, monkeypatch):
    """mednet_gn_finalize on rows the exact module writes.  That module gives the kernel a workspace of its own choosing (n * c * 2
    floats); here it gets what ops.py gives it: exactly mednet_gn_ws_bytes."""
    n, spatial = 2, 1000      # (test_gpu_exact_norm.test_groupnorm_finalize_alone's)
    with Fence() as fence, norm_helpers_in(fence, monkeypatch) as made:
        nan_f32 = N.nan_f32

        def sized(*shape):
            if shape == (n * c * 2,):
                made.append(fence.workspace(L.lib().mednet_gn_ws_bytes(n, c, spatial), torch.float32))
                return made[-1]
            return nan_f32(*shape)

        monkeypatch.setattr(N, "nan_f32", sized)
        N.test_groupnorm_finalize_alone(5, c, groups, 0.0)
        finish(fence, f"gn_finalize chunks=5 C={c}", ws=True, outputs=made)


@pytest.mark.parametrize("mode", N.MODES)
@pytest.mark.parametrize("case", [N.BN_CASES[0], N.BN_CASES[2], N.BN_CASES[3]] + BN_EXTRA, ids=N.case_id)
def test_batchnorm(case, mode, monkeypatch):
    """mednet_bn_stats (with running buffers), mednet_bn_act_bwd and mednet_bn_act_bwd_fused."""
    with Fence() as fence, norm_helpers_in(fence, monkeypatch) as made:
        N.test_batchnorm(case, 0.0, mode)
        finish(fence, f"bn_stats/bn_act_bwd/bn_act_bwd_fused {case} {mode}", ws=True, outputs=made)


@pytest.mark.parametrize("n,c", [(2, 6), (3, 200)])
def test_batchnorm_eval_coefficients(n, c, monkeypatch):
    with Fence() as fence, norm_helpers_in(fence, monkeypatch) as made:
        N.test_batchnorm_eval_coefficients(n, c, 0.0)
        finish(fence, f"bn_eval_coef n={n} C={c}", ws=False, outputs=made)


ACT_COUNTS = [1, 7, 2048 * 2 + 3, 2048 * 3 + 2047]


@pytest.mark.parametrize("mode", N.MODES)
@pytest.mark.parametrize("count", ACT_COUNTS)
def test_activation_and_add_on_ragged_counts(count, mode):
    """mednet_act_fwd / mednet_act_bwd / mednet_add: 8-wide grid-stride loops with a ragged tail; the output ends at its last
    element, the inputs at theirs."""
    dt, dc, lib = DT[mode], N.dcode_of(mode), L.lib()
    t = N.act_inputs(count)
    with Fence() as fence:
        put = lambda a: fence.put(a.to(DEV).to(dt))
        outs = []
        for x, act, want in ((t.x, N.NONE, t.x), (t.x, N.RELU, t.relu), (t.x.abs(), N.ELU, t.elu_pos)):
            xg, out = put(x), fence.alloc((count,), dt)
            L.check(lib.mednet_act_fwd(xg.data_ptr(), out.data_ptr(), count, act, dc, L.stream()), "act_fwd")
            N.equal_flat(out, want, dt, f"act_fwd act={act} count={count} {mode}")
            outs.append(out)
        for dz, z, act, want in ((t.dz, t.relu, N.RELU, t.bwd_relu), (t.dz, t.z, N.ELU, t.bwd_elu)):
            dg, zg, out = put(dz), put(z), fence.alloc((count,), dt)
            L.check(lib.mednet_act_bwd(dg.data_ptr(), zg.data_ptr(), out.data_ptr(), count, act, dc, L.stream()), "act_bwd")
            N.equal_flat(out, want, dt, f"act_bwd act={act} count={count} {mode}")
            outs.append(out)
        a, b, out = put(t.x), put(t.dz), fence.alloc((count,), dt)
        L.check(lib.mednet_add(a.data_ptr(), b.data_ptr(), out.data_ptr(), count, dc, L.stream()), "add")
        N.equal_flat(out, (t.x.double() + t.dz.double()).float(), dt, f"add count={count} {mode}")
        finish(fence, f"act_fwd/act_bwd/add count={count} {mode}", outputs=outs + [out])


@pytest.mark.parametrize("mode", N.MODES)
@pytest.mark.parametrize("c,shape,kind", [(32, (4, 6, 8), "max"), (5, (4, 6, 8), "avg"), (32, (5, 7, 9), "max"), (5, (5, 7, 6), "avg"), (5, (7, 9, 11), "max")])
def test_pool2(mode, c, shape, kind):
    """ops.pool2 forward / backward and mednet_pool2_bwd with a second gradient: even extents, and odd ones whose last plane, row and
    column belong to no window (the backward's fill path); C = 5 (scalar) and C = 32 (vectors)."""
    n, dt = 2, DT[mode]
    x = lattice(f"fpp{c}{shape}", n, c, *shape, values=(-16, -8, 8, 16, 24), density=0.7)
    oshape = tuple(s // 2 for s in shape)
    g = lattice(f"fppg{c}{shape}", n, c, *oshape, values=(-16, -8, 8, 16), density=0.8)
    add = lattice(f"fppa{c}{shape}", n, c, *shape, density=0.5)
    xr = x.double().requires_grad_(True)
    yr = (F.max_pool3d if kind == "max" else F.avg_pool3d)(xr, 2)
    yr.backward(g.double())
    for ref, name in ((yr, "y"), (xr.grad, "dx"), (xr.grad + add.double(), "dx + add")):
        assert_representable(ref, dt, "pool " + name)
    code = L.POOL_MAX if kind == "max" else L.POOL_AVG
    with mednet_hip.precision(mode), Fence() as fence:
        xg = dev(fence, x, dt).requires_grad_(True)
        y = ops.pool2(xg, code)
        y.backward(dev(fence, g, dt))
        assert_exact(y, yr, f"pool2 {kind} {mode}: y")
        assert_exact(xg.grad, xr.grad, f"pool2 {kind} {mode}: dx")
        dx = fence.alloc((n, c, *shape), dt, memory_format=CL)
        gg, aa = dev(fence, g, dt), dev(fence, add, dt)
        L.check(L.lib().mednet_pool2_bwd(gg.data_ptr(), xg.data_ptr(), aa.data_ptr(), dx.data_ptr(), n, *shape, c, code, L.dt_of(dt), L.stream()),
                "pool2_bwd")
        torch.cuda.synchronize()
        assert_exact(dx, xr.grad + add.double(), f"pool2_bwd + add {kind} {mode}")
        finish(fence, f"pool2_fwd/pool2_bwd(+add) {kind} C={c} {shape} {mode}", outputs=(y.detach(), dx))


@pytest.mark.parametrize("mode", N.MODES)
@pytest.mark.parametrize("kind,act", [("max", L.ACT_RELU), ("max", L.ACT_ELU), ("avg", L.ACT_RELU)])
def test_pool2_backward_with_folded_activation(mode, kind, act):
    """mednet_pool2_bwd_act directly: dx = (pooling backward + add) * act'(x), x the activation's OUTPUT; `add` absent, dense, and as
    32 channels inside voxel rows of 96 (the gradient of UNet3D's concatenation, read where it lies) -- the leading slice, and the
    trailing one, whose last row ends at the guard.  The other 64 channels of a row hold the pattern: a read at the wrong pitch or
    of the wrong channels brings a NaN.  Even extents, C = 32: the launcher refuses these forms for odd extents and, for the strided
    gradient, for channel counts that are no multiples of 8."""
    n, c, wide, shape, dt = 2, 32, 96, (4, 6, 8), DT[mode]
    tag = f"fppa{kind}{act}"
    if act == L.ACT_ELU:
        x = U.elu_lattice(tag + "x", n, c, *shape, window_max=True)
    else:       # the output of a ReLU: zeros and positive numbers, ties inside the windows
        x = lattice(tag + "x", n, c, *shape, values=(8, 16, 24), density=0.7)
    dy = lattice(tag + "g", n, c, *(v // 2 for v in shape), values=(-16, -8, 8, 16), density=0.8) * (8 if kind == "avg" else 1)
    add = lattice(tag + "a", n, c, *shape, values=(-8, -4, 4, 8), density=0.6)
    xr = x.double().requires_grad_(True)
    (F.max_pool3d if kind == "max" else F.avg_pool3d)(xr, 2).backward(dy.double())
    grad = U.act_grad_from_out(x.double(), act)
    refs = {False: xr.grad * grad, True: (xr.grad + add.double()) * grad}
    for t in (x, dy, add, refs[False], refs[True]):
        assert_representable(t, dt, "pool2_bwd_act")
    assert bool((grad == 0).any() if act == L.ACT_RELU else ((grad > 0) & (grad < 1)).any())
    lib, code = L.lib(), L.POOL_MAX if kind == "max" else L.POOL_AVG
    d, h, w = shape
    with Fence() as fence:
        dyg, xg, addg = dev(fence, dy, dt), dev(fence, x, dt), dev(fence, add, dt)
        rows = {}
        for lo in (0, wide - c):
            rows[lo] = fence.alloc((n, wide, *shape), dt, memory_format=CL)      # (the pattern: NaN outside the slice)
            rows[lo][:, lo:lo + c] = addg
        outs = []
        for name, ptr, add_channels in (("none", None, 0), ("dense", addg.data_ptr(), 0), ("dense, pitch given", addg.data_ptr(), c),
                                        ("leading slice", rows[0][:, :c].data_ptr(), wide), ("trailing slice", rows[wide - c][:, wide - c:].data_ptr(), wide)):
            dx = fence.alloc((n, c, *shape), dt, memory_format=CL)
            L.check(lib.mednet_pool2_bwd_act(dyg.data_ptr(), xg.data_ptr(), ptr, add_channels, dx.data_ptr(), n, d, h, w, c, code, act, L.dt_of(dt),
                                             L.stream()), "pool2_bwd_act")
            torch.cuda.synchronize()
            assert_exact(dx, refs[ptr is not None], f"pool2_bwd_act {kind} act={act} add={name} {mode}")
            outs.append(dx)
        for lo, t in rows.items():      # the rows' other channels still hold the pattern
            keep = torch.ones(wide, dtype=torch.bool, device=DEV)
            keep[lo:lo + c] = False
            assert bool(torch.isnan(t[:, keep].float()).all())
        finish(fence, f"pool2_bwd_act {kind} act={act} C={c} add_channels 0/{c}/{wide} {shape} {mode}", outputs=outs, ws=False)


@pytest.mark.parametrize("mode", N.MODES)
@pytest.mark.parametrize("n,c,shape,pool,with_add", [E.POOL_GN_CASES[2], E.POOL_GN_CASES[0]])
def test_pooling_backward_with_groupnorm_sums(mode, n, c, shape, pool, with_add):
    """mednet_pool2_bwd_gn: the row buffer has exactly mednet_pool2_bwd_gn_rows rows."""
    dt, dcode = DT[mode], E.dcode_of(mode)
    lib = L.lib()
    d, h, w = shape
    rows = lib.mednet_pool2_bwd_gn_rows(n, d, h, w, c, dcode)
    assert rows > 0
    dyp, add, gy, refs = E.pool_gn_inputs(n, c, shape, pool, with_add, dt)
    with Fence() as fence:
        dypg, addg, gyg = dev(fence, dyp, dt), dev(fence, add, dt), dev(fence, gy, dt)
        outs = []
        for act in E.GN_ACTS:
            out, dx_ref, du = refs[act]
            outg = dev(fence, out, dt)
            dx, part = fence.alloc((n, c, *shape), dt, memory_format=CL), fence.alloc((n, rows, c, 2), torch.float32)
            L.check(lib.mednet_pool2_bwd_gn(dypg.data_ptr(), outg.data_ptr(), L.ptr(addg), dx.data_ptr(), gyg.data_ptr(), act, part.data_ptr(),
                                            n, d, h, w, c, L.POOL_MAX if pool == "max" else L.POOL_AVG, dcode, L.stream()), "pool2_bwd_gn")
            torch.cuda.synchronize()
            assert_exact(dx, dx_ref, f"pool2_bwd_gn {mode} act={act}: dx")
            E.compare_channel_sums(part, du, gy.double(), f"pool2_bwd_gn {mode} act={act}")
            outs += [dx, part]
        finish(fence, f"pool2_bwd_gn rows={rows} {n, c, shape, pool} {mode}", outputs=outs)


@pytest.mark.parametrize("mode", N.MODES)
@pytest.mark.parametrize("n,c,shape,pool,residual", [(2, 32, (4, 6, 8), "max", True), (1, 8, (5, 7, 9), None, True), (2, 16, (4, 8, 6), "avg", False)])
def test_groupnorm_apply_with_pooling(mode, n, c, shape, pool, residual):
    """mednet_gn_act_fwd and mednet_gn_act_pool_fwd driven directly with power-of-two coefficients (test_gpu_exact's inputs)."""
    dt, dcode = DT[mode], E.dcode_of(mode)
    lib = L.lib()
    d, h, w = shape
    tag = f"fpga{n, c, shape}"
    y = lattice(tag + "y", n, c, *shape, values=(-4, -2, 2, 4), density=0.7)
    r = lattice(tag + "r", n, c, *shape, values=(-8, 8, 16), density=0.5) if residual else None
    ca = lattice(tag + "ca", n, c, values=(-4, -2, 2, 4, 8), density=1.0)
    cb = lattice(tag + "cb", n, c, values=(-8, -4, 4, 8), density=1.0)
    u = ca.double()[:, :, None, None, None] * y.double() + cb.double()[:, :, None, None, None] + (r.double() if residual else 0)
    with Fence() as fence:
        coef = fence.put(torch.stack((ca, cb), -1).contiguous().to(DEV))
        yg, rg = dev(fence, y, dt), dev(fence, r, dt)
        outs = []
        for act, fn in ((L.ACT_NONE, lambda t: t), (L.ACT_RELU, F.relu)):
            zr = fn(u)
            assert_representable(zr, dt, "gn_act z")
            z = fence.alloc((n, c, *shape), dt, memory_format=CL)
            L.check(lib.mednet_gn_act_fwd(yg.data_ptr(), coef.data_ptr(), L.ptr(rg), z.data_ptr(), n, d * h * w, c, act, dcode, dcode, L.stream()), "gn_act_fwd")
            torch.cuda.synchronize()
            assert_exact(z, zr, f"gn_act_fwd {mode} act={act}")
            outs.append(z)
            if pool is not None:
                assert lib.mednet_gn_act_pool_supported(d, h, w, c, dcode)
                pr = (F.max_pool3d if pool == "max" else F.avg_pool3d)(zr, 2)
                assert_representable(pr, dt, "gn_act_pool pooled")
                z1 = fence.alloc((n, c, *shape), dt, memory_format=CL)
                p1 = fence.alloc((n, c, d // 2, h // 2, w // 2), dt, memory_format=CL)
                L.check(lib.mednet_gn_act_pool_fwd(yg.data_ptr(), coef.data_ptr(), L.ptr(rg), z1.data_ptr(), p1.data_ptr(), n, d, h, w, c, act,
                                                   L.POOL_MAX if pool == "max" else L.POOL_AVG, dcode, L.stream()), "gn_act_pool_fwd")
                torch.cuda.synchronize()
                assert_exact(z1, zr, f"gn_act_pool_fwd {mode} act={act}: z")
                assert_exact(p1, pr, f"gn_act_pool_fwd {mode} act={act}: pooled")
                outs += [z1, p1]
        finish(fence, f"gn_act_fwd/gn_act_pool_fwd {n, c, shape, pool} {mode}", outputs=outs)


@pytest.mark.parametrize("mode", N.MODES)
@pytest.mark.parametrize("ce,cx,eshape,xshape", [(5, 3, (5, 5, 5), (2, 2, 2)), (32, 64, (7, 9, 10), (3, 4, 5)), (32, 64, (8, 12, 10), (4, 6, 5))])
def test_upsample_concat(mode, ce, cx, eshape, xshape):
    """ops.upsample_concat forward / backward and mednet_upcat_fwd_stats (rows: mednet_upcat_stats_chunks), the encoder odd against
    twice the decoder's shape."""
    n, dt = 2, DT[mode]
    e = lattice(f"fpue{ce}{eshape}", n, ce, *eshape, density=0.6)
    x = lattice(f"fpux{cx}{xshape}", n, cx, *xshape, density=0.6)
    g = lattice(f"fpug{ce}{cx}{eshape}", n, ce + cx, *eshape, density=0.6)
    er, xr = e.double().requires_grad_(True), x.double().requires_grad_(True)
    yr = torch.cat((er, F.interpolate(xr, size=eshape, mode="nearest")), dim=1)
    yr.backward(g.double())
    assert_representable(xr.grad, dt, "upcat dx")
    lib, dcode = L.lib(), E.dcode_of(mode)
    with mednet_hip.precision(mode), Fence() as fence:
        eg, xg = dev(fence, e, dt).requires_grad_(True), dev(fence, x, dt).requires_grad_(True)
        y = ops.upsample_concat(eg, xg)
        y.backward(dev(fence, g, dt))
        assert_exact(y, yr, f"upcat {mode}: y")
        assert_exact(eg.grad, er.grad, f"upcat {mode}: denc")
        assert_exact(xg.grad, xr.grad, f"upcat {mode}: dx")
        outs = [y.detach()]
        chunks = lib.mednet_upcat_stats_chunks(n, *eshape, ce, cx, dcode)
        if chunks > 0:
            E.check_sum_conditions(yr.detach(), "upcat stats")
            out, part = fence.alloc((n, ce + cx, *eshape), dt, memory_format=CL), fence.alloc((n, chunks, ce + cx, 2), torch.float32)
            L.check(lib.mednet_upcat_fwd_stats(eg.data_ptr(), xg.data_ptr(), out.data_ptr(), part.data_ptr(), n, *eshape, ce, *xshape, cx,
                                               dcode, L.stream()), "upcat_stats")
            torch.cuda.synchronize()
            assert_exact(out, yr, f"upcat_fwd_stats {mode}: out")
            E.compare_pair_sums(part, yr.detach(), f"upcat_fwd_stats {mode}", per_channel=True)
            outs += [out, part]
        finish(fence, f"upcat_fwd/upcat_bwd/upcat_fwd_stats rows={chunks} {ce}+{cx} {eshape} {mode}", outputs=outs)


# ================================================================================================ (d) heads and losses
@contextlib.contextmanager
def head_helpers_in(fence, monkeypatch):
    to_dev_cl = H.to_dev_cl
    with monkeypatch.context() as m:
        m.setattr(H, "nan_like", lambda shape, dtype, cl=False: fence.alloc(tuple(shape), dtype, memory_format=CL if cl else None))
        m.setattr(H, "to_dev_cl", lambda t, dtype: fence.put(to_dev_cl(t, dtype)))
        factories_in(fence, m, [])      # (`saved` comes from torch.zeros, the loss scalar from torch.tensor)
        yield


def same_bits(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        if a is None or b is None:
            assert a is None and b is None, f"{what}: result {k} is missing on one side"
        elif torch.is_tensor(a):
            assert not bool(torch.isnan(a.float()).any()), f"{what}: result {k} holds a NaN"
            assert torch.equal(a.cpu(), b.cpu()), f"{what}: result {k} differs from the unfenced call"
        else:
            assert a == b, f"{what}: result {k} is {a!r}, {b!r} outside the fence"


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("cin", [16, 32, 64])
def test_small_fused_heads(mode, cin, monkeypatch):
    """mednet_head_dice_fwd / _bwd and mednet_head_ce_fwd / _bwd (part A of test_gpu_head_backward.py, its small odd shape): uint8
    labels as the last channel of a volume that ENDS with them, and an int64 map; with and without the GroupNorm rows."""
    shape = H.A_SHAPES[cin][0]
    n, eps = 2, 1e-5
    dt, dcode = DT[mode], L.dt_of(DT[mode])
    lib = L.lib()
    spatial = int(np.prod(shape))
    tag = f"hbA{cin}{shape}"
    u = U.rnd(tag + "u", n, cin, *shape)
    gy = U.half_round(U.rnd(tag + "y", n, cin, *shape), mode)
    z = H.act_output(u, L.ACT_ELU, mode)
    for kind, cout, sigmoid, ignore in H.A_LOSSES:
        wgt, b = U.rnd(tag + f"w{cout}", cout, cin, 1, 1, 1, scale=0.3), U.rnd(tag + f"b{cout}", cout)
        g = np.random.Generator(np.random.PCG64(91 + cout))
        vol = torch.from_numpy(g.integers(0, cout, size=(n, 2) + shape).astype(np.uint8))
        ii = (L.NO_IGNORE if kind == "DICE" else -100) if ignore is None else ignore
        args = (n, shape, cin, cout, dcode, None, eps, sigmoid, ii, dt)

        def run(put, lab_form, with_gy):
            with mednet_hip.precision(mode):
                pk = ops.pack_conv_weight(put(wgt.to(DEV)), 1, False)
            volg = put(vol.to(DEV))
            lab, lab_dt, lab_sn = (volg[:, -1], L.U8, 2 * spatial) if lab_form == "u8" else (put(vol[:, -1].long().contiguous().to(DEV)), L.I64, spatial)
            a = list(args)
            a[5] = put(torch.tensor(H.gscale_of(mode), dtype=torch.float32, device=DEV))
            zg = H.to_dev_cl(z, dt)
            gyg = H.to_dev_cl(gy, dt) if with_gy else None
            out = H._fused(lib, kind, zg, pk, put(b.to(DEV)), lab, lab_dt, lab_sn, put(torch.tensor(H.A_WEIGHT[:cout], device=DEV)), gyg, L.ACT_ELU, *a)
            torch.cuda.synchronize()
            return out

        for lab_form in ("u8", "i64"):
            for with_gy in (True, False):
                want = run(lambda t: t, lab_form, with_gy)
                with Fence() as fence, head_helpers_in(fence, monkeypatch):
                    got = run(fence.put, lab_form, with_gy)
                    what = f"head_{kind.lower()}_fwd/_bwd C={cout} cin={cin} {shape} labels={lab_form} gn_y={int(with_gy)} {mode}"
                    same_bits(got, want, what)
                    finish(fence, what, outputs=[t for t in got if torch.is_tensor(t)], ws=True)


HEAD_B = [("seg", (5, "DICE", False, 2)), ("seg", (16, "CE", False, 3)), ("lm", (5, 3, "CE", "L2", False, 2)), ("lm", (16, 2, "DICE", "L1", False, None))]


@pytest.mark.parametrize("mode", H.B_MODES)
@pytest.mark.parametrize("n,shape", [(1, (4, 6, 10)), (3, (12, 10, 6))])
@pytest.mark.parametrize("head,variant", HEAD_B)
def test_matrix_core_heads(head, variant, n, shape, mode, monkeypatch):
    """mednet_head_seg_fwd / _bwd and mednet_head_landmark_cls_fwd / _bwd (part B): the label volume ends with the class map's last
    byte, workspace of exactly the head's query, with and without the GroupNorm rows."""
    c = H.head_case(head, mode, n, shape, variant, "elu")
    ref = H._Device(c)
    want = {g: ref.backward(L.ACT_ELU, g) for g in (True, False)}
    with Fence() as fence, head_helpers_in(fence, monkeypatch):
        d = H._Device(c)        # (its constructor has run the forward already, on inputs that came from Tensor.to)
        assert fence.owns(d.ws) and fence.owns(d.pk) and fence.owns(d.saved) and d.ws.numel() == fence.ws_requests[-1][0]
        d.b, d.cw, d.vol, d.dl, d.saved = (fence.put(t) for t in (d.b, d.cw, d.vol, d.dl, torch.zeros_like(d.saved)))
        d.hm, d.lab = d.vol[:, :c.nh], d.vol[:, c.nh]
        d.rw = fence.put(d.rw)
        d.ws = L.workspace(d.ws.numel(), d.z.device)     # a fresh slab of the same exact size: the pattern again, not the first run's rows
        d.forward()
        for g in (True, False):
            got = d.backward(L.ACT_ELU, g)
            what = f"head_{'seg' if head == 'seg' else 'landmark_cls'}_fwd/_bwd {H.case_name(c)} gn_y={int(g)}"
            same_bits(got, want[g], what)
            assert all(t is None or fence.owns(t) for t in got)
        same_bits((d.saved,), (ref.saved,), "saved")
        finish(fence, f"head_{'seg' if head == 'seg' else 'landmark_cls'}_fwd/_bwd {H.case_name(c)}", ws=True)


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("n,cin,cout,shape", [E.HEAD_GN_CASES[2], E.HEAD_GN_CASES[1]])
def test_plain_head_and_its_data_gradient_with_groupnorm_sums(mode, n, cin, cout, shape):
    """The 1x1x1 head through hnn.Conv3d(planar_output=True) and mednet_head_dgrad_gn (rows: mednet_head_dgrad_gn_rows)."""
    dt, dcode = DT[mode], E.dcode_of(mode)
    lib = L.lib()
    d, h, w = shape
    rows = lib.mednet_head_dgrad_gn_rows(n, d, h, w, cin, dcode)
    assert rows > 0
    wt, dy, gy, dx_ref, refs = E.head_gn_inputs(n, cin, cout, shape, dt)
    x = lattice(f"fph{n, cin, cout, shape}x", n, cin, *shape, density=0.5)
    b = lattice(f"fph{n, cin, cout, shape}b", cout, values=(-3, -1, 1, 2), density=0.75)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, wt, b))
    yr = F.conv3d(xr, wr, br)
    yr.backward(dy.double())
    U.assert_sums_exact(F.conv3d(x.abs().double(), wt.abs().double(), b.abs().double()), "head y")
    U.assert_sums_exact(x.abs().double().sum() * dy.abs().double().max(), "head dw")
    with mednet_hip.precision(mode), Fence() as fence:
        conv = hnn.Conv3d(cin, cout, 1, planar_output=True).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(wt)
            conv.bias.copy_(b)
            conv.weight.data, conv.bias.data = fence.put(conv.weight.data), fence.put(conv.bias.data)
        xg = dev(fence, x, dt).requires_grad_(True)
        y = conv(xg)
        y.backward(fence.put(dy.to(DEV)))
        torch.cuda.synchronize()
        assert_exact(y, yr, f"head {mode}: logits")
        assert_exact(xg.grad, xr.grad, f"head {mode}: dx")
        assert_exact(conv.weight.grad, wr.grad, f"head {mode}: dw")
        assert_exact(conv.bias.grad, br.grad, f"head {mode}: db")
        pk = ops.pack_conv_weight(conv.weight.data, 1, False)
        dyg, gyg = fence.put(dy.to(DEV).contiguous()), dev(fence, gy, dt)
        outs = [y.detach(), pk]
        for act in E.GN_ACTS:
            gz, du = refs[act]
            gzg = dev(fence, gz, dt)
            dx, part = fence.alloc((n, cin, *shape), dt, memory_format=CL), fence.alloc((n, rows, cin, 2), torch.float32)
            L.check(lib.mednet_head_dgrad_gn(dyg.data_ptr(), pk.data_ptr(), dx.data_ptr(), gyg.data_ptr(), gzg.data_ptr(), act, part.data_ptr(),
                                             n, d, h, w, cin, cout, dcode, L.stream()), "head_dgrad_gn")
            torch.cuda.synchronize()
            assert_exact(dx, dx_ref, f"head_dgrad_gn {mode} act={act}: dx")
            E.compare_channel_sums(part, du, gy.double(), f"head_dgrad_gn {mode} act={act}")
            outs += [dx, part]
        finish(fence, f"1x1x1 head fwd/dgrad/wgrad + head_dgrad_gn rows={rows} {n, cin, cout, shape} {mode}", outputs=outs, ws=True)


class FencedPlaced:
    """test_gpu_losses.Placed with both tensors in slabs: the logits as a channel slice of a wider tensor or contiguous."""

    def __init__(self, fence, x, layout, made=None):
        n, c, S = x.shape
        self.lo, wide = (0, c) if layout == "contig" else (1, c + 2)
        full = torch.zeros(n, wide, S)
        full[:, self.lo:self.lo + c] = x
        self.full, self.gfull = fence.put(full.to(DEV)), fence.alloc((n, wide, S), torch.float32)
        if made is not None:
            made.append(self.gfull)
        self.x, self.g = self.full[:, self.lo:self.lo + c], self.gfull[:, self.lo:self.lo + c]
        self.sn, self.sc, self.c = wide * S, S, c

    outside_is_untouched = LS.Placed.outside_is_untouched


@contextlib.contextmanager
def loss_helpers_in(fence, monkeypatch):
    """test_gpu_losses' runners with outputs and the workspace (exactly mednet_loss_ws_bytes) in the fence.  Inputs are given to the
    runners as fenced device tensors: Tensor.to(DEV) of a tensor that is there already returns the tensor itself."""
    made = []       # outputs and workspaces of the runners (the tests add the gradient buffers): `finish` asserts fence.owns for them

    def keep(t):
        made.append(t)
        return t

    with monkeypatch.context() as m:
        m.setattr(LS, "nan_dev", lambda *shape: keep(fence.alloc(shape, torch.float32)))
        m.setattr(LS, "exact_ws", lambda n, c, S: keep(fence.workspace(L.lib().mednet_loss_ws_bytes(n, c, S))))
        factories_in(fence, m, made)        # (the loss scalar's gradient comes from torch.tensor)
        yield made


def fenced_labels(fence, lab, layout, tag):
    """int64 / uint8 labels [n, S], or labels as the LAST channel of an n x 3 x S uint8 (n x 2 x S int64) volume, a view with a sample
    stride of its own: the volume's last byte is the slab's last."""
    n, S = lab.shape
    if layout == "i64":
        return fence.put(lab.to(DEV)), L.I64, S
    if layout == "i64vol":
        wide = torch.full((n, 2, S), 255, dtype=torch.int64)
        wide[:, 1] = lab
        return fence.put(wide.to(DEV))[:, 1], L.I64, 2 * S
    if layout == "u8":
        return fence.put(lab.to(torch.uint8).to(DEV)), L.U8, S
    vol = torch.from_numpy(U._np_rng(tag + "vol").integers(0, 256, size=(n, 3, S)).astype(np.uint8))
    vol[:, 2] = lab.to(torch.uint8)
    return fence.put(vol.to(DEV))[:, 2], L.U8, 3 * S


LOSS_KEYS = [("plus1", 2), ("three", 3)]      # one voxel in a second workgroup; three workgroups, the last ragged (S odd)


@pytest.mark.parametrize("key,n", LOSS_KEYS)
@pytest.mark.parametrize("tgt", ["u8", "f32"])
def test_heatmap_loss(key, n, tgt, monkeypatch):
    """mednet_heatmap_loss_fwd_strided / _bwd_strided, L2 and L1: exact on integers; the uint8 target volume read as [:, :-1]."""
    c = 3
    case, refs = LS.hm_case(key, n, c, tgt)
    x = case.out.reshape(n, c, -1)
    with Fence() as fence, loss_helpers_in(fence, monkeypatch) as made:
        fcase = types.SimpleNamespace(**vars(case))
        fcase.volume, fcase.w = fence.put(case.volume.to(DEV)), fence.put(case.w.to(DEV))
        for layout in ("contig", "slice"):
            for kind in ("L2", "L1"):
                P = FencedPlaced(fence, x, layout, made)
                loss, dout = LS.run_hm(P, fcase, kind)
                what = f"heat map {kind} {key} n={n} target={tgt} {layout}"
                U.check_hm(case, refs[kind], loss, dout, what)      # (L2's dout keeps its existing bound of 4 roundings)
                assert P.outside_is_untouched(), what + ": the gradient buffer was written outside the channel slice"
        # ... and the target as a slab of its own, n x c x S with no label channel behind it: a heat map read past the last sample's
        # maps meets the guard's pattern and not label bytes
        lib, S = L.lib(), case.spatial
        own = fence.put(case.target.contiguous().to(DEV))
        for kind in ("L2", "L1"):
            P = FencedPlaced(fence, x, "contig", made)
            loss, ws, dl = LS.nan_dev(), LS.exact_ws(n, c, S), torch.tensor(case.dloss, dtype=torch.float32, device=DEV)
            k, u8 = (L.REG_L2 if kind == "L2" else L.REG_L1), int(tgt == "u8")
            L.check(lib.mednet_heatmap_loss_fwd_strided(P.x.data_ptr(), own.data_ptr(), c * S, fcase.w.data_ptr(), loss.data_ptr(), n, c, S, P.sn, P.sc,
                                                        k, u8, ws.data_ptr(), ws.numel(), L.stream()), "heatmap_loss_fwd")
            L.check(lib.mednet_heatmap_loss_bwd_strided(P.x.data_ptr(), own.data_ptr(), c * S, fcase.w.data_ptr(), dl.data_ptr(), P.g.data_ptr(), n, c, S,
                                                        P.sn, P.sc, k, u8, L.stream()), "heatmap_loss_bwd")
            torch.cuda.synchronize()
            U.check_hm(case, refs[kind], loss.cpu(), P.g.cpu(), f"heat map {kind} {key} n={n} target={tgt} in a slab of its own")
        finish(fence, f"heatmap_loss_fwd_strided/_bwd_strided {key} n={n} target={tgt}", ws=True, outputs=made)


@pytest.mark.parametrize("key,n", LOSS_KEYS)
@pytest.mark.parametrize("c", [2, 5, 17])
def test_cross_entropy_loss(key, n, c, monkeypatch):
    """mednet_ce_fwd exact on exact terms; mednet_ce_bwd on random logits equal to the unfenced call bit for bit."""
    case = U.ce_exact_case(f"ce{key}{n}{c}some", n, c, LS.SHAPES[key], -100, "some")
    ref = U.ce_exact_reference(case)
    rc = LS.random_case(key, n, c, False)
    want = LS.run_ce(LS.Placed(rc.lg, "contig"), U.ce_labels(rc, -100), rc.w, -100, rc.dloss)
    with Fence() as fence, loss_helpers_in(fence, monkeypatch) as made:
        for layout in ("contig", "slice"):
            loss, saved, _ = LS.run_ce(FencedPlaced(fence, case.lg, layout, made), fence.put(case.lab.to(DEV)), fence.put(case.w.to(DEV)), -100, 1.0, bwd=False)
            U.check_ce_exact(ref, loss, saved[0], f"CE {key} n={n} C={c} {layout}")
        P = FencedPlaced(fence, rc.lg, "contig", made)
        got = LS.run_ce(P, fence.put(U.ce_labels(rc, -100).to(DEV)), fence.put(rc.w.to(DEV)), -100, rc.dloss)
        pick = lambda r: (r[0], r[1][:1], r[2])     # (saved[1] is not cross-entropy's: nobody writes it)
        same_bits(pick(got), pick(want), f"ce_fwd/ce_bwd {key} n={n} C={c}")
        finish(fence, f"ce_fwd/ce_bwd {key} n={n} C={c}", ws=True, outputs=made)


@pytest.mark.parametrize("key,n", LOSS_KEYS)
@pytest.mark.parametrize("c,sigmoid", [(1, True), (4, False), (17, False)])
def test_dice_loss(key, n, c, sigmoid, monkeypatch):
    """mednet_dice_fwd_lt exact on dyadic probabilities for the three label forms; mednet_dice_bwd_lt on random logits equal to the
    unfenced call bit for bit."""
    case = U.dice_exact_case(f"dx{key}{n}{c}{int(sigmoid)}", n, c, LS.SHAPES[key], sigmoid)
    rc = LS.random_case(key, n, c, False)
    want = {}
    for form in ("u8v", "i64"):       # the unfenced calls first: inside the block the module's allocators are the fence's
        lab0, dt0, sn0 = LS.place_labels(rc.lab, "u8vol" if form == "u8v" else form, f"fpd{key}{c}")
        want[form] = LS.run_dice(LS.Placed(rc.lg, "contig"), lab0, dt0, sn0, rc.w, rc.eps, sigmoid, None, rc.dloss)
    with Fence() as fence, loss_helpers_in(fence, monkeypatch) as made:
        for i, ignore in enumerate((None, 0, 1)):
            ref = U.dice_exact_reference(case, ignore)
            form = LS.LABEL_LAYOUTS[i % 3]
            lab, lab_dt, lab_sn = fenced_labels(fence, case.lab, form, f"fpd{key}{c}")
            P = FencedPlaced(fence, case.lg, ("contig", "slice")[i % 2], made)
            loss, saved, dice, _ = LS.run_dice(P, lab, lab_dt, lab_sn, fence.put(case.w.to(DEV)), case.eps, sigmoid, ignore, 1.0, bwd=False)
            U.check_dice_exact(case, ref, saved, dice, loss, f"Dice exact {key} n={n} C={c} ignore={ignore} labels={form}")
        for form in ("u8vol", "i64", "i64vol"):     # (the int64 view holds the labels of the contiguous map: the same bits)
            lab, lab_dt, lab_sn = fenced_labels(fence, rc.lab, form, f"fpd{key}{c}")
            got = LS.run_dice(FencedPlaced(fence, rc.lg, "contig", made), lab, lab_dt, lab_sn, fence.put(rc.w.to(DEV)), rc.eps, sigmoid, None, rc.dloss)
            same_bits(got, want[form[:3]], f"dice_fwd_lt/dice_bwd_lt {key} n={n} C={c} labels={form}")
        finish(fence, f"dice_fwd_lt/dice_bwd_lt {key} n={n} C={c} sigmoid={int(sigmoid)}", ws=True, outputs=made)


@pytest.mark.parametrize("count", [1, 8 * 31 + 5, 65537])
def test_adam_steps(count):
    """mednet_adam_step and mednet_adam_step_scaled: p, g, m and v each in a slab of `count` floats; equal to the unfenced call."""
    case = U.adam_case(f"fpadam{count}", count)
    hp = U.ADAM_HP

    def plain(p, g, m, v):
        L.check(L.lib().mednet_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), count, hp["lr"], hp["b1"], hp["b2"], hp["eps"],
                                         0.01, 3, 0.125, L.stream()), "adam_step")
        torch.cuda.synchronize()
        return p, g, m, v

    def scaled(p, g, m, v, state):
        LS.scaled_step(p, g, m, v, state, 0.01, 0.125)
        return p, g, m, v, state

    want = plain(*LS.dev_state(case))
    want_s = scaled(*LS.dev_state(case), LS.scaler_state(1024.0, 1.0, 4.0, 7.0))
    assert want_s[4].cpu().tolist() == [1024.0, 2.0, 5.0, 0.0, 7.0, 0.0, 0.0, 0.0]
    with Fence() as fence:
        state = lambda: tuple(fence.put(t) for t in LS.dev_state(case))
        got = plain(*state())
        same_bits(got, want, f"adam_step count={count}")
        assert torch.equal(got[1].cpu(), case.g), "the gradient was written"
        got_s = scaled(*state(), fence.put(LS.scaler_state(1024.0, 1.0, 4.0, 7.0)))
        same_bits(got_s, want_s, f"adam_step_scaled count={count}")
        finish(fence, f"adam_step/adam_step_scaled count={count}", outputs=got + got_s)


# ================================================================================================ (e) vis.hip
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("shape,ncls,nh", [((5, 7, 9), 5, 2), ((16, 8, 64), 2, 0)])
def test_sample_panels(shape, ncls, nh, axis):
    """vis.sample_panels with a workspace of exactly mednet_sample_panels_ws_bytes (axis 2 answers 0: no request), both label
    forms; the uint8 label volume ends with the class map."""
    out, label, inputs = V.make_case(shape, ncls, nh, 2)
    ref = V.reference(out, label, inputs, nh, axis, "max")
    ws_bytes = L.lib().mednet_sample_panels_ws_bytes(*shape, nh, axis)
    assert (ws_bytes == 0) == (axis == 2)
    with Fence() as fence:
        o, l, x = fence.put(out.to(DEV)), fence.put(label.to(DEV)), fence.put(inputs.to(DEV))
        p1 = vis.sample_panels(o, l, x, nh, mip_axis=axis, projection_type="max")
        V.check_exact(p1, ref, f"{shape} axis {axis} u8 in place")
        lab64, hm = fence.put(label[:, -1].long().contiguous().to(DEV)), fence.put(label[:, :nh].float().to(DEV)) if nh else None
        p2 = vis.sample_panels(o, lab64, x, nh, mip_axis=axis, projection_type="max", heatmaps=hm)
        V.check_exact(p2, ref, f"{shape} axis {axis} i64 + fp32")
        assert [r[0] for r in fence.ws_requests] == ([ws_bytes] * 2 if ws_bytes else [])
        finish(fence, f"sample_panels axis={axis} {shape} classes={ncls} heatmaps={nh}", outputs=(p1.buffer, p2.buffer), ws=ws_bytes > 0)


# ================================================================================================ (f) one step of each class
def _net(kind, **kw):
    return O.keyed_init_(getattr(HM, kind)(**kw)).to(DEV)


STEPS = {
    "res_16":   ("bf16", 2, 1, (16, 16, 16), 4, 0, lambda: _net("ResidualUNet3D", in_channels=1, out_channels=4, final_sigmoid=False, f_maps=[32, 64])),
    "res_odd":  ("bf16", 1, 1, None, 4, 0, lambda: _net("ResidualUNet3D", in_channels=1, out_channels=4, final_sigmoid=False, f_maps=[32, 64])),
    "unet_gcr": ("bf16", 2, 1, (16, 16, 16), 4, 0, lambda: _net("UNet3D", in_channels=1, out_channels=4, final_sigmoid=False, f_maps=[32, 64],
                                                               layer_order="gcr")),
    "res_cbe":  ("bf16", 2, 1, (16, 16, 16), 4, 0, lambda: _net("ResidualUNet3D", in_channels=1, out_channels=4, final_sigmoid=False, f_maps=[32, 64],
                                                               conv_layer_order="cbe")),
    "res_c4_14": ("bf16", 2, 4, (16, 16, 16), 14, 0, lambda: _net("ResidualUNet3D", in_channels=4, out_channels=14, final_sigmoid=False, f_maps=[32, 64])),
    "landmark": ("bf16", 2, 1, (16, 16, 16), 2, 16, lambda: _net("ResidualUNet3D", in_channels=1, out_channels=18, final_sigmoid=False, f_maps=[32, 64])),
    "landmark_ce": ("bf16", 2, 1, (16, 16, 16), 2, 16, lambda: _net("ResidualUNet3D", in_channels=1, out_channels=18, final_sigmoid=False, f_maps=[32, 64])),
}


def _odd_shape(golden_dir):
    """Shape and batch size of the golden case res_odd (odd in every dimension)."""
    with np.load(os.path.join(golden_dir, "res_odd.npz")) as rec:
        return tuple(int(v) for v in rec["meta.shape"]), int(rec["meta.n"])


@pytest.mark.parametrize("name", list(STEPS))
def test_one_training_step_under_one_fence(name, golden_dir):
    """_fwd_bwd of a trainer built OUTSIDE the fence, the batch put in: every activation, partial buffer and workspace of the step in
    a slab of its own.  Loss and flat gradient equal the unfenced run bit for bit; the guards are intact."""
    from mednet_hip.train import LandmarkStep, SegmentationStep
    mode, n, cin, shape, ncls, nh, make = STEPS[name]
    if shape is None:
        shape, n = _odd_shape(golden_dir)
    batch = {k: v.to(DEV) for k, v in O.synthetic_batch(n, cin, shape, ncls, nh, seed=23).items()}

    def step_of():
        if nh:
            kw = dict(class_loss="CE") if name == "landmark_ce" else {}
            return LandmarkStep(make(), [0.05, 1.0], [0.015] * nh, "L2", **kw)
        return SegmentationStep(make(), loss_weight=[0.05] + [1.0] * (ncls - 1), lr=1e-3)

    def run(step, b):
        out = step._fwd_bwd(b)
        torch.cuda.synchronize()
        return out, [float(v) for v in out], step.flat.grad.clone()

    with mednet_hip.precision(mode):
        ref_step = step_of()
        _, want_loss, want_grad = run(ref_step, batch)
        ref_step.flat.release()
        del ref_step
        step = step_of()
        plane_bytes = shape[1] * shape[2] * max(64, cin) * 4
        with Fence(guard=guard_for(plane_bytes)) as fence:
            out, loss, grad = run(step, {k: fence.put(v) for k, v in batch.items()})
            assert all(np.isfinite(v) for v in loss) and loss == want_loss, f"{name}: loss {loss} inside the fence, {want_loss} outside"
            assert not bool(torch.isnan(grad).any()) and torch.equal(grad, want_grad), f"{name}: the flat gradient differs inside the fence"
            # (a LandmarkStep's first result is the sum of the two losses the fused node wrote: ATen's tensor, not the library's)
            finish(fence, f"{type(step).__name__}._fwd_bwd {name} n={n} {shape} {mode}", outputs=list(out[1:] if nh else out), ws=True)
        step.flat.release()
