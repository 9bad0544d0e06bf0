"""ExtResNetBlock as ONE autograd node (midasmednet/unet/components.py:136-180).

    z1 = act(GN1(conv1(x)));  z2 = act(GN2(conv2(z1)));  out = act(GN3(conv3(z2)) + z1)

Hand-written backward over the C ABI instead of 9 chained autograd nodes: the post-activation tensor z1 has two consumers
(conv2 and the residual add), so autograd would materialise both gradients and sum them with an ATen kernel (3 full-size
tensor passes per block).  Here GroupNorm-1's backward reads the two gradient streams directly (`dz2` operand of
mednet_gn_act_bwd), the weight gradients go to the side stream exactly as in the per-op path, and nothing but
libmednet_hip kernels runs between the block's input and output.
"""
from __future__ import annotations

import torch
from torch.autograd import Function

import os

from . import _lib as L
from . import config, debug, ops

ENABLED = os.environ.get("MEDNET_BLOCK_NODE", "1") == "1"
WGRAD_FIRST = ops.WGRAD_FIRST  # A/B knob: launch order of the two gradients (this module's own switch for the block's layers)


def _conv_fwd(x, packed, cout, want_stats, x_layout=L.NDHWC):
    return ops.conv_forward(x, x_layout, packed, None, cout, 3, False, config.act_dtype(), want_stats)


FUSE_POOL = os.environ.get("MEDNET_FUSE_POOL", "1") == "1"  # A/B knob: the next level's pooling inside the block's last apply pass


def _gn_fwd(y, partial, gamma, beta, groups, eps, act, residual, pool_mode=None):
    """-> (z, stats, coef, pooled) on the path of ops.GroupNormActFn.  `pool_mode`: also write the 2x2x2-pooled z in the same pass
    when the shape allows; `pooled` is None otherwise."""
    stats, coef = ops.gn_statistics(y, gamma, beta, groups, eps, partial)
    z, pooled = ops.norm_apply(y, coef, residual, act, pool_mode if FUSE_POOL else None)
    return z, stats, coef, pooled


def _gn_bwd(dz, dz2, y, z, coef, stats, gamma_p, beta_p, groups, act, want_dres, partial=None, lazy=None):
    """Returns (dy, dres, dgamma, dbeta).  `partial`: the first pass ({sum du, sum du*y} per channel) already taken by the
    kernel that produced dz; `z`: the residual layer, act' from the block output; `lazy`: dz was not written (ops.gn_backward)."""
    b = ops._NormBackward(y, gamma_p, beta_p, want_dres)
    ops.gn_backward(b, dz, y, z, coef, stats, gamma_p, act, L.ACT_NONE, partial, groups, dz2=dz2, lazy=lazy)
    return (b.dx, b.dres, *b.param_grads())


FUSE_C1GN = os.environ.get("MEDNET_FUSE_C1GN", "1") == "1"  # A/B knob: first layer's GroupNorm backward inside its weight gradient
C1GN_COUNT = {"fused": 0}  # (tests check that the fused form really ran, like ops.GN3_COUNT)


def _c1_gn_applies(xin, y, partial, need_dx):
    """The network's first SingleConv (Cin = 1, or 2-4 fp32 channels; no gradient of the input wanted): its GroupNorm backward
    feeds nothing but the weight gradient, so the apply pass can happen inside that kernel's staging (mednet_conv3d_wgrad_c1_gn /
    mednet_conv3d_wgrad_cm_gn)."""
    if not (FUSE_C1GN and partial is not None and not need_dx and y.dtype != torch.float32 and config.conv_algo() != L.ALGO_DIRECT):
        return False
    cin = xin.shape[1]
    if cin == 1:
        return bool(L.lib().mednet_conv3d_wgrad_c1_gn_supported(y.shape[1], L.dt(xin), L.dt(y)))
    return bool(L.lib().mednet_conv3d_wgrad_cm_gn_supported(cin, y.shape[1], L.dt(xin), L.dt(y)))


def _c1_gn_bwd(xin, dz, y, coef, stats, gamma_p, beta_p, weight_p, groups, act, partial, x_layout=L.NDHWC):
    """GroupNorm(+activation) backward and 3x3x3 weight gradient of the first layer without the gradient tensor between them.
    Returns (dw-or-None, dgamma-or-None, dbeta-or-None) like _gn_bwd / _conv_bwd.  On the caller's stream: the side stream is
    busy with the second layer's weight gradient at this point, and this kernel is HBM-bound like the pass it replaces."""
    n, c, d, h, w = y.shape
    cin = xin.shape[1]
    lib = L.lib()
    C1GN_COUNT["fused"] += 1
    dgamma, dg_direct = ops._grad_target(gamma_p, (c,))
    dbeta, db_direct = ops._grad_target(beta_p, (c,))
    dw, dw_direct = ops._grad_target(weight_p, (c, cin, 3, 3, 3))
    bcoef = torch.empty((n, c, 3), dtype=torch.float32, device=y.device)
    ws = L.workspace(max(lib.mednet_gn_ws_bytes(n, c, d * h * w), lib.mednet_conv3d_wgrad_ws_bytes(n, d, h, w, cin, c, 3, 0)), y.device)
    L.check(lib.mednet_gn_bwd_coefficients(stats.data_ptr(), gamma_p.data_ptr(), partial.data_ptr(), partial.shape[1],
                                           bcoef.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), n, d * h * w, c, groups,
                                           ws.data_ptr(), ws.numel(), L.stream()), "gn_bwd_coefficients")
    if cin == 1:
        L.check(lib.mednet_conv3d_wgrad_c1_gn(xin.data_ptr(), dz.data_ptr(), y.data_ptr(), coef.data_ptr(), bcoef.data_ptr(),
                                              dw.data_ptr(), n, d, h, w, c, act, L.dt(xin), L.dt(y), ws.data_ptr(), ws.numel(),
                                              L.stream()), "conv3d_wgrad_c1_gn")
    else:  # 2-4 input channels, read in the layout the forward read them in
        L.check(lib.mednet_conv3d_wgrad_cm_gn(xin.data_ptr(), x_layout, dz.data_ptr(), y.data_ptr(), coef.data_ptr(), bcoef.data_ptr(),
                                              dw.data_ptr(), n, d, h, w, cin, c, act, L.dt(xin), L.dt(y), ws.data_ptr(), ws.numel(),
                                              L.stream()), "conv3d_wgrad_cm_gn")
    return (None if dw_direct else dw), (None if dg_direct else dgamma), (None if db_direct else dbeta)


FUSE_DRES = os.environ.get("MEDNET_FUSE_DRES", "1") == "1"  # A/B knob: residual gradient summed in conv2's data gradient


FUSE_GNB = ops.FUSE_GNB  # A/B knob: GroupNorm-backward sums in the data-gradient epilogue (this module's own switch, as WGRAD_FIRST)


def _conv_bwd(x, dy, packed, weight_p, need_dx, add=None, gnb=None, x_layout=L.NDHWC):
    """ops.conv_backward under this module's switches.  Returns (dx, dw-or-None, partial-or-None)."""
    return ops.conv_backward(x, dy, packed, weight_p, need_dx, ops.block_dx_dtype(x), add=add, gnb=gnb if FUSE_GNB else None,
                             x_layout=x_layout, wgrad_first=WGRAD_FIRST)


class ResBlockFn(Function):
    @staticmethod
    def forward(ctx, x, w1, g1, b1, w2, g2, b2, w3, g3, b3, pk1, pk2, pk3, groups, eps, act, hook=None, pool=None):
        L.require_gpu(x, "ExtResNetBlock")
        ctx.algo = config.conv_algo()
        x = ops._as_act(x)
        cout = w1.shape[0]
        # Cin == 1: NCDHW and NDHWC coincide; 2-4 fp32 channels (16-bit storage) are read where they lie
        xin, x_layout = ops.first_layer_input(x, cout, 3, config.act_dtype())
        ctx.x_layout = x_layout
        fuse = (cout // groups) % 2 == 0  # fused partials are per channel pair (include/mednet_hip.h)
        y1, p1 = _conv_fwd(xin, pk1, cout, fuse, x_layout)
        z1, s1, c1, _ = _gn_fwd(y1, p1, g1, b1, groups, eps, act, None)
        y2, p2 = _conv_fwd(z1, pk2, cout, fuse)
        z2, s2, c2, _ = _gn_fwd(y2, p2, g2, b2, groups, eps, act, None)
        y3, p3 = _conv_fwd(z2, pk3, cout, fuse)
        # `pool`: a holder the caller reads the pooled output from (the next encoder level pools this block's output: one pass
        # writes both; ops.SkipPool2Fn uses the stash instead of launching the pooling kernel)
        out, s3, c3, pooled = _gn_fwd(y3, p3, g3, b3, groups, eps, act, z1, pool_mode=pool.mode if pool is not None else None)
        if pool is not None:
            pool.pooled = pooled
        if debug.TRACE is not None:
            debug.trace("resblock.fwd", y1, p1, s1, c1, z1, y2, p2, s2, c2, z2, y3, p3, s3, c3, out)
        ctx.save_for_backward(xin, y1, z1, y2, z2, y3, out, s1, c1, s2, c2, s3, c3, pk1, pk2, pk3)
        ctx.params = (w1, g1, b1, w2, g2, b2, w3, g3, b3)
        ctx.meta = (groups, act)
        ctx.gn3 = hook
        if hook is not None:
            hook.gn_in, hook.act = y3, act
        return out

    @staticmethod
    @ops._with_algo
    def backward(ctx, dout):
        xin, y1, z1, y2, z2, y3, out, s1, c1, s2, c2, s3, c3, pk1, pk2, pk3 = ctx.saved_tensors
        w1, g1, b1, w2, g2, b2, w3, g3, b3 = ctx.params
        groups, act = ctx.meta
        part3 = ctx.gn3.take(dout) if ctx.gn3 is not None else None  # (before any conversion: identity matters)
        lazy = None
        if ctx.gn3 is not None and part3 is not None:
            lazy, ctx.gn3.lazy = ctx.gn3.lazy, None  # dout is an unwritten placeholder: see ops.SkipPool2Fn / GN3Hook.take
        if lazy is None:
            dout = ops.to_cl(dout.to(out.dtype))
        # GN3 + residual + activation: act' from the block output; dres = gradient of the residual branch (into z1)
        dy3, dres, dg3, db3 = _gn_bwd(dout, None, y3, out, c3, s3, g3, b3, groups, act, True, partial=part3, lazy=lazy)
        dz2, dw3, part2 = _conv_bwd(z2, dy3, pk3, w3, True, gnb=(y2, c2, act))
        dy2, _, dg2, db2 = _gn_bwd(dz2, None, y2, None, c2, s2, g2, b2, groups, act, False, partial=part2)
        # z1 feeds conv2 AND the residual add: the two gradients are summed in the epilogue of conv2's data gradient (bf16
        # matrix-core path), otherwise inside GroupNorm-1's backward (two more tensor reads)
        n_, c_, d_, h_, w_ = z1.shape
        fuse = FUSE_DRES and dres.dtype == dy2.dtype and bool(
            L.lib().mednet_conv3d_dgrad_add_supported(n_, d_, h_, w_, c_, c_, config.conv_algo(), L.dt(dy2)))
        dz1, dw2, part1 = _conv_bwd(z1, dy2, pk2, w2, True, add=dres if fuse else None, gnb=(y1, c1, act) if fuse else None)
        if fuse and _c1_gn_applies(xin, y1, part1, ctx.needs_input_grad[0]):
            dy1 = dx = None  # (never materialised)
            dw1, dg1, db1 = _c1_gn_bwd(xin, dz1, y1, c1, s1, g1, b1, w1, groups, act, part1, ctx.x_layout)
        else:
            dy1, _, dg1, db1 = _gn_bwd(dz1, None if fuse else dres, y1, None, c1, s1, g1, b1, groups, act, False, partial=part1)
            dx, dw1, _ = _conv_bwd(xin, dy1, pk1, w1, ctx.needs_input_grad[0], x_layout=ctx.x_layout)
        if debug.TRACE is not None:
            debug.trace("resblock.bwd", None if lazy is not None else dout, part3, dy3, dres, dz2, part2, dy2, dz1, part1, dy1, dx)
        return (dx, dw1, dg1, db1, dw2, dg2, db2, dw3, dg3, db3) + (None,) * 8


class PoolStash:
    """Carried by a block output whose consumer is a 2x2x2 pooling of `mode`: the pooled tensor the block's last apply pass wrote
    beside the output (or None when the shape did not allow it).  ops.SkipPool2Fn / Pool2Fn take it instead of launching."""
    __slots__ = ("mode", "pooled", "version")

    def __init__(self, mode):
        self.mode, self.pooled, self.version = mode, None, -1  # version: the output's `_version` when the stash was attached


def res_block(x, convs, norms, groups, eps, act, pool_mode=None, head_next=False):
    """convs / norms: the three mednet_hip.nn.Conv3d / GroupNorm modules of the block.  `pool_mode`: the block's output goes into a
    2x2x2 pooling of that mode next (the next encoder level): the pooled tensor is produced in the same pass and stashed on the
    output (`_mednet_pooled`).  `head_next`: the caller (the U-Net's own forward) hands the output to the network's head and to
    nothing else: a fused head may then leave the output's gradient unwritten and let this block's backward rebuild it
    (ops.GN3Hook.lazy_head_ok, ops._valu_head_bwd)."""
    (k1, k2, k3), (n1, n2, n3) = convs, norms
    hook = ops.GN3Hook() if (ops.FUSE_GN3 and torch.is_grad_enabled()) else None  # (training only)
    if hook is not None:
        hook.lazy_head_ok = bool(head_next)  # (this node's backward is the one that consumes the gradient: it holds the hook)
    stash = PoolStash(pool_mode) if (pool_mode is not None and FUSE_POOL) else None
    out = ResBlockFn.apply(x, k1.weight, n1.weight, n1.bias, k2.weight, n2.weight, n2.bias, k3.weight, n3.weight, n3.bias,
                           k1._packed(x, converts=True), k2._packed(x, converts=True), k3._packed(x, converts=True), groups, eps, act,
                           hook, stash)  # (the node casts x to the storage type; its inner tensors have x's extent)
    if hook is not None:
        out._mednet_gn3 = hook  # see ops.GN3Hook: the consumer of `out` may take GroupNorm-3's first backward pass
    if stash is not None and stash.pooled is not None:
        stash.version = out._version
        out._mednet_pooled = stash
    return out
