"""Host-side checks of the multi-channel first-layer entries of the C ABI (2-4 fp32 input channels, 16-bit storage) -- no GPU.

The queries answer from the launchers' own planning code: which calls the matrix-core first-layer kernel takes, how many partial
rows it writes, and what the weight gradient's workspace has to hold.
"""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torch-mednet_amd"))
from mednet_hip import _lib as L  # noqa: E402

F32, BF16, F16 = L.F32, L.BF16, L.F16


def with_option(name, value, default, fn):
    lib = L.lib()
    lib.mednet_set_option(name, value)
    try:
        return fn()
    finally:
        lib.mednet_set_option(name, default)


def test_new_symbols_resolve_and_the_abi_version_stays():
    lib = L.lib()
    for name in ("mednet_conv3d_cm_supported", "mednet_conv3d_wgrad_cm_gn_supported", "mednet_conv3d_wgrad_cm_gn",
                 "mednet_conv3d_wgrad_cm_plan"):
        assert getattr(lib, name) is not None and name in L.SIGNATURES
    assert lib.mednet_abi_version() == 3


@pytest.mark.parametrize("cin", [2, 3, 4])
@pytest.mark.parametrize("cout", [16, 32, 48, 64])
def test_cm_supported_takes_the_first_layer_calls(cin, cout):
    lib = L.lib()
    for y in (BF16, F16):
        for algo in (L.ALGO_AUTO, L.ALGO_MFMA, L.ALGO_AUTO | L.ALGO_SPLITW_BIT):
            assert lib.mednet_conv3d_cm_supported(cin, cout, 3, F32, y, algo) == 1


def test_cm_supported_refuses_everything_else():
    lib = L.lib()
    q = lib.mednet_conv3d_cm_supported
    for cin in (1, 5, 8):
        assert q(cin, 32, 3, F32, BF16, L.ALGO_AUTO) == 0
    assert q(4, 8, 3, F32, BF16, L.ALGO_AUTO) == 0          # Cout % 16
    assert q(4, 32, 1, F32, BF16, L.ALGO_AUTO) == 0         # 1x1x1
    assert q(4, 32, 3, BF16, BF16, L.ALGO_AUTO) == 0        # 16-bit x
    assert q(4, 32, 3, F16, F16, L.ALGO_AUTO) == 0
    assert q(4, 32, 3, F32, F32, L.ALGO_AUTO) == 0          # fp32 storage
    assert q(4, 32, 3, F32, BF16, L.ALGO_DIRECT) == 0
    assert with_option(b"conv_cm", 0, 1, lambda: q(4, 32, 3, F32, BF16, L.ALGO_AUTO)) == 0
    assert q(4, 32, 3, F32, BF16, L.ALGO_AUTO) == 1
    g = lib.mednet_conv3d_wgrad_cm_gn_supported
    assert g(4, 32, F32, BF16) == 1 and g(2, 64, F32, F16) == 1 and g(3, 48, F32, BF16) == 1
    assert g(1, 32, F32, BF16) == 0 and g(5, 32, F32, BF16) == 0 and g(4, 128, F32, BF16) == 0 and g(4, 32, BF16, BF16) == 0
    assert g(4, 32, F32, F32) == 0
    assert with_option(b"wgrad_c1_mfma", 0, 1, lambda: g(4, 32, F32, BF16)) == 0
    assert with_option(b"conv_cm", 0, 1, lambda: g(4, 32, F32, BF16)) == 0


def c1_grid_rule(n, d, h, w, cout, cus=256):
    """The first-layer kernels' grid: 4, 3 or 2 workgroups per CU, whichever fills the walk's last round best, in multiples of the
    channel-block count; one per (brick, channel block) item when there are no more than 4 per CU."""
    ncb = (cout + 31) // 32
    nitems = n * ((d + 3) // 4) * ((h + 7) // 8) * ((w + 15) // 16) * ncb
    if nitems <= 4 * cus:
        return nitems, ncb
    best, best_fill = 0, 0.0
    for per_cu in (4, 3, 2):
        g = per_cu * cus // ncb * ncb
        fill = nitems / (-(-nitems // g) * g)
        if fill > best_fill + 0.01:
            best, best_fill = g, fill
    return best, ncb


@pytest.mark.parametrize("n,shape,cout", [(4, (128, 128, 128), 32), (2, (160, 160, 96), 64), (3, (40, 72, 80), 32), (2, (9, 11, 21), 48)])
def test_fused_rows_follow_the_grid_rule(n, shape, cout):
    lib = L.lib()

    def rows(cin, algo):
        return lib.mednet_conv3d_fused_stats_chunks(n, *shape, cin, cout, 3, F32, BF16, algo)

    grid, ncb = c1_grid_rule(n, *shape, cout)
    for cin in (2, 3, 4):
        assert with_option(b"assume_cus", 256, 0, lambda: rows(cin, L.ALGO_AUTO)) == 4 * grid // ncb
        assert with_option(b"assume_cus", 256, 0, lambda: rows(cin, L.ALGO_DIRECT)) == 0
    lib.mednet_set_option(b"assume_cus", 256)
    try:
        assert with_option(b"conv_cm", 0, 1, lambda: rows(4, L.ALGO_AUTO)) == 0
    finally:
        lib.mednet_set_option(b"assume_cus", 0)


def wgrad_plan(n, shape, cin, cout, dtype, gn):
    out = (C.c_int * 4)()
    assert L.lib().mednet_conv3d_wgrad_cm_plan(n, *shape, cin, cout, dtype, gn, C.addressof(out)) == 0, L.lib().mednet_last_error().decode()
    return list(out)


def test_weight_gradient_workspace_and_plan():
    lib = L.lib()
    n, shape = 4, (128, 128, 128)
    for cin in (2, 3, 4):
        for cout in (16, 32, 48, 64):
            for gn in (0, 1):
                blocks, nb, per_cu, lds = wgrad_plan(n, shape, cin, cout, BF16, gn)
                assert nb == (cout + 31) // 32 and per_cu in (1, 2) and 0 < blocks <= 512 * per_cu
                assert lds == cin * 4352 + 32768 * nb and lds * per_cu <= 160 * 1024
                assert lib.mednet_conv3d_wgrad_ws_bytes(n, *shape, cin, cout, 3, 0) >= blocks * 27 * cin * cout * 4
            assert wgrad_plan(n, shape, cin, cout, BF16, 1)[0] <= wgrad_plan(n, shape, cin, cout, BF16, 0)[0]
            assert wgrad_plan(n, shape, cin, cout, F16, 0) == wgrad_plan(n, shape, cin, cout, BF16, 0)
    assert wgrad_plan(1, (4, 8, 16), 4, 64, BF16, 0)[0] == 1     # one brick, one workgroup
    out = (C.c_int * 4)()
    assert lib.mednet_conv3d_wgrad_cm_plan(n, *shape, 1, 32, BF16, 0, C.addressof(out)) != 0
    assert lib.mednet_conv3d_wgrad_cm_plan(n, *shape, 4, 128, BF16, 0, C.addressof(out)) != 0
    # the other layers' workspace is what it was before this path existed (the maximum did not have to grow)
    assert lib.mednet_conv3d_wgrad_ws_bytes(n, *shape, 1, 32, 3, 0) == 57147904
    assert lib.mednet_conv3d_wgrad_ws_bytes(n, *shape, 32, 32, 3, 0) == 113771008
    assert lib.mednet_conv3d_wgrad_ws_bytes(n, *shape, 4, 32, 3, 0) == 57147904


# (n, shape, cout, mednet_conv3d_wgrad_ws_bytes as the library answered before the one- and multi-channel kernels became one)
C1_CASES = [(4, (128, 128, 128), 32, 57147904), (2, (160, 160, 96), 64, 57852416), (3, (40, 72, 80), 32, 56667008),
            (2, (9, 11, 21), 16, 6636160), (1, (5, 6, 7), 64, 1327872)]


@pytest.mark.parametrize("n,shape,cout,ws_bytes", C1_CASES)
def test_one_channel_plans_are_what_they_were(n, shape, cout, ws_bytes):
    """Cin = 1 through the merged first-layer host code: the weight gradient launches min(bricks, 1024) workgroups of 27 * cout
    partial sums -- the workspace query, a maximum over every weight-gradient path of the layer plus the bias partials, covers them
    and has not moved -- and the forward writes 4 partial rows per workgroup of a channel block, for fp32 and 16-bit input."""
    lib = L.lib()
    d, h, w = shape
    bricks = n * ((d + 3) // 4) * ((h + 7) // 8) * ((w + 15) // 16)
    got = lib.mednet_conv3d_wgrad_ws_bytes(n, d, h, w, 1, cout, 3, 0)
    assert got >= min(bricks, 1024) * 27 * cout * 4
    assert got == ws_bytes
    grid, ncb = c1_grid_rule(n, d, h, w, cout)
    for x_dtype, y_dtype in ((F32, BF16), (F32, F16), (BF16, BF16), (F16, F16)):
        for algo in (L.ALGO_AUTO, L.ALGO_AUTO | L.ALGO_SPLITW_BIT):
            rows = with_option(b"assume_cus", 256, 0, lambda: lib.mednet_conv3d_fused_stats_chunks(n, d, h, w, 1, cout, 3, x_dtype, y_dtype, algo))
            assert rows == 4 * grid // ncb
    # the conv_cm option gates 2 to 4 channels only; 16-bit input of the other 16-bit type is not taken
    assert with_option(b"conv_cm", 0, 1, lambda: lib.mednet_conv3d_fused_stats_chunks(n, d, h, w, 1, cout, 3, F32, BF16, L.ALGO_AUTO)) > 0
    assert lib.mednet_conv3d_fused_stats_chunks(n, d, h, w, 1, cout, 3, F16, BF16, L.ALGO_AUTO) == 0
    g = lib.mednet_conv3d_wgrad_c1_gn_supported
    assert g(cout, F32, BF16) == 1 and g(cout, F16, F16) == 1 and g(cout, BF16, F16) == 0 and g(48, F32, BF16) == 0
    assert with_option(b"wgrad_c1_mfma", 0, 1, lambda: g(cout, F32, BF16)) == 0
    assert with_option(b"conv_cm", 0, 1, lambda: g(cout, F32, BF16)) == 1
