"""The C ABI of the deep-supervision node (mednet_ds_head_*): symbols, ctypes rows, the truth table of mednet_ds_head_supported with
its knob, and the size queries.  No GPU needed."""
import ctypes
import itertools

from mednet_hip import _lib as L

NAMES = ["mednet_ds_head_supported", "mednet_ds_head_ws_bytes", "mednet_ds_head_gn_rows", "mednet_ds_head_fwd", "mednet_ds_head_bwd"]
EXTENTS = [(4, 4, 8), (6, 6, 6), (24, 24, 16), (64, 64, 64)]


def test_the_five_entries_resolve_and_the_abi_version_stays_3():
    h = ctypes.CDLL(L.LIB_PATH)
    for name in NAMES:
        assert hasattr(h, name), name
        assert name in L.SIGNATURES, name
    assert L.lib().mednet_abi_version() == 3


def test_supported_truth_table():
    lib = L.lib()
    ok = lib.mednet_ds_head_supported
    for cin, ncls, dt, (d, h, w), s in itertools.product(range(64, 257, 32), (1, 2, 4, 5, 8, 14, 16), (L.BF16, L.F16), EXTENTS, (1, 2, 3)):
        assert ok(cin, ncls, dt, L.U8, d, h, w, s) == 1, (cin, ncls, dt, d, h, w, s)
    for cin in (16, 32, 48, 72, 80, 288, 512):
        assert ok(cin, 4, L.BF16, L.U8, 4, 4, 8, 1) == 0, cin
    for ncls in (0, 17, 32):
        assert ok(64, ncls, L.BF16, L.U8, 4, 4, 8, 1) == 0, ncls
    assert ok(64, 4, L.F32, L.U8, 4, 4, 8, 1) == 0            # fp32 storage
    assert ok(64, 4, L.BF16, L.I64, 4, 4, 8, 1) == 0          # int64 labels
    for s in (-1, 0, 4, 5):
        assert ok(64, 4, L.BF16, L.U8, 4, 4, 8, s) == 0, s
    for d, h, w in ((3, 3, 3), (5, 6, 7), (0, 4, 4), (4, -4, 4)):  # d h w % 4 != 0, or no voxels
        assert ok(64, 4, L.F16, L.U8, d, h, w, 1) == 0, (d, h, w)
    try:
        assert lib.mednet_set_option(b"ds_head_fuse", 0) == 0
        assert ok(64, 4, L.BF16, L.U8, 4, 4, 8, 1) == 0 and ok(256, 16, L.F16, L.U8, 24, 24, 16, 2) == 0
    finally:
        lib.mednet_set_option(b"ds_head_fuse", 1)
    assert ok(64, 4, L.BF16, L.U8, 4, 4, 8, 1) == 1


def test_workspace_is_monotone_and_holds_both_directions():
    lib = L.lib()
    ws = lib.mednet_ds_head_ws_bytes
    ns, es, cins, cs = (1, 2, 3, 4, 8), ((4, 4, 8), (6, 6, 6), (24, 24, 16), (32, 32, 32), (64, 64, 64)), tuple(range(64, 257, 32)), (1, 4, 5, 16)
    for (d, h, w), cin, c in itertools.product(es, cins, cs):
        assert all(ws(a, d, h, w, cin, c) <= ws(b, d, h, w, cin, c) for a, b in zip(ns, ns[1:]))
    for n, cin, c in itertools.product(ns, cins, cs):
        assert all(ws(n, *a, cin, c) <= ws(n, *b, cin, c) for a, b in zip(es, es[1:]))
    for n, (d, h, w), c in itertools.product(ns, es, cs):
        assert all(ws(n, d, h, w, a, c) <= ws(n, d, h, w, b, c) for a, b in zip(cins, cins[1:]))
    for n, (d, h, w), cin in itertools.product(ns, es, cins):
        assert all(ws(n, d, h, w, cin, a) <= ws(n, d, h, w, cin, b) for a, b in zip(cs, cs[1:]))
    for n, (d, h, w), cin, c in itertools.product(ns, es, cins, cs):
        chunks = -(-(-(-(d * h * w) // 128)) // 64)   # (a lower bound: a workgroup takes at most 64 runs of 128 voxels)
        # forward: Dice rows + CE rows; backward: one row of 32 x 33 floats per workgroup and 32-channel tile
        assert ws(n, d, h, w, cin, c) >= 4 * n * chunks * max(2 * c + 2, (cin // 32) * 32 * 33)


def test_groupnorm_rows_are_none_or_one_per_workgroup():
    """0 (the node takes no GroupNorm-3 sums: the block falls back by itself) or the workgroups per sample."""
    lib = L.lib()
    for (d, h, w), cin, dt in itertools.product(EXTENTS, (64, 128, 256), (L.BF16, L.F16)):
        assert lib.mednet_ds_head_gn_rows(d, h, w, cin, dt) in (0, -(-(-(-(d * h * w) // 128)) // 64))
