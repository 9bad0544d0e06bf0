"""The C ABI of the matrix-core segmentation head for 5 .. 16 classes (mednet_head_seg_*): symbols, ctypes rows, the truth table of
mednet_head_seg_supported and the size queries.  No GPU needed."""
import ctypes
import itertools

from mednet_hip import _lib as L

NAMES = ["mednet_head_seg_supported", "mednet_head_seg_ws_bytes", "mednet_head_seg_gn_rows", "mednet_head_seg_fwd",
         "mednet_head_seg_bwd"]
SPATIALS = [64, 720, 2097152]


def test_the_five_entries_resolve_and_the_abi_version_stays_3():
    h = ctypes.CDLL(L.LIB_PATH)
    for name in NAMES:
        assert hasattr(h, name), name
        assert name in L.SIGNATURES, name
    assert L.lib().mednet_abi_version() == 3


def test_supported_truth_table():
    lib = L.lib()
    ok = lib.mednet_head_seg_supported
    for ncls, dt, sp in itertools.product(range(5, 17), (L.BF16, L.F16), SPATIALS):
        assert ok(32, ncls, dt, L.U8, sp) == 1, (ncls, dt, sp)
    for ncls in (4, 17):
        assert ok(32, ncls, L.BF16, L.U8, 720) == 0, ncls
    for cin in (16, 64):
        assert ok(cin, 14, L.BF16, L.U8, 720) == 0, cin
    assert ok(32, 14, L.F32, L.U8, 720) == 0
    assert ok(32, 14, L.BF16, L.I64, 720) == 0
    assert ok(32, 14, L.F16, L.U8, 27) == 0
    try:
        assert lib.mednet_set_option(b"head_seg_mfma", 0) == 0
        assert ok(32, 14, L.BF16, L.U8, 720) == 0 and ok(32, 5, L.F16, L.U8, 64) == 0
    finally:
        lib.mednet_set_option(b"head_seg_mfma", 1)
    assert ok(32, 14, L.BF16, L.U8, 720) == 1


def test_workspace_and_groupnorm_rows():
    lib = L.lib()
    for sp in SPATIALS + [128, 8192, 8196, 128 ** 3]:
        rows = lib.mednet_head_seg_gn_rows(sp)
        assert rows == -(-(-(-sp // 128)) // 64), (sp, rows)
        for n, ncls in itertools.product((1, 2, 4), (5, 9, 16)):
            assert lib.mednet_head_seg_ws_bytes(n, sp, ncls) >= n * rows * (16 * 32 + 16) * 4
    ns, sps, cs = (1, 2, 3, 4, 8), (64, 720, 8192, 8196, 2097152, 4 * 2097152), tuple(range(5, 17))
    ws = lib.mednet_head_seg_ws_bytes
    for sp, c in itertools.product(sps, cs):
        assert all(ws(a, sp, c) <= ws(b, sp, c) for a, b in zip(ns, ns[1:]))
    for n, c in itertools.product(ns, cs):
        assert all(ws(n, a, c) <= ws(n, b, c) for a, b in zip(sps, sps[1:]))
    for n, sp in itertools.product(ns, sps):
        assert all(ws(n, sp, a) <= ws(n, sp, b) for a, b in zip(cs, cs[1:]))


def test_the_narrow_heads_answer_as_before():
    lib = L.lib()
    for dt, ld in itertools.product((L.BF16, L.F16, L.F32), (L.U8, L.I64)):
        assert lib.mednet_head_dice_supported(32, 4, dt, ld) == 1
        assert lib.mednet_head_dice_supported(32, 5, dt, ld) == 0
