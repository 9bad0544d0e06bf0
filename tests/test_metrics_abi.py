"""The C ABI of the case-evaluation entries (additive to ABI 3), without a GPU: every new symbol is in the header, the library and the
ctypes table with matching argument counts, the workspace queries follow the plan of csrc/metrics.hip, and every refusal returns its
code with a message under the entry's own name before anything is launched."""
import ctypes
import re

import pytest

from test_abi import HEADER, declared_symbols

E_SHAPE, E_WORKSPACE, E_UNSUPPORTED = -1, -3, -5
NO_IGNORE = -(2 ** 31)
NEW = ["mednet_confusion_ws_bytes", "mednet_confusion", "mednet_surface_mask", "mednet_edt_sq", "mednet_surface_stats_ws_bytes",
       "mednet_surface_stats"]
NAN, INF = float("nan"), float("inf")
BAD_EXTENTS = [(0, 4, 4), (4, 0, 4), (4, 4, 0), (2049, 4, 4), (4, 2049, 4), (4, 4, 2049), (-1, 4, 4)]


@pytest.fixture(scope="module")
def L():
    from mednet_hip import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def p():
    """A non-null, 16-byte aligned pointer: the calls below stop before anything is read."""
    buf = (ctypes.c_double * 8)()
    yield (ctypes.addressof(buf) + 15) // 16 * 16


def _msg(L):
    return L.lib().mednet_last_error().decode()


def _confusion(lib, pred, label, counts, ws, shape=(4, 5, 6), ncls=3, ws_bytes=None):
    need = lib.mednet_confusion_ws_bytes(*shape, ncls)
    return lib.mednet_confusion(pred, label, *shape, ncls, NO_IGNORE, counts, ws, need if ws_bytes is None else ws_bytes, None)


def _mask(lib, vol, out, vol2=None, out2=None, cls=1, shape=(4, 5, 6)):
    return lib.mednet_surface_mask(vol, out, vol2, out2, cls, *shape, None)


def _edt(lib, seed, out, shape=(4, 5, 6), spacing=(1.0, 1.0, 1.0)):
    return lib.mednet_edt_sq(seed, out, *shape, *spacing, None)


def _stats(lib, surf, d2, counts, mx, sm, ws, shape=(4, 5, 6), tol_sq=1.0, ws_bytes=None):
    need = lib.mednet_surface_stats_ws_bytes(*shape)
    return lib.mednet_surface_stats(surf, d2, *shape, tol_sq, counts, mx, sm, ws, need if ws_bytes is None else ws_bytes, None)


def test_new_symbols_are_declared_exported_and_bound(L):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = declared_symbols()
    h = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in syms, f"{name}: not in the header"
        assert hasattr(h, name), f"{name}: not exported"
        assert name in L.SIGNATURES, f"{name}: not in the ctypes table"
        m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert len(m.group(1).split(",")) == len(L.SIGNATURES[name][1]), name
    assert L.lib().mednet_abi_version() == 3


def test_workspace_queries_follow_the_plan(L):
    """One row per workgroup of 4096 voxels up to 2048 rows; a confusion row holds ncls^2 + 1 uint32, a statistics row 28 bytes."""
    lib = L.lib()
    for shape, rows in (((1, 1, 1), 1), ((1, 64, 64), 1), ((1, 1, 2048), 1), ((1, 2, 2048), 1), ((1, 17, 241), 2), ((17, 9, 70), 3),
                        ((2047, 64, 64), 2047), ((2048, 64, 64), 2048), ((2048, 2048, 2048), 2048)):
        assert lib.mednet_surface_stats_ws_bytes(*shape) == 28 * rows, shape
        for ncls in (1, 2, 5, 32):
            assert lib.mednet_confusion_ws_bytes(*shape, ncls) == 4 * (ncls * ncls + 1) * rows, (shape, ncls)
    for shape in BAD_EXTENTS:
        assert lib.mednet_surface_stats_ws_bytes(*shape) == 0 and lib.mednet_confusion_ws_bytes(*shape, 3) == 0, shape
    assert lib.mednet_confusion_ws_bytes(4, 4, 4, 0) == 0 and lib.mednet_confusion_ws_bytes(4, 4, 4, 33) == 0


def test_null_pointers(L, p):
    lib = L.lib()
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert _confusion(lib, *args) == E_SHAPE and _msg(L).startswith("confusion: null pointer"), _msg(L)
    for args in ((None, p), (p, None), (p, p, p, None), (p, p, None, p)):
        assert _mask(lib, *args) == E_SHAPE and _msg(L).startswith("surface_mask: null pointer"), _msg(L)
    for args in ((None, p), (p, None)):
        assert _edt(lib, *args) == E_SHAPE and _msg(L).startswith("edt_sq: null pointer"), _msg(L)
    for k in range(6):
        args = [p] * 6
        args[k] = None
        assert _stats(lib, *args) == E_SHAPE and _msg(L).startswith("surface_stats: null pointer"), _msg(L)


def test_extents_outside_1_to_2048(L, p):
    lib = L.lib()
    for shape in BAD_EXTENTS:
        assert _confusion(lib, p, p, p, p, shape=shape, ws_bytes=1 << 20) == E_SHAPE and _msg(L).startswith("confusion: extents"), _msg(L)
        assert _mask(lib, p, p, shape=shape) == E_SHAPE and _msg(L).startswith("surface_mask: extents"), _msg(L)
        assert _edt(lib, p, p, shape=shape) == E_SHAPE and _msg(L).startswith("edt_sq: extents"), _msg(L)
        assert _stats(lib, p, p, p, p, p, p, shape=shape, ws_bytes=1 << 20) == E_SHAPE and _msg(L).startswith("surface_stats: extents"), _msg(L)


def test_class_counts_and_classes_out_of_range(L, p):
    lib = L.lib()
    for ncls in (0, -1):
        assert _confusion(lib, p, p, p, p, ncls=ncls, ws_bytes=1 << 20) == E_SHAPE and _msg(L).startswith("confusion: ncls"), _msg(L)
    for ncls in (33, 256):
        assert _confusion(lib, p, p, p, p, ncls=ncls, ws_bytes=1 << 20) == E_UNSUPPORTED and _msg(L).startswith("confusion: ncls"), _msg(L)
    for cls in (-1, 256):
        assert _mask(lib, p, p, cls=cls) == E_SHAPE and _msg(L).startswith("surface_mask: class"), _msg(L)


def test_spacing_and_tolerance(L, p):
    lib = L.lib()
    for bad in (0.0, -1.0, NAN, INF, -INF):
        for k in range(3):
            spacing = [1.0, 1.0, 1.0]
            spacing[k] = bad
            assert _edt(lib, p, p, spacing=spacing) == E_SHAPE and _msg(L).startswith("edt_sq: spacing"), (_msg(L), spacing)
    for tol_sq in (-1.0, -0.0001, NAN):
        assert _stats(lib, p, p, p, p, p, p, tol_sq=tol_sq) == E_SHAPE and _msg(L).startswith("surface_stats: squared tolerance"), _msg(L)


def test_undersized_workspaces(L, p):
    lib = L.lib()
    need = lib.mednet_confusion_ws_bytes(17, 9, 70, 5)
    assert need == 4 * 26 * 3
    assert _confusion(lib, p, p, p, p, shape=(17, 9, 70), ncls=5, ws_bytes=need - 1) == E_WORKSPACE and _msg(L).startswith("confusion: workspace"), _msg(L)
    need = lib.mednet_surface_stats_ws_bytes(17, 9, 70)
    assert need == 28 * 3
    assert _stats(lib, p, p, p, p, p, p, shape=(17, 9, 70), ws_bytes=need - 1) == E_WORKSPACE and _msg(L).startswith("surface_stats: workspace"), _msg(L)
