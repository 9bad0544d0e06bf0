"""The C ABI of the connected-component entries (additive to ABI 3), without a GPU: every new symbol is in the header, the library
and the ctypes table with matching argument counts, the workspace query follows the plan of csrc/components.hip, and every refusal
returns its code with a message under the entry's own name before anything is launched."""
import ctypes
import re

import pytest

from test_abi import HEADER, declared_symbols

E_SHAPE, E_WORKSPACE, E_UNSUPPORTED = -1, -3, -5
CC_ALL = -1
NEW = ["mednet_cc_ws_bytes", "mednet_cc_label", "mednet_cc_stats", "mednet_cc_select"]
BAD_EXTENTS = [(0, 4, 4), (4, 0, 4), (4, 4, 0), (2049, 4, 4), (4, 2049, 4), (4, 4, 2049), (-1, 4, 4)]
TOO_MANY = [(2048, 2048, 512), (512, 2048, 2048), (2048, 2048, 2048)]      # d * h * w >= 2^31


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


def _label(lib, vol, labels, info, ws, cls=1, invert=0, conn=26, shape=(4, 5, 6), ws_bytes=None):
    need = lib.mednet_cc_ws_bytes(*shape)
    return lib.mednet_cc_label(vol, cls, invert, conn, *shape, labels, info, ws, need if ws_bytes is None else ws_bytes, None)


def _stats(lib, vol, labels, table, k=3, shape=(4, 5, 6)):
    return lib.mednet_cc_stats(vol, labels, *shape, k, table, None)


def _select(lib, vol, labels, keep, out, fill=0, shape=(4, 5, 6)):
    return lib.mednet_cc_select(vol, labels, keep, fill, out, *shape, None)


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
    assert re.search(r"#define\s+MEDNET_CC_ALL\s+\(-1\)", text) and L.CC_ALL == CC_ALL


def test_workspace_query_follows_the_plan(L):
    """One uint32 per numbering row of 4096 voxels, up to 2048 rows; 0 for illegal extents and for 2^31 voxels or more."""
    lib = L.lib()
    for shape, rows in (((1, 1, 1), 1), ((1, 64, 64), 1), ((1, 1, 2048), 1), ((1, 2, 2048), 1), ((1, 17, 241), 2), ((9, 17, 70), 3),
                        ((2047, 64, 64), 2047), ((2048, 64, 64), 2048), ((2048, 2048, 511), 2048)):
        assert lib.mednet_cc_ws_bytes(*shape) == 4 * rows, shape
    for shape in BAD_EXTENTS + TOO_MANY:
        assert lib.mednet_cc_ws_bytes(*shape) == 0, shape


def test_null_pointers(L, p):
    lib = L.lib()
    for k in range(4):
        args = [p] * 4
        args[k] = None
        assert _label(lib, *args) == E_SHAPE and _msg(L).startswith("cc_label: null pointer"), _msg(L)
        assert _select(lib, *args) == E_SHAPE and _msg(L).startswith("cc_select: null pointer"), _msg(L)
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert _stats(lib, *args) == E_SHAPE and _msg(L).startswith("cc_stats: null pointer"), _msg(L)
    assert _stats(lib, p, p, None, k=0) == 0          # no component, no table: legal, nothing is launched


def test_extents(L, p):
    lib = L.lib()
    for shape in BAD_EXTENTS:
        assert _label(lib, p, p, p, p, shape=shape, ws_bytes=1 << 20) == E_SHAPE and _msg(L).startswith("cc_label: extents"), _msg(L)
        assert _stats(lib, p, p, p, shape=shape) == E_SHAPE and _msg(L).startswith("cc_stats: extents"), _msg(L)
        assert _select(lib, p, p, p, p, shape=shape) == E_SHAPE and _msg(L).startswith("cc_select: extents"), _msg(L)
    for shape in TOO_MANY:
        assert _label(lib, p, p, p, p, shape=shape, ws_bytes=1 << 20) == E_SHAPE and "32-bit index" in _msg(L) and _msg(L).startswith("cc_label:")
        assert _stats(lib, p, p, p, shape=shape) == E_SHAPE and "32-bit index" in _msg(L) and _msg(L).startswith("cc_stats:")
        assert _select(lib, p, p, p, p, shape=shape) == E_SHAPE and "32-bit index" in _msg(L) and _msg(L).startswith("cc_select:")


def test_class_invert_connectivity_k_fill(L, p):
    lib = L.lib()
    for cls in (-2, 256, -(2 ** 31)):
        assert _label(lib, p, p, p, p, cls=cls) == E_SHAPE and _msg(L).startswith("cc_label: class"), _msg(L)
    for invert in (2, -1):
        assert _label(lib, p, p, p, p, invert=invert) == E_SHAPE and _msg(L).startswith("cc_label: invert"), _msg(L)
    assert _label(lib, p, p, p, p, cls=CC_ALL, invert=1) == E_SHAPE and _msg(L).startswith("cc_label: invert with MEDNET_CC_ALL"), _msg(L)
    for conn in (0, 4, 8, 27, -6):
        assert _label(lib, p, p, p, p, conn=conn) == E_UNSUPPORTED and _msg(L).startswith("cc_label: connectivity"), _msg(L)
    for k in (-1, -(2 ** 40)):
        assert _stats(lib, p, p, p, k=k) == E_SHAPE and _msg(L).startswith("cc_stats: k"), _msg(L)
    assert _stats(lib, p, p, p, k=4 * 5 * 6 + 1) == E_SHAPE and _msg(L).startswith("cc_stats: k"), _msg(L)
    for fill in (-1, 256):
        assert _select(lib, p, p, p, p, fill=fill) == E_SHAPE and _msg(L).startswith("cc_select: fill"), _msg(L)


def test_misaligned_pointers(L, p):
    lib = L.lib()
    for off in (1, 2, 3):
        assert _label(lib, p, p + off, p, p) == E_SHAPE and _msg(L).startswith("cc_label: labels or workspace not 4-byte"), _msg(L)
        assert _label(lib, p, p, p, p + off) == E_SHAPE and _msg(L).startswith("cc_label: labels or workspace not 4-byte"), _msg(L)
        assert _stats(lib, p, p + off, p) == E_SHAPE and _msg(L).startswith("cc_stats: labels not 4-byte"), _msg(L)
        assert _select(lib, p, p + off, p, p) == E_SHAPE and _msg(L).startswith("cc_select: labels not 4-byte"), _msg(L)
    for off in (1, 4, 7):
        assert _label(lib, p, p, p + off, p) == E_SHAPE and _msg(L).startswith("cc_label: labels or workspace not 4-byte or info"), _msg(L)
        assert _stats(lib, p, p, p + off) == E_SHAPE and _msg(L).startswith("cc_stats: labels not 4-byte or table"), _msg(L)


def test_undersized_workspace(L, p):
    lib = L.lib()
    need = lib.mednet_cc_ws_bytes(9, 17, 70)
    assert need == 12
    assert _label(lib, p, p, p, p, shape=(9, 17, 70), ws_bytes=need - 1) == E_WORKSPACE and _msg(L).startswith("cc_label: workspace"), _msg(L)
