"""The C ABI of the degradation entries (additive to ABI 3), without a GPU: both symbols are in the header, the library and the ctypes
table with matching argument counts, and every refusal returns its code with a message under the entry's own name before anything
is launched."""
import ctypes
import re

import pytest

from test_abi import HEADER, declared_symbols

E_SHAPE = -1
NEW = ["mednet_noise_patches", "mednet_filter_rows"]
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


def _noise(lib, p, data=0, std=0, seed=1, rows=3, spatial=210):
    data, std = (p if v == 0 else v for v in (data, std))
    return lib.mednet_noise_patches(data, std, seed, rows, spatial, None)


def _filter(lib, p, src=0, dst=0, rows=3, shape=(4, 5, 6), axis=1, tab=(0, 0, 0, 0), n_tables=2, taps=4):
    src = p if src == 0 else src
    dst = p + 64 if dst == 0 else dst
    t = [p if v == 0 else v for v in tab]
    return lib.mednet_filter_rows(src, dst, rows, *shape, axis, t[0], n_tables, t[1], t[2], t[3], taps, None)


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
    assert len(L.SIGNATURES["mednet_noise_patches"][1]) == 6 and len(L.SIGNATURES["mednet_filter_rows"][1]) == 14
    assert L.SIGNATURES["mednet_noise_patches"][1][2] is ctypes.c_uint64
    assert L.lib().mednet_abi_version() == 3


def test_noise_refusals(L, p):
    lib = L.lib()
    assert _noise(lib, p, data=None) == E_SHAPE and _msg(L).startswith("noise_patches: null pointer"), _msg(L)
    assert _noise(lib, p, std=None) == E_SHAPE and _msg(L).startswith("noise_patches: null pointer"), _msg(L)
    for rows in (0, -1):
        assert _noise(lib, p, rows=rows) == E_SHAPE and _msg(L).startswith("noise_patches: rows"), _msg(L)
    assert _noise(lib, p, spatial=0) == E_SHAPE and _msg(L).startswith("noise_patches: spatial"), _msg(L)
    for spatial in (2 ** 32, 2 ** 32 + 5, 2 ** 40):
        assert _noise(lib, p, spatial=spatial) == E_SHAPE and _msg(L).startswith("noise_patches:") and "32-bit index" in _msg(L), _msg(L)
    for off in (1, 2, 3):
        assert _noise(lib, p, std=p + off) == E_SHAPE and _msg(L).startswith("noise_patches: std"), _msg(L)


def test_filter_null_pointers_and_alignment(L, p):
    lib = L.lib()
    assert _filter(lib, p, src=None) == E_SHAPE and _msg(L).startswith("filter_rows: null pointer"), _msg(L)
    assert _filter(lib, p, dst=None) == E_SHAPE and _msg(L).startswith("filter_rows: null pointer"), _msg(L)
    for k in range(4):
        tab = [0, 0, 0, 0]
        tab[k] = None
        assert _filter(lib, p, tab=tab) == E_SHAPE and _msg(L).startswith("filter_rows: null pointer"), _msg(L)
        for off in (1, 2, 3):
            tab[k] = p + off
            assert _filter(lib, p, tab=tab) == E_SHAPE and _msg(L).startswith("filter_rows: tables not 4-byte aligned"), _msg(L)
    assert _filter(lib, p, src=p, dst=p) == E_SHAPE and _msg(L).startswith("filter_rows: src == dst"), _msg(L)


def test_filter_extents_axis_rows_tables_taps(L, p):
    lib = L.lib()
    for shape in BAD_EXTENTS:
        assert _filter(lib, p, shape=shape) == E_SHAPE and _msg(L).startswith("filter_rows: extents"), _msg(L)
    for shape in TOO_MANY:
        assert _filter(lib, p, shape=shape) == E_SHAPE and _msg(L).startswith("filter_rows:") and "32-bit index" in _msg(L), _msg(L)
    for axis in (-1, 3, 7):
        assert _filter(lib, p, axis=axis) == E_SHAPE and _msg(L).startswith("filter_rows: axis"), _msg(L)
    for rows in (0, -2):
        assert _filter(lib, p, rows=rows) == E_SHAPE and _msg(L).startswith("filter_rows: rows"), _msg(L)
    for n_tables in (0, -1):
        assert _filter(lib, p, n_tables=n_tables) == E_SHAPE and _msg(L).startswith("filter_rows: n_tables"), _msg(L)
    for taps in (0, -1, 65, 1 << 20):
        assert _filter(lib, p, taps=taps) == E_SHAPE and _msg(L).startswith("filter_rows: taps"), _msg(L)
