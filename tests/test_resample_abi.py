"""The C ABI of the resampling entries (additive to ABI 3), without a GPU: both symbols are in the header, the library and the ctypes
table with matching argument counts, and every refusal returns its code with a message under the entry's own name before anything
is launched."""
import ctypes
import re

import pytest

from test_abi import HEADER, declared_symbols

E_SHAPE, E_DTYPE = -1, -2
F32, BF16, F16, U8, I64 = 0, 1, 2, 3, 4
NEW = ["mednet_resample_axis", "mednet_resample_argmax"]
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


def _axis(lib, p, src=0, dst=0, tab=(0, 0, 0), sdt=F32, ddt=F32, c=2, shape=(4, 5, 6), axis=1, n_out=7, taps=2):
    src, dst = (p if src == 0 else src), (p if dst == 0 else dst)
    tab = [p if t == 0 else t for t in tab]
    return lib.mednet_resample_axis(src, sdt, dst, ddt, c, *shape, axis, n_out, *tab, taps, None)


def _argmax(lib, p, src=0, out=0, out_max=0, tabs=(0,) * 9, dt=F32, ncls=3, shape=(4, 5, 6), size=(7, 8, 9), taps=(2, 2, 2)):
    src, out, out_max = (p if v == 0 else v for v in (src, out, out_max))
    t = [p if v == 0 else v for v in tabs]
    return lib.mednet_resample_argmax(src, dt, ncls, *shape, out, out_max, *size, t[0], t[1], t[2], taps[0], t[3], t[4], t[5], taps[1],
                                      t[6], t[7], t[8], taps[2], None)


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
    assert len(L.SIGNATURES["mednet_resample_axis"][1]) == 15 and len(L.SIGNATURES["mednet_resample_argmax"][1]) == 24
    assert L.lib().mednet_abi_version() == 3


def test_null_pointers(L, p):
    lib = L.lib()
    assert _axis(lib, p, src=None) == E_SHAPE and _msg(L).startswith("resample_axis: null pointer"), _msg(L)
    assert _axis(lib, p, dst=None) == E_SHAPE and _msg(L).startswith("resample_axis: null pointer"), _msg(L)
    for k in range(3):
        tab = [0, 0, 0]
        tab[k] = None
        assert _axis(lib, p, tab=tab) == E_SHAPE and _msg(L).startswith("resample_axis: null pointer"), _msg(L)
    assert _argmax(lib, p, src=None) == E_SHAPE and _msg(L).startswith("resample_argmax: null pointer"), _msg(L)
    assert _argmax(lib, p, out=None) == E_SHAPE and _msg(L).startswith("resample_argmax: null pointer"), _msg(L)
    for k in range(9):
        tabs = [0] * 9
        tabs[k] = None
        assert _argmax(lib, p, tabs=tabs) == E_SHAPE and _msg(L).startswith("resample_argmax: null pointer"), _msg(L)


def test_extents(L, p):
    lib = L.lib()
    for shape in BAD_EXTENTS:
        assert _axis(lib, p, shape=shape) == E_SHAPE and _msg(L).startswith("resample_axis: extents"), _msg(L)
        assert _argmax(lib, p, shape=shape) == E_SHAPE and _msg(L).startswith("resample_argmax: extents"), _msg(L)
        assert _argmax(lib, p, size=shape) == E_SHAPE and _msg(L).startswith("resample_argmax: extents"), _msg(L)
    for axis in (0, 1, 2):
        for n_out in (0, -3, 2049):
            assert _axis(lib, p, axis=axis, n_out=n_out) == E_SHAPE and _msg(L).startswith("resample_axis: extents"), _msg(L)
    for shape in TOO_MANY:
        assert _axis(lib, p, shape=shape) == E_SHAPE and "32-bit index" in _msg(L) and _msg(L).startswith("resample_axis:")
        assert _argmax(lib, p, shape=shape) == E_SHAPE and "32-bit index" in _msg(L) and _msg(L).startswith("resample_argmax:")
        assert _argmax(lib, p, size=shape) == E_SHAPE and "32-bit index" in _msg(L) and _msg(L).startswith("resample_argmax:")
    # the way out of an axis pass: 1024 x 1024 x 1024 in, axis 0 to 2048 is 2^31 voxels
    assert _axis(lib, p, shape=(1024, 1024, 1024), axis=0, n_out=2048) == E_SHAPE and "32-bit index" in _msg(L)


def test_axis_channels_taps_classes(L, p):
    lib = L.lib()
    for axis in (-1, 3, 7):
        assert _axis(lib, p, axis=axis) == E_SHAPE and _msg(L).startswith("resample_axis: axis"), _msg(L)
    for c in (0, -2):
        assert _axis(lib, p, c=c) == E_SHAPE and _msg(L).startswith("resample_axis: channels"), _msg(L)
    for taps in (0, -1, 65, 1 << 20):
        assert _axis(lib, p, taps=taps) == E_SHAPE and _msg(L).startswith("resample_axis: taps"), _msg(L)
        for k in range(3):
            t = [2, 2, 2]
            t[k] = taps
            assert _argmax(lib, p, taps=t) == E_SHAPE and _msg(L).startswith("resample_argmax: taps"), _msg(L)
    for ncls in (0, -1, 257, 1 << 16):
        assert _argmax(lib, p, ncls=ncls) == E_SHAPE and _msg(L).startswith("resample_argmax: classes"), _msg(L)


def test_dtypes(L, p):
    lib = L.lib()
    for dt in (BF16, I64, 5, -1):
        assert _axis(lib, p, sdt=dt) == E_DTYPE and _msg(L).startswith("resample_axis: dtype"), _msg(L)
        assert _axis(lib, p, ddt=dt) == E_DTYPE and _msg(L).startswith("resample_axis: dtype"), _msg(L)
        assert _argmax(lib, p, dt=dt) == E_DTYPE and _msg(L).startswith("resample_argmax: dtype"), _msg(L)


def test_misaligned_tables(L, p):
    lib = L.lib()
    for off in (1, 2, 3):
        for k in range(3):
            tab = [0, 0, 0]
            tab[k] = p + off
            assert _axis(lib, p, tab=tab) == E_SHAPE and _msg(L).startswith("resample_axis: tables not 4-byte aligned"), _msg(L)
        for k in range(9):
            tabs = [0] * 9
            tabs[k] = p + off
            assert _argmax(lib, p, tabs=tabs) == E_SHAPE and _msg(L).startswith("resample_argmax: tables"), _msg(L)
        assert _argmax(lib, p, out_max=p + off) == E_SHAPE and _msg(L).startswith("resample_argmax: tables or out_max"), _msg(L)
