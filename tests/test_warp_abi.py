"""The C ABI of the spatial augmentation (additive to ABI 3), without a GPU: mednet_warp_patches is in the header, the library and
the ctypes table with matching argument counts and enum values, mednet_crop_patches keeps its signature, and every refusal returns its
code and its message under `warp_patches:` before anything is launched."""
import ctypes
import re

import pytest

from test_abi import HEADER, declared_symbols

E_SHAPE, E_DTYPE, E_UNSUPPORTED = -1, -2, -5
F32, BF16, F16, U8, I64 = 0, 1, 2, 3, 4
LINEAR, NEAREST, CONSTANT, EDGE = 0, 1, 0, 1


@pytest.fixture(scope="module")
def L():
    from mednet_hip import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def p():
    """A non-null pointer: the calls below stop before anything is read."""
    buf = (ctypes.c_double * 4)()
    yield ctypes.addressof(buf)


def _msg(L):
    return L.lib().mednet_last_error().decode()


def _warp(L, p, **kw):
    a = dict(src=p, src_dtype=F16, affine=p, disp=None, gd=0, gh=0, gw=0, slot=p, count=3, out=p, dst_dtype=F32, c=2, d=9, h=11, w=13,
             c_total=4, c_off=1, pd=4, ph=5, pw=7, interp=LINEAR, border=EDGE, cval=0.0)
    a.update(kw)
    return L.lib().mednet_warp_patches(a["src"], a["src_dtype"], a["affine"], a["disp"], a["gd"], a["gh"], a["gw"], a["slot"], a["count"],
                                       a["out"], a["dst_dtype"], a["c"], a["d"], a["h"], a["w"], a["c_total"], a["c_off"], a["pd"], a["ph"],
                                       a["pw"], a["interp"], a["border"], a["cval"], None)


def test_the_symbol_is_declared_exported_and_bound(L):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    name = "mednet_warp_patches"
    assert name in declared_symbols(), "not in the header"
    assert hasattr(ctypes.CDLL(L.LIB_PATH), name), "not exported"
    assert name in L.SIGNATURES, "not in the ctypes table"
    m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert len(m.group(1).split(",")) == 24 == len(L.SIGNATURES[name][1])
    assert (L.INTERP_LINEAR, L.INTERP_NEAREST, L.BORDER_CONSTANT, L.BORDER_EDGE) == (0, 1, 0, 1)
    for enum, value in (("MEDNET_INTERP_LINEAR", 0), ("MEDNET_INTERP_NEAREST", 1), ("MEDNET_BORDER_CONSTANT", 0), ("MEDNET_BORDER_EDGE", 1)):
        assert re.search(enum + r"\s*=\s*%d\b" % value, text), enum
    assert L.lib().mednet_abi_version() == 3
    old = re.search(r"\bmednet_crop_patches\s*\((.*?)\)\s*;", text, flags=re.S)
    assert len(old.group(1).split(",")) == 17 == len(L.SIGNATURES["mednet_crop_patches"][1])   # the crop keeps its signature


def test_null_pointers_counts_and_extents_are_shape_errors(L, p):
    for kw in (dict(src=None), dict(affine=None), dict(slot=None), dict(out=None)):
        assert _warp(L, p, **kw) == E_SHAPE and _msg(L).startswith("warp_patches: null pointer"), _msg(L)
    for kw in (dict(count=0), dict(count=-1), dict(c=0), dict(d=0), dict(h=-3), dict(w=0), dict(pd=0), dict(ph=0), dict(pw=-1)):
        assert _warp(L, p, **kw) == E_SHAPE and _msg(L).startswith("warp_patches: bad shape"), (kw, _msg(L))
    for kw in (dict(c_off=3), dict(c_total=2), dict(c_off=-1)):
        assert _warp(L, p, **kw) == E_SHAPE and _msg(L).startswith("warp_patches: channels"), (kw, _msg(L))
    assert _warp(L, p, count=65536) == E_SHAPE and _msg(L).startswith("warp_patches: count 65536"), _msg(L)


def test_a_lattice_needs_two_points_per_axis(L, p):
    for g in ((1, 3, 3), (3, 1, 3), (3, 3, 1), (0, 0, 0), (2, 2, -2), (2 ** 24 - 1, 2, 2), (2, 2 ** 31 - 1, 2), (2, 2, 2 ** 24)):
        rc = _warp(L, p, disp=p, gd=g[0], gh=g[1], gw=g[2])
        assert rc == E_SHAPE and _msg(L).startswith("warp_patches: lattice"), (g, _msg(L))
    assert _warp(L, p, disp=None, gd=1, gh=1, gw=1, interp=7) == E_UNSUPPORTED    # no lattice: its extents are not looked at


def test_unknown_interpolation_border_and_dtype_pairs(L, p):
    for interp in (2, -1):
        assert _warp(L, p, interp=interp) == E_UNSUPPORTED and _msg(L).startswith("warp_patches: interpolation"), _msg(L)
    for border in (2, -1):
        assert _warp(L, p, border=border) == E_UNSUPPORTED and _msg(L).startswith("warp_patches: border"), _msg(L)
    ok = {(F16, F32), (F32, F32), (U8, U8)}
    for s in (F32, BF16, F16, U8, I64, 9):
        for d in (F32, BF16, F16, U8, I64):
            if (s, d) not in ok:
                assert _warp(L, p, src_dtype=s, dst_dtype=d) == E_DTYPE and _msg(L).startswith("warp_patches: %d -> %d" % (s, d)), _msg(L)
    # a cval that is no byte cannot be converted for the u8 pair (either interpolation, either border); the float pairs take any
    for cval in (-1.0, 255.5, 1e9, float("nan"), float("inf")):
        for interp in (LINEAR, NEAREST):
            rc = _warp(L, p, src_dtype=U8, dst_dtype=U8, cval=cval, interp=interp, border=CONSTANT)
            assert rc == E_UNSUPPORTED and _msg(L).startswith("warp_patches: cval"), (cval, _msg(L))
    # an extent for which n + 1 is no fp32 number any more
    for kw in (dict(d=2 ** 24 - 1), dict(h=2 ** 24), dict(w=2 ** 30), dict(pd=2 ** 24 - 1), dict(ph=2 ** 25), dict(pw=2 ** 24)):
        assert _warp(L, p, **kw) == E_SHAPE and _msg(L).startswith("warp_patches: bad shape"), (kw, _msg(L))
    # the order of the table: an unknown mode is reported before the dtype pair, the row limit last
    assert _warp(L, p, interp=5, src_dtype=BF16) == E_UNSUPPORTED
    assert _warp(L, p, count=70000, src_dtype=BF16) == E_DTYPE
