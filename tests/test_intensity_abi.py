"""The C ABI of the intensity entries (additive to ABI 3), without a GPU: every symbol is in the header, the library and the ctypes
table with matching argument counts, and every refusal returns its code with a message under the entry's own name before anything
is launched -- the pointers below are host addresses that are never read."""
import ctypes
import re

import pytest

from test_abi import HEADER, declared_symbols

E_SHAPE, E_DTYPE, E_WORKSPACE = -1, -2, -3
F32, BF16, F16, U8, I64, I16 = 0, 1, 2, 3, 4, 5
SOURCES = (F32, F16, I16, U8)
NEW = {"mednet_intensity_select_ws_bytes": 2, "mednet_intensity_select": 16, "mednet_intensity_moments_ws_bytes": 4,
       "mednet_intensity_moments": 13, "mednet_intensity_ranks": 10, "mednet_intensity_params": 10, "mednet_intensity_apply": 12,
       "mednet_nonzero_mask": 9}
BAD_EXTENTS = [(0, 4, 4), (4, 0, 4), (4, 4, 0), (2049, 4, 4), (4, 2049, 4), (4, 4, 2049), (-1, 4, 4)]
TOO_MANY = [(2048, 2048, 512), (512, 2048, 2048), (2048, 2048, 2048)]      # d * h * w >= 2^31
BIG = 1 << 40


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


def _or(v, p):
    return p if v == 0 else v


def _select(lib, p, src=0, mask=0, ranks=0, out=0, counts=0, ws=0, dt=F32, c=2, shape=(4, 5, 6), nr=4, level=-1, flags=0, ws_bytes=BIG):
    return lib.mednet_intensity_select(_or(src, p), dt, _or(mask, p), c, *shape, _or(ranks, p), nr, _or(out, p), _or(counts, p), level,
                                       flags, _or(ws, p), ws_bytes, None)


def _moments(lib, p, src=0, mask=0, table=0, ws=0, dt=F32, c=2, shape=(4, 5, 6), pss=-1, flags=0, ws_bytes=BIG):
    return lib.mednet_intensity_moments(_or(src, p), dt, _or(mask, p), c, *shape, pss, flags, _or(table, p), _or(ws, p), ws_bytes, None)


def _ranks(lib, p, table=0, ranks=0, frac=0, c=2, q=(0.5, 99.5, 0, 0), nq=2):
    return lib.mednet_intensity_ranks(_or(table, p), c, *q, nq, _or(ranks, p), _or(frac, p), None)


def _params(lib, p, scheme=1, table=0, order=0, frac=0, pct=0, out=0, nq=2, c=2, eps=1e-8):
    return lib.mednet_intensity_params(scheme, _or(table, p), _or(order, p), _or(frac, p), nq, c, eps, _or(pct, p), _or(out, p), None)


def _apply(lib, p, src=0, dst=0, mask=0, table=0, sdt=F32, ddt=F16, c=2, shape=(4, 5, 6)):
    return lib.mednet_intensity_apply(_or(src, p), sdt, p + 64 if dst == 0 else dst, ddt, _or(mask, p), c, *shape, _or(table, p), 0.0, None)


def _nonzero(lib, p, src=0, mask=0, box=0, dt=F32, c=2, shape=(4, 5, 6)):
    return lib.mednet_nonzero_mask(_or(src, p), dt, c, *shape, _or(mask, p), _or(box, p), None)


VOLUME_ENTRIES = (("intensity_select", _select), ("intensity_moments", _moments), ("intensity_apply", _apply), ("nonzero_mask", _nonzero))


def test_new_symbols_are_declared_exported_and_bound(L):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = declared_symbols()
    h = ctypes.CDLL(L.LIB_PATH)
    for name, nargs in NEW.items():
        assert name in syms, f"{name}: not in the header"
        assert hasattr(h, name), f"{name}: not exported"
        assert name in L.SIGNATURES, f"{name}: not in the ctypes table"
        m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert len(m.group(1).split(",")) == len(L.SIGNATURES[name][1]) == nargs, name
    assert L.lib().mednet_abi_version() == 3
    assert re.search(r"MEDNET_I16\s*=\s*5", text) and L.I16 == I16
    assert re.search(r"MEDNET_INTENSITY_MAX_RANKS\s*=\s*8", text) and L.INTENSITY_MAX_RANKS == 8


def test_null_pointers(L, p):
    lib = L.lib()
    for name, call, required in (("intensity_select", _select, ("src", "ranks", "out", "ws")),
                                 ("intensity_moments", _moments, ("src", "table", "ws")),
                                 ("intensity_ranks", _ranks, ("table", "ranks", "frac")),
                                 ("intensity_params", _params, ("table", "order", "frac", "out")),
                                 ("intensity_apply", _apply, ("src", "dst", "table")),
                                 ("nonzero_mask", _nonzero, ("src", "mask", "box"))):
        for arg in required:
            assert call(lib, p, **{arg: None}) == E_SHAPE and _msg(L).startswith(f"{name}: null pointer"), (name, arg, _msg(L))
    assert _params(lib, p, scheme=3, pct=None) == E_SHAPE and _msg(L).startswith("intensity_params: null pointer")


def test_extents_and_channels(L, p):
    lib = L.lib()
    for name, call in VOLUME_ENTRIES:
        for shape in BAD_EXTENTS:
            assert call(lib, p, shape=shape) == E_SHAPE and _msg(L).startswith(f"{name}: extents"), _msg(L)
        for shape in TOO_MANY:
            assert call(lib, p, shape=shape) == E_SHAPE and "32-bit index" in _msg(L) and _msg(L).startswith(f"{name}:"), _msg(L)
        for c in (0, -2):
            assert call(lib, p, c=c) == E_SHAPE and _msg(L).startswith(f"{name}: channels"), _msg(L)
    for c in (0, -2):
        assert _ranks(lib, p, c=c) == E_SHAPE and _msg(L).startswith("intensity_ranks: channels"), _msg(L)
        assert _params(lib, p, c=c) == E_SHAPE and _msg(L).startswith("intensity_params: channels"), _msg(L)
    assert lib.mednet_intensity_moments_ws_bytes(2, 0, 4, 4) == 0 and lib.mednet_intensity_moments_ws_bytes(0, 4, 4, 4) == 0
    assert lib.mednet_intensity_moments_ws_bytes(1, 2048, 2048, 512) == 0


def test_dtypes(L, p):
    lib = L.lib()
    for dt in (BF16, I64, 6, -1):
        assert _select(lib, p, dt=dt) == E_DTYPE and _msg(L).startswith("intensity_select: dtype"), _msg(L)
        assert _moments(lib, p, dt=dt) == E_DTYPE and _msg(L).startswith("intensity_moments: dtype"), _msg(L)
        assert _nonzero(lib, p, dt=dt) == E_DTYPE and _msg(L).startswith("nonzero_mask: dtype"), _msg(L)
        assert _apply(lib, p, sdt=dt) == E_DTYPE and _msg(L).startswith("intensity_apply: dtype"), _msg(L)
    for dt in (BF16, U8, I64, I16, 6, -1):
        assert _apply(lib, p, ddt=dt) == E_DTYPE and _msg(L).startswith("intensity_apply: dtype"), _msg(L)
    # in place with two dtypes
    assert _apply(lib, p, dst=p, sdt=F32, ddt=F16) == E_DTYPE and "in place" in _msg(L)


def test_ranks_levels_passes_schemes_percentiles(L, p):
    lib = L.lib()
    for nr in (0, -1, 9, 1 << 20):
        assert _select(lib, p, nr=nr) == E_SHAPE and _msg(L).startswith("intensity_select: ranks"), _msg(L)
        assert lib.mednet_intensity_select_ws_bytes(2, nr) == 0
    assert lib.mednet_intensity_select_ws_bytes(0, 4) == 0
    for level in (-2, 3, 11):
        assert _select(lib, p, level=level) == E_SHAPE and _msg(L).startswith("intensity_select: level"), _msg(L)
    for pss in (-2, 2):
        assert _moments(lib, p, pss=pss) == E_SHAPE and _msg(L).startswith("intensity_moments: pass"), _msg(L)
    for nq in (0, 5, -1):
        assert _ranks(lib, p, nq=nq) == E_SHAPE and _msg(L).startswith("intensity_ranks: percentiles"), _msg(L)
    for q in (-0.5, 100.5, float("nan")):
        assert _ranks(lib, p, q=(50.0, q, 0, 0)) == E_SHAPE and _msg(L).startswith("intensity_ranks: percentile "), _msg(L)
    for scheme in (-1, 4):
        assert _params(lib, p, scheme=scheme) == E_SHAPE and _msg(L).startswith("intensity_params: scheme"), _msg(L)
    for scheme, nq in ((1, 1), (2, 1), (1, 5), (3, 0), (3, 5)):
        assert _params(lib, p, scheme=scheme, nq=nq) == E_SHAPE and _msg(L).startswith("intensity_params: percentiles"), _msg(L)
    assert _params(lib, p, eps=-1.0) == E_SHAPE and _msg(L).startswith("intensity_params: eps"), _msg(L)


def test_misaligned_tables(L, p):
    lib = L.lib()
    for off in (1, 2, 4):
        for arg in ("ranks", "counts", "ws"):
            assert _select(lib, p, **{arg: p + off}) == E_SHAPE and _msg(L).startswith("intensity_select: misaligned"), _msg(L)
        for arg in ("table", "ws"):
            assert _moments(lib, p, **{arg: p + off}) == E_SHAPE and _msg(L).startswith("intensity_moments: misaligned"), _msg(L)
        for arg in ("table", "ranks", "frac"):
            assert _ranks(lib, p, **{arg: p + off}) == E_SHAPE and _msg(L).startswith("intensity_ranks: misaligned"), _msg(L)
        for arg in ("table", "frac", "pct"):
            assert _params(lib, p, **{arg: p + off}) == E_SHAPE and _msg(L).startswith("intensity_params: misaligned"), _msg(L)
    for off in (1, 2, 3):
        assert _select(lib, p, out=p + off) == E_SHAPE and _msg(L).startswith("intensity_select: misaligned"), _msg(L)
        assert _params(lib, p, order=p + off) == E_SHAPE and _msg(L).startswith("intensity_params: misaligned"), _msg(L)
        assert _params(lib, p, out=p + off) == E_SHAPE and _msg(L).startswith("intensity_params: misaligned"), _msg(L)
        assert _apply(lib, p, table=p + off) == E_SHAPE and _msg(L).startswith("intensity_apply: misaligned"), _msg(L)
        assert _nonzero(lib, p, box=p + off) == E_SHAPE and _msg(L).startswith("nonzero_mask: misaligned"), _msg(L)
    # a source at an address its own type cannot have
    assert _select(lib, p, src=p + 2) == E_SHAPE and _moments(lib, p, src=p + 1, dt=I16) == E_SHAPE
    assert _apply(lib, p, src=p + 1, sdt=F16) == E_SHAPE and _nonzero(lib, p, src=p + 2) == E_SHAPE
    assert _select(lib, p, src=p + 1, dt=U8, ws_bytes=0) == E_WORKSPACE          # (u8 lies anywhere: the next check answers)


def test_undersized_workspaces(L, p):
    lib = L.lib()
    for c, nr in ((1, 1), (2, 4), (4, 8)):
        need = lib.mednet_intensity_select_ws_bytes(c, nr)
        assert need >= c * nr * 2048 * 8
        for have in (0, need - 1):
            assert _select(lib, p, c=c, nr=nr, ws_bytes=have) == E_WORKSPACE and _msg(L).startswith("intensity_select: workspace"), _msg(L)
    for c, shape in ((1, (5, 6, 7)), (3, (17, 19, 13)), (2, (208, 208, 200))):
        need = lib.mednet_intensity_moments_ws_bytes(c, *shape)
        assert need > 0
        for have in (0, need - 1):
            assert _moments(lib, p, c=c, shape=shape, ws_bytes=have) == E_WORKSPACE and _msg(L).startswith("intensity_moments: workspace")
