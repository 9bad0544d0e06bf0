"""The C ABI of blended inference (additive to ABI 3), without a GPU: every new symbol is in the header, the library and the ctypes
table with matching argument counts; the entries answer null pointers with MEDNET_E_SHAPE under their own name; a mirror mask outside
0..7, an unknown class mode, a bad probability type, an undersized peaks workspace and a finalize without outputs are refused with
their own codes before anything is launched."""
import ctypes
import re

import pytest

from test_abi import HEADER, declared_symbols

E_SHAPE, E_DTYPE, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -3, -5
NEW = ["mednet_grid_gather_mirror", "mednet_blend_accumulate", "mednet_blend_finalize", "mednet_heatmap_peaks_ws_bytes",
       "mednet_heatmap_peaks"]
F32, BF16, F16, U8 = 0, 1, 2, 3


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


def _gather(lib, vol, pos, out, mirror=0, pad=0):
    return lib.mednet_grid_gather_mirror(vol, pos, out, 2, 1, 13, 19, 37, 8, 12, 16, 2, 3, 4, pad, mirror, None)


def _accumulate(lib, q, mirror=0, mode=0, logits=True, batch=2):
    return lib.mednet_blend_accumulate(q if logits else None, q, q, q, q, q, q, batch, 2, 4, 13, 19, 37, 8, 12, 16, 2, 3, 4, mirror, mode, None)


def _finalize(lib, acc, wsum, res, prob, heat, dt=F32, mode=0):
    return lib.mednet_blend_finalize(acc, wsum, res, prob, dt, heat, 2, 4, 13, 19, 37, mode, None)


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
    assert (L.BLEND_PROBABILITIES, L.BLEND_LOGITS) == (0, 1)
    assert re.search(r"MEDNET_BLEND_PROBABILITIES\s*=\s*0\b", text) and re.search(r"MEDNET_BLEND_LOGITS\s*=\s*1\b", text)
    assert L.lib().mednet_abi_version() == 3
    old = re.search(r"\bmednet_grid_gather\s*\((.*?)\)\s*;", text, flags=re.S)
    assert len(old.group(1).split(",")) == 16 == len(L.SIGNATURES["mednet_grid_gather"][1])   # the old entry keeps its signature


def test_null_pointers_are_a_shape_error_under_the_entrys_own_name(L, p):
    lib = L.lib()
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert _gather(lib, *args) == E_SHAPE and _msg(L).startswith("grid_gather_mirror:"), _msg(L)
    assert _accumulate(lib, p, logits=False) == E_SHAPE and _msg(L).startswith("blend_accumulate:"), _msg(L)
    assert _accumulate(lib, None) == E_SHAPE and _msg(L).startswith("blend_accumulate:"), _msg(L)
    assert _finalize(lib, None, p, p, p, p) == E_SHAPE and _msg(L).startswith("blend_finalize:"), _msg(L)
    assert _finalize(lib, p, None, p, p, p) == E_SHAPE and _msg(L).startswith("blend_finalize:"), _msg(L)
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        rc = lib.mednet_heatmap_peaks(args[0], 2, 70001, args[1], args[2], args[3], 1 << 20, None)
        assert rc == E_SHAPE and _msg(L).startswith("heatmap_peaks:"), _msg(L)


def test_mirror_masks_outside_0_to_7_are_refused(L, p):
    lib = L.lib()
    for mirror in (8, -1):
        assert _gather(lib, p, p, p, mirror=mirror) == E_UNSUPPORTED and _msg(L).startswith("grid_gather_mirror: mirror mask"), _msg(L)
        assert _accumulate(lib, p, mirror=mirror) == E_UNSUPPORTED and _msg(L).startswith("blend_accumulate: mirror mask"), _msg(L)
    assert _gather(lib, p, p, p, pad=2) == E_UNSUPPORTED and _msg(L).startswith("grid_gather_mirror: pad mode"), _msg(L)


def test_class_mode_probability_type_and_missing_outputs(L, p):
    lib = L.lib()
    for mode in (2, -1):
        assert _accumulate(lib, p, mode=mode) == E_UNSUPPORTED and _msg(L).startswith("blend_accumulate: class mode"), _msg(L)
        assert _finalize(lib, p, p, p, p, p, mode=mode) == E_UNSUPPORTED and _msg(L).startswith("blend_finalize: class mode"), _msg(L)
    for dt in (BF16, U8, 7):
        assert _finalize(lib, p, p, p, p, p, dt=dt) == E_DTYPE and _msg(L).startswith("blend_finalize: probability type"), _msg(L)
    assert _finalize(lib, p, p, None, None, None) == E_SHAPE and _msg(L).startswith("blend_finalize: no output"), _msg(L)
    assert _accumulate(lib, p, batch=0) == E_SHAPE and _msg(L).startswith("blend_accumulate: bad shape"), _msg(L)


def test_peaks_workspace_query_and_undersized_workspace(L, p):
    lib = L.lib()
    for nh, vox in ((1, 1), (2, 4096), (2, 4097), (2, 70001), (3, 512 ** 3)):
        assert lib.mednet_heatmap_peaks_ws_bytes(nh, vox) == nh * -(-vox // 4096) * 12
    assert lib.mednet_heatmap_peaks_ws_bytes(0, 100) == 0 and lib.mednet_heatmap_peaks_ws_bytes(2, 0) == 0
    need = lib.mednet_heatmap_peaks_ws_bytes(2, 70001)
    rc = lib.mednet_heatmap_peaks(p, 2, 70001, p, p, p, need - 1, None)
    assert rc == E_WORKSPACE and _msg(L).startswith("heatmap_peaks: workspace"), _msg(L)
    assert lib.mednet_heatmap_peaks(p, 0, 70001, p, p, p, need, None) == E_SHAPE
