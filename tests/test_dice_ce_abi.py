"""The C ABI of the Dice + cross-entropy class loss (additive to ABI 3), without a GPU: every new symbol is in the header, the library
and the ctypes table with matching argument counts; the new entries answer null pointers with MEDNET_E_SHAPE under their own name;
class kind 2 is a softmax form without ignore_index everywhere it is accepted, and kind 3 is still refused."""
import ctypes
import re

import pytest

from test_abi import HEADER, declared_symbols

E_SHAPE, E_UNSUPPORTED = -1, -5
NEW = ["mednet_dice_ce_ws_bytes", "mednet_dice_ce_fwd_lt", "mednet_dice_ce_bwd_lt", "mednet_head_dice_ce_supported",
       "mednet_head_dice_ce_ws_bytes", "mednet_head_dice_ce_gn_rows", "mednet_head_dice_ce_fwd", "mednet_head_dice_ce_bwd"]
BF16, U8 = 1, 3
SP = 720  # voxels (a multiple of 4: the matrix-core heads take it)


@pytest.fixture(scope="module")
def L():
    from mednet_hip import _lib
    _lib.lib()
    return _lib


def _msg(L):
    return L.lib().mednet_last_error().decode()


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
    assert L.CLASS_DICE_CE == 2 and re.search(r"MEDNET_CLASS_DICE_CE\s*=\s*2\b", text)
    assert L.lib().mednet_abi_version() == 3


def test_workspace_queries_cover_the_dice_rows_and_the_ce_rows(L):
    lib = L.lib()
    for n, c, s in ((1, 1, 1), (2, 4, 2197), (3, 32, 65 * 64 * 63), (4, 14, 128 ** 3)):
        blocks = -(-s // 2048)
        assert lib.mednet_dice_ce_ws_bytes(n, c, s) == (n * blocks * (2 * c + 2) + 64) * 4
        assert lib.mednet_dice_ce_ws_bytes(n, c, s) > lib.mednet_loss_ws_bytes(n, c, s)
    for cin in (16, 32, 64):
        for cout in (1, 2, 4):
            a, b = lib.mednet_head_dice_ce_ws_bytes(2, 2048 * 3, cin, cout), lib.mednet_head_dice_ws_bytes(2, 2048 * 3, cin, cout)
            assert a >= b and a >= (2 * 3 * (2 * cout + 2) + 64) * 4
            assert lib.mednet_head_dice_ce_gn_rows(2, 2048 * 3, cin) == lib.mednet_head_dice_gn_rows(2, 2048 * 3, cin)
            for dt in (0, 1, 2):
                for lt in (3, 4):
                    assert lib.mednet_head_dice_ce_supported(cin, cout, dt, lt) == lib.mednet_head_dice_supported(cin, cout, dt, lt)
    assert lib.mednet_head_dice_ce_supported(32, 5, 1, 3) == 0


def _loss_fwd(lib, **kw):
    a = dict(logits=None, labels=None, dt=U8, lsn=SP, weight=None, loss=None, saved=None, dice=None, n=2, c=4, sp=SP, sn=4 * SP, sc=SP,
             eps=1e-5, ws=None, wsb=0)
    a.update(kw)
    return lib.mednet_dice_ce_fwd_lt(a["logits"], a["labels"], a["dt"], a["lsn"], a["weight"], a["loss"], a["saved"], a["dice"], a["n"],
                                     a["c"], a["sp"], a["sn"], a["sc"], a["eps"], a["ws"], a["wsb"], None)


def test_new_entries_answer_null_pointers_with_a_shape_error_under_their_own_name(L):
    lib = L.lib()
    assert _loss_fwd(lib) == E_SHAPE and _msg(L).startswith("dice_ce_fwd"), _msg(L)
    rc = lib.mednet_dice_ce_bwd_lt(None, None, U8, SP, None, None, None, None, 2, 4, SP, 4 * SP, SP, 1e-5, None)
    assert rc == E_SHAPE and _msg(L).startswith("dice_ce_bwd"), _msg(L)
    rc = lib.mednet_head_dice_ce_fwd(None, None, None, None, U8, SP, None, None, None, None, 2, SP, 32, 4, 1e-5, 0, L.NO_IGNORE, BF16, None,
                                     0, None)
    assert rc == E_SHAPE and _msg(L).startswith("head_dice_ce_fwd"), _msg(L)
    rc = lib.mednet_head_dice_ce_bwd(None, None, U8, SP, None, None, None, None, None, None, None, 0, None, None, None, 2, SP, 32, 4, 1e-5, 0,
                                     L.NO_IGNORE, BF16, None, 0, None)
    assert rc == E_SHAPE and _msg(L).startswith("head_dice_ce_bwd"), _msg(L)


def _head_fwd(lib, L, sigmoid, ignore):
    return lib.mednet_head_dice_ce_fwd(None, None, None, None, U8, SP, None, None, None, None, 2, SP, 32, 4, 1e-5, sigmoid, ignore, BF16, None,
                                       0, None)


def _head_bwd(lib, L, sigmoid, ignore):
    return lib.mednet_head_dice_ce_bwd(None, None, U8, SP, None, None, None, None, None, None, None, 0, None, None, None, 2, SP, 32, 4, 1e-5,
                                       sigmoid, ignore, BF16, None, 0, None)


def _seg_fwd(lib, L, kind, sigmoid, ignore):
    return lib.mednet_head_seg_fwd(None, None, None, None, SP, None, None, None, None, 2, SP, 32, 9, kind, 1e-5, sigmoid, ignore, BF16, None,
                                   0, None)


def _seg_bwd(lib, L, kind, sigmoid, ignore):
    return lib.mednet_head_seg_bwd(None, None, None, None, SP, None, None, None, None, None, 0, None, None, None, 2, SP, 32, 9, kind, 1e-5,
                                   sigmoid, ignore, BF16, None, 0, None)


def _lm_fwd(lib, L, kind, sigmoid, ignore):
    return lib.mednet_head_landmark_cls_fwd(None, None, None, None, 5 * SP, None, SP, None, None, None, None, None, None, None, 2, SP, 32, 5,
                                            3, 0, kind, 1e-5, sigmoid, ignore, BF16, None, 0, None)


def _lm_bwd(lib, L, kind, sigmoid, ignore):
    return lib.mednet_head_landmark_cls_bwd(None, None, None, None, 5 * SP, None, SP, None, None, None, None, None, None, None, 0, None,
                                            None, None, 2, SP, 32, 5, 3, 0, kind, 1e-5, sigmoid, ignore, BF16, None, 0, None)


def test_kind_two_is_a_softmax_form_without_ignore_index(L):
    """sigmoid = 1 or an ignore_index with class kind 2: MEDNET_E_UNSUPPORTED, whatever else the call holds; with neither the same
    null-pointer call gets as far as the argument check."""
    lib = L.lib()
    for fn in (_seg_fwd, _seg_bwd, _lm_fwd, _lm_bwd):
        assert fn(lib, L, 2, 1, L.NO_IGNORE) == E_UNSUPPORTED, (fn.__name__, _msg(L))
        assert fn(lib, L, 2, 0, -100) == E_UNSUPPORTED, (fn.__name__, _msg(L))
        assert fn(lib, L, 2, 0, 1) == E_UNSUPPORTED, (fn.__name__, _msg(L))
        assert fn(lib, L, 2, 0, L.NO_IGNORE) == E_SHAPE, (fn.__name__, _msg(L))
    for fn in (_head_fwd, _head_bwd):
        assert fn(lib, L, 1, L.NO_IGNORE) == E_UNSUPPORTED, (fn.__name__, _msg(L))
        assert fn(lib, L, 0, -100) == E_UNSUPPORTED, (fn.__name__, _msg(L))
        assert fn(lib, L, 0, L.NO_IGNORE) == E_SHAPE, (fn.__name__, _msg(L))


def test_kind_three_is_still_refused_and_the_old_kinds_keep_their_rules(L):
    lib = L.lib()
    for fn in (_seg_fwd, _seg_bwd, _lm_fwd, _lm_bwd):
        assert fn(lib, L, 3, 0, L.NO_IGNORE) == E_UNSUPPORTED and "class-loss kind 3" in _msg(L), (fn.__name__, _msg(L))
        assert fn(lib, L, -1, 0, L.NO_IGNORE) == E_UNSUPPORTED, fn.__name__
        assert fn(lib, L, 1, 1, -100) == E_UNSUPPORTED, fn.__name__          # cross-entropy is a softmax form
        assert fn(lib, L, 1, 0, 3) == E_SHAPE, fn.__name__                   # ... with an ignore_index
        assert fn(lib, L, 0, 1, 2) == E_SHAPE, fn.__name__                   # Dice: sigmoid and ignore_index as before


def test_class_count_and_label_type_of_the_unfused_entries(L):
    lib = L.lib()
    one = ctypes.c_float(0.0)
    p = ctypes.addressof(one)  # (a non-null pointer: the calls below stop before anything is read)
    for c in (0, 33):
        assert _loss_fwd(lib, logits=p, labels=p, loss=p, saved=p, ws=p, c=c) == E_UNSUPPORTED and _msg(L).startswith("dice_ce_fwd")
    assert _loss_fwd(lib, logits=p, labels=p, loss=p, saved=p, ws=p, dt=0) == -2  # MEDNET_E_DTYPE: labels are int64 or uint8
    assert _loss_fwd(lib, logits=p, labels=p, loss=p, saved=p, ws=p, wsb=lib.mednet_loss_ws_bytes(2, 4, SP)) == -3  # MEDNET_E_WORKSPACE
