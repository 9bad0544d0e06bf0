"""The C ABI of the optimiser entries (additive to ABI 3), without a GPU: every new symbol is in the header, the library and the ctypes
table with matching argument counts, the two Adam entries keep theirs, the workspace query follows the plan, and every refusal returns
its code with a message under the entry's own name before anything is launched."""
import ctypes
import re

import pytest

from test_abi import HEADER, declared_symbols

E_SHAPE, E_WORKSPACE = -1, -3
NEW = ["mednet_grad_norm_ws_bytes", "mednet_grad_norm", "mednet_sgd_step", "mednet_adamw_step"]


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


def _norm(lib, g, ost, ws, count=1025, max_norm=1.0, ws_bytes=None, sc=None):
    need = lib.mednet_grad_norm_ws_bytes(count)
    return lib.mednet_grad_norm(g, count, 1.0, sc, max_norm, ost, ws, need if ws_bytes is None else ws_bytes, None)


def _sgd(lib, p_, g, buf, ost, count=1025, lr=0.1, mu=0.9, nesterov=0, wd=0.0, sc=None, interval=2000):
    return lib.mednet_sgd_step(p_, g, buf, count, lr, mu, nesterov, wd, 1.0, ost, sc, 2.0, 0.5, interval, None)


def _adamw(lib, p_, g, m, v, ost, count=1025, lr=1e-3, wd=0.0, sc=None, interval=2000):
    return lib.mednet_adamw_step(p_, g, m, v, count, lr, 0.9, 0.999, 1e-8, wd, 1, 1.0, ost, sc, 2.0, 0.5, interval, None)


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
    for name, n in (("mednet_adam_step", 13), ("mednet_adam_step_scaled", 16)):      # the old entries keep their signatures
        old = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert len(old.group(1).split(",")) == n == len(L.SIGNATURES[name][1]), name


def test_workspace_query_follows_the_plan(L):
    lib = L.lib()
    for count, rows in ((1, 1), (4096, 1), (4097, 2), (2047 * 4096, 2047), (2047 * 4096 + 1, 2048), (1 << 33, 2048)):
        assert lib.mednet_grad_norm_ws_bytes(count) == 4 * rows, count
    assert lib.mednet_grad_norm_ws_bytes(0) == 0


def test_null_pointers_and_an_empty_buffer(L, p):
    lib = L.lib()
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert _norm(lib, *args) == E_SHAPE and _msg(L).startswith("grad_norm: null pointer"), _msg(L)
    assert _norm(lib, p, p, p, count=0) == E_SHAPE and _msg(L).startswith("grad_norm: count"), _msg(L)
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p)):
        assert _sgd(lib, *args) == E_SHAPE and _msg(L).startswith("sgd_step: null pointer"), _msg(L)
    assert _sgd(lib, p, p, p, None, sc=p) == E_SHAPE and _msg(L).startswith("sgd_step: null pointer"), _msg(L)
    assert _sgd(lib, p, p, p, p, count=0) == E_SHAPE and _msg(L).startswith("sgd_step: count"), _msg(L)
    for args in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None)):
        assert _adamw(lib, *args) == E_SHAPE and _msg(L).startswith("adamw_step: null pointer"), _msg(L)
    assert _adamw(lib, p, p, p, p, p, count=0) == E_SHAPE and _msg(L).startswith("adamw_step: count"), _msg(L)


def test_undersized_workspace(L, p):
    lib = L.lib()
    need = lib.mednet_grad_norm_ws_bytes(70001)
    assert need == 4 * 18
    rc = _norm(lib, p, p, p, count=70001, ws_bytes=need - 1)
    assert rc == E_WORKSPACE and _msg(L).startswith("grad_norm: workspace"), _msg(L)


def test_hyper_parameters_out_of_range(L, p):
    lib = L.lib()
    nan = float("nan")
    for mu in (-0.1, 1.0, 1.5, nan):
        assert _sgd(lib, p, p, p, p, mu=mu) == E_SHAPE and _msg(L).startswith("sgd_step: momentum"), _msg(L)
    for kw in (dict(lr=-1e-3), dict(wd=-1e-5), dict(lr=nan)):
        assert _sgd(lib, p, p, p, p, **kw) == E_SHAPE and _msg(L).startswith("sgd_step: negative"), _msg(L)
        assert _adamw(lib, p, p, p, p, p, **kw) == E_SHAPE and _msg(L).startswith("adamw_step: negative"), _msg(L)
    for max_norm in (-1.0, nan):
        assert _norm(lib, p, p, p, max_norm=max_norm) == E_SHAPE and _msg(L).startswith("grad_norm: max_norm"), _msg(L)
    assert _sgd(lib, p, p, None, p, mu=0.0, nesterov=1) == E_SHAPE and _msg(L).startswith("sgd_step: nesterov"), _msg(L)
    assert _sgd(lib, p, p, p, p, sc=p, interval=0) == E_SHAPE and _msg(L).startswith("sgd_step: growth_interval"), _msg(L)
    assert _adamw(lib, p, p, p, p, p, sc=p, interval=0) == E_SHAPE and _msg(L).startswith("adamw_step: growth_interval"), _msg(L)
