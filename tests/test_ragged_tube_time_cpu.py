"""The ragged tube time entries' C ABI boundary and Python front end without a
device: the exported symbols, the workspace query and the argument checks
that return before a context or a pointer is looked at.  The non-NULL
pointers handed over are never dereferenced by a call that fails its checks.
"""
import ctypes
import os
import re

import pytest

OK, INVALID, UNSUPPORTED = 0, -1, -4
N, R = 10, 4
SYMBOLS = ("mtg_ragged_tube_time_workspace_bytes", "mtg_ragged_tube_time_cost",
           "mtg_ragged_tube_time_optimize")


@pytest.fixture(scope="module")
def L():
    import mav_tube_trajectory_generation_amd as mtg
    return mtg.lib()


@pytest.fixture(scope="module")
def buf():
    """An address that is not NULL (never read: the calls fail first)."""
    b = (ctypes.c_double * 8)()
    return ctypes.cast(b, ctypes.c_void_p), b


def _params(**kw):
    from mav_tube_trajectory_generation_amd._abi import make_time_params
    kw.setdefault("optimizer", "sbplx")
    return make_time_params(**kw)


def _cost(L, p, N=N, r=R, S_max=6, B=2, params=None, ctx=True, ptrs=True, tol=1e-10,
          max_iter=100, ws=True, ws_bytes=1 << 30):
    q = p if ptrs else None
    params = _params() if params is None else params
    pp = ctypes.byref(params) if params != "null" else None
    return L.mtg_ragged_tube_time_cost(p if ctx else None, N, r, S_max, B, q, q, q, q, q, q, tol,
                                       max_iter, pp, q, q, None, p if ws else None, ws_bytes,
                                       None)


def _opt(L, p, N=N, r=R, S_max=6, B=2, params=None, ctx=True, ptrs=True, tol=1e-10,
         max_iter=100, max_evals=10, ws=True, ws_bytes=1 << 30):
    q = p if ptrs else None
    params = _params() if params is None else params
    pp = ctypes.byref(params) if params != "null" else None
    return L.mtg_ragged_tube_time_optimize(p if ctx else None, N, r, S_max, B, q, q, q, q, q,
                                           tol, max_iter, pp, max_evals, q, None, None, None,
                                           p if ws else None, ws_bytes, None)


def _query(L, S_max=6, B=2, params=None, optimize=0, N=N):
    params = _params() if params is None else params
    return L.mtg_ragged_tube_time_workspace_bytes(N, S_max, B, ctypes.byref(params), optimize)


def test_symbols_exported_declared_and_in_all():
    import mav_tube_trajectory_generation_amd as mtg
    import mav_tube_trajectory_generation_amd._abi as abi
    lib = ctypes.CDLL(abi.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include",
                               "mtg_hip.h")).read()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), sym
        assert sym in abi.SIGNATURES, sym
        assert re.search(r"^int(64_t)? " + sym + r"\(", header, re.M), sym
    for name in ("ragged_tube_time_workspace_bytes", "ragged_tube_time_cost",
                 "ragged_tube_time_optimize"):
        assert callable(getattr(mtg, name)) and name in mtg.__all__, name


@pytest.mark.parametrize("call", [_cost, _opt])
def test_sizes_before_anything_else(L, buf, call):
    p = buf[0]
    none = dict(ctx=False, ptrs=False, ws=False)
    for S_max in (1, 0, -4):
        assert call(L, p, S_max=S_max) == INVALID
        assert call(L, p, S_max=S_max, **none) == INVALID
    for n in (7, 14, 2, 0):
        assert call(L, p, N=n, **none) == INVALID, n
    for r in (-1, 5):
        assert call(L, p, r=r, **none) == INVALID, r
    assert call(L, p, B=-1, **none) == INVALID
    assert call(L, p, B=1 << 26, **none) == INVALID
    assert call(L, p, B=1 << 25, S_max=64, **none) == INVALID  # B x S_max >= 2^31
    # sizes are looked at before the parameters
    assert call(L, p, S_max=1, params="null", **none) == INVALID
    bad = _params(grad_mode=1, optimizer="fd")
    assert call(L, p, N=7, params=bad, **none) == INVALID


@pytest.mark.parametrize("call", [_cost, _opt])
def test_unsupported_sizes(L, buf, call):
    """S_max above 64 (the rows the ragged extrema kernel stages) or a layout
    above the LDS limit: unsupported, before the parameters, ctx or pointers."""
    p = buf[0]
    none = dict(ctx=False, ptrs=False, ws=False)
    for S_max in (65, 1000, 0x7fffffff):
        assert call(L, p, S_max=S_max, B=1, **none) == UNSUPPORTED, S_max
        assert call(L, p, S_max=S_max, B=1, params="null", **none) == UNSUPPORTED, S_max
    first = None
    for S_max in range(2, 66):
        rc = call(L, p, S_max=S_max, **none)
        if first is None and rc == UNSUPPORTED:
            first = S_max
        assert rc == (INVALID if first is None else UNSUPPORTED), (S_max, rc)
    assert first is not None and first > 16


def test_parameter_checks_need_no_device(L, buf):
    p = buf[0]
    none = dict(ctx=False, ptrs=False, ws=False)
    for call in (_cost, _opt):
        assert call(L, p, params="null", **none) == INVALID
        assert call(L, p, params=_params(soft=[(1, 2.0)], hard=True), **none) == INVALID
        assert call(L, p, params=_params(soft=[(1, -2.0)]), **none) == INVALID
        assert call(L, p, params=_params(soft=[(5, 2.0)]), **none) == INVALID
        assert call(L, p, params=_params(increment=0.0), **none) == INVALID
        for bad in (dict(tol=0.0), dict(tol=-1e-9), dict(tol=float("nan")), dict(max_iter=0)):
            assert call(L, p, **bad) == INVALID, bad
            assert call(L, p, B=0, **bad, **none) == INVALID, bad
    # grad_mode: 0 and 2 exist, 1 needs d held fixed, anything else is invalid
    assert _cost(L, p, params=_params(grad_mode=1), **none) == UNSUPPORTED
    assert _cost(L, p, params=_params(grad_mode=1)) == UNSUPPORTED
    assert _cost(L, p, params=_params(grad_mode=3), **none) == INVALID
    # the optimiser ignores grad_mode (LN_SBPLX is gradient-free) ...
    assert _opt(L, p, B=0, params=_params(grad_mode=1), **none) == OK
    # ... and has LN_SBPLX only
    assert _opt(L, p, params=_params(optimizer="fd"), **none) == UNSUPPORTED
    assert _opt(L, p, params=_params(optimizer="fd")) == UNSUPPORTED
    odd = _params()
    odd.optimizer = 2
    assert _opt(L, p, params=odd, **none) == INVALID
    for E in (0, -3):
        assert _opt(L, p, max_evals=E) == INVALID
        assert _opt(L, p, max_evals=E, B=0, **none) == INVALID
    # the gradient's B x (2 S_max + 1) problems must fit one launch
    assert _cost(L, p, S_max=12, B=1 << 22, params=_params(grad_mode=2), **none) == INVALID
    assert _cost(L, p, S_max=12, B=0, params=_params(grad_mode=2), **none) == OK


def test_pointer_checks(L, buf):
    p = buf[0]
    for call in (_cost, _opt):
        assert call(L, p, ctx=False) == INVALID
        assert call(L, p, ptrs=False) == INVALID
        # B == 0 launches nothing and needs neither a context nor a workspace
        assert call(L, p, B=0, ctx=False, ptrs=False, ws=False, ws_bytes=0) == OK


def test_workspace_query(L):
    from mav_tube_trajectory_generation_amd._abi import make_time_params
    import mav_tube_trajectory_generation_amd as mtg
    soft = [(1, 2.0), (2, 3.0)]
    for optimize, kw in ((0, dict(grad_mode=0)), (0, dict(grad_mode=2)),
                         (0, dict(grad_mode=2, soft=soft)), (1, dict()), (1, dict(soft=soft))):
        prm = _params(**kw)
        prev = 0
        for B in (0, 1, 2, 7, 64, 1000):
            n = _query(L, S_max=8, B=B, params=prm, optimize=optimize)
            assert n >= prev and n > 0, (kw, B)
            prev = n
        prev = 0
        for S_max in range(2, 17):
            n = _query(L, S_max=S_max, B=16, params=prm, optimize=optimize)
            assert n > prev, (kw, S_max)
            prev = n
    # LN_SBPLX evaluates one point per round: its workspace is below what the
    # 2 S_max + 1 points of the gradient layout alone would take
    for S_max in (2, 8, 12):
        B = 64
        opt = _query(L, S_max=S_max, B=B, optimize=1)
        grad = _query(L, S_max=S_max, B=B, params=_params(grad_mode=2), optimize=0)
        assert opt < grad
        assert opt < B * (2 * S_max + 1) * S_max * 3 * N * 8  # that layout's coefficients
    # invalid sizes and parameters: < 0
    assert _query(L, S_max=1) == INVALID
    assert _query(L, N=7) == INVALID
    assert _query(L, B=-1) == INVALID
    assert _query(L, B=1 << 26) == INVALID
    assert _query(L, S_max=65) == UNSUPPORTED
    assert _query(L, S_max=12, B=1 << 22, params=_params(grad_mode=2)) == INVALID
    assert _query(L, params=_params(soft=soft, hard=True)) == INVALID
    assert _query(L, params=_params(grad_mode=1)) == UNSUPPORTED
    assert _query(L, params=_params(optimizer="fd"), optimize=1) == UNSUPPORTED
    assert L.mtg_ragged_tube_time_workspace_bytes(N, 6, 2, None, 0) == INVALID
    # the wrapper raises on them
    with pytest.raises(mtg.MTGError, match=r"\(-1\)"):
        mtg.ragged_tube_time_workspace_bytes(N, 1, 2, make_time_params(), False)
    with pytest.raises(mtg.MTGError, match=r"\(-4\)"):
        mtg.ragged_tube_time_workspace_bytes(N, 6, 2, make_time_params(optimizer="fd"), True)
    assert mtg.ragged_tube_time_workspace_bytes(N, 6, 2, _params(), True) == \
        _query(L, optimize=1)
