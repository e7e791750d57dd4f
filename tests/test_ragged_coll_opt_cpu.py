"""The ragged collision entries' C ABI boundary and Python front end without a
device: the exported symbols, the workspace query, the argument checks that
return before a context or a pointer is looked at, and the preconditions of
the GPU tests' fixture (ragged_coll_fixture.py) on the oracle alone.  The
non-NULL pointers handed over are never dereferenced by a call that fails its
checks."""
import ctypes
import os
import re

import numpy as np
import pytest

OK, INVALID, UNSUPPORTED = 0, -1, -4
N, R = 10, 4
SYMBOLS = ("mtg_ragged_coll_workspace_bytes", "mtg_ragged_coll_cost", "mtg_ragged_coll_optimize")


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
    from mav_tube_trajectory_generation_amd._abi import make_coll_params
    from mav_tube_trajectory_generation_amd.demo import coll_params
    return make_coll_params(**coll_params(**kw))


def _cost(L, p, N=N, r=R, S_max=6, B=2, mode=0, params=None, ctx=True, ptrs=True, ws=True,
          ws_bytes=1 << 30, grid=(4, 4, 4)):
    q = p if ptrs else None
    params = _params() if params is None else params
    pp = ctypes.byref(params) if params != "null" else None
    return L.mtg_ragged_coll_cost(p if ctx else None, N, r, S_max, B, mode, q, q, q, q, q,
                                  grid[0], grid[1], grid[2], None, pp, None, q, q, q, q, q,
                                  p if ws else None, ws_bytes, None)


def _opt(L, p, N=N, r=R, S_max=6, B=2, mode=0, params=None, ctx=True, ptrs=True, ws=True,
         ws_bytes=1 << 30, max_evals=10, grid=(4, 4, 4)):
    q = p if ptrs else None
    params = _params() if params is None else params
    pp = ctypes.byref(params) if params != "null" else None
    return L.mtg_ragged_coll_optimize(p if ctx else None, N, r, S_max, B, mode, q, q, q, q, None,
                                      None, None, q, grid[0], grid[1], grid[2], None, pp,
                                      max_evals, q, q, q, q, q, None, p if ws else None,
                                      ws_bytes, None)


def _query(L, S_max=6, B=2, mode=0, params=None, optimize=0, N=N):
    params = _params() if params is None else params
    return L.mtg_ragged_coll_workspace_bytes(N, S_max, B, mode, ctypes.byref(params), optimize)


NONE = dict(ctx=False, ptrs=False, ws=False)


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
    for name in ("ragged_coll_workspace_bytes", "ragged_coll_cost", "ragged_coll_optimize"):
        assert callable(getattr(mtg, name)) and name in mtg.__all__, name


@pytest.mark.parametrize("call", [_cost, _opt])
def test_sizes_before_anything_else(L, buf, call):
    p = buf[0]
    for S_max in (1, 0, -4):
        assert call(L, p, S_max=S_max) == INVALID
        assert call(L, p, S_max=S_max, **NONE) == INVALID
    for n in (7, 14, 2, 0):
        assert call(L, p, N=n, **NONE) == INVALID, n
    for r in (-1, 5):
        assert call(L, p, r=r, **NONE) == INVALID, r
    for mode in (-1, 2):
        assert call(L, p, mode=mode, **NONE) == INVALID, mode
    assert call(L, p, B=-1, **NONE) == INVALID
    assert call(L, p, B=1 << 31, **NONE) == INVALID
    # sizes are looked at before what is unsupported and before the parameters
    assert call(L, p, S_max=1, params="null", **NONE) == INVALID
    assert call(L, p, N=7, S_max=1000, params="null", **NONE) == INVALID
    assert call(L, p, mode=3, S_max=65, **NONE) == INVALID


@pytest.mark.parametrize("call", [_cost, _opt])
def test_unsupported_sizes(L, buf, call):
    """S_max above 64 (the rows the ragged extrema kernel stages), a prep
    layout above the LDS limit or a walk above 64 KiB: unsupported, before the
    parameters, ctx or pointers."""
    p = buf[0]
    for S_max in (65, 1000, 0x7fffffff):
        assert call(L, p, S_max=S_max, B=1, **NONE) == UNSUPPORTED, S_max
        assert call(L, p, S_max=S_max, B=1, params="null", **NONE) == UNSUPPORTED, S_max
    # every count up to 64 fits at every order: the calls get as far as the
    # (NULL) context
    for n in (4, 6, 8, 10, 12):
        for S_max in range(2, 65):
            assert call(L, p, N=n, r=n // 2 - 1, S_max=S_max, **NONE) == INVALID, (n, S_max)
            assert call(L, p, N=n, r=n // 2 - 1, S_max=S_max, B=0, **NONE) == OK, (n, S_max)


def test_parameter_checks_need_no_device(L, buf):
    p = buf[0]
    for call in (_cost, _opt):
        assert call(L, p, params="null", **NONE) == INVALID
        for bad in (dict(lbfgs_memory=0), dict(lbfgs_memory=17), dict(map_resolution=0.0),
                    dict(epsilon=0.0), dict(coll_check_time_increment=0.0),
                    dict(soft=[(1, 0.0)]), dict(soft=[(5, 2.0)]), dict(soft=[(1, -1.0)])):
            assert call(L, p, params=_params(**bad), **NONE) == INVALID, bad
        # the time increment matters in the time variant only
        assert call(L, p, mode=1, params=_params(increment_time=0.0), **NONE) == INVALID
        assert call(L, p, mode=0, B=0, params=_params(increment_time=0.0), **NONE) == OK
        assert call(L, p, grid=(-1, 4, 4), **NONE) == INVALID
        # B x problems per row must fit one launch: mode 1 walks 1 + S_max
        # (forward) or 1 + 2 S_max (central) times, soft constraints take
        # 1 + 2 x 3 np_max problems
        assert call(L, p, S_max=8, B=1 << 28, mode=1, **NONE) == INVALID
        assert call(L, p, S_max=8, B=1 << 27, mode=1, **NONE) == INVALID  # no pointers
        assert call(L, p, S_max=8, B=1 << 24, params=_params(soft=[(1, 2.0)]), **NONE) == INVALID
        assert call(L, p, S_max=8, B=0, mode=1, params=_params(soft=[(1, 2.0)]), **NONE) == OK
    for E in (0, -3):
        assert _opt(L, p, max_evals=E) == INVALID
        assert _opt(L, p, max_evals=E, B=0, **NONE) == INVALID


def test_problem_grid_boundary(L, buf):
    """B x max(P_max, Q_max) <= 2^31 - 1 exactly."""
    p = buf[0]
    # mode 1, forward differences: P_max = 1 + S_max = 8
    B = (2**31 - 1) // 8
    assert _query(L, S_max=7, B=B, mode=1) > 0
    assert _query(L, S_max=7, B=B + 1, mode=1) == INVALID
    # central time differences: P_max = 1 + 2 S_max = 15
    prm = _params(simple_numgrad_time=False)
    B = (2**31 - 1) // 15
    assert _query(L, S_max=7, B=B, mode=1, params=prm) > 0
    assert _query(L, S_max=7, B=B + 1, mode=1, params=prm) == INVALID
    # soft constraints, mode 0 (central): Q_max = 1 + 2 x 3 x 6 x 5 = 181
    prm = _params(soft=[(1, 2.0)])
    B = (2**31 - 1) // 181
    assert _query(L, S_max=7, B=B, mode=0, params=prm) > 0
    assert _query(L, S_max=7, B=B + 1, mode=0, params=prm) == INVALID
    assert _cost(L, p, S_max=7, B=B + 1, params=prm, **NONE) == INVALID


def test_pointer_checks(L, buf):
    p = buf[0]
    for call in (_cost, _opt):
        assert call(L, p, ctx=False) == INVALID
        assert call(L, p, ptrs=False) == INVALID
        # B == 0 launches nothing and needs neither a context nor a workspace
        assert call(L, p, B=0, ctx=False, ptrs=False, ws=False, ws_bytes=0) == OK
        # an empty map needs no occupancy; a NULL one with voxels is refused
        # (the other pointers are NULL too, so INVALID either way: no device)
        assert call(L, p, ptrs=False, grid=(0, 0, 0)) == INVALID


def test_workspace_query(L):
    import mav_tube_trajectory_generation_amd as mtg
    soft = [(1, 2.0), (2, 3.0)]
    for optimize in (0, 1):
        for mode in (0, 1):
            for kw in (dict(), dict(simple_numgrad_time=False), dict(soft=soft)):
                prm = _params(**kw)
                prev = 0
                for B in (0, 1, 2, 7, 64, 1000):
                    n = _query(L, S_max=8, B=B, mode=mode, params=prm, optimize=optimize)
                    assert n >= prev and n > 0, (kw, B)
                    prev = n
                prev = 0
                for S_max in range(2, 17):
                    n = _query(L, S_max=S_max, B=16, mode=mode, params=prm, optimize=optimize)
                    assert n > prev, (kw, S_max)
                    prev = n
                # the optimiser's state comes on top of the evaluation's
                assert _query(L, B=16, mode=mode, params=prm, optimize=1) > \
                    _query(L, B=16, mode=mode, params=prm, optimize=0)
    assert _query(L, S_max=1) == INVALID
    assert _query(L, N=7) == INVALID
    assert _query(L, B=-1) == INVALID
    assert _query(L, mode=2) == INVALID
    assert _query(L, S_max=65) == UNSUPPORTED
    assert _query(L, params=_params(lbfgs_memory=0)) == INVALID
    assert L.mtg_ragged_coll_workspace_bytes(N, 6, 2, 0, None, 0) == INVALID
    with pytest.raises(mtg.MTGError, match=r"\(-1\)"):
        mtg.ragged_coll_workspace_bytes(N, 1, 2, _params())
    with pytest.raises(mtg.MTGError, match=r"\(-4\)"):
        mtg.ragged_coll_workspace_bytes(N, 65, 2, _params())
    assert mtg.ragged_coll_workspace_bytes(N, 6, 2, _params(), 1, True) == \
        _query(L, mode=1, optimize=1)


def test_python_shape_checks():
    """The wrappers refuse wrong tensors before any call into the library
    (host tensors here: nothing reaches a device)."""
    torch = pytest.importorskip("torch")
    import mav_tube_trajectory_generation_amd as mtg
    B, S_max, M = 2, 4, N // 2
    cpu = dict(seg=torch.zeros(B, dtype=torch.int32), fixed=torch.zeros(B, 3, N, dtype=torch.float64),
               x=torch.zeros(B, 3, (S_max - 1) * M, dtype=torch.float64),
               times=torch.ones(B, S_max, dtype=torch.float64),
               occ=torch.zeros(2, 2, 2, dtype=torch.float32))
    for fn in (mtg.ragged_coll_cost, mtg.ragged_coll_optimize):
        with pytest.raises(mtg.MTGError):  # not CUDA tensors
            fn(None, N, R, cpu["seg"], cpu["fixed"], cpu["x"], cpu["times"], cpu["occ"], _params())
        with pytest.raises(mtg.MTGError):  # times must be [B, S_max]
            fn(None, N, R, cpu["seg"], cpu["fixed"], cpu["x"], cpu["times"][0], cpu["occ"],
               _params())
        with pytest.raises(mtg.MTGError):  # mode 1 needs S_max
            fn(None, N, R, cpu["seg"], cpu["fixed"], cpu["x"].reshape(B, -1), None, cpu["occ"],
               _params(), mode=1)


# -- the fixture's preconditions, on the oracle alone ------------------------

def test_fixture_paths_converge(oracle):
    import ragged_coll_fixture as F
    P = F.paths()
    assert [p["S"] for p in P] == [2, 3, 4, 5, 6]
    for p in P:
        assert p["sol"]["status"] == 0 and 0 < p["sol"]["iters"] < 100, p["S"]
        assert p["x0"].shape == (3 * (p["S"] - 1) * F.M,) and np.all(np.isfinite(p["x0"]))
        assert p["df"].shape == (3, N)
        r = oracle.tube_residuals(N, R, p["v"], p["t"], p["radii"], p["x0"])
        assert np.max(r) <= 1e-8, (p["S"], np.max(r))


def test_fixture_layout_round_trip():
    import ragged_coll_fixture as F
    rng = np.random.default_rng(0)
    for mode in (0, 1):
        for S in (2, 4, 7):
            x = rng.standard_normal(F.n_vars(S, mode))
            row = F.pad_x(x, S, 7, mode)
            assert row.size == (7 if mode else 0) + 3 * 6 * F.M
            assert np.array_equal(F.unpad_x(row, S, 7, mode), x)
            mask = F.padding_mask(S, 7, mode)
            assert np.all(np.isnan(row.reshape(-1)[mask])) and mask.sum() == row.size - x.size


@pytest.mark.parametrize("mode", [0, 1])
def test_fixture_cost_points_hit_and_miss(oracle, mode):
    """Among the cost tests' evaluation points both collision outcomes occur."""
    import ragged_coll_fixture as F
    from coll_fixture import coll_params
    P, occ = F.paths(), F.forest_map()
    flags = [oracle.coll_cost(N, R, P[i]["vt"], P[i]["t"], mode, x, occ, coll_params())[3]
             for i, x in F.cost_rows(mode)]
    assert 0 < sum(flags) < len(flags), flags
    assert {i for i, _ in F.cost_rows(mode)} == set(range(5))


@pytest.mark.parametrize("mode,variant,n", [(0, "main", 6), (0, "central", 12), (1, "central", 6),
                                            (0, "soft", 6), (1, "soft", 6)])
def test_fixture_oracle_descends(oracle, mode, variant, n):
    """oracle.coll_optimize lowers J on every optimiser start of the GPU tests."""
    import ragged_coll_fixture as F
    ref = F.oracle_optimize(mode, variant, n)
    for b, o in enumerate(ref):
        assert np.isfinite(o["J"]) and o["J"] < o["J0"], (b, o["J0"], o["J"])
        assert o["evals"] >= 2
