"""The ragged tube entries' C ABI boundary and Python front end without a
device: the exported symbols, the argument checks (which all return before
anything touches a GPU) and pack_ragged_tube.  The non-NULL pointers handed
over are never dereferenced by a call that fails its checks.
"""
import ctypes

import numpy as np
import pytest

OK, INVALID, UNSUPPORTED = 0, -1, -4


@pytest.fixture(scope="module")
def L():
    import mav_tube_trajectory_generation_amd as mtg
    return mtg.lib()


@pytest.fixture(scope="module")
def buf():
    """An address that is not NULL (never read: the calls fail first)."""
    b = (ctypes.c_double * 8)()
    return ctypes.cast(b, ctypes.c_void_p), b


def _solve(L, p, N=10, r=4, S_max=6, B=2, ctx=True, ptrs=True, coeffs=True, tol=1e-10,
           max_iter=100):
    q = p if ptrs else None
    return L.mtg_ragged_tube_solve(p if ctx else None, N, r, S_max, B, q, q, q, q, q, q, tol,
                                   max_iter, None, p if coeffs else None, None, None, None, None,
                                   None)


def _resid(L, p, N=10, r=4, S_max=6, B=2, ctx=True, ptrs=True, x=True, resid=True):
    q = p if ptrs else None
    return L.mtg_ragged_tube_residuals(p if ctx else None, N, r, S_max, B, q, q, q, q, q, q,
                                       p if x else None, p if resid else None, None)


def test_symbols_exported():
    import mav_tube_trajectory_generation_amd as mtg
    import mav_tube_trajectory_generation_amd._abi as abi
    lib = ctypes.CDLL(abi.LIB_PATH)
    for sym in ("mtg_ragged_tube_num_constraints", "mtg_ragged_tube_residuals",
                "mtg_ragged_tube_solve"):
        assert hasattr(lib, sym), sym
        assert sym in abi.SIGNATURES, sym
    for name in ("ragged_tube_solve", "ragged_tube_residuals", "pack_ragged_tube"):
        assert callable(getattr(mtg, name)) and name in mtg.__all__, name


def test_num_constraints(L):
    for N in (4, 6, 8, 10, 12):
        for S in (2, 3, 7, 12):
            n = L.mtg_ragged_tube_num_constraints(N, S)
            assert n == L.mtg_tube_num_constraints(N, S) == (S - 1) + 3 * S * (N - 2)
    assert L.mtg_ragged_tube_num_constraints(7, 4) == INVALID


@pytest.mark.parametrize("call", [_solve, _resid])
def test_sizes_before_pointers(L, buf, call):
    p = buf[0]
    none = dict(ctx=False, ptrs=False)
    for S_max in (1, 0, -4):
        assert call(L, p, S_max=S_max) == INVALID
        assert call(L, p, S_max=S_max, **none) == INVALID
    for N in (7, 14, 2, 0):
        assert call(L, p, N=N) == INVALID, N
        assert call(L, p, N=N, **none) == INVALID, N
    for r in (-1, 5):
        assert call(L, p, r=r, **none) == INVALID, r
    assert call(L, p, B=-1, **none) == INVALID
    assert call(L, p, B=1 << 26, **none) == INVALID          # one workgroup per row
    assert call(L, p, B=1 << 25, S_max=64, **none) == INVALID  # B x S_max >= 2^31


@pytest.mark.parametrize("call", [_solve, _resid])
@pytest.mark.parametrize("N", [4, 6, 8, 10, 12])
def test_lds_limit_is_monotone(L, buf, call, N):
    """The first S_max whose largest layout exceeds the LDS limit, found with
    every pointer NULL; every S_max above it is unsupported too (the layout is
    not monotone in S, the maximum over 2..S_max is)."""
    p = buf[0]
    none = dict(ctx=False, ptrs=False)
    first = None
    for S_max in range(2, 400):
        rc = call(L, p, N=N, r=N // 2 - 1, S_max=S_max, **none)
        if first is None:
            if rc == UNSUPPORTED:
                first = S_max
            else:
                assert rc == INVALID, (S_max, rc)   # supported: on to the pointer checks
        else:
            assert rc == UNSUPPORTED, (S_max, rc)
    assert first is not None
    if N == 10:
        assert first > 16
    for S_max in (1000, 100000, 0x7fffffff):
        assert call(L, p, N=N, r=N // 2 - 1, S_max=S_max, B=1, **none) == UNSUPPORTED
        assert call(L, p, N=N, r=N // 2 - 1, S_max=S_max, B=1) == UNSUPPORTED


def test_pointer_and_parameter_checks(L, buf):
    p = buf[0]
    assert _solve(L, p, ctx=False) == INVALID
    assert _resid(L, p, ctx=False) == INVALID
    assert _solve(L, p, ptrs=False) == INVALID
    assert _resid(L, p, ptrs=False) == INVALID
    # B == 0 launches nothing and needs no context
    assert _solve(L, p, B=0, ctx=False, ptrs=False, coeffs=False) == OK
    assert _resid(L, p, B=0, ctx=False, ptrs=False, x=False, resid=False) == OK
    # ... but its tolerances are still checked
    for bad in (dict(tol=0.0), dict(tol=-1e-9), dict(tol=float("nan")), dict(max_iter=0)):
        assert _solve(L, p, B=0, ctx=False, ptrs=False, **bad) == INVALID, bad


def _as_cuda(t):
    """A host tensor that answers is_cuda with True, so the wrapper's checks go
    on to dtype, shape and layout; every call below fails one of them before a
    pointer is taken."""
    import torch

    class Claimed(torch.Tensor):
        is_cuda = property(lambda self: True)

    return torch.Tensor._make_subclass(Claimed, t)


def test_wrappers_reject_wrong_arguments():
    torch = pytest.importorskip("torch")
    import mav_tube_trajectory_generation_amd as mtg
    N, r, B, S = 10, 4, 2, 4
    f64 = lambda *s: torch.ones(s, dtype=torch.float64)  # noqa: E731
    good = dict(seg_counts=torch.full((B,), 3, dtype=torch.int32), positions=f64(B, S + 1, 3),
                fixed_vals=f64(B, 3, N), times_cp=f64(B, S), times=f64(B, S),
                radii=f64(B, S, 2))
    xgood = f64(B, 3, (S - 1) * 5)

    def solve(claim=True, **kw):
        a = dict(good)
        a.update(kw)
        if claim:
            a = {k: _as_cuda(v) if isinstance(v, torch.Tensor) else v for k, v in a.items()}
        out = a.pop("out", None)
        return mtg.ragged_tube_solve(None, N, r, out=out, **a)

    def resid(x, **kw):
        a = dict(good)
        a.update(kw)
        a = {k: _as_cuda(v) for k, v in a.items()}
        return mtg.ragged_tube_residuals(None, N, r, x=x, **a)

    with pytest.raises(mtg.MTGError, match="CUDA"):
        solve(claim=False)                                   # host tensors
    with pytest.raises(mtg.MTGError):
        solve(times=good["times"].numpy())
    with pytest.raises(mtg.MTGError, match="int32"):
        solve(seg_counts=torch.full((B,), 3, dtype=torch.int64))
    with pytest.raises(mtg.MTGError, match="seg_counts has shape"):
        solve(seg_counts=torch.full((B + 1,), 3, dtype=torch.int32))
    with pytest.raises(mtg.MTGError, match="positions has shape"):
        solve(positions=f64(B, S, 3))
    with pytest.raises(mtg.MTGError, match="fixed_vals has shape"):
        solve(fixed_vals=f64(B, 3, N + 1))
    with pytest.raises(mtg.MTGError, match="times_cp has shape"):
        solve(times_cp=f64(B, S + 1))
    with pytest.raises(mtg.MTGError, match="radii has shape"):
        solve(radii=f64(B, S))
    with pytest.raises(mtg.MTGError, match="float64"):
        solve(radii=torch.ones((B, S, 2), dtype=torch.float32))
    with pytest.raises(mtg.MTGError, match="contiguous"):
        solve(times=f64(S, B).t())
    with pytest.raises(mtg.MTGError, match=r"\[B, S_max\]"):
        solve(times=f64(B * S))
    with pytest.raises(mtg.MTGError, match="coeffs has shape"):
        solve(out={"coeffs": _as_cuda(f64(B, S - 1, 3, N))})
    with pytest.raises(mtg.MTGError, match="x has shape"):
        solve(out={"x": _as_cuda(f64(B, 3 * (S - 1) * 5))})
    with pytest.raises(mtg.MTGError, match="status must be int32"):
        solve(out={"status": _as_cuda(torch.zeros(B, dtype=torch.int64))})
    with pytest.raises(mtg.MTGError, match="order has shape"):
        solve(out={"order": _as_cuda(torch.zeros(B + 1, dtype=torch.int32))})
    with pytest.raises(mtg.MTGError, match="x has shape"):
        resid(_as_cuda(f64(B, 3 * (S - 1) * 5)))
    with pytest.raises(mtg.MTGError, match="CUDA"):
        resid(xgood)
    with pytest.raises(mtg.MTGError, match="positions has shape"):
        resid(_as_cuda(xgood), positions=f64(B, S + 2, 3))


def test_pack_ragged_tube():
    torch = pytest.importorskip("torch")
    import mav_tube_trajectory_generation_amd as mtg
    N = 10
    rng = np.random.default_rng(5)
    counts = [3, 2, 5]
    probs = [(rng.normal(size=(S + 1, 3)), rng.normal(size=(3, N)), rng.uniform(1, 2, S),
              rng.uniform(0.1, 0.3, (S, 2))) for S in counts]
    for S_max in (None, 7):
        seg, pos, fv, t, rad = mtg.pack_ragged_tube(probs, N, "cpu", S_max=S_max)
        W = 5 if S_max is None else S_max
        assert seg.dtype == torch.int32 and seg.tolist() == counts
        assert pos.shape == (3, W + 1, 3) and fv.shape == (3, 3, N)
        assert t.shape == (3, W) and rad.shape == (3, W, 2)
        assert all(a.dtype == torch.float64 and a.is_contiguous() for a in (pos, fv, t, rad))
        for b, (p, f, tt, rd) in enumerate(probs):
            S = counts[b]
            assert np.array_equal(pos[b, :S + 1].numpy(), p)
            assert np.array_equal(fv[b].numpy(), f)
            assert np.array_equal(t[b, :S].numpy(), tt)
            assert np.array_equal(rad[b, :S].numpy(), rd)
            assert torch.isnan(pos[b, S + 1:]).all() and torch.isnan(t[b, S:]).all()
            assert torch.isnan(rad[b, S:]).all()
    with pytest.raises(mtg.MTGError, match="below the longest count"):
        mtg.pack_ragged_tube(probs, N, "cpu", S_max=4)
    with pytest.raises(mtg.MTGError, match="at least 2 segments"):
        mtg.pack_ragged_tube(probs + [(np.zeros((2, 3)), np.zeros((3, N)), np.ones(1),
                                       np.ones((1, 2)))], N, "cpu")
    with pytest.raises(mtg.MTGError, match="shapes"):
        mtg.pack_ragged_tube([(np.zeros((3, 3)), np.zeros((3, N)), np.ones(3), np.ones((3, 2)))],
                             N, "cpu")
    with pytest.raises(mtg.MTGError, match="at least one"):
        mtg.pack_ragged_tube([], N, "cpu")
