"""The ragged evaluators' C ABI boundary without a device
(mtg_ragged_max_magnitude, mtg_ragged_soft_constraint_cost,
mtg_ragged_sample_trajectories): exported symbols and the argument checks,
which all return before anything touches a GPU.  The non-NULL pointers
handed over are never dereferenced by a call that fails its checks.
"""
import ctypes

import pytest

INVALID, UNSUPPORTED = -1, -4
NAMES = ("mtg_ragged_max_magnitude", "mtg_ragged_soft_constraint_cost",
         "mtg_ragged_sample_trajectories")


@pytest.fixture(scope="module")
def L():
    import mav_tube_trajectory_generation_amd as mtg
    return mtg.lib()


@pytest.fixture(scope="module")
def buf():
    """An address that is not NULL (never read: the calls fail first)."""
    b = (ctypes.c_double * 8)()
    return ctypes.cast(b, ctypes.c_void_p), b


def _max(L, p, N=10, D=3, S_max=12, B=2, seg=True, coeffs=True, times=True, derivative=1):
    return L.mtg_ragged_max_magnitude(N, D, S_max, B, p if seg else None, p if coeffs else None,
                                      p if times else None, derivative, None, None, None, None)


def _soft(L, p, N=10, D=3, S_max=12, B=2, seg=True, coeffs=True, times=True, ders=(1, 2),
          lims=(3.0, 1.5), n=None, maxima=True, cost=True, gate_in=False, gate_out=False):
    n = len(ders) if n is None else n
    d = (ctypes.c_int * max(len(ders), 1))(*ders)
    v = (ctypes.c_double * max(len(lims), 1))(*lims)
    return L.mtg_ragged_soft_constraint_cost(
        N, D, S_max, B, p if seg else None, p if coeffs else None, p if times else None, n, d, v,
        100.0, 1e12, p if maxima else None, p if cost else None, p if gate_in else None,
        p if gate_out else None, None)


def _sample(L, p, N=10, D=3, S_max=12, B=2, seg=True, coeffs=True, times=True, t_start=0.0,
            t_end=-1.0, dt=0.01, n_max=64, K=2, samples=True):
    return L.mtg_ragged_sample_trajectories(N, D, S_max, B, p if seg else None,
                                            p if coeffs else None, p if times else None, t_start,
                                            t_end, dt, n_max, K, p if samples else None, None,
                                            None, None)


def test_symbols_exported():
    import mav_tube_trajectory_generation_amd as mtg
    import mav_tube_trajectory_generation_amd._abi as abi
    lib = ctypes.CDLL(abi.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in abi.SIGNATURES, name
    for name in ("ragged_max_magnitude", "ragged_soft_constraint_cost",
                 "ragged_sample_trajectories"):
        assert callable(getattr(mtg, name)) and name in mtg.__all__


@pytest.mark.parametrize("call", [_max, _soft, _sample], ids=["max", "soft", "sample"])
def test_sizes_before_pointers(L, buf, call):
    p = buf[0]
    nulls = dict(seg=False, coeffs=False, times=False)
    assert call(L, p, S_max=0) == INVALID
    assert call(L, p, S_max=0, **nulls) == INVALID
    assert call(L, p, S_max=65) == UNSUPPORTED
    assert call(L, p, S_max=65, **nulls) == UNSUPPORTED  # before any pointer check
    assert call(L, p, S_max=64, **nulls) == INVALID      # 64 itself is supported
    assert call(L, p, N=7) == INVALID and call(L, p, N=14) == INVALID
    assert call(L, p, D=0) == INVALID and call(L, p, D=5) == INVALID
    assert call(L, p, B=-1) == INVALID
    for missing in ("seg", "coeffs", "times"):
        assert call(L, p, **{missing: False}) == INVALID, missing
    assert call(L, p, B=0, **nulls) == 0


def test_extrema_argument_checks(L, buf):
    p = buf[0]
    for k in (-1, 5):
        assert _max(L, p, derivative=k) == INVALID
        assert _soft(L, p, ders=(1, k)) == INVALID
    assert _max(L, p, N=4, derivative=3) == INVALID       # derivative <= N - 2
    assert _soft(L, p, N=4, ders=(3,), lims=(1.0,)) == INVALID
    assert _soft(L, p, n=0) == INVALID
    assert _soft(L, p, ders=(1,) * 9, lims=(1.0,) * 9) == INVALID
    assert _soft(L, p, lims=(3.0, -1.0)) == INVALID
    assert _soft(L, p, maxima=False) == INVALID and _soft(L, p, cost=False) == INVALID
    assert _soft(L, p, gate_out=True) == INVALID          # a gate needs its input
    assert _soft(L, p, B=0, ders=(1,) * 8, lims=(1.0,) * 8) == 0
    assert _max(L, p, B=0, derivative=4) == 0


def test_sampling_argument_checks(L, buf):
    p = buf[0]
    assert _sample(L, p, dt=0.0) == INVALID and _sample(L, p, dt=-0.01) == INVALID
    assert _sample(L, p, dt=float("nan")) == INVALID
    assert _sample(L, p, t_start=-0.5) == INVALID
    assert _sample(L, p, B=65536) == INVALID
    assert _sample(L, p, n_max=-1) == INVALID
    assert _sample(L, p, K=-1) == INVALID and _sample(L, p, K=10) == INVALID
    assert _sample(L, p, samples=False) == INVALID
    assert _sample(L, p, B=0) == 0


def _as_cuda(t):
    """A host tensor that answers is_cuda with True, so the wrappers' checks
    go on to dtype, shape and layout; every call below fails one of them
    before a pointer is taken."""
    import torch

    class Claimed(torch.Tensor):
        is_cuda = property(lambda self: True)

    return torch.Tensor._make_subclass(Claimed, t)


def test_wrappers_reject_wrong_arguments():
    torch = pytest.importorskip("torch")
    import mav_tube_trajectory_generation_amd as mtg
    seg = torch.zeros(2, dtype=torch.int32)
    c = torch.zeros((2, 4, 3, 10), dtype=torch.float64)
    t = torch.ones((2, 4), dtype=torch.float64)
    calls = (lambda *a: mtg.ragged_max_magnitude(*a, 1),
             lambda *a: mtg.ragged_soft_constraint_cost(*a, [1], [3.0]),
             lambda *a: mtg.ragged_sample_trajectories(*a, 0.01, n_max=64))
    for call in calls:
        with pytest.raises(mtg.MTGError, match="CUDA"):
            call(seg, c, t)                      # host tensors
        with pytest.raises(mtg.MTGError):
            call(seg, c.numpy(), t)
    seg, c, t = _as_cuda(seg), _as_cuda(c), _as_cuda(t)
    for call in calls:
        with pytest.raises(mtg.MTGError, match="int32"):
            call(_as_cuda(torch.zeros(2, dtype=torch.int64)), c, t)
        with pytest.raises(mtg.MTGError, match="seg_counts has shape"):
            call(_as_cuda(torch.zeros(1, dtype=torch.int32)), c, t)
        with pytest.raises(mtg.MTGError, match="times has shape"):
            call(seg, c, _as_cuda(torch.ones((2, 3), dtype=torch.float64)))
        with pytest.raises(mtg.MTGError, match=r"\[B, S_max, D, N\]"):
            call(seg, _as_cuda(torch.zeros((4, 3, 10), dtype=torch.float64)), t)
        with pytest.raises(mtg.MTGError, match="float64"):
            call(seg, _as_cuda(torch.zeros((2, 4, 3, 10), dtype=torch.float32)), t)
        with pytest.raises(mtg.MTGError, match="contiguous"):
            call(seg, c, _as_cuda(torch.ones((4, 2), dtype=torch.float64).t()))
    with pytest.raises(mtg.MTGError, match="differ in length"):
        mtg.ragged_soft_constraint_cost(seg, c, t, [1, 2], [3.0])
    with pytest.raises(mtg.MTGError, match="gate has shape"):
        mtg.ragged_soft_constraint_cost(seg, c, t, [1], [3.0], gate=t)
