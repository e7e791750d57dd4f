"""The ragged coefficients-from-constraints entries' C ABI boundary without a
device (mtg_ragged_coeffs_from_constraints, mtg_ragged_tube_coeffs): exported
symbols, the argument checks in their documented order, which all return
before anything touches a GPU, and the Python wrappers' own checks.  The
non-NULL pointers handed over are never dereferenced by a call that fails its
checks.
"""
import ctypes

import pytest

INVALID, UNSUPPORTED = -1, -4
NAMES = ("mtg_ragged_coeffs_from_constraints", "mtg_ragged_tube_coeffs")


@pytest.fixture(scope="module")
def L():
    import mav_tube_trajectory_generation_amd as mtg
    return mtg.lib()


@pytest.fixture(scope="module")
def buf():
    """An address that is not NULL (never read: the calls fail first)."""
    b = (ctypes.c_double * 8)()
    return ctypes.cast(b, ctypes.c_void_p), b


def _tube(L, p, N=10, D=3, r=4, S_max=7, B=2, layout=0, ctx=True, seg=True, fixed=True, x=True,
          times=None, coeffs=True):
    times = (layout == 0) if times is None else times
    return L.mtg_ragged_tube_coeffs(p if ctx else None, N, D, r, S_max, B, layout,
                                    p if seg else None, p if fixed else None, p if x else None,
                                    p if times else None, p if coeffs else None, None, None, None,
                                    None)


def test_symbols_exported():
    import mav_tube_trajectory_generation_amd as mtg
    import mav_tube_trajectory_generation_amd._abi as abi
    lib = ctypes.CDLL(abi.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in abi.SIGNATURES, name
    assert callable(mtg.ragged_tube_coefficients) and "ragged_tube_coefficients" in mtg.__all__
    assert callable(mtg.RaggedLinearPlan.coefficients)


def test_tube_sizes_before_pointers(L, buf):
    p = buf[0]
    nulls = dict(ctx=False, seg=False, fixed=False, x=False, times=False, coeffs=False)
    for bad in (dict(N=7), dict(N=14), dict(N=2), dict(D=0), dict(D=5), dict(r=-1), dict(r=5),
                dict(N=4, r=2), dict(layout=2), dict(layout=-1), dict(S_max=1), dict(S_max=0),
                dict(B=-1)):
        assert _tube(L, p, **bad) == INVALID, bad
        assert _tube(L, p, **bad, **nulls) == INVALID, bad
    assert _tube(L, p, S_max=65) == UNSUPPORTED
    assert _tube(L, p, S_max=65, **nulls) == UNSUPPORTED   # before ctx or any pointer
    assert _tube(L, p, S_max=65, D=5) == INVALID           # the sizes before the limit
    assert _tube(L, p, S_max=64, **nulls) == INVALID       # 64 itself is supported
    for N, r in ((4, 1), (6, 2), (8, 3), (10, 0), (12, 5)):
        assert _tube(L, p, N=N, r=r, **nulls) == INVALID   # valid sizes reach the pointers


def test_tube_pointers_and_layout(L, buf):
    p = buf[0]
    for missing in ("ctx", "seg", "fixed", "x", "coeffs"):
        for layout in (0, 1):
            assert _tube(L, p, layout=layout, **{missing: False}) == INVALID, (missing, layout)
    assert _tube(L, p, layout=0, times=False) == INVALID   # layout 0 needs times
    assert _tube(L, p, layout=1, times=True) == INVALID    # layout 1 takes them from x
    nulls = dict(ctx=False, seg=False, fixed=False, x=False, times=False, coeffs=False)
    assert _tube(L, p, B=0, **nulls) == 0
    assert _tube(L, p, B=0, layout=1, **nulls) == 0
    assert _tube(L, p, B=0) == 0
    assert _tube(L, p, B=0, S_max=65, **nulls) == UNSUPPORTED
    assert _tube(L, p, B=0, D=0, **nulls) == INVALID


def test_standard_entry_checks(L, buf):
    p = buf[0]
    f = L.mtg_ragged_coeffs_from_constraints
    assert f(None, 2, p, p, p, p, p, None, None, None) == INVALID
    assert f(None, 0, None, None, None, None, None, None, None, None) == INVALID


def _as_cuda(t):
    """A host tensor that answers is_cuda with True, so the wrappers' checks
    go on to dtype, shape and layout; every call below fails one of them
    before a pointer is taken."""
    import torch

    class Claimed(torch.Tensor):
        is_cuda = property(lambda self: True)

    return torch.Tensor._make_subclass(Claimed, t)


def test_tube_wrapper_rejects_wrong_arguments():
    torch = pytest.importorskip("torch")
    import mav_tube_trajectory_generation_amd as mtg
    N, M, B, S_max = 10, 5, 2, 4
    f64 = dict(dtype=torch.float64)
    seg = torch.zeros(B, dtype=torch.int32)
    fv = torch.zeros((B, 3, N), **f64)
    x = torch.zeros((B, 3, (S_max - 1) * M), **f64)
    t = torch.ones((B, S_max), **f64)
    x1 = torch.zeros((B, S_max + 3 * (S_max - 1) * M), **f64)

    def call(*a, **kw):
        return mtg.ragged_tube_coefficients(None, N, 4, *a, **kw)   # ctx is never reached
    with pytest.raises(mtg.MTGError, match="CUDA"):
        call(seg, fv, x, t)                                  # host tensors
    with pytest.raises(mtg.MTGError):
        call(seg, fv.numpy(), x, t)
    with pytest.raises(mtg.MTGError, match="mode must be"):
        call(seg, fv, x, t, mode=2)
    seg, fv, x, t, x1 = (_as_cuda(a) for a in (seg, fv, x, t, x1))
    with pytest.raises(mtg.MTGError, match="int32"):
        call(_as_cuda(torch.zeros(B, dtype=torch.int64)), fv, x, t)
    with pytest.raises(mtg.MTGError, match="seg_counts has shape"):
        call(_as_cuda(torch.zeros(B + 1, dtype=torch.int32)), fv, x, t)
    with pytest.raises(mtg.MTGError, match="fixed_vals has shape"):
        call(seg, _as_cuda(torch.zeros((B, 3, N - 2), **f64)), x, t)
    with pytest.raises(mtg.MTGError, match=r"\[B, D, N\]"):
        call(seg, _as_cuda(torch.zeros((B, 3 * N), **f64)), x, t)
    with pytest.raises(mtg.MTGError, match="x has shape"):
        call(seg, fv, _as_cuda(torch.zeros((B, 3, (S_max - 1) * M + 1), **f64)), t)
    with pytest.raises(mtg.MTGError, match="x has shape"):   # D of x against D of fixed_vals
        call(seg, fv, _as_cuda(torch.zeros((B, 2, (S_max - 1) * M), **f64)), t)
    with pytest.raises(mtg.MTGError, match="float64"):
        call(seg, fv, _as_cuda(torch.zeros((B, 3, (S_max - 1) * M), dtype=torch.float32)), t)
    with pytest.raises(mtg.MTGError, match="contiguous"):
        call(seg, fv, x, _as_cuda(torch.ones((S_max, B), **f64).t()))
    with pytest.raises(mtg.MTGError, match=r"\[B, S_max\]"):
        call(seg, fv, x, None)                               # mode 0 needs times
    with pytest.raises(mtg.MTGError, match="S_max = 5"):
        call(seg, fv, x, t, S_max=5)
    with pytest.raises(mtg.MTGError, match="times must be None"):
        call(seg, fv, x1, t, mode=1)
    with pytest.raises(mtg.MTGError, match="no S_max"):
        call(seg, fv, _as_cuda(torch.zeros((B, x1.shape[1] + 1), **f64)), mode=1)
    with pytest.raises(mtg.MTGError, match="x has shape"):
        call(seg, fv, x1, mode=1, S_max=5)
    with pytest.raises(mtg.MTGError, match="coeffs has shape"):
        call(seg, fv, x, t, out={"coeffs": _as_cuda(torch.zeros((B, S_max, 3, N - 2), **f64))})
    with pytest.raises(mtg.MTGError, match="status must be int32"):
        call(seg, fv, x1, mode=1, out={"status": _as_cuda(torch.zeros(B, dtype=torch.int64))})


def test_standard_wrapper_rejects_wrong_arguments():
    """RaggedLinearPlan.coefficients on a plan object made without a device:
    its checks need the sizes only and fail before the handle is used."""
    torch = pytest.importorskip("torch")
    import mav_tube_trajectory_generation_amd as mtg
    N, D, S_max, B = 10, 3, 4, 2
    plan = mtg.RaggedLinearPlan.__new__(mtg.RaggedLinearPlan)
    plan.N, plan.D, plan.r, plan.S_max = N, D, 4, S_max
    plan.nf_max, plan.np_max = N + S_max - 1, (S_max - 1) * (N // 2 - 1)
    plan._h = ctypes.c_void_p()
    f64 = dict(dtype=torch.float64)
    seg = torch.zeros(B, dtype=torch.int32)
    fv = torch.zeros((B, D, plan.nf_max), **f64)
    fr = torch.zeros((B, D, plan.np_max), **f64)
    t = torch.ones((B, S_max), **f64)
    with pytest.raises(mtg.MTGError, match="CUDA"):
        plan.coefficients(seg, fv, fr, t)
    seg, fv, fr, t = (_as_cuda(a) for a in (seg, fv, fr, t))
    with pytest.raises(mtg.MTGError, match="free_vals has shape"):
        plan.coefficients(seg, fv, _as_cuda(torch.zeros((B, D, plan.np_max + 1), **f64)), t)
    with pytest.raises(mtg.MTGError, match="free_vals must be a CUDA tensor"):
        plan.coefficients(seg, fv, None, t)                  # None only where S_max == 1
    with pytest.raises(mtg.MTGError, match="fixed_vals has shape"):
        plan.coefficients(seg, _as_cuda(torch.zeros((B, D, plan.nf_max - 1), **f64)), fr, t)
    with pytest.raises(mtg.MTGError, match="times has shape"):
        plan.coefficients(seg, fv, fr, _as_cuda(torch.ones((B, S_max + 1), **f64)))
    with pytest.raises(mtg.MTGError, match="int32"):
        plan.coefficients(_as_cuda(torch.zeros(B, dtype=torch.int64)), fv, fr, t)
    with pytest.raises(mtg.MTGError, match="coeffs has shape"):
        plan.coefficients(seg, fv, fr, t,
                          out={"coeffs": _as_cuda(torch.zeros((B, S_max, D, N + 2), **f64))})
    with pytest.raises(mtg.MTGError, match="cost has shape"):
        plan.coefficients(seg, fv, fr, t, out={"cost": _as_cuda(torch.zeros(B + 1, **f64))})
    plan._h = ctypes.c_void_p()  # nothing to destroy
