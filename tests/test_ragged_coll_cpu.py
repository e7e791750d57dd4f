"""mtg_ragged_collision_cost's C ABI boundary without a device: the exported
symbol and the argument checks, which all return before anything touches a
GPU.  The non-NULL pointers handed over are never dereferenced by a call that
fails its checks.
"""
import ctypes

import pytest

INVALID, UNSUPPORTED = -1, -4


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
    import mav_tube_trajectory_generation_amd as mtg
    prm = dict(map_resolution=0.25, min_bound=[0.0] * 3, max_bound=[40.0] * 3, epsilon=0.5,
               robot_radius=0.1, coll_pot_multiplier=1.0, coll_check_time_increment=0.1,
               box_side=20)
    prm.update(kw)
    return mtg.make_collision_params(**prm)


def _call(L, p, N=10, S_max=12, B=2, seg=True, coeffs=True, times=True, occ=True, grid=(8, 8, 8),
          field=False, params=True, gate_in=False, gate_out=False, grad=False, **prm):
    cp = _params(**prm)
    nx, ny, nz = grid
    return L.mtg_ragged_collision_cost(
        N, S_max, B, p if seg else None, p if coeffs else None, p if times else None,
        p if occ else None, nx, ny, nz, p if field else None,
        ctypes.byref(cp) if params else None, None, None, None, None, p if grad else None,
        p if gate_in else None, p if gate_out else None, None)


def test_symbol_exported():
    import mav_tube_trajectory_generation_amd as mtg
    import mav_tube_trajectory_generation_amd._abi as abi
    lib = ctypes.CDLL(abi.LIB_PATH)
    assert hasattr(lib, "mtg_ragged_collision_cost")
    assert "mtg_ragged_collision_cost" in abi.SIGNATURES
    assert callable(mtg.ragged_collision_cost) and "ragged_collision_cost" in mtg.__all__


def test_sizes_before_pointers(L, buf):
    p = buf[0]
    nulls = dict(seg=False, coeffs=False, times=False)
    assert _call(L, p, S_max=0) == INVALID
    assert _call(L, p, S_max=0, **nulls) == INVALID
    assert _call(L, p, S_max=65) == UNSUPPORTED
    assert _call(L, p, S_max=65, **nulls) == UNSUPPORTED  # before any pointer check
    assert _call(L, p, S_max=65, params=False) == UNSUPPORTED
    assert _call(L, p, S_max=64, **nulls) == INVALID      # 64 itself is supported
    for N in (7, 14, 2, 0):
        assert _call(L, p, N=N) == INVALID, N
    assert _call(L, p, B=-1) == INVALID
    assert _call(L, p, B=0x80000000) == INVALID
    for missing in ("seg", "coeffs", "times", "params"):
        assert _call(L, p, **{missing: False}) == INVALID, missing
    assert _call(L, p, occ=False) == INVALID              # a non-empty grid needs its map
    assert _call(L, p, B=0, **nulls) == 0
    assert _call(L, p, B=0, occ=False, **nulls) == 0


def test_collision_parameter_checks(L, buf):
    p = buf[0]
    for bad in (dict(map_resolution=0.0), dict(map_resolution=-0.25),
                dict(map_resolution=float("nan")), dict(epsilon=0.0),
                dict(coll_check_time_increment=0.0), dict(coll_check_time_increment=-0.1),
                dict(robot_radius=-0.1), dict(box_side=0), dict(box_side=257)):
        assert _call(L, p, **bad) == INVALID, bad
        assert _call(L, p, B=0, **bad) == INVALID, bad    # before the empty-batch return
    assert _call(L, p, grid=(-1, 8, 8)) == INVALID
    # the near field holds squared offsets of boxes up to side 31
    assert _call(L, p, field=True, box_side=32) == INVALID
    assert _call(L, p, field=True, box_side=32, B=0) == INVALID
    assert _call(L, p, field=False, box_side=32, B=0) == 0
    assert _call(L, p, field=True, box_side=31, B=0) == 0


def test_gate_needs_its_input(L, buf):
    p = buf[0]
    assert _call(L, p, gate_out=True) == INVALID
    assert _call(L, p, gate_out=True, grad=True) == INVALID


def _as_cuda(t):
    """A host tensor that answers is_cuda with True, so the wrapper's checks go
    on to dtype, shape and layout; every call below fails one of them before a
    pointer is taken."""
    import torch

    class Claimed(torch.Tensor):
        is_cuda = property(lambda self: True)

    return torch.Tensor._make_subclass(Claimed, t)


def test_wrapper_rejects_wrong_arguments():
    torch = pytest.importorskip("torch")
    import mav_tube_trajectory_generation_amd as mtg
    cp = _params()
    seg = torch.zeros(2, dtype=torch.int32)
    c = torch.zeros((2, 4, 3, 10), dtype=torch.float64)
    t = torch.ones((2, 4), dtype=torch.float64)
    occ = torch.full((4, 5, 6), -1.0, dtype=torch.float32)
    call = mtg.ragged_collision_cost
    with pytest.raises(mtg.MTGError, match="CUDA"):
        call(seg, c, t, occ, cp)                          # host tensors
    with pytest.raises(mtg.MTGError):
        call(seg, c.numpy(), t, occ, cp)
    seg, c, t, gpu_occ = _as_cuda(seg), _as_cuda(c), _as_cuda(t), _as_cuda(occ)
    with pytest.raises(mtg.MTGError, match="int32"):
        call(_as_cuda(torch.zeros(2, dtype=torch.int64)), c, t, gpu_occ, cp)
    with pytest.raises(mtg.MTGError, match="seg_counts has shape"):
        call(_as_cuda(torch.zeros(1, dtype=torch.int32)), c, t, gpu_occ, cp)
    with pytest.raises(mtg.MTGError, match="times has shape"):
        call(seg, c, _as_cuda(torch.ones((2, 3), dtype=torch.float64)), gpu_occ, cp)
    with pytest.raises(mtg.MTGError, match=r"\[B, S_max, D, N\]"):
        call(seg, _as_cuda(torch.zeros((4, 3, 10), dtype=torch.float64)), t, gpu_occ, cp)
    with pytest.raises(mtg.MTGError, match="float64"):
        call(seg, _as_cuda(torch.zeros((2, 4, 3, 10), dtype=torch.float32)), t, gpu_occ, cp)
    with pytest.raises(mtg.MTGError, match="contiguous"):
        call(seg, c, _as_cuda(torch.ones((4, 2), dtype=torch.float64).t()), gpu_occ, cp)
    with pytest.raises(mtg.MTGError, match="D = 3"):
        call(seg, _as_cuda(torch.zeros((2, 4, 2, 10), dtype=torch.float64)), t, gpu_occ, cp)
    with pytest.raises(mtg.MTGError, match="occupancy"):
        call(seg, c, t, occ, cp)                          # a host map
    with pytest.raises(mtg.MTGError, match="occupancy"):
        call(seg, c, t, _as_cuda(occ.double()), cp)
    with pytest.raises(mtg.MTGError, match="occupancy"):
        call(seg, c, t, _as_cuda(occ[0]), cp)
    with pytest.raises(mtg.MTGError, match="near_field"):
        call(seg, c, t, gpu_occ, cp,
             near_field=_as_cuda(torch.zeros((4, 5, 6, 8), dtype=torch.int32)))
    with pytest.raises(mtg.MTGError, match="near_field"):
        call(seg, c, t, gpu_occ, cp,
             near_field=_as_cuda(torch.zeros((4, 5, 6, 7), dtype=torch.int16)))
    with pytest.raises(mtg.MTGError, match="gate has shape"):
        call(seg, c, t, gpu_occ, cp, gate=t)

    def outs(**wrong):  # caller-supplied outputs, all claimed to be on the device
        o = {"cost": torch.zeros(2, dtype=torch.float64),
             "hit_time": torch.zeros(2, dtype=torch.float64),
             "collision": torch.zeros(2, dtype=torch.int32),
             "hit_segment": torch.zeros(2, dtype=torch.int32)}
        o.update(wrong)
        return {k: _as_cuda(v) for k, v in o.items()}

    with pytest.raises(mtg.MTGError, match="hit_segment"):
        call(seg, c, t, gpu_occ, cp, out=outs(hit_segment=torch.zeros(2, dtype=torch.int64)))
    with pytest.raises(mtg.MTGError, match="collision"):
        call(seg, c, t, gpu_occ, cp, out=outs(collision=torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(mtg.MTGError, match="hit_time has shape"):
        call(seg, c, t, gpu_occ, cp, out=outs(hit_time=torch.zeros(1, dtype=torch.float64)))
    with pytest.raises(mtg.MTGError, match="grad_coeffs has shape"):
        call(seg, c, t, gpu_occ, cp, grad=True,
             out=outs(grad_coeffs=torch.zeros((2, 3, 3, 10), dtype=torch.float64)))
    with pytest.raises(mtg.MTGError, match="gated has shape"):
        call(seg, c, t, gpu_occ, cp, gate=_as_cuda(torch.zeros(2, dtype=torch.float64)),
             out=outs(gated=torch.zeros(3, dtype=torch.float64)))
