"""CPU checks of the ragged-batch front end (no GPU, no compute calls):
pack_ragged's padded layout, the argument checks of mtg_ragged_plan_create
and the new per-trajectory status code."""
import ctypes
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mtg_hip.h")


def test_pack_ragged_layout():
    import mav_tube_trajectory_generation_amd as mtg
    N, D = 10, 3
    rng = np.random.default_rng(7)
    counts = [1, 4, 2, 7]
    probs = [(rng.standard_normal((D, N + s - 1)), rng.uniform(0.5, 3.0, s)) for s in counts]
    seg, fixed, times = mtg.pack_ragged(probs, N, "cpu")
    S_max, nf_max = 7, N + 7 - 1
    assert seg.dtype == torch.int32 and seg.tolist() == counts
    assert fixed.dtype == torch.float64 and tuple(fixed.shape) == (4, D, nf_max)
    assert times.dtype == torch.float64 and tuple(times.shape) == (4, S_max)
    assert fixed.is_contiguous() and times.is_contiguous()
    f, t = fixed.numpy(), times.numpy()
    for b, (df, tt) in enumerate(probs):
        s = counts[b]
        nf = N + s - 1
        assert np.array_equal(f[b, :, :nf], df)          # values at the front of every row
        assert np.isnan(f[b, :, nf:]).all()              # padding is NaN on purpose
        assert np.array_equal(t[b, :s], tt)
        assert np.isnan(t[b, s:]).all()
    # a plan longer than the longest path
    seg2, fixed2, times2 = mtg.pack_ragged(probs, N, "cpu", S_max=12)
    assert tuple(fixed2.shape) == (4, D, N + 11) and tuple(times2.shape) == (4, 12)
    assert np.array_equal(fixed2.numpy()[1, :, :N + 3], probs[1][0])
    assert np.isnan(times2.numpy()[:, 7:]).all()


def test_pack_ragged_rejects_bad_shapes():
    import mav_tube_trajectory_generation_amd as mtg
    with pytest.raises(mtg.MTGError):
        mtg.pack_ragged([(np.zeros((3, 12)), np.ones(2))], 10, "cpu")   # nf_b should be 11
    with pytest.raises(mtg.MTGError):
        mtg.pack_ragged([(np.zeros((3, 11)), np.ones(2))], 10, "cpu", S_max=1)
    with pytest.raises(mtg.MTGError):
        mtg.pack_ragged([], 10, "cpu")


def test_plan_create_argument_checks():
    """NULL context and S_max = 0 are invalid arguments; S_max = 65 is beyond
    the kernels (as mtg_plan_create: S < 1 invalid, too large unsupported).
    The sizes are checked before the context, so both show without a device."""
    import mav_tube_trajectory_generation_amd as mtg
    L = mtg.lib()
    h = ctypes.c_void_p()
    assert L.mtg_ragged_plan_create(None, 10, 3, 4, 12, ctypes.byref(h)) == -1
    assert L.mtg_ragged_plan_create(None, 10, 3, 4, 0, ctypes.byref(h)) == -1
    assert L.mtg_ragged_plan_create(None, 10, 3, 4, 65, ctypes.byref(h)) == -4  # UNSUPPORTED
    assert L.mtg_ragged_plan_create(None, 10, 3, 4, 64, ctypes.byref(h)) == -1
    assert L.mtg_ragged_plan_create(None, 10, 3, 5, 12, ctypes.byref(h)) == -1   # r >= N/2
    assert L.mtg_ragged_plan_create(None, 10, 3, 4, 12, None) == -1
    assert L.mtg_ragged_plan_destroy(None) == -1
    assert L.mtg_ragged_plan_counts(None, None, None) == -1
    assert L.mtg_ragged_linear_solve(None, 1, None, None, None, None, None, None, None,
                                     None) == -1
    assert L.mtg_ragged_time_cost(None, 1, None, None, None, None, None, None, None, None) == -1
    assert L.mtg_ragged_time_optimize(None, 1, None, None, None, None, 10, None, None, None,
                                      None, None, None) == -1


def test_without_a_device_no_plan():
    """Without a device there is no context (MTG_ERR_NO_DEVICE), hence no
    ragged plan, and the front end raises instead of computing anything."""
    import mav_tube_trajectory_generation_amd as mtg
    if torch.cuda.is_available():
        return  # a device is present: the GPU suite covers the calls
    h = ctypes.c_void_p()
    assert mtg.lib().mtg_ctx_create(0, ctypes.byref(h)) == -2  # MTG_ERR_NO_DEVICE
    with pytest.raises(mtg.MTGError, match="no HIP device"):
        mtg.RaggedLinearPlan(mtg.Context(0), 10, 3, 4, 12)


def test_bad_segments_status_code():
    src = open(HEADER).read()
    m = re.search(r"\bMTG_TRAJ_BAD_SEGMENTS\s*=\s*(\d+)", src)
    assert m and int(m.group(1)) == 5
    assert re.search(r"\bMTG_TRAJ_NEAR_OPTIMAL\s*=\s*4\b", src)   # earlier codes unmoved
