"""SOLVER.DEVICE_LOSS_SCALE on the host: the config key and the restated DynamicLossScale rule (tests/loss_scale_ref.py) the device
kernel is compared with in tests/test_loss_scale_gpu.py.  That the header and the binding agree on the four new entry points is
tests/test_abi.py's."""
import pytest

import x3d_tf_amd as x
from x3d_tf_amd import hip
from x3d_tf_amd.config import device_loss_scale_settings

from tests import loss_scale_ref as R


# ---- config ---------------------------------------------------------------------------------------------------------------
def test_the_key_is_optional_and_typed():
    cfg = x.get_config("M")
    assert dict(cfg.SOLVER) == dict(CLIP_GRAD_L2NORM=0.0, ACCUM_STEPS=1, EMA_DECAY=0.0, EMA_EVAL=True)
    assert cfg.SOLVER.DEVICE_LOSS_SCALE is False and device_loss_scale_settings(cfg) is False
    on = x.get_config("M", ["SOLVER.DEVICE_LOSS_SCALE", True])            # a merge from a list
    assert device_loss_scale_settings(on) is True
    assert dict(on.SOLVER) == dict(CLIP_GRAD_L2NORM=0.0, ACCUM_STEPS=1, EMA_DECAY=0.0, EMA_EVAL=True, DEVICE_LOSS_SCALE=True)
    for bad in (1, "yes", 0.5, [True]):
        with pytest.raises(ValueError):
            x.get_config("M", ["SOLVER.DEVICE_LOSS_SCALE", bad])
    c = cfg.clone()
    c.defrost()
    c.SOLVER.DEVICE_LOSS_SCALE = 1                 # (set past the merge's type check)
    with pytest.raises(ValueError):
        device_loss_scale_settings(c)
    bare = cfg.clone()
    bare.defrost()
    del bare["SOLVER"]
    assert device_loss_scale_settings(bare) is False


def test_the_header_states_the_state_and_the_entry_points():
    assert hip.LOSS_SCALE_STATE == R.STATE == 8
    for name in ("x3d_loss_scale_apply", "x3d_unscale_sumsq", "x3d_seg_unscale_sumsq", "x3d_loss_scale_update"):
        assert name in hip.exported_symbols()


# ---- the restated rule, on hand-written sequences ---------------------------------------------------------------------------
def test_a_skip_halves_and_resets_the_run():
    s = R.update(R.initial(2.0 ** 15), False, 5)
    assert s == [2.0 ** 15, 2.0 ** -15, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    s = R.update(s, True, 5)
    assert s == [2.0 ** 14, 2.0 ** -14, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0]      # halved, good = 0, skipped 1, applied kept, flag
    s = R.update(s, False, 5)
    assert s == [2.0 ** 14, 2.0 ** -14, 1.0, 1.0, 2.0, 0.0, 0.0, 0.0]      # the flag clears with the next applied step


def test_the_floor_is_one():
    s = R.initial(2.0)
    s = R.update(s, True, 3)
    assert s[R.SCALE] == 1.0 and s[R.INV] == 1.0
    s = R.update(s, True, 3)
    assert s[R.SCALE] == 1.0 and s[R.INV] == 1.0 and s[R.SKIPPED] == 2.0 and s[R.APPLIED] == 0.0


def test_doubling_after_growth_steps_and_reset():
    states = R.run(R.initial(4.0), [0, 0, 0, 0, 0, 0, 0], 3)
    assert [s[R.SCALE] for s in states] == [4.0, 4.0, 8.0, 8.0, 8.0, 16.0, 16.0]
    assert [s[R.GOOD] for s in states] == [1.0, 2.0, 0.0, 1.0, 2.0, 0.0, 1.0]
    assert all(s[R.INV] == 1.0 / s[R.SCALE] for s in states)
    # a skip inside the run starts it again: two finite steps, a skip, then three more are needed
    states = R.run(R.initial(4.0), [0, 0, 1, 0, 0, 0], 3)
    assert [s[R.SCALE] for s in states] == [4.0, 4.0, 2.0, 2.0, 2.0, 4.0]
    assert [s[R.GOOD] for s in states] == [1.0, 2.0, 0.0, 1.0, 2.0, 0.0]
    # growth_steps = 1: every finite step doubles
    assert [s[R.SCALE] for s in R.run(R.initial(1.0), [0, 0, 1, 0], 1)] == [2.0, 4.0, 2.0, 4.0]
    with pytest.raises(ValueError):
        R.update(R.initial(), False, 0)


def test_the_totals_count_every_step_once():
    script = [0, 1, 1, 0, 0, 0, 1, 0]
    states = R.run(R.initial(), script, 2)
    assert [s[R.APPLIED] for s in states] == [1, 1, 1, 2, 3, 4, 4, 5]
    assert [s[R.SKIPPED] for s in states] == [0, 1, 2, 2, 2, 2, 3, 3]
    assert [s[R.LAST_SKIPPED] for s in states] == [float(b) for b in script]
    assert all(s[R.APPLIED] + s[R.SKIPPED] == i + 1 for i, s in enumerate(states))
    assert all(s[6] == 0.0 and s[7] == 0.0 for s in states)


def test_no_doubling_past_the_largest_float32():
    s = R.update(R.initial(2.0 ** 127), False, 1)
    assert s[R.SCALE] == 2.0 ** 127 and s[R.GOOD] == 1.0                    # 2^128 is no float32: the scale stays, the run goes on
    s = R.update(R.initial(2.0 ** 126), False, 1)
    assert s[R.SCALE] == 2.0 ** 127 and s[R.GOOD] == 0.0
