"""The solver step on the host: the SOLVER.* config switches, the additive C ABI (new symbols under the same version) and
the schedule checks of `fit` under gradient accumulation (the kernels and the trainer are held to fp64 references in
test_solver_gpu.py)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import x3d_tf_amd as x  # noqa: E402
from x3d_tf_amd import hip  # noqa: E402
from x3d_tf_amd.config import solver_settings  # noqa: E402

NEW_SYMBOLS = ("x3d_grad_sumsq_scratch", "x3d_grad_sumsq", "x3d_sgd_nesterov_ex", "x3d_adam_ex", "x3d_ema_update",
               "x3d_grad_accum")


# ---- config -----------------------------------------------------------------------------------------------------------
def test_config_defaults_and_overrides():
    d = x.get_default_config()
    assert dict(d.SOLVER) == dict(CLIP_GRAD_L2NORM=0.0, ACCUM_STEPS=1, EMA_DECAY=0.0, EMA_EVAL=True)
    s = solver_settings(x.get_config("M"))
    assert s == (0.0, 1, 0.0, True)
    assert (s.clip_grad_l2norm, s.accum_steps, s.ema_decay, s.ema_eval) == (0.0, 1, 0.0, True)
    c = x.get_config("M", ["SOLVER.CLIP_GRAD_L2NORM", 1, "SOLVER.ACCUM_STEPS", 4, "SOLVER.EMA_DECAY", 0.9999,
                           "SOLVER.EMA_EVAL", False])
    assert solver_settings(c) == (1.0, 4, 0.9999, False)
    assert isinstance(solver_settings(c).accum_steps, int)


def test_config_without_the_section_means_off_and_train_keys_are_unchanged():
    m = x.get_config("M")
    old = m.clone()
    old.defrost()
    del old["SOLVER"]
    assert solver_settings(old) == (0.0, 1, 0.0, True)
    assert set(m) == set(old) | {"SOLVER"}
    # the new keys live in their own section: TRAIN is key for key what it was
    assert set(m.TRAIN) == {"DATASET_SIZE", "BATCH_SIZE", "EPOCHS", "OPTIMIZER", "MOMENTUM", "BASE_LR", "WARMUP_EPOCHS",
                            "WARMUP_LR", "LABEL_SMOOTHING"}


@pytest.mark.parametrize("over", [
    ["SOLVER.CLIP_GRAD_L2NORM", -1.0], ["SOLVER.CLIP_GRAD_L2NORM", float("inf")], ["SOLVER.CLIP_GRAD_L2NORM", float("nan")],
    ["SOLVER.ACCUM_STEPS", 0], ["SOLVER.ACCUM_STEPS", -2],
    ["SOLVER.EMA_DECAY", 1.0], ["SOLVER.EMA_DECAY", -0.1], ["SOLVER.EMA_DECAY", 1.5], ["SOLVER.EMA_DECAY", float("nan")],
])
def test_config_rejects(over):
    with pytest.raises(ValueError, match=over[0]):
        x.get_config("M", over)


@pytest.mark.parametrize("accum", [2.0, 1.5, True, "2x"])
def test_config_rejects_a_non_integer_accum_steps(accum):
    c = x.get_config("M", freeze=False)
    c.SOLVER.ACCUM_STEPS = accum          # (merge_from_list would refuse the type before solver_settings sees it)
    with pytest.raises(ValueError, match="SOLVER.ACCUM_STEPS"):
        solver_settings(c)


# ---- ABI --------------------------------------------------------------------------------------------------------------
def test_abi_is_additive_and_the_new_symbols_are_declared_and_exported():
    assert hip.ABI_VERSION == 138
    lib = hip.load()
    assert lib.x3d_version() == 138
    declared = hip.exported_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert getattr(lib, name) is not None
    header = open(os.path.join(ROOT, "include", "x3d_hip.h")).read()
    assert len(re.findall(r"typedef struct", re.sub(r"/\*.*?\*/", "", header, flags=re.S))) == 16     # no new struct
    from ctypes import c_double as d, c_float as f, c_int as i, c_longlong as ll, c_void_p as vp   # noqa: F401
    sigs = {
        "x3d_grad_sumsq_scratch": ([ll], ll),
        "x3d_grad_sumsq": ([vp, ll, vp, vp, vp], i),
        "x3d_sgd_nesterov_ex": ([vp, vp, vp, vp, f, f, f, f, vp, f, vp, f, ll, vp], i),
        "x3d_adam_ex": ([vp, vp, vp, vp, vp, f, f, f, f, f, f, ll, vp, f, vp, f, ll, vp], i),
        "x3d_ema_update": ([vp, vp, f, vp, ll, vp], i),
        "x3d_grad_accum": ([vp, vp, ll, i, vp], i),
    }
    for name, (argtypes, restype) in sigs.items():
        fn = getattr(lib, name)
        assert (list(fn.argtypes), fn.restype) == (argtypes, restype), name


def test_scratch_size_and_argument_checks_need_no_gpu():
    """the partial count is a fixed function of n; bad arguments are refused before any launch (so also without a device)"""
    lib = hip.load()
    assert lib.x3d_grad_sumsq_scratch(0) == 0 and lib.x3d_grad_sumsq_scratch(-5) == 0
    assert lib.x3d_grad_sumsq_scratch(1) == 2
    sizes = [lib.x3d_grad_sumsq_scratch(n) for n in (1, 4096, 4100, 2_500_003, 1 << 33)]
    assert sizes == sorted(sizes) and sizes[-1] == 2 * 1024 and all(s % 2 == 0 for s in sizes)
    a = 4096                                   # any aligned non-null address: nothing is dereferenced on the refused paths
    bad = [
        ("x3d_grad_sumsq", (None, 8, a, a)), ("x3d_grad_sumsq", (a, 0, a, a)), ("x3d_grad_sumsq", (a, 8, None, a)),
        ("x3d_grad_sumsq", (a, 8, a, None)),
        ("x3d_sgd_nesterov_ex", (None, a, a, None, .1, .9, 0., 1., None, 0., None, 0., 8)),
        ("x3d_sgd_nesterov_ex", (a, a, a, None, .1, .9, 0., 1., None, 0., None, 0., 0)),
        ("x3d_sgd_nesterov_ex", (a, a, a, None, .1, .9, 0., 1., a, 0., None, 0., 8)),          # norm without a max_norm
        ("x3d_sgd_nesterov_ex", (a, a, a, None, .1, .9, 0., 1., a, -1., None, 0., 8)),
        ("x3d_sgd_nesterov_ex", (a, a, a, None, .1, .9, 0., 1., None, 0., a, 1.0, 8)),         # decay outside [0, 1)
        ("x3d_sgd_nesterov_ex", (a, a, a, None, .1, .9, 0., 1., None, 0., a, -0.1, 8)),
        ("x3d_adam_ex", (a, None, a, a, None, .1, .9, .999, 1e-7, 0., 1., 1, None, 0., None, 0., 8)),
        ("x3d_adam_ex", (a, a, a, a, None, .1, .9, .999, 1e-7, 0., 1., 0, None, 0., None, 0., 8)),   # step counts from 1
        ("x3d_adam_ex", (a, a, a, a, None, .1, .9, .999, 1e-7, 0., 1., 1, a, 0., None, 0., 8)),
        ("x3d_adam_ex", (a, a, a, a, None, .1, .9, .999, 1e-7, 0., 1., 1, None, 0., a, 1.0, 8)),
        ("x3d_ema_update", (None, a, .5, None, 8)), ("x3d_ema_update", (a, None, .5, None, 8)),
        ("x3d_ema_update", (a, a, 1.0, None, 8)), ("x3d_ema_update", (a, a, .5, None, 0)),
        ("x3d_grad_accum", (None, a, 8, 1)), ("x3d_grad_accum", (a, None, 8, 0)), ("x3d_grad_accum", (a, a, -1, 0)),
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args, None) == 1, (name, args)      # X3D_ERR_INVALID
        assert lib.x3d_last_error()


# ---- fit's schedule under accumulation ---------------------------------------------------------------------------------
def test_accumulation_schedule_checks():
    from x3d_tf_amd.train import check_accum_schedule
    check_accum_schedule(7, 3, 1)              # A = 1: anything goes
    check_accum_schedule(8, "epoch", 4)
    check_accum_schedule(8, 12, 4)
    with pytest.raises(ValueError, match="steps_per_epoch"):
        check_accum_schedule(7, "epoch", 2)
    with pytest.raises(ValueError, match="save_freq"):
        check_accum_schedule(8, 3, 2)


def test_fit_raises_before_any_gpu_work():
    """`fit` checks the schedule before it touches the data or the device: a Trainer that owns nothing but its settings"""
    from x3d_tf_amd.train import Trainer
    cfg = x.get_config("XS", ["SOLVER.ACCUM_STEPS", 2])
    t = Trainer.__new__(Trainer)
    t.cfg, t.solver, t.model = cfg, solver_settings(cfg), None

    class Untouched:
        def __iter__(self):
            raise AssertionError("fit read the dataset before checking the schedule")

    with pytest.raises(ValueError, match="steps_per_epoch"):
        t.fit(Untouched(), epochs=1, steps_per_epoch=3)
    with pytest.raises(ValueError, match="save_freq"):
        t.fit(Untouched(), epochs=1, steps_per_epoch=4, save_freq=3)
