"""A Trainer.step still makes the solver launches it made before the Python side of the optimizer update was written once
(solver.RULES, ops.solver_launch, X3D._apply): the same entry points, in the same order, with the same argument tuples.

tests/golden/solver_launches.json holds what tools/solver_launches.py records -- every hip.call of the solver family during two
steps of each case: the five rules x {no extras, clipping, clipping + EMA} x {plain, FREEZE + LAYER_DECAY}, float16 with dynamic
loss scaling, ACCUM_STEPS = 2; scalars by repr, the model's public buffers by name, other pointers in order of appearance --
recorded on an MI355X with the tree of the commit the file names.

A change that is meant to alter a launch records the file anew with the tool (and says so); this test has no tolerance, no skip
and no way to re-record."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("solver_launches", os.path.join(ROOT, "tools", "solver_launches.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_a_step_makes_the_recorded_solver_launches(gpu):
    with open(os.path.join(ROOT, "tests", "golden", "solver_launches.json")) as fh:
        golden = json.load(fh)
    want = golden["cases"]
    got = _tool().launches(gpu)
    assert list(got) == list(want), "the cases differ: " + str(sorted(set(got) ^ set(want))[:5])
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, (f"{len(bad)} of {len(want)} cases differ from commit {golden['commit'][:12]}; the first, {bad[0]}: "
                     f"got {got[bad[0]]}, recorded {want[bad[0]]}")
