"""Every kernel instantiation x3d_dw3d_fwd / x3d_dw3d_bwd can dispatch (tests/dw_classes.py: the enumeration of the domain through
the dry-run dispatch), one pytest case per class, each on the class's committed cases against fp64 with the reference and the
limits of test_dw3d_fwd / test_dw3d_bwd (tests/dw_checks.py: banded, NaN-prefilled outputs, operands at the case's offset, every
forward case in each prologue form -- table, folded BatchNorm -- that keeps it in its class).

The parametrisation is the committed list tests/golden/dw_classes.json, so collection needs no library; the module fixture
walks the domain (about 2 s on the CPU) and re-dispatches every case of every class before the first launch.  A listed class
the walk no longer reaches fails as such, the others still run; test_enumeration_is_the_committed_list fails with it.
Each case appends its id to a log and flushes before its first launch -- if the process dies, the last line names the case --
and each class its worst error-to-limit ratios afterwards (profiles/dw_classes_mi355x.txt is that log's `class` lines).  The
log is $X3D_DW_CLASSES_LOG, by default x3d_dw_classes.log in the temporary directory.

Measured on one MI355X: 250 classes, 3 568 cases (1 505 of the 1 585 forward cases also with the folded BatchNorm), 11 s for the
file with the walk; the slowest class 0.5 s (the first, which
loads the kernels), every other at most 0.2 s.  With deliberately wrong libraries (profiles/dw_classes_mi355x.txt lists them)
the classes of the mutated kernel go red and the rest stay green.
"""
import json
import os
import tempfile
import time

import pytest

from tests import dw_classes as DC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dw_classes.json")
LISTED = [(e, k) for e, k, _ in json.load(open(GOLDEN))["classes"]]
_broken = []       # a launch error or device fault in one class: the later classes start nothing on that device


@pytest.fixture(scope="module")
def sweep():
    """({class: [Case, ...]}, the open log): the enumeration on this machine, every case re-dispatched into its class."""
    classes = DC.enumerate_classes()
    cases = {cls: DC.class_cases(cls) for cls in classes}
    for cls, cs in cases.items():
        for case in cs:
            assert DC.dispatch(case) == cls, (cls, case)
    path = os.environ.get("X3D_DW_CLASSES_LOG") or os.path.join(tempfile.gettempdir(), "x3d_dw_classes.log")
    with open(path, "w") as log:
        yield cases, log


def test_enumeration_is_the_committed_list(sweep):
    classes = sorted(sweep[0])
    assert len(classes) >= DC.CLASSES_AT_LEAST, f"{len(classes)} classes: the enumeration on this machine is smaller than the CPU one"
    assert classes == sorted(LISTED), ("the enumeration differs from tests/golden/dw_classes.json: not listed "
                                       f"{sorted(set(classes) - set(LISTED))}, not reached {sorted(set(LISTED) - set(classes))}")


@pytest.mark.parametrize("cls", LISTED, ids=[DC.class_id(c) for c in LISTED])
def test_class_matches_fp64(gpu, sweep, cls):
    from tests import dw_checks
    cases, log = sweep
    assert cls in cases, f"{DC.class_id(cls)} is listed in tests/golden/dw_classes.json but the walk no longer reaches it"
    assert not _broken, f"not run: an earlier class ended in a launch error or device fault ({_broken[0]})"
    t0 = time.time()
    worst, fails = {}, []
    for case in cases[cls]:
        where = f"{DC.class_id(cls)} {DC.case_id(case)}"
        log.write(f"case {where}\n")
        log.flush()
        os.fsync(log.fileno())
        try:
            for name, frac in dw_checks.run_case(gpu, case, cls).items():
                worst[name] = max(worst.get(name, 0.0), frac)
        except AssertionError as e:       # a parity failure: finish the class, report them all
            fails.append(f"{where}: {str(e)[:400]}")
        except Exception as e:            # anything else (a launch error, a device fault) ends the sweep here
            _broken.append(where)
            raise AssertionError(f"{where}: {type(e).__name__}: {str(e)[:400]}") from e
    line = (f"class {DC.class_id(cls)}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items())
            + f"; {len(cases[cls])} cases, {len(fails)} failed, {time.time() - t0:.2f} s")
    log.write(line + "\n")
    log.flush()
    print(line)
    assert not fails, f"{len(fails)} of {len(cases[cls])} cases failed:\n" + "\n".join(fails)
