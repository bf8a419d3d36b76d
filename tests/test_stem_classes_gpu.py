"""Every kernel instantiation the six stem entry points can dispatch (tests/stem_classes.py: the enumeration of the domain through
the dry-run dispatch x3d_stem_kernel_name), one pytest case per class, each on the class's committed cases against fp64 with the
references and the limits of test_stem / test_stem_fused (tests/stem_checks.py: banded, NaN-prefilled outputs, operands at the
case's offset, every case in each launch form that keeps it in its class, the fused entry points against fp64 directly and bit
for bit against the two-kernel path).

The parametrisation is the committed list tests/golden/stem_classes.json, so collection needs no library; the module fixture
walks the domain (about 10 s on the CPU) and re-dispatches every case of every class before the first launch.  A listed class
the walk no longer reaches fails as such, the others still run; test_enumeration_is_the_committed_list fails with it.
Each case appends its id to a log and flushes before its first launch -- if the process dies, the last line names the case --
and each class its worst error-to-limit ratios afterwards (profiles/stem_classes_mi355x.txt is that log's `class` lines).  The
log is $X3D_STEM_CLASSES_LOG, by default x3d_stem_classes.log in the temporary directory.
"""
import json
import os
import tempfile
import time

import pytest

from tests import stem_classes as SC

pytestmark = pytest.mark.gpu

LISTED = [(e, k) for e, k, _ in json.load(open(SC.GOLDEN))["classes"]]
_broken = []       # a launch error or device fault in one class: the later classes start nothing on that device


@pytest.fixture(scope="module")
def sweep():
    """({class: [Case, ...]}, the open log): the enumeration on this machine, every case re-dispatched into its class."""
    classes = SC.enumerate_classes()
    cases = {cls: SC.class_cases(cls) for cls in classes}
    for cls, cs in cases.items():
        for case in cs:
            assert SC.dispatch(case) == cls, (cls, case)
    path = os.environ.get("X3D_STEM_CLASSES_LOG") or os.path.join(tempfile.gettempdir(), "x3d_stem_classes.log")
    with open(path, "w") as log:
        yield cases, log


def test_enumeration_is_the_committed_list(sweep):
    classes = sorted(sweep[0])
    assert len(classes) >= SC.CLASSES_AT_LEAST, f"{len(classes)} classes: the enumeration on this machine is smaller than the CPU one"
    assert classes == sorted(LISTED), ("the enumeration differs from tests/golden/stem_classes.json: not listed "
                                       f"{sorted(set(classes) - set(LISTED))}, not reached {sorted(set(LISTED) - set(classes))}")


@pytest.mark.parametrize("cls", LISTED, ids=[SC.class_id(c) for c in LISTED])
def test_class_matches_fp64(gpu, sweep, cls):
    from tests import stem_checks
    cases, log = sweep
    assert cls in cases, f"{SC.class_id(cls)} is listed in tests/golden/stem_classes.json but the walk no longer reaches it"
    assert not _broken, f"not run: an earlier class ended in a launch error or device fault ({_broken[0]})"
    t0 = time.time()
    worst, fails = {}, []
    for case in cases[cls]:
        where = f"{SC.class_id(cls)} {SC.case_id(case)}"
        log.write(f"case {where}\n")
        log.flush()
        os.fsync(log.fileno())
        try:
            for name, frac in stem_checks.run_case(gpu, case, cls).items():
                worst[name] = max(worst.get(name, 0.0), frac)
        except AssertionError as e:       # a parity failure: finish the class, report them all
            fails.append(f"{where}: {str(e)[:400]}")
        except Exception as e:            # anything else (a launch error, a device fault) ends the sweep here
            _broken.append(where)
            raise AssertionError(f"{where}: {type(e).__name__}: {str(e)[:400]}") from e
    line = (f"class {SC.class_id(cls)}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items())
            + f"; {len(cases[cls])} cases, {len(fails)} failed, {time.time() - t0:.2f} s")
    log.write(line + "\n")
    log.flush()
    print(line)
    assert not fails, f"{len(fails)} of {len(cases[cls])} cases failed:\n" + "\n".join(fails)
