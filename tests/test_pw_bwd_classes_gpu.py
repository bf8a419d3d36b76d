"""Every kernel instantiation x3d_pw_bwd can dispatch (tests/pw_bwd_classes.py: the enumeration of the admitted domain),
each on two seeded shapes inside its class, against the fp64 restatements of tests/test_kernels_gpu.py -- the test bodies and
their tolerances (tol_gemm, _wtol, _stol, the tie slack) exactly as the registered cases use them.

Chunk i runs the classes [i::CHUNKS] of the sorted enumeration; the class list comes from a module-scoped fixture (a 2 - 4 s
dry-run walk on the CPU), not from import time.  Measured on one MI355X: 300 classes, 782 kernel checks, 0.55 - 0.72 s per
chunk of 37 - 38 classes (1.1 s for the first, which loads the kernels), 6.6 s for the file with the walk -- the shapes are
small (at most 5 x 3 500 points) and the fp64 restatements with them, so 8 chunks and not the 40 first planned.  With a
deliberately wrong library (one k-step dropped from the fourth row tile of the MT = 4 panels) every pw_bwd_fused_kernel<., 4, ., .>
class fails in both test_pw_bwd_oracle and test_pw_bwd_fused and no other class does.
"""
import pytest

from tests import pw_bwd_classes as PC

pytestmark = pytest.mark.gpu

CHUNKS = 8
_broken = []       # a launch error or device fault in one chunk: the later chunks start nothing on that device


@pytest.fixture(scope="module")
def classes():
    return sorted(PC.enumerate_classes().items())


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_every_class_matches_the_fp64_restatement(gpu, classes, chunk):
    from tests import test_kernels_gpu as K
    assert len(classes) >= PC.CLASSES_AT_LEAST, f"{len(classes)} classes: the enumeration on this machine is smaller than the CPU one"
    assert not _broken, f"not run: an earlier chunk ended in a launch error or device fault ({_broken[0]})"
    fails, ran = [], 0
    for index in range(chunk, len(classes), CHUNKS):
        name, boxes = classes[index]
        cases, seed, _ = PC.class_cases(index, name, boxes)
        assert len(cases) == PC.DRAWS
        for case in cases:
            assert PC.dispatch(*case) == name
            for fn, args in PC.kernel_calls(case):
                where = f"class {name}, shape {case.shape} ({case.kind}, {case.dtype}), seed {seed}: {fn}"
                try:
                    getattr(K, fn)(gpu, *args)
                except AssertionError as e:       # a parity failure: finish the chunk, report them all
                    fails.append(f"{where}: {str(e)[:400]}")
                except Exception as e:            # anything else (a launch error, a device fault) ends the sweep here
                    _broken.append(where)
                    raise AssertionError(f"{where}: {type(e).__name__}: {str(e)[:400]}") from e
                ran += 1
    print(f"chunk {chunk}: {len(range(chunk, len(classes), CHUNKS))} of {len(classes)} classes, {ran} kernel checks")
    assert not fails, f"{len(fails)} of {ran} kernel checks failed:\n" + "\n".join(fails)
