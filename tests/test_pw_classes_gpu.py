"""Every kernel instantiation x3d_pw_fwd / x3d_pw_dgrad / x3d_pw_wgrad can dispatch (tests/pw_classes.py: the enumeration of
the walked domain), each on its committed cases (pw_classes.class_cases): a ragged and a whole plane in different boxes where its
aligned boxes hold them, the sample-crossing runs of the resident-panel kernel, and offset cases -- every activation operand 1 or
2 elements off its 16-byte alignment, on a ragged plane of more than 128 points, a whole 256-point plane and sample-crossing
runs, wherever the offset launch stays in the class -- against the fp64 restatements of tests/test_kernels_gpu.py: the test
bodies and their tolerances (tol_gemm, tol_store, _stol, _wtol, the tie slack) exactly as the registered cases use them.
The offset is how the scalar kernels (VEC = 1), which take aligned launches only below 8 points per sample, run planes of
several tiles.  32 classes run on 3 points per sample only: the generic fp32 kernels of stride 1 (pw_gemm_kernel<float, 1, ...,
0>, pw_wgrad_kernel<float, 1, ..., 0>), which the dispatch takes below 4 points and nowhere else.

Chunk i runs the classes [i::CHUNKS] of the sorted enumeration; the class list comes from a module-scoped fixture (the dry-run
walk on the CPU), not from import time.  Measured on one MI355X: 676 classes, 1 922 cases (370 of them with offset operands),
2 052 kernel checks; 0.62 - 0.70 s per chunk of 84 - 85 classes, 13.7 s for the file, of which 8.3 s are the walk -- the cases
are small (two to five samples of mostly 129 to 256 points; 1 300 for the resident-panel kernel's runs), and the fp64
restatements with them, so 8 chunks.

No kernel failed: every newly covered class matches its fp64 restatement within the tolerances of the registered cases, so
tests/shapes.py gets no new pinned shape.  That the sweep can see a wrong kernel was shown with two deliberately wrong
libraries (arithmetic only, no address or bound changed).  One k-step's accumulate dropped in the RAG = 1 instantiations of
pw_gemm_wst.h (`if (!(RAG && ks == 1)) acc = mfma(...)`): all 82 classes pw_gemm_wst_kernel<., ., ., ., ., ., ., 1> failed (66 of
x3d_pw_fwd in the training, folded-tail and inference forms, 16 of x3d_pw_dgrad), each in every one of its cases, and no other
class did; 44 of those 82 had no case before this sweep.  The first k-step's accumulate dropped in the scalar
instantiations of pw_gemm_bf16.h (`if (!(VEC == 1 && kk == 0)) acc = mfma(...)`): all 44 classes pw_gemm_bf16_kernel<., 1, ...>
failed (28 of x3d_pw_fwd, 16 of x3d_pw_dgrad) in every one of their 264 checks -- the offset cases on planes of 129 to 1 300
points among them -- and no other class did.
"""
import pytest

from tests import pw_classes as PC

pytestmark = pytest.mark.gpu

CHUNKS = 8
_broken = []       # a launch error or device fault in one chunk: the later chunks start nothing on that device


@pytest.fixture(scope="module")
def classes():
    return sorted(PC.enumerate_classes())


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_every_class_matches_the_fp64_restatement(gpu, classes, chunk):
    from tests import test_kernels_gpu as K
    assert len(classes) >= PC.CLASSES_AT_LEAST, f"{len(classes)} classes: the enumeration on this machine is smaller than the CPU one"
    assert not _broken, f"not run: an earlier chunk ended in a launch error or device fault ({_broken[0]})"
    fails, ran = [], 0
    for index in range(chunk, len(classes), CHUNKS):
        cls = classes[index]
        cases = PC.class_cases(cls)
        assert len(cases) >= 2, cls
        for case in cases:
            assert PC.dispatch(case) == cls, (cls, case)
            for fn, args, kw in PC.kernel_calls(case):
                where = (f"class {cls[0]} {cls[1]}, {case.form} {case.val}, shape {PC.case_shape(case)[:6]}, {case.dtype}"
                         f"{' panel' if case.panel else ''}, offset {case.off}: {fn}{' slab' if fn == 'test_pw_wgrad' and args[2] else ''}")
                try:
                    getattr(K, fn)(gpu, *args, **kw)
                except AssertionError as e:       # a parity failure: finish the chunk, report them all
                    fails.append(f"{where}: {str(e)[:400]}")
                except Exception as e:            # anything else (a launch error, a device fault) ends the sweep here
                    _broken.append(where)
                    raise AssertionError(f"{where}: {type(e).__name__}: {str(e)[:400]}") from e
                ran += 1
    print(f"chunk {chunk}: {len(range(chunk, len(classes), CHUNKS))} of {len(classes)} classes, {ran} kernel checks")
    assert not fails, f"{len(fails)} of {ran} kernel checks failed:\n" + "\n".join(fails)
