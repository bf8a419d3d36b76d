"""The five residual-tail entry points (csrc/elem.hip) still write the bits their separate kernels wrote before the plain, folded
and drop-path forms were given one body.

tests/golden/tail_bits.json holds SHA-256 digests of y, g (in place), g_branch, sums_c, sums_r and the tables x3d_tail_fwd_bn writes
for tools/tail_digest.py's fixed inputs -- fp32, fp16 and bf16; one vector, a second workgroup per plane in the vector and the
scalar form, an odd plane, P / 8 = 256, the small planes (1, 1, 8), (3, 2, 24) and (17, 2, 392); shortcut coefficients null and
given, no shortcut; four keep tables with NaN in the c_raw of dropped samples; g_branch as the only misaligned pointer; a random
family that pins the reduction order inside a workgroup and a dyadic one whose sums are exact in any order -- recorded on an
MI355X with the library of the commit the file names, built by the hipcc the file names.

The digests belong to that source and that compiler: a change that is meant to alter a rounding or a reduction order, or a new
compiler that contracts the sums differently, records the file anew with the tool (and says so); this test has no tolerance, no
skip and no way to re-record."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("tail_digest", os.path.join(ROOT, "tools", "tail_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_tail_outputs_have_the_recorded_bits(gpu):
    with open(os.path.join(ROOT, "tests", "golden", "tail_bits.json")) as fh:
        golden = json.load(fh)
    want = golden["digests"]
    got = _tool().digests(gpu)
    assert list(got) == list(want), "the entries differ: " + str(sorted(set(got) ^ set(want))[:5])
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, (f"{len(differ)} of {len(want)} digests differ from commit {golden['commit'][:12]} ({golden['hipcc']}); "
                        f"the first: {differ[:5]}")
