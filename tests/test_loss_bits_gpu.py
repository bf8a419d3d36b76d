"""The five loss entry points of csrc/loss.hip still write the bits the three files they were gathered from wrote.

tests/golden/loss_bits.json holds SHA-256 digests of probs, loss_rows, kd_rows and dlogits for tools/loss_digest.py's fixed
inputs -- N in {1, 3} x M in {1, 157, 256, 257, 400}; every combination of outputs, probs only included; grad_scale in {1, 1/64};
alpha in {0, 0.5, 1} and T in {1, 4} for the distillation forms; ordinary rows, a dominating logit, a label outside [0, M), NaN
targets, +inf and NaN teacher logits, multi-hot and soft multi-label targets -- recorded on an MI355X with the library of the
commit the file names, built by the hipcc the file names.

The digests belong to that source and that compiler: a change that is meant to alter a rounding or a reduction order, or a new
compiler that contracts the sums differently, records the file anew with the tool (and says so); this test has no tolerance, no
skip and no way to re-record."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("loss_digest", os.path.join(ROOT, "tools", "loss_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_loss_outputs_have_the_recorded_bits(gpu):
    with open(os.path.join(ROOT, "tests", "golden", "loss_bits.json")) as fh:
        golden = json.load(fh)
    want = golden["digests"]
    got = _tool().digests(gpu)
    assert list(got) == list(want), "the entries differ: " + str(sorted(set(got) ^ set(want))[:5])
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, (f"{len(differ)} of {len(want)} digests differ from commit {golden['commit'][:12]} ({golden['hipcc']}); "
                        f"the first: {differ[:5]}")
