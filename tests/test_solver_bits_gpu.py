"""Every entry point of csrc/solver.hip still writes the bits it wrote before the kernels were rewritten around the two walkers.

tests/golden/solver_bits.json holds the SHA-256 of every output buffer (w, the slots, ema, acc, out, partials[:used], q) of
tools/solver_digest.py's fixed inputs -- the flat CASES of test_solver_gpu.py and the chunk layout of test_layerwise_gpu.py, over
the extras {none, clipping norm, non-clipping norm, ema, norm + ema}, both alignment paths, a non-finite gradient -- recorded on
an MI355X with the library of the commit the file names, built by the hipcc the file names.

The digests belong to that source and that compiler: a change that is meant to alter a rounding, the element -> thread map or
a reduction order, or a new compiler that contracts the fp64 sums differently, records the file anew with the tool (and says so);
this test has no tolerance, no skip and no way to re-record."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("solver_digest", os.path.join(ROOT, "tools", "solver_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_solver_outputs_have_the_recorded_bits(gpu):
    with open(os.path.join(ROOT, "tests", "golden", "solver_bits.json")) as fh:
        golden = json.load(fh)
    want = golden["digests"]
    got = _tool().digests(gpu)
    assert list(got) == list(want), "the entries differ: " + str(sorted(set(got) ^ set(want))[:5])
    first = next((k for k in want if got[k] != want[k]), None)
    bad = sum(got[k] != want[k] for k in want)
    assert first is None, (f"{bad} of {len(want)} buffers differ from commit {golden['commit'][:12]} ({golden['hipcc']}); "
                           f"the first: {first}")
