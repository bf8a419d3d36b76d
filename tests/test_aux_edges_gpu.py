"""The head, the squeeze-excite path, the slab reducer, the plane-wise kernels, the layout converter and the grid-stride
reductions at the edges of their tiles (tests/shapes.py AUX_EDGE; tests/test_aux_edges.py keeps the table on the edges), against
fp64 on the GPU with the runners and the derived limits of tests/aux_checks.py: the fp32 summation bound, tol_store, a few fp32
roundings, or bit-equality.  Every output is a view into a larger allocation whose bands must come back untouched, and starts as
NaN (an accumulator: as its non-zero pre-fill), so an unwritten element fails as surely as a wrong one.  The cases that the host
code refuses before any launch check the status and that no output changed."""
import time

import pytest
import torch

from tests import shapes as S
from tests.aux_checks import _AUX_CASES, _aux_rn

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", S.AUX_EDGE, ids=[S.aux_edge_id(c) for c in S.AUX_EDGE])
def test_aux_edge(gpu, case):
    """One AUX_EDGE case; prints each check's worst error as a fraction of its limit."""
    t0 = time.time()
    rn, g_ = _aux_rn(gpu, 7000 + S.AUX_EDGE.index(case))
    msg = _AUX_CASES[case[0]](gpu, case, rn, g_, edge=True)
    torch.cuda.synchronize()
    print(f"edge {S.aux_edge_id(case)}: worst err / limit {msg}; {time.time() - t0:.2f} s")
