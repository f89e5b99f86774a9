"""Runs the edge-softmax cases (tests/softmax_cases.py) on the AddressSanitizer build of the host-emulated kernels
(launched by tests/test_softmax_asan.py with LD_PRELOAD=libclang_rt.asan): short rows, chunked long rows, ragged
widths, empty segments and E == 0, forward and backward."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch  # noqa: E402

import softmax_cases as sc  # noqa: E402
from gammagl_amd import _lib  # noqa: E402
from gammagl_amd.ops import Engine  # noqa: E402

eng = Engine(_lib.bind(os.path.join(HERE, "libggl_emul_asan.so")), require_cuda=False)
dev = torch.device("cpu")
routes = {"engine": eng.segment_softmax}


def explicit_plan(x, ids, N):
    plan = eng.build_plan(ids, N, chunk=64)
    assert plan.n_long > 0
    return eng.segment_softmax(x, plan)


sc.check_vs_float64(routes, dev, kinds=("power", "sorted"), widths=(1, 3, 8, 47), N=300, E=20_000, plan_route=explicit_plan,
                    log=lambda *_: None)
print("float64 ok", flush=True)
sc.check_winner_and_invariants(routes, eng, dev, N=300, E=20_000, K=4)
print("winner ok", flush=True)
sc.check_edge_cases(routes, dev)
print("edge ok", flush=True)
print("ASAN_CLEAN")
