"""Runs the mixed-precision aggregate's cases (tests/spmm16_cases.py) on the AddressSanitizer build of the host-emulated
kernels (launched by tests/test_spmm16_asan.py with LD_PRELOAD=libclang_rt.asan): every id vector and width class — one
element per lane, ragged 16-byte lanes, aligned lanes, column blocks — both dtypes, both output types, forward and backward."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch  # noqa: E402

import spmm16_cases as sc  # noqa: E402
from gammagl_amd import _lib  # noqa: E402
from gammagl_amd.ops import Engine  # noqa: E402

eng = Engine(_lib.bind(os.path.join(HERE, "libggl_emul_asan.so")), require_cuda=False)
dev = torch.device("cpu")
routes = {"engine": sc.engine_route(eng)}

sc.check_contract(routes, dev, N=120, E=2500)
print("contract ok", flush=True)
sc.check_long_rows(eng, dev, N=120, E=6000)
print("long rows ok", flush=True)
for name in (b"col_block_min_edges", b"col_block_min_degree"):
    eng.lib.ggl_set_option(name, 0)
eng.lib.ggl_set_option(b"col_block16", 64)
sc.check_contract(routes, dev, kinds=("power", "duplicates"), widths=(256, 264), N=120, E=2500)
print("column blocks ok", flush=True)
sc.check_f32_accumulation(routes, dev)
print("f32 sums ok", flush=True)
print("ASAN_CLEAN")
