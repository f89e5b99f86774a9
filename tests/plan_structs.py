"""What the kernels are handed for every kind of plan: one line per (case, launch) with the launch struct SegPlan.c_struct
fills (struct ggl_segplan) and the Python-side facts it does not show.  Not a test module: tests/test_plan_structs.py replays
`table()` on the host engine (tests/test_gpu_parity.py on cuda tensors) and compares it with tests/golden/plan_structs.txt.

The golden file is written from the commit whose plans are being pinned:

    python tests/plan_structs.py > tests/golden/plan_structs.txt

The cases tell the four builders apart (Engine.build_plan, Engine.plan_from_rowptr, sampler.Block and Block.transposed) and
the two ways a GraphPlan is made.  Launches 1, 2 and 3 of each plan are recorded: the row order appears on the second.
"""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SCALARS = ("n_long", "n_chunks", "chunk", "N", "E", "xcd_run_rows", "max_len")
POINTERS = ("rowptr", "perm", "long_rows", "chunk_ptr", "partial", "row_order", "long_order")

UNSORTED = [3, 0, 3, 3, 1, 3, 3, 3, 5, 3, 3, 0]            # N = 6: one row of 8 elements
ROWPTR = [0, 2, 3, 3, 11, 11, 12]                            # the same rows, already grouped
HUBS_FIRST = [r for r in range(8) for _ in range(5)] + list(range(8, 40))   # eight rows of 5 leading 32 rows of 1
EDGES = [[0, 1, 2, 3, 4, 0, 2, 4, 1, 3, 5, 0], [1, 0, 1, 2, 3, 4, 5, 1, 3, 1, 1, 2]]   # 12 edges on 6 nodes, unsorted


def _fact(plan, name, default):
    # (a commit whose builders leave a slot unset answers with the default its readers use)
    return getattr(plan, name, default)


def launches(name, plan, **kw):
    out = []
    for n in (1, 2, 3):
        cs = plan.c_struct(None, **kw)
        out.append(f"{name} launch {n}: " + " ".join(f"{f}={int(getattr(cs, f))}" for f in SCALARS) + " | "
                   + " ".join(f"{f}={'NULL' if not getattr(cs, f) else 'set'}" for f in POINTERS)
                   + f" | is_sorted={bool(plan.is_sorted)} hub_first={bool(_fact(plan, 'hub_first', False))}"
                   f" wperm_none={_fact(plan, 'wperm', None) is None} uid_pos={plan.uid > 0}")
    return out


def table(eng, dev="cpu"):
    """The lines of every case, built on `eng` from tensors on `dev`."""
    from gammagl_amd import sampler

    def i64(v):
        return torch.tensor(v, dtype=torch.int64, device=dev)

    out = []
    for tag, kw in (("plain", {}), ("unsplit", {"unsplit": True}), ("skip_long", {"skip_long": True})):
        out += launches(f"build_plan unsorted chunk4 {tag}", eng.build_plan(i64(UNSORTED), 6, chunk=4), **kw)
    out += launches("build_plan sorted", eng.build_plan(i64(sorted(UNSORTED)), 6))
    out += launches("plan_from_rowptr chunk4", eng.plan_from_rowptr(i64(ROWPTR), 12, chunk=4))
    out += launches("plan_from_rowptr max_len8", eng.plan_from_rowptr(i64(ROWPTR), 12, max_len=8))
    out += launches("build_plan one_row chunk4", eng.build_plan(i64([0] * 5), 1, chunk=4))
    out += launches("build_plan empty", eng.build_plan(i64([]), 3))
    out += launches("build_plan hubs_first chunk4", eng.build_plan(i64(HUBS_FIRST), 40, chunk=4))
    counts = torch.bincount(i64(HUBS_FIRST), minlength=40)
    rowptr = torch.cat([i64([0]), torch.cumsum(counts, 0)])
    out += launches("plan_from_rowptr hubs_first chunk4", eng.plan_from_rowptr(rowptr, len(HUBS_FIRST), chunk=4))
    ei = i64(EDGES)
    gp = eng.graph_plan(ei, 6)
    out += launches("graph_plan fwd", gp.fwd) + launches("graph_plan bwd", gp.bwd)
    keep, eng.chunk = eng.chunk, 4
    try:
        csr = eng.graph_plan_from_csr(gp.fwd.rowptr, gp.col, gp.bwd.rowptr, gp.colT, gp.posT)
    finally:
        eng.chunk = keep
    out += launches("graph_plan_from_csr fwd", csr.fwd) + launches("graph_plan_from_csr bwd", csr.bwd)
    # a sampled block: 3 destination rows, 5 source rows, fan-out 2, 5 of the 6 edge slots used
    blk = sampler.Block(eng, i64([0, 2, 3, 5]), torch.tensor([1, 3, 0, 2, 4, 0], dtype=torch.int32, device=dev),
                        torch.zeros(6, dtype=torch.int64, device=dev), i64([5, 5, 0]), 3, 5, 2)
    out += launches("block plan", blk.plan) + launches("block transposed", blk.transposed()[0])
    return out


if __name__ == "__main__":
    import gammagl_amd

    print("\n".join(table(gammagl_amd.host_engine())))
