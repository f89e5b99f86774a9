"""The launch struct of every kind of plan on the host engine: each (case, launch) of tests/plan_structs.py gives the line
recorded in tests/golden/plan_structs.txt (written from 5a5a65d, where a SegPlan was still assembled field by field by its
four builders)."""
import os

import plan_structs

HERE = os.path.dirname(os.path.abspath(__file__))


def want():
    return open(os.path.join(HERE, "golden", "plan_structs.txt")).read().splitlines()


def test_every_plan_hands_the_kernels_what_it_did():
    import gammagl_amd

    got = plan_structs.table(gammagl_amd.host_engine())
    assert len(want()) == 48 and [g.split(": ")[0] for g in got] == [w.split(": ")[0] for w in want()]
    wrong = [(g, w) for g, w in zip(got, want()) if g != w]
    assert not wrong, wrong


def test_the_table_tells_the_builders_apart():
    """hub_first / xcd_run_rows = -1 only through build_plan, wperm only on a CSR-built CSC side, no row order ever for a
    one-row plan or a sampler Block, and on every other plan from its second launch on"""
    rows = {w.split(": ")[0]: w for w in want()}
    assert "xcd_run_rows=-1" in rows["build_plan hubs_first chunk4 launch 1"] and "hub_first=True" in rows["build_plan hubs_first chunk4 launch 1"]
    assert "xcd_run_rows=0" in rows["plan_from_rowptr hubs_first chunk4 launch 1"]
    assert [k for k, w in rows.items() if "wperm_none=False" in w] == [f"graph_plan_from_csr bwd launch {n}" for n in (1, 2, 3)]
    for k, w in rows.items():
        never = k.startswith(("block ", "build_plan one_row")) or k.endswith("launch 1")
        assert ("row_order=NULL" in w) == never, k
        assert ("uid_pos=False" in w) == k.startswith("block "), k
