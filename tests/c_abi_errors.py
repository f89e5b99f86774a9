"""The argument-error contract of the C ABI: what every entry point that walks a plan (or draws a dropout mask) answers to
a malformed call — the return code and the full ggl_last_error() text.  Not a test module: tests/test_c_abi_errors.py replays
`table()` on the host build and compares it with tests/golden/c_abi_errors.txt, line by line.

The golden file is written from the library of the commit whose contract is being pinned:

    python tests/c_abi_errors.py path/to/libggl_mpops_host.so > tests/golden/c_abi_errors.txt

Host build only (a check that fails to reject must fail in a local process), so the GPU-only entry points (ggl_gat_fast_*,
ggl_gat_sh_*) are not in the table.  Every call is made on a 4-row, 8-edge plan and zeroed buffers: a call that is not
rejected runs to the end.
"""
import ctypes
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

F32, BF16, F16, F64 = 7, 6, 5, 8        # include/ggl_mpops.h dtype codes
N, E, K, H, C = 4, 8, 8, 2, 4

# entry point -> its parameters, by role, in the order of the prototype
ENTRIES = {
    "ggl_segment_sum": "dtype x plan K out stream",
    "ggl_segment_sum_ex": "dtype x x_ld plan K out out_ld accumulate stream",
    "ggl_segment_mean": "dtype x plan K out stream",
    "ggl_segment_max": "dtype x plan K out arg arg_fill stream",
    "ggl_segment_epi": "x plan K mean add add_ld bias relu p_drop rng out stream",
    "ggl_spmm_sum": "plan col w w_by_pos x K out stream",
    "ggl_spmm_sum_ex": "plan col w w_by_pos x x_ld K out out_ld accumulate stream",
    "ggl_spmm_epi_ex": "plan col w w_by_pos x x_ld K out out_ld accumulate mean add add_ld bias relu p_drop rng epi_K epi_col0 "
                       "advance_rng stream",
    "ggl_spmm_sum_bias_act": "plan col w w_by_pos x K bias relu p_drop rng out stream",
    "ggl_spmm_mean": "plan col w w_by_pos x K out stream",
    "ggl_spmm_max": "plan col w w_by_pos x K out arg stream",
    "ggl_spmm_mean_bwd": "plan col w w_by_pos x fwd_rowptr K out stream",
    "ggl_spmm_max_bwd": "plan col w w_by_pos x arg K out stream",
    "ggl_spmm_max_bwd32": "plan col w w_by_pos x arg K out stream",
    "ggl_spmm_max_bwd_mask": "plan col w w_by_pos x mask posT K out stream",
    "ggl_bspmm_sum": "plan col wh w_by_pos x H C out stream",
    "ggl_spmm_sum_x16": "plan col w w_by_pos x_dtype x x_ld K out_dtype out out_ld stream",
    "ggl_spmm_mean_x16": "plan col w w_by_pos x_dtype x x_ld K out_dtype out out_ld stream",
    "ggl_spmm_mean_bwd_x16": "plan col w w_by_pos x_dtype x fwd_rowptr K out_dtype out stream",
    "ggl_gat_fused_fwd": "plan col el er x slope H C p_drop rng out rowmax rowden stream",
    "ggl_gat_fused_bwd_dst": "plan col none el er x g saved rowmax rowden slope H C p_drop rng alpha de ger none stream",
    "ggl_gat_fused_bwd_src": "plan col posT alpha de g H C out gel stream",
    "ggl_gat_fused_fwd_x16": "plan col el er x_dtype x slope H C p_drop rng out_dtype out rowmax rowden stream",
    "ggl_gat_fused_bwd_dst_x16": "plan col el er x_dtype x out_dtype g out_dtype saved rowmax rowden slope H C p_drop rng alpha de "
                                 "ger stream",
    "ggl_gat_fused_bwd_src_x16": "plan col posT alpha de out_dtype g H C x_dtype out gel stream",
    "ggl_edge_softmax_agg_fwd": "plan col z x H C p_drop rng out rowmax rowden stream",
    "ggl_edge_softmax_agg_bwd_dst": "plan col z x g saved rowmax rowden H C p_drop rng alpha gz stream",
    "ggl_edge_softmax_agg_bwd_src": "plan col posT alpha g H C out stream",
    "ggl_gatv2_logit_bwd": "plan col other x gz att slope H C add out att_rows stream",
    "ggl_segment_multi_fwd": "x plan K C aggs n_aggs empty_zero out none none argmax stream",
    "ggl_segment_softmax_fwd": "x plan K out stream",
    "ggl_segment_softmax_bwd": "x g plan K out stream",
    "ggl_bias_act_fwd": "x bias N K relu p_drop rng out stream",
    "ggl_bias_act_bwd": "g x N K relu p_drop rng out gbias workspace workspace_bytes stream",
}

# malformed call -> (the roles it needs, the roles it overrides)
CASES = {
    "null_plan": (("plan",), {"plan": "null"}),
    "chunk_0": (("plan",), {"plan": "chunk0"}),
    "long_rows_no_partial": (("plan",), {"plan": "long"}),
    "partial_too_small": (("plan",), {"plan": "short"}),
    "p_drop_1": (("p_drop",), {"p_drop": 1.0}),
    "p_drop_no_rng": (("p_drop",), {"p_drop": 0.5, "rng": None}),
    "x_ld_below_K": (("x_ld",), {"x_ld": K - 1}),
    "out_ld_below_K": (("out_ld",), {"out_ld": K - 1}),
    "add_ld_below_K": (("add_ld",), {"add_ld": K - 1}),
    "mean_and_accumulate": (("mean", "accumulate"), {"mean": 1, "accumulate": 1}),
    "column_block_outside_row": (("epi_col0",), {"epi_K": K, "epi_col0": 4}),
    "wrong_dtype_pair": (("x_dtype",), {"x_dtype": BF16, "out_dtype": F16}),
    "f32_rows_in_x16": (("x_dtype",), {"x_dtype": F32, "out_dtype": F32}),
    "null_x": (("x",), {"x": None}),
    "null_out": (("out",), {"out": None}),
    "empty_plan_null_everything": ((), {"plan": "empty", "N": 0, "everything": None}),
}


def _plans(keep):
    from gammagl_amd._lib import SegPlanC

    def arr(v, dt):
        a = np.asarray(v, dtype=dt)
        keep.append(a)
        return a.ctypes.data

    def plan(rowptr, n, e, chunk=64, long_rows=None, chunk_ptr=None):
        p = SegPlanC()
        p.rowptr, p.N, p.E, p.chunk = arr(rowptr, np.int64), n, e, chunk
        if long_rows is not None:
            p.long_rows, p.chunk_ptr = arr(long_rows, np.int32), arr(chunk_ptr, np.int64)
            p.n_long, p.n_chunks = len(long_rows), chunk_ptr[-1]
        p.max_len = int(np.diff(rowptr).max()) if n else 0
        return p

    short = plan([0, 5, 6, 7, 8], N, E, chunk=2, long_rows=[0], chunk_ptr=[0, 3])
    short.partial, short.partial_bytes = arr(np.zeros(1 << 12, np.int32), np.int32), 1     # room enough, one byte declared
    return {"ok": plan([0, 2, 4, 6, 8], N, E), "null": None, "chunk0": plan([0, 2, 4, 6, 8], N, E, chunk=0),
            "long": plan([0, 5, 6, 7, 8], N, E, chunk=2, long_rows=[0], chunk_ptr=[0, 3]),     # partial stays NULL
            "short": short, "empty": plan([0], 0, 0)}


def table(lib):
    """one line per (entry point, malformed call): `entry case -> rc text`"""
    keep = []
    plans = _plans(keep)
    scalars = {"dtype": F32, "x_dtype": BF16, "out_dtype": BF16, "K": K, "H": H, "C": C, "N": N, "slope": 0.2, "p_drop": 0.0,
               "relu": 1, "stream": None, "w": None, "bias": None, "add": None, "gbias": None, "rng": None, "none": None,
               "workspace_bytes": 1 << 14, "n_aggs": 2, "empty_zero": 0}
    scalars["aggs"] = (ctypes.c_int * 2)(0, 3)                 # GGL_AGG_SUM, GGL_AGG_MAX
    lines = []
    for name, roles in ENTRIES.items():
        roles = roles.split()
        fn = getattr(lib, name)
        for case, (needs, over) in CASES.items():
            if not all(r in roles for r in needs):
                continue
            args = []
            for r in roles:
                if r == "plan":
                    p = plans[over.get("plan", "ok")]
                    v = ctypes.byref(p) if p is not None else None
                elif r in over:
                    v = over[r]
                elif r in scalars:
                    v = scalars[r]
                elif r in ("x_ld", "out_ld", "add_ld", "accumulate", "mean", "epi_K", "epi_col0", "advance_rng", "w_by_pos",
                           "arg_fill"):
                    v = 0
                elif "everything" in over:
                    v = None                                   # every buffer of the call is NULL
                elif r == "fwd_rowptr":
                    v = plans["ok"].rowptr
                else:                                          # a buffer of its own, zeroed (ids: node 0, position 0)
                    keep.append(np.zeros(1 << 12, np.int32))
                    v = keep[-1].ctypes.data
                args.append(v)
            rc = int(fn(*args))
            lines.append(f"{name} {case} -> {rc}" + (f" {lib.ggl_last_error().decode()}" if rc else ""))
    return lines


if __name__ == "__main__":
    from gammagl_amd import _lib

    print("\n".join(table(_lib.bind(sys.argv[1]))))
