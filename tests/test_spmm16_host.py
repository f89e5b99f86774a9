"""The mixed-precision aggregate (bf16 / f16 rows, f32 sums, one rounding: ggl_spmm_{sum,mean,mean_bwd}_x16) on the HOST
library, CPU tensors, through the ctypes engine, the C++-registered ``torch.ops.ggl`` and the Python-registered
``torch.ops.gammagl_amd``.  Every comparison is on the bits.  Cases: tests/spmm16_cases.py."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import spmm16_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DEV = torch.device("cpu")


@pytest.fixture(scope="module")
def eng():
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "gammagl_amd", "csrc"), "host", "torch"])
    import gammagl_amd

    return gammagl_amd.host_engine()


@pytest.fixture(scope="module")
def routes(eng):
    return sc.make_routes(eng)


def test_gspmm_accepts_16_bit_rows(eng):
    """Fails on the parent commit: gspmm raised "expected scalar type Float" for bf16 / f16 x."""
    sc.check_accepts(DEV)


def test_still_refuses_what_it_refused(routes):
    sc.check_refusals(routes, DEV)


def test_contract_bit_for_bit(routes):
    """out == F(x.float()).to(dtype), f32 output == F(x.float()), x.grad == F's gradient rounded: every id vector, width,
    dtype, weight form and reduce, on all three routes."""
    n = sc.check_contract(routes, DEV)
    assert n == len(sc.KINDS) * len(sc.WIDTHS) * len(sc.DTYPES) * 2 * 2 * 3


def test_contract_on_a_plan_with_long_rows(eng):
    sc.check_long_rows(eng, DEV)


def test_column_blocks_give_the_one_launch_bits(eng):
    sc.check_column_blocks(eng, DEV)


def test_sums_are_made_in_f32(routes):
    sc.check_f32_accumulation(routes, DEV)


def test_gcnconv_is_linear_then_mixed_aggregate_then_torch_epilogue(eng):
    sc.check_gcnconv(DEV)


def test_gcn_model_and_trainer_under_autocast(eng):
    sc.check_model_autocast(DEV)


def test_gcn_trainer_example_runs_with_amp_bf16():
    """examples/gcn_trainer_amd.py --gpu -1 --amp bf16: exits 0, the loss decreases, the accuracy beats chance (7 classes)."""
    env = {k: v for k, v in os.environ.items() if k != "GGL_BENCH_EMUL"}
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "gcn_trainer_amd.py"), "--gpu", "-1", "--n_epoch", "12",
                        "--hidden_dim", "16", "--amp", "bf16"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    losses = [float(m) for m in re.findall(r"train loss: ([0-9.]+)", r.stdout)]
    assert len(losses) >= 2 and losses[-1] < losses[0], r.stdout[-1000:]
    acc = float(re.search(r"Test acc:\s+([0-9.]+)", r.stdout).group(1))
    assert acc > 1.0 / 7 + 0.1, r.stdout[-500:]


def test_dispatcher_contracts(routes):
    """schemas, Meta kernels and autograd registration of the ops that take 16-bit rows; the backward ops on their own"""
    from gammagl_amd import cpp_ops, torch_ops

    g = torch.Generator().manual_seed(3)
    ei = sc.make_index("uniform", 11, 60, g, DEV)
    w = torch.rand(60, generator=g)
    x = torch.randn(11, 8, generator=g).bfloat16()
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    C = cpp_ops.load()
    for ns in (C, torch_ops.ops):
        for op in (ns.spmm_sum, ns.spmm_mean):
            torch.library.opcheck(op.default, (ei, w, x), test_utils=utils)
            torch.library.opcheck(op.default, (ei, w, x.clone().requires_grad_(True)), test_utils=utils)
        for op in (ns.spmm_sum_x16, ns.spmm_mean_x16):
            for f32 in (False, True):
                torch.library.opcheck(op.default, (ei, w, x.clone().requires_grad_(True), f32), test_utils=utils)
            assert op(ei, w, x, True).dtype == torch.float32 and op(ei, w, x, False).dtype == torch.bfloat16
            with pytest.raises(RuntimeError):
                op(ei, w, x.float(), True)
    go = torch.randn(11, 8, generator=g).bfloat16()
    for fwd, bwd in ((C.spmm_sum, C.spmm_sum_backward), (C.spmm_mean, C.spmm_mean_backward)):
        xr = x.clone().requires_grad_(True)
        fwd(ei, w, xr).backward(go)
        assert sc.same_bits(bwd(ei, w, go), xr.grad)
        torch.library.opcheck(bwd.default, (ei, w, go), test_utils=("test_schema", "test_faketensor"))
        with pytest.raises(RuntimeError, match="Float"):
            bwd(ei, w, go.double())


def test_c_abi_surface(eng):
    """the additive entry points: dtype pairs, the block-width option, and the ABI number"""
    from gammagl_amd import _lib

    assert _lib.ABI_VERSION == 12 and eng.lib.ggl_abi_version() == 12     # (they came under 10; 11 removed forms elsewhere)
    g = torch.Generator().manual_seed(4)
    ei = sc.make_index("uniform", 40, 300, g, DEV)
    gp = eng.graph_plan(ei, 40)
    cs = gp.fwd.c_struct(None)
    x = torch.randn(40, 16, generator=g).bfloat16()
    out = torch.empty(40, 16, dtype=torch.float64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    EDTYPE = eng.lib.ggl_spmm_sum_x16(ctypes.byref(cs), p(gp.col), None, 0, 7, p(x), 0, 16, 7, p(out), 0, None)   # f32 rows
    assert EDTYPE != 0
    for xd, od in ((6, 5), (5, 6), (6, 8), (8, 8)):      # bf16 -> f16, f16 -> bf16, bf16 -> f64, f64 rows
        for fn in (eng.lib.ggl_spmm_sum_x16, eng.lib.ggl_spmm_mean_x16):
            assert fn(ctypes.byref(cs), p(gp.col), None, 0, xd, p(x), 0, 16, od, p(out), 0, None) == EDTYPE
    assert eng.lib.ggl_spmm_mean_bwd_x16(ctypes.byref(cs), p(gp.col), None, 0, 6, p(x), p(gp.fwd.rowptr), 16, 8, p(out),
                                         None) == EDTYPE
    # launches per call: one for short / sparse plans, K / col_block16 for wide rows of a dense plan
    blocks = eng.lib.ggl_spmm_col_blocks_x16
    assert blocks(ctypes.byref(cs), 256) == 1 and blocks(None, 256) == 1
    old = (eng.lib.ggl_get_option(b"col_block16"), eng.lib.ggl_get_option(b"col_block_min_edges"),
           eng.lib.ggl_get_option(b"col_block_min_degree"))
    try:
        eng.lib.ggl_set_option(b"col_block_min_edges", 0)
        eng.lib.ggl_set_option(b"col_block_min_degree", 0)
        w = torch.rand(300, generator=g)
        xw = torch.randn(40, 256, generator=g).bfloat16()
        want = None
        for bw, n in ((64, 4), (128, 2), (256, 1), (0, 1), (60, 1)):     # (60: not a multiple of 8 columns -> one launch)
            eng.lib.ggl_set_option(b"col_block16", bw)
            assert eng.lib.ggl_get_option(b"col_block16") == bw and blocks(ctypes.byref(cs), 256) == n, bw
            got = eng.spmm(gp, w, xw, "sum")
            want = got if want is None else want
            assert sc.same_bits(got, want), bw          # columns are independent sums: the same bits at every block width
        assert sc.same_bits(want, eng.spmm(gp, w, xw.float(), "sum").bfloat16())
    finally:
        for name, v in zip((b"col_block16", b"col_block_min_edges", b"col_block_min_degree"), old):
            eng.lib.ggl_set_option(name, v)
