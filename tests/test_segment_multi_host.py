"""The fused multi-statistic segment aggregate (Engine.segment_multi, torch.ops.ggl_agg.segment_multi,
torch.ops.gammagl_amd.segment_multi, utils.segment_multi_aggregate), mpops.unsorted_segment_min, the global_*_pool functions and
layers.PNAConv on the HOST library, CPU tensors: the same kernel sources (csrc/multiagg.hpp) one thread at a time.  Every test
here fails on the parent commit, where the symbols, ops and names do not exist.  Cases: tests/segment_multi_cases.py."""
import os
import subprocess

import pytest
import torch

import segment_multi_cases as mc

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
    return mc.make_routes(eng)


@pytest.mark.parametrize("aggs", mc.AGG_SETS, ids="-".join)
@pytest.mark.parametrize("K,C", mc.SHAPES)
def test_forward_and_backward_have_the_serial_oracle_bits(eng, K, C, aggs):
    mc.check_oracle(eng, DEV, K, C, aggs)


@pytest.mark.parametrize("aggs", mc.AGG_SETS, ids="-".join)
@pytest.mark.parametrize("K,C", mc.SHAPES)
def test_bit_equality_with_the_composition(eng, K, C, aggs):
    mc.check_composition(eng, DEV, K, C, aggs)


@pytest.mark.parametrize("aggs", mc.AGG_SETS, ids="-".join)
@pytest.mark.parametrize("K,C", ((8, 8), (48, 16), (75, 75)))
def test_against_float64(eng, K, C, aggs):
    mc.check_against_f64(eng, DEV, K, C, aggs)


def test_ties_and_special_values(eng):
    mc.check_special_values(eng, DEV)


def test_routes_agree(routes, eng):
    mc.check_routes_agree(routes, eng, DEV)


def test_only_what_the_backward_reads_is_saved(eng):
    mc.check_saved_tensors(eng, DEV)


def test_refusals(routes, eng):
    mc.check_refusals(routes, eng, DEV)


def test_c_abi_with_exact_size_buffers(eng):
    mc.check_c_abi(eng, DEV)


def test_dispatcher_contracts(eng):
    """schema, Meta kernels and autograd registration of ggl_agg::segment_multi{,_forward,_backward} and of the
    Python-registered op (torch.library.opcheck on CPU tensors); Meta shapes; nothing new under ggl::"""
    from gammagl_amd import cpp_ops, torch_ops

    ids, x = mc.make_ids(DEV), mc.make_x(20, DEV)
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    A = cpp_ops.load_agg()
    for ns in (A, torch_ops.ops):
        for codes, C in (([1, 2, 3, 5], 5), ([2], 20), ([0, 1, 2, 3, 4, 5], 20)):
            torch.library.opcheck(ns.segment_multi.default, (x, ids, mc.N, codes, C, True), test_utils=utils)
            torch.library.opcheck(ns.segment_multi.default, (x.clone().requires_grad_(True), ids, mc.N, codes, C, False),
                                  test_utils=utils)
    two = ("test_schema", "test_faketensor")
    for want_mean in (True, False):
        torch.library.opcheck(A.segment_multi_forward.default, (x, ids, mc.N, [1, 2, 3, 5], 5, True, want_mean), test_utils=two)
    out, mean, amin, amax = A.segment_multi_forward(x, ids, mc.N, [1, 2, 3, 5], 5, True, True)
    assert out.shape == (mc.N, 80) and mean.shape == amin.shape == amax.shape == (mc.N, 20) and amin.dtype == torch.int32
    o2, m2, a2, b2 = A.segment_multi_forward(x, ids, mc.N, [0], 20, False, True)
    assert o2.shape == (mc.N, 20) and m2.numel() == a2.numel() == b2.numel() == 0
    g = mc.make_g(20, 4, DEV)
    torch.library.opcheck(A.segment_multi_backward.default, (g, x, out, mean, amin, amax, ids, mc.N, [1, 2, 3, 5], 5), test_utils=two)
    xx = x.clone().requires_grad_(True)
    A.segment_multi(xx, ids, mc.N, [1, 2, 3, 5], 5, True).backward(g)
    assert mc.same_bits(A.segment_multi_backward(g, x, out, mean, amin, amax, ids, mc.N, [1, 2, 3, 5], 5), xx.grad)
    xm, im = x.to("meta"), ids.to("meta")
    for ns in (A, torch_ops.ops):
        assert ns.segment_multi(xm, im, mc.N, [1, 3], 20, False).shape == (mc.N, 40)
    assert not hasattr(cpp_ops.load(), "segment_multi")


def test_unsorted_segment_min_all_dtypes(eng):
    mc.check_segment_min(DEV)


def test_global_pools(eng):
    mc.check_pools(DEV)


def test_pnaconv_fused_against_composed_and_float64(eng):
    mc.check_pnaconv(eng, DEV)
