"""The edge-softmax aggregate on per-edge logits (ggl_edge_softmax_agg_{fwd,bwd_dst,bwd_src}: the general GAT walks with the
logit read from z [E, H] in the caller's edge order) on the HOST library, CPU tensors, through the ctypes engine, the
C++-registered ``torch.ops.ggl_attn`` and the Python-registered ``torch.ops.gammagl_amd``; and its first consumer,
layers.AGNNConv.  Every test here fails on the parent commit: the op does not exist.  Cases: tests/edge_softmax_agg_cases.py."""
import os
import subprocess

import pytest
import torch

import edge_softmax_agg_cases as ec
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
    return ec.make_routes(eng)


@pytest.mark.parametrize("kind", ec.KINDS)
def test_equals_the_general_gat_kernels_bit_for_bit(routes, eng, kind):
    """out, rowmax, rowden, alpha, gx and gz (= the GAT call's de, in the caller's order) on z = LeakyReLU(el[src] + er[dst]):
    every head shape of the table, with and without attention dropout, the C ABI and all three routes"""
    assert ec.check_contract(routes, eng, DEV, kind) == len(ec.SHAPES) * 2


def test_gz_is_in_the_callers_order_and_sums_to_ger(eng):
    ec.check_gz_order(eng, DEV)


def test_one_edge_per_destination_is_exact(routes, eng):
    ec.check_one_edge_per_destination(routes, eng, DEV)


def test_4096_equal_terms_sum_to_one(routes):
    ec.check_f32_accumulation(routes, DEV)


def test_rows_of_inf_and_nan_logits_behave_as_in_gat(routes, eng):
    ec.check_inf_and_nan_rows(routes, eng, DEV)


def test_equality_on_a_plan_with_long_rows(eng):
    ec.check_long_rows(eng, DEV)


def test_against_float64(routes, eng):
    ec.check_against_f64(routes["engine"], eng, DEV)


def test_dropout_state_discipline(eng):
    ec.check_dropout_state(eng, DEV)


def test_routes_agree(routes, eng):
    ec.check_routes_agree(routes, eng, DEV)


def test_refusals(routes, eng):
    ec.check_refusals(routes, eng, DEV)


def test_one_sided_gradients(routes, eng):
    ec.check_one_sided_gradients(routes, eng, DEV)


def test_public_function(eng):
    ec.check_public_function(eng, DEV)


def test_dispatcher_contracts(eng):
    """schema, Meta kernels and autograd registration of ggl_attn::edge_softmax_aggregate (torch.library.opcheck on CPU
    tensors) and of the Python-registered op; the forward / backward ops on their own; the Meta kernel's shapes"""
    from gammagl_amd import cpp_ops, torch_ops

    g = torch.Generator().manual_seed(3)
    ei = sc.make_index("uniform", 11, 60, g, DEV)
    z = torch.randn(60, 2, generator=g)
    x = torch.randn(11, 2, 8, generator=g)
    go = torch.randn(11, 2, 8, generator=g)
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    A = cpp_ops.load_attn()
    for ns in (A, torch_ops.ops):
        torch.library.opcheck(ns.edge_softmax_aggregate.default, (ei, z, x, 11, 0.0), test_utils=utils)
        torch.library.opcheck(ns.edge_softmax_aggregate.default,
                              (ei, z.clone().requires_grad_(True), x.clone().requires_grad_(True), 11, 0.0), test_utils=utils)
        torch.library.opcheck(ns.edge_softmax_aggregate.default, (ei, z[:, 0].contiguous(), x[:, 0].contiguous(), None, 0.0),
                              test_utils=utils)
    two = ("test_schema", "test_faketensor")
    torch.library.opcheck(A.edge_softmax_aggregate_forward.default, (ei, z, x, 11, 0.0), test_utils=two)
    out, rmax, rden, used = A.edge_softmax_aggregate_forward(ei, z, x, 11, 0.0)
    assert out.shape == (11, 2, 8) and rmax.shape == rden.shape == (11, 2) and used.numel() == 0
    for nz, nx in ((True, True), (True, False), (False, True)):
        torch.library.opcheck(A.edge_softmax_aggregate_backward.default, (ei, z, x, go, out, rmax, rden, used, 11, 0.0, nz, nx),
                              test_utils=two)
    za, xa = z.clone().requires_grad_(True), x.clone().requires_grad_(True)
    A.edge_softmax_aggregate(ei, za, xa, 11, 0.0).backward(go)
    gz, gx = A.edge_softmax_aggregate_backward(ei, z, x, go, out, rmax, rden, used, 11, 0.0, True, True)
    assert sc.same_bits(gz, za.grad) and sc.same_bits(gx, xa.grad)
    gz, gx = A.edge_softmax_aggregate_backward(ei, z, x, go, out, rmax, rden, used, 11, 0.0, False, False)
    assert gz.numel() == 0 and gx.numel() == 0
    # rectangular: 7 destinations.  The op itself under FakeTensor (its Meta kernel answers), the forward op on meta tensors
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode() as mode:
        zf, xf, eif = mode.from_tensor(z), mode.from_tensor(x), mode.from_tensor(ei)
        assert A.edge_softmax_aggregate(eif, zf, xf, 7, 0.0).shape == (7, 2, 8)
        assert A.edge_softmax_aggregate(eif, zf, xf, None, 0.0).shape == (11, 2, 8)
        assert A.edge_softmax_aggregate(eif, zf[:, 0], xf[:, 0], 7, 0.0).shape == (7, 8)
    zm, xm, eim = z.to("meta"), x.to("meta"), ei.to("meta")
    P = torch_ops.ops
    assert P.edge_softmax_aggregate(eim, zm, xm, 7, 0.0).shape == (7, 2, 8)
    assert P.edge_softmax_aggregate(eim, zm, xm, None, 0.0).shape == (11, 2, 8)
    assert P.edge_softmax_aggregate(eim, zm[:, 0], xm[:, 0], 7, 0.0).shape == (7, 8)
    o, a, b, u = A.edge_softmax_aggregate_forward(eim, zm, xm, 7, 0.0)
    assert o.shape == (7, 2, 8) and a.shape == b.shape == (7, 2) and u.dtype == torch.int64 and o.device.type == "meta"
    # nothing new under ggl::
    assert not hasattr(cpp_ops.load(), "edge_softmax_aggregate")


def test_c_abi_surface(eng):
    """the additive entry points: bound with the header's parameter counts, the rejections of their GAT twins, and the ABI
    number stays"""
    import ctypes

    from gammagl_amd import _lib

    assert _lib.ABI_VERSION == 12 and eng.lib.ggl_abi_version() == 12
    for name, n in (("ggl_edge_softmax_agg_fwd", 12), ("ggl_edge_softmax_agg_bwd_dst", 15), ("ggl_edge_softmax_agg_bwd_src", 9)):
        assert len(_lib.SIGNATURES[name][1]) == n
    g = torch.Generator().manual_seed(4)
    ei = sc.make_index("uniform", 40, 300, g, DEV)
    gp = eng.graph_plan(ei, 40)
    H, C = 2, 8
    z, x = torch.randn(300, H, generator=g), torch.randn(40, H, C, generator=g)
    out, rmax, rden = torch.zeros(40, H, C), torch.zeros(40, H), torch.zeros(40, H)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    cs = gp.fwd.c_struct(None)
    L = eng.lib
    fwd = lambda plan, H_, pd, rng: L.ggl_edge_softmax_agg_fwd(plan, p(gp.col), p(z), p(x), H_, C, pd, rng, p(out), p(rmax),  # noqa: E731
                                                                p(rden), None)
    assert fwd(ctypes.byref(cs), H, 0.0, None) == 0
    assert fwd(None, H, 0.0, None) == _lib.GGL_EINVAL and b"plan is NULL" in L.ggl_last_error()
    assert fwd(ctypes.byref(cs), 0, 0.0, None) == _lib.GGL_EINVAL
    assert fwd(ctypes.byref(cs), H, 1.0, None) == _lib.GGL_EINVAL and b"p_drop" in L.ggl_last_error()
    assert fwd(ctypes.byref(cs), H, 0.5, None) == _lib.GGL_EINVAL and b"rng_state" in L.ggl_last_error()
    assert L.ggl_edge_softmax_agg_fwd(ctypes.byref(cs), p(gp.col), None, p(x), H, C, 0.0, None, p(out), p(rmax), p(rden),
                                      None) == _lib.GGL_EINVAL
    assert L.ggl_edge_softmax_agg_bwd_src(None, p(gp.colT), p(gp.posT), p(z), p(x), H, C, p(out), None) == _lib.GGL_EINVAL


def test_agnnconv_fused_against_the_composition_in_float64(eng):
    ec.check_agnn(DEV)
