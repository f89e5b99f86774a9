"""Scaled dot-product graph attention (Engine.dot_attention, utils.dot_attention, torch.ops.ggl_attn.dot_attention,
torch.ops.gammagl_amd.dot_attention, layers.HGTConv) on the HOST library, CPU tensors: the composed route (edge dot +
ggl_edge_softmax_agg_fwd) and the backward both routes share.  Every test here fails on the parent commit: the op does not
exist.  Cases: tests/dot_attention_cases.py."""
import os
import subprocess

import pytest
import torch

import dot_attention_cases as dc
from spmm16_cases import same_bits

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
    return dc.make_routes(eng)


@pytest.mark.parametrize("p", dc.DROPS)
@pytest.mark.parametrize("H,C", dc.SHAPES)
def test_everything_behind_the_logits_is_the_existing_op(eng, H, C, p):
    """out / gv against edge_softmax_aggregate on the returned z, gq / gk against mpops.bspmm on its gz * scale, bit for bit;
    z within the gamma bound; hub row chunked and whole; no logits kept without grad.  CPU tensors take the composed route"""
    assert dc.check_contract(eng, DEV, H, C, p) == [False, False]


def test_one_sided_gradients(eng):
    dc.check_one_sided_gradients(eng, DEV)


def test_single_needs_have_the_aggregates_backward_bits(routes, eng):
    dc.check_single_needs_against_the_aggregate(routes, eng, DEV)


def test_routes_agree(routes, eng):
    dc.check_routes_agree(routes, eng, DEV)


def test_refusals(routes, eng):
    dc.check_refusals(routes, eng, DEV)


def test_public_function(eng):
    dc.check_public_function(eng, DEV)


def test_against_float64(eng):
    dc.check_against_f64(eng, DEV)


def test_a_forward_without_grad_keeps_no_logits(eng):
    """through the engine: nothing is saved for a backward when no input requires grad or grad mode is off (the fused
    forward then forms no [E, H] array at all: tests/test_gpu_dot_attention.py measures it)"""
    index = dc.make_graph(DEV)
    q, k, v, _ = dc.make_qkv(2, 16, DEV)
    out = eng.dot_attention(index, q, k, v, dc.N_DST)
    assert out.grad_fn is None and not eng.stats["dot_attention"]["logits_saved"]
    qa = q.clone().requires_grad_(True)
    with torch.no_grad():
        o2 = eng.dot_attention(index, qa, k, v, dc.N_DST)
    assert not eng.stats["dot_attention"]["logits_saved"] and same_bits(o2, out)
    o3 = eng.dot_attention(index, qa, k, v, dc.N_DST)
    assert eng.stats["dot_attention"]["logits_saved"] and o3.grad_fn is not None


def test_dispatcher_contracts(eng):
    """schema, Meta kernels and autograd registration of ggl_attn::dot_attention{,_forward,_backward} and of the
    Python-registered op (torch.library.opcheck on CPU tensors); the passes on their own"""
    from gammagl_amd import cpp_ops, torch_ops

    index = dc.make_graph(DEV)
    q, k, v, go = dc.make_qkv(2, 8, DEV)
    n = dc.N_DST
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    A = cpp_ops.load_attn()
    for ns in (A, torch_ops.ops):
        torch.library.opcheck(ns.dot_attention.default, (index, q, k, v, n, None, 0.0), test_utils=utils)
        torch.library.opcheck(ns.dot_attention.default,
                              (index, *(t.clone().requires_grad_(True) for t in (q, k, v)), n, 0.5, 0.0), test_utils=utils)
        torch.library.opcheck(ns.dot_attention.default,
                              (index, q[:, 0].contiguous(), k[:, 0].contiguous(), v[:, 0].contiguous(), n, None, 0.0),
                              test_utils=utils)
    two = ("test_schema", "test_faketensor")
    for keep in (True, False):
        torch.library.opcheck(A.dot_attention_forward.default, (index, q, k, v, n, 0.25, 0.0, keep), test_utils=two)
    out, rmax, rden, used, z = A.dot_attention_forward(index, q, k, v, n, 0.25, 0.0, True)
    assert out.shape == (n, 2, 8) and rmax.shape == rden.shape == (n, 2) and used.numel() == 0 and z.shape == (dc.E, 2)
    assert A.dot_attention_forward(index, q, k, v, n, 0.25, 0.0, False)[4].numel() == 0
    for need in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
        torch.library.opcheck(A.dot_attention_backward.default,
                              (index, q, k, v, z, go, out, rmax, rden, used, n, 0.25, 0.0, *need), test_utils=two)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    A.dot_attention(index, *leaves, n, 0.25, 0.0).backward(go)
    gq, gk, gv = A.dot_attention_backward(index, q, k, v, z, go, out, rmax, rden, used, n, 0.25, 0.0, True, True, True)
    assert all(same_bits(a, b.grad) for a, b in zip((gq, gk, gv), leaves))
    assert all(t.numel() == 0 for t in A.dot_attention_backward(index, q, k, v, z, go, out, rmax, rden, used, n, 0.25, 0.0,
                                                                  False, False, False))
    qm, km, vm, im = (t.to("meta") for t in (q, k, v, index))
    for ns in (A, torch_ops.ops):
        assert ns.dot_attention(im, qm, km, vm, n, None, 0.0).shape == (n, 2, 8)
        assert ns.dot_attention(im, qm[:, 0], km[:, 0], vm[:, 0], n, None, 0.0).shape == (n, 8)
    # nothing new under ggl::
    assert not hasattr(cpp_ops.load(), "dot_attention")


def test_c_abi_surface(eng):
    """three additive symbols, bound with the header's parameter counts; the ABI number stays; the host build answers
    "not supported" and fails the launch loudly"""
    from gammagl_amd import _lib

    assert _lib.ABI_VERSION == 12 and eng.lib.ggl_abi_version() == 12
    for name, n in (("ggl_dot_attn_supported", 2), ("ggl_policy_dot_attn_fused", 4), ("ggl_dot_attn_fwd", 15)):
        assert len(_lib.SIGNATURES[name][1]) == n
    for H, C in dc.SHAPES:
        assert eng.lib.ggl_dot_attn_supported(H, C) == 0 and eng.lib.ggl_policy_dot_attn_fused(H, C, dc.E, dc.N_SRC) == 0
    index = dc.make_graph(DEV)
    q, k, v, _ = dc.make_qkv(2, 8, DEV)
    gp = eng.graph_plan(index, dc.N_DST, dc.N_SRC)
    rc, *_ = dc.raw_dot_forward(eng, gp, q, k, v, 1.0, 0.0, None)
    assert rc == _lib.GGL_EINVAL and b"GPU build only" in eng.lib.ggl_last_error()


def test_hgtconv_fused_against_the_message_formula_and_float64(eng):
    dc.check_hgt(DEV)
