"""GATv2's additive graph attention (Engine.gatv2_attention, utils.gatv2_attention, torch.ops.ggl_attn.gatv2_attention,
torch.ops.gammagl_amd.gatv2_attention, layers.GATv2Conv) on the HOST library, CPU tensors: the composed route (logits formed
by torch in edge blocks + ggl_edge_softmax_agg_fwd) and the backward both routes share, whose new walk
(ggl_gatv2_logit_bwd) is held to a serial numpy oracle on the bits.  Every test here fails on the parent commit: the op does
not exist.  Cases: tests/gatv2_cases.py."""
import os
import subprocess

import pytest
import torch

import gatv2_cases as vc
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
    return vc.make_routes(eng)


@pytest.mark.parametrize("p", vc.DROPS)
@pytest.mark.parametrize("H,C", vc.SHAPES)
def test_everything_behind_the_logits_is_the_existing_op(eng, H, C, p):
    """z within the gamma bound and without a sign flip; out against edge_softmax_aggregate on the returned z, g_xr / g_att /
    g_xl against ggl_gatv2_logit_bwd on its gz and gv, bit for bit; empty rows zero; hub row chunked and whole; two calls
    identical; no logits kept without grad.  CPU tensors take the composed route"""
    assert vc.check_contract(eng, DEV, H, C, p) == [False, False]


@pytest.mark.parametrize("H,C", vc.SHAPES)
def test_logit_backward_kernel_has_the_serial_oracle_bits(eng, H, C):
    vc.check_logit_bwd_oracle(eng, DEV, H, C)


def test_composed_logits_are_formed_in_edge_blocks(eng, monkeypatch):
    """the composed route's [E_block, H, C] scratch: a block limit that cuts the 1500 edges into many pieces gives the bits of
    one piece"""
    from gammagl_amd import autograd

    index = vc.make_graph(DEV)
    xl, xr, att, _ = vc.make_inputs(3, 16, DEV)
    _, z = eng.gatv2_attention(index, xl, xr, att, vc.N_DST, return_logits=True)
    monkeypatch.setattr(autograd, "GATV2_BLOCK_BYTES", 4 * 3 * 16 * 101)       # 101 edges per block
    _, z2 = eng.gatv2_attention(index, xl, xr, att, vc.N_DST, return_logits=True)
    assert z.shape == (vc.E, 3) and same_bits(z, z2)


def test_one_sided_gradients(eng):
    vc.check_one_sided_gradients(eng, DEV)


def test_single_needs_have_the_aggregates_backward_bits(routes, eng):
    vc.check_single_needs_against_the_aggregate(routes, eng, DEV)


def test_routes_agree(routes, eng):
    vc.check_routes_agree(routes, eng, DEV)


def test_refusals(routes, eng):
    vc.check_refusals(routes, eng, DEV)


def test_public_function(eng):
    vc.check_public_function(eng, DEV)


def test_against_float64(eng):
    """Worst max|got - truth| / max|truth| over the nine shapes, two dropout rates and two chunkings, measured on the host
    build: out 1.08e-06, g_xl 5.12e-07, g_xr 1.76e-06, g_att 6.56e-07 (bound 1e-5); on the MI355X, fused where supported:
    9.17e-07, 4.64e-07, 1.94e-06, 6.13e-07."""
    vc.check_against_f64(eng, DEV)


def test_a_forward_without_grad_keeps_no_logits(eng):
    index = vc.make_graph(DEV)
    xl, xr, att, _ = vc.make_inputs(2, 16, DEV)
    out = eng.gatv2_attention(index, xl, xr, att, vc.N_DST)
    assert out.grad_fn is None and not eng.stats["gatv2_attention"]["logits_saved"]
    aa = att.clone().requires_grad_(True)
    with torch.no_grad():
        o2 = eng.gatv2_attention(index, xl, xr, aa, vc.N_DST)
    assert not eng.stats["gatv2_attention"]["logits_saved"] and same_bits(o2, out)
    o3 = eng.gatv2_attention(index, xl, xr, aa, vc.N_DST)
    assert eng.stats["gatv2_attention"]["logits_saved"] and o3.grad_fn is not None
    assert set(eng.stats["gatv2_attention"]) == {"fused", "logits_bytes", "logits_saved"}


def test_dispatcher_contracts(eng):
    """schema, Meta kernels and autograd registration of ggl_attn::gatv2_attention{,_forward,_backward} and of the
    Python-registered op (torch.library.opcheck on CPU tensors); the passes on their own; Meta shapes"""
    from gammagl_amd import cpp_ops, torch_ops

    index = vc.make_graph(DEV)
    xl, xr, att, go = vc.make_inputs(2, 8, DEV)
    n = vc.N_DST
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    A = cpp_ops.load_attn()
    for ns in (A, torch_ops.ops):
        torch.library.opcheck(ns.gatv2_attention.default, (index, xl, xr, att, n, 0.2, 0.0), test_utils=utils)
        torch.library.opcheck(ns.gatv2_attention.default,
                              (index, *(t.clone().requires_grad_(True) for t in (xl, xr, att)), n, 0.1, 0.0), test_utils=utils)
        torch.library.opcheck(ns.gatv2_attention.default,
                              (index, xl[:, 0].contiguous(), xr[:, 0].contiguous(), att[0].contiguous(), n, 0.2, 0.0),
                              test_utils=utils)
    two = ("test_schema", "test_faketensor")
    for keep in (True, False):
        torch.library.opcheck(A.gatv2_attention_forward.default, (index, xl, xr, att, n, 0.2, 0.0, keep), test_utils=two)
    out, rmax, rden, used, z = A.gatv2_attention_forward(index, xl, xr, att, n, 0.2, 0.0, True)
    assert out.shape == (n, 2, 8) and rmax.shape == rden.shape == (n, 2) and used.numel() == 0 and z.shape == (vc.E, 2)
    assert A.gatv2_attention_forward(index, xl, xr, att, n, 0.2, 0.0, False)[4].numel() == 0
    for need in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
        torch.library.opcheck(A.gatv2_attention_backward.default,
                              (index, xl, xr, att, z, go, out, rmax, rden, used, n, 0.2, 0.0, *need), test_utils=two)
    leaves = [t.clone().requires_grad_(True) for t in (xl, xr, att)]
    A.gatv2_attention(index, *leaves, n, 0.2, 0.0).backward(go)
    grads = A.gatv2_attention_backward(index, xl, xr, att, z, go, out, rmax, rden, used, n, 0.2, 0.0, True, True, True)
    assert all(same_bits(a, b.grad) for a, b in zip(grads, leaves))
    assert all(t.numel() == 0 for t in A.gatv2_attention_backward(index, xl, xr, att, z, go, out, rmax, rden, used, n, 0.2,
                                                                    0.0, False, False, False))
    lm, rm, am, im = (t.to("meta") for t in (xl, xr, att, index))
    for ns in (A, torch_ops.ops):
        assert ns.gatv2_attention(im, lm, rm, am, n, 0.2, 0.0).shape == (n, 2, 8)
        assert ns.gatv2_attention(im, lm[:, 0], rm[:, 0], am[0], n, 0.2, 0.0).shape == (n, 8)
    fm = A.gatv2_attention_forward(im, lm, rm, am, n, 0.2, 0.0, True)
    assert fm[0].shape == (n, 2, 8) and fm[4].shape == (vc.E, 2)
    # nothing new under ggl::
    assert not hasattr(cpp_ops.load(), "gatv2_attention")


def test_c_abi_surface(eng):
    """five additive symbols, bound with the header's parameter counts; the ABI number stays; the host build answers
    "not supported", fails the fused launch loudly and has the backward walk"""
    from gammagl_amd import _lib

    assert _lib.ABI_VERSION == 12 and eng.lib.ggl_abi_version() == 12
    for name, n in (("ggl_gatv2_supported", 2), ("ggl_policy_gatv2_fused", 4), ("ggl_gatv2_fwd", 15),
                    ("ggl_gatv2_logit_bwd_partial_bytes", 4), ("ggl_gatv2_logit_bwd", 13)):
        assert len(_lib.SIGNATURES[name][1]) == n
    for H, C in vc.SHAPES:
        assert eng.lib.ggl_gatv2_supported(H, C) == 0 and eng.lib.ggl_policy_gatv2_fused(H, C, vc.E, vc.N_SRC) == 0
    index = vc.make_graph(DEV)
    xl, xr, att, _ = vc.make_inputs(2, 8, DEV)
    gp = eng.graph_plan(index, vc.N_DST, vc.N_SRC)
    rc, *_ = vc.raw_gatv2_forward(eng, gp, xl, xr, att, 0.0, None)
    assert rc == _lib.GGL_EINVAL and b"GPU build only" in eng.lib.ggl_last_error()
    assert eng.lib.ggl_gatv2_logit_bwd_partial_bytes(0, 2, 8, 1) == 0
    assert eng.lib.ggl_gatv2_logit_bwd_partial_bytes(5, 2, 8, 0) >= 5 * 16 * 4
    assert eng.lib.ggl_gatv2_logit_bwd_partial_bytes(5, 2, 8, 1) >= 2 * 5 * 16 * 4


def test_gatv2conv_paper_against_the_message_formula_and_float64(eng):
    vc.check_conv_paper(DEV)


def test_gatv2conv_reference_variant_against_float64(eng):
    vc.check_conv_reference(DEV)
