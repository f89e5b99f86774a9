"""gspmm's gradient with respect to its edge weights (ggl_spmm_grad_w: sum and mean, f32 / bf16 / f16 rows) on the HOST
library, CPU tensors, through the ctypes engine, the C++-registered ``torch.ops.ggl`` and the Python-registered
``torch.ops.gammagl_amd``.  Bit comparisons throughout; the float64 comparisons use the dot product's a-priori bound.
Cases: tests/spmm_gradw_cases.py."""
import os
import subprocess

import pytest
import torch

import spmm_gradw_cases as gc

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
    return gc.make_routes(eng)


@pytest.fixture(scope="module")
def namespaces(eng):
    from gammagl_amd import cpp_ops, torch_ops

    return (cpp_ops.load(), torch_ops.ops)


def test_weight_gradient_exists(routes):
    """Fails on the parent commit: gspmm treated the weight as a constant and w.grad stayed None."""
    gc.check_exists(routes, DEV)


def test_f32_sum_is_bspmm_one_head_and_mean_is_sum_of_prescaled(routes, eng):
    n = gc.check_f32(routes, eng, DEV)
    assert n == (len(gc.KINDS) + len(gc.EDGES)) * len(gc.WIDTHS) * 3 * 2


def test_rectangular_graph(eng):
    gc.check_rectangular(eng, DEV)


def test_16_bit_storage_is_the_f32_form_on_widened_rows(routes, eng):
    assert gc.check_x16(routes, eng, DEV) > 0


def test_sums_are_made_in_f32(routes):
    gc.check_f32_accumulation(routes, DEV)


def test_lowered_block_thresholds_are_restored(routes, eng):
    """(the host build runs every width as one launch: one width of the GPU test's case list, on the serial form)"""
    assert gc.check_carried_chain(routes, eng, DEV, f32_widths=(264,), x16_widths=(264,)) > 0


def test_block_width_that_is_not_a_multiple_of_8(eng):
    """(one launch per width in the host build: the GPU test's cases on the serial form, options restored)"""
    gc.check_block_width_not_a_multiple_of_8(eng, DEV)
    assert int(eng.lib.ggl_get_option(b"col_block")) == 64


def test_constant_weight_costs_nothing(routes):
    gc.check_constant_weight_costs_nothing(routes, DEV)


def test_epilogue_weight_gradient_against_float64(eng, namespaces):
    gc.check_epilogue(eng, namespaces, DEV)


def test_gcnconv_learnable_edge_weight_takes_the_fused_route(eng):
    gc.check_gcnconv_learnable_edge_weight(DEV)


def test_propagate_learnable_edge_weight_takes_the_spmm(eng):
    gc.check_propagate_takes_the_spmm(DEV)


def test_max_and_rows_keep_their_behaviour(routes, eng, namespaces):
    gc.check_max_and_rows_unchanged(routes, eng, namespaces, DEV)


def test_dispatcher_registration(eng, namespaces):
    """opcheck on the new op and on spmm_sum / spmm_mean with a weight that requires grad; numerical gradients of every
    component of the weight (f32 ops, linear in w: a difference is exact up to the f32 rounding of the outputs)"""
    g = torch.Generator().manual_seed(0)
    ei = torch.randint(0, 11, (2, 60), generator=g)
    xn = torch.randn(11, 4, generator=g)
    gn = torch.randn(11, 4, generator=g)
    w = torch.rand(60, generator=g)
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    for op in gc.grad_w_ops():
        for mean in (False, True):
            torch.library.opcheck(op.default, (ei, xn, gn, mean), test_utils=utils)
            torch.library.opcheck(op.default, (ei, xn.bfloat16(), gn.half(), mean), test_utils=utils)
        assert op(ei, xn, gn, False).dtype == torch.float32
        with pytest.raises(RuntimeError, match="Float"):
            op(ei, xn.double(), gn, False)
        with pytest.raises(RuntimeError, match="row width"):
            op(ei, xn, gn[:, :3], False)
    for ns in namespaces:
        torch.library.opcheck(ns.spmm_sum.default, (ei, w.clone().requires_grad_(True), xn.clone().requires_grad_(True)),
                              test_utils=utils)
        torch.library.opcheck(ns.spmm_mean.default, (ei, w.clone().requires_grad_(True), xn), test_utils=utils)
        for op, mean in ((ns.spmm_sum, False), (ns.spmm_mean, True)):
            # Numerical gradient of EVERY component.  The op is linear in w: <w.grad, dw> == <op(w + dw) - op(w), g> up to
            # the f32 rounding of the three results, for dw = 0.5 e_e (each of the 60 edges) and one random direction.
            # (torch.autograd.gradcheck perturbs w through .data without a version bump, which the sorted-weight cache,
            # keyed on storage and version, cannot see — DESIGN 3.3e; fresh tensors here.)  A row sum of d terms carries
            # gamma(2 d + 1) of its magnitude (the mean's divide is the + 1), gw gamma(K + 1) of its own.
            wl = w.clone().requires_grad_(True)
            y0 = op(ei, wl, xn)
            y0.backward(gn)
            deg = torch.bincount(ei[1], minlength=11).clamp(min=1).double()
            gsc = gn.double() / (deg[:, None] if mean else 1.0)
            mag = (xn.double()[ei[0]] * gsc[ei[1]]).abs().sum(1)
            told = 0
            for dw in list(0.5 * torch.eye(60)) + [torch.rand(60, generator=g) - 0.5]:
                y1 = op(ei, w + dw, xn)
                lhs = (wl.grad.double() * dw.double()).sum()
                rhs = ((y1.double() - y0.detach().double()) * gn.double()).sum()
                absmsg = torch.zeros(11, 4, dtype=torch.float64).index_add_(
                    0, ei[1], xn.double().abs()[ei[0]] * (w.double().abs() + (w + dw).double().abs())[:, None])
                if mean:
                    absmsg = absmsg / deg[:, None]
                bound = gc.gamma(2 * int(deg.max()) + 1) * (absmsg * gn.double().abs()).sum()
                bound = bound + gc.gamma(4 + 1) * (mag * dw.double().abs()).sum()
                assert abs(float(lhs - rhs)) <= float(bound), (str(op), float(lhs - rhs), float(bound))
                told += abs(float(lhs)) > 100 * float(bound)
            assert told >= 45, ("the check must be able to tell a wrong gradient in most components", told)
