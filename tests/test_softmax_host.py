"""The edge-softmax op (ggl_segment_softmax_fwd / _bwd) on the HOST library, CPU tensors: through the ctypes engine
(Engine.segment_softmax), the C++-registered ``torch.ops.ggl.segment_softmax`` and the Python-registered
``torch.ops.gammagl_amd.segment_softmax`` — against float64 autograd of gammagl/utils/softmax.py:29-35, the reference-made
fixture, the segment op's own argmax, and each other.  Cases: tests/softmax_cases.py."""
import os
import subprocess

import pytest
import torch

import softmax_cases as sc

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
    from gammagl_amd import cpp_ops, torch_ops

    return {"engine": eng.segment_softmax, "torch.ops.ggl": cpp_ops.load().segment_softmax,
            "torch.ops.gammagl_amd": torch_ops.ops.segment_softmax}


def test_reference_made_fixture(routes, golden):
    sc.check_kat(routes, DEV, golden)


def test_forward_and_gradient_within_1e5_of_float64(eng, routes):
    """Measured on the host library (this test prints every figure): forward 9.1e-8 ... 1.2e-7, gradient 3.3e-7 ... 1.8e-6
    for logits randn x 3 on every id vector and width, while the f32 composition reaches 1.7e-5 forward and 5.9e-5 in the
    gradient on the power-law rows."""
    def explicit_plan(x, ids, N):
        plan = eng.build_plan(ids, N, chunk=256)
        assert plan.n_long > 0
        return eng.segment_softmax(x, plan)

    gen = torch.Generator().manual_seed(0)
    assert eng.seg_plan(sc.make_ids("power", 2000, 200_000, gen, DEV), 2000).n_long > 0, "rows must exceed the default chunk"
    sc.check_vs_float64(routes, DEV, plan_route=explicit_plan)


def test_sharply_peaked_rows(routes):
    """logits randn x 10.  Measured (host library): K = 3 forward 9.9e-8, gradient 5.6e-6 against the composition's
    3.2e-5 ... 3.5e-5; K = 47 forward 1.0e-7, gradient 6.9e-6 against 2.6e-5 ... 2.8e-5 (the composition's figure moves
    from run to run with the order of torch's index_add_)."""
    sc.check_peaked(routes, DEV)


def test_winner_is_the_segment_maximum_and_rows_sum_to_one(eng, routes):
    sc.check_winner_and_invariants(routes, eng, DEV)


def test_edge_cases(routes):
    sc.check_edge_cases(routes, DEV)


def test_hosts_agree_bit_for_bit(routes):
    sc.check_routes_agree(routes, DEV)


def test_public_function_and_fallback(routes):
    sc.check_public_function(DEV, routes["torch.ops.ggl"])


def test_dispatcher_contracts(routes):
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 11, (60,), generator=g)
    x = torch.randn(60, 5, generator=g)
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    for name in ("torch.ops.ggl", "torch.ops.gammagl_amd"):
        op = routes[name]
        torch.library.opcheck(op.default, (x, ids, 11), test_utils=utils)
        torch.library.opcheck(op.default, (x.clone().requires_grad_(True), ids, 11), test_utils=utils)
        xr = x.clone().requires_grad_(True)
        assert op(xr, ids, 11).grad_fn is not None
        with torch.no_grad():
            assert op(xr, ids, 11).grad_fn is None
    from gammagl_amd import cpp_ops

    C = cpp_ops.load()
    y = C.segment_softmax(x, ids, 11)
    go = torch.randn(60, 5, generator=g)
    xr = x.clone().requires_grad_(True)
    C.segment_softmax(xr, ids, 11).backward(go)
    assert torch.equal(C.segment_softmax_backward(go, y, ids, 11), xr.grad)
    torch.library.opcheck(C.segment_softmax_backward.default, (go, y, ids, 11), test_utils=("test_schema", "test_faketensor"))
    # a width the library has no kernel for is an error of the op, never a quiet fall-back (the public function composes)
    for op in routes.values():
        with pytest.raises(RuntimeError):
            op(torch.randn(60, 65, generator=g), ids, 11)
        with pytest.raises(RuntimeError):
            op(x.double(), ids, 11)


def test_abi_10_surface(eng):
    from gammagl_amd import _lib

    assert _lib.ABI_VERSION == 12 and eng.lib.ggl_abi_version() == 12     # (the entry points came with 10; 11 removed forms elsewhere)
    assert eng.lib.ggl_segment_softmax_supported(1) == 1 and eng.lib.ggl_segment_softmax_supported(64) == 1
    assert eng.lib.ggl_segment_softmax_supported(65) == 0 and eng.lib.ggl_segment_softmax_supported(0) == 0
    assert eng.lib.ggl_segment_softmax_partial_bytes(0, 8) == 0
    assert eng.lib.ggl_segment_softmax_partial_bytes(3, 8) >= 3 * 8 * 32
    # lanes per (row, column): a power of two with lanes x K <= 64, 1 for widths that are not a power of two; the option overrides
    pol = eng.lib.ggl_policy_softmax_sublanes
    for K in (1, 2, 4, 8, 16, 32, 64):
        for E, N in ((1 << 27, 1 << 18), (1 << 27, 1 << 21), (1000, 1000)):
            S = pol(K, E, N)
            assert S >= 1 and S & (S - 1) == 0 and S * K <= 64, (K, E, N, S)
    assert pol(1, 1000, 1000) == 1 and pol(1, 1 << 27, 1 << 18) == 1 and pol(8, 1 << 27, 1 << 18) == 1   # the measured default
    assert pol(3, 1 << 27, 1 << 18) == 1 and pol(47, 1 << 27, 1 << 18) == 1
    old = eng.lib.ggl_get_option(b"softmax_sublanes")
    try:
        eng.lib.ggl_set_option(b"softmax_sublanes", 16)
        assert pol(1, 1000, 1000) == 16 and pol(8, 1000, 1000) == 8 and pol(6, 1000, 1000) == 1
        # the host build walks every row with one lane whatever the policy says: same bits
        g = torch.Generator().manual_seed(1)
        ids = sc.make_ids("power", 300, 30_000, g, DEV)
        x = torch.randn(30_000, 4, generator=g) * 3
        go = torch.randn(30_000, 4, generator=g)
        y8, g8 = sc.run(eng.segment_softmax, x, ids, 300, go)
        eng.lib.ggl_set_option(b"softmax_sublanes", 1)
        y4, g4 = sc.run(eng.segment_softmax, x, ids, 300, go)
        assert torch.equal(y8, y4) and torch.equal(g8, g4)
    finally:
        eng.lib.ggl_set_option(b"softmax_sublanes", old)
