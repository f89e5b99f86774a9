"""-m gpu: the edge-softmax aggregate on per-edge logits (ggl_edge_softmax_agg_*) on the MI355X, through the ctypes engine,
``torch.ops.ggl_attn`` and ``torch.ops.gammagl_amd``: the host suite's cases on cuda tensors (tests/edge_softmax_agg_cases.py;
here 1 x 64, 4 x 24 and 8 x 41 take the wide backward kernel), the arxiv-sized synthetic graph against the general f32 GAT
kernels on the same machine, run-to-run bits and hipGraph capture of forward + backward."""
import pytest
import torch

import edge_softmax_agg_cases as ec
import gat16_cases as gc
from spmm16_cases import same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; the HIP path has no fallback")
    from gammagl_amd import engine

    return engine()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def routes(eng):
    return ec.make_routes(eng)


@pytest.mark.parametrize("kind", ec.KINDS)
def test_equals_the_general_gat_kernels_bit_for_bit_gpu(routes, eng, dev, kind):
    assert ec.check_contract(routes, eng, dev, kind) == len(ec.SHAPES) * 2


def test_gz_is_in_the_callers_order_and_sums_to_ger_gpu(eng, dev):
    ec.check_gz_order(eng, dev)


def test_exact_corner_cases_gpu(routes, eng, dev):
    ec.check_one_edge_per_destination(routes, eng, dev)
    ec.check_f32_accumulation(routes, dev)
    ec.check_inf_and_nan_rows(routes, eng, dev)


def test_equality_on_a_plan_with_long_rows_gpu(eng, dev):
    """chunk = 64, long rows both ways; at 4 x 24 and 8 x 44 the wide backward kernel meets hub chunks"""
    ec.check_long_rows(eng, dev)


def test_against_float64_gpu(routes, eng, dev):
    ec.check_against_f64(routes["torch.ops.ggl_attn"], eng, dev)


def test_dropout_state_discipline_gpu(eng, dev):
    ec.check_dropout_state(eng, dev)


def test_routes_refusals_and_plumbing_gpu(routes, eng, dev):
    ec.check_routes_agree(routes, eng, dev)
    ec.check_refusals(routes, eng, dev)
    ec.check_one_sided_gradients(routes, eng, dev)
    ec.check_public_function(eng, dev)


def test_agnnconv_fused_against_the_composition_in_float64_gpu(eng, dev):
    ec.check_agnn(dev)


@pytest.fixture(scope="module")
def arxiv(eng, dev):
    from gammagl_amd.synth import DATASETS, rmat_graph

    n, e, _, _ = DATASETS["arxiv"]
    ei = rmat_graph(n, e, seed=0, device=dev)
    gp = eng.graph_plan(ei, n)
    assert gp.fwd.n_long > 0, "the arxiv-sized plan is meant to have hub rows"
    return n, ei, gp


@pytest.mark.parametrize("shape", ((8, 8), (4, 24), (1, 64)))
def test_arxiv_size_against_the_general_gat_kernels(eng, routes, dev, arxiv, shape):
    """§1's equality on EVERY row of the arxiv-sized graph (hub rows through the chunk items and the merges), the same bits
    twice in a row, and the engine route and torch.ops.ggl_attn agreeing"""
    n, ei, gp = arxiv
    H, C = shape
    g = torch.Generator(device=dev).manual_seed(5)
    el, er, x, go = gc.make_inputs(n, n, H, C, g, dev)
    z, _ = ec.make_z(ei, el, er)
    ec.check_equality({"torch.ops.ggl_attn": routes["torch.ops.ggl_attn"]}, eng, gp, ei, el, er, x, go, n, 0.0, 9,
                      ("arxiv", H, C))
    r1 = ec.run_route(routes["torch.ops.ggl_attn"], eng, ei, z, x, go, n, 0.0, 0)
    r2 = ec.run_route(routes["torch.ops.ggl_attn"], eng, ei, z, x, go, n, 0.0, 0)
    re = ec.run_route(routes["engine"], eng, ei, z, x, go, n, 0.0, 0)
    for a, b, c, what in zip(r1, r2, re, ("out", "gz", "gx")):
        assert same_bits(a, b), ("run to run", what)
        assert same_bits(a, c), ("engine route", what)


def test_forward_and_backward_capture_into_one_hipgraph(eng, routes, dev, arxiv):
    """forward + backward recorded into one hipGraph and replayed twice: the eager bits"""
    n, ei, gp = arxiv
    H, C = 8, 8
    g = torch.Generator(device=dev).manual_seed(7)
    el, er, x, go = gc.make_inputs(n, n, H, C, g, dev)
    z, _ = ec.make_z(ei, el, er)
    route = routes["torch.ops.ggl_attn"]
    want = ec.run_route(route, eng, ei, z, x, go, n, 0.0, 0)
    want = ec.run_route(route, eng, ei, z, x, go, n, 0.0, 0)       # (the plan has been seen: nothing is built during the capture)
    za, xa = (t.clone().requires_grad_(True) for t in (z, x))
    leaves = (za, xa)

    def step():
        y = route(ei, za, xa, n, 0.0)
        y.backward(go)
        return y

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            for t in leaves:
                t.grad = None
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    for t in leaves:
        t.grad = None
    with torch.cuda.graph(graph):
        y = step()
    for _ in range(2):
        y.zero_()
        for t in leaves:
            t.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, exp, what in zip((y.detach(), za.grad, xa.grad), want, ("out", "gz", "gx")):
            assert same_bits(got, exp), what
