"""-m gpu: the fused GAT on 16-bit rows (bf16 / f16 storage, f32 softmax and sums, one rounding: ggl_gat_fused_*_x16) on the
MI355X, through the ctypes engine, ``torch.ops.ggl`` and ``torch.ops.gammagl_amd``: the host suite's cases on cuda tensors
(tests/gat16_cases.py), the wide backward kernel on hub chunks, the arxiv-sized synthetic graph against the general f32
kernels on the same machine, run-to-run bits and hipGraph capture of forward + backward.  Every comparison is on the bits."""
import pytest
import torch

import gat16_cases as gc
from spmm16_cases import same_bits

pytestmark = pytest.mark.gpu
KINDS = gc.KINDS + ("rectangular",)


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
    return gc.make_routes(eng)


def test_gat_fused_accepts_16_bit_rows_gpu(routes, dev):
    gc.check_accepts(routes, dev)


def test_still_refuses_what_it_refused_gpu(routes, eng, dev):
    gc.check_refusals(routes, eng, dev)


@pytest.mark.parametrize("kind", KINDS)
def test_contract_bit_for_bit_gpu(routes, eng, dev, kind):
    """4 x 24 and 8 x 41 (padded to 44 or not) take the wide backward kernel here, 1 x 320 and the narrow heads the
    lane-per-head one; F is the general f32 kernel of the same form"""
    n = gc.check_contract(routes, eng, dev, kind)
    assert n == len(gc.SHAPES) * len(gc.DTYPES) * 2


def test_contract_on_a_plan_with_long_rows_gpu(eng, dev):
    """chunk = 64, long rows both ways; at 4 x 24 and 8 x 44 the 16-bit WIDE backward meets hub chunks"""
    gc.check_long_rows(eng, dev, shapes=((3, 5), (2, 12), (8, 8), (4, 24), (8, 44)))


def test_sums_are_made_in_f32_gpu(routes, dev):
    gc.check_f32_accumulation(routes, dev)


def test_a_panel_one_element_into_its_buffer_gpu(eng, dev):
    """(4 x 24: the wide kernel keeps its four-channel assignment and reads the channels one by one)"""
    gc.check_alignment(eng, dev)


def test_layer_and_model_under_autocast_gpu(eng, dev):
    gc.check_layer_parts(eng, dev)
    gc.check_model_autocast(dev)


@pytest.fixture(scope="module")
def arxiv(eng, dev):
    from gammagl_amd.synth import DATASETS, rmat_graph

    n, e, _, _ = DATASETS["arxiv"]
    ei = rmat_graph(n, e, seed=0, device=dev)
    gp = eng.graph_plan(ei, n)
    assert gp.fwd.n_long > 0, "the arxiv-sized plan is meant to have hub rows"
    return n, ei, gp


def _fwd_bwd(route, eng, ei, el, er, x, go, n, p=0.0, seed=0):
    return gc.run_route(route, eng, ei, el, er, x, go, n, p, False, seed)


@pytest.mark.parametrize("shape", ((8, 8), (4, 24)))
def test_arxiv_size_against_the_general_f32_kernels(eng, routes, dev, arxiv, shape):
    """the contract on EVERY row of the arxiv-sized graph (hub rows through the chunk items and the merges), the same bits
    twice in a row, and the engine route and torch.ops.ggl agreeing"""
    n, ei, gp = arxiv
    H, C = shape
    g = torch.Generator(device=dev).manual_seed(5)
    el, er, x, go = gc.make_inputs(n, n, H, C, g, dev)
    for dt in gc.DTYPES:
        x16, g16 = x.to(dt), go.to(dt)
        rng = gc.drawn_rng(9, dev)
        ref = gc.reference(eng, gp, el, er, x16, g16, 0.0, rng)
        gc.check_raw(eng, gp, el, er, x16, g16, 0.0, rng, ref, ("arxiv", H, C, str(dt)))
        want = ref[False]
        r1 = _fwd_bwd(routes["torch.ops.ggl"], eng, ei, el, er, x16, g16, n)
        for got, exp, what in zip(r1, (ref["out"].to(dt), want["gel"], want["ger"], want["gx"]), ("out", "gel", "ger", "gx")):
            assert same_bits(got, exp), (what, dt)
        r2 = _fwd_bwd(routes["torch.ops.ggl"], eng, ei, el, er, x16, g16, n)
        re = _fwd_bwd(routes["engine"], eng, ei, el, er, x16, g16, n)
        for a, b, c, what in zip(r1, r2, re, ("out", "gel", "ger", "gx")):
            assert same_bits(a, b), ("run to run", what, dt)
            assert same_bits(a, c), ("engine route", what, dt)


def test_forward_and_backward_capture_into_one_hipgraph(eng, routes, dev, arxiv):
    """forward + backward of the bf16 op recorded into one hipGraph and replayed twice: the eager bits"""
    n, ei, gp = arxiv
    H, C = 8, 8
    g = torch.Generator(device=dev).manual_seed(7)
    el, er, x, go = gc.make_inputs(n, n, H, C, g, dev)
    x, go = x.bfloat16(), go.bfloat16()
    route = routes["torch.ops.ggl"]
    want = _fwd_bwd(route, eng, ei, el, er, x, go, n)
    want = _fwd_bwd(route, eng, ei, el, er, x, go, n)       # (the plan has been seen: nothing is built during the capture)
    ea, ra, xa = (t.clone().requires_grad_(True) for t in (el, er, x))
    leaves = (ea, ra, xa)

    def step():
        y = route(ei, ea, ra, xa, gc.SLOPE, n, 0.0)
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
        for got, exp, what in zip((y.detach(), ea.grad, ra.grad, xa.grad), want, ("out", "gel", "ger", "gx")):
            assert same_bits(got, exp), what
