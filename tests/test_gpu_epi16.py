"""-m gpu: the fused epilogue on 16-bit rows (ggl_spmm_epi_x16, ggl_bias_act_{fwd,bwd}_x16) on the MI355X, through the ctypes
engine and ``torch.ops.ggl``: the host suite's cases on cuda tensors (tests/epi16_cases.py), then the arxiv-sized synthetic
graph against the f32 op on the same machine and hipGraph capture of forward + backward with dropout.  Every comparison is on
the bits."""
import pytest
import torch

import epi16_cases as ec

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


def test_epilogue_ops_accept_16_bit_rows_gpu(eng, dev):
    ec.check_accepts(eng, dev)
    ec.check_sage_accepts(dev)


def test_contract_bit_for_bit_gpu(routes, dev):
    n = ec.check_contract(routes, dev)
    assert n == (len(ec.WIDTHS) + len(ec.KINDS) - 1) * len(ec.DTYPES) * 2 * len(ec.FORMS) * 2
    ec.check_mean_forms(routes, dev)


def test_dropout_keeps_about_half_gpu(eng, dev):
    ec.check_kept_share(eng, dev)


def test_one_rounding_at_the_store_gpu(eng, routes, dev):
    """row 0 holds 4111 / 4097 edges: a hub row (the default chunk is shorter), so the value under test is the one
    long_final_kernel rounds at its 16-bit store"""
    ec.check_one_rounding(routes, dev)
    n = 4111
    ei = torch.stack([torch.arange(n, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)])
    assert eng.graph_plan(ei, n).fwd.n_long > 0


def test_contract_on_a_plan_with_long_rows_gpu(routes, dev):
    """chunk = 64: the 16-bit hub walk into the epilogue, and the f32 chunk partials of the mean backward"""
    ec.check_long_rows(routes, dev)


def test_column_blocks_give_the_one_launch_bits_gpu(eng, dev):
    ec.check_column_blocks(eng, dev)


def test_bias_act_alone_gpu(routes, dev):
    ec.check_bias_act(routes, dev)


def test_still_refuses_what_it_refused_gpu(routes, dev):
    ec.check_refusals(routes, dev)


def test_layers_are_their_parts_gpu(eng, dev):
    ec.check_sage_parts(eng, dev)
    ec.check_gcn_model_parts(eng, dev)
    ec.check_trainers(dev)


def test_dispatcher_and_c_abi_gpu(eng, dev):
    ec.check_dispatcher(eng, dev)
    ec.check_c_abi(eng, dev)


def _graph(name, dev):
    from gammagl_amd.layers import calc_gcn_norm
    from gammagl_amd.synth import DATASETS, rmat_graph

    n, e, _, _ = DATASETS[name]
    ei = rmat_graph(n, e, seed=0, device=dev)
    return n, ei, calc_gcn_norm(ei, n).contiguous()


def test_arxiv_size_against_the_f32_op(eng, routes, dev):
    n, ei, w = _graph("arxiv", dev)
    assert eng.graph_plan(ei, n).fwd.n_long > 0, "the arxiv-sized plan is meant to have hub rows"
    g = torch.Generator(device=dev).manual_seed(5)
    for K in (64, 256):
        x = torch.randn(n, K, generator=g, device=dev)
        go = torch.randn(n, K, generator=g, device=dev)
        for dt in ec.DTYPES:
            for route in routes:
                ec.check_case(route, dev, ei, n, w, x.to(dt), go.to(dt), "bias_relu_drop", "arxiv")


def test_forward_and_backward_with_dropout_capture_into_hipgraphs(eng, routes, dev):
    """forward + backward (bias + ReLU + dropout 0.5, K = 64, bf16) captured once for the 16-bit and once for the f32 op after
    the same reseed: replay i of the 16-bit graph is replay i of the f32 graph, rounded; the two replays differ from each
    other (the state lives on the device and advances inside the graph: a new mask per replay)"""
    n, ei, w = _graph("arxiv", dev)
    K, p = 64, 0.5
    g = torch.Generator(device=dev).manual_seed(7)
    x16 = torch.randn(n, K, generator=g, device=dev).bfloat16()
    bias = torch.randn(K, generator=g, device=dev)
    go16 = torch.randn(n, K, generator=g, device=dev).bfloat16()
    route = routes[1]      # torch.ops.ggl

    def record(x, go):
        xs = x.clone().requires_grad_(True)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):       # (plans, sorted weights and the side stream exist before the capture)
                xs.grad = None
                route.fwd(ei, n, w, xs, False, None, bias, True, p).backward(go)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        eng.reseed(ec.SEED)
        with torch.no_grad():        # (the first draw after a reseed creates the device state: outside the capture)
            route.fwd(ei, n, w, x, False, None, bias, True, p)
        graph = torch.cuda.CUDAGraph()
        xs.grad = None
        with torch.cuda.graph(graph):
            y = route.fwd(ei, n, w, xs, False, None, bias, True, p)
            y.backward(go)
        outs = []
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            outs.append((y.detach().clone(), xs.grad.clone()))
        return outs

    r32 = record(x16.float(), go16.float())
    r16 = record(x16, go16)
    for i in range(2):
        assert ec.same_bits(r16[i][0], r32[i][0].bfloat16()), ("replay", i)
    assert not ec.same_bits(r16[0][0], r16[1][0]), "a new mask per replay"
    # the gradient of replay i is the stepwise one on replay i's stored output
    for i in range(2):
        y16, gx16 = r16[i]
        ga, _ = route.epi_bwd(go16.float(), y16.float(), bias, True, p, torch.empty(0, dtype=torch.int64, device=dev))
        assert ec.same_bits(gx16, route.aggT(ei, n, w, ga.bfloat16().float(), False).bfloat16()), ("gx of replay", i)
