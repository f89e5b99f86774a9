"""-m gpu: the mixed-precision aggregate (bf16 / f16 rows, f32 sums, one rounding: ggl_spmm_{sum,mean,mean_bwd}_x16) on the
MI355X, through the ctypes engine, ``torch.ops.ggl`` and ``torch.ops.gammagl_amd``: the host suite's cases on cuda tensors
(tests/spmm16_cases.py), then at size against the f32 op on the same machine — which tests/test_gpu_refsize.py holds
bit-identical to the reference's own extension — the arxiv- and the products-sized synthetic graph, run-to-run bits and
hipGraph capture of forward + backward.  Every comparison is on the bits."""
import ctypes

import pytest
import torch

import spmm16_cases as sc

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
    return sc.make_routes(eng)


def test_gspmm_accepts_16_bit_rows_gpu(eng, dev):
    sc.check_accepts(dev)


def test_still_refuses_what_it_refused_gpu(routes, dev):
    sc.check_refusals(routes, dev)


def test_contract_bit_for_bit_gpu(routes, dev):
    n = sc.check_contract(routes, dev)
    assert n == len(sc.KINDS) * len(sc.WIDTHS) * len(sc.DTYPES) * 2 * 2 * 3


def test_contract_on_a_plan_with_long_rows_gpu(eng, dev):
    """chunk = 64: the long rows go through the 16-bit-source hub walk (light stages, every width class: narrow slabs,
    unaligned rows, 8-byte pieces), the mean backward through f32 chunk partials"""
    gp = sc.check_long_rows(eng, dev)
    assert gp.bwd.n_long > 0, "the transposed plan is meant to have long rows as well"


def test_column_blocks_give_the_one_launch_bits_gpu(eng, dev):
    sc.check_column_blocks(eng, dev)


def test_sums_are_made_in_f32_gpu(routes, dev):
    sc.check_f32_accumulation(routes, dev)


def test_layer_and_model_under_autocast_gpu(eng, dev):
    sc.check_gcnconv(dev)
    sc.check_model_autocast(dev)


def _graph(name, dev):
    from gammagl_amd.layers import calc_gcn_norm
    from gammagl_amd.synth import DATASETS, rmat_graph

    n, e, _, _ = DATASETS[name]
    ei = rmat_graph(n, e, seed=0, device=dev)
    return n, ei, calc_gcn_norm(ei, n).contiguous()


def _fwd_bwd(route, ei, w, x, go):
    xr = x.clone().requires_grad_(True)
    y = route("sum", ei, w, xr)
    y.backward(go)
    return y.detach(), xr.grad


def test_arxiv_size_against_the_f32_op(eng, routes, dev):
    n, ei, w = _graph("arxiv", dev)
    gp = eng.graph_plan(ei, n)
    assert gp.fwd.n_long > 0, "the arxiv-sized plan is meant to have hub rows"
    g = torch.Generator(device=dev).manual_seed(5)
    for K in (16, 64, 256):
        x = torch.randn(n, K, generator=g, device=dev)
        go = torch.randn(n, K, generator=g, device=dev)
        for dt in sc.DTYPES:
            for reduce in ("sum", "mean"):
                for name, route in routes.items():
                    sc.check_contract_case(route, ei, w, x.to(dt), go.to(dt), reduce, f"arxiv/{name}")


def test_products_size_against_the_f32_op(eng, routes, dev):
    """K = 256 on the products-sized graph, forward and transposed: column blocks, hub rows through the exact walk (heavy
    stages) — EVERY row of the 16-bit result is F(x.float()).to(dtype); twice in a row: the same bits."""
    if torch.cuda.get_device_properties(dev).total_memory < 100 * 2**30:
        pytest.skip("needs > 100 GB of HBM")
    n, ei, w = _graph("products", dev)
    K = 256
    gp = eng.graph_plan(ei, n)
    assert gp.fwd.n_long > 0 and gp.bwd.n_long > 0, "hub rows both ways"
    assert gp.E < 2**31 and max(gp.fwd.max_len, gp.bwd.max_len) <= int(eng.lib.ggl_get_option(b"exact_long_max"))
    assert int(eng.lib.ggl_spmm_col_blocks_x16(ctypes.byref(gp.fwd.c_struct(None)), K)) == \
        K // int(eng.lib.ggl_get_option(b"col_block16"))
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(n, K, generator=g, device=dev)
    go = torch.randn(n, K, generator=g, device=dev)
    route = routes["torch.ops.ggl"]
    wy, wg = _fwd_bwd(route, ei, w, x.bfloat16().float(), go.bfloat16().float())
    for dt in sc.DTYPES:
        x16, g16 = x.to(dt), go.to(dt)
        if dt != torch.bfloat16:
            wy, wg = _fwd_bwd(route, ei, w, x16.float(), g16.float())
        y1, g1 = _fwd_bwd(route, ei, w, x16, g16)
        assert sc.same_bits(y1, wy.to(dt)) and sc.same_bits(g1, wg.to(dt)), dt
        y2, g2 = _fwd_bwd(route, ei, w, x16, g16)
        assert sc.same_bits(y1, y2) and sc.same_bits(g1, g2), ("run to run", dt)
        ye, ge = _fwd_bwd(routes["engine"], ei, w, x16, g16)
        assert sc.same_bits(y1, ye) and sc.same_bits(g1, ge), ("engine route", dt)
        with torch.no_grad():
            assert sc.same_bits(route("sum", ei, w, x16, True), wy), ("f32 output", dt)


def test_forward_and_backward_capture_into_one_hipgraph(eng, routes, dev):
    """forward + backward of the 16-bit aggregate (hub launch forked to the side stream and joined inside the library)
    recorded into one hipGraph, replayed: the eager bits"""
    n, ei, w = _graph("arxiv", dev)
    K = 64
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn(n, K, generator=g, device=dev).bfloat16()
    go = torch.randn(n, K, generator=g, device=dev).bfloat16()
    route = routes["torch.ops.ggl"]
    ey, eg = _fwd_bwd(route, ei, w, x, go)
    ey, eg = _fwd_bwd(route, ei, w, x, go)          # (second sight of w: the sorted copy exists before the capture)
    xs = x.clone().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            xs.grad = None
            route("sum", ei, w, xs).backward(go)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    xs.grad = None
    with torch.cuda.graph(graph):
        y = route("sum", ei, w, xs)
        y.backward(go)
    for _ in range(2):
        y.zero_()
        xs.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert sc.same_bits(y.detach(), ey) and sc.same_bits(xs.grad, eg)
