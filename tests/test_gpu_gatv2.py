"""-m gpu: GATv2's additive graph attention on the MI355X — the fused forward (ggl_gatv2_fwd, csrc/gatv2.hip: the logit formed
inside the aggregate's walk from the value row, a butterfly over the head's lane group) for C = 8, 16, 32, 64, the composed
route for the other widths, and the backward both share (ggl_gatv2_logit_bwd, csrc/gatv2_bwd.hpp).  The host suite's cases on
cuda tensors (tests/gatv2_cases.py), the C entry point through ctypes, the routes the capability query announces, the backward
kernel against the numpy oracle the host build is held to, and memory."""
import pytest
import torch

import gatv2_cases as vc
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
    return vc.make_routes(eng)


def test_capability_query(eng):
    for H, C in vc.SHAPES:
        assert eng.lib.ggl_gatv2_supported(H, C) == (1 if C in (8, 16, 32, 64) else 0), (H, C)
        assert eng.lib.ggl_policy_gatv2_fused(H, C, vc.E, vc.N_SRC) <= eng.lib.ggl_gatv2_supported(H, C)
    assert eng.lib.ggl_gatv2_supported(0, 8) == 0 and eng.lib.ggl_gatv2_supported(1, 4) == 0


@pytest.mark.parametrize("p", vc.DROPS)
@pytest.mark.parametrize("H,C", vc.SHAPES)
def test_everything_behind_the_logits_is_the_existing_op_gpu(eng, dev, H, C, p):
    """the host suite's contract on the route the query announces (check_contract asserts the route), hub row chunked and
    whole, two identical calls identical, no [E, H] array formed by a fused forward without grad"""
    taken = vc.check_contract(eng, dev, H, C, p)
    assert taken == [vc.expects_fused(eng, dev, H, C)] * 2


def test_c_entry_point_gpu(eng, dev):
    """ggl_gatv2_fwd through ctypes: every z written and in the gamma bound, out / rowmax / rowden the bits of
    ggl_edge_softmax_agg_fwd on that z, z_out = NULL gives the same out; 7 supported shapes x 2 dropout rates x 2 chunkings;
    the other widths refused"""
    assert vc.check_c_abi(eng, dev) == 7 * 2 * 2


def test_composed_route_on_supported_shapes_gpu(eng, dev):
    """the A/B switch: with the fused forward off the supported shapes take the composed route and keep the contract"""
    old = eng.gatv2_fused
    eng.gatv2_fused = False
    try:
        for H, C in ((8, 8), (1, 64)):
            assert vc.check_contract(eng, dev, H, C, 0.5) == [False, False]
    finally:
        eng.gatv2_fused = old


@pytest.mark.parametrize("H,C", vc.SHAPES)
def test_logit_backward_kernel_has_the_serial_oracle_bits_gpu(eng, dev, H, C):
    """the HIP build of ggl_gatv2_logit_bwd against the oracle the host build is held to: the two builds agree on the bits"""
    vc.check_logit_bwd_oracle(eng, dev, H, C)


def test_one_sided_gradients_gpu(eng, dev):
    vc.check_one_sided_gradients(eng, dev)


def test_single_needs_have_the_aggregates_backward_bits_gpu(routes, eng, dev):
    """on the fused route (2 x 16) and on the composed one (2 x 12)"""
    vc.check_single_needs_against_the_aggregate(routes, eng, dev)
    vc.check_single_needs_against_the_aggregate(routes, eng, dev, 2, 12)


def test_routes_agree_gpu(routes, eng, dev):
    vc.check_routes_agree(routes, eng, dev)


def test_refusals_and_public_function_gpu(routes, eng, dev):
    vc.check_refusals(routes, eng, dev)
    vc.check_public_function(eng, dev)


def test_against_float64_gpu(eng, dev):
    vc.check_against_f64(eng, dev)


def test_memory_gpu(eng, dev):
    """N = 2000, E = 400 000, 8 x 8: one [E, H] array is 12.8 MB, one [E, H, C] array 102.4 MB.  A fused forward without grad
    grows peak memory by less than a tenth of an [E, H] array; a forward + backward by less than half of an [E, H, C] array
    (51.2 MB; the three [E, H] arrays z, alpha and gz are 38.4 MB)"""
    g = torch.Generator(device="cpu").manual_seed(4)
    n, e, H, C = 2000, 400_000, 8, 8
    index = torch.randint(0, n, (2, e), generator=g).to(dev)
    xl, xr = (torch.randn(n, H, C, generator=g).to(dev) for _ in range(2))
    att = (torch.randn(H, C, generator=g) / C ** 0.5).to(dev)
    go = torch.randn(n, H, C, generator=g).to(dev)
    assert vc.expects_fused(eng, dev, H, C)
    gp = eng.graph_plan(index, n, n)
    leaves = [t.clone().requires_grad_(True) for t in (xl, xr, att)]
    eng.gatv2_attention(gp, *leaves, n).backward(go)       # plans of both directions and row orders built
    eng.gatv2_attention(gp, xl, xr, att, n)
    for t in leaves:
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = eng.gatv2_attention(gp, xl, xr, att, n)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated(dev) - base
    assert eng.stats["gatv2_attention"] == {"fused": True, "logits_bytes": 0, "logits_saved": False}
    assert grown < e * H * 4 // 10, grown
    del out
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    o2 = eng.gatv2_attention(gp, *leaves, n)
    assert eng.stats["gatv2_attention"]["logits_bytes"] == e * H * 4
    o2.backward(go)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated(dev) - base
    print("forward + backward peak growth:", grown, "bytes")
    assert grown < e * H * C * 4 // 2, grown
    assert all(t.grad is not None for t in leaves)


def test_gatv2conv_gpu():
    vc.check_conv_paper(torch.device("cuda", 0))
    vc.check_conv_reference(torch.device("cuda", 0))
