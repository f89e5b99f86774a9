"""-m gpu: scaled dot-product graph attention on the MI355X — the fused forward (ggl_dot_attn_fwd, csrc/dotattn.hip: the dot
formed inside the aggregate's walk by a butterfly over the head's lane group) for C = 8, 16, 32, 64, the composed route for the
other widths, and the backward both share.  The host suite's cases on cuda tensors (tests/dot_attention_cases.py), the C entry
point through ctypes, the routes the capability query announces, run-to-run bits, and memory of a forward without grad."""
import pytest
import torch

import dot_attention_cases as dc
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
    return dc.make_routes(eng)


def test_capability_query(eng):
    for H, C in dc.SHAPES:
        assert eng.lib.ggl_dot_attn_supported(H, C) == (1 if C in (8, 16, 32, 64) else 0), (H, C)
        assert eng.lib.ggl_policy_dot_attn_fused(H, C, dc.E, dc.N_SRC) <= eng.lib.ggl_dot_attn_supported(H, C)
    assert eng.lib.ggl_dot_attn_supported(0, 8) == 0 and eng.lib.ggl_dot_attn_supported(1, 4) == 0


@pytest.mark.parametrize("p", dc.DROPS)
@pytest.mark.parametrize("H,C", dc.SHAPES)
def test_everything_behind_the_logits_is_the_existing_op_gpu(eng, dev, H, C, p):
    """the host suite's contract on the route the query announces (check_contract asserts the route), hub row chunked and
    whole, two identical calls identical, no [E, H] array formed by a fused forward without grad"""
    taken = dc.check_contract(eng, dev, H, C, p)
    assert taken == [dc.expects_fused(eng, dev, H, C)] * 2


def test_c_entry_point_gpu(eng, dev):
    """ggl_dot_attn_fwd through ctypes: z in the gamma bound, out / rowmax / rowden the bits of ggl_edge_softmax_agg_fwd on
    that z, z_out = NULL gives the same out; 7 supported shapes x 2 dropout rates x 2 chunkings"""
    assert dc.check_c_abi(eng, dev) == 7 * 2 * 2


def test_composed_route_on_supported_shapes_gpu(eng, dev):
    """the A/B switch: with the fused forward off the supported shapes take the composed route and keep the contract"""
    old = eng.dot_attn_fused
    eng.dot_attn_fused = False
    try:
        for H, C in ((8, 8), (1, 64)):
            assert dc.check_contract(eng, dev, H, C, 0.5) == [False, False]
    finally:
        eng.dot_attn_fused = old


def test_one_sided_gradients_gpu(eng, dev):
    dc.check_one_sided_gradients(eng, dev)


def test_single_needs_have_the_aggregates_backward_bits_gpu(routes, eng, dev):
    """on the fused route (2 x 16) and on the composed one (2 x 12)"""
    dc.check_single_needs_against_the_aggregate(routes, eng, dev)
    dc.check_single_needs_against_the_aggregate(routes, eng, dev, 2, 12)


def test_routes_agree_gpu(routes, eng, dev):
    dc.check_routes_agree(routes, eng, dev)


def test_refusals_and_public_function_gpu(routes, eng, dev):
    dc.check_refusals(routes, eng, dev)
    dc.check_public_function(eng, dev)


def test_against_float64_gpu(eng, dev):
    """the fused route within 4x of the composed route's distance from float64, every shape, dropout rate and chunking"""
    dc.check_against_f64(eng, dev)


def test_a_forward_without_grad_allocates_no_logits_gpu(eng, dev):
    """E = 400 000 edges, 8 x 8: z would be 12.8 MB; the forward's peak above its inputs stays below a tenth of that"""
    g = torch.Generator(device="cpu").manual_seed(4)
    n, e, H, C = 2000, 400_000, 8, 8
    index = torch.randint(0, n, (2, e), generator=g).to(dev)
    q, k, v = (torch.randn(n, H, C, generator=g).to(dev) for _ in range(3))
    assert dc.expects_fused(eng, dev, H, C)
    gp = eng.graph_plan(index, n, n)
    eng.dot_attention(gp, q, k, v, n)             # plans and row order built
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = eng.dot_attention(gp, q, k, v, n)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated(dev) - base
    assert eng.stats["dot_attention"] == {"fused": True, "logits_bytes": 0, "logits_saved": False}
    assert grown < e * H * 4 // 10, grown
    qa = q.clone().requires_grad_(True)
    o2 = eng.dot_attention(gp, qa, k, v, n)
    assert eng.stats["dot_attention"]["logits_bytes"] == e * H * 4 and same_bits(o2.detach(), out)


def test_hgtconv_gpu():
    dc.check_hgt(torch.device("cuda", 0))
