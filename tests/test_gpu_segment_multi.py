"""-m gpu: the fused multi-statistic segment aggregate on the MI355X (ggl_segment_multi_fwd / _bwd, csrc/multiagg.hpp compiled
for gfx950): the host suite's cases on cuda tensors (tests/segment_multi_cases.py) — the serial numpy oracle the host build is
held to, so the two builds agree on the bits —, the C entry points through ctypes, the routes, unsorted_segment_min, PNAConv,
and memory."""
import pytest
import torch

import segment_multi_cases as mc

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
    return mc.make_routes(eng)


@pytest.mark.parametrize("K,C", mc.SHAPES)
def test_forward_and_backward_have_the_serial_oracle_bits_gpu(eng, dev, K, C):
    for aggs in mc.AGG_SETS:
        mc.check_oracle(eng, dev, K, C, aggs)


def test_host_build_equals_hip_build_gpu(eng, dev):
    """the same call on the host library and on the GPU: same bits, forward and backward, hub row chunked"""
    import gammagl_amd

    host = gammagl_amd.host_engine()
    cpu = torch.device("cpu")
    for (K, C), aggs in (((48, 16), mc.PNA_SET), ((75, 75), mc.AGG_SETS[1])):
        res = []
        for e, d in ((host, cpu), (eng, dev)):
            with mc.forced_chunk(e, 8):
                out, amin, amax, gx = mc.run_engine(e, mc.make_x(K, d, "ties"), mc.make_ids(d), aggs, C, True,
                                                    mc.make_g(K, len(aggs), d))
            res.append([t.cpu() for t in (out, amin, amax, gx)])
        assert all(mc.same_bits(a, b) for a, b in zip(*res))


@pytest.mark.parametrize("K,C", mc.SHAPES)
def test_bit_equality_with_the_composition_gpu(eng, dev, K, C):
    for aggs in mc.AGG_SETS:
        mc.check_composition(eng, dev, K, C, aggs)


@pytest.mark.parametrize("K,C", ((8, 8), (48, 16), (75, 75)))
def test_against_float64_gpu(eng, dev, K, C):
    for aggs in mc.AGG_SETS:
        mc.check_against_f64(eng, dev, K, C, aggs)


def test_ties_and_special_values_gpu(eng, dev):
    mc.check_special_values(eng, dev)


def test_routes_refusals_and_saved_tensors_gpu(routes, eng, dev):
    mc.check_routes_agree(routes, eng, dev)
    mc.check_refusals(routes, eng, dev)
    mc.check_saved_tensors(eng, dev)


def test_c_abi_with_exact_size_buffers_gpu(eng, dev):
    mc.check_c_abi(eng, dev)


def test_unsorted_segment_min_and_pools_gpu(eng, dev):
    mc.check_segment_min(dev)
    mc.check_pools(dev)


def test_pnaconv_gpu(eng, dev):
    mc.check_pnaconv(eng, dev)


def test_memory_gpu(eng, dev):
    """E = 400 000, K = 64, the PNA set: a forward + backward grows peak memory by less than 2.5 [E, K] arrays (gx, the saved x
    reference and slack).  Measured on the MI355X: fused 1.47 arrays, the composition 4.26 (the squares, -x, and the per-op
    gradients torch holds at once; the estimate of "at least 5" counted buffers that autograd frees before the peak)"""
    g = torch.Generator(device="cpu").manual_seed(4)
    n, e, K = 20_000, 400_000, 64
    ids = torch.randint(0, n, (e,), generator=g).to(dev)
    x = torch.randn(e, K, generator=g).to(dev).requires_grad_(True)
    go = torch.randn(n, 4 * K, generator=g).to(dev)
    eng.segment_multi(x, ids, n, mc.PNA_SET).backward(go)      # the plan and its row order built
    x.grad = None

    def grown(fused):
        old = eng.segment_multi_fused
        eng.segment_multi_fused = fused
        try:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            eng.segment_multi(x, ids, n, mc.PNA_SET).backward(go)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated(dev) - base
            x.grad = None
            return peak / (e * K * 4)
        finally:
            eng.segment_multi_fused = old

    fused, composed = grown(True), grown(False)
    print(f"forward + backward peak growth in [E, K] arrays: fused {fused:.2f}, composed {composed:.2f}")
    assert eng.stats["segment_multi"]["route"] == "composed"
    assert fused < 2.5, fused
    assert composed > fused, (fused, composed)
