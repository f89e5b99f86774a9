"""-m gpu: gspmm's gradient with respect to its edge weights (ggl_spmm_grad_w: sum and mean, f32 / bf16 / f16 rows) on the
MI355X, through the ctypes engine, ``torch.ops.ggl`` and ``torch.ops.gammagl_amd``: the host suite's cases on cuda tensors
(tests/spmm_gradw_cases.py) — here the LDS-staged kernels, their tails and the carried chain of the column-block launches
run — then the fused route's memory against the message tensor it replaces, and the HIP library against the host build on
the bits."""
import pytest
import torch

import spmm_gradw_cases as gc

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
    return gc.make_routes(eng)


@pytest.fixture(scope="module")
def namespaces(eng):
    from gammagl_amd import cpp_ops, torch_ops

    return (cpp_ops.load(), torch_ops.ops)


def test_weight_gradient_exists_gpu(routes, dev):
    """Fails on the parent commit: w.grad stayed None."""
    gc.check_exists(routes, dev)


def test_f32_sum_is_bspmm_one_head_and_mean_is_sum_of_prescaled_gpu(routes, eng, dev):
    n = gc.check_f32(routes, eng, dev)
    assert n == (len(gc.KINDS) + len(gc.EDGES)) * len(gc.WIDTHS) * 3 * 2


def test_rectangular_graph_gpu(eng, dev):
    gc.check_rectangular(eng, dev)


def test_16_bit_storage_is_the_f32_form_on_widened_rows_gpu(routes, eng, dev):
    assert gc.check_x16(routes, eng, dev) > 0


def test_sums_are_made_in_f32_gpu(routes, dev):
    gc.check_f32_accumulation(routes, dev)


def test_column_blocks_carry_the_chain_gpu(routes, eng, dev):
    """thresholds lowered through the option table: K = 128 / 256 / 264 run as two to five launches that hand the running dot
    on in the scratch (64-column blocks for f32 x, 128-column ones for 16-bit x, the last with a tail): the serial bits"""
    with gc.low_block_thresholds(eng):
        assert eng.lib.ggl_spmm_grad_w_scratch_bytes(gc.E, gc.N, 264, 7, 0) >= 4 * gc.E      # f32 x: a carried chain
        assert eng.lib.ggl_spmm_grad_w_scratch_bytes(gc.E, gc.N, 264, 6, 0) >= 4 * gc.E      # bf16 x
    assert eng.lib.ggl_spmm_grad_w_scratch_bytes(gc.E, gc.N, 264, 7, 0) == 0
    assert gc.check_carried_chain(routes, eng, dev) > 0


def test_block_width_that_is_not_a_multiple_of_8_gpu(eng, dev):
    """Fails without the one-launch rule in gradw16_launch: f32 x / 16-bit g under col_block = 36 dropped columns."""
    gc.check_block_width_not_a_multiple_of_8(eng, dev)


def test_constant_weight_costs_nothing_gpu(routes, dev):
    gc.check_constant_weight_costs_nothing(routes, dev)


def test_epilogue_weight_gradient_against_float64_gpu(eng, namespaces, dev):
    gc.check_epilogue(eng, namespaces, dev)
    gc.check_epilogue(eng, namespaces, dev, p_drop=0.3)


def test_layers_take_the_fused_route_gpu(eng, dev):
    gc.check_gcnconv_learnable_edge_weight(dev)
    gc.check_propagate_takes_the_spmm(dev)


def test_max_and_rows_keep_their_behaviour_gpu(routes, eng, namespaces, dev):
    gc.check_max_and_rows_unchanged(routes, eng, namespaces, dev)


def test_no_edge_by_width_tensor_is_allocated(eng, dev):
    """N = 2 000, E = 200 000, K = 64: the message tensor would be E K 4 = 51 MB, and the message route allocates it and its
    gradient.  One learnable-weight GCNConv forward + backward on the fused route grows the peak by a few [N, K] panels and
    [E] vectors (about 3 MB): less than a QUARTER of one message tensor."""
    from gammagl_amd import layers

    n, e, K = 2000, 200_000, 64
    gen = torch.Generator(device=dev).manual_seed(0)
    ei = torch.randint(0, n, (2, e), generator=gen, device=dev)
    x = torch.randn(n, K, generator=gen, device=dev)
    torch.manual_seed(0)
    conv = layers.GCNConv(K, K, norm="none").to(dev)
    ew = torch.rand(e, generator=gen, device=dev).requires_grad_(True)

    def step():
        conv.zero_grad()
        ew.grad = None
        conv(x, ei, ew, n).sum().backward()

    step()                                    # builds the plan (both sides) and the row index
    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    step()
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated(dev) - base
    print(f"peak growth {growth / 1e6:.2f} MB, bound {e * K * 4 / 4 / 1e6:.2f} MB")
    assert ew.grad is not None and growth < e * K * 4 // 4, growth


def test_host_library_and_hip_library_agree_on_the_bits(eng, dev):
    """the cases of the f32, mean and 16-bit checks through Engine.spmm_grad_w on both builds of the kernel sources"""
    import gammagl_amd

    host = gammagl_amd.host_engine()
    cpu = torch.device("cpu")
    with gc.low_block_thresholds(eng):
        for gi, (name, index, nn) in enumerate(gc.graphs(cpu)):
            index_d = index.to(dev)              # one tensor per graph: one cached plan
            for K in gc.WIDTHS if name in ("uniform", "power", "E=257") else (7, 8, 264):
                _, x, g = gc.inputs(index, nn, nn, K, cpu, 300 * gi + K)
                for xd in (torch.float32,) + gc.DTYPES:
                    for gd in (torch.float32,) + gc.DTYPES:
                        for mean in (False, True):
                            xx, gg = x.to(xd), g.to(gd)
                            want = host.spmm_grad_w(index, xx, gg, mean)
                            got = eng.spmm_grad_w(index_d, xx.to(dev), gg.to(dev), mean)
                            assert gc.same_bits(got.cpu(), want), (name, K, xd, gd, mean)
