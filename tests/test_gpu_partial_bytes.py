"""-m gpu: plan->partial_bytes on the MI355X — the host suite's cases on cuda tensors, plus the walks only the GPU build has
(the fast fused GAT, the head-mean GAT, the serial f32 hub walk): a partial of exactly the library's own size between canary
bands gives the unpatched Engine's bits and leaves the canaries intact; one byte short is refused with the GGL_EWORKSPACE text
and nothing is launched.  Cases: tests/partial_bytes_cases.py."""
import pytest
import torch

import partial_bytes_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; the HIP path has no fallback")
    from gammagl_amd import engine

    return engine()


@pytest.mark.parametrize("name", sorted(pc.HOST_AND_GPU) + sorted(pc.GPU_ONLY))
def test_exact_partial_same_bits_and_one_byte_short_refused_gpu(eng, name, monkeypatch):
    pc.check_case(eng, torch.device("cuda", 0), name, monkeypatch)


def test_the_new_sizers_answer_the_documented_rules_gpu(eng):
    L, f32 = eng.lib, 7
    for n, H, C in ((0, 2, 4), (3, 2, 4), (5, 8, 8), (7, 3, 5), (1, 1, 64)):
        assert L.ggl_gat_bwd_dst_partial_bytes(n, H) == L.ggl_partial_bytes(f32, n, H, 0)
        assert L.ggl_gat_bwd_src_partial_bytes(n, H, C) == L.ggl_partial_bytes(f32, n, H * C + H, 0)
        assert L.ggl_gat_fast_bwd_dst_partial_bytes(n, H) == L.ggl_partial_bytes(f32, n, 8 * H, 0)
        assert L.ggl_gat_sh_bwd_dst_partial_bytes(n) == L.ggl_gat_sh_partial_bytes(n, 8)
        assert L.ggl_gat_sh_bwd_src_partial_bytes(n, C) == L.ggl_gat_sh_partial_bytes(n, C)
