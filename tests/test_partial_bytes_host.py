"""plan->partial_bytes on the HOST library, CPU tensors: every op that hands the kernel library a hub partial runs with a partial
of exactly the library's own size between canary bands (same bits as the unpatched Engine, canaries intact) and is refused with
the GGL_EWORKSPACE text when the declared size is one byte short.  Cases: tests/partial_bytes_cases.py."""
import os
import subprocess

import pytest
import torch

import partial_bytes_cases as pc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cpu")


@pytest.fixture(scope="module")
def eng():
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "gammagl_amd", "csrc"), "host", "torch"])
    import gammagl_amd

    return gammagl_amd.host_engine()


@pytest.mark.parametrize("name", sorted(pc.HOST_AND_GPU))
def test_exact_partial_same_bits_and_one_byte_short_refused(eng, name, monkeypatch):
    pc.check_case(eng, DEV, name, monkeypatch)


def test_the_new_sizers_answer_the_documented_rules(eng):
    """the exports added with ABI 12 return what include/ggl_mpops.h documented for their walks before (slack included), and
    0 for a plan without hub chunks"""
    L, f32 = eng.lib, 7
    for n, H, C in ((0, 2, 4), (3, 2, 4), (5, 8, 8), (7, 3, 5), (1, 1, 64)):
        assert L.ggl_gat_bwd_dst_partial_bytes(n, H) == L.ggl_partial_bytes(f32, n, H, 0)
        assert L.ggl_gat_bwd_src_partial_bytes(n, H, C) == L.ggl_partial_bytes(f32, n, H * C + H, 0)
        assert L.ggl_gat_fast_bwd_dst_partial_bytes(n, H) == L.ggl_partial_bytes(f32, n, 8 * H, 0)
        assert L.ggl_gat_sh_bwd_dst_partial_bytes(n) == L.ggl_gat_sh_partial_bytes(n, 8)
        assert L.ggl_gat_sh_bwd_src_partial_bytes(n, C) == L.ggl_gat_sh_partial_bytes(n, C)
        assert L.ggl_gat_partial_bytes(n, H, C) == (n * (H * C + 2 * H) * 4 + 64 if n else 0)
