"""ggl_linear_bias_act_bwd and ggl_colsum_f32 on CPU tensors: the HOST library (ctypes engine; the training step also through
torch.ops.ggl) and the emulation build of the same sources.  Cases: tests/lin_epi_bwd_cases.py."""
import os
import subprocess

import pytest
import torch

import lin_epi_bwd_cases as lc
import spmm_rows_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DEV = torch.device("cpu")


@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "gammagl_amd", "csrc"), "host", "torch"])
    import gammagl_amd

    return gammagl_amd.host_engine()


@pytest.fixture(scope="module")
def emul():
    subprocess.check_call([os.path.join(HERE, "emul", "build.sh")])
    from gammagl_amd import _lib
    from gammagl_amd.ops import Engine

    return Engine(_lib.bind(os.path.join(HERE, "emul", "libggl_emul.so")), require_cuda=False)


@pytest.fixture(scope="module", params=["host", "emul"])
def eng(request, host, emul):
    return host if request.param == "host" else emul


@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "J%d-K%d-ld%d" % s)
@pytest.mark.parametrize("N", lc.NS)
def test_fused_equals_bias_act_bwd_of_its_own_product(eng, N, shape):
    lc.check_self_consistency(eng, DEV, N, *shape)


@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "J%d-K%d-ld%d" % s)
@pytest.mark.parametrize("N", lc.NS)
def test_product_against_float64(host, N, shape):
    lc.check_against_f64(host, DEV, N, *shape)


def test_bad_arguments(eng):
    lc.check_bad_arguments(eng, DEV)


@pytest.mark.parametrize("K", lc.COLSUM_KS)
@pytest.mark.parametrize("N", lc.COLSUM_NS)
def test_colsum_is_the_documented_sum_on_the_bits(host, N, K):
    lc.check_colsum(host, DEV, N, K)


def test_training_step_fused_on_and_off(host, monkeypatch):
    from gammagl_amd import dist as D

    lc.check_model(D, host, DEV, rc, monkeypatch, ("ctypes", "cpp"))


def test_training_step_on_the_emulation_build(emul, monkeypatch):
    from gammagl_amd import dist as D

    lc.check_model(D, emul, DEV, rc, monkeypatch, ("ctypes",))
