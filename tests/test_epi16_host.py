"""The fused epilogue on 16-bit rows (ggl_spmm_epi_x16, ggl_bias_act_{fwd,bwd}_x16: bf16 / f16 storage, f32 arithmetic, one
rounding at the store) on the HOST library, CPU tensors, through the ctypes engine and the C++-registered ``torch.ops.ggl``.
Every comparison is on the bits.  Cases: tests/epi16_cases.py."""
import os
import subprocess

import pytest
import torch

import epi16_cases as ec

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DEV = torch.device("cpu")


@pytest.fixture(scope="module")
def eng():
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "gammagl_amd", "csrc"), "host", "torch"])
    import gammagl_amd

    return gammagl_amd.host_engine()


@pytest.fixture(scope="module")
def routes(eng):
    return ec.make_routes(eng)


def test_epilogue_ops_accept_16_bit_rows(eng):
    """Fails on the parent commit: spmm_epi / bias_act raised "expected scalar type Float" for bf16 / f16 tensors."""
    ec.check_accepts(eng, DEV)


def test_sageconv_and_graphsage_run_under_autocast(eng):
    """Fails on the parent commit: the aggregate-first branch raised, the other returned f32."""
    ec.check_sage_accepts(DEV)


def test_contract_bit_for_bit(routes):
    """forward (16-bit and f32 output, mask and state motion included) and the stepwise backward (ga, gbias, gx, gw): every id
    vector at K = 64, every width on the power-law ids, both dtypes, weights and None, six epilogue forms, both routes."""
    n = ec.check_contract(routes, DEV)
    assert n == (len(ec.WIDTHS) + len(ec.KINDS) - 1) * len(ec.DTYPES) * 2 * len(ec.FORMS) * 2


def test_mean_with_dropout_forms(routes):
    ec.check_mean_forms(routes, DEV)


def test_dropout_keeps_about_half(eng):
    ec.check_kept_share(eng, DEV)


def test_one_rounding_at_the_store(routes):
    """Fails on the parent commit (the ops refuse 16-bit rows; its composition gives 4096.0 both times)."""
    ec.check_one_rounding(routes, DEV)


def test_contract_on_a_plan_with_long_rows(routes):
    ec.check_long_rows(routes, DEV)


def test_column_blocks_give_the_one_launch_bits(eng):
    ec.check_column_blocks(eng, DEV)


def test_bias_act_alone(routes):
    ec.check_bias_act(routes, DEV)


def test_still_refuses_what_it_refused(routes):
    ec.check_refusals(routes, DEV)


def test_sageconv_is_its_parts(eng):
    ec.check_sage_parts(eng, DEV)


def test_gcn_model_hidden_layer_is_its_parts(eng):
    ec.check_gcn_model_parts(eng, DEV)


def test_gcn_trainer_with_dropout_under_amp(eng):
    ec.check_trainers(DEV)


def test_dispatcher_contracts(eng):
    ec.check_dispatcher(eng, DEV)


def test_c_abi_surface(eng):
    ec.check_c_abi(eng, DEV)
