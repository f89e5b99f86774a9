"""The argument-error contract of the C ABI on the host build: every malformed call of tests/c_abi_errors.py answers with
the return code and the ggl_last_error() text recorded in tests/golden/c_abi_errors.txt (written from the library of
740084d, before the entry points' preambles were merged into shared helpers)."""
import os
import subprocess

import pytest

import c_abi_errors

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def got():
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "gammagl_amd", "csrc"), "host"])
    from gammagl_amd import _lib

    return c_abi_errors.table(_lib.host_lib())


def test_every_malformed_call_keeps_its_code_and_text(got):
    want = open(os.path.join(HERE, "golden", "c_abi_errors.txt")).read().splitlines()
    assert len(want) > 200 and [g.split(" -> ")[0] for g in got] == [w.split(" -> ")[0] for w in want]
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, wrong


def test_the_table_covers_the_codes_and_the_empty_plan(got):
    """EINVAL, EDTYPE and EWORKSPACE all occur, and an empty plan with NULL buffers is GGL_OK wherever nothing else is asked"""
    codes = {int(g.split(" -> ")[1].split()[0]) for g in got}
    assert {0, -1, -3, -5} <= codes
    empty = [g for g in got if " empty_plan_null_everything " in g]
    assert len(empty) == len(c_abi_errors.ENTRIES) and sum(g.endswith("-> 0") for g in empty) >= len(empty) - 2
