"""The restricted plan pair (ggl_plan_rows_*) and ggl_bias_grad_rows under AddressSanitizer, as a stand-alone program:
tests/emul/spmm_rows_asan_main.cpp (its own main) is compiled with -fsanitize=address, linked against the AddressSanitizer
build of the host-emulated kernel sources and run directly.  Every buffer it hands the library is a heap block of exactly
the documented size, so a read or write past an end ends the run with a report."""
from sanitized import run_program


def test_rows_plan_and_bias_grad_rows_sanitized():
    run_program("spmm_rows")
