"""gspmm's weight gradient (ggl_spmm_grad_w) under AddressSanitizer, as a stand-alone program:
tests/emul/spmm_gradw_asan_main.cpp (its own main) is compiled with -fsanitize=address, linked against the AddressSanitizer
build of the host-emulated kernel sources (the entry point lives in edgedot.hip) and run directly.  gw, the scratch (carried
chain + mean panel) and the 16-bit panels are heap blocks of exactly the documented sizes, so a read or write past an end ends
the run with a report."""
from sanitized import run_program


def test_spmm_grad_w_sanitized():
    run_program("spmm_gradw", ("-ffp-contract=off",))
