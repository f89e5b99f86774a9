"""The fused epilogue on 16-bit rows (ggl_spmm_epi_x16, ggl_bias_act_{fwd,bwd}_x16) under AddressSanitizer, as a stand-alone
program: tests/emul/epi16_asan_main.cpp (its own main) is compiled with -fsanitize=address, linked against the AddressSanitizer
build of the host-emulated kernel sources (its entry points live in reduce.hip, epilogue.hip and, for ggl_colsum_f32,
backward.hip) and run directly.  x, add, out, y, ga, gbias and the workspace are heap blocks of exactly the documented sizes, so
a read or write past an end ends the run with a report."""
from sanitized import run_program


def test_epi16_sanitized():
    run_program("epi16", ("-ffp-contract=off",), timeout=600)
