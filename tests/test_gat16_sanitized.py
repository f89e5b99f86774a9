"""The fused GAT on 16-bit rows (ggl_gat_fused_{fwd,bwd_dst,bwd_src}_x16) under AddressSanitizer, as a stand-alone program:
tests/emul/gat16_asan_main.cpp (its own main) is compiled with -fsanitize=address, linked against the AddressSanitizer build
of the host-emulated kernel sources and run directly.  Every buffer it hands the library is a heap block of exactly the
documented size — the 16-bit panels once aligned on a plan with long rows, once starting one element into their blocks — so
a read or write past an end ends the run with a report."""
from sanitized import run_program


def test_gat16_entry_points_sanitized():
    run_program("gat16")
