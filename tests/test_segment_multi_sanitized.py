"""The multi-statistic segment aggregate (ggl_segment_multi_fwd / _bwd) under AddressSanitizer, as a stand-alone program:
tests/emul/segment_multi_asan_main.cpp (its own main) is compiled with -fsanitize=address, linked against the AddressSanitizer
build of the host-emulated kernel sources and run directly; nothing is loaded into Python.  Every buffer it hands the library
is a heap block of exactly the documented size (out exactly N * A * K floats, plan->partial exactly
ggl_segment_multi_partial_bytes, the witnesses exactly N * K int32), on a plan with a perm and long rows and on one with sorted
ids and no perm, for the shapes (20, 5) and (48, 16); every output is compared on the bits with a serial loop in the program."""
from sanitized import run_program


def test_segment_multi_sanitized():
    run_program("segment_multi", ("-ffp-contract=off",))
