"""GATv2's backward walk (ggl_gatv2_logit_bwd) under AddressSanitizer, as a stand-alone program:
tests/emul/gatv2_asan_main.cpp (its own main) is compiled with -fsanitize=address, linked against the AddressSanitizer build
of the host-emulated kernel sources and run directly.  Every buffer it hands the library is a heap block of exactly the
documented size (gz exactly E * H floats, plan->partial exactly ggl_gatv2_logit_bwd_partial_bytes), on a plan pair with a
perm and long rows both ways and on one with sorted ids and no perm, so a read or write past an end ends the run with a
report; every output is compared on the bits with a serial loop in the program."""
from sanitized import run_program


def test_gatv2_logit_backward_sanitized():
    run_program("gatv2", ("-ffp-contract=off",))
