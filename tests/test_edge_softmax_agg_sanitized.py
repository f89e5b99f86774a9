"""The edge-softmax aggregate (ggl_edge_softmax_agg_{fwd,bwd_dst,bwd_src}) under AddressSanitizer, as a stand-alone program:
tests/emul/edge_softmax_agg_asan_main.cpp (its own main) is compiled with -fsanitize=address, linked against the
AddressSanitizer build of the host-emulated kernel sources and run directly.  Every buffer it hands the library is a heap
block of exactly the documented size (z, gz and alpha exactly E * H floats), on a plan with a perm and long rows both ways
and on one with sorted ids and no perm, so a read or write past an end ends the run with a report."""
from sanitized import run_program


def test_edge_softmax_agg_entry_points_sanitized():
    run_program("edge_softmax_agg")
