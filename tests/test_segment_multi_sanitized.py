"""The multi-statistic segment aggregate (ggl_segment_multi_fwd / _bwd) under AddressSanitizer, as a stand-alone program:
tests/emul/segment_multi_asan_main.cpp (its own main) is compiled with -fsanitize=address, linked against the AddressSanitizer
build of the host-emulated kernel sources and run directly; nothing is loaded into Python.  Every buffer it hands the library
is a heap block of exactly the documented size (out exactly N * A * K floats, plan->partial exactly
ggl_segment_multi_partial_bytes, the witnesses exactly N * K int32), on a plan with a perm and long rows and on one with sorted
ids and no perm, for the shapes (20, 5) and (48, 16); every output is compared on the bits with a serial loop in the program."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL = os.path.join(HERE, "emul")
CXX = os.environ.get("CXX", "/opt/rocm/lib/llvm/bin/clang++")


def test_segment_multi_sanitized():
    subprocess.check_call([os.path.join(EMUL, "build_asan.sh")], env=dict(os.environ, CXX=CXX))
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "segment_multi_asan")
        subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address", "-fno-omit-frame-pointer",
                               "-ffp-contract=off", "-I", os.path.join(HERE, "..", "include"),
                               os.path.join(EMUL, "segment_multi_asan_main.cpp"), "-L", EMUL, "-lggl_emul_asan",
                               "-Wl,-rpath," + EMUL, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases ok" in r.stdout
