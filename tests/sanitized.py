"""Builds and runs one stand-alone AddressSanitizer program (tests/emul/<name>_asan_main.cpp, its own main, on
tests/emul/asan_common.hpp): compiled with -fsanitize=address, linked against the AddressSanitizer build of the host-emulated
kernel sources (tests/emul/build_asan.sh: libggl_emul_asan.so) and run directly — nothing is loaded into Python and the
environment is the caller's.  A plain helper for the tests/test_*_sanitized.py drivers."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL = os.path.join(HERE, "emul")
CXX = os.environ.get("CXX", "/opt/rocm/lib/llvm/bin/clang++")


def run_program(name, extra_flags=(), timeout=300):
    """stdout of tests/emul/<name>_asan_main.cpp; asserts exit status 0 and its closing "cases ok".  extra_flags: what the
    program's own arithmetic needs (-ffp-contract=off where its serial oracle is compared bit for bit)."""
    subprocess.check_call([os.path.join(EMUL, "build_asan.sh")], env=dict(os.environ, CXX=CXX))
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, name + "_asan")
        subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address", "-fno-omit-frame-pointer", *extra_flags,
                               "-I", os.path.join(HERE, "..", "include"), "-I", EMUL,
                               os.path.join(EMUL, name + "_asan_main.cpp"), "-L", EMUL, "-lggl_emul_asan",
                               "-Wl,-rpath," + EMUL, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases ok" in r.stdout
    return r.stdout
