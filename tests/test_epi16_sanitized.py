"""The fused epilogue on 16-bit rows (ggl_spmm_epi_x16, ggl_bias_act_{fwd,bwd}_x16) under AddressSanitizer, as a stand-alone
program: tests/emul/epi16_asan_main.cpp (its own main) is compiled with -fsanitize=address together with the host-emulated
(-DGGL_EMULATE) kernel sources its entry points live in — reduce.hip, epilogue.hip, backward.hip (ggl_colsum_f32) and
plan.hip (options, error text) — and run directly.  x, add, out, y, ga, gbias and the workspace are heap blocks of exactly the
documented sizes, so a read or write past an end ends the run with a report.  (reduce.hip is the library's largest source:
line tables instead of full debug info keep its sanitized build to a couple of minutes.)"""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL = os.path.join(HERE, "emul")
CSRC = os.path.join(HERE, "..", "gammagl_amd", "csrc")
CXX = os.environ.get("CXX", "/opt/rocm/lib/llvm/bin/clang++")


def test_epi16_sanitized():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "epi16_asan")
        subprocess.check_call([CXX, "-DGGL_EMULATE", "-x", "c++", "-std=c++17", "-O1", "-gline-tables-only", "-fsanitize=address",
                               "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wno-unused-function",
                               "-I", os.path.join(HERE, "..", "include"), os.path.join(CSRC, "plan.hip"),
                               os.path.join(CSRC, "reduce.hip"), os.path.join(CSRC, "epilogue.hip"),
                               os.path.join(CSRC, "backward.hip"), os.path.join(EMUL, "epi16_asan_main.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases ok" in r.stdout
