"""The drop-in boundary without a GPU: libggl_mpops_hip.so loads, exports every function
include/ggl_mpops.h declares, reports the header's ABI version, and the ctypes prototypes in
gammagl_amd/_lib.py have the declared number of parameters (no compute calls here, but for one entry point that only
forwards: its direct call is the caller that keeps it honest)."""
import ctypes
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HEADER = os.path.join(REPO, "include", "ggl_mpops.h")
LIB = os.path.join(REPO, "gammagl_amd", "lib", "libggl_mpops_hip.so")


def declared_functions():
    """name -> number of parameters, for every prototype in the header."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    protos = {}
    for m in re.finditer(r"\b(?:int|size_t|int64_t|const\s+char\s*\*)\s*(ggl_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        name, args = m.group(1), m.group(2).strip()
        protos[name] = 0 if args in ("", "void") else args.count(",") + 1
    return protos


def header_abi_version():
    return int(re.search(r"#define\s+GGL_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))


def test_header_declares_the_path():
    fns = declared_functions()
    for must in ("ggl_plan_build", "ggl_segment_sum", "ggl_segment_mean", "ggl_segment_max", "ggl_spmm_sum",
                 "ggl_spmm_mean", "ggl_spmm_max", "ggl_bspmm_sum", "ggl_gat_fused_fwd", "ggl_gat_fused_bwd_dst",
                 "ggl_gat_fused_bwd_src", "ggl_spmm_sum_bias_act", "ggl_abi_version", "ggl_last_error"):
        assert must in fns, must
    assert len(fns) >= 40


def test_hip_library_exports_every_declared_symbol():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(REPO, "gammagl_amd", "csrc"), "-s"])
    lib = ctypes.CDLL(LIB)
    missing = [n for n in declared_functions() if not hasattr(lib, n)]
    assert not missing, missing
    lib.ggl_abi_version.restype = ctypes.c_int
    assert lib.ggl_abi_version() == header_abi_version()


def test_ctypes_prototypes_match_the_header():
    from gammagl_amd import _lib

    fns = declared_functions()
    assert _lib.ABI_VERSION == header_abi_version()
    unbound = sorted(set(fns) - set(_lib.SIGNATURES))
    undeclared = sorted(set(_lib.SIGNATURES) - set(fns))
    assert not unbound and not undeclared, (unbound, undeclared)
    wrong = {n: (len(_lib.SIGNATURES[n][1]), fns[n]) for n in fns if len(_lib.SIGNATURES[n][1]) != fns[n]}
    assert not wrong, f"(ctypes, header) parameter counts differ: {wrong}"


def test_host_emulation_build_has_the_same_surface():
    subprocess.check_call([os.path.join(HERE, "emul", "build.sh")])
    lib = ctypes.CDLL(os.path.join(HERE, "emul", "libggl_emul.so"))
    missing = [n for n in declared_functions() if not hasattr(lib, n)]
    assert not missing, missing


def test_host_library_is_a_product_artefact_with_the_same_surface():
    """libggl_mpops_host.so (the CPU dispatch key's library: `make -C gammagl_amd/csrc host`) exports every declared
    symbol at the header's ABI version, and binds through the same ctypes table as the HIP library."""
    from gammagl_amd import _lib

    if not os.path.exists(_lib.HOST_LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(REPO, "gammagl_amd", "csrc"), "-s", "host"])
    lib = _lib.bind(_lib.HOST_LIB_PATH)
    assert lib.ggl_abi_version() == header_abi_version()
    assert not [n for n in declared_functions() if not hasattr(lib, n)]
    # the capability queries of the GPU-only kernels answer "no" there (gpu_only_stubs.cpp)
    assert lib.ggl_gat_fast_supported(8, 8) == 0 and lib.ggl_gat_sh_supported(8, 64, 41) == 0


def test_spmm_sum_bias_act_forwards_to_spmm_epi_ex():
    """ggl_spmm_sum_bias_act stays in the header for its callers, but the engine launches ggl_spmm_epi_ex and the old entry
    point forwards to it: called directly on the host library (N = 40, E = 600 with a hub row walked in one piece and in
    chunks, K = 8, bias + ReLU, no dropout) it writes the bits of the general entry point, and those of the two-kernel form."""
    import torch

    from gammagl_amd import _lib
    from gammagl_amd.ops import Engine, _ptr

    eng = Engine(_lib.bind(_lib.HOST_LIB_PATH), require_cuda=False)
    g = torch.Generator().manual_seed(7)
    N, E, K = 40, 600, 8
    ei = torch.randint(0, N, (2, E), generator=g)
    ei[1, : E // 3] = 3
    w, x, bias = torch.rand(E, generator=g), torch.randn(N, K, generator=g), torch.randn(K, generator=g)
    for chunk in (0, 8):
        eng.chunk = chunk
        eng.graph_cache.clear()
        gp = eng.graph_plan(ei, N)
        part = eng._partial(gp.fwd, torch.float32, K, False, x.device)
        ww, w_by_pos, wp = eng._weights(gp.fwd, w)
        cs = gp.fwd.c_struct(part, wp)
        st = eng._stream(x.device)
        ya, yb = torch.full((N, K), float("nan")), torch.full((N, K), float("nan"))
        assert eng.lib.ggl_spmm_sum_bias_act(ctypes.byref(cs), _ptr(gp.col), _ptr(ww), w_by_pos, _ptr(x), K, _ptr(bias), 1,
                                             0.0, None, _ptr(ya), st) == 0, eng.lib.ggl_last_error()
        assert eng.lib.ggl_spmm_epi_ex(ctypes.byref(cs), _ptr(gp.col), _ptr(ww), w_by_pos, _ptr(x), K, K, _ptr(yb), K, 0, 0,
                                       None, 0, _ptr(bias), 1, 0.0, None, 0, 0, 1, st) == 0, eng.lib.ggl_last_error()
        assert torch.equal(ya, yb), chunk
        assert torch.equal(ya, torch.relu(eng.spmm(gp, w, x) + bias)), chunk


def test_missing_library_is_an_import_error(monkeypatch, tmp_path):
    from gammagl_amd import _lib

    with pytest.raises((ImportError, OSError)):
        _lib.bind(str(tmp_path / "libggl_mpops_hip.so"))


def test_maxbwd_form_policy_gates_the_winner_mask_on_its_footprint():
    """ggl_policy_maxbwd_form (round 6, advisor): the 1-bit winner mask is an E x K/8-byte transient — chosen for
    128 <= K <= 256 (measured faster on the products- and the Reddit-sized graph, <= 32 B per edge), not at K = 602 (slower on
    both, 96 B per edge = 11.9 GiB on the Reddit-sized graph), never for narrow K; kmax 0 removes the bound (tests)."""
    from gammagl_amd import _lib

    lib = _lib.bind(_lib.HOST_LIB_PATH)
    form = lib.ggl_policy_maxbwd_form
    assert form(126_167_309, 2_449_029, 256) == 2 and form(114_848_857, 232_965, 256) == 2
    assert form(126_167_309, 2_449_029, 128) == 2
    assert form(126_167_309, 2_449_029, 64) == 1
    assert form(114_848_857, 232_965, 602) == 1 and form(126_167_309, 2_449_029, 602) == 1
    old = lib.ggl_get_option(b"maxbwd_mask_kmax")
    try:
        lib.ggl_set_option(b"maxbwd_mask_kmax", 0)
        assert form(400, 64, 602) == 2
    finally:
        lib.ggl_set_option(b"maxbwd_mask_kmax", old)



# the options of the forms removed in ABI 11 (DESIGN.md "Forms removed in ABI 11")
REMOVED_OPTIONS = ("gat_sh_pk", "gat_sh_pipe", "gat_sh_glds", "gat_sh_prefetch", "gat_sh_zlds", "gat_sh_waves",
                   "hop_fused_scans", "hop_small_scans", "hub_priority", "hub_pipe", "maxbwd_mask_scatter",
                   "maxbwd_mask_wlane", "maxbwd_mask_cols")


def option_names(lib):
    names = []
    while True:
        n = lib.ggl_option_name(len(names))
        if n is None:
            return names
        names.append(n.decode())
        assert len(names) < 1000, "ggl_option_name never answers NULL"


def test_option_table_enumerates_unique_names():
    from gammagl_amd import _lib

    lib = _lib.bind(_lib.HOST_LIB_PATH)
    names = option_names(lib)
    assert names and all(names) and len(set(names)) == len(names), names
    assert lib.ggl_option_name(-1) is None and lib.ggl_option_name(len(names) + 5) is None
    for kept in ("exact_long_rows", "hub_one_launch", "col_block", "col_block16", "ragged4", "ragged_max", "row_order",
                 "xcd_swizzle", "unroll", "force_generic", "max_grid_x", "maxbwd_arg32", "maxbwd_mask", "maxbwd_mask_kmax",
                 "softmax_sublanes"):
        assert kept in names, kept
    assert not set(REMOVED_OPTIONS) & set(names)


def test_every_option_round_trips_through_set_and_get():
    from gammagl_amd import _lib

    lib = _lib.bind(_lib.HOST_LIB_PATH)
    for name in option_names(lib):
        key = name.encode()
        old = lib.ggl_get_option(key)
        try:
            assert lib.ggl_set_option(key, old) == 0 and lib.ggl_get_option(key) == old, name
            assert lib.ggl_set_option(key, old + 1) == 0 and lib.ggl_get_option(key) == old + 1, name
        finally:
            assert lib.ggl_set_option(key, old) == 0
        assert lib.ggl_get_option(key) == old, name
    # the one special case: max_grid_x is clamped to >= 1 when set
    old = lib.ggl_get_option(b"max_grid_x")
    try:
        assert lib.ggl_set_option(b"max_grid_x", 0) == 0 and lib.ggl_get_option(b"max_grid_x") == 1
        assert lib.ggl_set_option(b"max_grid_x", -7) == 0 and lib.ggl_get_option(b"max_grid_x") == 1
    finally:
        lib.ggl_set_option(b"max_grid_x", old)


@pytest.mark.parametrize("name", REMOVED_OPTIONS + ("no_such_option",))
def test_removed_and_unknown_options_are_refused(name):
    from gammagl_amd import _lib

    lib = _lib.bind(_lib.HOST_LIB_PATH)
    assert lib.ggl_set_option(name.encode(), 1) != 0
    assert lib.ggl_last_error().decode() == f"unknown option {name}"
    assert lib.ggl_get_option(name.encode()) == -1


def test_every_option_reads_its_environment_variable():
    """GGL_ + the upper-cased name, read once at first use: checked in a fresh process (ragged_max and softmax_sublanes had
    no variable before the option table)."""
    import sys

    code = ("from gammagl_amd import _lib; lib = _lib.bind(_lib.HOST_LIB_PATH); "
            "print(*[lib.ggl_get_option(n) for n in (b'ragged_max', b'softmax_sublanes', b'col_block16', b'row_order')])")
    env = dict(os.environ, GGL_RAGGED_MAX="0", GGL_SOFTMAX_SUBLANES="4", GGL_COL_BLOCK16="64")   # (`-c` in cwd = REPO: the package imports from the tree)
    env.pop("GGL_ROW_ORDER", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=REPO, capture_output=True, text=True, check=True).stdout
    assert out.split() == ["0", "4", "64", "1"], out     # (row_order: not set, its default)
