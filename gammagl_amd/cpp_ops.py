"""``torch.ops.ggl.*`` — the seven reference operators registered with the dispatcher FROM C++
(gammagl_amd/csrc/torch/ggl_torch.cpp -> gammagl_amd/lib/libggl_torch.so, ``TORCH_LIBRARY(ggl, m)``).

Same schemas as the Python-registered ``torch.ops.gammagl_amd.*`` (gammagl_amd/torch_ops.py) and the same kernels
behind them, but with no Python between the dispatcher and the C ABI: plan cache, launch policy and autograd
formulas are C++ (dispatcher -> libggl_torch.so -> include/ggl_mpops.h -> kernel).  That is the registration style the
reference's docs name as intended (register_cpp_ops.md:29-31); its code binds pybind11 functions instead
(src/operators.cpp:51-59).  ``gammagl_amd/compat/_torch_ext.py`` — the zero-edit drop-in for that pybind module —
binds these when the library is built.

    from gammagl_amd import cpp_ops
    ops = cpp_ops.load()                       # torch.ops.ggl
    out = ops.spmm_sum(edge_index, weight, x)  # CUDA tensors -> libggl_mpops_hip.so, CPU tensors -> libggl_mpops_host.so
"""
import os

import torch

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libggl_torch.so")
_loaded = False


def available():
    return os.path.exists(LIB_PATH)


def enabled():
    """Built, and not switched off with GGL_CPP_OPS=0 (A/B against the Python-registered ops)."""
    return available() and os.environ.get("GGL_CPP_OPS", "1") != "0"


def load():
    """Load libggl_torch.so (once) and return ``torch.ops.ggl``.  The kernel libraries themselves are opened by the
    C++ side on the first call for a device (a missing one raises there, naming the file)."""
    global _loaded
    if not _loaded:
        if not available():
            raise ImportError(f"{LIB_PATH} is not built: run `make -C gammagl_amd/csrc torch` "
                              f"(or __graft_entry__.build())")
        torch.ops.load_library(LIB_PATH)
        _loaded = True
    return torch.ops.ggl


def load_grad():
    """``torch.ops.ggl_grad`` (the same library): ``spmm_grad_w(index, x, grad, mean)``, gspmm's gradient with respect to its
    edge weights — the op the autograd formulas of spmm_sum / spmm_mean / spmm_*_x16 / spmm_epi call.  A namespace of its own:
    the surface under ``ggl::`` is the reference's operators and their passes, pinned name by name."""
    load()
    return torch.ops.ggl_grad


def load_agg():
    """``torch.ops.ggl_agg`` (the same library): ``segment_multi(x, index, N, aggs, C, empty_zero=False)``, several statistics
    (GGL_AGG_* codes: 0 sum, 1 mean, 2 min, 3 max, 4 var, 5 std) of ``x [E, K]`` per segment from one walk, with its
    ``_forward`` / ``_backward`` passes.  A namespace of its own for the reason ``load_grad`` gives."""
    load()
    return torch.ops.ggl_agg


def load_attn():
    """``torch.ops.ggl_attn`` (the same library): ``edge_softmax_aggregate(index, logits, x, num_nodes=None, dropout_rate=0.)``,
    edge softmax + weighted aggregate on per-edge logits, with its ``_forward`` / ``_backward`` passes, and
    ``dot_attention(index, q, k, v, num_nodes=None, scale=None, dropout_rate=0.)``, the same with the logits formed from
    ``scale * <q[dst], k[src]>``, with its passes, and ``gatv2_attention(index, xl, xr, att, num_nodes=None,
    negative_slope=0.2, dropout_rate=0.)``, the same with GATv2's additive logits, with its passes.  A namespace of its own for the reason ``load_grad`` gives."""
    load()
    return torch.ops.ggl_attn
