"""``torch.ops.gammagl_amd.*`` — the HIP message-passing ops registered with the PyTorch dispatcher.

The reference binds its native ops as seven pybind11 free functions (src/operators.cpp:51-59) and notes
``TORCH_LIBRARY`` as the intended style (docs register_cpp_ops.md:29-31).  Here the same seven entry
points (+ the fused GAT op and the fused epilogue) are dispatcher ops:

    torch.ops.gammagl_amd.segment_sum(x, index, N)        -> Tensor          c_segment_sum
    torch.ops.gammagl_amd.segment_mean(x, index, N)       -> Tensor          c_segment_mean
    torch.ops.gammagl_amd.segment_max(x, index, N)        -> (Tensor, Tensor) c_segment_max (+ argmax)
    torch.ops.gammagl_amd.segment_softmax(x, index, N)    -> Tensor          utils/softmax.py segment_softmax
    torch.ops.gammagl_amd.spmm_sum(index, weight, x)      -> Tensor          c_spmm_sum
    torch.ops.gammagl_amd.spmm_mean(index, weight, x)     -> Tensor          c_spmm_mean
    torch.ops.gammagl_amd.spmm_max(index, weight, x)      -> Tensor          c_spmm_max
    torch.ops.gammagl_amd.bspmm_sum(index, weight, x)     -> Tensor          c_bspmm_sum
    torch.ops.gammagl_amd.gat_fused(index, el, er, x, negative_slope, num_nodes, dropout_rate) -> Tensor
    torch.ops.gammagl_amd.bias_act(a, bias, relu, p_drop) -> Tensor
    torch.ops.gammagl_amd.spmm_sum_x16(index, weight, x, out_f32) -> Tensor   (not in the reference, see below)
    torch.ops.gammagl_amd.spmm_mean_x16(index, weight, x, out_f32) -> Tensor
    torch.ops.gammagl_amd.gat_fused_x16(index, el, er, x, negative_slope, num_nodes, dropout_rate, out_f32) -> Tensor
    torch.ops.gammagl_amd.spmm_grad_w(index, x, grad, mean) -> Tensor         (not in the reference, see below)
    torch.ops.gammagl_amd.edge_softmax_aggregate(index, logits, x, num_nodes, dropout_rate) -> Tensor   (see below)
    torch.ops.gammagl_amd.dot_attention(index, q, k, v, num_nodes, scale, dropout_rate) -> Tensor        (see below)
    torch.ops.gammagl_amd.gatv2_attention(index, xl, xr, att, num_nodes, negative_slope, dropout_rate) -> Tensor  (see below)
    torch.ops.gammagl_amd.segment_multi(x, index, N, aggs, C, empty_zero) -> Tensor                      (see below)

``spmm_sum`` / ``spmm_mean`` also take ``x`` stored as bf16 / f16 (the reference is f32 only): the sums are made in f32 and
rounded once to x's dtype.  ``spmm_*_x16(..., out_f32=True)`` returns those f32 sums unrounded.  ``gat_fused`` does the
same for its ``x`` (``el`` / ``er`` stay f32; softmax and sums in f32), ``gat_fused_x16`` adds the ``out_f32`` choice.
``spmm_sum`` / ``spmm_mean`` differentiate with respect to ``weight`` too (the reference's extension does not):
``spmm_grad_w`` is that gradient, ``gw[e] = sum_k x[src_e, k] * grad[dst_e, k]`` in f32 (``mean``: grad / edge count first).
``edge_softmax_aggregate`` is ``gat_fused`` on per-edge logits ``[E, H]`` (any attention layer that calls segment_softmax on
its logits and sums ``alpha * x[src]``): ``out[i, h] = sum_{e -> i} dropout(softmax_i(logits[:, h]))[e] * x[src_e, h]``, f32.
``dot_attention`` is that op with the logits formed from node rows, ``logits[e, h] = scale * <q[dst_e, h], k[src_e, h]>``
(``scale`` defaults to ``1 / sqrt(C)``) and ``x = v``: scaled dot-product attention over a graph, f32.
``gatv2_attention`` is that op with GATv2's additive logits, ``logits[e, h] = sum_c att[h, c] * leaky_relu(xl[src_e, h, c] +
xr[dst_e, h, c])`` and ``x = xl``, f32, differentiable in ``xl``, ``xr`` and ``att``.
``segment_multi`` returns several statistics of ``x [E, K]`` per segment from one walk: ``aggs`` are distinct GGL_AGG_* codes
(0 sum, 1 mean, 2 min, 3 max, 4 var, 5 std), the result is ``[N, K / C, A, C]`` stored as ``[N, A * K]``, f32.

Kernels are registered for ``CUDA`` / ``AutogradCUDA`` (= HIP on ROCm: libggl_mpops_hip.so) and for ``CPU`` /
``AutogradCPU`` (libggl_mpops_host.so, the host build of the same kernel sources) — the reference's ops dispatch
on ``x.is_cuda()`` / ``x.is_cpu()`` the same way (src/segment_sum.cpp:19-33).  The dispatcher routes by the
tensors' device: a GPU tensor can only ever reach the HIP library (a missing one fails loudly at first use), a CPU
tensor only the host build.  Each kernel forwards to the engine entry point of the same name (gammagl_amd/ops.py),
i.e. ctypes -> C ABI (include/ggl_mpops.h) -> kernel; the autograd formulas are the ``torch.autograd.Function``s
defined there.  Fake (meta) kernels
give shapes/dtypes so the ops trace under ``torch.compile`` / FakeTensor without running.
"""
import torch
from torch.library import Library

NS = "gammagl_amd"

_SCHEMAS = {
    "segment_sum": "(Tensor x, Tensor index, int N) -> Tensor",
    "segment_mean": "(Tensor x, Tensor index, int N) -> Tensor",
    "segment_max": "(Tensor x, Tensor index, int N) -> (Tensor, Tensor)",
    "segment_softmax": "(Tensor x, Tensor index, int N) -> Tensor",
    "spmm_sum": "(Tensor index, Tensor? weight, Tensor x) -> Tensor",
    "spmm_mean": "(Tensor index, Tensor? weight, Tensor x) -> Tensor",
    "spmm_max": "(Tensor index, Tensor? weight, Tensor x) -> Tensor",
    "bspmm_sum": "(Tensor index, Tensor weight, Tensor x) -> Tensor",
    "gat_fused": "(Tensor index, Tensor el, Tensor er, Tensor x, float negative_slope=0.2, "
                 "int? num_nodes=None, float dropout_rate=0.0) -> Tensor",
    "bias_act": "(Tensor a, Tensor? bias, bool relu, float p_drop) -> Tensor",
    "spmm_sum_x16": "(Tensor index, Tensor? weight, Tensor x, bool out_f32=False) -> Tensor",
    "spmm_mean_x16": "(Tensor index, Tensor? weight, Tensor x, bool out_f32=False) -> Tensor",
    "gat_fused_x16": "(Tensor index, Tensor el, Tensor er, Tensor x, float negative_slope=0.2, "
                     "int? num_nodes=None, float dropout_rate=0.0, bool out_f32=False) -> Tensor",
    "spmm_grad_w": "(Tensor index, Tensor x, Tensor grad, bool mean) -> Tensor",
    "edge_softmax_aggregate": "(Tensor index, Tensor logits, Tensor x, int? num_nodes=None, float dropout_rate=0.0) -> Tensor",
    "dot_attention": "(Tensor index, Tensor q, Tensor k, Tensor v, int? num_nodes=None, float? scale=None, "
                     "float dropout_rate=0.0) -> Tensor",
    "gatv2_attention": "(Tensor index, Tensor xl, Tensor xr, Tensor att, int? num_nodes=None, float negative_slope=0.2, "
                       "float dropout_rate=0.0) -> Tensor",
    "segment_multi": "(Tensor x, Tensor index, int N, int[] aggs, int C, bool empty_zero=False) -> Tensor",
}

_DEF = Library(NS, "DEF")
for _name, _sig in _SCHEMAS.items():
    _DEF.define(_name + _sig)
_IMPLS = []  # Library handles must stay alive for their registrations to stay
_ENGINES = {}  # dispatch key -> [callable returning the engine its kernels run on]


def _kernels(get_engine):
    """name -> python kernel, each a thin call into the engine returned by ``get_engine()``."""
    return {
        "segment_sum": lambda x, index, N: get_engine().c_segment_sum(x, index, N),
        "segment_mean": lambda x, index, N: get_engine().c_segment_mean(x, index, N),
        "segment_max": lambda x, index, N: get_engine().segment_max_with_arg(x, index, N),
        "segment_softmax": lambda x, index, N: get_engine().segment_softmax(x, index, N),
        "spmm_sum": lambda index, weight, x: get_engine().c_spmm_sum(index, weight, x),
        "spmm_mean": lambda index, weight, x: get_engine().c_spmm_mean(index, weight, x),
        "spmm_max": lambda index, weight, x: get_engine().c_spmm_max(index, weight, x),
        "bspmm_sum": lambda index, weight, x: get_engine().c_bspmm_sum(index, weight, x),
        "gat_fused": lambda index, el, er, x, negative_slope=0.2, num_nodes=None, dropout_rate=0.0:
            get_engine().gat_fused(index, el, er, x, negative_slope, num_nodes, dropout_rate, True),
        "bias_act": lambda a, bias, relu, p_drop: get_engine().bias_act(a, bias, relu, p_drop, True),
        "spmm_sum_x16": lambda index, weight, x, out_f32=False: _x16(get_engine().c_spmm_sum, index, weight, x, out_f32),
        "spmm_mean_x16": lambda index, weight, x, out_f32=False: _x16(get_engine().c_spmm_mean, index, weight, x, out_f32),
        "gat_fused_x16": lambda index, el, er, x, negative_slope=0.2, num_nodes=None, dropout_rate=0.0, out_f32=False:
            _gat_x16(get_engine(), index, el, er, x, negative_slope, num_nodes, dropout_rate, out_f32),
        "spmm_grad_w": lambda index, x, grad, mean: get_engine().spmm_grad_w(index, x, grad, mean),
        "edge_softmax_aggregate": lambda index, logits, x, num_nodes=None, dropout_rate=0.0:
            get_engine().edge_softmax_aggregate(index, logits, x, num_nodes, dropout_rate, True),
        "dot_attention": lambda index, q, k, v, num_nodes=None, scale=None, dropout_rate=0.0:
            get_engine().dot_attention(index, q, k, v, num_nodes, scale, dropout_rate, True),
        "gatv2_attention": lambda index, xl, xr, att, num_nodes=None, negative_slope=0.2, dropout_rate=0.0:
            get_engine().gatv2_attention(index, xl, xr, att, num_nodes, negative_slope, dropout_rate, True),
        "segment_multi": lambda x, index, N, aggs, C, empty_zero=False:
            get_engine().segment_multi(x, index, N, tuple(aggs), C, empty_zero),
    }


def _gat_x16(eng, index, el, er, x, negative_slope, num_nodes, dropout_rate, out_f32):
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError(f"gat_fused_x16 takes f16 / bf16 rows (x is {x.dtype})")
    return eng.gat_fused(index, el, er, x, negative_slope, num_nodes, dropout_rate, True,
                         out_dtype=torch.float32 if out_f32 else None)


def _x16(fn, index, weight, x, out_f32):
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError(f"spmm_*_x16 takes f16 / bf16 rows (x is {x.dtype})")
    return fn(index, weight, x, out_dtype=torch.float32 if out_f32 else None)


def register_backend(get_engine, backend="CUDA"):
    """Bind every op to ``get_engine()`` for dispatch key ``backend`` and its autograd key.

    The package registers ``CUDA`` (the MI355X engine) and ``CPU`` (the host build) at import; a later
    registration for the same key replaces the earlier one's engine (the CPU test-suite binds ``CPU`` to its own
    -O1 / AddressSanitizer builds of the same sources).
    """
    slot = _ENGINES.get(backend)
    if slot is not None:        # already registered: swap the engine the registered kernels resolve to
        slot[0] = get_engine
        return None
    slot = _ENGINES[backend] = [get_engine]
    lib = Library(NS, "IMPL")
    for name, fn in _kernels(lambda: slot[0]()).items():
        lib.impl(name, fn, backend)
        lib.impl(name, fn, "Autograd" + backend)
    _IMPLS.append(lib)
    return lib


def _register_fakes():
    lib = Library(NS, "IMPL")

    def seg(x, index, N):
        return x.new_empty((N,) + tuple(x.shape[1:]))

    def seg_max(x, index, N):
        shape = (N,) + tuple(x.shape[1:])
        return x.new_empty(shape), x.new_empty(shape, dtype=torch.int64)

    def like_x(index, weight, x):
        return torch.empty_like(x)  # gspmm.cpp:16 — out = zeros_like(x): square

    def like_x16(index, weight, x, out_f32=False):
        return torch.empty_like(x, dtype=torch.float32) if out_f32 else torch.empty_like(x)

    def gat(index, el, er, x, negative_slope=0.2, num_nodes=None, dropout_rate=0.0):
        n = x.shape[0] if num_nodes is None else num_nodes
        return x.new_empty((n,) + tuple(x.shape[1:]))

    def gat_x16(index, el, er, x, negative_slope=0.2, num_nodes=None, dropout_rate=0.0, out_f32=False):
        n = x.shape[0] if num_nodes is None else num_nodes
        return x.new_empty((n,) + tuple(x.shape[1:]), dtype=torch.float32 if out_f32 else x.dtype)

    def esa(index, logits, x, num_nodes=None, dropout_rate=0.0):
        n = x.shape[0] if num_nodes is None else num_nodes
        return x.new_empty((n,) + tuple(x.shape[1:]))

    def dot(index, q, k, v, num_nodes=None, scale=None, dropout_rate=0.0):
        n = q.shape[0] if num_nodes is None else num_nodes
        return v.new_empty((n,) + tuple(v.shape[1:]))

    def gatv2(index, xl, xr, att, num_nodes=None, negative_slope=0.2, dropout_rate=0.0):
        n = xr.shape[0] if num_nodes is None else num_nodes
        return xl.new_empty((n,) + tuple(xl.shape[1:]))

    def multi(x, index, N, aggs, C, empty_zero=False):
        return x.new_empty((N, len(aggs) * x.shape[1]))

    for name, fn in (("segment_multi", multi), ("gatv2_attention", gatv2), ("dot_attention", dot), ("edge_softmax_aggregate", esa), ("segment_sum", seg), ("segment_mean", seg), ("segment_max", seg_max),
                     ("segment_softmax", lambda x, index, N: torch.empty_like(x)),
                     ("spmm_sum", like_x), ("spmm_mean", like_x), ("spmm_max", like_x),
                     ("bspmm_sum", like_x), ("gat_fused", gat),
                     ("bias_act", lambda a, bias, relu, p_drop: torch.empty_like(a)),
                     ("spmm_sum_x16", like_x16), ("spmm_mean_x16", like_x16), ("gat_fused_x16", gat_x16),
                     ("spmm_grad_w", lambda index, x, grad, mean: grad.new_empty((index.shape[1],), dtype=torch.float32))):
        lib.impl(name, fn, "Meta")
    _IMPLS.append(lib)


def _product_engine():
    from . import engine  # raises ImportError when the HIP library is missing: loud, no fallback

    return engine()


def _host_engine():
    import gammagl_amd

    if gammagl_amd._engine is not None and not gammagl_amd._engine.require_cuda:
        return gammagl_amd._engine     # an injected any-device engine (tests)
    return gammagl_amd.host_engine()


_register_fakes()
register_backend(_product_engine, "CUDA")
register_backend(_host_engine, "CPU")

ops = getattr(torch.ops, NS)
