"""Drop-in for ``gammagl/mpops/torch.py`` (the op surface ``from gammagl.mpops import *`` exposes).

Same names, argument meaning and return types as the reference module
(gammagl/mpops/torch.py:43,99,159,209,240,271,302,354), including the module globals ``use_ext``
(read by MessagePassing.message_aggregate, layers/conv/message_passing.py:99) and ``torch`` (which
leaks through the star-import and is used at message_passing.py:101).  Differences, on purpose:

* the work runs in hand-written HIP kernels on MI355X, reached through the dispatcher ops ``torch.ops.ggl.*`` registered from
  C++ (csrc/torch/ggl_torch.cpp; ``torch.ops.gammagl_amd.*``, the same schemas over the ctypes engine, for engines injected by the
  test-suite); CPU tensors dispatch to the host build of the same kernel sources, as the reference dispatches on ``x.is_cpu()``
  (BASELINE config 1: ``--gpu -1``);
* native errors are NOT swallowed: the reference's segment wrappers catch every exception and
  silently re-run a pure-torch fallback (torch.py:83-86,139-142,199-202) that disagrees with the
  C++ extension on empty max segments and integer dtypes; here an error is an error;
* results follow the reference's C++ CPU extension (the implementation its own known-answer tests
  pass on): empty max segments hold numeric_limits<T>::lowest(), integer mean truncates, ties go to
  the first edge.
"""
import torch  # noqa: F401  (re-exported on purpose, see above)

from . import engine as _engine
from . import torch_ops as _torch_ops  # registers torch.ops.gammagl_amd.* (CUDA = HIP kernels, CPU = host build)

_py_ops = _torch_ops.ops
use_ext = True


def _ops_for(x):
    """The operator namespace that serves `x`: ``torch.ops.ggl`` — the seven operators registered from C++ (libggl_torch.so: plan
    cache, launch policy and autograd in C++; what compat/_torch_ext.py binds and, since round 6, what bench.py's one-GPU step runs)
    — whenever the engine for x's device is the shipped library; the Python-registered ``torch.ops.gammagl_amd`` (same schemas over
    the ctypes engine) for an engine injected on another build of the kernel sources (host-emulation / ASan tests) or with
    GGL_CPP_OPS=0."""
    eng = _engine(x)
    eng._dev(x)
    if getattr(eng, "is_product", False):
        from . import cpp_ops

        if cpp_ops.enabled():
            return cpp_ops.load()
    return _py_ops

def _agg_ops_for(x):
    """The namespace of ``segment_multi`` for `x`: ``torch.ops.ggl_agg`` (registered from C++) where ``_ops_for`` answers
    ``torch.ops.ggl``, the Python-registered ``torch.ops.gammagl_amd`` otherwise."""
    ops = _ops_for(x)
    if ops is not _py_ops:
        from . import cpp_ops

        return cpp_ops.load_agg()
    return ops


__all__ = ["unsorted_segment_sum", "unsorted_segment_mean", "unsorted_segment_max", "unsorted_segment_min", "segment_sum",
           "segment_mean", "segment_max", "segment_min", "gspmm", "bspmm", "use_ext", "torch"]


def _num_segments(segment_ids, num_segments):
    if num_segments is None:  # torch.py:74-75 — the one host sync the reference API forces
        num_segments = int(segment_ids.max().item()) + 1
    return int(num_segments)


def _ids(segment_ids, x):
    # the reference extension wants int64 (segment_sum_cpu.cpp:36); its Python fallback casts
    # anything else with .to(torch.long) (torch.py:11) — so the surface accepts any integer dtype
    if segment_ids.dtype != torch.int64:
        segment_ids = segment_ids.to(torch.int64)
    if segment_ids.device != x.device:
        segment_ids = segment_ids.to(x.device)
    return segment_ids


def unsorted_segment_sum(x, segment_ids, num_segments=None):
    """out[s] = sum of x[e] over e with segment_ids[e] == s (torch.py:43-86)."""
    assert x.shape[0] == segment_ids.shape[0], "the length of segment_ids should be equal to data.shape[0]."
    n = _num_segments(segment_ids, num_segments)
    return _ops_for(x).segment_sum(x, _ids(segment_ids, x), n)


def unsorted_segment_mean(x, segment_ids, num_segments=None):
    """Mean along segments; empty segments give 0 (torch.py:99-142)."""
    assert x.shape[0] == segment_ids.shape[0], "the length of segment_ids should be equal to data.shape[0]."
    n = _num_segments(segment_ids, num_segments)
    return _ops_for(x).segment_mean(x, _ids(segment_ids, x), n)


def unsorted_segment_max(x, segment_ids, num_segments=None):
    """Max along segments (torch.py:159-202); empty segments hold lowest() as in the C++ extension."""
    n = _num_segments(segment_ids, num_segments)
    assert x.shape[0] == segment_ids.shape[0], "the length of segment_ids should be equal to data.shape[0]."
    return _ops_for(x).segment_max(x, _ids(segment_ids, x), n)[0]


def unsorted_segment_min(x, segment_ids, num_segments=None):
    """Min along segments (what layers/pool/glob.py:89-114 and pna_conv.py:169 call): the mirror of
    :func:`unsorted_segment_max` — the first element wins ties, NaN never wins, empty segments hold
    ``numeric_limits<T>::max()``.  f32 runs the multi-statistic walk with the one aggregate ``min`` (no sums are carried;
    the gradient goes to the witness only, like max's); f16 / bf16 / f64 run ``-unsorted_segment_max(-x)``, which is exact
    (same winner, same tie and NaN rule, ``-lowest() == max()``); integer dtypes run ``~unsorted_segment_max(~x)``, which
    reverses the order without overflow."""
    n = _num_segments(segment_ids, num_segments)
    assert x.shape[0] == segment_ids.shape[0], "the length of segment_ids should be equal to data.shape[0]."
    if x.dtype == torch.float32:
        E = x.shape[0]
        K = x.numel() // E if E > 0 else int(torch.Size(x.shape[1:]).numel())
        out = _agg_ops_for(x).segment_multi(x.reshape(E, K), _ids(segment_ids, x), n, [2], max(K, 1), False)
        return out.reshape((n,) + tuple(x.shape[1:]))
    if x.dtype.is_floating_point:
        return -unsorted_segment_max(-x, segment_ids, n)
    return ~unsorted_segment_max(~x, segment_ids, n)


def segment_min(x, segment_ids, num_segments=None):
    return unsorted_segment_min(x, segment_ids, num_segments)


def segment_max(x, segment_ids, num_segments=None):
    return unsorted_segment_max(x, segment_ids, num_segments)  # torch.py:209-237


def segment_mean(x, segment_ids, num_segments=None):
    return unsorted_segment_mean(x, segment_ids, num_segments)  # torch.py:240-268


def segment_sum(x, segment_ids, num_segments=None):
    return unsorted_segment_sum(x, segment_ids, num_segments)  # torch.py:271-299


def gspmm(index, weight=None, x=None, reduce='sum'):
    """Generalized SpMM: out[dst] = reduce_e weight[e] * x[src] (torch.py:302-351).

    An extension over the reference, which is f32 only: for 'sum' and 'mean', ``x`` may be STORED as bfloat16 / float16
    (what a preceding Linear produces under ``torch.autocast``).  Every product and add is then made in f32, in the f32
    op's order, and the result is rounded once to x's dtype: ``gspmm(i, w, x16) == gspmm(i, w, x16.float()).to(x16.dtype)``
    bit for bit; the gradient w.r.t. x follows the same rule.  ``weight`` stays f32.  'max' and ``bspmm`` are f32 only.
    (The layer epilogue on such rows — f32 bias, ReLU, dropout, one rounding at the aggregate's store — is ``Engine.spmm_epi`` /
    ``torch.ops.ggl.spmm_epi``; nothing here applies it in torch.)

    A second extension: 'sum' and 'mean' differentiate with respect to ``weight`` (the reference's extension returns no
    weight gradient, gspmm.cpp:79).  ``weight.grad[e] = sum_k x[src_e, k] * g[dst_e, k]`` — for 'mean' with ``g`` divided
    by the destination row's edge count first — in f32, k ascending, rounded multiply then rounded add, whatever ``x``
    and ``g`` are stored as; no [E, K] tensor is formed.  A weight that does not require grad costs nothing new.  'max'
    does not: its witnesses are source-node ids, so its weight stays a constant there.  A weight used twice on the same
    graph is read from a sorted copy cached by its storage and version: change a learnable weight with in-place ops on the
    tensor (an optimizer step does), not through ``weight.data``, which leaves the version and so the cached copy as they were."""
    _engine(x)._dev(index, weight, x)
    _ops = _ops_for(x)
    # weight=None: torch.py:332-333 builds ones([E]) f32; w * x == x exactly, so the kernels simply skip
    # the multiply when no weight pointer is passed
    if reduce == 'sum':
        return _ops.spmm_sum(index, weight, x)
    elif reduce == 'mean':
        return _ops.spmm_mean(index, weight, x)
    elif reduce == 'max':
        return _ops.spmm_max(index, weight, x)
    else:
        raise Exception("Unsupported reduce type, please choose from ['sum', 'mean', 'max'].")


def bspmm(index, weight=None, x=None, reduce='sum'):
    """Multi-head SpMM: out[dst,h,:] = sum_e weight[e,h] * x[src,h,:] (torch.py:354-365)."""
    if weight is None:
        # torch.py:355-356 builds a 1-D ones([E]) that the C++ kernel then indexes as [E,H] (an
        # out-of-bounds read for H > 1); the only meaningful reading is "all heads weigh 1"
        weight = torch.ones((index.shape[1], x.shape[1]), dtype=torch.float32, device=x.device)
    if reduce == 'sum':
        _engine(x)._dev(index, weight, x)
        return _ops_for(x).bspmm_sum(index, weight, x)
    else:
        raise Exception("Unsupported reduce type, please choose from ['sum'].")
