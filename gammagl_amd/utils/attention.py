"""``edge_softmax_aggregate(edge_index, logits, x)``: the edge softmax of per-edge attention logits and the weighted sum of
the source rows, as ONE op per direction.

Every attention layer of the reference but GAT computes one logit per edge and head, calls ``segment_softmax`` on it and
sums ``alpha * x[src]`` per destination (agnn_conv.py:54-66; hgt_conv, fagcn_conv, hardgat_conv, simplehgn_conv, han_conv
likewise).  Composed from this package's ops that is ``utils.segment_softmax`` + ``mpops.bspmm`` and their backward walks:
four passes over ``[E, H]`` more than the data needs.  Here it is the fused GAT's general kernels with the logit READ
instead of built from ``el[src] + er[dst]``: online softmax in one walk of the destination's edges, hub rows
cut into chunks, attention dropout from the library's counter-based draw.
"""

from .. import engine as _engine
from .. import mpops

__all__ = ["edge_softmax_aggregate"]


def edge_softmax_aggregate(edge_index, logits, x, num_nodes=None, dropout_rate=0.0, training=True):
    """``out[i, h, :] = sum over edges e with dst(e) = i of drop(softmax_i(logits[:, h]))[e] * x[src(e), h, :]``.

    ``logits`` [E, H] f32 in the order of ``edge_index``'s columns, taken as they are (no activation); ``x`` [N_src, H, C]
    f32; ``logits`` [E] with ``x`` [N_src, K] are one head.  ``num_nodes`` is the number of destinations (default: x's rows;
    rectangular graphs are fine).  ``dropout_rate`` in [0, 1) drops attention coefficients as ``gat_fused`` does: the softmax
    runs over all edges, kept coefficients weigh ``1 / (1 - p)``.  Differentiable in ``logits`` and ``x``; f32 only — other
    dtypes raise a RuntimeError ("expected scalar type Float").

    Numerics are the fused GAT's: ``-FLT_MAX`` start and strict ``<`` for the maximum, one-walk online softmax,
    ``out = acc / (den + 1e-16)``, zeros for a destination without edges.  A destination whose logits are all ``-inf`` gets
    zeros, like one without edges (no ``-inf`` beats the ``-FLT_MAX`` start, so every ``exp(-inf + FLT_MAX)`` is 0, and
    ``0 / 1e-16 = 0``; its gradients are zeros too); one with a NaN among its logits gets NaN (the NaN never becomes the
    maximum, its ``exp`` poisons the sums): exactly what ``gat_fused`` returns for the same values of
    ``LeakyReLU(el[src] + er[dst])``.

    No shape at which the fused form loses to ``segment_softmax`` + ``bspmm`` has been measured; profiles/edge_softmax_agg.txt
    holds what has been.

    Route: ``torch.ops.ggl_attn`` (registered from C++) when the engine for x's device is the shipped library, the
    Python-registered ``torch.ops.gammagl_amd`` otherwise — as ``mpops`` chooses for the seven reference operators."""
    _engine(x)._dev(edge_index, logits, x)
    p = float(dropout_rate) if training else 0.0
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout_rate must be in [0, 1)")
    ops = mpops._ops_for(x)
    if ops is not mpops._py_ops:
        from .. import cpp_ops

        ops = cpp_ops.load_attn()
    n = None if num_nodes is None else int(num_nodes)
    return ops.edge_softmax_aggregate(mpops._ids(edge_index, x), logits, x, n, p)
