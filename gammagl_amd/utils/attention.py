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

__all__ = ["edge_softmax_aggregate", "dot_attention", "gatv2_attention"]


def _drop_rate(dropout_rate, training):
    """the rate the op is called with: 0 outside training, else dropout_rate in [0, 1)"""
    p = float(dropout_rate) if training else 0.0
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout_rate must be in [0, 1)")
    return p


def _attn_ops(x):
    """``torch.ops.ggl_attn`` when the engine for x's device is the shipped library, the Python-registered operators otherwise"""
    ops = mpops._ops_for(x)
    if ops is not mpops._py_ops:
        from .. import cpp_ops

        ops = cpp_ops.load_attn()
    return ops


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
    p = _drop_rate(dropout_rate, training)
    n = None if num_nodes is None else int(num_nodes)
    return _attn_ops(x).edge_softmax_aggregate(mpops._ids(edge_index, x), logits, x, n, p)


def dot_attention(edge_index, q, k, v, num_nodes=None, scale=None, dropout_rate=0.0, training=True):
    """Scaled dot-product attention over a graph: ``z[e, h] = scale * <q[dst(e), h, :], k[src(e), h, :]>`` and
    ``out[i, h, :] = sum over edges e with dst(e) = i of drop(softmax_i(z[:, h]))[e] * v[src(e), h, :]``.

    What hgt_conv.py:115-153 writes as ``reduce_sum(k_j * q_i, -1) * rel / sqrt(D)`` -> ``segment_softmax`` -> ``v_j * alpha``
    with three ``[E, H, C]`` gathers.  ``q`` [N_dst, H, C], ``k`` and ``v`` [N_src, H, C] f32 (``v`` has k's head width;
    2-d tensors are one head); ``scale`` is a float, ``1 / sqrt(C)`` by default — a learnable per-head factor such as HGT's
    ``p_rel`` is applied to ``q`` on the nodes, where torch differentiates it.  ``num_nodes``, ``dropout_rate`` and
    ``training`` as :func:`edge_softmax_aggregate`, whose numerics everything behind ``z`` shares bit for bit.

    On the GPU, for C = 8, 16, 32 or 64, the dot is formed inside the aggregate's walk (``ggl_dot_attn_fwd``):
    the edge list is read once and ``z`` is written only when a backward will read it — a forward without grad touches no
    ``[E, H]`` array.  Other widths and CPU tensors compose the library's edge dot with :func:`edge_softmax_aggregate`.
    The two routes sum the C products of a dot in different orders, so their ``z`` agree to
    ``gamma_{C+1} |scale| sum_c |q_c k_c|`` of the exact value each, not bit for bit.  Differentiable in q, k and v.

    Route: as :func:`edge_softmax_aggregate` (``torch.ops.ggl_attn`` on the shipped library)."""
    _engine(v)._dev(edge_index, q, k, v)
    p = _drop_rate(dropout_rate, training)
    n = None if num_nodes is None else int(num_nodes)
    return _attn_ops(v).dot_attention(mpops._ids(edge_index, v), q, k, v, n, None if scale is None else float(scale), p)


def gatv2_attention(edge_index, xl, xr, att, num_nodes=None, negative_slope=0.2, dropout_rate=0.0, training=True):
    """GATv2's additive attention over a graph ("How Attentive are Graph Attention Networks?"):
    ``z[e, h] = sum_c att[h, c] * leaky_relu(xl[src(e), h, c] + xr[dst(e), h, c])`` and
    ``out[i, h, :] = sum over edges e with dst(e) = i of drop(softmax_i(z[:, h]))[e] * xl[src(e), h, :]``.

    The LeakyReLU sits inside the channel sum, so the logit is neither GAT's ``el[src] + er[dst]`` nor a dot product; written
    with torch it needs ``xl[src] + xr[dst]`` as an ``[E, H, C]`` tensor, and a second one in the backward.  ``xl`` [N_src, H, C],
    ``xr`` [N_dst, H, C], ``att`` [H, C] f32 (2-d ``xl``, ``xr`` with a 1-d ``att`` are one head).  ``num_nodes``,
    ``dropout_rate`` and ``training`` as :func:`edge_softmax_aggregate`, whose numerics everything behind ``z`` shares bit for bit.

    On the GPU, for C = 8, 16, 32 or 64, the logit is formed inside the aggregate's walk from the value row it gathers anyway
    (``ggl_gatv2_fwd``): ``z`` is written only when a backward will read it.  Other widths and CPU tensors form
    ``z`` with torch in edge blocks of at most 256 MiB in front of the aggregate.  The two routes add the C terms in different
    orders, so their ``z`` agree to ``gamma_{C+2} sum_c |att_c| |leaky_relu(xl_c + xr_c)|`` of the exact value each, not bit
    for bit.  Differentiable in xl, xr and att: the backward is the aggregate's two walks and ``ggl_gatv2_logit_bwd`` on the
    graph and on its transpose; its peak memory is three ``[E, H]`` arrays plus node-sized ones.

    Route: as :func:`edge_softmax_aggregate` (``torch.ops.ggl_attn`` on the shipped library)."""
    _engine(xl)._dev(edge_index, xl, xr, att)
    p = _drop_rate(dropout_rate, training)
    n = None if num_nodes is None else int(num_nodes)
    return _attn_ops(xl).gatv2_attention(mpops._ids(edge_index, xl), xl, xr, att, n, float(negative_slope), p)
