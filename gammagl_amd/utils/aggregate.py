"""``segment_multi_aggregate(x, segment_ids, ...)``: several statistics of the same messages per segment from ONE walk.

PNA's aggregate (pna_conv.py:159-181) asks for the mean, minimum, maximum and standard deviation of one ``[E, T, F]``
message tensor.  Composed from ``mpops.unsorted_segment_*`` that is four to five row walks that each gather the same rows,
an ``[E, T, F]`` tensor of squares and its saved copy; here every message row is read once and a lane carries sum, sum of
squares, minimum, maximum and both witnesses in registers (``ggl_segment_multi_fwd``).
"""
import torch

from .. import engine as _engine
from .. import mpops

__all__ = ["segment_multi_aggregate", "segment_multi_composed", "AGGREGATORS"]

AGGREGATORS = ("sum", "mean", "min", "max", "var", "std")


def segment_multi_aggregate(x, segment_ids, num_segments=None, aggregators=("mean", "min", "max", "std"), empty_zero=False):
    """``x`` [E, F] gives ``[N, A * F]``: the statistics named in ``aggregators`` (distinct names from sum, mean, min, max,
    var, std), concatenated along the last axis in that order; ``x`` [E, T, F] gives ``[N, T, A * F]``, the per-tower
    concatenation of pna_conv.py:182, without a permute.

    ``var = mean(x * x) - mean(x) ** 2`` and ``std = sqrt(relu(var) + 1e-5)`` are the reference's formulas, cancellation
    included; ``mean`` divides where a segment has more than one element.  ``min`` / ``max``: the first element wins ties,
    NaN never wins.  Segments without elements hold 0 for sum / mean / var, ``sqrt(1e-5)`` for std and ``+-FLT_MAX`` for
    min / max — or 0 with ``empty_zero``, which a layer that feeds the result to a Linear wants.  Differentiable in ``x``; the
    backward is one walk that keeps ``x`` only when var or std is requested and the witnesses only for min / max.
    f32 only: other dtypes raise a RuntimeError ("expected scalar type Float").

    Route: ``torch.ops.ggl_agg`` (registered from C++) when the engine for x's device is the shipped library, the
    Python-registered ``torch.ops.gammagl_amd`` otherwise — as ``mpops`` chooses for the seven reference operators."""
    eng = _engine(x)
    eng._dev(x, segment_ids)
    if x.dtype != torch.float32:
        raise RuntimeError(f"expected scalar type Float but found {x.dtype} for x")
    if x.dim() not in (2, 3):
        raise RuntimeError(f"segment_multi_aggregate expects x [E, F] or [E, T, F], got {tuple(x.shape)}")
    assert x.shape[0] == segment_ids.shape[0], "the length of segment_ids should be equal to data.shape[0]."
    codes = list(eng.agg_codes(aggregators))
    n = mpops._num_segments(segment_ids, num_segments)
    E, F = int(x.shape[0]), int(x.shape[-1])
    K = F * (int(x.shape[1]) if x.dim() == 3 else 1)
    out = mpops._agg_ops_for(x).segment_multi(x.reshape(E, K), mpops._ids(segment_ids, x), n, codes, F, bool(empty_zero))
    return out.reshape((n,) + tuple(x.shape[1:-1]) + (len(codes) * F,))


class _ComposedMulti(torch.autograd.Function):
    """The statistics composed from the mpops segment ops (pna_conv.py:159-181), with the backward of the fused walk's
    contract (include/ggl_mpops.h) written in torch, one rounded f32 operation per step and in the contract's order —
    ``c1 = 2 gv / n'``, ``c0 = g_sum + g_mean / n' - c1 mean``, ``t = c0 + c1 x``, ``+ g_max`` and ``+ g_min`` at the witnesses.
    Autograd through the five ops computes the same gradient but adds its terms in its own order, so it agrees with the
    fused walk only to rounding; written this way the two routes of ``PNAConv`` agree on the bits wherever the composed
    forward does (rows walked in one piece)."""

    @staticmethod
    def forward(ctx, x, ids, n, aggs, empty_zero):
        from ..ops import sqrt_rn

        ops = mpops._ops_for(x)
        tail = (1,) * (x.dim() - 1)
        cnt = torch.bincount(ids, minlength=n)
        has = (cnt > 0).reshape((n,) + tail)
        sq = "var" in aggs or "std" in aggs
        mean = var = std = amin = amax = None
        if sq or "mean" in aggs:
            mean = ops.segment_mean(x, ids, n)
        if sq:
            var = ops.segment_mean(x * x, ids, n) - mean * mean
        if "std" in aggs:
            std = sqrt_rn(torch.relu(var) + 1e-5)
        outs = []
        for a in aggs:
            if a == "sum":
                o = ops.segment_sum(x, ids, n)
            elif a == "mean":
                o = mean
            elif a == "max":
                o, amax = ops.segment_max(x, ids, n)
            elif a == "min":
                o, amin = ops.segment_max(-x, ids, n)
                o = -o
            else:
                o = var if a == "var" else std
            if empty_zero and a in ("min", "max"):
                o = torch.where(has, o, torch.zeros((), dtype=o.dtype, device=o.device))
            outs.append(o)
        ctx.aggs, ctx.F = aggs, int(x.shape[-1])
        ctx.save_for_backward(ids, cnt, *(t if t is not None else x.new_empty(0) for t in (x if sq else None, mean if sq else None,
                                                                                          std, amin, amax)))
        return torch.cat(outs, dim=-1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        ids, cnt, x, mean, std, amin, amax = ctx.saved_tensors
        aggs, F = ctx.aggs, ctx.F
        n, A = g.shape[0], len(aggs)
        gs = {a: g[..., i * F:(i + 1) * F] for i, a in enumerate(aggs)}
        shape = gs[aggs[0]].shape
        tail = (1,) * (len(shape) - 1)
        nf = cnt.clamp(min=1).to(g.dtype).reshape((n,) + tail)
        sq = "var" in aggs or "std" in aggs
        c0 = torch.zeros(shape, dtype=g.dtype, device=g.device)
        if "sum" in aggs:
            c0 = c0 + gs["sum"]
        if "mean" in aggs:
            c0 = c0 + gs["mean"] / nf
        if sq:
            gv = gs["var"] if "var" in aggs else None
            if "std" in aggs:
                s0 = float(torch.sqrt(torch.tensor(1e-5, dtype=torch.float32).double()).float())     # sqrtf(1e-5f)
                t = torch.where(std > s0, gs["std"] / (2.0 * std), torch.zeros((), dtype=g.dtype, device=g.device))
                gv = t if gv is None else gv + t
            c1 = (2.0 * gv) / nf
            c0 = c0 - c1 * mean
            gx = c1[ids] * x
            gx = c0[ids] + gx
        else:
            gx = c0[ids]
        e = torch.arange(ids.shape[0], device=g.device).reshape((-1,) + tail)
        if "max" in aggs:
            gx = torch.where(amax[ids] == e, gx + gs["max"][ids], gx)
        if "min" in aggs:
            gx = torch.where(amin[ids] == e, gx + gs["min"][ids], gx)
        return gx, None, None, None, None


def segment_multi_composed(x, segment_ids, num_segments, aggregators=("mean", "min", "max", "std"), empty_zero=False):
    """The result of :func:`segment_multi_aggregate` composed from the ``mpops`` segment ops — one walk per statistic and a
    tensor of squares, the reference's way (pna_conv.py:159-181) — with a backward that follows the fused walk's operation
    order (see ``_ComposedMulti``).  The slow route of ``PNAConv(fused=False)`` and the A/B partner of the fused one."""
    aggs = tuple(aggregators)
    for a in aggs:
        if a not in AGGREGATORS:
            raise ValueError(f'Unknown aggregator "{a}".')
    return _ComposedMulti.apply(x.contiguous(), mpops._ids(segment_ids, x), int(num_segments), aggs, bool(empty_zero))
