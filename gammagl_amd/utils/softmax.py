"""Drop-in for ``gammagl/utils/softmax.py``: ``segment_softmax(data, segment_ids, num_segments)``.

The reference composes the edge softmax from its segment ops (softmax.py:29-35: segment_max -> gather -> sub / exp ->
segment_sum -> gather -> add / div) and lets autograd replay the chain.  Here f32 logits whose rows the kernel library
takes (``ggl_segment_softmax_supported``: 2 to 64 trailing elements; one-column logits: see ``NATIVE_MIN_WIDTH``) run as ONE op with its own backward
(``torch.ops.ggl.segment_softmax`` -> ``ggl_segment_softmax_fwd`` / ``_bwd``: double row sums, no [N, K] temporaries).
Everything else the composition accepts — f16 / bf16 / f64 logits, wider rows, one-column rows — IS the composition on
``gammagl_amd.mpops``, so this function never handles less than ``gammagl_amd.layers.segment_softmax`` does.
"""
import math

import torch

from .. import engine as _engine
from .. import mpops

__all__ = ["segment_softmax"]

# Rows of ONE column ([E] or [E, 1] logits) are composed too: measured on the MI355X the op's walk is latency-bound, not byte-bound,
# and at K = 1 it loses to the composition's streaming stages (7.9 -> 22.1 ms forward, 27.1 -> 44.6 ms forward + backward on 114.8 M
# elements, profiles/segment_softmax.txt; K = 4 and 8 win 2-4x / 11-13x).  The op itself (torch.ops.ggl.segment_softmax) takes K = 1.
NATIVE_MIN_WIDTH = 2


def _composition(data, segment_ids, num_segments):
    max_values = mpops.unsorted_segment_max(data, segment_ids, num_segments=num_segments)
    exp = torch.exp(data - max_values[segment_ids])
    denominator = mpops.unsorted_segment_sum(exp, segment_ids, num_segments=num_segments)
    return exp / (denominator[segment_ids] + 1e-16)


def segment_softmax(data, segment_ids, num_segments=None):
    """Softmax of ``data[E, ...]`` over the elements that share a segment id, per trailing column (softmax.py:10-36)."""
    assert data.shape[0] == segment_ids.shape[0], "the length of segment_ids should be equal to data.shape[0]."
    n = mpops._num_segments(segment_ids, num_segments)
    ids = mpops._ids(segment_ids, data)
    if math.prod(data.shape[1:]) < NATIVE_MIN_WIDTH or not _engine(data).segment_softmax_supported(data):
        return _composition(data, ids, n)
    return mpops._ops_for(data).segment_softmax(data, ids, n)
