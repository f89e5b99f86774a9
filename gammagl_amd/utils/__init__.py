"""Drop-ins for ``gammagl/utils`` functions that have a native op here (same module paths as the reference)."""
from .aggregate import segment_multi_aggregate
from .attention import dot_attention, edge_softmax_aggregate, gatv2_attention
from .softmax import segment_softmax

__all__ = ["segment_softmax", "edge_softmax_aggregate", "dot_attention", "gatv2_attention", "segment_multi_aggregate"]
