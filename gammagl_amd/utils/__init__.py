"""Drop-ins for ``gammagl/utils`` functions that have a native op here (same module paths as the reference)."""
from .softmax import segment_softmax

__all__ = ["segment_softmax"]
