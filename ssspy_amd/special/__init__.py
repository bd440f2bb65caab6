from .flooring import add_flooring, identity, max_flooring
from .psd import to_psd
from .softmax import logsumexp, softmax

__all__ = ["identity", "max_flooring", "add_flooring", "to_psd", "logsumexp", "softmax"]
