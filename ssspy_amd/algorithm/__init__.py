from .minimal_distortion_principle import minimal_distortion_principle
from .permutation_alignment import (
    correlation_based_permutation_solver,
    score_based_permutation_solver,
)
from .projection_back import projection_back

__all__ = [
    "projection_back",
    "minimal_distortion_principle",
    "correlation_based_permutation_solver",
    "score_based_permutation_solver",
]
