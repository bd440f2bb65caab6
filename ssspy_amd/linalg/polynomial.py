"""Cube roots and the roots of cubic equations.  Host only: O(n) NumPy expressions, no kernel.

Counterparts of ``ssspy.linalg.cbrt`` and ``ssspy.linalg.solve_cubic`` (ssspy/linalg/cubic.py,
polynomial.py), written from Cardano's formula.
"""

from typing import Optional

import numpy as np
from numpy.linalg import LinAlgError

__all__ = ["cbrt", "solve_cubic"]

# the primitive cube roots of unity
_OMEGA = complex(-0.5, np.sqrt(3) / 2)
_OMEGA_CONJ = complex(-0.5, -np.sqrt(3) / 2)


def cbrt(x: np.ndarray) -> np.ndarray:
    """Cube root.  Host only.

    Real input: the real cube root (negative for a negative number).  Complex input: the principal
    root, a third of the argument in (-pi, pi] and the real cube root of the modulus.
    """
    if np.iscomplexobj(x):
        return np.cbrt(np.abs(x)) * np.exp(1j * np.angle(x) / 3)
    return np.cbrt(x)


def solve_cubic(
    A: np.ndarray,
    B: np.ndarray,
    C: np.ndarray,
    D: Optional[np.ndarray] = None,
    all: bool = True,
) -> np.ndarray:
    """Roots of cubic equations, elementwise over arrays of coefficients.  Host only.

    With ``D``: ``A x^3 + B x^2 + C x + D = 0`` (``A`` nowhere zero, else ``LinAlgError``); without:
    ``x^3 + A x^2 + B x + C = 0``.  Returns the three complex roots stacked on a new leading axis,
    ``(3, *)``, or with ``all=False`` the first of them, ``(*)``.
    """
    if D is not None:
        if np.any(A == 0):
            raise LinAlgError("Coefficients include zero.")
        return solve_cubic(B / A, C / A, D / A, all=all)
    # x = y - A / 3 turns the monic cubic into the depressed one y^3 + P y + Q = 0
    P = B - A**2 / 3
    Q = 2 * A**3 / 27 - A * B / 3 + C
    roots = _depressed_cubic_roots(P, Q) - A / 3
    return roots if all else roots[0]


def _depressed_cubic_roots(P, Q):
    """The three roots of y^3 + P y + Q = 0, (3, *) complex: Cardano, y = u + v with u^3 one root of
    z^2 + Q z - P^3 / 27 = 0 and u v = -P / 3.  Where P == 0 that u may vanish, and the roots are the
    three cube roots of -Q themselves."""
    P = np.asarray(P).astype(np.complex128)
    Q = np.asarray(Q).astype(np.complex128)
    pure = P == 0
    u = cbrt(-Q / 2 + np.sqrt((Q / 2) ** 2 + (P / 3) ** 3))
    u = np.where(pure, 1, u)  # (any nonzero value: those elements are replaced below)
    v = -P / (3 * u)
    first = np.where(pure, cbrt(-Q), u + v)
    second = np.where(pure, first * _OMEGA, u * _OMEGA + v * _OMEGA_CONJ)
    third = np.where(pure, first * _OMEGA_CONJ, u * _OMEGA_CONJ + v * _OMEGA)
    return np.stack([first, second, third], axis=0)
