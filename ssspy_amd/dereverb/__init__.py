"""Dereverberation in front of the separators: weighted prediction error (WPE)."""

from .wpe import WPE

__all__ = ["WPE"]
