"""Route selection of the separators: which of two equivalent formulations an iteration takes.

Every entry has ONE production value; the other exists because it is the fallback the production
route returns to at run time (the on-Y iterations behind the implied-filter guard, the plain passes
for shapes without a hand-over buffer) and the tests drive it directly to compare the two.  These
are not environment switches: ``override()`` is a context manager for tests and benchmarks
(process-wide: the separators are not re-entrant per instance anyway).
"""

import contextlib

_DEFAULTS = {
    # ISS / ISS2 / IPA iterations read the mixture through the filters their updates imply
    # (bss/ilrma.py: _update_spatial_model_implied, bss/iva.py: _update_once_implied); False: the
    # reference's iterations on Y -- the route the rounding guard falls back to
    "implied_filter": True,
    # ILRMA ISS2 / IPA on Y with the power normalisation folded into the update matrix; False: the
    # literal update -> mean |y|^2 -> y / psi passes (what non-stock subclasses and
    # normalization="projection_back" run)
    "folded_norm": True,
    # ILRMA ISS1 on per-bin statistics: None = by size (batches), True / False force either
    "iss1_statistics": None,
    # FastGaussMNMF keeps |Q x|^2 between the spatial and the NMF passes; False: every pass
    # recomputes it (what shapes without a hand-over buffer run)
    "handover": True,
    # FDICA runs whole iterations of a (mixture, bin) inside ssspy_fdica_steps where
    # ssspy_fdica_route allows; False: the per-iteration operators (what IP2, user closures, host
    # floors and 9..16 sources run)
    "fdica_kernel": True,
    # time-domain ICA applies a named nonlinearity (bss.ica.NAMED: laplace, logistic, logcosh passed
    # as themselves) inside the statistics pass; False: the compatibility route every other callable
    # takes (Y down, Phi up once per iteration; bss.ica.route decides, once per call)
    "ica_named": True,
    # FDICA and CACGMM align the permutations on the device (csrc/permutation.hip) where
    # ssspy_permutation_route allows; False: the NumPy solvers on host copies, one mixture after the
    # other (what 1 or 9..16 sources, flooring callables and overlong frame axes run)
    "device_alignment": True,
    # WPE keeps the slab of a bin in LDS where ssspy_wpe_route puts it there; False: every walk
    # re-reads it in tiles (what longer frame axes run)
    "wpe_resident": True,
    # the beamformers keep the slab of a bin in LDS where ssspy_beamform_route puts it there; False:
    # the apply walk re-reads it in tiles (what longer frame axes run)
    "beamform_resident": True,
    # WPD keeps the slab of a bin in LDS where ssspy_wpd_route puts it there; False: every walk
    # re-reads it in tiles (what longer frame axes run)
    "wpd_resident": True,
    # ConvIVA's statistics kernel keeps the slab of a bin in LDS where ssspy_conviva_route puts it
    # there; False: the walk re-reads it in tiles (what longer frame axes run)
    "conviva_resident": True,
}
VALUES = dict(_DEFAULTS)  # (tests: monkeypatch.setitem(_routes.VALUES, "implied_filter", False))


def get(name):
    return VALUES[name]


@contextlib.contextmanager
def override(**values):
    unknown = set(values) - set(_DEFAULTS)
    if unknown:
        raise KeyError("unknown route(s): {}".format(sorted(unknown)))
    before = dict(VALUES)
    VALUES.update(values)
    try:
        yield
    finally:
        VALUES.clear()
        VALUES.update(before)
