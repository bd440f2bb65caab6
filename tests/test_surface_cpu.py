"""The public surface against the reference's, without a device: every name of
tests/golden/public_api.json exists with the reference's parameter names, the host forms of the
small helpers reproduce their fixtures (tests/golden/make_golden_surface.py), and the error paths
raise what the reference raises.

Bars.  The host forms are elementwise NumPy expressions or one small matmul on the fixture's own
float64 inputs; the fixture holds what the reference's expression gave for them.  Two correctly
rounded evaluations of the same formula in another association differ by the operation count times
u = 2^-53 times the magnitude of the terms; each assertion states its count.  None is taken from the
code under test.
"""

import importlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, load_golden

U = 2.0 ** -53


def _resolve(path):
    """ssspy.<module>[.<Class>] of the table -> the object of ssspy_amd."""
    parts = ("ssspy_amd" + path[len("ssspy"):]).split(".")
    for cut in range(len(parts), 0, -1):
        try:
            obj = importlib.import_module(".".join(parts[:cut]))
        except ImportError:
            continue
        for name in parts[cut:]:
            obj = getattr(obj, name)
        return obj
    raise ImportError(path)


def _parameters(fn):
    import inspect

    return [p.name for p in inspect.signature(fn).parameters.values()
            if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD, p.KEYWORD_ONLY)]


def missing_names():
    """Every 'owner.name' of the table that ssspy_amd lacks or declares with other parameters."""
    with open(os.path.join(GOLDEN_DIR, "public_api.json")) as f:
        table = json.load(f)
    missing = []
    for owner, names in sorted(table.items()):
        try:
            target = _resolve(owner)
        except (ImportError, AttributeError):
            missing.append(owner)
            continue
        for name, params in sorted(names.items()):
            if not hasattr(target, name):
                missing.append("{}.{}".format(owner, name))
            elif params is not None:
                ours = _parameters(getattr(target, name))
                if ours[:len(params)] != params:
                    missing.append("{}.{}{}".format(owner, name, tuple(params)))
    return missing


def test_every_reference_name_exists():
    """Fails without this feature on exactly: compute_logdet of the ILRMA and IVA classes,
    update_by_ip2_one_pair, the three PSDTF methods of IPSDTA, linalg.quadratic / cbrt / solve_cubic
    and special.softmax / logsumexp."""
    assert missing_names() == []


# ---------------------------------------------------------------- host forms against the fixtures
def test_cbrt():
    """One cbrt (real), or abs, angle, cbrt, a division, exp and a product (complex): <= 8 roundings
    of a result of magnitude |out|."""
    from ssspy_amd.linalg import cbrt

    g = load_golden("surface_cbrt")
    out = cbrt(g["x_real"])
    assert out.dtype == g["out_real"].dtype
    assert (np.abs(out - g["out_real"]) <= 2 * U * np.abs(g["out_real"])).all()
    assert (out[g["x_real"] < 0] < 0).all()
    outc = cbrt(g["x_complex"])
    assert np.iscomplexobj(outc)
    assert (np.abs(outc - g["out_complex"]) <= 8 * U * np.abs(g["out_complex"])).all()


def _cubic_bars(a, b, c, roots, ref):
    """Roots of x^3 + a x^2 + b x + c.  Cardano's chain is about 40 operations from (a, b, c) to a
    root -- P (3), Q (7), the discriminant (6), sqrt, cbrt (8), v (3), the combinations (6), the
    shift (2) -- on terms no larger than m = max(|a|, |b|^(1/2), |c|^(1/3), |root|); its
    intermediates cancel (U + V, -Q / 2 + sqrt(.)) by at most 1 / |disc|^(1/2) relative to m^3, which
    the generator bounds away from a double root.  Against the fixture, two runs of the same chain:
    |root - ref| <= 40 u m / sep^2 with sep = min_{j != k} |ref_j - ref_k| / m (the conditioning of a
    root: 1 / |p'(root)| = 1 / prod |root - other| <= 1 / (m sep)^2, times the backward error
    40 u m^3).  Residual: |p(root)| <= 40 u (|root|^3 + |a| |root|^2 + |b| |root| + |c|) / sep, the
    same count on the polynomial's own terms, with one factor 1 / sep for the cancellation in
    U + V."""
    m = np.maximum.reduce([np.abs(a), np.sqrt(np.abs(b)), np.cbrt(np.abs(c)), np.abs(ref).max(axis=0)])
    gaps = [np.abs(ref[j] - ref[k]) for j in range(3) for k in range(j + 1, 3)]
    sep = np.minimum(np.minimum.reduce(gaps) / m, 1.0)
    assert (sep > 1e-3).all(), "the fixture must hold no double root"
    assert (np.abs(roots - ref) <= 40 * U * m / sep**2).all()
    terms = np.abs(roots) ** 3 + np.abs(a) * np.abs(roots) ** 2 + np.abs(b) * np.abs(roots) + np.abs(c)
    resid = np.abs(roots**3 + a * roots**2 + b * roots + c)
    assert (resid <= 40 * U * terms / sep).all()


def test_solve_cubic():
    from ssspy_amd.linalg import solve_cubic

    g = load_golden("surface_solve_cubic")
    A, B, C = g["A"], g["B"], g["C"]
    assert np.count_nonzero(B - A**2 / 3 == 0) == 1, "the fixture holds one P == 0 element"
    roots = solve_cubic(A, B, C)
    assert roots.shape == (3,) + A.shape and roots.dtype == np.complex128
    _cubic_bars(A, B, C, roots, g["roots"])
    # all=False is the first of the three, in the reference (the fixture) and here
    assert np.array_equal(g["first"], g["roots"][0]) and np.array_equal(g["first4"], g["roots4"][0])
    assert np.array_equal(solve_cubic(A, B, C, all=False), roots[0])
    A4, B4, C4, D4 = g["A4"], g["B4"], g["C4"], g["D4"]
    roots4 = solve_cubic(A4, B4, C4, D4)
    _cubic_bars(B4 / A4, C4 / A4, D4 / A4, roots4, g["roots4"])
    assert np.array_equal(solve_cubic(A4, B4, C4, D4, all=False), roots4[0])


def test_solve_cubic_zero_leading_coefficient():
    from ssspy_amd.linalg import solve_cubic

    one = np.ones(3)
    with pytest.raises(np.linalg.LinAlgError, match="Coefficients include zero."):
        solve_cubic(np.array([1.0, 0.0, 2.0]), one, one, one)


def test_quadratic_host():
    """(x^H A) x: n^2 complex products and as many additions per form, each of a real or imaginary
    part a sum of 2 n^2 real products: |d| <= (2 n^2 + 2) u sum_ac |x_a| |A_ac| |x_c| in any order."""
    from ssspy_amd.linalg import quadratic

    g = load_golden("surface_quadratic")
    for X, A, ref in ((g["X"], g["A"], g["out"]), (g["X_real"], g["A_real"], g["out_real"])):
        out = quadratic(X, A)
        n = X.shape[-1]
        assert out.shape == ref.shape and out.dtype == ref.dtype
        terms = np.einsum("...a,...ac,...c->...", np.abs(X), np.abs(A), np.abs(X))
        assert (np.abs(out - ref) <= (2 * n * n + 2) * U * terms).all()


def test_softmax_logsumexp_host():
    """x - max is exact up to u |x - max|, exp two roundings on top, the sum of len positive terms
    (len - 1) u, the quotient one: |d softmax| <= (2 max|x - max| + len + 6) u softmax;
    |d logsumexp| <= (2 max|x - max| + len + 6) u + 2 u |log s| + u |out|."""
    from ssspy_amd.special import logsumexp, softmax

    g = load_golden("surface_softmax")
    X = g["X"]
    for axis, key in ((None, "none"), (0, "0"), (1, "1"), (2, "2"), ((0, 2), "02")):
        length = X.size if axis is None else int(np.prod([X.shape[a] for a in np.atleast_1d(axis)]))
        spread = np.max(X) - np.min(X)
        rel = (2 * spread + length + 6) * U
        out = softmax(X, axis=axis)
        ref = g["softmax_" + key]
        assert out.shape == ref.shape and out.dtype == X.dtype and np.isfinite(out).all()
        assert (np.abs(out - ref) <= rel * ref).all()
        lse = logsumexp(X, axis=axis)
        ref = g["logsumexp_" + key]
        assert np.shape(lse) == ref.shape and np.isfinite(lse).all()
        assert (np.abs(lse - ref) <= rel + 3 * U * (np.abs(ref) + np.log(length))).all()
    keep = logsumexp(X, axis=(0, 2), keepdims=True)
    assert keep.shape == g["logsumexp_02_keep"].shape == (1, 7, 1)
    assert softmax(X.astype(np.float32), axis=1).dtype == np.float32


def test_compute_logdet_host():
    """numpy.linalg.slogdet on both sides, the reference's own line: the same LAPACK call on the same
    input; n^3 operations of an LU on entries of magnitude ||W||, conditioned by kappa(W):
    |d| <= n^3 u kappa_2(W)."""
    from ssspy_amd.bss.ilrma import GGDILRMA, TILRMA, GaussILRMA
    from ssspy_amd.bss.iva import AuxGaussIVA, AuxLaplaceIVA

    g = load_golden("surface_logdet")
    for cls, key in ((GaussILRMA, "ilrma"), (TILRMA, "ilrma"), (GGDILRMA, "ilrma"),
                     (AuxLaplaceIVA, "iva"), (AuxGaussIVA, "iva")):
        kwargs = {"n_basis": 2} if key == "ilrma" else {}
        if cls is TILRMA:
            kwargs["dof"] = 100
        if cls is GGDILRMA:
            kwargs["beta"] = 1.5
        W = g["W_" + key]
        out = cls(**kwargs).compute_logdet(W)
        n = W.shape[-1]
        assert out.shape == g["logdet_" + key].shape
        assert (np.abs(out - g["logdet_" + key]) <= n**3 * U * np.linalg.cond(W)).all()


def test_normalize_psdtf_host():
    """A trace (n - 1 additions), one division per entry, one product per activation: 2 u |out| for
    the activation, (n + 1) u |out| for the basis."""
    from ssspy_amd.bss.ipsdta import IPSDTABase

    g = load_golden("surface_normalize_psdtf")
    m = IPSDTABase(n_basis=3)
    m.source_normalization = True
    m.basis, m.activation = g["basis"].copy(), g["activation"].copy()
    m.normalize_psdtf()
    n = g["basis"].shape[-1]
    assert (np.abs(m.basis - g["out_basis"]) <= (n + 1) * U * np.abs(g["out_basis"])).all()
    assert (np.abs(m.activation - g["out_activation"]) <= (n + 1) * U * g["out_activation"]).all()
    tr = np.trace(m.basis, axis1=-2, axis2=-1).real
    assert (np.abs(tr - 1) <= (n + 2) * U).all()


# ---------------------------------------------------------------- error paths
def test_normalize_psdtf_needs_source_normalization():
    from ssspy_amd.bss.ipsdta import GaussIPSDTA, IPSDTABase

    m = IPSDTABase(n_basis=2)
    m.source_normalization = False
    m.basis, m.activation = np.eye(2)[None, None] + 0j, np.ones((1, 1, 3))
    with pytest.raises(AssertionError, match="Set source_normalization."):
        m.normalize_psdtf()
    b = GaussIPSDTA(n_basis=2, n_blocks=2, source_normalization=False)
    with pytest.raises(AssertionError, match="Set source_normalization."):
        b.normalize_block_decomposition_psdtf()


def test_reconstruct_tuple_needs_remainder():
    from ssspy_amd.bss.ipsdta import GaussIPSDTA

    m = GaussIPSDTA(n_basis=2, n_blocks=2)
    m.n_bins = 4  # no remainder: a pair of bases has no meaning
    pair = (np.zeros((2, 2, 1, 2, 2), complex), np.zeros((2, 2, 1, 3, 3), complex))
    with pytest.raises(AssertionError, match="n_remains is expected to be positive."):
        m.reconstruct_block_decomposition_psdtf(pair, np.ones((2, 2, 3)))


def test_unsupported_device_tensors_raise():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no device present")
    from ssspy_amd.bss.ilrma import GaussILRMA
    from ssspy_amd.linalg import quadratic
    from ssspy_amd.special import logsumexp, softmax

    x = torch.zeros((3, 4), dtype=torch.float64, device="cuda")
    for call in (lambda: softmax(x), lambda: softmax(x, axis=(0, 1)), lambda: logsumexp(x),
                 lambda: logsumexp(x, axis=(0, 1)), lambda: softmax(x.float(), axis=0),
                 lambda: logsumexp(x.float(), axis=0),
                 lambda: quadratic(torch.zeros((2, 17), dtype=torch.complex128, device="cuda"),
                                   torch.zeros((2, 17, 17), dtype=torch.complex128, device="cuda")),
                 lambda: quadratic(x, torch.zeros((3, 4, 4), dtype=torch.float64, device="cuda")),
                 lambda: GaussILRMA(n_basis=2).compute_logdet(
                     torch.zeros((2, 17, 17), dtype=torch.complex128, device="cuda"))):
        with pytest.raises(NotImplementedError, match="convert to NumPy"):
            call()
