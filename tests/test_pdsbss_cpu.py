"""What of the proximal classes needs no device: the extended-precision reference of
``prox.neg_logdet`` against the fp64 SVD form, the host proximal operators, constructor errors,
``repr`` strings (against the reference's, tests/golden/pdsbss_repr.npz), the ``record_loss=None``
quirk and which callables the separator recognises as device operators."""

import functools
import warnings

import numpy as np
import pytest

import pdsbss_numpy as pn
import prox_reference as pr
from conftest import load_golden, rel_err


def _pds():
    from ssspy_amd.bss import pdsbss

    return pdsbss


def _prox():
    from ssspy_amd.linalg import prox

    return prox


def _fn(y, step_size=1):
    return y


# ---- the extended reference
@pytest.mark.parametrize("N", [1, 2, 3, 4, 7, 8, 9, 12, 16])
def test_extended_reference_matches_svd_form(N):
    """On matrices with kappa <= 1e4 the one-sided Jacobi in clongdouble and the fp64 SVD form agree
    to 1e-12 (the SVD form's own error is eps * kappa ~ 1e-12 at most)."""
    rng = np.random.default_rng(40 + N)
    for kappa in (1.0, 1e2, 1e4):
        for mu in (1e-3, 1.0, 1e3):
            X = pr.with_singular_values(rng, N, pr.graded(kappa, N))
            ext = pr.neg_logdet_one(X, mu).astype(np.complex128)
            assert rel_err(ext, pr.neg_logdet_svd(X, mu)) < 1e-12, (kappa, mu)
    X = rng.standard_normal((5, N, N)) + 1j * rng.standard_normal((5, N, N))
    keep = np.linalg.cond(X) <= 1e4
    assert rel_err(pr.neg_logdet(X[keep]).astype(np.complex128), pr.neg_logdet_svd(X[keep])) < 1e-12


def test_extended_reference_on_singular_matrices():
    for X in (np.zeros((4, 4), dtype=complex), np.outer([1, 2, 3, 4], [1, 1j, 0, 2]).astype(complex),
              np.diag([2.0, 0.0, 1.0]).astype(complex)):
        s = np.linalg.svd(X, compute_uv=False)
        want = np.sort((s + np.sqrt(s * s + 4 * 0.7)) / 2)
        R = pr.neg_logdet_one(X, 0.7).astype(np.complex128)
        assert np.isfinite(R).all()
        np.testing.assert_allclose(np.sort(np.linalg.svd(R, compute_uv=False)), want, atol=1e-12)


# ---- the host operators
def test_host_operators_match_restatement():
    prox = _prox()
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, 5, 7)) + 1j * rng.standard_normal((3, 5, 7))
    x[1, :, 2] = 0  # an exactly zero group: 0, not NaN
    for step in (0.3, 1.0, 4.0):
        assert np.array_equal(prox.l1(x, step_size=step), pn.l1(x, step_size=step))
        for axis2 in (0, 1, 2, -1, -2, -3):
            got = prox.l21(x, step_size=step, axis1=0, axis2=axis2)
            # (two ways to round the group norm, eps apart, through 1 - step / norm: the
            # cancellation amplifies eps by |x| / |result|, below 100 on this input)
            assert rel_err(got, pn.l21(x, step_size=step, axis2=axis2)) < 1e-13
            assert np.isfinite(got).all()
    assert np.all(prox.l21(x, axis2=1)[1, :, 2] == 0)
    s = rng.random(6)
    assert np.array_equal(prox.neg_log(s, 2.0), (s + np.sqrt(s**2 + 8.0)) / 2)
    with pytest.raises(AssertionError):
        prox.neg_log(np.array([1.0, -1e-3]))
    from ssspy_amd import linalg

    assert linalg.prox is prox and "prox" in linalg.__all__
    assert set(prox.__all__) == {"l1", "l21", "neg_log", "neg_logdet"}


# ---- constructors
def test_constructor_errors():
    pds = _pds()
    from ssspy_amd.bss.proxbss import ProxBSSBase

    for cls in (ProxBSSBase, pds.PDSBSSBase, pds.PDSBSS):
        with pytest.raises(ValueError, match="proximal operator"):
            cls(prox_penalty=None)
        with pytest.raises(ValueError, match="reference_id"):
            cls(prox_penalty=_fn, reference_id=None)
        cls(prox_penalty=_fn, reference_id=None, scale_restoration=False)
        with pytest.raises(AssertionError, match="set penalty_fn"):
            cls(prox_penalty=_fn, record_loss=True)
        with pytest.raises(AssertionError, match="Length"):
            cls(penalty_fn=[_fn], prox_penalty=[_fn, _fn])
    with pytest.raises(ValueError, match="masking function"):
        pds.MaskingPDSBSS(mask_fn=None)
    with pytest.raises(ValueError, match="reference_id"):
        pds.MaskingPDSBSS(mask_fn=_fn, reference_id=None)
    with pytest.raises(AssertionError, match="set penalty_fn"):
        pds.MaskingPDSBSS(mask_fn=_fn, record_loss=True)
    with pytest.raises(AssertionError, match="callable"):
        pds.MaskingPDSBSS(mask_fn=_fn, penalty_fn=[_fn])
    for cls, kw in ((pds.PDSBSS, dict(prox_penalty=_fn)), (pds.MaskingPDSBSS, dict(mask_fn=_fn))):
        with pytest.warns(DeprecationWarning, match="alpha is deprecated"):
            assert cls(alpha=1.25, **kw).relaxation == 1.25
        with pytest.raises(AssertionError, match="simultaneously"):
            cls(alpha=1.25, relaxation=1.5, **kw)
    m = pds.PDSBSS(prox_penalty=[_fn, _fn, _fn])
    assert m.n_penalties == 3 and pds.MaskingPDSBSS(mask_fn=_fn).n_penalties == 1
    import ssspy_amd.bss as bss

    for name in ("ProxBSSBase", "PDSBSSBase", "PDSBSS", "MaskingPDSBSS"):
        assert name in bss.__all__ and hasattr(bss, name)


def _repr_objects(ns, base):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return {
            "base": base(prox_penalty=_fn),
            "base_noscale": base(prox_penalty=[_fn, _fn], scale_restoration=False),
            "pds_default": ns.PDSBSS(prox_penalty=_fn),
            "pds_two_loss": ns.PDSBSS(mu1=0.5, mu2=2, relaxation=1.5, penalty_fn=[_fn, _fn],
                                      prox_penalty=[_fn, _fn], record_loss=True, reference_id=2,
                                      scale_restoration="minimal_distortion_principle"),
            "pds_alpha_noscale": ns.PDSBSS(alpha=1.25, prox_penalty=_fn, scale_restoration=False),
            "masking_default": ns.MaskingPDSBSS(mask_fn=_fn),
            "masking_loss": ns.MaskingPDSBSS(mu1=2.0, penalty_fn=_fn, mask_fn=_fn, record_loss=False,
                                             scale_restoration=False),
        }


def test_repr_strings_are_the_references():
    from ssspy_amd.bss.proxbss import ProxBSSBase

    want = load_golden("pdsbss_repr")
    for ns, base in ((_pds(), ProxBSSBase), (pn, pn.ProxBSSBase)):
        objs = _repr_objects(ns, base)
        assert set(objs) == set(want)
        for key, obj in objs.items():
            assert repr(obj) == str(want[key]), key
    assert repr(_pds().PDSBSSBase(prox_penalty=_fn)) == \
        "PDSBSS(n_penalties=1, scale_restoration=True, record_loss=None, reference_id=0)"


def test_record_loss_none_records_nothing():
    """The reference works the default of record_loss=None out in a local variable and never stores
    it: the attribute stays None and no loss list exists, with or without penalty_fn."""
    pds = _pds()
    for m in (pds.PDSBSS(penalty_fn=_fn, prox_penalty=_fn), pds.PDSBSS(prox_penalty=_fn),
              pds.MaskingPDSBSS(penalty_fn=_fn, mask_fn=_fn)):
        assert m.record_loss is None and m.loss is None
    m = pds.PDSBSS(penalty_fn=_fn, prox_penalty=_fn, record_loss=True)
    assert m.record_loss is True and m.loss == []
    assert pds.PDSBSS(penalty_fn=_fn, prox_penalty=_fn, record_loss=False).loss is None


def test_device_operator_recognition():
    from ssspy_amd import _lib
    from ssspy_amd.bss.proxbss import device_prox

    prox = _prox()
    partial = functools.partial
    assert device_prox(prox.l1) == _lib.PROX_L1
    assert device_prox(partial(prox.l1)) == _lib.PROX_L1
    assert device_prox(prox.l21) == _lib.PROX_L21_FRAMES  # (the reference's default axis2=-1)
    for axis2, kind in ((1, _lib.PROX_L21_BINS), (-2, _lib.PROX_L21_BINS), (2, _lib.PROX_L21_FRAMES),
                        (-1, _lib.PROX_L21_FRAMES), (0, _lib.PROX_L21_SOURCES),
                        (-3, _lib.PROX_L21_SOURCES)):
        assert device_prox(partial(prox.l21, axis2=axis2)) == kind
        assert device_prox(partial(partial(prox.l21, axis1=0), axis2=axis2)) == kind
    # not recognised: the compatibility path
    assert device_prox(partial(prox.l1, step_size=0.5)) is None
    assert device_prox(partial(prox.l21, step_size=0.5, axis2=1)) is None
    assert device_prox(partial(prox.l21, axis2=3)) is None
    assert device_prox(partial(prox.l21, axis2=(0, 1))) is None
    assert device_prox(lambda z, step_size=1: prox.l21(z, step_size=step_size, axis2=1)) is None
    assert device_prox(pn.l21) is None and device_prox(partial(pn.l21, axis2=1)) is None
    assert device_prox(pn.l1) is None
    assert device_prox(prox.neg_log) is None
    assert device_prox(partial(prox.l1, 1.0)) is None
