"""What of ADMMBSS / MaskingADMMBSS / ADMMIVA / PDSIVA needs no device: constructor errors and
warnings, ``repr`` strings (against the reference's, tests/golden/admmbss_repr.npz), the
``record_loss`` defaults, the exports and the default penalty of the IVA front ends being one the
kernels apply."""

import functools
import warnings

import numpy as np
import pytest

import admmbss_numpy as an
from conftest import load_golden


def _admm():
    from ssspy_amd.bss import admmbss

    return admmbss


def _iva():
    from ssspy_amd.bss import iva

    return iva


def _fn(y, step_size=1):
    return y


def test_constructor_errors():
    admm = _admm()
    for cls in (admm.ADMMBSSBase, admm.ADMMBSS):
        with pytest.raises(ValueError, match="proximal operator"):
            cls(prox_penalty=None, record_loss=False)
        with pytest.raises(ValueError, match="reference_id"):
            cls(prox_penalty=_fn, reference_id=None, record_loss=False)
        cls(prox_penalty=_fn, reference_id=None, scale_restoration=False, record_loss=False)
        with pytest.raises(AssertionError, match="set penalty_fn"):
            cls(prox_penalty=_fn, record_loss=True)
        with pytest.raises(AssertionError, match="Length"):
            cls(penalty_fn=[_fn], prox_penalty=[_fn, _fn])
    # record_loss defaults to True in ADMMBSS (the reference's): no penalty_fn, no default object
    with pytest.raises(AssertionError, match="set penalty_fn"):
        admm.ADMMBSS(prox_penalty=_fn)
    with pytest.raises(ValueError, match="masking function"):
        admm.MaskingADMMBSS(mask_fn=None)
    with pytest.raises(ValueError, match="reference_id"):
        admm.MaskingADMMBSS(mask_fn=_fn, reference_id=None)
    with pytest.raises(AssertionError, match="set penalty_fn"):
        admm.MaskingADMMBSS(mask_fn=_fn, record_loss=True)
    with pytest.raises(AssertionError, match="callable"):
        admm.MaskingADMMBSS(mask_fn=_fn, penalty_fn=[_fn])
    for cls, kw in ((admm.ADMMBSS, dict(prox_penalty=_fn, record_loss=False)),
                    (admm.MaskingADMMBSS, dict(mask_fn=_fn)),
                    (_iva().ADMMIVA, {}), (_iva().PDSIVA, {})):
        with pytest.warns(DeprecationWarning, match="alpha is deprecated"):
            assert cls(alpha=1.25, **kw).relaxation == 1.25
        with pytest.raises(AssertionError, match="simultaneously"):
            cls(alpha=1.25, relaxation=1.5, **kw)
    m = admm.ADMMBSS(prox_penalty=[_fn, _fn, _fn], record_loss=False)
    assert m.n_penalties == 3 and m.rho == 1 and m.relaxation == 1
    assert admm.MaskingADMMBSS(mask_fn=_fn).n_penalties == 1


def test_record_loss_defaults():
    admm = _admm()
    m = admm.ADMMBSS(penalty_fn=_fn, prox_penalty=_fn)
    assert m.record_loss is True and m.loss == []
    assert admm.ADMMBSS(prox_penalty=_fn, record_loss=False).loss is None
    # the masking class keeps the quirk of the family: None stays None and records nothing
    for m in (admm.MaskingADMMBSS(mask_fn=_fn), admm.MaskingADMMBSS(penalty_fn=_fn, mask_fn=_fn)):
        assert m.record_loss is None and m.loss is None
    assert admm.MaskingADMMBSS(penalty_fn=_fn, mask_fn=_fn, record_loss=True).loss == []
    for cls in (_iva().ADMMIVA, _iva().PDSIVA):
        assert cls().record_loss is True and cls().loss == []


def _repr_objects(ns, iva_ns):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return {
            "base": ns.ADMMBSSBase(prox_penalty=_fn),
            "base_noscale": ns.ADMMBSSBase(prox_penalty=[_fn, _fn], scale_restoration=False),
            "admm_default": ns.ADMMBSS(penalty_fn=_fn, prox_penalty=_fn),
            "admm_two": ns.ADMMBSS(rho=0.5, relaxation=1.5, penalty_fn=[_fn, _fn],
                                   prox_penalty=[_fn, _fn], reference_id=2,
                                   scale_restoration="minimal_distortion_principle"),
            "admm_alpha_noscale": ns.ADMMBSS(alpha=1.25, prox_penalty=_fn, record_loss=False,
                                             scale_restoration=False),
            "masking_default": ns.MaskingADMMBSS(mask_fn=_fn),
            "masking_loss": ns.MaskingADMMBSS(rho=2.0, penalty_fn=_fn, mask_fn=_fn,
                                              record_loss=False, scale_restoration=False),
            "admmiva_default": iva_ns.ADMMIVA(),
            "pdsiva_default": iva_ns.PDSIVA(),
        }


def test_repr_strings_are_the_references():
    want = load_golden("admmbss_repr")
    for ns, iva_ns in ((_admm(), _iva()), (an, an)):
        objs = _repr_objects(ns, iva_ns)
        assert set(objs) == set(want)
        for key, obj in objs.items():
            assert repr(obj) == str(want[key]), key
    assert str(want["masking_default"]).startswith("ADMMBSS(n_penalties=1")
    assert str(want["admm_default"]).startswith("ADMMBSS(rho=1, relaxation=1, n_penalties=1")


def test_exports():
    import ssspy_amd.bss as bss

    assert _admm().__all__ == ["ADMMBSS", "MaskingADMMBSS"]
    assert bss.admmbss is _admm() and "admmbss" in bss.__all__
    for name in ("ADMMBSSBase", "ADMMBSS", "MaskingADMMBSS"):
        assert name in bss.__all__ and getattr(bss, name) is getattr(_admm(), name)
    assert "PDSIVA" in _iva().__all__ and "ADMMIVA" in _iva().__all__
    assert issubclass(_iva().PDSIVA, bss.PDSBSS) and issubclass(_iva().ADMMIVA, bss.ADMMBSS)
    assert issubclass(bss.ADMMBSSBase, bss.ProxBSSBase)
    assert "out of scope" not in _iva().__doc__


def test_iva_front_ends():
    from ssspy_amd import _lib
    from ssspy_amd.bss.proxbss import device_prox
    from ssspy_amd.linalg import prox

    rng = np.random.default_rng(4)
    y = rng.standard_normal((3, 5, 7)) + 1j * rng.standard_normal((3, 5, 7))
    for cls in (_iva().PDSIVA, _iva().ADMMIVA):
        with pytest.raises(ValueError, match="Set prox_penalty."):
            cls(contrast_fn=_fn)
        with pytest.raises(ValueError, match="Set contrast_fn."):
            cls(prox_penalty=_fn)
        m = cls()
        # the default penalty is one the kernels apply: the default classes run on the device
        assert m.n_penalties == 1 and device_prox(m.prox_penalty[0]) == _lib.PROX_L21_BINS
        assert isinstance(m.prox_penalty[0], functools.partial)
        assert "step_size" not in m.prox_penalty[0].keywords
        assert np.array_equal(m.prox_penalty[0](y, step_size=0.7), prox.l21(y, step_size=0.7, axis2=1))
        assert np.array_equal(m.contrast_fn(y), np.linalg.norm(y, axis=1))
        assert len(m.penalty_fn) == 1
        value = m.penalty_fn[0](y)
        assert isinstance(value, float) and value == np.sum(np.linalg.norm(y, axis=1))

        def contrast(x):
            return 2 * np.linalg.norm(x, axis=1)

        user = cls(contrast_fn=contrast, prox_penalty=_fn)
        assert user.contrast_fn is contrast and user.prox_penalty == [_fn]
        assert user.penalty_fn[0](y) == np.sum(contrast(y))
        assert device_prox(user.prox_penalty[0]) is None
    assert _iva().PDSIVA(mu1=0.5, mu2=2).mu1 == 0.5 and _iva().ADMMIVA(rho=3).rho == 3
