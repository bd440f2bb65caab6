"""What of the HVA classes needs no device: the host ``mask_fn`` against the reference's mask
(tests/golden/hva_mask.npz), ``repr`` strings before and after the first evaluation of the mask
(tests/golden/hva_repr.npz), constructor errors and defaults, which ``flooring_fn`` takes the device
route, the refusal of a single bin and the exports."""

import functools
import inspect

import numpy as np
import pytest

import hva_cases as hc
import hva_numpy as hn
from conftest import load_golden, rel_err


def _hva():
    from ssspy_amd.bss import hva

    return hva


def test_host_mask_fn_matches_the_references():
    g = load_golden("hva_mask")
    for F in hc.MASK_BINS:
        m = _hva().MaskingPDSHVA(attenuation=float(g["meta_attenuation"]),
                                 mask_iter=int(g["meta_mask_iter"]))
        mask = m.mask_fn(g["Z_f{}".format(F)])
        assert mask.shape == g["Z_f{}".format(F)].shape and mask.dtype == np.float64
        assert rel_err(mask, g["mask_f{}".format(F)]) < 1e-14


def test_repr_strings_are_the_references():
    want = load_golden("hva_repr")
    for classes in (_hva(), hn.CLASSES):
        objs = hc.repr_objects(classes)
        assert {k for k in want if not k.endswith("_after")} == set(objs)
        for key, obj in objs.items():
            assert repr(obj) == str(want[key]), key
            obj.mask_fn(hc.repr_probe())
            assert repr(obj) == str(want[key + "_after"]), key
    # the quirk: attenuation=None is resolved, and stored, at the first evaluation of the mask
    m = _hva().HVA()
    assert m.attenuation is None and "attenuation" not in repr(m)
    m.mask_fn(hc.repr_probe())
    assert m.attenuation == 1 / 3 and "attenuation=0.3333333333333333" in repr(m)
    assert repr(m).startswith("HVA(") and repr(_hva().MaskingPDSHVA()).startswith("MaskingPDSHVA(")


def test_constructor_defaults_and_errors():
    hva = _hva()
    for cls in (hva.MaskingPDSHVA, hva.HVA):
        params = inspect.signature(cls.__init__).parameters
        assert list(params)[1:] == ["mu1", "mu2", "alpha", "relaxation", "attenuation", "mask_iter",
                                    "flooring_fn", "callbacks", "scale_restoration", "record_loss",
                                    "reference_id"]
        defaults = {k: p.default for k, p in params.items() if k not in ("self", "flooring_fn")}
        assert defaults == dict(mu1=1, mu2=1, alpha=None, relaxation=1, attenuation=None,
                                mask_iter=1, callbacks=None, scale_restoration=True,
                                record_loss=None, reference_id=0)
        floor = params["flooring_fn"].default
        assert isinstance(floor, functools.partial) and floor.keywords == {"eps": 1e-10}
        assert floor.func.__name__ == "max_flooring"
        m = cls()
        assert m.n_penalties == 1 and m.penalty_fn is None and m.loss is None
        assert callable(m.mask_fn) and m.mask_iter == 1 and m.attenuation is None
        assert cls(flooring_fn=None).flooring_fn(3.5) == 3.5  # None becomes the identity
        with pytest.raises(ValueError, match="reference_id"):
            cls(reference_id=None)
        cls(reference_id=None, scale_restoration=False)
        with pytest.raises(AssertionError, match="set penalty_fn"):
            cls(record_loss=True)
        with pytest.warns(DeprecationWarning, match="alpha is deprecated"):
            assert cls(alpha=1.25).relaxation == 1.25
        with pytest.raises(AssertionError, match="simultaneously"):
            cls(alpha=1.25, relaxation=1.5)
    from ssspy_amd.bss.pdsbss import MaskingPDSBSS

    assert issubclass(hva.HVA, hva.MaskingPDSHVA) and issubclass(hva.MaskingPDSHVA, MaskingPDSBSS)


def test_which_flooring_takes_the_device_route():
    from ssspy_amd import _lib
    from ssspy_amd.special import flooring as fl

    cls = _hva().MaskingPDSHVA
    partial = functools.partial
    assert tuple(cls().device_floor()) == (_lib.FLOOR_MAX, 1e-10)
    assert tuple(cls(flooring_fn=None).device_floor()) == (_lib.FLOOR_NONE, 0.0)
    assert tuple(cls(flooring_fn=fl.identity).device_floor()) == (_lib.FLOOR_NONE, 0.0)
    assert tuple(cls(flooring_fn=fl.max_flooring).device_floor()) == (_lib.FLOOR_MAX, fl.EPS)
    assert tuple(cls(flooring_fn=fl.add_flooring).device_floor()) == (_lib.FLOOR_ADD, fl.EPS)
    assert tuple(cls(flooring_fn=partial(fl.add_flooring, eps=1e-6)).device_floor()) == \
        (_lib.FLOOR_ADD, 1e-6)
    assert tuple(cls(flooring_fn=partial(fl.max_flooring, eps=1e-3)).device_floor()) == \
        (_lib.FLOOR_MAX, 1e-3)
    # anything else: the compatibility route with the host mask_fn
    assert cls(flooring_fn=lambda x: np.maximum(x, 1e-10)).device_floor() is None
    assert cls(flooring_fn=partial(fl.max_flooring, 1e-3)).device_floor() is None
    assert cls(flooring_fn=partial(np.maximum, 1e-10)).device_floor() is None
    assert cls(flooring_fn=hc.flooring_of("lambda", fl)).device_floor() is None
    for name in ("max", "add", "none"):
        assert cls(flooring_fn=hc.flooring_of(name, fl)).device_floor() is not None


def test_a_single_bin_is_refused():
    """The reference's irfft raises there ("Invalid number of FFT data points (0)")."""
    Z = np.ones((2, 1, 5), dtype=complex)
    with pytest.raises(ValueError, match="Invalid number of FFT data points"):
        _hva().MaskingPDSHVA().mask_fn(Z)
    with pytest.raises(ValueError, match="Invalid number of FFT data points"):
        hn.varrho(Z)


def test_exports():
    import ssspy_amd.bss as bss

    assert bss.hva is _hva() and "hva" in bss.__all__
    for name in ("MaskingPDSHVA", "HVA"):
        assert name in bss.__all__ and getattr(bss, name) is getattr(_hva(), name)
    assert _hva().__all__ == ["MaskingPDSHVA", "HVA"]


def test_route_constants_mirror_the_header():
    import os
    import re

    from conftest import ROOT
    from ssspy_amd import _lib

    text = open(os.path.join(ROOT, "include", "ssspy_amd.h")).read()
    for name in ("AUTO", "FFT", "DIRECT"):
        value = int(re.search(r"SSSPY_HVA_ROUTE_{} = (\d+)".format(name), text).group(1))
        assert getattr(_lib, "HVA_ROUTE_" + name) == value
    assert int(re.search(r"#define SSSPY_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 11
