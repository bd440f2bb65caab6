"""What of MaskingADMMHVA needs no device: the constructor against the reference's signature (the
table below), ``repr`` strings (tests/golden/admmhva_repr.npz), the host ``mask_fn`` against the NumPy
restatement of the mask, which ``flooring_fn`` takes the device route (the answers of MaskingPDSHVA),
the refusal of a single bin, the exports and the two entry points in header, binding and library."""

import functools
import inspect
import os
import re

import numpy as np
import pytest

import admmhva_cases as ac
import admmhva_numpy as an
import hva_cases as hc
import hva_numpy as hn
from conftest import ROOT, load_golden, rel_err

# inspect.signature of the reference's MaskingADMMHVA.__init__ (ssspy/bss/hva.py:185-201), without
# ``self``: (name, default); flooring_fn's default is partial(max_flooring, eps=1e-10)
SIGNATURE = [("rho", 1), ("alpha", None), ("relaxation", 1), ("attenuation", None), ("mask_iter", 1),
             ("flooring_fn", "partial(max_flooring, eps=1e-10)"), ("callbacks", None),
             ("scale_restoration", True), ("record_loss", None), ("reference_id", 0)]
ENTRY_POINTS = {"ssspy_hva_admm_cepstrum": 17, "ssspy_hva_aux_step": 13}


def _hva():
    from ssspy_amd.bss import hva

    return hva


def test_constructor_signature_is_the_references():
    cls = _hva().MaskingADMMHVA
    params = inspect.signature(cls.__init__).parameters
    assert list(params)[0] == "self"
    got = []
    for name, p in list(params.items())[1:]:
        assert p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
        default = p.default
        if name == "flooring_fn":
            assert isinstance(default, functools.partial) and not default.args
            assert default.func.__name__ == "max_flooring" and default.keywords == {"eps": 1e-10}
            default = "partial(max_flooring, eps=1e-10)"
        got.append((name, default))
    assert got == SIGNATURE
    m = cls()
    assert m.n_penalties == 1 and m.penalty_fn is None and m.loss is None and m.record_loss is None
    assert (m.rho, m.relaxation, m.mask_iter, m.attenuation) == (1, 1, 1, None)
    assert callable(m.mask_fn)
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
    from ssspy_amd.bss.admmbss import MaskingADMMBSS

    assert issubclass(cls, MaskingADMMBSS)


def test_repr_strings_are_the_references():
    want = load_golden("admmhva_repr")
    for classes in (_hva(), an.CLASSES):
        objs = ac.repr_objects(classes)
        assert set(objs) == set(want)
        for key, obj in objs.items():
            assert repr(obj) == str(want[key]), key
    assert str(want["default"]).startswith("MaskingADMMHVA(rho=1, relaxation=1, mask_iter=1")
    # the quirk: attenuation=None is resolved, and stored, at the first evaluation of the mask
    m = _hva().MaskingADMMHVA()
    assert m.attenuation is None and "attenuation" not in repr(m)
    m.mask_fn(hc.repr_probe())
    assert m.attenuation == 1 / 3 and "attenuation=0.3333333333333333" in repr(m)
    assert repr(m) == str(want["default_after_mask"])


@pytest.mark.parametrize("floor", ["max", "add", "none", "lambda"])
def test_host_mask_fn_matches_the_restatement(floor):
    """hva_numpy's mask (pinned against the reference's by tests/golden/hva_mask.npz in
    tests/test_hva_cpu.py) through the DCT-I; the class goes through irfft as the reference does."""
    from ssspy_amd.special import flooring as fl

    for F in hc.MASK_BINS:
        Z = hc.mask_input(F)
        m = _hva().MaskingADMMHVA(attenuation=hc.MASK_ATTENUATION, mask_iter=hc.MASK_ITER,
                                  flooring_fn=hc.flooring_of(floor, fl))
        mask = m.mask_fn(Z)
        want = hn.mask_of(hn.varrho(Z, hc.flooring_of(floor, hn), hc.MASK_ITER), hc.MASK_ATTENUATION)
        assert mask.shape == Z.shape and mask.dtype == np.float64
        assert rel_err(mask, want) < 1e-13
    g = load_golden("hva_mask")  # and the reference's own mask, which does not depend on the solver
    for F in hc.MASK_BINS:
        m = _hva().MaskingADMMHVA(attenuation=float(g["meta_attenuation"]),
                                  mask_iter=int(g["meta_mask_iter"]))
        assert rel_err(m.mask_fn(g["Z_f{}".format(F)]), g["mask_f{}".format(F)]) < 1e-14


def test_device_floor_answers_as_on_maskingpdshva():
    from ssspy_amd.special import flooring as fl

    admm, pds = _hva().MaskingADMMHVA, _hva().MaskingPDSHVA
    partial = functools.partial
    floors = [fl.identity, None, fl.max_flooring, fl.add_flooring, partial(fl.add_flooring, eps=1e-6),
              partial(fl.max_flooring, eps=1e-3), lambda x: np.maximum(x, 1e-10),
              partial(fl.max_flooring, 1e-3), partial(np.maximum, 1e-10)]
    floors += [hc.flooring_of(name, fl) for name in ("max", "add", "none", "lambda")]
    answers = []
    for floor in floors:
        a, p = admm(flooring_fn=floor).device_floor(), pds(flooring_fn=floor).device_floor()
        assert (a is None) == (p is None) and (a is None or tuple(a) == tuple(p))
        answers.append(a is not None)
    assert answers == [True] * 6 + [False] * 3 + [True, True, True, False]
    assert tuple(admm().device_floor()) == tuple(pds().device_floor())
    # one statement of what the two classes share
    shared = _hva().HVAMask
    for name in ("_host_mask", "device_floor", "transform_route", "_resolve_attenuation"):
        assert getattr(admm, name) is getattr(pds, name) is getattr(shared, name)


def test_a_single_bin_is_refused():
    Z = np.ones((2, 1, 5), dtype=complex)
    with pytest.raises(ValueError, match="Invalid number of FFT data points"):
        _hva().MaskingADMMHVA().mask_fn(Z)


def test_exports():
    import ssspy_amd.bss as bss

    hva = _hva()
    assert "MaskingADMMHVA" in bss.__all__ and bss.MaskingADMMHVA is hva.MaskingADMMHVA
    assert hva.__all__ == ["MaskingPDSHVA", "HVA"]  # (pinned by tests/test_hva_cpu.py as well)
    assert bss.admmbss.__all__ == ["ADMMBSS", "MaskingADMMBSS"]


def test_entry_points_in_header_binding_and_library():
    from ssspy_amd import _build, _lib

    text = open(os.path.join(ROOT, "include", "ssspy_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    _build.build()
    lib = _lib.load()
    for name, n_args in ENTRY_POINTS.items():
        m = re.search(r"\bint " + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_lib.PROTOTYPES[name][1])
        assert hasattr(lib, name)
        # each cites the reference lines it replaces
        comment = text[:text.index("int " + name)].rsplit("/*", 1)[1]
        assert "ssspy/bss/admmbss.py:415-442" in comment and "ssspy/bss/hva.py:2" in comment
    assert _lib.ABI_VERSION == 11  # additions only
