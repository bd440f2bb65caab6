"""NumPy restatement of MaskingADMMHVA, written for this project: the ADMM iteration of
tests/admmbss_numpy.py (``MaskingADMMBSS``) carrying the mask of tests/hva_numpy.py (``varrho`` by the
DCT-I, ``mask_of``).  The oracle of the GPU tests on shapes no fixture has;
tests/test_golden_admmhva.py pins it against the fixtures generated from the reference."""

import functools

import admmbss_numpy as an
import hva_numpy as hn
from hva_numpy import EPS, add_flooring, identity, max_flooring  # noqa: F401  (a flooring namespace)


class MaskingADMMHVA(an.MaskingADMMBSS):
    def __init__(self, rho=1, alpha=None, relaxation=1, attenuation=None, mask_iter=1,
                 flooring_fn=functools.partial(max_flooring, eps=EPS), callbacks=None,
                 scale_restoration=True, record_loss=None, reference_id=0):
        super().__init__(rho=rho, alpha=alpha, relaxation=relaxation, penalty_fn=None,
                         mask_fn=self._mask, callbacks=callbacks,
                         scale_restoration=scale_restoration, record_loss=record_loss,
                         reference_id=reference_id)
        self.attenuation, self.mask_iter = attenuation, mask_iter
        self.flooring_fn = identity if flooring_fn is None else flooring_fn

    def _mask(self, y):
        if self.attenuation is None:
            self.attenuation = 1 / y.shape[0]
        return hn.mask_of(hn.varrho(y, self.flooring_fn, self.mask_iter), self.attenuation)

    def __repr__(self):
        s = "MaskingADMMHVA(rho={}, relaxation={}".format(self.rho, self.relaxation)
        if self.attenuation is not None:
            s += ", attenuation={}".format(self.attenuation)
        s += ", mask_iter={}, scale_restoration={}, record_loss={}".format(
            self.mask_iter, self.scale_restoration, self.record_loss)
        if self.scale_restoration:
            s += ", reference_id={}".format(self.reference_id)
        return s + ")"


CLASSES = {"MaskingADMMHVA": MaskingADMMHVA}
