"""NumPy restatement of ADMMBSSBase / ADMMBSS / MaskingADMMBSS and of the PDSIVA / ADMMIVA front
ends, written for this project from the equations on top of tests/pdsbss_numpy.py: the oracle of the
GPU tests on shapes no fixture has.  tests/test_golden_admmbss.py pins it against the fixtures
generated from the reference.

One iteration, per bin i with the frames of X_i (N, T) in its columns and Q penalties:
    A_i = Q conj(X_i) X_i^T + I,  R_i = (sum_q (V2_q - Y2_q))_i X_i^H
    W_i = A_i^-1 (V1_i - Y1_i + R_i)
    U1 = a W + (1 - a) V1,  V1 <- prox_{-log|det| / rho}(U1 + Y1),  Y1 <- Y1 + U1 - V1
    U2_q = a W x + (1 - a) V2_q,  V2_q <- prox_q(U2_q + Y2_q, 1 / rho),  Y2_q <- Y2_q + U2_q - V2_q
with V1 / Y1 = auxiliary1 / dual1, V2 / Y2 = auxiliary2 / dual2 and a the relaxation."""

import functools
import warnings

import numpy as np

import pdsbss_numpy as pn
from pdsbss_numpy import l1, l21, neg_logdet  # noqa: F401  (a prox namespace like pdsbss_numpy)


class ADMMBSSBase(pn.ProxBSSBase):
    _aux2_rank = 4  # (Q, N, F, T)

    def __repr__(self):
        return self._repr("ADMMBSS")

    def _init_steps(self, rho, alpha, relaxation):
        self.rho = rho
        if alpha is None:
            self.relaxation = relaxation
        else:
            assert relaxation == 1, "You cannot specify relaxation and alpha simultaneously."
            warnings.warn("alpha is deprecated. Set relaxation instead.", DeprecationWarning)
            self.relaxation = alpha

    def __call__(self, input, n_iter=100, initial_call=True, **kwargs):
        self.input = np.array(input)
        self._reset(**kwargs)
        self._iterate(n_iter, initial_call)
        if self.scale_restoration:
            self.restore_scale()
        self.output = self.separate(self.input, self.demix_filter)
        return self.output

    def _reset(self, **kwargs):
        for old, new in (("aux1", "auxiliary1"), ("aux2", "auxiliary2")):
            if old in kwargs:
                warnings.warn("{} is deprecated. Use {} instead.".format(old, new),
                              DeprecationWarning)
                kwargs[new] = kwargs.pop(old)
        super()._reset(**kwargs)
        N, F, T = self.input.shape
        big = (self.n_penalties, N, F, T) if self._aux2_rank == 4 else (N, F, T)
        for name, shape in (("auxiliary1", (F, N, N)), ("dual1", (F, N, N)), ("auxiliary2", big),
                            ("dual2", big)):
            if not hasattr(self, name):
                setattr(self, name, np.zeros(shape, dtype=np.complex128))
            else:
                setattr(self, name, np.array(getattr(self, name), dtype=np.complex128))

    def _filter_step(self, difference):
        """``difference``: sum_q (auxiliary2_q - dual2_q), (N, F, T).  Updates demix_filter,
        auxiliary1 and dual1; returns the relaxed separated signal without its auxiliary2 share,
        a W x (N, F, T)."""
        X, a = self.input, self.relaxation
        N = X.shape[0]
        A = self.n_penalties * np.einsum("mft,kft->fmk", X.conj(), X) + np.eye(N)
        R = np.einsum("nft,mft->fnm", difference, X.conj())
        W = np.linalg.solve(A, self.auxiliary1 - self.dual1 + R)
        U = a * W + (1 - a) * self.auxiliary1
        V = neg_logdet(U + self.dual1, step_size=1 / self.rho)
        self.dual1 = self.dual1 + U - V
        self.auxiliary1, self.demix_filter = V, W
        return a * pn._apply(W, X)


class ADMMBSS(ADMMBSSBase):
    def __init__(self, rho=1, alpha=None, relaxation=1, penalty_fn=None, prox_penalty=None,
                 callbacks=None, scale_restoration=True, record_loss=True, reference_id=0):
        super().__init__(penalty_fn=penalty_fn, prox_penalty=prox_penalty, callbacks=callbacks,
                         scale_restoration=scale_restoration, record_loss=record_loss,
                         reference_id=reference_id)
        self._init_steps(rho, alpha, relaxation)

    def __repr__(self):
        return self._repr("ADMMBSS", "rho={}, relaxation={}".format(self.rho, self.relaxation))

    def update_once(self):
        aXW = self._filter_step(np.sum(self.auxiliary2 - self.dual2, axis=0))
        V2, Y2 = [], []
        for v, y, prox_q in zip(self.auxiliary2, self.dual2, self.prox_penalty):
            Z = aXW + (1 - self.relaxation) * v + y
            V2.append(prox_q(Z, step_size=1 / self.rho))
            Y2.append(Z - V2[-1])
        self.auxiliary2, self.dual2 = np.stack(V2), np.stack(Y2)


class MaskingADMMBSS(ADMMBSSBase):
    _aux2_rank = 3  # (N, F, T)

    def __init__(self, rho=1, alpha=None, relaxation=1, penalty_fn=None, mask_fn=None,
                 callbacks=None, scale_restoration=True, record_loss=None, reference_id=0):
        self.callbacks = [callbacks] if callable(callbacks) else callbacks
        self.record_loss = record_loss
        self.loss = [] if record_loss else None
        if penalty_fn is None:
            assert not record_loss, "To record loss, set penalty_fn."
        else:
            assert callable(penalty_fn), "penalty_fn should be callable."
        if mask_fn is None:
            raise ValueError("Specify masking function.")
        assert callable(mask_fn), "mask_fn should be callable."
        self.penalty_fn, self.mask_fn = penalty_fn, mask_fn
        self._init_scale(scale_restoration, reference_id)
        self._init_steps(rho, alpha, relaxation)

    @property
    def n_penalties(self):
        return 1

    def _penalty_fns(self):
        return [self.penalty_fn]

    def update_once(self):
        aXW = self._filter_step(self.auxiliary2 - self.dual2)
        Z = aXW + (1 - self.relaxation) * self.auxiliary2 + self.dual2
        self.auxiliary2 = self.mask_fn(Z) * Z
        self.dual2 = Z - self.auxiliary2


def _vector_penalty(contrast_fn, prox_penalty):
    if contrast_fn is not None and prox_penalty is None:
        raise ValueError("Set prox_penalty.")
    if contrast_fn is None and prox_penalty is not None:
        raise ValueError("Set contrast_fn.")
    if contrast_fn is None:
        contrast_fn = functools.partial(np.linalg.norm, axis=1)
        prox_penalty = functools.partial(l21, axis2=1)
    return contrast_fn, prox_penalty, lambda y: float(np.sum(contrast_fn(y)))


class PDSIVA(pn.PDSBSS):
    def __init__(self, mu1=1, mu2=1, alpha=None, relaxation=1, contrast_fn=None, prox_penalty=None,
                 callbacks=None, scale_restoration=True, record_loss=True, reference_id=0):
        contrast_fn, prox_penalty, penalty_fn = _vector_penalty(contrast_fn, prox_penalty)
        super().__init__(mu1=mu1, mu2=mu2, alpha=alpha, relaxation=relaxation, penalty_fn=penalty_fn,
                         prox_penalty=prox_penalty, callbacks=callbacks,
                         scale_restoration=scale_restoration, record_loss=record_loss,
                         reference_id=reference_id)
        self.contrast_fn = contrast_fn


class ADMMIVA(ADMMBSS):
    def __init__(self, rho=1, alpha=None, relaxation=1, contrast_fn=None, prox_penalty=None,
                 callbacks=None, scale_restoration=True, record_loss=True, reference_id=0):
        contrast_fn, prox_penalty, penalty_fn = _vector_penalty(contrast_fn, prox_penalty)
        super().__init__(rho=rho, alpha=alpha, relaxation=relaxation, penalty_fn=penalty_fn,
                         prox_penalty=prox_penalty, callbacks=callbacks,
                         scale_restoration=scale_restoration, record_loss=record_loss,
                         reference_id=reference_id)
        self.contrast_fn = contrast_fn


CLASSES = {cls.__name__: cls for cls in (ADMMBSSBase, ADMMBSS, MaskingADMMBSS, PDSIVA, ADMMIVA)}
