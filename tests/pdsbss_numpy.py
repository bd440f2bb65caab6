"""NumPy restatement of the proximal operators and of ProxBSSBase / PDSBSSBase / PDSBSS /
MaskingPDSBSS, written for this project: the oracle of the GPU tests on shapes no fixture has.
tests/test_golden_pdsbss.py pins it against the fixtures generated from the reference."""

import warnings

import numpy as np


# ---- proximal operators
def _shrink(norm, step_size):
    norm = np.where(norm < step_size, step_size, norm)
    return np.maximum(1 - step_size / norm, 0)


def l1(x, step_size=1):
    return _shrink(np.abs(x), step_size) * x


def l21(x, step_size=1, axis1=-2, axis2=-1):
    return _shrink(np.sqrt(np.sum(np.abs(x) ** 2, axis=axis2, keepdims=True)), step_size) * x


def neg_log(x, step_size=1):
    assert np.all(x >= 0)
    return (x + np.sqrt(x**2 + 4 * step_size)) / 2


def neg_logdet(X, step_size=1):
    U, s, Vh = np.linalg.svd(X)
    return (U * neg_log(s, step_size)[..., None, :]) @ Vh


# ---- scale restoration
def _projection_back(W, reference_id):
    A = np.linalg.inv(W)  # (F, N, N)
    return A[:, reference_id, :, None] * W


def _mdp_output(Y, X, reference_id):
    ref = X[reference_id]  # (F, T)
    num = np.sum(Y.conj() * ref, axis=-1)
    den = np.sum(np.abs(Y) ** 2, axis=-1)
    return (num / den)[..., None] * Y


def _apply(W, X):
    return np.einsum("fnm,mft->nft", W, X)


class ProxBSSBase:
    def __init__(self, penalty_fn=None, prox_penalty=None, callbacks=None, scale_restoration=True,
                 record_loss=None, reference_id=0):
        self.callbacks = [callbacks] if callable(callbacks) else callbacks
        self.record_loss = record_loss  # (None stays None: no loss is recorded then)
        self.loss = [] if record_loss else None
        if penalty_fn is None:
            assert not record_loss, "To record loss, set penalty_fn."
        elif callable(penalty_fn):
            penalty_fn = [penalty_fn]
        if prox_penalty is None:
            raise ValueError("Specify proximal operator of penalty function.")
        if callable(prox_penalty):
            prox_penalty = [prox_penalty]
        self.penalty_fn, self.prox_penalty = penalty_fn, prox_penalty
        if penalty_fn is not None:
            assert len(penalty_fn) == len(prox_penalty), \
                "Length of penalty_fn and prox_penalty are different."
        self._init_scale(scale_restoration, reference_id)

    def _init_scale(self, scale_restoration, reference_id):
        self.input = None
        self.scale_restoration = scale_restoration
        if reference_id is None and scale_restoration:
            raise ValueError("Specify 'reference_id' if scale_restoration=True.")
        self.reference_id = reference_id

    @property
    def n_penalties(self):
        return len(self.prox_penalty)

    def _repr(self, name, head=""):
        s = name + "(" + head
        if name != "MaskingPDSBSS":
            s += "{}n_penalties={}".format(", " if head else "", self.n_penalties)
        s += ", scale_restoration={}, record_loss={}".format(self.scale_restoration, self.record_loss)
        if self.scale_restoration:
            s += ", reference_id={}".format(self.reference_id)
        return s + ")"

    def __repr__(self):
        return self._repr("ProxBSSBase")

    def _reset(self, **kwargs):
        assert self.input is not None, "Specify data!"
        for key, value in kwargs.items():
            setattr(self, key, value)
        N, F, T = self.input.shape
        self.n_sources = self.n_channels = N
        self.n_bins, self.n_frames = F, T
        if not hasattr(self, "demix_filter"):
            self.demix_filter = np.tile(np.eye(N, dtype=np.complex128), (F, 1, 1))
        else:
            self.demix_filter = np.array(self.demix_filter, dtype=np.complex128)
        self.output = self.separate(self.input, self.demix_filter)

    def separate(self, input, demix_filter):
        return _apply(demix_filter, input)

    def _penalty_fns(self):
        return self.penalty_fn

    def compute_loss(self):
        Y = self.separate(self.input, self.demix_filter)
        penalty = sum(fn(Y) for fn in self._penalty_fns())
        return float(penalty - np.sum(self.compute_logdet(self.demix_filter)))

    def compute_logdet(self, demix_filter):
        return np.linalg.slogdet(demix_filter)[1]

    def normalize_by_spectral_norm(self, input, n_penalties=None):
        if n_penalties is None:
            n_penalties = self.n_penalties
        norms = np.linalg.svd(input.transpose(1, 0, 2), compute_uv=False)[:, 0]
        return input / (np.sqrt(n_penalties) * np.max(norms))

    def _after_step(self):
        if self.record_loss:
            self.loss.append(self.compute_loss())
        for hook in self.callbacks or ():
            hook(self)

    def _iterate(self, n_iter, initial_call):
        if initial_call:
            self._after_step()
        for _ in range(n_iter):
            self.update_once()
            self._after_step()

    def restore_scale(self):
        how = self.scale_restoration
        assert how, "Set self.scale_restoration=True."
        if type(how) is bool:
            how = "projection_back"
        X, W = self.input, self.demix_filter
        if how == "projection_back":
            W = _projection_back(W, self.reference_id)
            Y = self.separate(X, W)
        elif how == "minimal_distortion_principle":
            Y = _mdp_output(self.separate(X, W), X, self.reference_id)
            Xf, Yf = X.transpose(1, 0, 2), Y.transpose(1, 0, 2)
            XH = Xf.transpose(0, 2, 1).conj()
            W = Yf @ XH @ np.linalg.inv(Xf @ XH)
        else:
            raise ValueError("{} is not supported for scale restoration.".format(how))
        self.output, self.demix_filter = Y, W


class PDSBSSBase(ProxBSSBase):
    _dual_rank = 4  # (Q, N, F, T)

    def __repr__(self):
        return self._repr("PDSBSS")

    def _init_steps(self, mu1, mu2, alpha, relaxation):
        self.mu1, self.mu2 = mu1, mu2
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
        super()._reset(**kwargs)
        N, F, T = self.input.shape
        shape = (self.n_penalties, N, F, T) if self._dual_rank == 4 else (N, F, T)
        if not hasattr(self, "dual"):
            self.dual = np.zeros(shape, dtype=np.complex128)
        else:
            self.dual = np.array(self.dual, dtype=np.complex128)

    def _filter_step(self, dual_sum):
        """(Wt, the separated signal of the filter 2 Wt - W)."""
        X, W = self.input, self.demix_filter
        XY = np.einsum("nft,mft->fnm", dual_sum, X.conj())
        Wt = neg_logdet(W - self.mu1 * self.mu2 * XY, step_size=self.mu1)
        return Wt, _apply(2 * Wt - W, X)

    def _relax(self, Wt, Yt):
        a = self.relaxation
        self.demix_filter = a * Wt + (1 - a) * self.demix_filter
        self.dual = a * Yt + (1 - a) * self.dual


class PDSBSS(PDSBSSBase):
    def __init__(self, mu1=1, mu2=1, alpha=None, relaxation=1, penalty_fn=None, prox_penalty=None,
                 callbacks=None, scale_restoration=True, record_loss=None, reference_id=0):
        super().__init__(penalty_fn=penalty_fn, prox_penalty=prox_penalty, callbacks=callbacks,
                         scale_restoration=scale_restoration, record_loss=record_loss,
                         reference_id=reference_id)
        self._init_steps(mu1, mu2, alpha, relaxation)

    def __repr__(self):
        return self._repr("PDSBSS", "mu1={}, mu2={}, relaxation={}".format(
            self.mu1, self.mu2, self.relaxation))

    def update_once(self):
        Wt, XW = self._filter_step(self.dual.sum(axis=0))
        Yt = []
        for dual_q, prox_q in zip(self.dual, self.prox_penalty):
            Z = dual_q + XW
            Yt.append(Z - prox_q(Z, step_size=1 / self.mu2))
        self._relax(Wt, np.stack(Yt))


class MaskingPDSBSS(PDSBSSBase):
    _dual_rank = 3  # (N, F, T)

    def __init__(self, mu1=1, mu2=1, alpha=None, relaxation=1, penalty_fn=None, mask_fn=None,
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
        self._init_steps(mu1, mu2, alpha, relaxation)

    @property
    def n_penalties(self):
        return 1

    def _penalty_fns(self):
        return [self.penalty_fn]

    def __repr__(self):
        return self._repr("MaskingPDSBSS", "mu1={}, mu2={}, relaxation={}".format(
            self.mu1, self.mu2, self.relaxation))

    def update_once(self):
        Wt, XW = self._filter_step(self.dual)
        Z = self.dual + XW
        self._relax(Wt, Z - self.mask_fn(Z) * Z)


CLASSES = {cls.__name__: cls for cls in (ProxBSSBase, PDSBSSBase, PDSBSS, MaskingPDSBSS)}
