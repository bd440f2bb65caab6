"""NumPy restatement of the gradient / natural-gradient IVA classes of the reference
(ssspy/bss/iva.py:284-406, :644-988, :2341-2973), with its expression structure: the estimate is
formed, the score applied to it, PhiY = mean_j phi(y) y^H, the step, the estimate again.

A test helper: the product never imports it.  Single mixtures only, (n_channels, n_bins, n_frames).
"""

import functools

import numpy as np

from oracle import spatial as sp

EPS = 1e-10


def max_flooring(x, eps=EPS):
    return np.maximum(x, eps)


def add_flooring(x, eps=EPS):
    return x + eps


def identity(x):
    return x


class GradIVABase:
    natural = False

    def __init__(self, step_size=1e-1, contrast_fn=None, score_fn=None,
                 flooring_fn=functools.partial(max_flooring, eps=EPS), callbacks=None,
                 is_holonomic=False, scale_restoration=True, record_loss=True, reference_id=0):
        if contrast_fn is None:
            raise ValueError("Specify contrast function.")
        if score_fn is None:
            raise ValueError("Specify score function.")
        self.step_size, self.contrast_fn, self.score_fn = step_size, contrast_fn, score_fn
        self.flooring_fn = identity if flooring_fn is None else flooring_fn
        self.callbacks = [callbacks] if callable(callbacks) else callbacks
        self.is_holonomic, self.scale_restoration = is_holonomic, scale_restoration
        self.record_loss, self.reference_id = record_loss, reference_id
        self.loss = [] if record_loss else None

    def _reset(self, **kwargs):
        for key, value in kwargs.items():
            setattr(self, key, value)
        N, F, T = self.input.shape
        self.n_sources, self.n_channels, self.n_bins, self.n_frames = N, N, F, T
        if not hasattr(self, "demix_filter"):
            self.demix_filter = np.tile(np.eye(N, dtype=np.complex128), (F, 1, 1))
        else:
            self.demix_filter = self.demix_filter.copy()
        self.output = sp.separate(self.input, self.demix_filter)

    def _after_step(self):
        if self.record_loss:
            self.loss.append(self.compute_loss())
        for hook in self.callbacks or ():
            hook(self)

    def __call__(self, input, n_iter=100, initial_call=True, **kwargs):
        self.input = input.copy()
        self._reset(**kwargs)
        if initial_call:
            self._after_step()
        for _ in range(n_iter):
            self.update_once()
            self._after_step()
        if self.scale_restoration:
            self.restore_scale()
        self.output = sp.separate(self.input, self.demix_filter)
        return self.output

    def update_once(self):
        X, W = self.input, self.demix_filter
        Y = sp.separate(X, W)
        Phi = self.score_fn(Y)
        PhiY = np.mean(Phi[:, np.newaxis, :, :] * Y.conj()[np.newaxis, :, :, :], axis=-1)
        PhiY = PhiY.transpose(2, 0, 1)  # (n_bins, n_sources, n_sources)
        eye = np.eye(self.n_sources)
        D = PhiY - eye if self.is_holonomic else (1 - eye) * PhiY
        if self.natural:
            delta = D @ W
        else:
            delta = D @ np.linalg.inv(W).transpose(0, 2, 1).conj()
        W = W - self.step_size * delta
        self.demix_filter, self.output = W, sp.separate(X, W)

    def compute_loss(self):
        Y = sp.separate(self.input, self.demix_filter)
        G = self.contrast_fn(Y)
        loss = np.sum(np.mean(G, axis=1), axis=0) - 2 * np.sum(sp.logdet(self.demix_filter), axis=0)
        return loss.item()

    def restore_scale(self):
        kind = self.scale_restoration
        if type(kind) is bool:
            kind = "projection_back"
        X, W = self.input, self.demix_filter
        if kind == "projection_back":
            W = sp.projection_back_filter(W, reference_id=self.reference_id)
            self.output, self.demix_filter = sp.separate(X, W), W
        elif kind == "minimal_distortion_principle":
            Y = sp.minimal_distortion_output(sp.separate(X, W), X, reference_id=self.reference_id)
            self.output, self.demix_filter = Y, sp.demix_from_output(Y, X)
        else:
            raise ValueError("{} is not supported for scale restoration.".format(kind))


class GradIVA(GradIVABase):
    def __init__(self, *args, is_holonomic=True, **kwargs):
        super().__init__(*args, is_holonomic=is_holonomic, **kwargs)


class NaturalGradIVA(GradIVA):
    natural = True


def _laplace(self):
    def contrast_fn(y):
        return 2 * np.linalg.norm(y, axis=1)

    def score_fn(y):
        norm = np.linalg.norm(y, axis=1, keepdims=True)
        return y / self.flooring_fn(norm)

    return dict(contrast_fn=contrast_fn, score_fn=score_fn)


def _gauss(self):
    def contrast_fn(y):
        norm = np.linalg.norm(y, axis=1)
        return self.n_bins * np.log(self.variance) + (norm**2) / self.variance

    def score_fn(y):
        return y / self.variance[:, np.newaxis, :]

    return dict(contrast_fn=contrast_fn, score_fn=score_fn)


class _Gauss:
    def _reset(self, **kwargs):
        super()._reset(**kwargs)
        self.variance = np.ones((self.n_sources, self.n_frames))

    def update_once(self):
        self.update_source_model()
        super().update_once()

    def update_source_model(self):
        Y = sp.separate(self.input, self.demix_filter)
        self.variance = np.mean(np.abs(Y) ** 2, axis=1)


class GradLaplaceIVA(GradIVA):
    def __init__(self, step_size=1e-1, **kwargs):
        super().__init__(step_size=step_size, **_laplace(self), **kwargs)


class NaturalGradLaplaceIVA(NaturalGradIVA):
    def __init__(self, step_size=1e-1, **kwargs):
        super().__init__(step_size=step_size, **_laplace(self), **kwargs)


class GradGaussIVA(_Gauss, GradIVA):
    def __init__(self, step_size=1e-1, **kwargs):
        super().__init__(step_size=step_size, **_gauss(self), **kwargs)


class NaturalGradGaussIVA(_Gauss, NaturalGradIVA):
    def __init__(self, step_size=1e-1, **kwargs):
        super().__init__(step_size=step_size, **_gauss(self), **kwargs)


CLASSES = {cls.__name__: cls for cls in (GradIVA, NaturalGradIVA, GradLaplaceIVA, GradGaussIVA,
                                         NaturalGradLaplaceIVA, NaturalGradGaussIVA)}
