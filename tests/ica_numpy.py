"""NumPy restatement of the time-domain ICA classes, written from the formulas:

    y_t = W x_t,  PhiY = (1/T) sum_t phi(y_t) y_t^T,  D = PhiY - I (holonomic) or offdiag(PhiY)
    GradICA:         W <- W - eta D W^-T          loss = sum_n mean_t G(y_tn) - log|det W|
    NaturalGradICA:  W <- W - eta D W
    FastICA (on z = Lambda^-1/2 Gamma^T x):  for n in order
        w <- mean_t phi'(y_tn) w_n - mean_t phi(y_tn) z_t,  w <- w - sum_{q<n} (w_q . w) w_q,
        w_n <- w / |w|                             loss = sum_n mean_t G(y_tn)

Pinned against the reference by tests/test_golden_ica.py; the GPU tests compare the device classes
with it where no golden vector exists.  float64 throughout; no device, no library.
"""

import numpy as np


def whiten(x):
    """z = Lambda^-1/2 Gamma^T x, mean_t x x^T = Gamma Lambda Gamma^T (eigenvalues ascending)."""
    covariance = x @ x.T / x.shape[-1]
    lam, gamma = np.linalg.eigh(covariance)
    return (gamma.T / np.sqrt(lam)[:, None]) @ x


class _Iterative:
    def __init__(self, callbacks=None, record_loss=True):
        self.callbacks = [callbacks] if callable(callbacks) else callbacks
        self.record_loss = record_loss
        self.loss = [] if record_loss else None

    def _tail(self):
        if self.record_loss:
            self.loss.append(self.compute_loss())
        for hook in self.callbacks or ():
            hook(self)

    def _iterate(self, n_iter, initial_call):
        if initial_call:
            self._tail()
        for _ in range(n_iter):
            self.update_once()
            self._tail()

    def _start(self, input, kwargs):
        self.input = np.array(input, dtype=np.float64)
        for key, value in kwargs.items():
            setattr(self, key, value)
        N, T = self.input.shape
        self.n_sources = self.n_channels = N
        self.n_samples = T
        if hasattr(self, "demix_filter"):
            self.demix_filter = np.array(self.demix_filter, dtype=np.float64)
        else:
            self.demix_filter = np.eye(N)


class _Grad(_Iterative):
    natural = False

    def __init__(self, step_size=1e-1, contrast_fn=None, score_fn=None, callbacks=None,
                 is_holonomic=False, record_loss=True):
        super().__init__(callbacks, record_loss)
        self.step_size, self.is_holonomic = step_size, is_holonomic
        self.contrast_fn, self.score_fn = contrast_fn, score_fn

    def __call__(self, input, n_iter=100, initial_call=True, **kwargs):
        self._start(input, kwargs)
        self._iterate(n_iter, initial_call)
        self.output = self.demix_filter @ self.input
        return self.output

    def compute_loss(self):
        Y = self.demix_filter @ self.input
        data = sum(np.mean(row) for row in self.contrast_fn(Y))
        return float(data - np.log(np.abs(np.linalg.det(self.demix_filter))))

    def update_once(self):
        W, X = self.demix_filter, self.input
        Y = W @ X
        PhiY = self.score_fn(Y) @ Y.T / self.n_samples
        if self.is_holonomic:
            D = PhiY - np.eye(self.n_sources)
        else:
            D = PhiY - np.diag(np.diag(PhiY))
        if self.natural:
            delta = D @ W
        else:
            delta = np.linalg.solve(W, D.T).T  # D W^-T
        self.demix_filter = W - self.step_size * delta


class GradICA(_Grad):
    pass


class NaturalGradICA(_Grad):
    natural = True


def _laplace(cls):
    class Laplace(cls):
        def __init__(self, step_size=1e-1, callbacks=None, is_holonomic=False, record_loss=True):
            super().__init__(step_size=step_size, contrast_fn=np.abs, score_fn=np.sign,
                             callbacks=callbacks, is_holonomic=is_holonomic,
                             record_loss=record_loss)
    return Laplace


GradLaplaceICA = _laplace(GradICA)
NaturalGradLaplaceICA = _laplace(NaturalGradICA)


class FastICA(_Iterative):
    def __init__(self, contrast_fn=None, score_fn=None, d_score_fn=None, callbacks=None,
                 record_loss=True):
        super().__init__(callbacks, record_loss)
        self.contrast_fn, self.score_fn, self.d_score_fn = contrast_fn, score_fn, d_score_fn

    def __call__(self, input, n_iter=100, initial_call=True, **kwargs):
        self._start(input, kwargs)
        self.whitened_input = whiten(self.input)
        self._iterate(n_iter, initial_call)
        self.output = self.demix_filter @ self.whitened_input
        return self.output

    def compute_loss(self):
        Y = self.demix_filter @ self.whitened_input
        return float(sum(np.mean(row) for row in self.contrast_fn(Y)))

    def update_once(self):
        Z, W_old = self.whitened_input, self.demix_filter
        W = np.zeros_like(W_old)
        for n in range(self.n_sources):
            y = W_old[n] @ Z
            w = np.mean(self.d_score_fn(y)) * W_old[n] - Z @ self.score_fn(y) / self.n_samples
            w = w - W[:n].T @ (W[:n] @ w)
            with np.errstate(invalid="ignore", divide="ignore"):
                W[n] = w / np.sqrt(w @ w)
        self.demix_filter = W


CLASSES = {"GradICA": GradICA, "NaturalGradICA": NaturalGradICA, "FastICA": FastICA,
           "GradLaplaceICA": GradLaplaceICA, "NaturalGradLaplaceICA": NaturalGradLaplaceICA}
