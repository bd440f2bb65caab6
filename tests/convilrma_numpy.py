"""Plain NumPy restatement of ILRMA with joint dereverberation as ssspy_amd.bss.ConvGaussILRMA
defines it (Ikeshita et al., WASPAA 2019; the source-wise factorisation of Nakatani et al.,
Interspeech 2020): the statistics, the IP1 sweep and the composition are those of conviva_numpy, the
stacked vector that of wpd_numpy, the source model is the non-partitioned NMF of GaussILRMA.  With
``dtype=numpy.longdouble`` the whole iteration runs in extended precision.

Per mixture, M channels and sources, K taps, delay D, Lb = (K + 1) M, p = domain, basis T (M, F, Kb),
activation V (M, Kb, T), one iteration from Y = W xb:
    TV = T V, T <- floor(T (sum_t V |y|^2 / TV^((p+2)/p) / sum_t V / TV)^(p/(p+2)))
    TV = T V, V <- floor(V (sum_f T |y|^2 / TV^((p+2)/p) / sum_f T / TV)^(p/(p+2)))
    phi_nft = (T V)_nft^(-2/p) (not floored), Sigma_n, G_n = conviva_numpy.statistics(xb_f, phi_nf)
    IP1 on Q = W[f, :, :M], W[f, n] = compose(Q[n], G_n), Y = W xb
    psi_n = floor(sqrt(mean_{f,t} |y_nft|^2)), Y_n /= psi_n, W[:, n, :] /= psi_n, T_n /= psi_n^p
    loss = sum_{n,f} mean_t (|y|^2 / TV^(2/p) + (2/p) log TV) - 2 sum_f log|det Q_f|
A failed pivot is counted and handled as in conviva_numpy.run.
"""

import numpy as np

import conviva_numpy
import wpd_numpy
import wpe_numpy

MAX_FLOOR = conviva_numpy.MAX_FLOOR


def make_factors(shape, n_basis, rng, flooring=MAX_FLOOR):
    """(basis, activation) as the class draws them: floor(rng.random(...)), basis first.  ``shape`` is
    (M, F, T) or (B, M, F, T)."""
    lead, (M, F, T) = tuple(shape[:-3]), shape[-3:]
    basis = wpe_numpy.floor(rng.random(lead + (M, F, n_basis)), flooring)
    activation = wpe_numpy.floor(rng.random(lead + (M, n_basis, T)), flooring)
    return basis, activation


def weights(basis, activation, domain):
    """phi (M, F, T) = (T V)^(-2/p), in the dtype of the factors; 1 / TV at p = 2."""
    real = basis.dtype.type
    TV = basis @ activation
    with np.errstate(divide="ignore"):
        if domain == 2:
            return real(1) / TV
        return TV ** (-real(2) / real(domain))


def update_factors(Y2, basis, activation, domain, flooring):
    """The MM updates of GaussILRMA (no partitioning) on |Y|^2 (M, F, T): new (basis, activation)."""
    real = basis.dtype.type
    p = real(domain)
    expo = p / (p + real(2))
    TV = basis @ activation
    numer = Y2 / TV ** ((p + real(2)) / p)
    num = np.einsum("nkt,nft->nfk", activation, numer)
    den = np.einsum("nkt,nft->nfk", activation, real(1) / TV)
    basis = wpe_numpy.floor(basis * (num / den) ** expo, flooring)
    TV = basis @ activation
    numer = Y2 / TV ** ((p + real(2)) / p)
    num = np.einsum("nfk,nft->nkt", basis, numer)
    den = np.einsum("nfk,nft->nkt", basis, real(1) / TV)
    activation = wpe_numpy.floor(activation * (num / den) ** expo, flooring)
    return basis, activation


def data_term(Y2, basis, activation, domain):
    real = basis.dtype.type
    p = real(domain)
    TV = basis @ activation
    return np.sum(Y2 / TV ** (real(2) / p) + (real(2) / p) * np.log(TV)) / real(Y2.shape[-1])


def run(X, taps, delay, n_basis=None, domain=2, n_iter=3, basis=None, activation=None, rng=None,
        loading=0.0, flooring=MAX_FLOOR, dtype=np.float64, convolutional_filter=None,
        normalization=True, scale_restoration=True, reference_id=0):
    """X (M, F, T) or (B, M, F, T); ``basis`` / ``activation`` given or drawn from ``rng`` by
    make_factors.  Returns ``output``, ``convolutional_filter``, ``demix_filter``,
    ``prediction_filter`` as conviva_numpy.run, ``basis``, ``activation``, ``loss`` (n_iter + 1
    entries, before scale restoration), ``failed`` and ``max_cond``."""
    ctype = conviva_numpy._complex(dtype)
    extended = ctype is np.clongdouble
    X = np.asarray(X)
    batched = X.ndim == 4
    X4 = (X if batched else X[None]).astype(ctype)
    B, M, F, T = X4.shape
    K, L, Lb = taps, taps * M, (taps + 1) * M
    if basis is None or activation is None:
        drawn = make_factors(X.shape, n_basis, rng, flooring)
        basis = drawn[0] if basis is None else basis
        activation = drawn[1] if activation is None else activation
    Tb = np.array(basis, dtype=dtype).reshape((B, M, F, -1))
    Vb = np.array(activation, dtype=dtype).reshape((B, M, -1, T))
    W = np.zeros((B, F, M, Lb), dtype=ctype)
    if convolutional_filter is None:
        W[:, :, :, :M] = np.eye(M, dtype=ctype)
    else:
        W[...] = np.asarray(convolutional_filter).reshape(B, F, M, Lb)
    G = np.zeros((B, F, M, L, M), dtype=ctype)
    Sigma = np.tile(np.eye(M, dtype=ctype), (B, F, M, 1, 1))
    Y = np.zeros((B, M, F, T), dtype=ctype)
    loss = np.zeros((n_iter + 1, B), dtype=dtype)
    ever_failed = np.zeros((B, F, M), dtype=bool)
    max_cond = 0.0
    for b in range(B):
        xb = [wpd_numpy.stack(X4[b, :, f, :], K, delay) for f in range(F)]

        def separate():
            for f in range(F):
                Y[b, :, f, :] = W[b, f] @ xb[f]
            return Y[b].real ** 2 + Y[b].imag ** 2

        def current_loss(Y2):
            logdet = sum(conviva_numpy.logabsdet(W[b, f, :, :M]) for f in range(F))
            return data_term(Y2, Tb[b], Vb[b], domain) - 2 * logdet

        Y2 = separate()
        for it in range(n_iter):
            loss[it, b] = current_loss(Y2)
            Tb[b], Vb[b] = update_factors(Y2, Tb[b], Vb[b], domain, flooring)
            phi = weights(Tb[b], Vb[b], domain)
            for f in range(F):
                failed_now = np.zeros(M, dtype=bool)
                for n in range(M):
                    try:
                        Sigma[b, f, n], G[b, f, n], st = conviva_numpy.statistics(
                            xb[f], phi[n, f], M, loading, extended)
                        max_cond = max(max_cond, st["cond"])
                    except np.linalg.LinAlgError:
                        failed_now[n] = ever_failed[b, f, n] = True
                Q = conviva_numpy.ip1_sweep(W[b, f, :, :M], Sigma[b, f], flooring, extended)
                for n in range(M):
                    if not failed_now[n]:
                        W[b, f, n] = conviva_numpy.compose(Q[n], G[b, f, n])
            Y2 = separate()
            if normalization:
                psi = wpe_numpy.floor(np.sqrt(np.mean(Y2, axis=(1, 2))), flooring)
                W[b] /= psi[None, :, None]
                Y[b] /= psi[:, None, None]
                Tb[b] /= (psi ** dtype(domain))[:, None, None]
                Y2 = Y[b].real ** 2 + Y[b].imag ** 2
        loss[n_iter, b] = current_loss(Y2)
        if scale_restoration:
            for f in range(F):
                Q = W[b, f, :, :M]
                if extended:
                    scale = np.array([conviva_numpy.solve_vector(Q, np.eye(M, dtype=ctype)[n])[
                        reference_id] for n in range(M)])
                else:
                    scale = np.linalg.inv(Q)[reference_id, :]
                for n in range(M):
                    W[b, f, n] = conviva_numpy.compose(Q[n] * scale[n], G[b, f, n])
            separate()
    result = {"output": Y, "convolutional_filter": W.reshape(B, F, M, K + 1, M),
              "demix_filter": W[..., :M].copy(), "prediction_filter": G.reshape(B, F, M, K, M, M),
              "basis": Tb, "activation": Vb}
    if not batched:
        result = {k: v[0] for k, v in result.items()}
    result["loss"] = [row.copy() if batched else row[0] for row in loss]
    result["failed"] = int(ever_failed.sum())
    result["max_cond"] = max_cond
    return result
