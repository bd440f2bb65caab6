"""Shared generators of the WPE tests: reverberant test mixtures and the shape list."""

import numpy as np

# (n_channels, taps, delay, n_bins, n_frames, n_mixtures)
CASES = (
    (1, 1, 1, 1, 8, 1),
    (2, 3, 1, 3, 40, 1),
    (3, 5, 3, 2, 97, 2),      # odd order L = 15
    (4, 10, 3, 3, 257, 1),    # n_frames is one past a tile of 256
    (8, 8, 2, 2, 300, 1),     # L = 64, the limit
    (2, 16, 3, 2, 1700, 1),   # 2 * (1700 + 15) * 16 bytes > 48 KiB: the slab is re-read, not resident
)
SMALL = CASES[:3]
MA_ORDER = 7


def case_id(case):
    return "M{}-K{}-D{}-F{}-T{}-B{}".format(*case)


def make_mixture(case, seed=0):
    """An M-channel moving-average process per bin, x_t = sum_{k < 7} A_k s_{t - k} + 1e-2 n_t, with
    A_k random (M, M) decaying like 0.6^k, scaled to RMS 1 before the noise that keeps R well
    conditioned.  (M, F, T), or (B, M, F, T) when B > 1."""
    M, _, _, F, T, B = case
    rng = np.random.default_rng([seed, M, F, T, B])

    def cnormal(shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)

    A = cnormal((B, F, MA_ORDER, M, M)) * (0.6 ** np.arange(MA_ORDER))[None, None, :, None, None]
    s = cnormal((B, F, M, T + MA_ORDER - 1))
    X = np.zeros((B, M, F, T), dtype=np.complex128)
    for k in range(MA_ORDER):
        # s_{t - k}: column t + MA_ORDER - 1 - k of the padded source
        seg = s[:, :, :, MA_ORDER - 1 - k:MA_ORDER - 1 - k + T]
        X += np.einsum("bfmn,bfnt->bmft", A[:, :, k], seg)
    X /= np.sqrt(np.mean(np.abs(X) ** 2, axis=(1, 2, 3), keepdims=True))
    X += 1e-2 * cnormal((B, M, F, T))
    return X if B > 1 else X[0]


def make_autoregression(n_channels, taps, delay, n_bins, n_frames, seed=0):
    """x_t = G0^H xs_t + e_t with exactly ``taps`` and ``delay`` and white innovations e: returns
    (X, E), both (M, F, T).  G0 is small enough for the recursion to be stable."""
    M, K, D, F, T = n_channels, taps, delay, n_bins, n_frames
    rng = np.random.default_rng([seed, M, K, D, F, T])
    L = K * M
    G0 = (rng.standard_normal((F, L, M)) + 1j * rng.standard_normal((F, L, M))) * (0.5 / L)
    E = (rng.standard_normal((M, F, T)) + 1j * rng.standard_normal((M, F, T))) / np.sqrt(2.0)
    X = np.zeros((M, F, T), dtype=np.complex128)
    for t in range(T):
        for f in range(F):
            xs = np.zeros(L, dtype=np.complex128)
            for k in range(K):
                if t - D - k >= 0:
                    xs[k * M:(k + 1) * M] = X[:, f, t - D - k]
            X[:, f, t] = np.conj(G0[f].T) @ xs + E[:, f, t]
    return X, E
