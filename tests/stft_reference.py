"""Extended-precision restatement of the STFT / ISTFT entry points, with error bars per segment.

TEST INFRASTRUCTURE ONLY.  Written from the formulas in the header comment of
ssspy_amd/csrc/stft_kernels.hip and the documented conventions of ``scipy.signal.stft`` / ``istft``
(``boundary="zeros"``, ``padded=True``, one-sided, ``scaling="spectrum"``), in ``np.longdouble`` /
``np.clongdouble`` (x87 extended: 64 mantissa bits).  Every function takes ``dtype``: with
``np.float64`` the SAME formulas are evaluated in plain float64 NumPy, which is what
tests/test_stft_reference_cpu.py uses to show that the bars are attainable.  Nothing here calls into
oracle/ or the library.

The transform is the direct DFT, a matrix of twiddles e^{-+ 2 pi i r / n} indexed by
r = (k t) mod n reduced in integers, with pi = 4 arctan(1) formed in ``dtype`` (a Python float for pi
is itself 0.4 u off relative, 7 u of the phase at the far end of the table: it would spoil the
reference).

The bars
--------
Absolute, per element, and per SEGMENT: every quantity below is formed from the one segment (one
channel, one frame) the element belongs to, so a quiet frame next to a loud one keeps a bar of its
own size.  u = 2^-53.  They are derived, not tuned:

* A radix-2 transform of length len with twiddles accurate to mu has the normwise error
  (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., theorem 24.2)
  ``||dy||_2 <= log2(len) eta ||y||_2``, ``eta = mu + gamma_4 (sqrt(2) + mu)``, gamma_4 = 4u/(1-4u),
  to first order.  R(len) = log2(len) eta below.
* mu: the twiddles come from ``sincospi``.  The ROCm installation carries no document that states
  its ULP figure (none mentions the function), so mu = 4 u is used, as for the other double
  precision trigonometric functions of that family.  The argument pos / half of a butterfly's
  twiddle is exact (half is a power of two).
* Each element is bounded by the norm: ``|dy_k| <= ||dy||_2``, with ``||y||_2 = sqrt(len) ||v||_2``
  for the transform of v.  Write s = ||v||_2 for the segment's input: the windowed samples for the
  forward transform (their product carries `pre` = 1 rounding, u s in norm), the Hermitian
  extension of the frame's bins for the inverse (`pre` = 0).
* Direct route (n a power of two): one transform,
      bar_y = (R(n) + pre u) sqrt(n) s.
* Bluestein (any other n): y_k = c_k sum_t (v_t c_t) b_{k-t}, c_t = e^{-+ i pi t^2 / n},
  b = conj(c) at offsets -(n-1) .. n-1, the convolution through three transforms of length
  m = the power of two >= 2 n - 1.  A chirp value is sincospi of r / n with r = t^2 mod 2n reduced in
  integers: the quotient lies below 2, so its rounding is at most u absolute, pi u of phase:
  mu_c = mu + pi u.  To first order
    - a = v c carries (pre + 2) u + mu_c per element and its transform R(m): eps_A relative to
      ||A||_2 = sqrt(m) s.  Through the exact remainder (times bhat, inverse transform, / m) an error
      dA is the convolution of b with a sequence of norm eps_A s, at most eps_A s ||b||_2
      = eps_A s sqrt(2n - 1) per element (Cauchy-Schwarz).
    - bhat, the transform of b, carries eps_b = mu_c + R(m) relative to ||bhat||_2 = sqrt(m (2n-1));
      an error dbhat is a perturbation db of b with ||db||_2 = eps_b sqrt(2n - 1), convolved with a:
      at most eps_b sqrt(2n - 1) s per element.
    - the product A bhat: 2 u |A_j| |bhat_j|; through the inverse transform and 1/m at most
      (2 u / m) ||A||_2 ||bhat||_2 = 2 u sqrt(2n - 1) s.
    - the inverse transform of P = A bhat: R(m) ||P||_2 / sqrt(m) after the 1/m, and
      ||P||_2 <= ||A||_2 max|bhat| = sqrt(m) s B, so R(m) B s.  B = max_j |bhat_j| is a companion
      magnitude; float64 computes it (`chirp_peak`).
    - the last product with c_k and the 1/m: (2 + 1) u + mu_c on |y_k| itself.
      bar_y = sqrt(2n-1) s ((pre + 2) u + mu_c + R(m) + mu_c + R(m) + 2 u) + R(m) B s
              + (3 u + mu_c) |y_k|.
* Forward output Z = y / sum(w): the kernel multiplies by fl(1 / fl(sum w)), 2 u, and the caller's
  float64 sum of the window is off by at most S u sum|w|, S = min(n - 1, 24 + ceil(log2 n)) (NumPy
  sums pairwise: at most 15 + 3 additions deep inside a block of 128 on 8 accumulators, then a
  binary tree over the blocks):
      bar_Z = bar_y / |sum w| + (2 + S sum|w| / |sum w|) u |Z|.
* ISTFT, per output sample.  A frame's contribution is seg = Re(y_t) (sum(w) / n) w_t: the bar of
  y_t times |sum(w) w_t / n|, plus (3 + S sum|w| / |sum w|) u |seg| (the sum's error, the division
  by n, two products).  Then: the bars of the n_ov segments overlapping the sample are summed;
  n_ov u sum|seg| is added for the accumulation; the result is divided by norm = the overlapped
  w^2 where that exceeds 1e-10 (else by 1), and (n_ov + 1) u for norm's own sum of positive terms
  plus 2 u for the division are added on |x|.
* A segment whose input is exactly zero has s = 0 and y = 0, hence bar 0: its output must be
  exactly zero.  (-0.0 compares equal.)
"""

import functools

import numpy as np

LD = np.longdouble
U = float(2.0 ** -53)
MU = 4.0 * U  # sincospi; see the module docstring
ETA = MU + (4.0 * U / (1.0 - 4.0 * U)) * (np.sqrt(2.0) + MU)
MU_CHIRP = MU + np.pi * U
NORM_THRESHOLD = 1e-10
LEVELS = (1.0, 1e-6, 1e6, 0.0)


def _c(dtype):
    return np.clongdouble if dtype is LD else np.complex128


def _pi(dtype):
    return 4 * np.arctan(dtype(1))


def twiddles(n, sign, dtype=LD):
    """e^{sign 2 pi i r / n}, r = 0 .. n-1."""
    ang = (2 * _pi(dtype)) * np.arange(n).astype(dtype) / dtype(n)
    out = np.empty(n, _c(dtype))
    out.real = np.cos(ang)
    out.imag = sign * np.sin(ang)
    return out


def bluestein_len(n):
    """0 for a power of two (transformed directly), else the power of two >= 2 n - 1."""
    if n & (n - 1) == 0:
        return 0
    m = 1
    while m < 2 * n - 1:
        m *= 2
    return m


@functools.lru_cache(maxsize=None)
def chirp_peak(n):
    """max_j |bhat_j| of the Bluestein chirp's spectrum: a companion magnitude, float64 suffices."""
    m = bluestein_len(n)
    j = np.arange(-(n - 1), n)
    b = np.zeros(m, np.complex128)
    b[j % m] = np.exp(1j * np.pi * ((j * j) % (2 * n)) / n)
    return float(np.abs(np.fft.fft(b)).max())


def sum_roundings(n):
    return min(n - 1, 24 + int(np.ceil(np.log2(n))))


def transform_bar(n, s, absy, pre):
    """Bar on one element of the unnormalised DFT of length n.  s: the 2-norm of the segment's input
    (broadcasts against absy); absy: |y| of the element; pre: roundings (in u) already in the input."""
    s = np.asarray(s, np.float64)
    absy = np.asarray(absy, np.float64)
    m = bluestein_len(n)
    if m == 0:
        return (np.log2(n) * ETA + pre * U) * np.sqrt(n) * s + 0.0 * absy
    R = np.log2(m) * ETA
    conv = ((pre + 2) * U + MU_CHIRP + R) + (MU_CHIRP + R) + 2 * U
    return np.sqrt(2 * n - 1) * s * conv + R * chirp_peak(n) * s + (3 * U + MU_CHIRP) * absy


def frames(L, n, hop):
    """(starts, n_frames): n // 2 zeros either side, then zeros at the end up to a whole number of
    hops; segment j covers samples start_j .. start_j + n - 1 of the unpadded signal."""
    padded = L + 2 * (n // 2)
    n_frames = -(-(padded - n) // hop) + 1  # ceil
    return np.arange(n_frames) * hop - n // 2, n_frames


def segments(x, n, hop):
    """x (..., L) -> (..., n_frames, n): the zero-padded segments, unwindowed."""
    x = np.asarray(x)
    L = x.shape[-1]
    starts, J = frames(L, n, hop)
    total = (J - 1) * hop + n
    xp = np.zeros(x.shape[:-1] + (max(total, L + n // 2),), x.dtype)
    xp[..., n // 2: n // 2 + L] = x
    idx = (starts + n // 2)[:, None] + np.arange(n)[None, :]
    return xp[..., idx]


def check_bins(n, seed=0):
    """All bins up to n = 1024; beyond, 64 fixed by seed that include 0, 1, F-2 and F-1."""
    F = n // 2 + 1
    if n <= 1024:
        return np.arange(F)
    rng = np.random.default_rng(seed)
    rest = rng.choice(np.arange(2, F - 2), size=60, replace=False)
    return np.sort(np.concatenate([[0, 1, F - 2, F - 1], rest]))


def check_samples(L_out, n, seed=0):
    """All samples up to n = 1024; beyond, 64 fixed by seed that include both ends."""
    if n <= 1024 or L_out <= 64:
        return np.arange(L_out)
    rng = np.random.default_rng(seed)
    rest = rng.choice(np.arange(2, L_out - 2), size=60, replace=False)
    return np.sort(np.concatenate([[0, 1, L_out - 2, L_out - 1], rest]))


def stft(x, window, n, hop, bins=None, dtype=LD):
    """Z[..., k, j] = (1 / sum w) sum_t x[start_j + t] w[t] e^{-2 pi i k t / n} -> (Z, bar)."""
    c = _c(dtype)
    w = np.asarray(window).astype(dtype)
    ks = np.arange(n // 2 + 1) if bins is None else np.asarray(bins)
    seg = segments(np.asarray(x).astype(dtype), n, hop) * w  # (..., J, n)
    E = twiddles(n, -1, dtype)[(ks[:, None] * np.arange(n)[None, :]) % n]  # (K, n)
    Y = np.swapaxes(seg.astype(c) @ E.T, -1, -2)  # (..., K, J)
    sw = w.sum()
    Z = Y / sw
    s = np.sqrt((np.abs(seg) ** 2).sum(axis=-1)).astype(np.float64)[..., None, :]
    rel_sum = sum_roundings(n) * float(np.abs(w).sum() / np.abs(sw))
    absZ = np.abs(Z).astype(np.float64)
    bar = transform_bar(n, s, np.abs(Y), 1) / float(np.abs(sw)) + (2 + rel_sum) * U * absZ
    return Z, bar


def istft_samples(n_frames, n, hop):
    return n + (n_frames - 1) * hop - 2 * (n // 2)


def istft(Z, window, n, hop, samples=None, dtype=LD):
    """Hermitian extension (imaginary parts of DC and, for even n, Nyquist ignored), inverse DFT / n,
    times window * sum(window), overlap-add divided by the overlapped window^2 where that exceeds
    1e-10 (else by 1), boundary removed -> (x, bar, norm), at `samples` (default: all)."""
    c = _c(dtype)
    Z = np.asarray(Z)
    F, J = Z.shape[-2:]
    assert F == n // 2 + 1
    L_out = istft_samples(J, n, hop)
    samples = np.arange(L_out) if samples is None else np.asarray(samples)
    p = samples + n // 2
    w = np.asarray(window).astype(dtype)
    sw = w.sum()
    g = sw / dtype(n)
    rel_sum = sum_roundings(n) * float(np.abs(w).sum() / np.abs(sw))
    Zc = Z.astype(c).copy()
    Zc.imag[..., 0, :] = 0
    ck = np.full(F, 2.0)
    ck[0] = 1.0
    if n % 2 == 0:
        Zc.imag[..., F - 1, :] = 0
        ck[F - 1] = 1.0
    # the 2-norm of the frame's Hermitian extension
    s = np.sqrt(np.einsum("k,...kj->...j", ck, np.abs(Zc).astype(np.float64) ** 2))
    tw = twiddles(n, 1, dtype)
    k = np.arange(F)
    ckd = ck.astype(dtype)
    shape = Z.shape[:-2] + (len(samples),)
    acc = np.zeros(shape, dtype)
    acc_abs = np.zeros(shape, np.float64)
    acc_bar = np.zeros(shape, np.float64)
    norm = np.zeros(len(samples), dtype)
    count = np.zeros(len(samples), np.float64)
    chunk = max(1, (1 << 21) // F)
    for j in range(J):
        t = p - j * hop
        where = np.nonzero((t >= 0) & (t < n))[0]
        for lo in range(0, len(where), chunk):
            sel = where[lo: lo + chunk]
            tv = t[sel]
            E = tw[(tv[:, None] * k[None, :]) % n] * ckd  # (T, F)
            y = (Zc[..., :, j] @ E.T).real  # (..., T)
            gw = g * w[tv]
            seg = y * gw
            bar_y = transform_bar(n, s[..., j][..., None], np.abs(y), 0)
            agw = np.abs(gw).astype(np.float64)
            aseg = np.abs(seg).astype(np.float64)
            acc[..., sel] += seg
            acc_abs[..., sel] += aseg
            acc_bar[..., sel] += bar_y * agw + (3 + rel_sum) * U * aseg
            norm[sel] += w[tv] ** 2
            count[sel] += 1
    big = norm > dtype(NORM_THRESHOLD)
    den = np.where(big, norm, dtype(1))
    x = acc / den
    denf = den.astype(np.float64)
    bar = (acc_bar + count * U * acc_abs) / denf
    bar = bar + np.where(big, (count + 3) * U, 0.0) * np.abs(x).astype(np.float64)
    return x, bar, norm


def propagate(bar_Z, window, n, hop):
    """What an error of at most bar_Z (..., F, J; all bins) in a spectrogram does to the exact ISTFT
    of it, per output sample: |dx| <= sum_j |sum(w) w_t / n| sum_k c_k bar_Z[k, j] / norm."""
    F, J = bar_Z.shape[-2:]
    w = np.asarray(window, np.float64)
    ck = np.full(F, 2.0)
    ck[0] = 1.0
    if n % 2 == 0:
        ck[F - 1] = 1.0
    per_frame = np.einsum("k,...kj->...j", ck, bar_Z) * abs(w.sum()) / n
    L_out = istft_samples(J, n, hop)
    p = np.arange(L_out) + n // 2
    out = np.zeros(bar_Z.shape[:-2] + (L_out,))
    norm = np.zeros(L_out)
    for j in range(J):
        t = p - j * hop
        sel = np.nonzero((t >= 0) & (t < n))[0]
        out[..., sel] += per_frame[..., j][..., None] * np.abs(w[t[sel]])
        norm[sel] += w[t[sel]] ** 2
    return out / np.where(norm > NORM_THRESHOLD, norm, 1.0)


def assert_norm_clear_of_threshold(norm):
    """A condition on the inputs: no position's overlapped window^2 lies within a relative 1e-3 of
    the 1e-10 branch, so that the reference and a float64 evaluation take the same side."""
    rel = np.abs(np.asarray(norm, np.float64) / NORM_THRESHOLD - 1.0)
    assert rel.min() > 1e-3, "window^2 sum within 1e-3 of the 1e-10 threshold: choose another input"


# ------------------------------------------------------------------------------------- test inputs
def envelope(n_stretches_of, L, hop, ch):
    """Piecewise constant over hop-aligned stretches; the levels 1, 1e-6, 1e6 and exactly 0 in an
    order rotated by the channel, so neighbouring frames differ by up to 12 decades."""
    stretch = max(1, (L // hop) // n_stretches_of) * hop
    which = (np.arange(L) // stretch + ch) % len(LEVELS)
    return np.asarray(LEVELS)[which]


def signal(seed, C, L, n, hop):
    """(C, L) float64: per channel a white-noise carrier times `envelope`, and a sinusoid exactly on
    a bin (added under the envelope on even channels, so that their zero stretches stay exactly zero,
    and on top of it on odd ones).  Channel 0 starts at 1e6; channel 1 (where C > 1) is all zeros."""
    rng = np.random.default_rng(seed)
    t = np.arange(L)
    x = np.zeros((C, L))
    for ch in range(C):
        k0 = 1 + (ch + n // 3) % max(1, n // 2)
        tone = np.sin(2 * np.pi * ((k0 * t) % n) / n)
        env = envelope(4, L, hop, ch + 2)
        carrier = rng.standard_normal(L)
        x[ch] = env * carrier + tone if ch % 2 else env * (carrier + tone)
    if C > 1:
        x[1] = 0.0
    return x


def spectrogram(seed, C, n, J):
    """(C, F, J) complex128, arbitrary (no forward transform of anything): non-zero imaginary DC and
    Nyquist rows, per-frame amplitude steps through LEVELS rotated by the channel, channel 1 zero."""
    rng = np.random.default_rng(seed)
    F = n // 2 + 1
    Z = rng.standard_normal((C, F, J)) + 1j * rng.standard_normal((C, F, J))
    for ch in range(C):
        Z[ch] *= np.asarray(LEVELS)[(np.arange(J) + ch + 2) % len(LEVELS)]
    if C > 1:
        Z[1] = 0.0
    return Z
