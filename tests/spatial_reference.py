"""Extended-precision restatement of the ISS, IP2 and scale-restoration entry points, with error bars.

TEST INFRASTRUCTURE ONLY, in the style of tests/pass_reference.py (whose rules for the elementwise
bars apply here unchanged).  One function per entry point of include/ssspy_amd.h, written from the
update rules its header comments cite (ssspy/bss/_update_spatial_model.py, ssspy/algorithm/
projection_back.py, ssspy/algorithm/minimal_distortion_principle.py) in ``np.longdouble``; with
``dtype=np.float64`` the SAME formula runs in plain float64, which is the yardstick below.

Two kinds of bars.

* Plain sums (``r2_next``, the tracked log-determinant increment, ``mdp_scale``,
  ``ilrma_scale_basis``, ``scale_filter_row``): elementwise ``m u companion``, m counted from the
  operation; a reciprocal or reciprocal square root by seed + two Newton steps counts 2, as rcp_nr.
* Solves and recurrences (the N sweeps of fused ISS1 on Y, G of the ISS transforms, the rows of IP2
  and ip1_source_solve, projection_back_*, demix_from_covariance): the IP1 rule.  A norm per bin
  (per (bin, source) over the frames for the fused kernel), ``|got - ref| <= c g u |ref|`` with g a
  growth or condition factor computed in extended precision and c = 8 x the largest g-normalised
  error the float64 run of the restatement makes ON THE SAME INPUTS (``yardstick``).  Nothing is
  fitted to a kernel.  The g of each operation:

  - fused ISS1 / iss1_transform / iss2_transform: a sweep is Y <- A Y with A = I - v e_n^T (ISS2:
    the pair's two rows and the pair's two columns of the others); rounding made in one sweep is
    carried by the later ones, so g = | |A_last| ... |A_1| |Y0| | / |ref| row by row (entrywise
    moduli; for the transforms Y0 = I), times, for the transforms, the cancellation of forming the
    statistics through G: max over (step, set) of (|G| |V| |G|^H)_nn / (G V G^H)_nn.
  - IP2: the largest kappa_2(W U) over the pair's two solves and the pairs walked, divided by the
    relative gap (l1 - l0) / l1 of the pair's 2 x 2 generalised eigenvalues (an eigenvector moves by
    the perturbation over the gap).  ip1_source_solve: kappa_2(W U_n).
  - projection_back_filter: kappa_2(W); projection_back_scale: kappa_2(YY); demix_from_covariance:
    kappa_2(XX).

* Phase.  The rows an eigenvector produces (IP2's pair rows, ISS2's pair rows of G) carry the
  arbitrary unit phase of that eigenvector; ``align_phase`` turns each such row onto the reference
  before the comparison.  Nothing else is gauged away.

Nothing here calls into oracle/ or reads the kernels.  ``mutant`` arguments switch on one
deliberate mistake each; tests/test_spatial_reference_cpu.py shows every one is caught.
"""

import numpy as np

import pass_reference as pr

LD, U = pr.LD, pr.U
floor, lu_solve = pr.floor, pr.lu_solve
FRAME, BIN_FRAME = 1, 2


def _c(dtype):
    return np.clongdouble if dtype is LD else np.complex128


def _f64(a):
    return np.asarray(a, dtype=np.complex128 if np.iscomplexobj(a) else np.float64)


def cond2(A):
    """kappa_2 of a stack of matrices given in any precision (the norm needs no more than float64;
    the inverse is taken in the precision given)."""
    n = A.shape[-1]
    flat = A.reshape(-1, n, n)
    inv = lu_solve(flat, np.broadcast_to(np.eye(n, dtype=flat.dtype), flat.shape).copy())[0]
    k = np.linalg.norm(_f64(flat), 2, axis=(1, 2)) * np.linalg.norm(_f64(inv), 2, axis=(1, 2))
    return k.reshape(A.shape[:-2])


def normwise(got, ref, g, axes):
    """max of |got - ref| / (g u |ref|), 2-norms over `axes`; g has the shape that is left."""
    d = np.asarray(got).astype(ref.dtype) - ref
    num = np.sqrt((np.abs(d) ** 2).sum(axis=axes))
    den = np.sqrt((np.abs(ref) ** 2).sum(axis=axes)) * g * U
    return float(np.max(num / den))


def rowwise(got, ref, comp):
    """normwise() over the last axis with the bar's g |ref| given as `comp` (defined where |ref| = 0)."""
    d = np.asarray(got).astype(ref.dtype) - ref
    return float(np.max(np.sqrt((np.abs(d) ** 2).sum(axis=-1)) / (comp * U)))


def align_phase(got, ref, rows=None):
    """got with each row (last axis) turned by the unit phase that brings it onto ref's."""
    got = np.array(got, dtype=ref.dtype)
    ip = (got.conj() * ref).sum(axis=-1, keepdims=True)
    a = np.abs(ip)
    ph = np.where(a > 0, ip / np.where(a > 0, a, 1), 1)
    if rows is not None:
        keep = np.ones(got.shape[-2], bool)
        keep[list(rows)] = False
        ph[..., keep, :] = 1
    return got * ph


# --------------------------------------------------------------------------------------- fused ISS1
def _weights(weight, kind, shape, dtype):
    B, N, F, T = shape
    w = weight.astype(dtype)
    return np.broadcast_to(w[:, :, None, :], shape) if kind == FRAME else w


def iss1_fused(Y, weight, kind, flooring, dtype=LD, mutant=None):
    """update_by_iss1 on Y (B,N,F,T), weight (B,N,T) [FRAME] or (B,N,F,T) [BIN_FRAME]:
    for n: num_s = mean_j w_s y_s conj(y_n), den_s = floor(mean_j w_s |y_n|^2), v_s = num_s / den_s,
    v_n = 1 - den_n^(-1/2), Y <- Y - v y_n.
    Returns dict: Y, g (B,N,F), comp (B,N,F) = g |ref| (the companion's row norms), d (B,F,N) the
    floored den_n of sweep n, wspread (B,F,N)."""
    c = _c(dtype)
    B, N, F, T = Y.shape
    Yc = Y.astype(c).copy()
    w = _weights(weight, kind, Y.shape, dtype)
    S = np.abs(Yc).astype(dtype)  # the companion: moduli carried through |A_n|
    d_all = np.zeros((B, F, N), dtype)
    Tm = T - 1 if mutant == "drop_last_frame" else T
    for n in range(N):
        yn = Yc[:, n]
        cy = yn if mutant == "no_conj" else yn.conj()
        wn = np.broadcast_to(w[:, n:n + 1], w.shape) if mutant == "weight_n" else w
        num = (wn * Yc * cy[:, None])[..., :Tm].sum(axis=-1) / dtype(T)
        den = floor((wn * (np.abs(yn) ** 2)[:, None])[..., :Tm].sum(axis=-1) / dtype(T), flooring)
        v = num / den
        if mutant == "one_minus_inv":
            v[:, n] = 1 - 1 / den[:, n]
        else:
            v[:, n] = 1 - 1 / np.sqrt(den[:, n])
        d_all[:, :, n] = den[:, n]
        Yc = Yc - v[..., None] * yn[:, None]
        av = np.abs(v).astype(dtype)
        Sn = S[:, n].copy()
        S = S + av[..., None] * Sn[:, None]
        S[:, n] = np.abs(1 - v[:, n])[..., None] * Sn + 0 * S[:, n]
    if mutant == "drop_last_bin":
        Yc[:, :, -1] = Y.astype(c)[:, :, -1]
    nrm = np.sqrt((np.abs(Yc) ** 2).sum(axis=-1))
    comp = np.sqrt((S ** 2).sum(axis=-1))
    # (T < N: a row the sweeps cancel exactly is zero in the reference; g |ref| = the companion's norm
    #  stays defined there, and `rowwise` measures against it)
    g = comp / np.where(nrm > 0, nrm, comp)
    wf = _f64(w)
    wspread = np.sqrt(wf.max(axis=-1) / wf.min(axis=-1)).transpose(0, 2, 1)  # (B, F, N)
    return {"Y": Yc, "g": np.maximum(_f64(g), 1.0), "d": d_all, "wspread": wspread,
            "comp": np.maximum(comp, nrm)}


def frame_power_of(Ygot, dtype=LD):
    """r2_next[b,n,j] = sum_i |y_nij|^2 OF THE Y THE KERNEL LEFT (the registers it squares are the
    values it stores): F terms in any order, each |y|^2 two products and a sum: m = F + 3."""
    P = np.abs(Ygot.astype(_c(dtype))) ** 2
    r2 = P.sum(axis=2)
    return r2, (Ygot.shape[2] + 3) * U * r2


def iss1_logdet(ref, logdet0, c, T, nblocks, dtype=LD, mutant=None):
    """logdet[b] = logdet0[b] - 1/2 sum_{i,n} log d_in (absolute bar).  d_in = floor(mean_j w |y_n|^2)
    is a sum of T terms of a row that carries c g u normwise: rel(d) = (T + 3) + 2 c g wspread
    (Cauchy-Schwarz on the weighted sum, wspread = sqrt(max w / min w)), and log d moves by that
    absolutely; kept as a mantissa product and an exponent sum per block, log(mant) + ln 2 expo: 2 u of
    each part, at most 2 ln 2 per factor; the sum of N F logs, the fold over the blocks and the
    addition to logdet0: (N F + nblocks + 2) u on the magnitudes."""
    d = ref["d"].astype(dtype)
    B, F, N = d.shape
    lg = np.log(d)
    sign, half = (1, 0.5)
    if mutant == "logdet_sign":
        sign = -1
    if mutant == "logdet_half":
        half = 1.0
    val = logdet0.astype(dtype) - sign * dtype(half) * lg.sum(axis=(1, 2))
    g = ref["g"].transpose(0, 2, 1)  # (B, F, N)
    rel_d = (T + 3) + 2 * c * g * ref["wspread"]
    mag = np.abs(logdet0.astype(dtype)) + 0.5 * np.abs(lg).sum(axis=(1, 2))
    bar = U * (0.5 * (rel_d + 2 * 2 * np.log(2.0) + 2).sum(axis=(1, 2)) + (N * F + nblocks + 2) * mag)
    return val, bar


# --------------------------------------------------------------------------------------- 2 x 2 pencil
def eigh2(A, Bm):
    """A z = lamb Bm z for stacks of 2 x 2 Hermitian matrices (Bm positive definite), closed form in
    the dtype given.  lamb ascending (n,2); Z[...,:,k] the eigenvector of lamb[k], scaled to
    z^H Bm z = 1 as the reference's Cholesky route leaves it (the floors see h^H G h at that scale),
    of arbitrary phase.  Also the relative gap (l1 - l0) / l1."""
    a00, a11, a01 = A[:, 0, 0].real, A[:, 1, 1].real, A[:, 0, 1]
    b00, b11, b01 = Bm[:, 0, 0].real, Bm[:, 1, 1].real, Bm[:, 0, 1]
    detB = b00 * b11 - np.abs(b01) ** 2
    detA = a00 * a11 - np.abs(a01) ** 2
    tr = (a00 * b11 + a11 * b00 - 2 * (a01 * b01.conj()).real) / detB
    disc = np.sqrt(np.maximum(tr * tr - 4 * detA / detB, 0))
    # (the larger root first, the smaller from the product: no cancellation for a positive pencil)
    l1 = (tr + np.where(tr >= 0, disc, -disc)) / 2
    l0 = (detA / detB) / l1
    lo, hi = np.minimum(l0, l1), np.maximum(l0, l1)
    lamb = np.stack([lo, hi], axis=-1)
    Z = np.zeros(A.shape, A.dtype)
    for k in range(2):
        M = A - lamb[:, k, None, None] * Bm
        z1 = np.stack([-M[:, 0, 1], M[:, 0, 0]], axis=-1)
        z2 = np.stack([M[:, 1, 1], -M[:, 1, 0]], axis=-1)
        use1 = (np.abs(z1) ** 2).sum(axis=-1) >= (np.abs(z2) ** 2).sum(axis=-1)
        z = np.where(use1[:, None], z1, z2)
        Z[:, :, k] = z / np.sqrt(_quad(z, Bm))[:, None]
    gap = _f64((hi - lo) / np.maximum(np.abs(hi), np.abs(lo)))
    return lamb, Z, gap


def _quad(h, G):
    return np.einsum("fa,fab,fb->f", h.conj(), G, h).real


# --------------------------------------------------------------------------------------- IP1 / IP2
def ip1_source_solve(W, Ucov, n, dtype=LD):
    """w = (W U_n)^-1 e_n; row n of W <- conj(w) (UNNORMALISED), denom = sqrt(max(Re w^H U_n w, 0)).
    Returns (W_new, denom (B,F), kappa (B,F))."""
    c = _c(dtype)
    B, F, N, _ = W.shape
    Wc = W.astype(c).reshape(B * F, N, N).copy()
    Un = Ucov.astype(c).reshape(B * F, N, N, N)[:, n]
    A = np.einsum("fab,fbc->fac", Wc, Un)
    e = np.zeros((B * F, N, 1), c)
    e[:, n, 0] = 1
    w = lu_solve(A, e)[0][:, :, 0]
    q = _quad(w, Un)
    Wc[:, n, :] = w.conj()
    return Wc.reshape(B, F, N, N), np.sqrt(np.maximum(q, 0)).reshape(B, F), cond2(A).reshape(B, F)


def scale_filter_row(W, denom, n, dtype=LD):
    """row n of W divided by denom (B,F): a real divisor, each component rounded once: 2 u in modulus."""
    Wc = W.astype(_c(dtype)).copy()
    Wc[:, :, n, :] = Wc[:, :, n, :] / denom.astype(dtype)[:, :, None]
    bar = np.zeros(W.shape, LD)
    bar[:, :, n, :] = 2 * U * np.abs(Wc[:, :, n, :])
    return Wc, bar


def update_by_ip2(W, Ucov, pairs, flooring, pair_only=False, dtype=LD, deferred=False, mutant=None,
                  parts=None):
    """Pairwise iterative projection (update_by_ip2_one_pair per pair, in order).  Ucov (B,F,N,N,N)
    indexed by source, or with pair_only (B,F,2,N,N): the pair's own two.  deferred: rows left
    unnormalised, denom (B,F,2) returned.  Returns (W_new, g (B,F), denom or None); `parts`, if given,
    receives kappa (B,F) and gap (B,F), the two factors of g."""
    c = _c(dtype)
    B, F, N, _ = W.shape
    Wc = W.astype(c).reshape(B * F, N, N).copy()
    Uc = Ucov.astype(c).reshape(B * F, -1, N, N)
    g, kap, gp = np.zeros(B * F), np.zeros(B * F), np.ones(B * F)
    denom = None
    for m, n in pairs:
        if pair_only and mutant != "pair_only_by_source":
            Um, Un = Uc[:, 0], Uc[:, 1]
        else:
            Um, Un = Uc[:, m % Uc.shape[1]], Uc[:, n % Uc.shape[1]]
        E = np.zeros((B * F, N, 2), c)
        E[:, m, 0] = 1
        E[:, n, 1] = 1
        Am, An = np.einsum("fab,fbc->fac", Wc, Um), np.einsum("fab,fbc->fac", Wc, Un)
        Pm, Pn = lu_solve(Am, E)[0], lu_solve(An, E)[0]
        Gm = np.einsum("faj,fab,fbk->fjk", Pm.conj(), Um, Pm)
        Gn = np.einsum("faj,fab,fbk->fjk", Pn.conj(), Un, Pn)
        _, Z, gap = eigh2(Gm, Gn)
        # the reference reverses the ascending order: h_m belongs to the LARGER eigenvalue
        hm, hn = (Z[:, :, 0], Z[:, :, 1]) if mutant == "swap_eigenvectors" else (Z[:, :, 1], Z[:, :, 0])
        qm, qn = np.maximum(_quad(hm, Gm), 0), np.maximum(_quad(hn, Gn), 0)
        if deferred:
            denom = np.stack([np.sqrt(qm), np.sqrt(qn)], axis=-1).reshape(B, F, 2)
            dm = dn = np.ones_like(qm)
        elif mutant == "floor_q":
            dm, dn = np.sqrt(floor(qm, flooring)), np.sqrt(floor(qn, flooring))
        else:
            dm, dn = floor(np.sqrt(qm), flooring), floor(np.sqrt(qn), flooring)
        Wc[:, m, :] = (np.einsum("fak,fk->fa", Pm, hm) / dm[:, None]).conj()
        Wc[:, n, :] = (np.einsum("fak,fk->fa", Pn, hn) / dn[:, None]).conj()
        if dtype is LD:
            k = np.maximum(cond2(Am), cond2(An))
            g, kap, gp = np.maximum(g, k / gap), np.maximum(kap, k), np.minimum(gp, gap)
    if parts is not None:
        parts.update(kappa=kap.reshape(B, F), gap=gp.reshape(B, F))
    return Wc.reshape(B, F, N, N), g.reshape(B, F), denom


# --------------------------------------------------------------------------------------- ISS transforms
def iss_statistics(Y, weight, kind, dtype=LD):
    """Vc[b,i,s] = (1/T) sum_j w_s y y^H (B,F,N,N,N)."""
    c = _c(dtype)
    w = _weights(weight, kind, Y.shape, dtype)
    Yc = Y.astype(c)
    return np.einsum("bsij,baij,bcij->bisac", w.astype(c), Yc, Yc.conj()) / dtype(Y.shape[-1])


def _growth(Gabs, G, cancel):
    g = np.sqrt((Gabs ** 2).sum(axis=(-2, -1))) / np.sqrt((np.abs(G) ** 2).sum(axis=(-2, -1)))
    return np.maximum(_f64(g), 1.0) * np.maximum(cancel, 1.0)


def iss1_transform(Vc, flooring, dtype=LD, mutant=None):
    """The N rank-1 steps of update_by_iss1 on the statistics: with G the transform so far the
    covariance of set s is G Vc_s G^H; num_s = its [s, n], den_s = floor(its [n, n]).
    Returns (G (B,F,N,N), g (B,F))."""
    c = _c(dtype)
    B, F, N = Vc.shape[0], Vc.shape[1], Vc.shape[-1]
    V = Vc.astype(c).reshape(B * F, N, N, N)
    Va = np.abs(V).astype(dtype)
    G = np.broadcast_to(np.eye(N, dtype=c), (B * F, N, N)).copy()
    Ga = np.abs(G).astype(dtype)
    cancel = np.ones(B * F)
    for n in range(N):
        gn = G[:, n, :]
        t = np.einsum("fsad,fd->fsa", V, gn.conj())          # V_s g_n^H
        num = np.einsum("fsa,fsa->fs", G, t)                  # row s of G against set s
        if mutant == "no_conj":
            num = num.conj()
        dn = np.einsum("fa,fsa->fs", gn, t).real
        if mutant == "weight_n":
            num = np.einsum("fsa,fa->fs", G, t[:, n])
            dn = np.broadcast_to(dn[:, n:n + 1], dn.shape)
        den = floor(dn, flooring)
        v = num / den
        v[:, n] = 1 - (1 / den[:, n] if mutant == "one_minus_inv" else 1 / np.sqrt(den[:, n]))
        comp = np.einsum("fa,fsad,fd->fs", np.abs(gn), Va, np.abs(gn))
        cancel = np.maximum(cancel, _f64(np.max(comp / np.abs(dn), axis=1)))
        G = G - v[:, :, None] * gn[:, None, :]
        gan = Ga[:, n, :].copy()
        Ga = Ga + np.abs(v)[:, :, None] * gan[:, None, :]
        Ga[:, n, :] = np.abs(1 - v[:, n])[:, None] * gan
    return G.reshape(B, F, N, N), _growth(Ga, G, cancel).reshape(B, F)


def iss2_transform(Vc, pairs, flooring, dtype=LD, deferred=False, G0=None):
    """update_by_iss2 on the statistics, pair by pair: the others take y_s += conj(q_s) y_pair,
    q_s = -(V_s[pair,pair])^-1 V_s[pair,s]; the pair takes conj(h_k) y_pair / floor(sqrt(h_k^H G_k h_k)),
    h the eigenvectors of G_m z = lamb G_n z in ASCENDING order (no reversal here).  deferred: the
    pair's rows left unnormalised, denom (B,F,2) returned; G0: continue from this transform.
    Returns (G, g (B,F), denom or None)."""
    c = _c(dtype)
    B, F, N = Vc.shape[0], Vc.shape[1], Vc.shape[-1]
    V = Vc.astype(c).reshape(B * F, N, N, N)
    Va = np.abs(V).astype(dtype)
    G = (np.broadcast_to(np.eye(N, dtype=c), (B * F, N, N)).copy() if G0 is None
         else G0.astype(c).reshape(B * F, N, N).copy())
    Ga = np.abs(G).astype(dtype)
    cancel, gapmin, denom = np.ones(B * F), np.ones(B * F), None
    for m, n in pairs:
        pr_ = [m, n]
        Gp = G[:, pr_, :]                                                  # (f, 2, N)
        blk = np.einsum("fja,fsad,fkd->fsjk", Gp, V, Gp.conj())           # 2 x 2 block of every set
        comp = np.einsum("fja,fsad,fjd->fsj", np.abs(Gp), Va, np.abs(Gp))
        diag = np.stack([blk[:, :, 0, 0].real, blk[:, :, 1, 1].real], axis=-1)
        cancel = np.maximum(cancel, _f64(np.max(comp / np.abs(diag), axis=(1, 2))))
        A = np.broadcast_to(np.eye(N, dtype=c), (B * F, N, N)).copy()
        for s in range(N):
            if s in pr_:
                continue
            Fv = np.einsum("fja,fad,fd->fj", Gp, V[:, s], G[:, s, :].conj())  # mean w_s y_pair conj(y_s)
            b = blk[:, s]
            det = b[:, 0, 0] * b[:, 1, 1] - b[:, 0, 1] * b[:, 1, 0]
            q0 = -(b[:, 1, 1] * Fv[:, 0] - b[:, 0, 1] * Fv[:, 1]) / det
            q1 = -(-b[:, 1, 0] * Fv[:, 0] + b[:, 0, 0] * Fv[:, 1]) / det
            A[:, s, m], A[:, s, n] = q0.conj(), q1.conj()
        Gm, Gn = blk[:, m], blk[:, n]
        _, Z, gap = eigh2(Gm, Gn)
        gapmin = np.minimum(gapmin, gap)
        h = [Z[:, :, 0], Z[:, :, 1]]
        q = [np.maximum(_quad(h[0], Gm), 0), np.maximum(_quad(h[1], Gn), 0)]
        if deferred:
            denom = np.stack([np.sqrt(q[0]), np.sqrt(q[1])], axis=-1).reshape(B, F, 2)
            d = [np.ones_like(q[0])] * 2
        else:
            d = [floor(np.sqrt(q[0]), flooring), floor(np.sqrt(q[1]), flooring)]
        for k, row in enumerate(pr_):
            A[:, row, :] = 0
            A[:, row, m] = (h[k][:, 0] / d[k]).conj()
            A[:, row, n] = (h[k][:, 1] / d[k]).conj()
        G = np.einsum("fab,fbc->fac", A, G)
        Ga = np.einsum("fab,fbc->fac", np.abs(A).astype(dtype), Ga)
    g = _growth(Ga, G, cancel) / gapmin
    return G.reshape(B, F, N, N), g.reshape(B, F), denom


# --------------------------------------------------------------------------------------- scale restoration
def _inv(A):
    return lu_solve(A, np.broadcast_to(np.eye(A.shape[-1], dtype=A.dtype), A.shape).copy())[0]


def projection_back_filter(W, reference_id, dtype=LD, mutant=None):
    """scale_n = (W^-1)[ref, n]; W <- W * scale[:, None] (rows).  Returns (W_new, scale (B,F,N),
    kappa (B,F))."""
    c = _c(dtype)
    B, F, N, _ = W.shape
    Wc = W.astype(c).reshape(B * F, N, N)
    Inv = _inv(Wc)
    s = Inv[:, :, reference_id] if mutant == "pb_column" else Inv[:, reference_id, :]
    return ((Wc * s[:, :, None]).reshape(B, F, N, N), s.reshape(B, F, N), cond2(Wc).reshape(B, F))


def projection_back_scale(XY, YY, reference_id, dtype=LD):
    """scale_n = ((X Y^H) (Y Y^H)^-1)[ref, n].  Returns (scale (B,F,N), kappa(YY) (B,F))."""
    c = _c(dtype)
    B, F, N, _ = XY.shape
    A = YY.astype(c).reshape(B * F, N, N)
    s = np.einsum("fc,fcn->fn", XY.astype(c).reshape(B * F, N, N)[:, reference_id, :], _inv(A))
    return s.reshape(B, F, N), cond2(A).reshape(B, F)


def demix_from_covariance(YX, XX, dtype=LD):
    """W = YX XX^-1.  Returns (W, kappa(XX) (B,F))."""
    c = _c(dtype)
    B, F, N, _ = YX.shape
    A = XX.astype(c).reshape(B * F, N, N)
    Wn = np.einsum("fab,fbc->fac", YX.astype(c).reshape(B * F, N, N), _inv(A))
    return Wn.reshape(B, F, N, N), cond2(A).reshape(B, F)


def diag_of(scale):
    """(B,F,N) -> the (B,F,N,N) diagonal matrices the kernels write."""
    N = scale.shape[-1]
    return scale[..., :, None] * np.eye(N, dtype=scale.dtype)


def mdp_scale(YX, YY, reference_id, dtype=LD, mutant=None):
    """G = diag(conj(z_n)), z_n = YX[n, ref] / Re YY[n, n]: a real divisor, 2 u in modulus."""
    c = _c(dtype)
    N = YX.shape[-1]
    z = YX.astype(c)[..., :, reference_id] / np.einsum("bfnn->bfn", YY.astype(c)).real
    G = diag_of(z if mutant == "mdp_no_conj" else z.conj())
    return G, 2 * U * np.abs(G).astype(LD)


def ilrma_scale_basis(basis, G, domain, dtype=LD):
    """basis[b,n,i,:] *= |G[b,i,n,n]|^p.  |g|^2 carries 3 u (x^2 + y^2: two products and a sum of
    positives, 2 u; as hypot(x, y)^2, which is how NumPy's float64 forms it: 1 + 2 for the square);
    p = 2: the product with the basis, 4 u in all; otherwise a power with exponent p / 2 (exact for
    p = 1): p / 2 * 3 for what |g|^2 carries, 2 for the power (+ |e ln x| where p / 2 is not a
    float64), 1 for the product."""
    p = dtype(domain)
    a2 = np.abs(np.einsum("bfnn->bnf", G.astype(_c(dtype)))) ** 2
    sc = a2 if p == 2 else a2 ** (p / 2)
    out = basis.astype(dtype) * sc[..., None]
    if p == 2:
        m = 4 + 0 * sc
    else:
        exact = LD(np.float64(p / 2)) == LD(p) / 2
        m = 1.5 * p + 3 + (0 if exact else np.abs((p / 2) * np.log(a2)))
    return out, U * m[..., None] * out


# --------------------------------------------------------------------------------------- generators
def gen_iss_inputs(seed, B, N, F, T, kind, tiny_bin=True):
    """Y (B,N,F,T): unit complex Gaussians times a per-(mixture, source, bin) scale over 2^-3..2^3;
    the first bin of the first mixture is scaled by 1e-6, so that its denominators (1e-12-ish) fall
    below eps = 1e-10 and stay far inside the normal range.  Weights over 2^-2..2^2."""
    rng = np.random.default_rng(seed)
    Y = (rng.standard_normal((B, N, F, T)) + 1j * rng.standard_normal((B, N, F, T))) \
        * np.exp2(rng.uniform(-3, 3, (B, N, F, 1)))
    if tiny_bin:
        Y[0, :, 0, :] *= 1e-6
    w = np.exp2(rng.uniform(-2, 2, (B, N, T) if kind == FRAME else (B, N, F, T)))
    return np.ascontiguousarray(Y), w


def gen_ip2_inputs(seed, B, F, N, n_sets=None, log2_cond=0.0, T=None):
    """(W, U): filters with rows over 2^-1..2^1 and covariances U_s = (1/T) sum_j w_sj x x^H of a
    spread x, the channels of x scaled over 2^(-log2_cond/4)..2^(log2_cond/4) (kappa(U) up to
    2^log2_cond).  Weights over 2^-2..2^2 per frame: the pair's pencil keeps a relative gap."""
    rng = np.random.default_rng(seed)
    W = pr.gen_filters(seed, B, F, N, log2_range=1)
    S = N if n_sets is None else n_sets
    T = T or 8 * N
    x = rng.standard_normal((B, N, F, T)) + 1j * rng.standard_normal((B, N, F, T))
    x = x * np.exp2(rng.uniform(-log2_cond / 4, log2_cond / 4, (B, N, F, 1)))
    w = np.exp2(rng.uniform(-2, 2, (B, S, F, T)))
    Uc = np.einsum("bsij,baij,bcij->bisac", w, x, x.conj()) / T
    return W, np.ascontiguousarray(Uc)


def gen_conditioned(seed, B, F, N, log2_range):
    """(B,F,N,N) matrices Q1 diag(s) Q2, Q unitary, s log-uniform in 2^-r..2^r: kappa_2 <= 2^(2 r) that
    no row or column scaling explains (for a diagonally scaled matrix kappa_2 overstates what a solve
    loses, and an error normalised by it says little)."""
    rng = np.random.default_rng(seed)
    q = [np.linalg.qr(rng.standard_normal((B, F, N, N)) + 1j * rng.standard_normal((B, F, N, N)))[0]
         for _ in range(2)]
    s = np.exp2(rng.uniform(-log2_range, log2_range, (B, F, N)))
    return np.ascontiguousarray(np.einsum("bfac,bfc,bfcd->bfad", q[0], s, q[1]))


def yardstick(err_f64):
    """c of the normwise bars: 8 x the g-normalised error of the float64 restatement."""
    return 8.0 * float(err_f64)
