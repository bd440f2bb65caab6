"""Thin Python wrappers over the C ABI: torch HBM tensors in, torch HBM tensors out.

Shapes carry the leading batch axis B (see include/ssspy_amd.h).  Nothing here
synchronises with the device.
"""

from . import _device as dv
from . import _lib, _routes
from ._device import ptr


def _L():
    return _lib.load()


# ---- workspace allocation.  With SSSPY_AMD_WS_CANARY=1 (the GPU tests set it) every workspace gets
# a guard band behind it, filled with a pattern that check_workspace_canaries() verifies: a kernel
# that writes past the size the C ABI asked for is caught instead of corrupting a neighbour.
import os as _os

_CANARY_DOUBLES = 4096 if _os.environ.get("SSSPY_AMD_WS_CANARY") else 0
_CANARY_VALUE = -7.25e300
_canaries = []


def _workspace(nbytes, dev):
    n = (int(nbytes) + 7) // 8
    buf = dv.empty((n + _CANARY_DOUBLES,), dv.f64, dev)
    if not _CANARY_DOUBLES:
        return buf, int(nbytes)
    import weakref

    buf[n:].fill_(_CANARY_VALUE)
    view = buf[:n]
    view._guard = buf[n:]  # keeps the band addressable for as long as the workspace lives
    _canaries.append((weakref.ref(view), n))
    return view, int(nbytes)


def check_workspace_canaries():
    """Raise if anything wrote behind a live workspace (only active with SSSPY_AMD_WS_CANARY=1)."""
    alive = []
    for ref, n in _canaries:
        view = ref()
        if view is None:
            continue
        alive.append((ref, n))
        if not bool((view._guard == _CANARY_VALUE).all().item()):
            raise RuntimeError("a kernel wrote past the end of a {}-byte workspace".format(8 * n))
    _canaries[:] = alive


def _st():
    return dv.stream_handle()


# ---- transient scratch of single operators (partial sums folded inside the same C-ABI call): one
# growing buffer per (device, stream): calls on one stream run in order, so the buffer is never
# needed by two operators at once; separators driven on different streams of one device (threads,
# parallel.separate_pipelined callers) get their own (round-3 advisor finding)
_scratch_bufs = {}


def _scratch(nbytes, dev):
    nbytes = int(nbytes)
    if nbytes == 0:
        return None, 0
    key = (str(dev), _st())
    ent = _scratch_bufs.get(key)
    if ent is None or ent[1] < nbytes:
        ent = _workspace(nbytes, dev)
        _scratch_bufs[key] = ent
    return ent


def separate(X, W, out=None):
    B, N, F, T = X.shape
    if out is None:
        out = dv.empty((B, N, F, T), dv.c128, X.device)
    _lib.check(_L().ssspy_separate(ptr(X), ptr(W), ptr(out), B, N, F, T, _st()), "separate")
    return out


def weighted_covariance(A, weight=None, kind=_lib.WEIGHT_UNIT, n_sets=1, out=None):
    B, N, F, T = A.shape
    if out is None:
        out = dv.empty((B, F, n_sets, N, N), dv.c128, A.device)
    _lib.check(
        _L().ssspy_weighted_covariance(ptr(A), ptr(weight), kind, ptr(out), B, N, n_sets, F, T, _st()),
        "weighted_covariance",
    )
    return out


def covariance_congruence(C, G, out, tracked=None):
    """out = G C G^H per bin: C, out (B, F, N, N) or (B, F, S, N, N) with the S matrices of a bin
    sharing its G (B, F, N, N).  ``tracked`` = (power (B, F, N, N), slots (2, B, 2) f64, phase): the
    launch also leaves its power-weighted rounding amplification per mixture in slots[phase & 1]
    and clears the other half (2..4 sources, see the header)."""
    B, F, N = C.shape[0], C.shape[1], C.shape[-1]
    S = C.shape[2] if C.dim() == 5 else 1
    if tracked is not None:
        power, slots, phase = tracked
        assert tuple(slots.shape) == (2, B, 2) and tuple(power.shape) == (B, F, N, N)
        _lib.check(_L().ssspy_covariance_congruence_tracked(ptr(C), ptr(G), ptr(out), B, F, S, N,
                                                            ptr(power), ptr(slots), int(phase),
                                                            _st()),
                   "covariance_congruence")
        return out
    _lib.check(_L().ssspy_covariance_congruence_sets(ptr(C), ptr(G), ptr(out), B, F, S, N, _st()),
               "covariance_congruence")
    return out


def compose_filters(G, W, out):
    """out = G W per bin, (B, F, N, N)."""
    B, F, N = W.shape[0], W.shape[1], W.shape[-1]
    _lib.check(_L().ssspy_compose_filters(ptr(G), ptr(W), ptr(out), B, F, N, _st()),
               "compose_filters")
    return out


def cross_covariance(A, Bm, out=None):
    B, N, F, T = A.shape
    if out is None:
        out = dv.empty((B, F, N, N), dv.c128, A.device)
    _lib.check(_L().ssspy_cross_covariance(ptr(A), ptr(Bm), ptr(out), B, N, F, T, _st()),
               "cross_covariance")
    return out


def _apply_host(fn, dev_tensor):
    """fn on the host copy of a device tensor, one mixture (leading axis) at a time: the shapes the
    callable sees are the reference's."""
    import numpy as np

    host = dv.to_host(dev_tensor)
    out = np.stack([np.asarray(fn(h), dtype=host.dtype) for h in host])
    if out.shape != host.shape:
        raise ValueError("flooring_fn must return an array of the shape it was given")
    return out


def update_by_ip1(W, U, flooring, info=None):
    B, F, N, _ = W.shape
    host = getattr(flooring, "host", None)
    if host is not None:
        # an arbitrary flooring callable: one source at a time, the denominators d (B, F) come down,
        # are floored on the host and go back up (ssspy/bss/_update_spatial_model.py:63-76)
        denom = dv.empty((B, F), dv.f64, W.device)
        for n in range(N):
            _lib.check(_L().ssspy_ip1_source_solve(ptr(W), ptr(U), ptr(denom), n, B, F, N,
                                                   ptr(info), _st()), "ip1_source_solve")
            denom.copy_(dv.to_device(_apply_host(host, denom), dev=W.device))
            _lib.check(_L().ssspy_scale_filter_row(ptr(W), ptr(denom), n, B, F, N, _st()),
                       "scale_filter_row")
        return W
    _lib.check(
        _L().ssspy_update_by_ip1(ptr(W), ptr(U), B, F, N, flooring[0], flooring[1], ptr(info), _st()),
        "update_by_ip1",
    )
    return W


def update_by_ip1_logdet_slots(B, F, N):
    """Shares per mixture ``update_by_ip1_logdet`` leaves in ``logdet``."""
    return int(_L().ssspy_update_by_ip1_logdet_slots(B, F, N))


def update_by_ip1_logdet(W, U, flooring, info, logdet, logdet_stride):
    """update_by_ip1 that also leaves sum_i log|det W_i| of the filters as they come in, as shares at
    logdet[s * logdet_stride + b] (device floors only; the caller zeroes the array once per run)."""
    B, F, N, _ = W.shape
    _lib.check(
        _L().ssspy_update_by_ip1_logdet(ptr(W), ptr(U), B, F, N, flooring[0], flooring[1], ptr(info),
                                        ptr(logdet), int(logdet_stride), _st()),
        "update_by_ip1_logdet",
    )
    return W


def update_by_iss1_host_floor(Y, weight, kind, host):
    """ISS1 with an arbitrary flooring callable: per source one covariance pass and one pass that
    applies the steering step; the N x F denominators are floored on the host in between.
    ref: ssspy/bss/_update_spatial_model.py:178-192."""
    import numpy as np

    B, N, F, T = Y.shape
    Vc = None
    eye = np.eye(N, dtype=np.complex128)
    for n in range(N):
        Vc = weighted_covariance(Y, weight, kind, N, out=Vc)  # (B, F, m, a, b) = mean varphi_m y y^H
        V = dv.to_host(Vc)
        num = V[:, :, np.arange(N), np.arange(N), n]          # (B, F, m): mean varphi_m y_m conj(y_n)
        den = np.real(V[:, :, :, n, n])                       # (B, F, m): mean varphi_m |y_n|^2
        # the callable sees (n_sources, n_bins) as in the reference
        den = np.stack([np.asarray(host(d.T), dtype=np.float64).T for d in den])
        v = num / den
        v[:, :, n] = 1.0 - 1.0 / np.sqrt(den[:, :, n])
        G = np.broadcast_to(eye, (B, F, N, N)).copy()
        G[:, :, :, n] -= v                                     # y <- y - v y_n
        separate(Y, dv.to_device(G, dev=Y.device), out=Y)
    return Y


def iss1_transform(Vc, flooring, out=None):
    B, F, N = Vc.shape[0], Vc.shape[1], Vc.shape[-1]
    if out is None:
        out = dv.empty((B, F, N, N), dv.c128, Vc.device)
    _lib.check(
        _L().ssspy_iss1_transform(ptr(Vc), ptr(out), B, F, N, flooring[0], flooring[1], _st()),
        "iss1_transform",
    )
    return out


def _pair_array(pairs):
    import ctypes

    flat = [int(v) for pair in pairs for v in pair]
    return (ctypes.c_int * len(flat))(*flat), len(flat) // 2


def update_by_ip2(W, U, pairs, flooring, info=None, pair_only=False):
    """Pairwise iterative projection in place on W; U (B,F,N,N,N), or with pair_only the pair's own
    two covariances (B,F,2,N,N)."""
    B, F, N, _ = W.shape
    host = getattr(flooring, "host", None)
    if host is not None:
        # an arbitrary flooring callable: pair by pair, the two denominators (B, F) floored on the
        # host between the projection and the division (ref: _update_spatial_model.py:381-388)
        import numpy as np

        denom = dv.empty((B, F, 2), dv.f64, W.device)
        for pair in pairs:
            arr, _ = _pair_array([pair])
            _lib.check(_L().ssspy_update_by_ip2_deferred(ptr(W), ptr(U), int(bool(pair_only)), arr,
                                                         B, F, N, ptr(denom), ptr(info), _st()),
                       "update_by_ip2 (deferred)")
            d = dv.to_host(denom)
            for k, row in enumerate(pair):
                # (the callable sees (n_bins, 1), as in the reference)
                dk = np.stack([np.asarray(host(d[b, :, k][:, None]), dtype=np.float64).reshape(F)
                               for b in range(B)])
                _lib.check(_L().ssspy_scale_filter_row(ptr(W), ptr(dv.to_device(dk, dev=W.device)),
                                                       int(row), B, F, N, _st()), "scale_filter_row")
        return W
    arr, n_pairs = _pair_array(pairs)
    _lib.check(
        _L().ssspy_update_by_ip2(ptr(W), ptr(U), int(bool(pair_only)), arr, n_pairs, B, F, N,
                                 flooring[0], flooring[1], ptr(info), _st()),
        "update_by_ip2",
    )
    return W


def iss2_transform(Vc, pairs, flooring, info=None, out=None):
    B, F, N = Vc.shape[0], Vc.shape[1], Vc.shape[-1]
    if out is None:
        out = dv.empty((B, F, N, N), dv.c128, Vc.device)
    host = getattr(flooring, "host", None)
    if host is not None:
        # an arbitrary flooring callable: pair by pair on the accumulated transform, the two
        # denominators floored on the host (ref: _update_spatial_model.py:300-312)
        import numpy as np

        denom = dv.empty((B, F, 2), dv.f64, Vc.device)
        for p, pair in enumerate(pairs):
            arr, _ = _pair_array([pair])
            _lib.check(_L().ssspy_iss2_transform_deferred(ptr(Vc), ptr(out), arr, int(p > 0), B, F,
                                                          N, ptr(denom), ptr(info), _st()),
                       "iss2_transform (deferred)")
            d = dv.to_host(denom)
            # (the callable sees both members at once, (2, n_bins, 1), as in the reference:
            #  _update_spatial_model.py:300-312 floors the square root with keepdims)
            fl = np.stack([np.asarray(host(d[b].T[:, :, None]), dtype=np.float64).reshape(2, F)
                           for b in range(B)])
            for k, row in enumerate(pair):
                dk = np.ascontiguousarray(fl[:, k, :])
                _lib.check(_L().ssspy_scale_filter_row(ptr(out), ptr(dv.to_device(dk, dev=Vc.device)),
                                                       int(row), B, F, N, _st()), "scale_filter_row")
        return out
    arr, n_pairs = _pair_array(pairs)
    _lib.check(
        _L().ssspy_iss2_transform(ptr(Vc), ptr(out), arr, n_pairs, B, F, N, flooring[0],
                                  flooring[1], ptr(info), _st()),
        "iss2_transform",
    )
    return out


def ipa_sweep(Vc, normalization, max_iter, flooring, info=None, out=None, newton_ws=None,
              not_converged=None):
    """All N source steps of an IPA sweep on the per-bin statistics Vc (overwritten: V_m <- G V_m G^H
    after each step); returns the accumulated transform G (B, F, N, N)."""
    B, F, N = Vc.shape[0], Vc.shape[1], Vc.shape[-1]
    if out is None:
        out = dv.empty((B, F, N, N), dv.c128, Vc.device)
    _lib.check(
        _L().ssspy_ipa_sweep(ptr(Vc), ptr(out), B, F, N, int(bool(normalization)), int(max_iter),
                             flooring[0], flooring[1], ptr(info), ptr(newton_ws),
                             ptr(not_converged), _st()),
        "ipa_sweep",
    )
    return out


def update_by_ipa(Y, weight, kind, normalization, max_iter, flooring, newton_ws, info=None,
                  not_converged=None, Vc=None, frame_power=False):
    """One IPA sweep in place on the device spectrogram Y (B, N, F, T).  The weights are fixed over
    the sweep (ref: _update_spatial_model.py:436-445), so the covariances the reference recomputes
    from the updated spectrogram before every source step are G V G^H of the previous ones: one
    weighted covariance, the N steps on the per-bin statistics, one Y <- G Y (round 5; three passes
    over Y instead of 3 N).
    Vc: the weighted covariances of Y when the caller has formed them already (then `weight` is not
    read; overwritten).  newton_ws: the sweep's vote words (bss._device_state.newton_words)."""
    N = Y.shape[1]
    if Vc is None:
        Vc = weighted_covariance(Y, weight, kind, N)
    G = ipa_sweep(Vc, normalization, max_iter, flooring, info, newton_ws=newton_ws,
                  not_converged=not_converged)
    if frame_power:  # (AuxIVA: the next iteration's weights want sum_i |y|^2 of the new Y)
        r2 = separate_frame_power(Y, G)
        if r2 is not None:
            return r2
    separate(Y, G, out=Y)
    return None if frame_power else Y


def iss1_fused_max_frames(n_sources):
    return int(_L().ssspy_iss1_fused_max_frames(n_sources))


def iss1_fused(Y, weight, kind, flooring, r2_next=None, logdet=None):
    """In-place fused ISS1 on Y; optionally leaves the next iteration's frame powers (summed without
    atomics: blocks' partial sums in a scratch buffer, folded in order), and moves `logdet` (B,) =
    sum_i log|det W_i| of the implied demixing filters along with the sweeps."""
    B, N, F, T = Y.shape
    ws, ws_bytes = (None, 0)
    if r2_next is not None or logdet is not None:
        ws, ws_bytes = _scratch(_L().ssspy_iss1_fused_workspace_bytes(B, N, F, T), Y.device)
    if logdet is not None:
        _lib.check(
            _L().ssspy_iss1_fused_tracked(ptr(Y), ptr(weight), kind, ptr(r2_next), B, N, F, T,
                                          flooring[0], flooring[1], ptr(logdet), ptr(ws), ws_bytes,
                                          _st()),
            "iss1_fused_tracked",
        )
        return Y
    _lib.check(
        _L().ssspy_iss1_fused(ptr(Y), ptr(weight), kind, ptr(r2_next), B, N, F, T, flooring[0],
                              flooring[1], ptr(ws), ws_bytes, _st()),
        "iss1_fused",
    )
    return Y


def projection_back_filter(W, reference_id, info=None, scale_out=None):
    B, F, N, _ = W.shape
    _lib.check(
        _L().ssspy_projection_back_filter(ptr(W), ptr(scale_out), B, F, N, reference_id, ptr(info),
                                          _st()),
        "projection_back_filter",
    )
    return W


def mdp_scale(YX, YY, reference_id, out=None):
    B, F, N, _ = YX.shape
    if out is None:
        out = dv.empty((B, F, N, N), dv.c128, YX.device)
    _lib.check(_L().ssspy_mdp_scale(ptr(YX), ptr(YY), ptr(out), B, F, N, int(reference_id), _st()),
               "mdp_scale")
    return out


def ilrma_scale_basis(basis, G, domain):
    B, N, F, K = basis.shape
    _lib.check(_L().ssspy_ilrma_scale_basis(ptr(basis), ptr(G), B, N, F, K, domain, _st()),
               "ilrma_scale_basis")


def projection_back_scale(XY, YY, reference_id, info=None, out=None):
    B, F, N, _ = XY.shape
    if out is None:
        out = dv.empty((B, F, N, N), dv.c128, XY.device)
    _lib.check(
        _L().ssspy_projection_back_scale(ptr(XY), ptr(YY), ptr(out), B, F, N, reference_id,
                                         ptr(info), _st()),
        "projection_back_scale",
    )
    return out


def demix_from_covariance(YX, XX, info=None, out=None):
    B, F, N, _ = YX.shape
    if out is None:
        out = dv.empty((B, F, N, N), dv.c128, YX.device)
    _lib.check(
        _L().ssspy_demix_from_covariance(ptr(YX), ptr(XX), ptr(out), B, F, N, ptr(info), _st()),
        "demix_from_covariance",
    )
    return out


def sum_logdet(W, out=None):
    B, F, N, _ = W.shape
    if out is None:
        out = dv.empty((B,), dv.f64, W.device)
    _lib.check(_L().ssspy_sum_logdet(ptr(W), ptr(out), B, F, N, _st()), "sum_logdet")
    return out


def logdet(W):
    """log|det W| of every matrix of a device stack (..., N, N) c128 -> f64 (...); -inf where singular."""
    N = W.shape[-1]
    out = dv.empty(tuple(W.shape[:-2]), dv.f64, W.device)
    if out.numel():
        _lib.check(_L().ssspy_logdet(ptr(W), ptr(out), out.numel(), N, _st()), "logdet")
    return out


# ----------------------------------------------------------------------------- ILRMA
def ilrma_workspace(B, N, F, T, K, dev):
    return _workspace(_L().ssspy_ilrma_workspace_bytes(B, N, F, T, K), dev)


GAUSS = (_lib.SOURCE_GAUSS, 0.0)  # source model as (SSSPY_SOURCE_*, model_param); see include/ssspy_amd.h


def ilrma_update_basis(X, W, basis, activation, domain, flooring, ws, ws_bytes, model=GAUSS):
    B, N, F, T = X.shape
    K = basis.shape[-1]
    _lib.check(
        _L().ssspy_ilrma_update_basis(ptr(X), ptr(W), ptr(basis), ptr(activation), B, N, F, T, K,
                                      domain, model[0], model[1], flooring[0], flooring[1], ptr(ws),
                                      ws_bytes, _st()),
        "ilrma_update_basis",
    )


def ilrma_update_activation(X, W, basis, activation, domain, flooring, ws, ws_bytes, model=GAUSS):
    B, N, F, T = X.shape
    K = basis.shape[-1]
    _lib.check(
        _L().ssspy_ilrma_update_activation(ptr(X), ptr(W), ptr(basis), ptr(activation), B, N, F, T,
                                           K, domain, model[0], model[1], flooring[0], flooring[1],
                                           ptr(ws), ws_bytes, _st()),
        "ilrma_update_activation",
    )


def ilrma_weighted_covariance(X, basis, activation, domain, ws, ws_bytes, out=None, W=None,
                              model=GAUSS, flooring=(0, 0.0)):
    B, N, F, T = X.shape
    K = basis.shape[-1]
    if out is None:
        out = dv.empty((B, F, N, N, N), dv.c128, X.device)
    _lib.check(
        _L().ssspy_ilrma_weighted_covariance(ptr(X), ptr(W), ptr(basis), ptr(activation), ptr(out),
                                             B, N, F, T, K, domain, model[0], model[1], flooring[0],
                                             flooring[1], ptr(ws), ws_bytes, _st()),
        "ilrma_weighted_covariance",
    )
    return out


def ilrma_normalize_filter(W, C, basis, domain, flooring, ws, ws_bytes):
    B, F, N, _ = W.shape
    K = basis.shape[-1]
    _lib.check(
        _L().ssspy_ilrma_normalize_filter(ptr(W), ptr(C), ptr(basis), B, N, F, K, domain,
                                          flooring[0], flooring[1], ptr(ws), ws_bytes, _st()),
        "ilrma_normalize_filter",
    )


def ilrma_normalize_output(Y, basis, domain, flooring, ws, ws_bytes, frame_power=None, logdet=None):
    """frame_power (B,N,T): sum over bins of |Y|^2 of the current Y when the caller already has it.
    logdet (B,): the tracked sum_i log|det W_i| of the ISS state, moved along with the scaling."""
    B, N, F, T = Y.shape
    K = basis.shape[-1]
    if logdet is not None:
        _lib.check(
            _L().ssspy_ilrma_normalize_output_tracked(
                ptr(Y), ptr(basis), ptr(frame_power), B, N, F, T, K, domain, flooring[0],
                flooring[1], ptr(ws), ws_bytes, ptr(logdet), _st()),
            "ilrma_normalize_output_tracked",
        )
        return
    _lib.check(
        _L().ssspy_ilrma_normalize_output(ptr(Y), ptr(basis), ptr(frame_power), B, N, F, T, K,
                                          domain, flooring[0], flooring[1], ptr(ws), ws_bytes,
                                          _st()),
        "ilrma_normalize_output",
    )


def ilrma_iss_weight(basis, activation, domain, out=None, Y=None, model=GAUSS, flooring=(0, 0.0),
                     Ypow=None):
    """Ypow: |y|^2 (B, N, F, T) float64 handed in instead of y (ssspy_ilrma_iss_weight_power)."""
    B, N, F, K = basis.shape
    T = activation.shape[-1]
    if out is None:
        out = dv.empty((B, N, F, T), dv.f64, basis.device)
    if Ypow is not None:
        _lib.check(
            _L().ssspy_ilrma_iss_weight_power(ptr(Ypow), ptr(basis), ptr(activation), ptr(out), B, N,
                                              F, T, K, domain, model[0], model[1], flooring[0],
                                              flooring[1], _st()),
            "ilrma_iss_weight_power",
        )
        return out
    _lib.check(
        _L().ssspy_ilrma_iss_weight(ptr(Y), ptr(basis), ptr(activation), ptr(out), B, N, F, T, K,
                                    domain, model[0], model[1], flooring[0], flooring[1], _st()),
        "ilrma_iss_weight",
    )
    return out


def ilrma_loss_data(X, W, basis, activation, domain, out=None, model=GAUSS):
    B, N, F, T = X.shape
    K = basis.shape[-1]
    if out is None:
        out = dv.empty((B,), dv.f64, X.device)
    ws, ws_bytes = _scratch(_L().ssspy_ilrma_loss_workspace_bytes(B, N, F, T, K, int(W is not None)),
                            X.device)
    _lib.check(
        _L().ssspy_ilrma_loss_data(ptr(X), ptr(W), ptr(basis), ptr(activation), ptr(out), B, N, F,
                                   T, K, domain, model[0], model[1], ptr(ws), ws_bytes, _st()),
        "ilrma_loss_data",
    )
    return out


def ilrma_ip1_update(X, C, W, basis, activation, U, domain, normalize, flooring, ws, ws_bytes,
                     info, model=GAUSS):
    B, N, F, T = X.shape
    K = basis.shape[-1]
    _lib.check(
        _L().ssspy_ilrma_ip1_update(ptr(X), ptr(C), ptr(W), ptr(basis), ptr(activation), ptr(U), B,
                                    N, F, T, K, domain, model[0], model[1], int(bool(normalize)),
                                    flooring[0], flooring[1], ptr(ws), ws_bytes, ptr(info), _st()),
        "ilrma_ip1_update",
    )


def ilrma_deferred_loss_supported(N, F, T, K, domain, model=GAUSS):
    return bool(_L().ssspy_ilrma_deferred_loss_supported(N, F, T, K, domain, model[0]))


def ilrma_ip1_update_deferred_loss(X, C, W, basis, activation, U, domain, normalize, flooring, ws,
                                   ws_bytes, info, loss_data, logdet, model=GAUSS):
    """The fused update_once() that also leaves the loss of the state at entry (data term, log-dets);
    returns False without touching the state when the shape has no such by-product."""
    B, N, F, T = X.shape
    K = basis.shape[-1]
    rc = _L().ssspy_ilrma_ip1_update_deferred_loss(
        ptr(X), ptr(C), ptr(W), ptr(basis), ptr(activation), ptr(U), B, N, F, T, K, domain, model[0],
        model[1], int(bool(normalize)), flooring[0], flooring[1], ptr(ws), ws_bytes, ptr(info),
        ptr(loss_data), ptr(logdet), _st())
    if rc == _lib.ERR_UNSUPPORTED:
        return False
    _lib.check(rc, "ilrma_ip1_update_deferred_loss")
    return True


def ilrma_deferred_logdet_slots(B, N, F, T, K, domain, model=GAUSS):
    """Shares per mixture ``ilrma_ip1_update_loss_slots`` leaves in ``logdet`` (0: no by-product)."""
    return int(_L().ssspy_ilrma_deferred_logdet_slots(B, N, F, T, K, domain, model[0]))


def ilrma_deferred_loss_slots(B, N, F, T, K, domain, model=GAUSS):
    """Raw loss slots per mixture of ilrma_ip1_update_loss_slots (0: no by-product for this shape)."""
    return int(_L().ssspy_ilrma_deferred_loss_slots(B, N, F, T, K, domain, model[0]))


def ilrma_ip1_update_loss_slots(X, C, W, basis, activation, U, domain, normalize, flooring, ws,
                                ws_bytes, info, slots, slot_stride, logdet, model=GAUSS):
    """ilrma_ip1_update_deferred_loss with the data term left as raw slots (slot s of mixture b at
    slots[s * slot_stride + b]); the caller zeroes the array once and folds it once
    (fold_scalar_slots) for a whole run."""
    B, N, F, T = X.shape
    K = basis.shape[-1]
    _lib.check(_L().ssspy_ilrma_ip1_update_loss_slots(
        ptr(X), ptr(C), ptr(W), ptr(basis), ptr(activation), ptr(U), B, N, F, T, K, domain, model[0],
        model[1], int(bool(normalize)), flooring[0], flooring[1], ptr(ws), ws_bytes, ptr(info),
        ptr(slots), int(slot_stride), ptr(logdet), _st()), "ilrma_ip1_update_loss_slots")


def fold_scalar_slots(slots, total, nslots, out):
    """out[e] = sum_s slots[s * total + e] in slot order."""
    ws, ws_bytes = _scratch(_L().ssspy_fold_scalar_slots_workspace_bytes(int(total), int(nslots)),
                            slots.device)
    _lib.check(_L().ssspy_fold_scalar_slots(ptr(slots), int(total), int(nslots), ptr(out), ptr(ws),
                                            ws_bytes, _st()), "fold_scalar_slots")
    return out


def ilrma_route(B, N, F, T, K, domain, model=GAUSS):
    """(route, act_chunks, basis_plan): the _lib.ROUTE_* the ILRMA passes take for this shape and
    model, the number of bin chunks the activation pass folds, and the basis pass's (unsplit items,
    split items, frame chunks per split item).  Host only."""
    import ctypes

    chunks = ctypes.c_int(0)
    plan = (ctypes.c_int * 3)()
    route = int(_L().ssspy_ilrma_route(B, N, F, T, K, float(domain), model[0], ctypes.byref(chunks),
                                       plan))
    if route < 0:
        raise ValueError("ilrma_route: bad shape")
    return route, int(chunks.value), tuple(plan)


def ilrma_partition_expand(basis, activation, latent, Teff, Vrep):
    B, N, F, K = Teff.shape
    T = Vrep.shape[-1]
    _lib.check(
        _L().ssspy_ilrma_partition_expand(ptr(basis), ptr(activation), ptr(latent), ptr(Teff),
                                          ptr(Vrep), B, N, F, T, K, _st()),
        "ilrma_partition_expand",
    )


def ilrma_partition_update(X, W, basis, activation, latent, Teff, Vrep, domain, steps, flooring, ws,
                           ws_bytes, model=GAUSS):
    B, N, F, T = X.shape
    K = basis.shape[-1]
    _lib.check(
        _L().ssspy_ilrma_partition_update(ptr(X), ptr(W), ptr(basis), ptr(activation), ptr(latent),
                                          ptr(Teff), ptr(Vrep), B, N, F, T, K, domain, model[0],
                                          model[1], steps, flooring[0], flooring[1], ptr(ws),
                                          ws_bytes, _st()),
        "ilrma_partition_update",
    )


def ilrma_partition_normalize(W, C, Y, basis, latent, domain, flooring, ws, ws_bytes):
    B, N, K = latent.shape
    F = basis.shape[-2]
    T = Y.shape[-1] if Y is not None else 1
    _lib.check(
        _L().ssspy_ilrma_partition_normalize(ptr(W), ptr(C), ptr(Y), ptr(basis), ptr(latent), B, N,
                                             F, T, K, domain, flooring[0], flooring[1], ptr(ws),
                                             ws_bytes, _st()),
        "ilrma_partition_normalize",
    )


# ------------------------------------------------------------------------------- IVA
def iva_frame_power(X, W, out=None):
    B, N, F, T = X.shape
    if out is None:
        out = dv.empty((B, N, T), dv.f64, X.device)
    ws, ws_bytes = _scratch(_L().ssspy_iva_frame_power_workspace_bytes(B, N, F, T), X.device)
    _lib.check(_L().ssspy_iva_frame_power(ptr(X), ptr(W), ptr(out), B, N, F, T, ptr(ws), ws_bytes,
                                          _st()), "iva_frame_power")
    return out


def separate_frame_power(Y, G, r2=None):
    """Y <- G Y in place and the frame powers sum_i |y|^2 (B, N, T) of the result in one walk; None
    when the shape has no such kernel (more than 8 sources: the caller makes the two passes)."""
    B, N, F, T = Y.shape
    if N > _lib.MAX_SOURCES:
        return None
    if r2 is None:
        r2 = dv.empty((B, N, T), dv.f64, Y.device)
    ws, ws_bytes = _scratch(_L().ssspy_iva_frame_power_workspace_bytes(B, N, F, T), Y.device)
    _lib.check(_L().ssspy_separate_frame_power(ptr(Y), ptr(G), ptr(Y), ptr(r2), B, N, F, T, ptr(ws),
                                               ws_bytes, _st()), "separate_frame_power")
    return r2


def iva_weight(r2, n_bins, contrast, flooring, weight=None, variance=None):
    B, N, T = r2.shape
    if weight is None:
        weight = dv.empty((B, N, T), dv.f64, r2.device)
    _lib.check(
        _L().ssspy_iva_weight(ptr(r2), ptr(weight), ptr(variance), B, N, n_bins, T, contrast,
                              flooring[0], flooring[1], _st()),
        "iva_weight",
    )
    return weight


def iva_loss_data(r2, variance, n_bins, contrast, out=None):
    B, N, T = r2.shape
    if out is None:
        out = dv.empty((B,), dv.f64, r2.device)
    _lib.check(
        _L().ssspy_iva_loss_data(ptr(r2), ptr(variance), ptr(out), B, N, n_bins, T, contrast, _st()),
        "iva_loss_data",
    )
    return out


def overiva_frame_power(X, W, n_sources, r2=None, Y=None, packed=False):
    """r2 (B, N, T) = sum_i |W_t x|^2 with W_t the first N rows of the full filter W (B, F, M, M),
    or W itself (B, F, N, M) when ``packed``; ``Y`` (B, N, F, T), when given, receives W_t x in the
    same walk."""
    B, M, F, T = X.shape
    N = int(n_sources)
    if r2 is None:
        r2 = dv.empty((B, N, T), dv.f64, X.device)
    ws, ws_bytes = _scratch(_L().ssspy_overiva_frame_power_workspace_bytes(B, N, F, T), X.device)
    _lib.check(_L().ssspy_overiva_frame_power(ptr(X), ptr(W), (N if packed else M) * M, ptr(Y),
                                              ptr(r2), B, M, N, F, T, ptr(ws), ws_bytes, _st()),
               "overiva_frame_power")
    return r2


def overiva_step(W_full, V, C, n_sources, flooring, info=None, logdet=None, trace=None):
    """One OverIVA sweep on the full filter (B, F, M, M) in place (see the header): the loss terms of
    the filter as it comes in into ``logdet`` / ``trace`` (B,) when given, the N row updates from
    ``V`` (B, F, N, M, M) when given, the background rows re-formed from ``C`` (B, F, M, M)."""
    B, F, M, _ = W_full.shape
    ws, ws_bytes = (None, 0)
    if logdet is not None:
        ws, ws_bytes = _scratch(_L().ssspy_overiva_step_workspace_bytes(B, F), W_full.device)
    _lib.check(_L().ssspy_overiva_step(ptr(W_full), ptr(V), ptr(C), B, F, M, int(n_sources),
                                       flooring[0], flooring[1], ptr(info), ptr(logdet), ptr(trace),
                                       ptr(ws), ws_bytes, _st()), "overiva_step")
    return W_full


def iva_score_weight(r2, n_bins, contrast, flooring, weight=None, variance=None):
    """Score weights of the gradient IVA classes: Laplace 1 / floor(r), Gauss 1 / alpha with the
    variance alpha = r2 / n_bins refreshed in ``variance``; (B, N, T)."""
    B, N, T = r2.shape
    if weight is None:
        weight = dv.empty((B, N, T), dv.f64, r2.device)
    _lib.check(
        _L().ssspy_iva_score_weight(ptr(r2), ptr(weight), ptr(variance), B, N, n_bins, T, contrast,
                                    flooring[0], flooring[1], _st()),
        "iva_score_weight",
    )
    return weight


def iva_grad_step_logdet_slots(B, F, N):
    """Shares per mixture ``iva_grad_step`` leaves in ``logdet``."""
    return int(_L().ssspy_iva_grad_step_logdet_slots(B, F, N))


def iva_grad_step(W, stats, natural, holonomic, step_size, info, logdet=None, logdet_stride=0):
    """W <- W - step_size D W (natural) or D W^-H in place, D from ``stats``: the weighted covariances
    (B, F, N, N, N) of the mixture, or mean_j phi(y) y^H (B, F, N, N) itself.  ``logdet``: shares of
    sum_i log|det W_i| of the filters as they come in, at logdet[s * logdet_stride + b]."""
    B, F, N, _ = W.shape
    ready = stats.dim() == 4
    assert tuple(stats.shape) == ((B, F, N, N) if ready else (B, F, N, N, N))
    _lib.check(
        _L().ssspy_iva_grad_step(ptr(W), ptr(stats), int(ready), B, F, N, int(bool(natural)),
                                 int(bool(holonomic)), float(step_size), ptr(info), ptr(logdet),
                                 int(logdet_stride), _st()),
        "iva_grad_step",
    )
    return W


# ------------------------------------------------------------------------------- FDICA
def fdica_weight(Y, aux_form, flooring, weight=None, contrast=None, contrast_stride=0,
                 want_weight=True):
    """Laplace weights of the estimate Y (B, S, F, T): 1 / floor(|y|), or 2 / floor(2 |y|) with
    ``aux_form``.  ``contrast``: the per-bin contrast term sum_s mean_j 2 |y| at
    contrast[i * contrast_stride + b] (F slots, folded with ``fold_scalar_slots``)."""
    B, S, F, T = Y.shape
    if weight is None and want_weight:
        weight = dv.empty((B, S, F, T), dv.f64, Y.device)
    _lib.check(
        _L().ssspy_fdica_weight(ptr(Y), ptr(weight), B, S, F, T, int(bool(aux_form)), flooring[0],
                                flooring[1], ptr(contrast), int(contrast_stride), _st()),
        "fdica_weight",
    )
    return weight


def fdica_route(B, N, F, T, algorithm):
    """The _lib.FDICA_ROUTE_* a shape takes.  Host only."""
    route = int(_L().ssspy_fdica_route(B, N, F, T, int(algorithm)))
    if route < 0:
        raise ValueError("fdica_route: bad shape")
    return route


def fdica_steps(X, W, algorithm, holonomic, step_size, flooring, n_steps, info, loss_data=None,
                logdet=None, slot_stride=0):
    """``n_steps`` whole FDICA iterations on W (B, F, N, N) in place in one launch.  ``loss_data``
    / ``logdet`` (F, slot_stride): the per-bin terms of the state every step starts from and, in
    entry ``n_steps``, of the final state, at [i, s * B + b]."""
    B, N, F, T = X.shape
    assert tuple(W.shape) == (B, F, N, N)
    _lib.check(
        _L().ssspy_fdica_steps(ptr(X), ptr(W), B, N, F, T, int(algorithm), int(bool(holonomic)),
                               float(step_size), flooring[0], flooring[1], int(n_steps),
                               ptr(loss_data), ptr(logdet), int(slot_stride), ptr(info), _st()),
        "fdica_steps",
    )
    return W


# --------------------------------------------------------------------------------- WPE
def _wpe_route_arg():
    """The `route` argument of the WPE entry points: the slab of a bin in LDS where it fits, unless
    the route table forces the re-reading walk."""
    return _lib.WPE_ROUTE_STREAMING if _routes.get("wpe_resident") is False else _lib.WPE_ROUTE_AUTO


def wpe_route(B, M, F, T, taps):
    """(_lib.WPE_ROUTE_RESIDENT or _STREAMING, dynamic LDS bytes of a workgroup).  Host only."""
    import ctypes

    lds = ctypes.c_int(0)
    route = int(_L().ssspy_wpe_route(B, M, F, T, int(taps), ctypes.byref(lds)))
    if route < 0:
        raise ValueError("wpe_route: a shape the WPE kernels do not take")
    return route, lds.value


def wpe_steps(X, G, taps, delay, flooring, n_steps, info, Y=None, loss_data=None, slot_stride=0):
    """``n_steps`` whole WPE iterations on G (B, F, taps * M, M) in place in one launch, then
    Y (B, M, F, T) of the last filter.  ``loss_data`` (F, slot_stride): the per-bin loss terms of
    the state every iteration starts from and, in entry ``n_steps``, of the last, at [f, s * B + b]."""
    B, M, F, T = X.shape
    assert tuple(G.shape) == (B, F, int(taps) * M, M)
    if Y is None:
        Y = dv.empty((B, M, F, T), dv.c128, X.device)
    _lib.check(
        _L().ssspy_wpe_steps(ptr(X), ptr(G), ptr(Y), B, M, F, T, int(taps), int(delay), flooring[0],
                             flooring[1], int(n_steps), ptr(loss_data), int(slot_stride), ptr(info),
                             _wpe_route_arg(), _st()),
        "wpe_steps",
    )
    return Y


def wpe_step(X, G, taps, delay, flooring, info, Y=None, want_statistics=False):
    """One WPE iteration on G in place and Y of the new filter.  With ``want_statistics`` also what
    the iteration formed: (Y, lambda (B, F, T), R (B, F, L, L), P (B, F, L, M), U (B, F, L, L))."""
    B, M, F, T = X.shape
    L = int(taps) * M
    assert tuple(G.shape) == (B, F, L, M)
    if Y is None:
        Y = dv.empty((B, M, F, T), dv.c128, X.device)
    lam = R = P = U = None
    if want_statistics:
        lam = dv.zeros((B, F, T), dv.f64, X.device)
        R = dv.zeros((B, F, L, L), dv.c128, X.device)
        P = dv.zeros((B, F, L, M), dv.c128, X.device)
        U = dv.zeros((B, F, L, L), dv.c128, X.device)
    _lib.check(
        _L().ssspy_wpe_step(ptr(X), ptr(G), ptr(Y), B, M, F, T, int(taps), int(delay), flooring[0],
                            flooring[1], ptr(info), ptr(lam), ptr(R), ptr(P), ptr(U),
                            _wpe_route_arg(), _st()),
        "wpe_step",
    )
    return (Y, lam, R, P, U) if want_statistics else Y


def wpe_apply(X, G, taps, delay, flooring=(_lib.FLOOR_NONE, 0.0), Y=None, loss_data=None,
              slot_stride=0, want_output=True):
    """Y = X - G^H xs for a given G (B, F, taps * M, M); ``loss_data`` (F, slot_stride >= B): the
    per-bin loss terms of that state at [f, b]."""
    B, M, F, T = X.shape
    assert tuple(G.shape) == (B, F, int(taps) * M, M)
    if Y is None and want_output:
        Y = dv.empty((B, M, F, T), dv.c128, X.device)
    _lib.check(
        _L().ssspy_wpe_apply(ptr(X), ptr(G), ptr(Y), B, M, F, T, int(taps), int(delay), flooring[0],
                             flooring[1], ptr(loss_data), int(slot_stride), _wpe_route_arg(), _st()),
        "wpe_apply",
    )
    return Y


# ------------------------------------------------------------------- mask-based beamformers
def _beamform_route_arg():
    """The `route` argument of ssspy_beamform_run: the slab of a bin in LDS where it fits, unless the
    route table forces the re-reading walk."""
    return (_lib.BEAMFORM_ROUTE_STREAMING if _routes.get("beamform_resident") is False
            else _lib.BEAMFORM_ROUTE_AUTO)


def beamform_route(B, M, N, F, T):
    """(_lib.BEAMFORM_ROUTE_RESIDENT or _STREAMING, dynamic LDS bytes of a workgroup).  Host only."""
    import ctypes

    lds = ctypes.c_int(0)
    route = int(_L().ssspy_beamform_route(B, M, N, F, T, ctypes.byref(lds)))
    if route < 0:
        raise ValueError("beamform_route: a shape the beamformer kernel does not take")
    return route, lds.value


def _beamform_masks(X, mask, noise_mask):
    """(B, M, N, F, T, noise_shared) after checking the layouts of the masks against X."""
    B, M, F, T = X.shape
    N = mask.shape[1]
    assert tuple(mask.shape) == (B, N, F, T) and mask.dtype == dv.f64
    shared = False
    if noise_mask is not None:
        assert noise_mask.dtype == dv.f64
        shared = noise_mask.dim() == 3
        assert tuple(noise_mask.shape) == ((B, F, T) if shared else (B, N, F, T))
    return B, M, N, F, T, shared


def beamform_covariances(X, mask, noise_mask=None, normalize=False):
    """(S, Nv (B, F, N, M, M), a, b (B, F, N)): the mask-weighted sums of x x^H and of the weights;
    with ``normalize`` S and Nv divided by max(a, eps) and max(b, eps)."""
    B, M, N, F, T, shared = _beamform_masks(X, mask, noise_mask)
    S = dv.empty((B, F, N, M, M), dv.c128, X.device)
    Nv = dv.empty((B, F, N, M, M), dv.c128, X.device)
    a = dv.empty((B, F, N), dv.f64, X.device)
    b = dv.empty((B, F, N), dv.f64, X.device)
    _lib.check(
        _L().ssspy_beamform_covariances(ptr(X), ptr(mask), ptr(noise_mask), int(shared), ptr(S),
                                        ptr(Nv), ptr(a), ptr(b), B, M, N, F, T, int(bool(normalize)),
                                        _st()),
        "beamform_covariances",
    )
    return S, Nv, a, b


def beamform_filter(Phi_s, Phi_v, kind, reference_id, mu=1.0, info=None):
    """W (B, F, N, M), rows w_n^H, from given covariances (B, F, N, M, M)."""
    B, F, N, M = Phi_s.shape[:4]
    assert tuple(Phi_s.shape) == (B, F, N, M, M) and tuple(Phi_v.shape) == (B, F, N, M, M)
    W = dv.empty((B, F, N, M), dv.c128, Phi_s.device)
    _lib.check(
        _L().ssspy_beamform_filter(ptr(Phi_s), ptr(Phi_v), ptr(W), B, M, N, F, int(kind),
                                   int(reference_id), float(mu), ptr(info), _st()),
        "beamform_filter",
    )
    return W


def beamform_run(X, mask, noise_mask, kind, reference_id, diagonal_loading, mu, info=None,
                 want_output=True, want_covariances=False):
    """One launch from X and the masks to the filters and Y: (W (B, F, N, M), Y (B, N, F, T) or None,
    Phi_s, Phi_v (B, F, N, M, M) or None)."""
    B, M, N, F, T, shared = _beamform_masks(X, mask, noise_mask)
    W = dv.empty((B, F, N, M), dv.c128, X.device)
    Y = dv.empty((B, N, F, T), dv.c128, X.device) if want_output else None
    Ps = Pv = None
    if want_covariances:
        Ps = dv.empty((B, F, N, M, M), dv.c128, X.device)
        Pv = dv.empty((B, F, N, M, M), dv.c128, X.device)
    _lib.check(
        _L().ssspy_beamform_run(ptr(X), ptr(mask), ptr(noise_mask), int(shared), ptr(W), ptr(Y),
                                ptr(Ps), ptr(Pv), B, M, N, F, T, int(kind), int(reference_id),
                                float(diagonal_loading), float(mu), ptr(info), _beamform_route_arg(),
                                _st()),
        "beamform_run",
    )
    return W, Y, Ps, Pv


def beamform_apply(X, W, Y=None):
    """Y (B, N, F, T) = W X per bin for filters W (B, F, N, M)."""
    B, M, F, T = X.shape
    N = W.shape[2]
    assert tuple(W.shape) == (B, F, N, M)
    if Y is None:
        Y = dv.empty((B, N, F, T), dv.c128, X.device)
    _lib.check(_L().ssspy_beamform_apply(ptr(X), ptr(W), ptr(Y), B, M, N, F, T, _st()),
               "beamform_apply")
    return Y


# --------------------------------------------------------------------------------- WPD
def _wpd_route_arg():
    """The `route` argument of the WPD entry points: the slab of a bin in LDS where it fits, unless
    the route table forces the re-reading walk."""
    return _lib.WPD_ROUTE_STREAMING if _routes.get("wpd_resident") is False else _lib.WPD_ROUTE_AUTO


def wpd_route(B, M, N, F, T, taps):
    """(_lib.WPD_ROUTE_RESIDENT or _STREAMING, dynamic LDS bytes of a workgroup).  Host only."""
    import ctypes

    lds = ctypes.c_int(0)
    route = int(_L().ssspy_wpd_route(B, M, N, F, T, int(taps), ctypes.byref(lds)))
    if route < 0:
        raise ValueError("wpd_route: a shape the WPD kernel does not take")
    return route, lds.value


def _wpd_operands(X, mask, steering, W, taps):
    """(B, M, N, F, T) after checking the layouts of the masks, the steering vectors and W against X."""
    B, M, F, T = X.shape
    N = W.shape[2]
    assert tuple(W.shape) == (B, F, N, (int(taps) + 1) * M)
    assert mask is None or (tuple(mask.shape) == (B, N, F, T) and mask.dtype == dv.f64)
    assert steering is None or tuple(steering.shape) == (B, F, N, M)
    return B, M, N, F, T


def wpd_steps(X, mask, steering, W, taps, delay, reference_id, diagonal_loading, flooring, n_steps,
              info, Y=None, Phi_s=None, loss_data=None, slot_stride=0):
    """``n_steps`` whole WPD iterations on W (B, F, N, (taps + 1) M) in place in one launch, then
    Y (B, N, F, T) of the last filter.  ``loss_data`` (F N, slot_stride): the per-(bin, source) loss
    terms of the state every iteration starts from and, in entry ``n_steps``, of the last, at
    [f N + n, s * B + b]."""
    B, M, N, F, T = _wpd_operands(X, mask, steering, W, taps)
    if Y is None:
        Y = dv.empty((B, N, F, T), dv.c128, X.device)
    _lib.check(
        _L().ssspy_wpd_steps(ptr(X), ptr(mask), ptr(steering), ptr(W), ptr(Phi_s), ptr(Y), B, M, N, F,
                             T, int(taps), int(delay), int(reference_id), float(diagonal_loading),
                             flooring[0], flooring[1], int(n_steps), ptr(loss_data), int(slot_stride),
                             ptr(info), _wpd_route_arg(), _st()),
        "wpd_steps",
    )
    return Y


def wpd_step(X, mask, steering, W, taps, delay, reference_id, diagonal_loading, flooring, info,
             Y=None, Phi_s=None, want_statistics=False):
    """One WPD iteration on W in place and Y of the new filter.  With ``want_statistics`` also what the
    iteration formed: (Y, lambda (B, F, N, T), R (B, F, N, Lb, Lb), Phi_s (B, F, N, M, M),
    U (B, F, N, Lb, Lb))."""
    B, M, N, F, T = _wpd_operands(X, mask, steering, W, taps)
    Lb = (int(taps) + 1) * M
    if Y is None:
        Y = dv.empty((B, N, F, T), dv.c128, X.device)
    lam = R = U = None
    if want_statistics:
        lam = dv.zeros((B, F, N, T), dv.f64, X.device)
        R = dv.zeros((B, F, N, Lb, Lb), dv.c128, X.device)
        U = dv.zeros((B, F, N, Lb, Lb), dv.c128, X.device)
        if Phi_s is None:
            Phi_s = dv.zeros((B, F, N, M, M), dv.c128, X.device)
    _lib.check(
        _L().ssspy_wpd_step(ptr(X), ptr(mask), ptr(steering), ptr(W), ptr(Phi_s), ptr(Y), B, M, N, F, T,
                            int(taps), int(delay), int(reference_id), float(diagonal_loading),
                            flooring[0], flooring[1], ptr(info), ptr(lam), ptr(R), ptr(U),
                            _wpd_route_arg(), _st()),
        "wpd_step",
    )
    return (Y, lam, R, Phi_s, U) if want_statistics else Y


def wpd_apply(X, W, taps, delay, flooring=(_lib.FLOOR_NONE, 0.0), Y=None, loss_data=None,
              slot_stride=0, want_output=True):
    """Y (B, N, F, T) = W xb for given filters W (B, F, N, (taps + 1) M); ``loss_data``
    (F N, slot_stride >= B): the per-(bin, source) loss terms of that state at [f N + n, b]."""
    B, M, N, F, T = _wpd_operands(X, None, None, W, taps)
    if Y is None and want_output:
        Y = dv.empty((B, N, F, T), dv.c128, X.device)
    _lib.check(
        _L().ssspy_wpd_apply(ptr(X), ptr(W), ptr(Y), B, M, N, F, T, int(taps), int(delay), flooring[0],
                             flooring[1], ptr(loss_data), int(slot_stride), _wpd_route_arg(), _st()),
        "wpd_apply",
    )
    return Y


# ------------------------------------------------------------------------------- ConvIVA
def conviva_route(B, M, F, T, taps):
    """(_lib.CONVIVA_ROUTE_RESIDENT or _STREAMING, dynamic LDS bytes of a workgroup).  Host only."""
    import ctypes

    lds = ctypes.c_int(0)
    route = int(_L().ssspy_conviva_route(B, M, F, T, int(taps), ctypes.byref(lds)))
    if route < 0:
        raise ValueError("conviva_route: a shape the ConvIVA kernel does not take")
    return route, lds.value


def conviva_statistics(X, phi, taps, delay, diagonal_loading, info, want_statistics=False, Sigma=None,
                       G=None, failed=None):
    """The Schur complements Sigma (B, F, M, M, M) and the prediction filters G (B, F, M, taps M, M)
    of every (mixture, bin, source) from the mixture X (B, M, F, T) and the weights phi (B, M, T);
    ``failed`` (B, F, M) int32 as ssspy_conviva_statistics keeps it (fresh zeros when not given).
    Returns (Sigma, G, failed), with ``want_statistics`` (Sigma, G, failed, Rb (B, F, M, Lb, Lb),
    U (B, F, M, L, L))."""
    B, M, F, T = X.shape
    K = int(taps)
    L, Lb = K * M, (K + 1) * M
    assert tuple(phi.shape) == (B, M, T) and phi.dtype == dv.f64
    if Sigma is None:
        Sigma = dv.zeros((B, F, M, M, M), dv.c128, X.device)
    if G is None:
        G = dv.zeros((B, F, M, L, M), dv.c128, X.device)
    if failed is None:
        failed = dv.zeros((B, F, M), dv.i32, X.device)
    Rb = U = None
    if want_statistics:
        Rb = dv.zeros((B, F, M, Lb, Lb), dv.c128, X.device)
        U = dv.zeros((B, F, M, L, L), dv.c128, X.device)
    route = (_lib.CONVIVA_ROUTE_STREAMING if _routes.get("conviva_resident") is False
             else _lib.CONVIVA_ROUTE_AUTO)
    _lib.check(
        _L().ssspy_conviva_statistics(ptr(X), ptr(phi), ptr(Sigma), ptr(G) if L else None, B, M, F, T,
                                      K, int(delay), float(diagonal_loading), ptr(info), ptr(failed),
                                      ptr(Rb), ptr(U) if L else None, route, _st()),
        "conviva_statistics",
    )
    return (Sigma, G, failed, Rb, U) if want_statistics else (Sigma, G, failed)


def conviva_statistics_nmf(X, basis, activation, domain, taps, delay, diagonal_loading, info,
                           want_statistics=False, Sigma=None, G=None, failed=None):
    """conviva_statistics with the weights of the ILRMA source model, formed in the kernel from basis
    (B, M, F, n_basis) and activation (B, M, n_basis, T): phi = (basis activation)^(-2 / domain).
    Returns (Sigma, G, failed), with ``want_statistics`` (Sigma, G, failed, Rb, U, phi (B, M, F, T))."""
    B, M, F, T = X.shape
    K = int(taps)
    L, Lb = K * M, (K + 1) * M
    Kb = basis.shape[-1]
    assert tuple(basis.shape) == (B, M, F, Kb) and basis.dtype == dv.f64
    assert tuple(activation.shape) == (B, M, Kb, T) and activation.dtype == dv.f64
    if Sigma is None:
        Sigma = dv.zeros((B, F, M, M, M), dv.c128, X.device)
    if G is None:
        G = dv.zeros((B, F, M, L, M), dv.c128, X.device)
    if failed is None:
        failed = dv.zeros((B, F, M), dv.i32, X.device)
    Rb = U = phi = None
    if want_statistics:
        Rb = dv.zeros((B, F, M, Lb, Lb), dv.c128, X.device)
        U = dv.zeros((B, F, M, L, L), dv.c128, X.device)
        phi = dv.zeros((B, M, F, T), dv.f64, X.device)
    route = (_lib.CONVIVA_ROUTE_STREAMING if _routes.get("conviva_resident") is False
             else _lib.CONVIVA_ROUTE_AUTO)
    _lib.check(
        _L().ssspy_conviva_statistics_nmf(ptr(X), ptr(basis), ptr(activation), ptr(Sigma),
                                          ptr(G) if L else None, B, M, F, T, K, int(delay), int(Kb),
                                          float(domain), float(diagonal_loading), ptr(info),
                                          ptr(failed), ptr(Rb), ptr(U) if L else None, ptr(phi),
                                          route, _st()),
        "conviva_statistics_nmf",
    )
    return (Sigma, G, failed, Rb, U, phi) if want_statistics else (Sigma, G, failed)


def convilrma_normalize(Y, W, basis, taps, domain, flooring):
    """Y (B, M, F, T), the rows of W (B, F, M, (taps + 1) M) and basis (B, M, F, n_basis) divided by
    psi_n = floor(sqrt(mean |y_n|^2)) (the basis by psi_n^domain), in place."""
    B, M, F, T = Y.shape
    K = int(taps)
    assert tuple(W.shape) == (B, F, M, (K + 1) * M) and tuple(basis.shape[:3]) == (B, M, F)
    ws, ws_bytes = _scratch(_L().ssspy_convilrma_normalize_workspace_bytes(B, M, F), Y.device)
    _lib.check(
        _L().ssspy_convilrma_normalize(ptr(Y), ptr(W), ptr(basis), B, M, F, T, K, basis.shape[-1],
                                       float(domain), flooring[0], flooring[1], ptr(ws), ws_bytes,
                                       _st()),
        "convilrma_normalize",
    )


def conviva_compose(Q, G, W, taps, failed=None):
    """W (B, F, M, (taps + 1) M) from the demixing rows Q (B, F, M, M) and G (B, F, M, taps M, M);
    rows of triples whose ``failed`` word has bit 0 set stay as they are."""
    B, F, M, _ = Q.shape
    K = int(taps)
    assert tuple(W.shape) == (B, F, M, (K + 1) * M) and tuple(G.shape) == (B, F, M, K * M, M)
    _lib.check(_L().ssspy_conviva_compose(ptr(Q), ptr(G) if K else None, ptr(W), ptr(failed), B, M, F,
                                          K, _st()), "conviva_compose")
    return W


# ------------------------------------------------------------------------------ time-domain ICA
def ica_chunk_samples(N, T):
    """Samples per partial record of the statistics pass (a function of the shape only)."""
    return int(_L().ssspy_ica_chunk_samples(int(N), int(T)))


def ica_workspace(B, N, T, dev):
    """(buffer, bytes) for the records of ``ica_stats`` on a (B, N, T) problem."""
    nbytes = int(_L().ssspy_ica_workspace_bytes(int(B), int(N), int(T)))
    if nbytes == 0:
        raise ValueError("ica_workspace: bad shape ({}, {}, {})".format(B, N, T))
    return _workspace(nbytes, dev)


def ica_stats(X, W, ws, kind, right, phi=None, dphi=None):
    """The statistics pass on X (B, N, T) f64 with the filters W (B, N, N): one record per (mixture,
    chunk) into ``ws`` = (buffer, bytes).  ``phi`` / ``dphi`` (B, N, T): only with ICA_GIVEN."""
    B, N, T = X.shape
    assert tuple(W.shape) == (B, N, N)
    assert phi is None or tuple(phi.shape) == (B, N, T)
    assert dphi is None or tuple(dphi.shape) == (B, N, T)
    _lib.check(_L().ssspy_ica_stats(ptr(X), ptr(W), ptr(phi), ptr(dphi), ptr(ws[0]), ws[1], B, N, T,
                                    int(kind), int(right), _st()), "ica_stats")


def ica_step(ws, W, T, algorithm, holonomic=False, step_size=0.0, loss_data=None, logdet=None,
             means=None, info=None):
    """Fold the records of ``ws`` and update W (B, N, N) in place by ``algorithm``; the loss terms of
    the state the records were formed from go to ``loss_data`` / ``logdet`` (B,), the folded record
    over T to ``means`` (B, N N + 2 N)."""
    B, N = W.shape[0], W.shape[1]
    _lib.check(_L().ssspy_ica_step(ptr(ws[0]), ws[1], ptr(W), B, N, int(T), int(algorithm),
                                   int(bool(holonomic)), float(step_size), ptr(loss_data),
                                   ptr(logdet), ptr(means), ptr(info), _st()), "ica_step")
    return W


def ica_separate(X, W, out=None):
    """Y (B, N, T) = W (B, N, N) X (B, N, T), real f64."""
    B, N, T = X.shape
    assert tuple(W.shape) == (B, N, N)
    if out is None:
        out = dv.empty((B, N, T), dv.f64, X.device)
    _lib.check(_L().ssspy_ica_separate(ptr(X), ptr(W), ptr(out), B, N, T, _st()), "ica_separate")
    return out


# ------------------------------------------------------------------------------ PDSBSS
def prox_neg_logdet(X, step_size, out=None):
    """prox of -step_size log|det| of the matrices X (..., N, N), a device tensor."""
    N = X.shape[-1]
    if out is None:
        out = dv.empty(tuple(X.shape), dv.c128, X.device)
    _lib.check(_L().ssspy_prox_neg_logdet(ptr(X), ptr(out), X.numel() // (N * N), N,
                                          float(step_size), _st()), "prox_neg_logdet")
    return out


def pdsbss_contract(dual, X, out=None):
    """XY (B, F, N, N) = (sum_q dual_q) X^H per bin; dual (B, Q, N, F, T)."""
    B, Q, N, F, T = dual.shape
    assert tuple(X.shape) == (B, N, F, T)
    if out is None:
        out = dv.empty((B, F, N, N), dv.c128, X.device)
    _lib.check(_L().ssspy_pdsbss_contract(ptr(dual), ptr(X), ptr(out), B, Q, N, F, T, _st()),
               "pdsbss_contract")
    return out


def pdsbss_filter_step(W, XY, W2, mu1, mu2, relaxation):
    """Wt = prox(W - mu1 mu2 XY, mu1), W2 = 2 Wt - W, W <- relaxed, in place; all (B, F, N, N)."""
    B, F, N, _ = W.shape
    assert tuple(XY.shape) == tuple(W2.shape) == (B, F, N, N)
    _lib.check(_L().ssspy_pdsbss_filter_step(ptr(W), ptr(XY), ptr(W2), B, F, N, float(mu1),
                                             float(mu2), float(relaxation), _st()),
               "pdsbss_filter_step")
    return W


def _dual_slice(dual, q):
    """(pointer to penalty q of the dual variable, elements between mixtures, (B, N, F, T))."""
    B, Q, N, F, T = dual.shape
    assert dual.is_contiguous()
    return dual.data_ptr() + 16 * q * N * F * T, Q * N * F * T, (B, N, F, T)


def pdsbss_bin_norms(X, W2, dual, q, out=None):
    """r2 (B, N, T): sum over bins of |dual_q + W2 x|^2."""
    dq, stride, (B, N, F, T) = _dual_slice(dual, q)
    if out is None:
        out = dv.empty((B, N, T), dv.f64, X.device)
    ws, ws_bytes = _scratch(_L().ssspy_pdsbss_bin_norms_workspace_bytes(B, N, F, T), X.device)
    _lib.check(_L().ssspy_pdsbss_bin_norms(ptr(X), ptr(W2), dq, stride, ptr(out), B, N, F, T,
                                           ptr(ws), ws_bytes, _st()), "pdsbss_bin_norms")
    return out


def pdsbss_dual_step(X, W2, dual, q, kind, step_size, relaxation, r2=None, aux=None):
    """dual_q <- relaxation (Z - prox(Z)) + (1 - relaxation) dual_q in place, by _lib.PROX_*."""
    dq, stride, (B, N, F, T) = _dual_slice(dual, q)
    assert aux is None or tuple(aux.shape) == (B, N, F, T)
    assert r2 is None or tuple(r2.shape) == (B, N, T)
    _lib.check(_L().ssspy_pdsbss_dual_step(ptr(X), ptr(W2), dq, stride, int(kind), float(step_size),
                                           float(relaxation), ptr(r2), ptr(aux), B, N, F, T, _st()),
               "pdsbss_dual_step")
    return dual


def pdsbss_form_z(X, W2, dual, q, out=None):
    """Z = dual_q + W2 x, (B, N, F, T)."""
    dq, stride, (B, N, F, T) = _dual_slice(dual, q)
    if out is None:
        out = dv.empty((B, N, F, T), dv.c128, X.device)
    _lib.check(_L().ssspy_pdsbss_form_z(ptr(X), ptr(W2), dq, stride, ptr(out), B, N, F, T, _st()),
               "pdsbss_form_z")
    return out


# ------------------------------------------------------------------------------ ADMMBSS
def admmbss_gram_inverse(X, Q, out=None):
    """Ainv (B, F, N, N) = (Q conj(X) X^T + I)^-1 per bin."""
    B, N, F, T = X.shape
    if out is None:
        out = dv.empty((B, F, N, N), dv.c128, X.device)
    _lib.check(_L().ssspy_admmbss_gram_inverse(ptr(X), ptr(out), B, int(Q), N, F, T, _st()),
               "admmbss_gram_inverse")
    return out


def admmbss_contract(aux2, dual2, X, out=None):
    """R (B, F, N, N) = (sum_q (aux2_q - dual2_q)) X^H per bin; aux2, dual2 (B, Q, N, F, T)."""
    B, Q, N, F, T = aux2.shape
    assert tuple(dual2.shape) == (B, Q, N, F, T) and tuple(X.shape) == (B, N, F, T)
    assert aux2.is_contiguous() and dual2.is_contiguous()
    if out is None:
        out = dv.empty((B, F, N, N), dv.c128, X.device)
    _lib.check(_L().ssspy_admmbss_contract(ptr(aux2), ptr(dual2), ptr(X), ptr(out), B, Q, N, F, T,
                                           _st()), "admmbss_contract")
    return out


def admmbss_filter_step(Ainv, R, W, aux1, dual1, rho, relaxation):
    """W = Ainv (aux1 - dual1 + R), U = relaxation W + (1 - relaxation) aux1,
    aux1 <- prox.neg_logdet(U + dual1, 1 / rho), dual1 <- dual1 + U - aux1; all (B, F, N, N)."""
    B, F, N, _ = W.shape
    for t in (Ainv, R, aux1, dual1):
        assert tuple(t.shape) == (B, F, N, N) and t.is_contiguous()
    _lib.check(_L().ssspy_admmbss_filter_step(ptr(Ainv), ptr(R), ptr(W), ptr(aux1), ptr(dual1), B, F,
                                              N, float(rho), float(relaxation), _st()),
               "admmbss_filter_step")
    return W


def _admm_slices(aux2, dual2, q):
    assert tuple(aux2.shape) == tuple(dual2.shape)
    aq, stride, shape = _dual_slice(aux2, q)
    dq, _, _ = _dual_slice(dual2, q)
    return aq, dq, stride, shape


def admmbss_bin_norms(X, W, aux2, dual2, q, relaxation, out=None):
    """r2 (B, N, T): sum over bins of |relaxation W x + (1 - relaxation) aux2_q + dual2_q|^2."""
    aq, dq, stride, (B, N, F, T) = _admm_slices(aux2, dual2, q)
    if out is None:
        out = dv.empty((B, N, T), dv.f64, X.device)
    ws, ws_bytes = _scratch(_L().ssspy_admmbss_bin_norms_workspace_bytes(B, N, F, T), X.device)
    _lib.check(_L().ssspy_admmbss_bin_norms(ptr(X), ptr(W), aq, dq, stride, float(relaxation),
                                            ptr(out), B, N, F, T, ptr(ws), ws_bytes, _st()),
               "admmbss_bin_norms")
    return out


def admmbss_aux_step(X, W, aux2, dual2, q, kind, step_size, relaxation, r2=None, given=None):
    """aux2_q <- prox(Z, step_size) by _lib.PROX_*, dual2_q <- Z - aux2_q, in place."""
    aq, dq, stride, (B, N, F, T) = _admm_slices(aux2, dual2, q)
    assert given is None or tuple(given.shape) == (B, N, F, T)
    assert r2 is None or tuple(r2.shape) == (B, N, T)
    _lib.check(_L().ssspy_admmbss_aux_step(ptr(X), ptr(W), aq, dq, stride, int(kind),
                                           float(step_size), float(relaxation), ptr(r2), ptr(given),
                                           B, N, F, T, _st()), "admmbss_aux_step")
    return aux2, dual2


def admmbss_form_z(X, W, aux2, dual2, q, relaxation, out=None):
    """Z = relaxation W x + (1 - relaxation) aux2_q + dual2_q, (B, N, F, T)."""
    aq, dq, stride, (B, N, F, T) = _admm_slices(aux2, dual2, q)
    if out is None:
        out = dv.empty((B, N, F, T), dv.c128, X.device)
    _lib.check(_L().ssspy_admmbss_form_z(ptr(X), ptr(W), aq, dq, stride, float(relaxation), ptr(out),
                                         B, N, F, T, _st()), "admmbss_form_z")
    return out


# ------------------------------------------------------------------------------ HVA
def hva_route(F, route=_lib.HVA_ROUTE_AUTO):
    """The transform route (_lib.HVA_ROUTE_FFT / _DIRECT) the cepstral pass takes for F bins when
    asked for ``route``.  Host only."""
    got = int(_L().ssspy_hva_route(int(F), int(route)))
    if got < 0:
        raise ValueError("hva_route: no such route for {} bins".format(F))
    return got


def hva_cos_table(F, dev):
    """cos(pi j / (F - 1)), j < 2 (F - 1): the table both transform routes read."""
    table = dv.empty((2 * (F - 1),), dv.f64, dev)
    _lib.check(_L().ssspy_hva_cos_table(ptr(table), int(F), _st()), "hva_cos_table")
    return table


def hva_cepstrum(X, W2, dual, q, table, flooring, mask_iter, route=_lib.HVA_ROUTE_AUTO, out=None):
    """varrho (B, N, F, T) f64 of Z = dual_q + W2 x: the log-magnitude after the cosine shrinkage
    of its cepstrum along the bins (see the header)."""
    dq, stride, (B, N, F, T) = _dual_slice(dual, q)
    assert tuple(table.shape) == (2 * (F - 1),)
    if out is None:
        out = dv.empty((B, N, F, T), dv.f64, X.device)
    assert tuple(out.shape) == (B, N, F, T)
    _lib.check(_L().ssspy_hva_cepstrum(ptr(X), ptr(W2), dq, stride, ptr(table), ptr(out), B, N, F, T,
                                       flooring[0], float(flooring[1]), int(mask_iter), int(route),
                                       _st()), "hva_cepstrum")
    return out


def hva_dual_step(X, W2, dual, q, varrho, attenuation, relaxation):
    """dual_q <- relaxation (Z - mask Z) + (1 - relaxation) dual_q in place, the mask the softmax of
    2 varrho over sources to the power ``attenuation``."""
    dq, stride, (B, N, F, T) = _dual_slice(dual, q)
    assert tuple(varrho.shape) == (B, N, F, T)
    _lib.check(_L().ssspy_hva_dual_step(ptr(X), ptr(W2), dq, stride, ptr(varrho), float(attenuation),
                                        float(relaxation), B, N, F, T, _st()), "hva_dual_step")
    return dual


def hva_admm_cepstrum(X, W, aux2, dual2, q, table, flooring, mask_iter, relaxation,
                      route=_lib.HVA_ROUTE_AUTO, out=None):
    """varrho (B, N, F, T) f64 of Z = relaxation W x + (1 - relaxation) aux2_q + dual2_q: the pass of
    ``hva_cepstrum`` on ADMM's operand (aux2_q is not read at relaxation 1)."""
    aq, dq, stride, (B, N, F, T) = _admm_slices(aux2, dual2, q)
    assert tuple(table.shape) == (2 * (F - 1),)
    if out is None:
        out = dv.empty((B, N, F, T), dv.f64, X.device)
    assert tuple(out.shape) == (B, N, F, T)
    _lib.check(_L().ssspy_hva_admm_cepstrum(ptr(X), ptr(W), aq, dq, stride, ptr(table), ptr(out), B, N,
                                            F, T, float(relaxation), flooring[0], float(flooring[1]),
                                            int(mask_iter), int(route), _st()), "hva_admm_cepstrum")
    return out


def hva_aux_step(X, W, aux2, dual2, q, varrho, attenuation, relaxation):
    """aux2_q <- mask Z, dual2_q <- Z - aux2_q in place with Z as in ``hva_admm_cepstrum`` and the mask
    of ``hva_dual_step``."""
    aq, dq, stride, (B, N, F, T) = _admm_slices(aux2, dual2, q)
    assert tuple(varrho.shape) == (B, N, F, T)
    _lib.check(_L().ssspy_hva_aux_step(ptr(X), ptr(W), aq, dq, stride, ptr(varrho), float(attenuation),
                                       float(relaxation), B, N, F, T, _st()), "hva_aux_step")
    return aux2, dual2


# --------------------------------------------------------------- FastIVA / FasterIVA, whitening
def fast_iva_weights(r2, d_contrast, dd_contrast, flooring, want_psi=True):
    """(phi, psi) (B, N, T) from the frame powers and the closures' values on the norms; psi None
    unless ``want_psi``."""
    B, N, T = r2.shape
    phi = dv.empty((B, N, T), dv.f64, r2.device)
    psi = dv.empty((B, N, T), dv.f64, r2.device) if want_psi else None
    _lib.check(_L().ssspy_fast_iva_weights(ptr(r2), ptr(d_contrast), ptr(dd_contrast), ptr(phi),
                                           ptr(psi), B, N, T, flooring[0], flooring[1], _st()),
               "fast_iva_weights")
    return phi, psi


def fast_iva_stats(Z, W, phi, psi):
    """(c (B, F, N, N), b (B, F, N), a (B, F, N)): the moments of the FastIVA update, one pass over Z."""
    B, N, F, T = Z.shape
    c = dv.empty((B, F, N, N), dv.c128, Z.device)
    b = dv.empty((B, F, N), dv.f64, Z.device)
    a = dv.empty((B, F, N), dv.f64, Z.device)
    _lib.check(_L().ssspy_fast_iva_stats(ptr(Z), ptr(W), ptr(phi), ptr(psi), ptr(c), ptr(b), ptr(a),
                                         B, N, F, T, _st()), "fast_iva_stats")
    return c, b, a


def fast_iva_step(W, c, b, a, n_frames, info=None):
    B, F, N, _ = W.shape
    _lib.check(_L().ssspy_fast_iva_step(ptr(W), ptr(c), ptr(b), ptr(a), B, F, N, int(n_frames),
                                        ptr(info), _st()), "fast_iva_step")
    return W


def faster_iva_step(W, U, info=None):
    B, F, N, _ = W.shape
    assert tuple(U.shape) == (B, F, N, N, N)
    _lib.check(_L().ssspy_faster_iva_step(ptr(W), ptr(U), B, F, N, ptr(info), _st()),
               "faster_iva_step")
    return W


def orthonormalize_rows(W, info=None):
    """W <- (W W^H)^-1/2 W per bin, in place; (B, F, N, N)."""
    B, F, N, _ = W.shape
    _lib.check(_L().ssspy_orthonormalize_rows(ptr(W), B, F, N, ptr(info), _st()),
               "orthonormalize_rows")
    return W


def whitening_filter(C, mode=_lib.WHITEN, info=None, out=None):
    """P (B, F, N, N) with ssspy_separate(X, P) the whitened / PCA-rotated X; C (B, F, N, N)."""
    B, F, N, _ = C.shape
    if out is None:
        out = dv.empty((B, F, N, N), dv.c128, C.device)
    _lib.check(_L().ssspy_whitening_filter(ptr(C), ptr(out), B, F, N, int(mode), ptr(info), _st()),
               "whitening_filter")
    return out


def whitened(X, info=None):
    """Z (B, N, F, T) = P X with mean_j z z^H = I per bin.  The filter from the eigen-decomposition of
    C = mean_j x x^H leaves mean_j z z^H = I only to eps cond(C) (the rounding of C itself, seen
    through Lambda^-1/2), so one correction follows: the covariance D of the first Z, which is
    well conditioned, and P <- D^-1/2 P with the Hermitian inverse square root -- it rotates
    nothing, so the rows keep the eigenvectors' order and phase."""
    B, N, F, T = X.shape
    C = weighted_covariance(X).reshape(B, F, N, N)
    P = whitening_filter(C, _lib.WHITEN, info)
    D = weighted_covariance(separate(X, P)).reshape(B, F, N, N)
    R = dv.empty((B, F, N, N), dv.c128, X.device)
    _lib.check(_L().ssspy_sqrtmh(ptr(D), ptr(R), B * F, N, 1, _lib.FLOOR_NONE, 0.0, _st()), "sqrtmh")
    return separate(X, compose_filters(R, P, D))


# ----------------------------------------------------------------------------- FastMNMF
def fastmnmf_workspace(B, N, M, F, T, K, dev):
    return _workspace(_L().ssspy_fastmnmf_workspace_bytes(B, N, M, F, T, K), dev)


def fastmnmf_route(B, N, M, F, T, K, handover=False):
    """(route, plan): the _lib.MNMF_ROUTE_* kernel family of the FastGaussMNMF entry points for this
    shape and, for the tiled family, what its launchers decide, as a dict over
    _lib.MNMF_PLAN_FIELDS (see ssspy_fastmnmf_route in the header).  Host only."""
    import ctypes

    plan = (ctypes.c_int * len(_lib.MNMF_PLAN_FIELDS))()
    route = int(_L().ssspy_fastmnmf_route(B, N, M, F, T, K, 1 if handover else 0, plan))
    if route < 0:
        raise ValueError("fastmnmf_route: bad shape")
    return route, dict(zip(_lib.MNMF_PLAN_FIELDS, (int(v) for v in plan)))


def fastmnmf_update(X, C, Q, D, basis, activation, steps, flooring, ws, ws_bytes, info):
    B, M, F, T = X.shape
    N, K = basis.shape[1], basis.shape[-1]
    _lib.check(
        _L().ssspy_fastmnmf_update(ptr(X), ptr(C), ptr(Q), ptr(D), ptr(basis), ptr(activation), B,
                                   N, M, F, T, K, steps, flooring[0], flooring[1], ptr(ws),
                                   ws_bytes, ptr(info), _st()),
        "fastmnmf_update",
    )


def fastmnmf_handover(B, N, M, F, T, K, dev):
    """The |Q x|^2 hand-over buffer of ssspy_fastmnmf_update_handover, or None for shapes without it."""
    n = _L().ssspy_fastmnmf_handover_doubles(B, N, M, F, T, K)
    if not n or not _routes.get("handover"):
        return None
    return _workspace(8 * n, dev)[0]


def fastmnmf_update_handover(X, C, Q, D, basis, activation, steps, flooring, ws, ws_bytes, info,
                             handover, valid):
    """`valid`: whether `handover` matches (Q, X); returns whether it does afterwards."""
    import ctypes

    B, M, F, T = X.shape
    N, K = basis.shape[1], basis.shape[-1]
    flag = ctypes.c_int(1 if valid else 0)
    _lib.check(
        _L().ssspy_fastmnmf_update_handover(
            ptr(X), ptr(C), ptr(Q), ptr(D), ptr(basis), ptr(activation), B, N, M, F, T, K, steps,
            flooring[0], flooring[1], ptr(ws), ws_bytes, ptr(info), ptr(handover),
            ctypes.cast(ctypes.pointer(flag), ctypes.c_void_p), _st()),
        "fastmnmf_update_handover",
    )
    return bool(flag.value)


def fastmnmf_deferred_logdet_slots(B, N, M, F, T, K):
    """Shares per mixture ``fastmnmf_update_logdet`` leaves in ``logdet``."""
    return int(_L().ssspy_fastmnmf_deferred_logdet_slots(B, N, M, F, T, K))


def fastmnmf_update_logdet(X, C, Q, D, basis, activation, steps, flooring, ws, ws_bytes, info,
                           handover, valid, logdet, logdet_stride):
    """fastmnmf_update(_handover) that also leaves sum_i log|det Q_i| of the diagonalisers as they
    come in, as shares at logdet[s * logdet_stride + b] (the caller zeroes the array once per run
    and folds it once).  handover None: no hand-over buffer.  Returns the buffer's validity."""
    import ctypes

    B, M, F, T = X.shape
    N, K = basis.shape[1], basis.shape[-1]
    flag = ctypes.c_int(1 if valid else 0)
    _lib.check(
        _L().ssspy_fastmnmf_update_handover_logdet(
            ptr(X), ptr(C), ptr(Q), ptr(D), ptr(basis), ptr(activation), B, N, M, F, T, K, steps,
            flooring[0], flooring[1], ptr(ws), ws_bytes, ptr(info), ptr(handover),
            ctypes.cast(ctypes.pointer(flag), ctypes.c_void_p) if handover is not None else None,
            ptr(logdet), int(logdet_stride), _st()),
        "fastmnmf_update_handover_logdet",
    )
    return bool(flag.value) if handover is not None else False


def fastmnmf_diagonalizer_covariance(X, D, basis, activation, out=None, ws=None, ws_bytes=0):
    """ws (the separator's fastmnmf_workspace): the tuned covariance pass instead of the generic one."""
    B, M, F, T = X.shape
    N, K = basis.shape[1], basis.shape[-1]
    if out is None:
        out = dv.empty((B, F, M, M, M), dv.c128, X.device)
    _lib.check(
        _L().ssspy_fastmnmf_diagonalizer_covariance(ptr(X), ptr(D), ptr(basis), ptr(activation),
                                                    ptr(out), B, N, M, F, T, K, ptr(ws),
                                                    int(ws_bytes), _st()),
        "fastmnmf_diagonalizer_covariance",
    )
    return out


def fastmnmf_weights(X, Q, D, basis, activation, out=None):
    """1 / R~ per (channel, bin, frame), (B, M, F, T): the weights of the diagonaliser covariance."""
    B, M, F, T = X.shape
    N, K = basis.shape[1], basis.shape[-1]
    if out is None:
        out = dv.empty((B, M, F, T), dv.f64, X.device)
    _lib.check(
        _L().ssspy_fastmnmf_weights(ptr(X), ptr(Q), ptr(D), ptr(basis), ptr(activation), ptr(out), B,
                                    N, M, F, T, K, _st()),
        "fastmnmf_weights",
    )
    return out


def fastmnmf_loss_data(X, Q, D, basis, activation, out=None):
    B, M, F, T = X.shape
    N, K = basis.shape[1], basis.shape[-1]
    if out is None:
        out = dv.empty((B,), dv.f64, X.device)
    ws, ws_bytes = _scratch(_L().ssspy_fastmnmf_loss_workspace_bytes(B, N, M, F, T), X.device)
    _lib.check(
        _L().ssspy_fastmnmf_loss_data(ptr(X), ptr(Q), ptr(D), ptr(basis), ptr(activation), ptr(out),
                                      B, N, M, F, T, K, ptr(ws), ws_bytes, _st()),
        "fastmnmf_loss_data",
    )
    return out


def fastmnmf_loss_data_handover(D, basis, activation, handover, n_channels, n_frames, out=None):
    """Data term of the loss from a valid |Q x|^2 hand-over (see fastmnmf_update_handover)."""
    B, N, F, K = basis.shape
    if out is None:
        out = dv.empty((B,), dv.f64, basis.device)
    ws, ws_bytes = _scratch(
        _L().ssspy_fastmnmf_loss_workspace_bytes(B, N, n_channels, F, n_frames), basis.device)
    _lib.check(
        _L().ssspy_fastmnmf_loss_data_handover(ptr(D), ptr(basis), ptr(activation), ptr(handover),
                                               ptr(out), B, N, n_channels, F, n_frames, K, ptr(ws),
                                               ws_bytes, _st()),
        "fastmnmf_loss_data_handover",
    )
    return out


def fastmnmf_loss_handover_slots(B, N, M, F, T, K):
    """Shares per mixture ``fastmnmf_loss_data_handover_slots`` writes (0: no hand-over)."""
    return int(_L().ssspy_fastmnmf_loss_handover_slots(B, N, M, F, T, K))


def fastmnmf_loss_data_handover_slots(D, basis, activation, handover, n_channels, n_frames, slots,
                                      slot_stride):
    """fastmnmf_loss_data_handover with the per-wave shares left raw (share s of mixture b at
    slots[s * slot_stride + b]); the caller zeroes the array once per run and folds it once."""
    B, N, F, K = basis.shape
    _lib.check(
        _L().ssspy_fastmnmf_loss_data_handover_slots(
            ptr(D), ptr(basis), ptr(activation), ptr(handover), ptr(slots), int(slot_stride), B, N,
            n_channels, F, n_frames, K, _st()),
        "fastmnmf_loss_data_handover_slots",
    )


def fastmnmf_separate(X, Q, D, basis, activation, reference_id, flooring, ws, ws_bytes, info,
                      out=None):
    B, M, F, T = X.shape
    N, K = basis.shape[1], basis.shape[-1]
    if out is None:
        out = dv.empty((B, N, F, T), dv.c128, X.device)
    _lib.check(
        _L().ssspy_fastmnmf_separate(ptr(X), ptr(Q), ptr(D), ptr(basis), ptr(activation), ptr(out),
                                     B, N, M, F, T, K, reference_id, flooring[0], flooring[1],
                                     ptr(ws), ws_bytes, ptr(info), _st()),
        "fastmnmf_separate",
    )
    return out


_HOST_FLOOR_EIG_BYTES = 1 << 28  # eigenvector scratch of fastmnmf_separate_host_floor


def fastmnmf_separate_host_floor(X, Q, D, basis, activation, reference_id, host_fn, ws, ws_bytes,
                                 info, out=None):
    """The Wiener filter with an arbitrary flooring callable on the eigenvalues of R_ij: stage 1
    leaves ascending eigenvalues (B, F, T, M) and eigenvectors in HBM, the callable runs on the host
    on each mixture's (F, T, M) array -- what to_psd hands it in the reference (special/psd.py:54-62)
    -- and stage 2 finishes from the floored values."""
    B, M, F, T = X.shape
    N, K = basis.shape[1], basis.shape[-1]
    if out is None:
        out = dv.empty((B, N, F, T), dv.c128, X.device)
    # a few mixtures at a time: the eigenvectors of every point are (F, T, M, M) complex128 per
    # mixture (34 MB at 4 channels of 513 x 256, 1 GB for 32 of them), the buffers are reused
    per = F * T * M * M * 16
    cb = max(1, min(B, _HOST_FLOOR_EIG_BYTES // per))
    lam = dv.empty((cb, F, T, M), dv.f64, X.device)
    P = dv.empty((cb, F, T, M, M), dv.c128, X.device)
    for b0 in range(0, B, cb):
        n = min(cb, B - b0)
        sl = slice(b0, b0 + n)
        for stage in (1, 2):
            _lib.check(
                _L().ssspy_fastmnmf_separate_eig(ptr(X[sl]), ptr(Q[sl]), ptr(D[sl]), ptr(basis[sl]),
                                                 ptr(activation[sl]), ptr(out[sl]), n, N, M, F, T, K,
                                                 reference_id, stage, ptr(lam), ptr(P), ptr(ws),
                                                 ws_bytes, ptr(info), _st()),
                "fastmnmf_separate_eig",
            )
            if stage == 1:
                lam[:n].copy_(dv.to_device(_apply_host(host_fn, lam[:n]), dev=X.device))
    return out


# ------------------------------------------------------------------------- GaussMNMF
def gmnmf_workspace(B, N, M, F, T, K, dev):
    return _workspace(_L().ssspy_gmnmf_workspace_bytes(B, N, M, F, T, K), dev)


def gmnmf_route(B, N, M, F, T, K, partitioning=False):
    """What the launchers of the GaussMNMF entry points decide for this shape, as a dict over
    _lib.GMNMF_PLAN_FIELDS (see ssspy_gmnmf_route in the header).  Host only; ValueError for a shape
    the entry points reject."""
    import ctypes

    plan = (ctypes.c_int * len(_lib.GMNMF_PLAN_FIELDS))()
    if int(_L().ssspy_gmnmf_route(B, N, M, F, T, K, 1 if partitioning else 0, plan)) < 0:
        raise ValueError("gmnmf_route: shape rejected")
    return dict(zip(_lib.GMNMF_PLAN_FIELDS, (int(v) for v in plan)))


def gmnmf_update(X, basis, activation, spatial, steps, flooring, ws, ws_bytes, latent=None):
    B, M, F, T = X.shape
    N, K = spatial.shape[1], basis.shape[-1]
    _lib.check(
        _L().ssspy_gmnmf_update(ptr(X), ptr(basis), ptr(activation), ptr(latent), ptr(spatial), B,
                                N, M, F, T, K, steps, flooring[0], flooring[1], ptr(ws), ws_bytes,
                                _st()),
        "gmnmf_update",
    )


def gmnmf_loss(X, basis, activation, spatial, flooring, out=None):
    B, M, F, T = X.shape
    N, K = basis.shape[1], basis.shape[-1]
    if out is None:
        out = dv.empty((B,), dv.f64, X.device)
    ws, ws_bytes = _scratch(_L().ssspy_gmnmf_loss_workspace_bytes(B, F, T), X.device)
    _lib.check(
        _L().ssspy_gmnmf_loss(ptr(X), ptr(basis), ptr(activation), ptr(spatial), ptr(out), B, N, M,
                              F, T, K, flooring[0], flooring[1], ptr(ws), ws_bytes, _st()),
        "gmnmf_loss",
    )
    return out


def gmnmf_separate(X, basis, activation, spatial, reference_id, flooring, out=None):
    B, M, F, T = X.shape
    N, K = basis.shape[1], basis.shape[-1]
    if out is None:
        out = dv.empty((B, N, F, T), dv.c128, X.device)
    _lib.check(
        _L().ssspy_gmnmf_separate(ptr(X), ptr(basis), ptr(activation), ptr(spatial), ptr(out), B,
                                  N, M, F, T, K, int(reference_id), flooring[0], flooring[1],
                                  _st()),
        "gmnmf_separate",
    )
    return out


# ----------------------------------------------------------------------------- cACGMM
def cacgmm_unit_input(X, flooring):
    """Z = X / floor(||x||_2) per (bin, frame); X (B, M, F, T)."""
    B, M, F, T = X.shape
    Z = dv.empty((B, M, F, T), dv.c128, X.device)
    _lib.check(_L().ssspy_cacgmm_unit_input(ptr(X), ptr(Z), B, M, F, T, int(flooring[0]),
                                            float(flooring[1]), _st()), "cacgmm_unit_input")
    return Z


def cacgmm_prepare(covariance, mixing, info=None, binv=None, logp=None):
    """(binv, logp): the packed inverse covariances (B, N, F, M * M) and log mixing - log det
    covariance (B, N, F) that ``cacgmm_frame_pass`` stages."""
    B, N, F, M, _ = covariance.shape
    assert tuple(mixing.shape) == (B, N, F)
    if binv is None:
        binv = dv.empty((B, N, F, M * M), dv.f64, covariance.device)
    if logp is None:
        logp = dv.empty((B, N, F), dv.f64, covariance.device)
    _lib.check(_L().ssspy_cacgmm_prepare(ptr(covariance), ptr(mixing), ptr(binv), ptr(logp), B, N, F,
                                         M, ptr(info), _st()), "cacgmm_prepare")
    return binv, logp


def cacgmm_frame_pass(Z, binv, logp, flooring, sum_gamma=None, num=None, loss=None, posterior=None,
                      posterior_in=None):
    """One pass over the unit mixture Z (B, M, F, T) with the staged parameters: whichever of
    sum_gamma (B, N, F), num (B, N, F, M, M) (the two together), loss (B, F) and posterior
    (B, N, F, T) are given are filled.  ``posterior_in``: posteriors the sums take instead of the
    pass's own."""
    B, M, F, T = Z.shape
    N = logp.shape[1]
    assert tuple(binv.shape) == (B, N, F, M * M) and tuple(logp.shape) == (B, N, F)
    assert sum_gamma is None or tuple(sum_gamma.shape) == (B, N, F)
    assert num is None or tuple(num.shape) == (B, N, F, M, M)
    assert loss is None or tuple(loss.shape) == (B, F)
    assert posterior is None or tuple(posterior.shape) == (B, N, F, T)
    assert posterior_in is None or tuple(posterior_in.shape) == (B, N, F, T)
    _lib.check(_L().ssspy_cacgmm_frame_pass(ptr(Z), ptr(binv), ptr(logp), B, M, N, F, T,
                                            int(flooring[0]), float(flooring[1]), ptr(sum_gamma),
                                            ptr(num), ptr(loss), ptr(posterior), ptr(posterior_in),
                                            _st()),
               "cacgmm_frame_pass")


def cacgmm_parameter_step(sum_gamma, num, n_frames, flooring, normalize, mixing=None, covariance=None):
    """(mixing, covariance) from the sums of a frame pass; ``num`` is overwritten."""
    B, N, F, M, _ = num.shape
    if mixing is None:
        mixing = dv.empty((B, N, F), dv.f64, num.device)
    if covariance is None:
        covariance = dv.empty((B, N, F, M, M), dv.c128, num.device)
    _lib.check(_L().ssspy_cacgmm_parameter_step(ptr(sum_gamma), ptr(num), ptr(mixing), ptr(covariance),
                                                B, N, F, M, int(n_frames), int(flooring[0]),
                                                float(flooring[1]), int(bool(normalize)), _st()),
               "cacgmm_parameter_step")
    return mixing, covariance


def cacgmm_normalize(covariance):
    """covariance / Re tr covariance, in place; (B, N, F, M, M)."""
    B, N, F, M, _ = covariance.shape
    _lib.check(_L().ssspy_cacgmm_normalize(ptr(covariance), B, N, F, M, _st()), "cacgmm_normalize")
    return covariance


def cacgmm_fold_loss(terms, out=None):
    """out[...] = sum over the last axis of ``terms`` in a fixed order."""
    F = terms.shape[-1]
    rows = terms.numel() // F
    if out is None:
        out = dv.empty(tuple(terms.shape[:-1]), dv.f64, terms.device)
    _lib.check(_L().ssspy_cacgmm_fold_loss(ptr(terms), ptr(out), rows, F, _st()), "cacgmm_fold_loss")
    return out


def cacgmm_separate(posterior, X, reference_id, out=None):
    """out = posterior * X[:, reference_id]; posterior (B, N, F, T), X (B, M, F, T)."""
    B, N, F, T = posterior.shape
    M = X.shape[1]
    if out is None:
        out = dv.empty((B, N, F, T), dv.c128, X.device)
    _lib.check(_L().ssspy_cacgmm_separate(ptr(posterior), ptr(X), ptr(out), B, N, M, F, T,
                                          int(reference_id), _st()), "cacgmm_separate")
    return out


# ---- permutation alignment (csrc/permutation.hip).  A sequence is a tensor indexed (b, n, f, t) with
# the frames contiguous and any strides on the other axes -- the library's (B, N, F, T), or a
# permuted view of the solvers' (B, F, N, T): nothing is copied.  perm is int32 (B, F, N).
def permutation_route(N, T, solver, flooring):
    """True where the device solver takes N sources and T frames with this floor.  Host only."""
    kind = -1 if getattr(flooring, "host", None) is not None else int(flooring[0])
    route = int(_L().ssspy_permutation_route(int(N), int(T), int(solver), kind))
    if route < 0:
        raise ValueError("permutation_route: bad argument")
    return route == _lib.PERM_ROUTE_DEVICE


def permutation_limit(N, T, solver, flooring):
    """Why ``permutation_route`` says host, in words."""
    if getattr(flooring, "host", None) is not None:
        return "flooring_fn must be None, identity, max_flooring or add_flooring, got {!r}".format(
            flooring.host)
    if N < 2 or N > _lib.MAX_SOURCES:
        return "2..{} sources, got {}".format(_lib.MAX_SOURCES, N)
    return "n_sources * n_frames <= 16384 for the correlation solver, got {} x {}".format(N, T)


def _sequence_strides(sequence, dtype_ok):
    assert sequence.ndim == 4 and sequence.dtype in dtype_ok, "bad sequence"
    if sequence.stride(3) != 1 and sequence.shape[3] > 1:
        raise ValueError("the frames of a sequence must be contiguous")
    return sequence.stride(0), sequence.stride(1), sequence.stride(2)


def best_permutation(tables):
    """Index, in ``itertools.permutations`` order, of the first permutation p maximising
    sum_i tables[m, p[i], i]; tables (n, N, N) f64 -> int32 (n,)."""
    n, N, _ = tables.shape
    out = dv.empty((n,), dv.i32, tables.device)
    _lib.check(_L().ssspy_best_permutation(ptr(tables), ptr(out), n, N, _st()), "best_permutation")
    return out


def permutation_envelope_overlap(sequence, flooring):
    """(envelope (B, F, N, T), overlap (B, F)) of a real or complex sequence (b, n, f, t)."""
    sb, sn, sf = _sequence_strides(sequence, (dv.f64, dv.c128))
    B, N, F, T = sequence.shape
    envelope = dv.empty((B, F, N, T), dv.f64, sequence.device)
    overlap = dv.empty((B, F), dv.f64, sequence.device)
    _lib.check(_L().ssspy_permutation_envelope_overlap(
        sequence.data_ptr(), int(sequence.is_complex()), sb, sn, sf, ptr(envelope), ptr(overlap), B,
        N, F, T, int(flooring[0]), float(flooring[1]), _st()), "permutation_envelope_overlap")
    return envelope, overlap


def permutation_correlation_sweep(envelope, order):
    """perm (B, F, N) of the correlation solver; order (B, F) int32: the bins as they are visited."""
    B, F, N, T = envelope.shape
    assert tuple(order.shape) == (B, F) and order.dtype == dv.i32
    perm = dv.empty((B, F, N), dv.i32, envelope.device)
    _lib.check(_L().ssspy_permutation_correlation_sweep(ptr(envelope), ptr(order), ptr(perm), B, N, F,
                                                        T, _st()), "permutation_correlation_sweep")
    return perm


def permutation_score_normalize(sequence):
    """normalized (B, F, N, T) of a real sequence (b, n, f, t)."""
    sb, sn, sf = _sequence_strides(sequence, (dv.f64,))
    B, N, F, T = sequence.shape
    normalized = dv.empty((B, F, N, T), dv.f64, sequence.device)
    _lib.check(_L().ssspy_permutation_score_normalize(sequence.data_ptr(), sb, sn, sf,
                                                      ptr(normalized), B, N, F, T, _st()),
               "permutation_score_normalize")
    return normalized


def permutation_identity(B, F, N, dev):
    """perm (B, F, N) of the sequences as they are (plumbing: a torch fill)."""
    import torch

    return torch.arange(N, dtype=dv.i32, device=dev).expand(B, F, N).contiguous()


def permutation_score_global(normalized, perm, global_iter, flooring):
    """The global stage on ``perm`` in place; returns centroid_std (B, N) of the last centroid."""
    B, F, N, T = normalized.shape
    assert tuple(perm.shape) == (B, F, N) and perm.dtype == dv.i32
    centroid = dv.empty((B, N, T), dv.f64, normalized.device)
    centroid_std = dv.empty((B, N), dv.f64, normalized.device)
    _lib.check(_L().ssspy_permutation_score_global(
        ptr(normalized), ptr(perm), ptr(centroid), ptr(centroid_std), B, N, F, T, int(global_iter),
        int(flooring[0]), float(flooring[1]), _st()), "permutation_score_global")
    return centroid_std


def permutation_score_local(normalized, centroid_std, perm, local_iter, flooring):
    """The local stage on ``perm`` in place."""
    B, F, N, T = normalized.shape
    assert tuple(perm.shape) == (B, F, N) and tuple(centroid_std.shape) == (B, N)
    _lib.check(_L().ssspy_permutation_score_local(
        ptr(normalized), ptr(centroid_std), ptr(perm), B, N, F, T, int(local_iter), int(flooring[0]),
        float(flooring[1]), _st()), "permutation_score_local")
    return perm


def permute_sources(array, perm, layout):
    """The sources of ``array`` gathered by ``perm`` into a new contiguous tensor of the same shape.
    layout PERM_LAYOUT_BIN_SOURCE: array (B, F, N, ...), PERM_LAYOUT_SOURCE_BIN: (B, N, F, ...); the
    leading three axes may be strided, the rest is contiguous; elements of 8 or 16 bytes."""
    B, F, N = perm.shape
    lead = (B, F, N) if layout == _lib.PERM_LAYOUT_BIN_SOURCE else (B, N, F)
    assert tuple(array.shape[:3]) == lead and perm.dtype == dv.i32
    words = array.element_size() // 8
    if words * 8 != array.element_size():
        raise NotImplementedError("permute_sources moves elements of 8 or 16 bytes, got {}".format(
            array.dtype))
    flat = array.reshape(lead + (-1,)) if array.ndim != 4 else array
    if flat.shape[3] > 1 and flat.stride(3) != 1:
        flat = flat.contiguous()
    inner = flat.shape[3] * words
    sb, s1, s2 = (flat.stride(k) * words for k in range(3))
    sf, sn = (s1, s2) if layout == _lib.PERM_LAYOUT_BIN_SOURCE else (s2, s1)
    out = dv.empty(tuple(array.shape), array.dtype, array.device)
    if out.numel():
        _lib.check(_L().ssspy_permute_sources(flat.data_ptr(), ptr(out), ptr(perm), B, N, F, inner,
                                              int(layout), sb, sf, sn, _st()), "permute_sources")
    return out


def permutation_amplitude(posterior, X, reference_id):
    """|posterior * X[:, reference_id]| (B, N, F, T)."""
    B, N, F, T = posterior.shape
    M = X.shape[1]
    out = dv.empty((B, N, F, T), dv.f64, X.device)
    _lib.check(_L().ssspy_permutation_amplitude(ptr(posterior), ptr(X), ptr(out), B, N, M, F, T,
                                                int(reference_id), _st()), "permutation_amplitude")
    return out


# ---- IPSDTA (csrc/ipsdta.hip).  A partition is (basis (B, N, K, Cn, L, L), first bin, first block):
# the blocks of one size, see ssspy_ipsdta_frame_pass.
def ipsdta_frame_pass(X, W, part, activation, pi, n_blocks, mode, out0, out1=None, route=None):
    basis, first_bin, first_block = part
    B, N, F, T = X.shape
    K, Cn, L = basis.shape[2], basis.shape[3], basis.shape[4]
    _lib.check(_L().ssspy_ipsdta_frame_pass(
        ptr(X), ptr(W), ptr(basis), ptr(activation), ptr(pi), B, N, F, T, K, Cn, L, first_bin,
        first_block, n_blocks, mode, ptr(out0), ptr(out1), ptr(route), _st()), "ipsdta_frame_pass")


def ipsdta_quadratic(X, W, parts, activation, n_blocks, route=None):
    """(quad, logdet) (B, N, n_blocks, T) over every partition."""
    B, N, F, T = X.shape
    quad = dv.empty((B, N, n_blocks, T), dv.f64, X.device)
    logdet = dv.empty((B, N, n_blocks, T), dv.f64, X.device)
    for part in parts:
        ipsdta_frame_pass(X, W, part, activation, None, n_blocks, _lib.IPSDTA_QUAD, quad, logdet,
                          route)
    return quad, logdet


def ipsdta_weight_loss(quad, logdet, n_low_blocks, n_bins, model, dof, want_pi=False, loss=None):
    B, N, n_blocks, T = quad.shape
    pi = dv.empty((B, N, T), dv.f64, quad.device) if want_pi else None
    _lib.check(_L().ssspy_ipsdta_weight_loss(ptr(quad), ptr(logdet), B, N, n_blocks, n_low_blocks, T,
                                             n_bins, model, float(dof), ptr(pi), ptr(loss), _st()),
               "ipsdta_weight_loss")
    return pi


def ipsdta_basis_statistics(X, W, part, activation, pi, n_blocks):
    """(P, Q), each shaped as the partition's basis."""
    basis = part[0]
    P = dv.empty(tuple(basis.shape), dv.c128, X.device)
    Q = dv.empty(tuple(basis.shape), dv.c128, X.device)
    ipsdta_frame_pass(X, W, part, activation, pi, n_blocks, _lib.IPSDTA_BASIS, P, Q)
    return P, Q


def ipsdta_activation_terms(X, W, parts, activation, pi, n_blocks):
    """(num, den) (B, N, K, n_blocks, T): the per-block terms of the activation update."""
    B, N, F, T = X.shape
    K = activation.shape[2]
    num = dv.empty((B, N, K, n_blocks, T), dv.f64, X.device)
    den = dv.empty((B, N, K, n_blocks, T), dv.f64, X.device)
    for part in parts:
        ipsdta_frame_pass(X, W, part, activation, pi, n_blocks, _lib.IPSDTA_ACT, num, den)
    return num, den


def ipsdta_activation(activation, num, den):
    B, N, K, n_blocks, T = num.shape
    _lib.check(_L().ssspy_ipsdta_activation(ptr(activation), ptr(num), ptr(den), B, N, K, n_blocks, T,
                                            _st()), "ipsdta_activation")
    return activation


def ipsdta_weighted_covariance(X, W, part, activation, pi, n_blocks):
    """(B, Cn, L, L, N, N, N): the weighted covariance of the VCD sweep of one partition."""
    basis = part[0]
    B, N = X.shape[0], X.shape[1]
    Cn, L = basis.shape[3], basis.shape[4]
    out = dv.empty((B, Cn, L, L, N, N, N), dv.c128, X.device)
    ipsdta_frame_pass(X, W, part, activation, pi, n_blocks, _lib.IPSDTA_COV, out)
    return out


def ipsdta_normalize(basis_low, basis_high, activation):
    B, N, K, Clow, Llow = basis_low.shape[:5]
    Chigh, Lhigh = (basis_high.shape[3], basis_high.shape[4]) if basis_high is not None else (0, 0)
    _lib.check(_L().ssspy_ipsdta_normalize(ptr(basis_low), ptr(basis_high), ptr(activation), B, N, K,
                                           Clow, Llow, Chigh, Lhigh, activation.shape[-1], _st()),
               "ipsdta_normalize")


def ipsdta_vcd(W, weighted_covariance, first_bin, threshold, info=None):
    """The VCD sweep of one partition, in place on W (B, F, N, N)."""
    B, F, N = W.shape[0], W.shape[1], W.shape[2]
    Cn, L = weighted_covariance.shape[1], weighted_covariance.shape[2]
    _lib.check(_L().ssspy_ipsdta_vcd(ptr(W), ptr(weighted_covariance), B, F, N, Cn, L, first_bin,
                                     float(threshold), ptr(info), _st()), "ipsdta_vcd")
    return W


def ipsdta_reconstruct(basis, activation, flooring, basis_last=False):
    """to_psd(sum_k v T) (..., T, C, L, L) from a device basis (..., K, C, L, L) -- with basis_last
    (..., C, L, L, K) -- and activation (..., K, T); flooring a device floor (kind, eps)."""
    if basis_last:
        C, L, K = basis.shape[-4], basis.shape[-3], basis.shape[-1]
    else:
        K, C, L = basis.shape[-4], basis.shape[-3], basis.shape[-1]
    lead = tuple(activation.shape[:-2])
    T = activation.shape[-1]
    assert activation.shape[-2] == K and basis.numel() == activation.numel() // T * C * L * L
    out = dv.empty(lead + (T, C, L, L), dv.c128, basis.device)
    if out.numel():
        _lib.check(_L().ssspy_ipsdta_reconstruct(
            ptr(basis), ptr(activation), ptr(out), activation.numel() // (K * T), K, T, C, L,
            int(bool(basis_last)), int(flooring[0]), float(flooring[1]), _st()), "ipsdta_reconstruct")
    return out


def matmul3(A, Bm, C):
    """(A B) C for stacks (..., L, L) of small matrices on the device."""
    L = A.shape[-1]
    out = dv.empty(tuple(A.shape), dv.c128, A.device)
    _lib.check(_L().ssspy_matmul3(ptr(A), ptr(Bm), ptr(C), ptr(out), A.numel() // (L * L), L, _st()),
               "matmul3")
    return out


def to_psd_dev(A, flooring):
    """to_psd on a device stack (..., L, L) with one of the kernels' floors (kind, eps)."""
    L = A.shape[-1]
    out = dv.empty(tuple(A.shape), dv.c128, A.device)
    _lib.check(_L().ssspy_to_psd(ptr(A), ptr(out), A.numel() // (L * L), L, flooring[0], flooring[1],
                                 _st()), "to_psd")
    return out


def sqrtmh_dev(A, inverse=False, flooring=(_lib.FLOOR_NONE, 0.0)):
    L = A.shape[-1]
    out = dv.empty(tuple(A.shape), dv.c128, A.device)
    _lib.check(_L().ssspy_sqrtmh(ptr(A), ptr(out), A.numel() // (L * L), L, int(inverse), flooring[0],
                                 flooring[1], _st()), "sqrtmh")
    return out


def gmeanmh_dev(A, Bm, type=1):
    L = A.shape[-1]
    out = dv.empty(tuple(A.shape), dv.c128, A.device)
    _lib.check(_L().ssspy_gmeanmh(ptr(A), ptr(Bm), ptr(out), A.numel() // (L * L), L, type, _st()),
               "gmeanmh")
    return out


# ---- softmax, logsumexp, quadratic forms of device tensors (csrc/special.hip).  The reduced axis of
# a contiguous tensor is addressed as (outer, len, inner): nothing is transposed.
def _axis_split(X, axis):
    outer = 1
    for s in X.shape[:axis]:
        outer *= s
    inner = 1
    for s in X.shape[axis + 1:]:
        inner *= s
    return outer, X.shape[axis], inner


def softmax_dev(X, axis):
    """softmax over ``axis`` (normalised, >= 0) of a contiguous f64 device tensor."""
    outer, n, inner = _axis_split(X, axis)
    out = dv.empty(tuple(X.shape), dv.f64, X.device)
    if out.numel():
        _lib.check(_L().ssspy_softmax(ptr(X), ptr(out), outer, n, inner, _st()), "softmax")
    return out


def logsumexp_dev(X, axis):
    """log-sum-exp over ``axis`` of a contiguous f64 device tensor; that axis is dropped."""
    outer, n, inner = _axis_split(X, axis)
    out = dv.empty(tuple(X.shape[:axis]) + tuple(X.shape[axis + 1:]), dv.f64, X.device)
    if out.numel():
        _lib.check(_L().ssspy_logsumexp(ptr(X), ptr(out), outer, n, inner, _st()), "logsumexp")
    return out


def quadratic_dev(X, A):
    """x^H A x of contiguous c128 device stacks X (..., n), A (..., n, n) -> c128 (...)."""
    n = X.shape[-1]
    out = dv.empty(tuple(X.shape[:-1]), dv.c128, X.device)
    if out.numel():
        _lib.check(_L().ssspy_quadratic(ptr(X), ptr(A), ptr(out), out.numel(), n, _st()), "quadratic")
    return out
