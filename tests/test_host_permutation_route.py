"""The route of the device permutation alignment exists and can be switched off (no device)."""

import pytest


def test_device_alignment_route():
    from ssspy_amd import _routes

    assert _routes._DEFAULTS["device_alignment"] is True
    assert _routes.get("device_alignment") is True
    with _routes.override(device_alignment=False):
        assert _routes.get("device_alignment") is False
    assert _routes.get("device_alignment") is True
    with pytest.raises(KeyError):
        with _routes.override(device_alinement=False):
            pass


def test_route_function_limits():
    from ssspy_amd import _lib, _ops
    from ssspy_amd.utils.flooring import device_flooring

    floor = device_flooring(None)
    callable_floor = device_flooring(lambda x: x, allow_host=True)
    corr, score = _lib.PERM_SOLVER_CORRELATION, _lib.PERM_SOLVER_SCORE
    for N in range(2, 9):
        assert _ops.permutation_route(N, 512, corr, floor)
        assert _ops.permutation_route(N, 512, score, floor)
        assert not _ops.permutation_route(N, 512, score, callable_floor)
    for N in (1, 9, 16):
        assert not _ops.permutation_route(N, 512, corr, floor)
        assert not _ops.permutation_route(N, 512, score, floor)
    assert _ops.permutation_route(4, 4096, corr, floor)
    assert not _ops.permutation_route(4, 4097, corr, floor)
    assert _ops.permutation_route(4, 100000, score, floor)
    assert "16384" in _ops.permutation_limit(4, 4097, corr, floor)
    assert "sources" in _ops.permutation_limit(9, 16, corr, floor)
    assert "flooring_fn" in _ops.permutation_limit(4, 16, corr, callable_floor)
