"""GaussMNMF fixtures at 9-16 sources (tests/golden/make_golden_gmnmf_sources.py), replayed through the
NumPy oracle at the tolerances of test_oracle_golden.py: the fixtures the GPU tests of
test_gpu_gmnmf_sources.py compare against are pinned to the oracle here."""

import pytest

from conftest import load_golden
from test_oracle_golden import test_gauss_mnmf as _replay_gauss_mnmf

# (case, n_channels, n_sources, partitioning)
GMNMF_SOURCES_CASES = [("gmnmf_m2_n9", 2, 9, False), ("gmnmf_m4_n12", 4, 12, False),
                       ("gmnmf_m8_n16", 8, 16, False), ("gmnmf_part_m3_n10", 3, 10, True),
                       ("gmnmf_m6_n16_nonorm_add", 6, 16, False),
                       ("gmnmf_floor_m5_n9", 5, 9, False)]


@pytest.mark.parametrize("case", [c[0] for c in GMNMF_SOURCES_CASES])
def test_gauss_mnmf_sources(case):
    """Snapshots, loss list and Wiener output."""
    _replay_gauss_mnmf(case)


def test_gmnmf_sources_fixture_shapes():
    """The fixtures hold the shapes their names promise (M channels, N sources)."""
    for case, M, N, part in GMNMF_SOURCES_CASES:
        g = load_golden(case)
        K = int(g["meta_n_basis"])
        assert g["X"].shape[0] == M and int(g["meta_n_sources"]) == N, case
        assert g["final_output"].shape[0] == N, case
        assert g["final_spatial"].shape[:1] == (N,) and g["final_spatial"].shape[-2:] == (M, M), case
        assert bool(g["meta_partitioning"]) == part, case
        if part:
            assert g["final_latent"].shape == (N, K) and K > N, case
        else:
            assert g["final_basis"].shape[0] == N, case
