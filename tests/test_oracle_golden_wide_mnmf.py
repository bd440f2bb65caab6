"""FastGaussMNMF fixtures at 9-16 channels and above 8 sources (tests/golden/make_golden_wide_mnmf.py),
replayed through the NumPy oracle at the tolerances of test_oracle_golden.py: the fixtures the GPU
tests of test_gpu_fmnmf_wide.py compare against are pinned to the oracle here."""

import pytest

from conftest import load_golden
from test_oracle_golden import TOL, _golden_custom_floor, _oracle_for, _replay_uninjected
from test_oracle_golden import test_fast_gauss_mnmf as _replay_fast_gauss_mnmf

WIDE_MNMF_CASES = ["fmnmf_ip1_m10", "fmnmf_ip1_m16_n3", "fmnmf_ip2_m12", "fmnmf_ip2_m16_comb",
                   "fmnmf_ip1_m4_n12", "fmnmf_ip1_m9_nonorm_add"]


@pytest.mark.parametrize("case", WIDE_MNMF_CASES)
def test_fast_gauss_mnmf_wide(case):
    """Snapshots, loss list and Wiener output; IP2 diagonalisers up to phase."""
    _replay_fast_gauss_mnmf(case)


def test_fast_gauss_mnmf_wide_custom_floor():
    g = load_golden("customfloor_fmnmf_m10")
    m, names = _oracle_for(g, flooring=_golden_custom_floor)
    _replay_uninjected(g, m, names, TOL)


def test_wide_fixture_shapes():
    """The fixtures hold the shapes their names promise (M channels, N sources)."""
    for case, M, N in [("fmnmf_ip1_m10", 10, 10), ("fmnmf_ip1_m16_n3", 16, 3),
                       ("fmnmf_ip2_m12", 12, 12), ("fmnmf_ip2_m16_comb", 16, 16),
                       ("fmnmf_ip1_m4_n12", 4, 12), ("fmnmf_ip1_m9_nonorm_add", 9, 9)]:
        g = load_golden(case)
        assert g["X"].shape[0] == M and int(g["meta_n_sources"]) == N, case
        assert g["final_output"].shape[0] == N, case
