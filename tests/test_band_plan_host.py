"""The band dispatch rule, without a GPU: maus_band_plan (csrc/band.hip's band_plan, pure and context-free) against its
restatement in band.py (kernel_for, band_bytes_per_solve) over every boundary of the ranges and block widths."""
import itertools

import pytest

from adaptive_matrix_solver_amd import _cabi
from adaptive_matrix_solver_amd.band import DIRECT_METHOD, band_bytes_per_solve, kernel_for

METHODS = (0, 1, 2, 4, 8)
KLS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 1008, 1009, 1016, 1017, 1024, 1025, 1520, 1521, 3064, 3065, 4096, 4097)
KUS = (0, 5, 16, 17, 31, 40, 5000)
N = 6000
FLAG = {0: {}, 1: {"blocked": True}, 2: {"tiled": True}, 4: {"wide": True}, 8: {"narrow": True}}


def test_the_method_table_names_every_method():
    assert DIRECT_METHOD == {"band": 0, "blocked": 1, "tiled": 2, "wide": 4, "narrow": 8}
    assert (_cabi.BAND_COLUMN, _cabi.BAND_BLOCKED, _cabi.BAND_TILED, _cabi.BAND_WIDE, _cabi.BAND_NARROW) == METHODS


def test_the_library_and_the_python_rule_agree_at_every_boundary():
    for method, kl, ku in itertools.product(METHODS, KLS, KUS):
        kind, nb, outer_nb, per = _cabi.band_plan(method, N, kl, ku)
        where = f"method {method}, kl {kl}, ku {ku}"
        assert (kind, nb) == kernel_for(method, kl, ku), where
        assert outer_nb == (64 if kind == 4 else 0), where
        assert per == band_bytes_per_solve(N, kl, ku, **FLAG[method]), where
        assert per == band_bytes_per_solve(N, kl, ku, method=method), where


def _nb(method, kl):
    return _cabi.band_plan(method, N, kl, 40)[:2]


def test_block_widths_at_the_documented_boundaries():
    for kl in (16, 17, 63, 64, 65, 1008):
        assert _nb(1, kl) == (1, 16) and _nb(2, kl) == (2, 16)
    for kl in (1009, 1016, 1017, 1024):
        assert _nb(1, kl) == (1, 8) and _nb(2, kl) == (2, 8)
    for kl, nb in ((1025, 16), (1520, 16), (1521, 8), (3064, 8), (3065, 4), (4096, 4)):
        assert _nb(1, kl) == (0, 1)
        assert _nb(2, kl) == (2, nb) and _nb(4, kl) == (4, nb)
    for kl, nb in ((16, 16), (17, 16), (63, 16)):                       # under wide, below its range: the tiled kernels
        assert _nb(4, kl) == (2, nb)
    for kl, nb in ((64, 16), (65, 16), (1008, 16), (1009, 8), (1024, 8)):
        assert _nb(4, kl) == (4, nb)
    for method in (1, 2, 4):
        assert _nb(method, 15) == (0, 1) and _nb(method, 4097) == (0, 1)
    assert _cabi.band_plan(8, N, 15, 16)[:2] == (8, 1) and _cabi.band_plan(8, N, 15, 17)[:2] == (0, 1)
    assert _cabi.band_plan(8, N, 16, 5)[:2] == (0, 1)


@pytest.mark.parametrize("method", (-1, 3, 5, 6, 7, 9, 16))
def test_a_bad_method_is_refused(method):
    lib = _cabi.load_library()
    assert lib.maus_band_plan(method, N, 100, 20, None, None, None, None) == -1
    with pytest.raises(_cabi.MausHipError):
        _cabi.band_plan(method, N, 100, 20)


def test_negative_sizes_are_refused_and_null_outputs_are_allowed():
    lib = _cabi.load_library()
    assert lib.maus_band_plan(2, N, 100, 20, None, None, None, None) == 0
    for n, kl, ku in ((-1, 100, 20), (N, -1, 20), (N, 100, -1)):
        assert lib.maus_band_plan(2, n, kl, ku, None, None, None, None) == -1
