"""The zgemm dispatch rule, without a GPU: maus_zgemm_plan (csrc/zgemm.hip's zgemm_plan, pure and context-free) against its
independent statement in tests/zgemm_cases.py (variant, lu_variant) on both sides of every threshold, for both forms, the three
MAUS_LU_TILE modes, both layouts and the four conjugation forms; and against literals taken from INTEGRATION.md (the
MAUS_LU_TILE row) and profiles/zgemm_large_tile_rates.txt, which come from neither statement."""
import ctypes as C
import itertools
import os
import re

import pytest

from adaptive_matrix_solver_amd import _cabi
from zgemm_cases import CONJ, LU_TILES, all_variants, lu_variant, plan_of, variant

MS = (1, 16, 17, 32, 33, 64, 1023, 1024, 1535, 1536, 2048)
NS = (1, 16, 17, 64, 1023, 1024, 1535, 1536, 1984, 2048, 40000)
KS = (1, 8, 56, 60, 63, 64, 72, 77, 248, 255, 256, 512)
BATCHES = (1, 2, 31, 32, 136)
TILE_MODE = {"default": _cabi.LU_TILE_DEFAULT, "64x64": _cabi.LU_TILE_64X64, "128x64": _cabi.LU_TILE_128X64}
DMA, REG3M = _cabi.ZGEMM_3M_DMA, _cabi.ZGEMM_3M


def test_the_constants_are_the_headers():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "maus_hip.h")).read()
    declared = {k: int(v) for k, v in re.findall(r"\bMAUS_((?:ZGEMM|LU_TILE)_[A-Z0-9_]+) = (\d+)", header)}
    assert declared == {k: getattr(_cabi, k) for k in ("ZGEMM_ROWS", "ZGEMM_LU", "LU_TILE_DEFAULT", "LU_TILE_64X64", "LU_TILE_128X64",
                                                        "ZGEMM_4M", "ZGEMM_3M", "ZGEMM_3M_DMA")}
    assert list(TILE_MODE) == LU_TILES


def test_the_grid_holds_the_tile_count_boundaries():
    """The shapes whose tile counts sit exactly on, and just under, the two tile-count thresholds."""
    def tiles(M, N, G, bm, bn):
        return -(-M // bm) * -(-N // bn) * G
    assert {1024} <= set(MS) and {1984, 2048, 1024} <= set(NS) and {1, 31, 32} <= set(BATCHES)
    assert tiles(1024, 2048, 1, 64, 64) == 512
    assert tiles(1024, 1984, 1, 64, 64) == 496 and tiles(1024, 1984, 1, 32, 64) == 992
    assert tiles(1024, 1024, 32, 128, 64) == 4096 and tiles(1024, 1024, 31, 128, 64) == 3968


def test_the_library_and_the_python_rule_agree_at_every_boundary():
    lib = _cabi.load_library()
    bm, bn = C.c_int(), C.c_int()
    seen_rows, seen_lu = set(), set()
    for M, N, K, G in itertools.product(MS, NS, KS, BATCHES):
        for tile, mode in TILE_MODE.items():
            where = f"{M} x {N} x {K}, batch {G}, MAUS_LU_TILE {tile}"
            name = lu_variant(tile, M, N, K, G)[0]
            fam = lib.maus_zgemm_plan(_cabi.ZGEMM_LU, mode, M, N, K, G, 0, 0, 0, C.byref(bm), C.byref(bn))
            assert (fam, bm.value, bn.value) == plan_of(name), f"LU form, {where}: {name}"
            seen_lu.add(name)
            for bl, (ca, cb) in itertools.product((0, 1), CONJ):      # the rows form does not look at the tile mode
                name = variant(M, N, K, bl, ca, cb, G)[0]
                fam = lib.maus_zgemm_plan(_cabi.ZGEMM_ROWS, mode, M, N, K, G, bl, ca, cb, C.byref(bm), C.byref(bn))
                assert (fam, bm.value, bn.value) == plan_of(name), f"rows form, {where}, layout {bl}, conj {ca} {cb}: {name}"
                seen_rows.add(name)
    # no branch of either form is missed: 6 + 10 + 21 for the rows form (test_gpu_zgemm_variants.py states the same count), 7 for the LU form
    assert len(seen_rows) == 6 + 10 + 21 and seen_rows == set(all_variants()), sorted(set(all_variants()) ^ seen_rows)
    assert seen_lu == {"4m_128x16_lu", "4m_16x128_lu", "reg3m_32x64_lu", "reg3m_64x32_lu", "dma3m_64x32_lu", "dma3m_64x64_lu",
                       "dma3m_128x64_lu"}


# the DMA-staged tile of an LU-form update under each tile mode: (M, N, K, batch) -> {mode: (BM, BN)}
PINNED_LU = [
    ((1024, 1056, 512, 181), {"default": (128, 64), "64x64": (64, 32), "128x64": (128, 64)}),
    ((1024, 1056, 512, 1), {"default": (64, 32), "128x64": (128, 64)}),
    ((1536, 1568, 512, 1), {"default": (64, 64), "64x64": (64, 64)}),
    ((1024, 1056, 64, 181), {"default": (64, 32)}),                   # K < 256
]


@pytest.mark.parametrize("shape,tiles", PINNED_LU)
def test_pinned_lu_tiles(shape, tiles):
    M, N, K, G = shape
    for tile, want in tiles.items():
        assert _cabi.zgemm_plan(_cabi.ZGEMM_LU, TILE_MODE[tile], M, N, K, batch=G) == (DMA,) + want, (shape, tile)


def test_pinned_rows_edge():
    """The two shapes tests/zgemm_cases.py documents as the edge of the DMA path."""
    assert _cabi.zgemm_plan(_cabi.ZGEMM_ROWS, _cabi.LU_TILE_DEFAULT, 33, 65, 128) == (DMA, 64, 32)
    assert _cabi.zgemm_plan(_cabi.ZGEMM_ROWS, _cabi.LU_TILE_DEFAULT, 32, 65, 128) == (REG3M, 32, 64)


BAD = [
    dict(form=2), dict(form=-1), dict(lu_tile=3), dict(lu_tile=-1), dict(M=0), dict(N=0), dict(K=0), dict(batch=0), dict(M=-5),
    dict(b_layout=2), dict(b_layout=-1),
    dict(form=1, b_layout=1), dict(form=1, conj_a=1), dict(form=1, conj_b=1),
]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_bad_arguments_are_refused(bad):
    lib = _cabi.load_library()
    a = dict(form=0, lu_tile=0, M=100, N=100, K=64, batch=1, b_layout=0, conj_a=0, conj_b=0)
    assert lib.maus_zgemm_plan(*a.values(), None, None) == _cabi.ZGEMM_3M_DMA
    a.update(bad)
    assert lib.maus_zgemm_plan(*a.values(), None, None) == -1
    with pytest.raises(_cabi.MausHipError):
        _cabi.zgemm_plan(*a.values())


def test_null_outputs_are_allowed():
    lib = _cabi.load_library()
    bm = C.c_int()
    assert lib.maus_zgemm_plan(1, 2, 2048, 2048, 512, 1, 0, 0, 0, None, None) == _cabi.ZGEMM_3M_DMA
    assert lib.maus_zgemm_plan(1, 2, 2048, 2048, 512, 1, 0, 0, 0, C.byref(bm), None) == _cabi.ZGEMM_3M_DMA and bm.value == 128
    assert lib.maus_zgemm_plan(0, 0, 5, 7, 3, 1, 1, 1, 1, None, C.byref(bm)) == _cabi.ZGEMM_4M and bm.value == 32
