"""The workgroup tiles of the large LU trailing updates (csrc/zgemm.hip, MAUS_LU_TILE) against planted factors, bit for bit.

The 128 x 64 tile (zgemm3m_dma_kernel<2, 2, 4, 2, true>) takes the updates with M, N >= 1024 and K >= 256 whose grid is at
least 4096 tiles; MAUS_LU_TILE=128x64 gives it every update with M, N >= 1024 on the DMA path (K >= 64, a multiple of 8),
MAUS_LU_TILE=64x64 restores the rule before it (64 x 64 tiles from 1536, 64 x 32 below).  The library reads the switch once
per process, so every value runs in a child process of its own (tests/lu_tile_child.py) with a fresh Context, and so does the
default dispatch -- which, with the one to three matrices of these cases, stays on the 64 x 64 rule: the default rule's way
into the 128 x 64 tile is the full-size population of tests/test_gpu_full_size.py and tests/test_gpu_bench_path.py.  The
systems are those of tests/lu_cases.py (planted factors, exact in 45 bits: checked here on the CPU for the sizes this file
adds), so status, ipiv and x must equal the planted ones under every tile, and a Gaussian batch must give the same x and ipiv,
element for element, under all of them: each accumulator takes k ascending, 4 per MFMA, whatever the tile."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lu_cases as lc
import lu_tile_child as child
from zgemm_cases import LT_MIN, LU_TILES as TILES, lu_variant

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = list(child.lu_tile_cases())


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """tile -> the arrays its child wrote."""
    d = tmp_path_factory.mktemp("lu_tile")
    out = {}
    for tile in TILES:
        env = dict(os.environ)
        env.pop("MAUS_LU_NBO", None)
        env.pop("MAUS_LU_TILE", None)
        if tile != "default":
            env["MAUS_LU_TILE"] = tile
        env["MAUS_LU_TRACE"] = str(d / f"trace_{tile}.txt")
        path = str(d / f"{tile}.npz")
        p = subprocess.run([sys.executable, "-s", os.path.join(HERE, "lu_tile_child.py"), path], env=env,
                           capture_output=True, text=True)
        assert p.returncode == 0, f"MAUS_LU_TILE={tile}: child failed ({p.returncode})\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
        with np.load(path) as z:
            out[tile] = {k: z[k] for k in z.files}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("tile", TILES)
def test_planted_bit_for_bit(runs, tile, name):
    r = runs[tile]
    status, pg, xg = r[f"{name}/status"], r[f"{name}/ipiv"], r[f"{name}/x"]
    ipiv, x = r[f"{name}/ipiv_planted"], r[f"{name}/x_planted"]
    assert (status == 0).all(), (tile, name, status)
    for g in range(x.shape[0]):
        bad = np.flatnonzero(pg[g] != ipiv[g])
        assert bad.size == 0, f"{tile}/{name}[{g}]: ipiv differs first at column {bad[:1]} ({bad.size} columns)"
        bad = np.flatnonzero(xg[g] != x[g])
        assert bad.size == 0, f"{tile}/{name}[{g}]: x differs first at row {bad[:1]}: {xg[g][bad[:3]]} for {x[g][bad[:3]]} ({bad.size} rows)"
    assert np.array_equal(pg, ipiv) and np.array_equal(xg, x)
    assert int(r["mw_aborts"]) == 0, "a multi-workgroup panel timed out; the path was not exercised"


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("tile", TILES)
def test_case_reaches_the_large_tile(runs, tile, name):
    """From the library's launch log: under MAUS_LU_TILE=128x64 the case issued an update that the 128 x 64 tile serves, at
    the K the case is about, and one below the threshold beside it.  A threshold that moves out from under a case fails it
    here.  The other two runs are the comparison: none of their updates goes to the large tile."""
    L = runs[tile][f"{name}/launches"]
    assert L.shape[0] > 0, "no trailing update was logged"
    served = np.array([lu_variant(tile, *row)[0] == "dma3m_128x64_lu" for row in L.tolist()])
    if tile != "128x64":
        assert not served.any(), f"{tile}/{name}: {L[served][:4].tolist()} go to the 128 x 64 tile"
        return
    assert served.any(), f"{tile}/{name}: no update with M, N >= {LT_MIN}: {L[:4].tolist()} ..."
    want_k = child.lu_tile_cases()[name][0] or 512
    K = L[:, 2]
    assert (K[served] == want_k).any(), f"{tile}/{name}: no large update with K = {want_k}"
    assert (K[~served] == want_k).any(), f"{tile}/{name}: no update with K = {want_k} below the threshold"


@pytest.mark.gpu
def test_gaussian_same_bits_under_every_tile(runs):
    ref = runs[TILES[0]]
    assert (ref["gaussian/status"] == 0).all()
    for tile in TILES[1:]:
        r = runs[tile]
        assert np.array_equal(r["gaussian/status"], ref["gaussian/status"]), tile
        assert np.array_equal(r["gaussian/ipiv"], ref["gaussian/ipiv"]), tile
        assert np.array_equal(r["gaussian/x"], ref["gaussian/x"]), tile
    # and the answer is an answer: against LAPACK on the same batch
    A, b = child.gaussian_batch()
    for g in range(A.shape[0]):
        xl = np.linalg.solve(A[g], b[g])
        assert np.max(np.abs(ref["gaussian/x"][g] - xl)) <= 1e-8 * np.max(np.abs(xl))


@pytest.mark.parametrize("name", ["n2080_g2", "n2112_g3", "n2080_piv_reverse"])
def test_cases_stay_exact_in_45_bits(name):
    """CPU: the planted systems of this file keep every intermediate within 45 significand bits (lu_cases.budget_bits)."""
    nbo, build = child.lu_tile_cases()[name]
    if name.startswith("n2080_piv"):
        kw = lc._family(2080)[name[len("n2080_"):]]
        systems = [lc.system(2080, lc.family_seed(2080, name[len("n2080_"):]), **kw)]
    else:
        n, G, seed = (2080, 2, 2080) if name == "n2080_g2" else (2112, 3, 2112)
        case = lc._case(f"tile_n{n}", n, G, ("default",), [], seed)
        systems = [lc.system(n, seed + 1000 * g, False, **lc.case_kwargs(case, g)) for g in range(G)]
    for A, b, x, ipiv, L, U in systems:
        assert lc.budget_bits(L, U, x) <= 45
