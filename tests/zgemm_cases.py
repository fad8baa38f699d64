"""The zgemm dispatch rule, stated in Python, and the shapes that reach every kernel it can pick.

`variant()` (the rows form: maus_zgemm_launch_rows, i.e. everything Context.zgemm can reach) and `lu_variant()` (the LU form:
maus_zgemm_launch_lu) are written from the rule's description, not generated from the library: tests/test_zgemm_plan_host.py
holds the library's own statement (zgemm_plan in csrc/zgemm.hip, through maus_zgemm_plan) against them on both sides of every
threshold, without a GPU.  tests/test_gpu_zgemm_variants.py runs CASES; tests/test_gpu_lu_tile.py reads the LU's launch log
with lu_variant()."""
import itertools

CONJ = [(False, False), (True, False), (False, True), (True, True)]
LU_TILES = ["default", "64x64", "128x64"]                    # MAUS_LU_TILE: unset, or one of the two values it takes
# the thresholds of the LU form's 128 x 64 tile, and the smallest K of the DMA-staged kernel (both forms)
LT_MIN, LT_K, LT_TILES, DMA_KMIN = 1024, 256, 4096, 64
FAMILY = {"4m": 0, "reg3m": 1, "dma3m": 2}                   # maus_zgemm_plan's return value, by the prefix of a variant's name


def _b(x):
    return "true" if x else "false"


def variant(M, N, K, b_layout, conj_a, conj_b, batch=1):
    """(name, demangled kernel instantiation) that maus_zgemm_launch_rows picks."""
    def ceil(a, b):
        return (a + b - 1) // b
    tag = f"b{b_layout}" + ("_ca" if conj_a else "") + ("_cb" if conj_b else "")
    dma = M > 32 and K % 8 == 0 and K >= DMA_KMIN
    big = M >= 1536 and N >= 1536

    def dma_kernel():
        return (f"dma3m_{'64x64' if big else '64x32'}_{tag}",
                f"zgemm3m_dma_kernel<2, {3 if big else 5}, 2, {2 if big else 1}, false, {b_layout}, {_b(conj_a)}, {_b(conj_b)}>")
    if b_layout == 0 and not conj_a and not conj_b:
        if N <= 16:
            return "4m_128x16_b0", "zgemm_kernel<128, 16, 16, 4, 1, 0, false, false, 4, false, false>"
        if M <= 16:
            return "4m_16x128_b0", "zgemm_kernel<16, 128, 16, 1, 4, 0, false, false, 3, false, false>"
        if dma:
            return dma_kernel()
        if M <= 32:
            return "reg3m_32x64_b0", "zgemm_kernel<32, 64, 16, 1, 4, 0, false, false, 4, true, false>"
        return "reg3m_64x32_b0", "zgemm_kernel<64, 32, 16, 2, 2, 0, false, false, 4, true, false>"
    if dma and not (conj_a and conj_b):
        return dma_kernel()
    if ceil(M, 64) * ceil(N, 64) * batch >= 512:
        shape, targs, minw = "64x64", "64, 64, 16, 2, 2", 3
    elif ceil(M, 32) * ceil(N, 64) * batch >= 512:
        shape, targs, minw = "32x64", "32, 64, 16, 1, 4", 4
    else:
        shape, targs, minw = "32x32", "32, 32, 16, 2, 2", 4
    return f"4m_{shape}_{tag}", f"zgemm_kernel<{targs}, {b_layout}, {_b(conj_a)}, {_b(conj_b)}, {minw}, false, false>"


def lu_variant(tile, M, N, K, G):
    """(name, demangled kernel instantiation) that maus_zgemm_launch_lu picks for an M x N x K update of G matrices under
    MAUS_LU_TILE = `tile` (one of LU_TILES).  The operands are tile-major: the last template argument of every kernel."""
    assert tile in LU_TILES
    if N <= 16:
        return "4m_128x16_lu", "zgemm_kernel<128, 16, 16, 4, 1, 0, false, false, 4, false, true>"
    if M <= 16:
        return "4m_16x128_lu", "zgemm_kernel<16, 128, 16, 1, 4, 0, false, false, 3, false, true>"
    if M <= 32:
        return "reg3m_32x64_lu", "zgemm_kernel<32, 64, 16, 1, 4, 0, false, false, 4, true, true>"
    if K % 8 or K < DMA_KMIN:
        return "reg3m_64x32_lu", "zgemm_kernel<64, 32, 16, 2, 2, 0, false, false, 4, true, true>"
    if M >= LT_MIN and N >= LT_MIN:
        if tile == "128x64" or (tile == "default" and K >= LT_K and -(-M // 128) * -(-N // 64) * G >= LT_TILES):
            return "dma3m_128x64_lu", "zgemm3m_dma_kernel<2, 2, 4, 2, true, 0, false, false>"
    if M >= 1536 and N >= 1536:
        return "dma3m_64x64_lu", "zgemm3m_dma_kernel<2, 3, 2, 2, true, 0, false, false>"
    return "dma3m_64x32_lu", "zgemm3m_dma_kernel<2, 5, 2, 1, true, 0, false, false>"


def plan_of(name):
    """(family, BM, BN) as maus_zgemm_plan reports them, from a variant's name."""
    family, shape = name.split("_")[:2]
    bm, bn = shape.split("x")
    return FAMILY[family], int(bm), int(bn)


def all_variants():
    """Every kernel the rule can return: enumerated from the rule's own branches."""
    out = {}
    probes = [(5, 7, 3), (9, 200, 64), (24, 100, 48), (33, 65, 128), (70, 50, 60), (70, 50, 64), (1536, 1536, 64), (1536, 1536, 60),
              (1000, 1500, 77), (17, 17, 8)]
    for (M, N, K), bl, (ca, cb) in itertools.product(probes, (0, 1), CONJ):
        name, kern = variant(M, N, K, bl, ca, cb)
        out[name] = kern
    return out


# (M, N, K).  What each is there for:
SHAPES = [
    (5, 7, 3),               # N <= 16: the 128 x 16 skinny kernel; everything else in one 32 x 32 tile, K < one K-tile
    (16, 130, 40),           # M <= 16: the 16 x 128 skinny kernel, ragged N, K = 2.5 K-tiles
    (9, 200, 64),
    (24, 100, 48),           # M in 17..32: register-staged 3M with 32 x 64 tiles
    (32, 65, 128),           # M = 32: the last M below the DMA path
    (33, 65, 128),           # M = 33: the first M on it
    (17, 17, 8),
    (100, 130, 77),          # K tail of 13 on 32 x 32 tiles (the K-edge shape of test_gpu_kernels.py)
    (1500, 1500, 77),        # the same K tail on 64 x 64 4M tiles (576 tiles)
    (1000, 1500, 77),        # ... and on 32 x 64 4M tiles (384 tiles of 64 x 64, 768 of 32 x 64)
    (40, 40000, 12),         # 625 tiles in one tile row
    (1536, 1536, 64),        # the smallest product on 64 x 64 DMA tiles: one K stage more than the ring holds
    (1537, 1599, 200),       # ragged edges on both sides of 64 x 64 DMA tiles
    (1535, 1700, 64),        # one row short of them: 64 x 32 DMA tiles
    (70, 50, 64),            # DMA path at its smallest K
    (70, 50, 60),            # K a multiple of 4 only: 4M / register-staged 3M
    (64, 32, 8192),          # long K
]
CASES = [(M, N, K, bl, ca, cb) for (M, N, K) in SHAPES for bl in (0, 1) for (ca, cb) in CONJ]
