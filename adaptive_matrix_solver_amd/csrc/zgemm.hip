// Batched complex128 GEMM on v_mfma_f64_16x16x4_f64 (gfx950), the dense contraction of
// the MAUS hot path:
//   * LU trailing update  C -= L21 * U12            (AMS:59 -> zgetrf)
//   * population matvec   Y  = X * A^T  (= A@v per candidate row; AMS:268, 297)
//   * SVD                 S  = U * conj(A)          (A^H u per candidate; AMS:240, 301)
//   * Hermitian match     S  = conj(X) * V          (AMS:165)
//
// C[M,N] = alpha * opA(A)[M,K] * opB(B)[K,N] + beta * C     (alpha = +-1, beta in {0,1})
// A is row-major [m][k].  B is row-major [k][n] (BLAY=0) or [n][k] (BLAY=1, dot-product form).
//
// Complex product on real MFMAs (4M form, same rounding structure as a scalar FMA chain):
//   Cre += Are*Bre ; Cre += (-Aim)*Bim   (BLGP bit0 = negate A, measured on gfx950)
//   Cim += Are*Bim ; Cim += Aim*Bre
// Operand / result lane maps of v_mfma_f64_16x16x4_f64 (verified by tools/probe_mfma_f64):
//   a = A[row = lane&15][k = lane>>4], b = B[k = lane>>4][col = lane&15],
//   d[r] = D[row = (lane>>4) + 4r][col = lane&15].
//
// Tiling: BM x BN block tile, BK = 16, tiles staged through LDS as [k][m] / [k][n]
// (k-major, XOR-swizzled, see the kernel) so every fragment is one ds_read_b128 of an
// interleaved (re,im) pair; the next K-tile is prefetched into registers while the
// current one feeds the MFMAs.  The fp64 matrix pipe sustains 77.9 TFLOP/s with VGPR
// accumulators (tools/probe_mfma_f64_v2; AGPR accumulators run at less than half of that),
// but only if independent waves fill each other's waits: see zgemm_plan for the measured
// tile / occupancy choice.
//
// Population products of at most 32 rows have a split-K form of the 4M kernel behind maus_few_rows_set_method(ctx, 1)
// (zgemm_slice_kernel / zgemm_join_kernel and maus_zgemm_launch_few below); the default dispatch is unchanged.
#include "ctx.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#ifndef MAUS_WC
#define MAUS_WC 8
#endif

namespace {

// TILED (LU workspace, luws.h): A, B and C are whole matrices stored tile-major -- tiles of 64 columns, the `lda` (= ldb = ldc)
// rows of a tile contiguous at 64 elements each -- and the operands are the sub-blocks
//   A[a_rows[m]][tcol.x + k],  B[tcol.y + k][tcol.z + n],  C[c_rows[m]][tcol.z + n]        (tcol.x, .y multiples of 16).
// A K-tile of 16 columns and a 16-column C block never straddle a tile, so inside a tile everything is row-major with a
// leading dimension of 64 and only the tile base moves.
struct TCol { int x, y, z; };
__device__ __forceinline__ long tile_off(long rows, int col) { return ((long)(col >> 6) * rows << 6) + (col & 63); }

template <int BM, int BN, int BK, int WM, int WN, int BLAY, bool CONJA, bool CONJB, int MINW, bool M3 = false, bool TILED = false>
__global__ void __launch_bounds__(64 * WM * WN, MINW)
zgemm_kernel(int M, int N, int K,
             const c128* __restrict__ Ag, long lda, long strideA,
             const c128* __restrict__ Bg, long ldb, long strideB,
             c128* __restrict__ Cg, long ldc, long strideC,
             double alpha, int beta, int tiles_n, int nwg,
             const int* __restrict__ a_rows, const int* __restrict__ c_rows, long rows_stride, TCol tcol)
{
    static_assert(!TILED || (BLAY == 0 && !CONJA && !CONJB && BK == 16), "tiled operands: plain layout, K-tiles of 16");
    constexpr int NT = 64 * WM * WN;
    constexpr int WTM = BM / WM, WTN = BN / WN;      // wave tile
    constexpr int MB = WTM / 16, NB = WTN / 16;      // 16x16 blocks per wave
    // LDS images are [k][m] / [k][n] with UNPADDED rows and the element index XOR-swizzled by (k & 7).
    // ds_read_b128 is served in the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, ... (banks mod 64
    // dwords): a fragment read (lanes 0-15 -> 16 consecutive elements of row k, lanes 16-31 -> row k+1) is
    // conflict-free exactly when consecutive rows have the same bank alignment, i.e. without padding --
    // the +1 padding used before cost 33 % extra LDS cycles (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE).
    // ds_write_b128 is served in groups of 8 consecutive lanes (banks mod 32 dwords): the transposing
    // A store (8 lanes = 8 consecutive k of one row) lands on 8 different 16-B columns through the XOR,
    // which permutes inside aligned blocks of 8 and therefore keeps the reads conflict-free.
    constexpr int LDA_S = BM, LDB_S = BN;            // LDS row strides (elements)
    constexpr int A_PER = BM * BK / NT, B_PER = BN * BK / NT;
    static_assert(A_PER * NT == BM * BK && B_PER * NT == BN * BK, "tile/threads mismatch");

    constexpr int TILE_S = BK * LDA_S + BK * LDB_S;          // one staged K-tile (A then B), elements
    __shared__ c128 smem[TILE_S];

    // XCD-aware block -> tile map: blocks b and b+8 share an XCD (L2); give each XCD a
    // contiguous run of tiles so neighbouring tiles (same A row-panel) hit one L2.
    int bid = blockIdx.x;
    {
        int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    // L2 blocking: tiles are walked column-block-major (WC tile columns wide, all tile rows), so the
    // B block of the current column block (WC x BN x K) stays resident in the XCD's 4 MB L2 while the
    // A row panels stream past it once.  Row-major order re-streamed all of B for every tile row
    // (PMC: FETCH_SIZE 3.5x the algorithmic reads; profiles/r01_pmc_traffic_before_l2_blocking.txt).
    // (4 / 8 / 16 / 32 tile columns per block: 79.3-79.8 TFLOP/s at K = 512 in every case, tools/gemm_k512_check.py)
#ifndef MAUS_WC
#define MAUS_WC 8
#endif
    constexpr int WC = MAUS_WC;
    const int tiles_m = nwg / tiles_n;
    const int full = tiles_m * WC;
    int cb = bid / full, rem = bid - cb * full, wl = WC;
    const int ncb = (tiles_n + WC - 1) / WC;
    if (cb >= ncb - 1) { cb = ncb - 1; rem = bid - cb * full; wl = tiles_n - cb * WC; }
    const int tm = rem / wl, tn = cb * WC + (rem - tm * wl);
    const int m0 = tm * BM, n0 = tn * BN;
    const long batch = blockIdx.y;
    const c128* A = Ag + batch * strideA;
    const c128* B = Bg + batch * strideB;
    c128* C = Cg + batch * strideC;
    // row gather (A) / scatter (C): one index list for every matrix (rows_stride = 0: population slots, Krylov rows) or
    // one list per matrix (the LU's row permutation: implicit pivoting)
    if (a_rows) a_rows += batch * rows_stride;
    if (c_rows) c_rows += batch * rows_stride;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave - wm * WN;

    // 4M: cre / cim are the two result planes.  3M: cre = sum Are*Bre, cim = sum Aim*Bim,
    // c3 = sum (Are+Aim)*(Bre+Bim); combined in the epilogue.
    d4 cre[MB][NB], cim[MB][NB], c3[M3 ? MB : 1][M3 ? NB : 1];
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            cre[i][j] = (d4){0, 0, 0, 0}; cim[i][j] = (d4){0, 0, 0, 0};
            if (M3) c3[i][j] = (d4){0, 0, 0, 0};
        }

    c128 ra[A_PER], rb[B_PER];

    // Branch-free tile loads: per-thread base pointers are computed once (row / column indices
    // clamped into range -- out-of-range rows and columns only feed C entries that are never
    // stored), so a K-tile costs one pointer add per element inside the loop.  Only when K is not
    // a multiple of BK (KEDGE) is the k index clamped and the value zeroed by a select.
    const bool KEDGE = (K % BK) != 0;
    const c128* pa[A_PER];
    const c128* pb[B_PER];
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
        int r = tid / BK + i * (NT / BK);
        int gm = min(m0 + r, M - 1);
        pa[i] = A + (long)(a_rows ? a_rows[gm] : gm) * (TILED ? 64 : lda);
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
        if (BLAY == 0) { int gn = min(n0 + tid % BN, N - 1); pb[i] = B + (TILED ? tile_off(ldb, tcol.z + gn) + (long)tcol.y * 64 : (long)gn); }
        else { int gn = min(n0 + tid / BK + i * (NT / BK), N - 1); pb[i] = B + (long)gn * ldb; }
    }
    const long ldb_e = TILED ? 64 : ldb;             // B row step inside the operand
    // plain layout: pb[i] points at this thread's B row for k0 = 0, so the per-tile step (k0 * ldb) is wave-uniform
    if (BLAY == 0) {
#pragma unroll
        for (int i = 0; i < B_PER; ++i) pb[i] += (long)(tid / BN + i * (NT / BN)) * ldb_e;
    }
    // The loads only LOAD: zeroing the K edge and conjugation happen when the registers are written to
    // LDS one K-tile later.  (Touching the values here makes the compiler wait for the loads right away,
    // which exposes the whole L2 latency in every K-tile: measured 76 -> 87 TFLOP/s on the 3M kernel.)
    int kload = 0;                                   // k0 of the tile held in ra / rb
    auto load_tiles = [&](int k0) {
        kload = k0;
        const long ta = TILED ? tile_off(lda, tcol.x + k0) : 0;          // wave-uniform: the K-tile's place in its 64-column tile
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            int gk = k0 + (tid & (BK - 1));
            if (TILED) ra[i] = pa[i][ta + (tid & (BK - 1))];
            else ra[i] = pa[i][KEDGE ? min(gk, K - 1) : gk];
        }
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            if (BLAY == 0) {
                const int kr = tid / BN + i * (NT / BN);
                if (!KEDGE || TILED) rb[i] = pb[i][(long)k0 * ldb_e];
                else rb[i] = pb[i][(long)(min(k0 + kr, K - 1) - kr) * ldb];
            } else {
                int gk = k0 + (tid & (BK - 1));
                rb[i] = pb[i][KEDGE ? min(gk, K - 1) : gk];
            }
        }
    };
    auto store_tiles = [&](int buf) {
        c128* As = smem + buf * TILE_S;
        c128* Bs = As + BK * LDA_S;
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            int k = tid & (BK - 1), r = tid / BK + i * (NT / BK);
            c128 v = ra[i];
            if (KEDGE && kload + k >= K) v = cmake(0.0, 0.0);
            if (CONJA) v.y = -v.y;
            As[k * LDA_S + (r ^ (k & 7))] = v;
        }
        if (BLAY == 0) {
#pragma unroll
            for (int i = 0; i < B_PER; ++i) {
                int n = tid % BN, k = tid / BN + i * (NT / BN);
                c128 v = rb[i];
                if (KEDGE && kload + k >= K) v = cmake(0.0, 0.0);
                if (CONJB) v.y = -v.y;
                Bs[k * LDB_S + (n ^ (k & 7))] = v;
            }
        } else {
#pragma unroll
            for (int i = 0; i < B_PER; ++i) {
                int k = tid & (BK - 1), r = tid / BK + i * (NT / BK);
                c128 v = rb[i];
                if (KEDGE && kload + k >= K) v = cmake(0.0, 0.0);
                if (CONJB) v.y = -v.y;
                Bs[k * LDB_S + (r ^ (k & 7))] = v;
            }
        }
    };

    // ---- main loop ------------------------------------------------------------------------------
    // One LDS buffer, two barriers per K-tile: while the MFMAs of tile t run, the fragments of the next k-step are already in
    // flight (register double buffer) and tile t+1 is requested from global memory.  Made for >= 2 workgroups per CU: the
    // bubbles of one workgroup are filled by the independent waves of the others.
    const int nkt = (K + BK - 1) / BK;
    constexpr int KSTEPS = BK / 4;
    c128 fa[2][MB], fb[2][NB];
    auto read_frags = [&](int buf, int kk, int slot) {
        const c128* As = smem + buf * TILE_S;
        const c128* Bs = As + BK * LDA_S;
        const int krow = kk * 4 + (lane >> 4);
#pragma unroll
        for (int i = 0; i < MB; ++i) fa[slot][i] = As[krow * LDA_S + ((wm * WTM + i * 16 + (lane & 15)) ^ (krow & 7))];
#pragma unroll
        for (int j = 0; j < NB; ++j) fb[slot][j] = Bs[krow * LDB_S + ((wn * WTN + j * 16 + (lane & 15)) ^ (krow & 7))];
    };
    auto mfma_group = [&](int slot) {
        if (M3) {
            double as[MB], bs[NB];
#pragma unroll
            for (int i = 0; i < MB; ++i) as[i] = fa[slot][i].x + fa[slot][i].y;
#pragma unroll
            for (int j = 0; j < NB; ++j) bs[j] = fb[slot][j].x + fb[slot][j].y;
#pragma unroll
            for (int i = 0; i < MB; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    cre[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[slot][i].x, fb[slot][j].x, cre[i][j], 0, 0, 0);
                    cim[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[slot][i].y, fb[slot][j].y, cim[i][j], 0, 0, 0);
                    c3[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(as[i], bs[j], c3[i][j], 0, 0, 0);
                }
        } else {
            // first products of every block (independent accumulators back to back) ...
#pragma unroll
            for (int i = 0; i < MB; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    cre[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[slot][i].x, fb[slot][j].x, cre[i][j], 0, 0, 0);
                    cim[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[slot][i].x, fb[slot][j].y, cim[i][j], 0, 0, 0);
                }
            // ... then the second products (BLGP=1: negate A -> Cre -= Aim*Bim)
#pragma unroll
            for (int i = 0; i < MB; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    cre[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[slot][i].y, fb[slot][j].y, cre[i][j], 0, 0, 1);
                    cim[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[slot][i].y, fb[slot][j].x, cim[i][j], 0, 0, 0);
                }
        }
    };

    load_tiles(0);
    for (int kt = 0; kt < nkt; ++kt) {
        __syncthreads();
        store_tiles(0);
        __syncthreads();
        if (kt + 1 < nkt) load_tiles((kt + 1) * BK);
        read_frags(0, 0, 0);
#pragma unroll
        for (int kk = 0; kk < KSTEPS; ++kk) {
            if (kk + 1 < KSTEPS) read_frags(0, kk + 1, (kk + 1) & 1);
            mfma_group(kk & 1);
        }
    }

    // epilogue: d[r] -> row (lane>>4) + 4r, col lane&15 of each 16x16 block; per block the four old
    // C values are fetched together, then combined and stored
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int gn = n0 + wn * WTN + j * 16 + (lane & 15);
            c128 cold[4];
            long off[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gm = m0 + wm * WTM + i * 16 + (lane >> 4) + 4 * r;
                const int cm = min(gm, M - 1), cn = min(gn, N - 1);
                off[r] = TILED ? (long)(c_rows ? c_rows[cm] : cm) * 64 + tile_off(ldc, tcol.z + cn)
                               : (long)(c_rows ? c_rows[cm] : cm) * ldc + cn;
                cold[r] = cmake(0.0, 0.0);
                if (beta) cold[r] = C[off[r]];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gm = m0 + wm * WTM + i * 16 + (lane >> 4) + 4 * r;
                if (gm < M && gn < N) {
                    const double vr = M3 ? cre[i][j][r] - cim[i][j][r] : cre[i][j][r];
                    const double vi = M3 ? (c3[i][j][r] - cre[i][j][r]) - cim[i][j][r] : cim[i][j][r];
                    C[off[r]] = cmake(alpha * vr + cold[r].x, alpha * vi + cold[r].y);
                }
            }
        }
}

// ---------------------------------------------------------------------------------------
// 3M zgemm with LDS-DMA staging (plain layout, the LU trailing updates).  Same 64 x 32 workgroup tile, 2 x 2 waves and
// 32 x 16 wave tile as the register-staged 3M kernel above, but the operand tiles go global -> LDS directly
// (global_load_lds_dwordx4: no staging VGPRs, no ds_write), in K-steps of 8 through a ring of NST buffers with ONE barrier
// per step.  Without the 24 staging VGPRs the kernel fits 96 VGPRs, i.e. five workgroups per CU instead of four.
//
// An LDS-DMA wave-instruction writes 64 x 16 B contiguously (lane-linear), so the LDS images are linear and any swizzle
// goes on the per-lane SOURCE address (and, identically, on the fragment read):
//   A image [64 rows][8 k]  (128 B per row): slot (r, kk) holds A[r][k0 + (kk ^ ((r >> 1) & 7))].  One instruction fills
//       8 rows (8 lanes = one row = 128 contiguous bytes of global memory).  The fragment read a = A[row = lane&15][k = lane>>4]
//       then takes 16 rows at a 128-B stride: the row parity selects the bank half and the XOR spreads the 8 rows of equal
//       parity over the 8 16-B columns -- conflict-free in every 16-lane group the hardware forms.
//   B image [8 k][32 n]  (512 B per k-row): natural order; the fragment read b = B[k = lane>>4][col = lane&15] is 16
//       consecutive elements of one row.
// ---------------------------------------------------------------------------------------
// MB x NB = 4 x 2 (the 128 x 64 workgroup tile of the large LU updates, 64 x 32 per wave): 192 accumulator registers, so the
// kernel runs at two workgroups per CU and keeps everything else small -- see OFF32 below.  Per MFMA it reads a quarter less
// from LDS than the 32 x 32 wave tile and passes half as many barriers and DMA issues.
// BLAY = 1 (round 3): B is row-major [n][k] (dot-product form: Y = X A^T, Gram blocks, [V W][W V]^H) and gets the A image's
// treatment -- [BN rows][8 k], 8 lanes per row, the same source-side swizzle and fragment read.  CONJA / CONJB: the operand's
// imaginary part enters with the opposite sign, i.e. with a_i' = -Ai (b_i' = -Bi)
//     Re = Ar Br - a_i' b_i',   Im = (Ar + a_i')(Br + b_i') - Ar Br - a_i' b_i':
// the third product's operand sums become differences (one VALU op either way) and the epilogue takes P2 = Ai Bi with the sign
// sa sb; the MFMA stream is unchanged.  With these the population products (A@X of the Rayleigh / residual phases and of every
// GMRES inner iteration, A^H u of the SVD step, conj(X) V of the Hermitian match) run 6 M N K on the pipe instead of the 4M
// kernel's 8 M N K.
template <int NST, int MINW, int MB, int NB, bool TILED = false, int BLAY = 0, bool CONJA = false, bool CONJB = false>
__global__ void __launch_bounds__(256, MINW)
zgemm3m_dma_kernel(int M, int N, int K,
                   const c128* __restrict__ Ag, long lda, long strideA,
                   const c128* __restrict__ Bg, long ldb, long strideB,
                   c128* __restrict__ Cg, long ldc, long strideC,
                   double alpha, int beta, int tiles_n, int nwg,
                   const int* __restrict__ a_rows, const int* __restrict__ c_rows, long rows_stride, TCol tcol)
{
    constexpr int WN = 2, BM = 2 * 16 * MB, BN = WN * 16 * NB, BKS = 8;      // 2 x 2 waves, wave tile (16 MB) x (16 NB)
    constexpr int A_ST = BM * BKS, B_ST = BKS * BN;            // elements per stage
    constexpr int A_PW = BM / 32;                              // A instructions per wave and stage (8 rows each)
    constexpr int B_PW = BN / 32;                              // B instructions per wave and stage (64 elements each)
    constexpr int DMA_PW = A_PW + B_PW;
    __shared__ c128 smem[NST * (A_ST + B_ST)];

    int bid = blockIdx.x;
    {
        int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    constexpr int WC = MAUS_WC;
    const int tiles_m = nwg / tiles_n;
    const int full = tiles_m * WC;
    int cb = bid / full, rem = bid - cb * full, wl = WC;
    const int ncb = (tiles_n + WC - 1) / WC;
    if (cb >= ncb - 1) { cb = ncb - 1; rem = bid - cb * full; wl = tiles_n - cb * WC; }
    const int tm = rem / wl, tn = cb * WC + (rem - tm * wl);
    const int m0 = tm * BM, n0 = tn * BN;
    const long batch = blockIdx.y;
    const c128* A = Ag + batch * strideA;
    const c128* B = Bg + batch * strideB;
    c128* C = Cg + batch * strideC;
    if (a_rows) a_rows += batch * rows_stride;
    if (c_rows) c_rows += batch * rows_stride;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave - wm * WN;

    // per-lane DMA sources.  A: wave w issues the 8-row blocks A_PW*w .. ; B: wave w issues the 64-element pieces B_PW*w ..
    // OFF32 (the 128 x 64 tile of the LU updates, whose 192 accumulator registers leave no room for six 64-bit pointers per
    // lane): the sources are 32-bit byte offsets of the lane against a wave-uniform base.  Tile-major, everything that moves
    // with k0 or with the wave is uniform: an A source is row * 1 KB + 16 kk inside the 64-column tile of k0 (at most npad KB),
    // and the B sources of a wave differ from one per-lane column offset (per 64-column piece of the image) only by whole
    // rows of 1 KB (the columns reach at most two column tiles past the tile of n0: 2 npad KB).  global_load_lds takes
    // exactly this form (SGPR base + VGPR offset).
    constexpr bool OFF32 = TILED && BLAY == 0 && MB * NB >= 8;
    constexpr int B_CP = OFF32 ? BN / 64 : 1;                  // 64-column pieces per k-row of the B image
    static_assert(!OFF32 || (BN % 64 == 0 && B_PW % B_CP == 0), "OFF32: whole 64-column pieces");
    const c128* srcA[OFF32 ? 1 : A_PW];
    const c128* srcB[OFF32 ? 1 : B_PW];
    unsigned offA[OFF32 ? A_PW : 1], offB[OFF32 ? B_CP : 1];
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const long ldb_e = TILED ? 64 : ldb;
    static_assert(!(TILED && BLAY), "tiled operands: plain layout only");
    if constexpr (OFF32) {
#pragma unroll
        for (int j = 0; j < A_PW; ++j) {
            const int r = (A_PW * wave + j) * 8 + (lane >> 3);
            const int kk = (lane & 7) ^ ((r >> 1) & 7);
            const int gm = min(m0 + r, M - 1);
            offA[j] = (unsigned)((a_rows ? a_rows[gm] : gm) * 64 + kk) * 16u;
        }
        const int ct0 = (tcol.z + n0) >> 6;                    // column tile of the block's first column
#pragma unroll
        for (int c = 0; c < B_CP; ++c) {
            const int col = tcol.z + min(n0 + c * 64 + lane, N - 1);
            offB[c] = (unsigned)(((col >> 6) - ct0) * (int)ldb * 64 + (col & 63)) * 16u;
        }
        srcA[0] = A;
        srcB[0] = B + ((long)ct0 * ldb << 6) + (long)(tcol.y + (B_PW / B_CP) * wave_u) * 64;
    } else {
#pragma unroll
    for (int j = 0; j < A_PW; ++j) {
        const int r = (A_PW * wave + j) * 8 + (lane >> 3);
        const int kk = (lane & 7) ^ ((r >> 1) & 7);
        const int gm = min(m0 + r, M - 1);
        srcA[j] = A + (long)(a_rows ? a_rows[gm] : gm) * (TILED ? 64 : lda) + kk;
    }
#pragma unroll
    for (int j = 0; j < B_PW; ++j) {
        if (BLAY == 0) {
            const int e = (B_PW * wave + j) * 64 + lane;             // element of the [8][BN] image
            const int gn = min(n0 + (e % BN), N - 1);
            srcB[j] = B + (long)(e / BN) * ldb_e + (TILED ? tile_off(ldb, tcol.z + gn) + (long)tcol.y * 64 : (long)gn);
        } else {
            const int r = (B_PW * wave + j) * 8 + (lane >> 3);       // row of the [BN][8] image = column n of the product
            const int kk = (lane & 7) ^ ((r >> 1) & 7);
            srcB[j] = B + (long)min(n0 + r, N - 1) * ldb + kk;
        }
    }
    }

    auto issue = [&](int st, int k0) {
        c128* As = smem + st * (A_ST + B_ST);
        c128* Bs = As + A_ST;
        const long ta = TILED ? tile_off(lda, tcol.x + k0) : (long)k0;     // wave-uniform; 8 consecutive k never leave a tile
        if constexpr (OFF32) {
            // the bases pass through an SGPR constraint and the offsets through a VGPR one: otherwise loop strength reduction
            // turns base + offset back into per-lane 64-bit pointers that advance with k0, or the zero extension of the
            // offset is hoisted out of the loop and the SGPR-base form of the instruction is no longer matched.  The LDS
            // destinations (m0) come from the scalar wave number.
            const char* ba = (const char*)(srcA[0] + ta);
            const char* bb = (const char*)(srcB[0] + (long)k0 * 64);
            asm volatile("" : "+s"(ba), "+s"(bb));
#pragma unroll
            for (int j = 0; j < A_PW; ++j) {
                unsigned o = offA[j];
                asm volatile("" : "+v"(o));
                __builtin_amdgcn_global_load_lds((const void*)(ba + o), (__attribute__((address_space(3))) void*)(As + (A_PW * wave_u + j) * 64), 16, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < B_PW; ++j) {    // piece j: k-row (B_PW / B_CP) * wave + j / B_CP, columns 64 (j % B_CP) ..
                unsigned o = offB[j % B_CP];
                asm volatile("" : "+v"(o));
                if (j && j % B_CP == 0) { bb += 1024; asm volatile("" : "+s"(bb)); }
                __builtin_amdgcn_global_load_lds((const void*)(bb + o), (__attribute__((address_space(3))) void*)(Bs + (B_PW * wave_u + j) * 64), 16, 0, 0);
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < A_PW; ++j)
            __builtin_amdgcn_global_load_lds((const void*)(srcA[j] + ta), (__attribute__((address_space(3))) void*)(As + (A_PW * wave + j) * 64), 16, 0, 0);
#pragma unroll
        for (int j = 0; j < B_PW; ++j)
            __builtin_amdgcn_global_load_lds((const void*)(srcB[j] + (BLAY ? (long)k0 : (long)k0 * ldb_e)), (__attribute__((address_space(3))) void*)(Bs + (B_PW * wave + j) * 64), 16, 0, 0);
    };

    d4 cre[MB][NB], cim[MB][NB], c3[MB][NB];
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) { cre[i][j] = (d4){0, 0, 0, 0}; cim[i][j] = (d4){0, 0, 0, 0}; c3[i][j] = (d4){0, 0, 0, 0}; }

    const int nst = K / BKS;                         // K is a multiple of 8 on this path (launcher)
    // prologue: NST-1 stages in flight
#pragma unroll
    for (int s = 0; s < NST - 1; ++s) if (s < nst) issue(s, s * BKS);

    const int arow0 = wm * 16 * MB + (lane & 15);
    const int bcol0 = wn * 16 * NB + (lane & 15);
    const int q = lane >> 4;
    // OFF32: the fragment reads as three per-lane LDS byte addresses (A for each half-step: the swizzle (r >> 1) & 7 is the
    // same for every 16-row block of the wave tile; B), everything else an instruction offset
    typedef double lds_d2_t __attribute__((ext_vector_type(2)));
    typedef __attribute__((address_space(3))) const lds_d2_t lds_d2;          // one ds_read_b128
    unsigned ra[2] = {0, 0}, rb = 0;
    if constexpr (OFF32) {
        static_assert(NST == 2, "OFF32: two stages");
        const unsigned sb = (unsigned)(unsigned long)(__attribute__((address_space(3))) void*)smem;
        for (int ks = 0; ks < 2; ++ks) ra[ks] = sb + 16u * (arow0 * BKS + ((ks * 4 + q) ^ ((arow0 >> 1) & 7)));
        rb = sb + 16u * (A_ST + q * BN + bcol0);
    }
    for (int t = 0; t < nst; ++t) {
        // stage t has landed once at most NST-2 younger stages (DMA_PW instructions each) are still in flight
        if (NST >= 3 && t + NST - 2 < nst) asm volatile("s_waitcnt vmcnt(%0)" :: "n"((NST - 2) * DMA_PW) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                // everybody's part of stage t is in LDS; everybody has left stage t-1
        asm volatile("" ::: "memory");
        const c128* As = smem + (t % NST) * (A_ST + B_ST);
        const c128* Bs = As + A_ST;
        // all fragment reads of the stage BEFORE the prefetch is issued: hipcc protects the first ds_read that follows a
        // global_load_lds it has seen with s_waitcnt vmcnt(0) (possible alias); issued first, the prefetch was waited for
        // at once (seen in the .s).  Behind the reads, the next ds_read is the one after the next rendezvous.
        c128 fa[2][MB], fb[2][NB];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int k = ks * 4 + q;
#pragma unroll
            for (int i = 0; i < MB; ++i) {
                const int r = arow0 + i * 16;
                if constexpr (OFF32) { const lds_d2_t v = *(lds_d2*)(unsigned long)(ra[ks] + (t & 1) * (16u * (A_ST + B_ST)) + 16u * (i * 16 * BKS)); fa[ks][i] = cmake(v.x, v.y); }
                else fa[ks][i] = As[r * BKS + (k ^ ((r >> 1) & 7))];
            }
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const int cn = bcol0 + j * 16;
                if constexpr (OFF32) { const lds_d2_t v = *(lds_d2*)(unsigned long)(rb + (t & 1) * (16u * (A_ST + B_ST)) + 16u * (ks * 4 * BN + j * 16)); fb[ks][j] = cmake(v.x, v.y); }
                else fb[ks][j] = BLAY ? Bs[cn * BKS + (k ^ ((cn >> 1) & 7))] : Bs[k * BN + cn];
            }
        }
        if (t + NST - 1 < nst) issue((t + NST - 1) % NST, (t + NST - 1) * BKS);     // into the buffer stage t-1 used
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            double as[MB], bs[NB];
#pragma unroll
            for (int i = 0; i < MB; ++i) as[i] = CONJA ? fa[ks][i].x - fa[ks][i].y : fa[ks][i].x + fa[ks][i].y;
#pragma unroll
            for (int j = 0; j < NB; ++j) bs[j] = CONJB ? fb[ks][j].x - fb[ks][j].y : fb[ks][j].x + fb[ks][j].y;
#pragma unroll
            for (int i = 0; i < MB; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    cre[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[ks][i].x, fb[ks][j].x, cre[i][j], 0, 0, 0);
                    cim[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[ks][i].y, fb[ks][j].y, cim[i][j], 0, 0, 0);
                    c3[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(as[i], bs[j], c3[i][j], 0, 0, 0);
                }
        }
    }
    constexpr double S2 = (CONJA != CONJB) ? -1.0 : 1.0;       // sign of P2 = Ai Bi in the result (sa sb)

    // epilogue (as in zgemm_kernel)
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int gn = n0 + wn * 16 * NB + j * 16 + (lane & 15);
            c128 cold[4];
            long off[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gm = m0 + wm * 16 * MB + i * 16 + (lane >> 4) + 4 * r;
                const int cm = min(gm, M - 1), cn = min(gn, N - 1);
                off[r] = TILED ? (long)(c_rows ? c_rows[cm] : cm) * 64 + tile_off(ldc, tcol.z + cn)
                               : (long)(c_rows ? c_rows[cm] : cm) * ldc + cn;
                cold[r] = cmake(0.0, 0.0);
                if (beta) cold[r] = C[off[r]];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gm = m0 + wm * 16 * MB + i * 16 + (lane >> 4) + 4 * r;
                if (gm < M && gn < N) {
                    const double vr = cre[i][j][r] - S2 * cim[i][j][r];
                    const double vi = (c3[i][j][r] - cre[i][j][r]) - S2 * cim[i][j][r];
                    C[off[r]] = cmake(alpha * vr + cold[r].x, alpha * vi + cold[r].y);
                }
            }
        }
}

// ---------------------------------------------------------------------------------------
// Split-K population products for at most 32 rows (maus_few_rows_set_method(ctx, 1); DESIGN §3 "Few rows").  The 4M kernels above
// give a product of up to 32 rows ceil(N / 32) workgroups, each walking the whole K alone: M = 15 against 8192 x 8192 occupies
// one workgroup per CU and reads the operand at a third of the copy rate; a Gram block of 32 rows is ONE workgroup.  Here K is
// cut into S slices (few_slices below) and every (column tile, slice) is a workgroup of its own: the K-range form of the
// register-staged 4M kernel -- same LDS images, same fragment reads, the same four real MFMA products per complex one, hence the
// componentwise bound on the imaginary part -- on a BM x 64 tile, BM = 16 for up to 16 rows (no MFMA on padding rows) and 32
// above.  An element's partial sum is one MFMA chain over its slice in k order whatever BM is, so a row's bits depend on neither.
// Slice s of tile t writes its BM x 64 partial sums, all of them, to slab (s, t) of the context's workspace; zgemm_join_kernel,
// the next launch on the same stream, adds the slabs of an element in the order 0, 1, .., S - 1 and applies the epilogue.  The
// launch boundary is the only synchronisation: no counters, no flags, no atomics, nothing that waits.
// ---------------------------------------------------------------------------------------
constexpr int FEW_BN = 64, FEW_SLAB = 32 * FEW_BN;       // a slab holds 32 x 64 partial sums whatever BM is

template <int BM, int BLAY, bool CONJA, bool CONJB>
__global__ void __launch_bounds__(256, 4)
zgemm_slice_kernel(int M, int N, int K, const c128* __restrict__ A, long lda, const c128* __restrict__ B, long ldb,
                   c128* __restrict__ ws, int q, int r, const int* __restrict__ a_rows)
{
    constexpr int BN = FEW_BN, BK = 16, NT = 256, WN = 4;
    constexpr int WTN = BN / WN, MB = BM / 16;       // 1 x 4 waves, BM x 16 per wave
    constexpr int A_PER = BM * BK / NT, B_PER = BN * BK / NT;
    static_assert(A_PER >= 1 && WTN == 16, "tile/threads mismatch");
    __shared__ c128 smem[BK * BM + BK * BN];         // [k][m] then [k][n], XOR-swizzled as in zgemm_kernel
    c128* As = smem;
    c128* Bs = smem + BK * BM;

    // slice s covers the 16-column chunks [s q + min(s, r), (s + 1) q + min(s + 1, r)); the last one also takes K % 16
    const int s = blockIdx.y, S = gridDim.y, tn = blockIdx.x;
    const int kb = 16 * (s * q + min(s, r));
    const int ke = (s + 1 == S) ? K : 16 * ((s + 1) * q + min(s + 1, r));
    const int n0 = tn * BN;
    const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;

    d4 cre[MB], cim[MB];
#pragma unroll
    for (int i = 0; i < MB; ++i) { cre[i] = (d4){0, 0, 0, 0}; cim[i] = (d4){0, 0, 0, 0}; }

    c128 ra[A_PER], rb[B_PER];
    const bool KEDGE = ((ke - kb) % BK) != 0;
    const c128* pa[A_PER];
    const c128* pb[B_PER];
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
        const int gm = min(tid / BK + i * (NT / BK), M - 1);
        pa[i] = A + (long)(a_rows ? a_rows[gm] : gm) * lda;
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
        if (BLAY == 0) pb[i] = B + (long)min(n0 + tid % BN, N - 1) + (long)(tid / BN + i * (NT / BN)) * ldb;
        else pb[i] = B + (long)min(n0 + tid / BK + i * (NT / BK), N - 1) * ldb;
    }
    int kload = kb;
    auto load_tiles = [&](int k0) {
        kload = k0;
        const int gk = k0 + (tid & (BK - 1));
#pragma unroll
        for (int i = 0; i < A_PER; ++i) ra[i] = pa[i][KEDGE ? min(gk, ke - 1) : gk];
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            if (BLAY == 0) {
                const int kr = tid / BN + i * (NT / BN);
                rb[i] = pb[i][(long)((KEDGE ? min(k0 + kr, ke - 1) : k0 + kr) - kr) * ldb];
            } else rb[i] = pb[i][KEDGE ? min(gk, ke - 1) : gk];
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            const int k = tid & (BK - 1), m = tid / BK + i * (NT / BK);
            c128 v = ra[i];
            if (KEDGE && kload + k >= ke) v = cmake(0.0, 0.0);
            if (CONJA) v.y = -v.y;
            As[k * BM + (m ^ (k & 7))] = v;
        }
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const int k = BLAY == 0 ? tid / BN + i * (NT / BN) : (tid & (BK - 1));
            const int n = BLAY == 0 ? tid % BN : tid / BK + i * (NT / BK);
            c128 v = rb[i];
            if (KEDGE && kload + k >= ke) v = cmake(0.0, 0.0);
            if (CONJB) v.y = -v.y;
            Bs[k * BN + (n ^ (k & 7))] = v;
        }
    };
    c128 fa[2][MB], fb[2];
    auto read_frags = [&](int kk, int slot) {
        const int krow = kk * 4 + (lane >> 4);
#pragma unroll
        for (int i = 0; i < MB; ++i) fa[slot][i] = As[krow * BM + ((i * 16 + (lane & 15)) ^ (krow & 7))];
        fb[slot] = Bs[krow * BN + ((wn * WTN + (lane & 15)) ^ (krow & 7))];
    };

    const int nkt = (ke - kb + BK - 1) / BK;
    load_tiles(kb);
    for (int kt = 0; kt < nkt; ++kt) {
        __syncthreads();
        store_tiles();
        __syncthreads();
        if (kt + 1 < nkt) load_tiles(kb + (kt + 1) * BK);
        read_frags(0, 0);
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            if (kk + 1 < BK / 4) read_frags(kk + 1, (kk + 1) & 1);
            const int sl = kk & 1;
#pragma unroll
            for (int i = 0; i < MB; ++i) {
                cre[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[sl][i].x, fb[sl].x, cre[i], 0, 0, 0);
                cim[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[sl][i].x, fb[sl].y, cim[i], 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < MB; ++i) {
                cre[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[sl][i].y, fb[sl].y, cre[i], 0, 0, 1);   // BLGP = 1: Cre -= Aim Bim
                cim[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[sl][i].y, fb[sl].x, cim[i], 0, 0, 0);
            }
        }
    }

    // the whole BM x 64 slab, padding rows and columns included (finite or not, the join reads only rows < M, columns < N)
    c128* P = ws + ((size_t)s * gridDim.x + tn) * FEW_SLAB;
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
            P[(i * 16 + (lane >> 4) + 4 * rr) * BN + wn * WTN + (lane & 15)] = cmake(cre[i][rr], cim[i][rr]);
}

// C[c_rows[m]][n] = alpha * (slab 0 + slab 1 + .. + slab S-1)[m][n] + (beta ? C : 0) for m < M, n < N: one thread per element
__global__ void __launch_bounds__(256)
zgemm_join_kernel(int M, int N, int S, int tiles_n, const c128* __restrict__ ws, c128* __restrict__ C, long ldc,
                  double alpha, int beta, const int* __restrict__ c_rows)
{
    const int n = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
    if (n >= N || m >= M) return;
    const c128* p = ws + (size_t)(n / FEW_BN) * FEW_SLAB + m * FEW_BN + (n % FEW_BN);
    const size_t step = (size_t)tiles_n * FEW_SLAB;
    double vr = p[0].x, vi = p[0].y;
    for (int s = 1; s < S; ++s) { const c128 t = p[s * step]; vr += t.x; vi += t.y; }
    const long off = (long)(c_rows ? c_rows[m] : m) * ldc + n;
    c128 cold = cmake(0.0, 0.0);
    if (beta) cold = C[off];
    C[off] = cmake(alpha * vr + cold.x, alpha * vi + cold.y);
}

// The slicing rule, stated once (maus_few_rows_plan / maus_few_rows_kernel_for report it; tests ask them).  S depends on
// (N, K, layout) only -- never on M, the batch, the slots or the device -- so a candidate's row has the same bits alone and
// among 32.  Aim: FEW_TARGET_WG workgroups over the ceil(N / 64) column tiles, no slice shorter than FEW_MIN_SLICE, at most 32
// slices; constants from the sweep of tools/few_rows_rates.py (profiles/few_rows_rates.txt).  The layout does not enter yet.
constexpr int FEW_TARGET_WG = 1024, FEW_MIN_SLICE = 256, FEW_MAX_S = 32;
int few_rule(int N, int K, int /*blay*/)
{
    const int tiles = (N + FEW_BN - 1) / FEW_BN;
    int S = FEW_TARGET_WG / tiles;
    if (S > K / FEW_MIN_SLICE) S = K / FEW_MIN_SLICE;
    if (S > FEW_MAX_S) S = FEW_MAX_S;
    return S < 1 ? 1 : S;
}

// MAUS_LU_TILE=64x64|128x64 (read once per process): the workgroup tile of the large LU trailing updates, for timing one tile
// against the other in one binary and for comparing their bits.  128x64: every update with M, N >= MAUS_LU_LT_MIN on the DMA
// path, whatever its K; 64x64: the rule before the 128 x 64 tile (64 x 64 from 1536).  Unset: the rule of zgemm_plan.
int lu_tile_mode()
{
    static const int mode = [] {
        const char* e = getenv("MAUS_LU_TILE");
        if (!e || !*e) return (int)MAUS_LU_TILE_DEFAULT;
        if (!strcmp(e, "128x64")) return (int)MAUS_LU_TILE_128X64;
        if (!strcmp(e, "64x64")) return (int)MAUS_LU_TILE_64X64;
        fprintf(stderr, "MAUS_LU_TILE=%s: expected 64x64 or 128x64\n", e);
        abort();
        return 0;
    }();
    return mode;
}

// ---- dispatch: one plan, one launch table ------------------------------------------------------------------------------------
// zgemm_plan is the rule "which kernel does a product run", stated once for the rows form (maus_zgemm_launch_rows and what calls
// it) and the LU form (maus_zgemm_launch_lu): host arithmetic on its arguments, nothing read from the environment or a device.
// maus_zgemm_plan exports it, and tests/test_zgemm_plan_host.py holds it against the independent statement of
// tests/zgemm_cases.py on both sides of every threshold below.
//
// All kernels: 4 waves per workgroup and registers / LDS small enough for 2-5 INDEPENDENT workgroups per CU.  Measured on MI355X
// (profiles/r01_gemm_sweep_configs.txt, r02_zgemm_tile_variants_small_shapes.txt; K = 256, 136 matrices, 8MNK-equivalent
// TFLOP/s): every one-workgroup-per-CU shape (128 x 64 / 128 x 128, BK 16 / 32, software-pipelined or not) stays at 50-59 -- with
// all waves of a SIMD in one workgroup they run in lockstep and every wait or barrier of one is a bubble for all; 8-wave
// workgroups lose to 4-wave ones at equal tile area.  The variants that lost those sweeps are gone.
// What the plan can answer: kernel family and workgroup tile BM x BN.  with_kernel below turns each into its instantiation.
enum ZgemmKind { ZG_4M_128x16, ZG_4M_16x128, ZG_4M_64x64, ZG_4M_32x64, ZG_4M_32x32, ZG_3M_32x64, ZG_3M_64x32,
                 ZG_DMA_64x32, ZG_DMA_64x64, ZG_DMA_128x64 };

// Plain layout without conjugation (LU workspaces, row-major workspaces of the GMRES path, host-matrix entry points): skinny
// shapes keep the workgroup tile shaped like the problem so that no MFMA runs on padding.
constexpr int ZG_SKINNY_N = 16;                  // N <= 16: 128 x 16 tiles
constexpr int ZG_SKINNY_M = 16;                  // M <= 16: 16 x 128 tiles
constexpr int ZG_FEW_M = 32;                     // M <= 32: one 32-row tile, never DMA-staged
// The LDS-DMA staged 3M kernel, in K-steps of 8 through a ring of two buffers.  3584 x 3616 x 512, 136 matrices: register-staged
// kernel 79.2; DMA staging, 64 x 32 tiles, five workgroups per CU 86.8 (prefetch issued behind the fragment reads); 64 x 64 tiles
// at three workgroups per CU 88.7 on large updates (86.3 at 1024 x 1056: the 64 x 32 form is kept below 1536).  Same summation
// order as the register-staged kernel, hence the same bits.  It has every layout / conjugation form but the doubly conjugated.
// (64 x 64 tiles from M >= 1024 / 512 and N >= 128 / 256 / 1024, or only from 2048: the 181-solve sweep stays within 0.5 ms of
// 494 ms -- the K = 128 / 256 levels are not bound by the tile shape.)
constexpr int ZG_DMA_KSTEP = 8, ZG_DMA_KMIN = 64;
constexpr int ZG_DMA_BIG = 1536;                 // M, N >= 1536: 64 x 64 tiles
// LU form only: 128 x 64 tiles (64 x 32 per wave: a quarter less LDS traffic per MFMA than the 32 x 32 wave tile, half the barriers
// and DMA issues), two workgroups per CU, for the outer updates: 90.4 against 88.4 at 3584 x 3616 x 512 and 86.6 against 84.9
// (64 x 32 tiles) at 1024 x 1056 x 512, 181 matrices; the 64 x 128 tile stayed at 64 x 64's rate (89.1) and is gone
// (profiles/zgemm_large_tile_rates.txt).  Same summation order, same bits.  Only where the grid is at least eight rounds of the
// 512 workgroups the chip holds: with fewer, larger tiles the last, partly filled round weighs more (one to eight matrices: 37-66
// against 47-70 at 1024, 46 / 62 against 58 / 69 at 1536 with one / two matrices, equal from 1200-3200 tiles on).
#ifndef MAUS_LU_LT_MIN
#define MAUS_LU_LT_MIN 1024
#endif
constexpr int ZG_LT_MIN = MAUS_LU_LT_MIN, ZG_LT_KMIN = 256, ZG_LT_TILES = 4096;
// 4M for what is left of the population products (a handful of candidates, K not a multiple of 8, both operands conjugated):
// 64 x 64 tiles, 32 x 32 wave tile; with the next K-tile genuinely in flight during the MFMAs this needs ~160 VGPRs: three
// workgroups per CU.  A population of a few hundred candidates against an n x n matrix gives few such tiles (M = 512, N = 2048:
// 256 -- one workgroup on each CU where three fit): below two tiles per CU the tile shrinks to 32 x 64 / 32 x 32 so that the grid
// covers the chip (M = 15 against 8192 x 8192 runs 0.57 ms per product on 256 workgroups of 32 x 32, 0.86 on 128 of 64 x 64).
constexpr int ZG_4M_TILES = 512;

ZgemmKind zgemm_plan(int form, int lu_tile, int M, int N, int K, int batch, int blay, bool conja, bool conjb)
{
    const bool plain = blay == 0 && !conja && !conjb;
    auto tiles = [&](int bm, int bn) { return (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn) * batch; };
    if (plain && N <= ZG_SKINNY_N) return ZG_4M_128x16;
    if (plain && M <= ZG_SKINNY_M) return ZG_4M_16x128;
    const bool few = M <= ZG_FEW_M;
    if (!few && K % ZG_DMA_KSTEP == 0 && K >= ZG_DMA_KMIN && !(conja && conjb)) {
        if (form == MAUS_ZGEMM_LU && M >= ZG_LT_MIN && N >= ZG_LT_MIN &&
            (lu_tile == MAUS_LU_TILE_128X64 || (lu_tile == MAUS_LU_TILE_DEFAULT && K >= ZG_LT_KMIN && tiles(128, 64) >= ZG_LT_TILES)))
            return ZG_DMA_128x64;
        return M >= ZG_DMA_BIG && N >= ZG_DMA_BIG ? ZG_DMA_64x64 : ZG_DMA_64x32;
    }
    // 3M complex product on the register-staged kernel: three real MFMA products per complex one (ArBr, AiBi, (Ar+Ai)(Br+Bi)); a
    // 32 x 16 wave tile keeps the three accumulator planes, the fragments and the in-flight prefetch of the next K-tile inside 128
    // VGPRs.  Error is normwise the same as 4M (9.5e-16 vs 1.1e-15 relative on random data); the imaginary part loses its
    // componentwise bound, which LU with partial pivoting does not rely on.
    if (plain) return few ? ZG_3M_32x64 : ZG_3M_64x32;
    if (tiles(64, 64) >= ZG_4M_TILES) return ZG_4M_64x64;
    if (tiles(32, 64) >= ZG_4M_TILES) return ZG_4M_32x64;
    return ZG_4M_32x32;
}

// Runtime (layout, conj A, conj B) -> compile-time constants: f(BLAY, CONJA, CONJB) with three std::integral_constant values.
// Every kernel family that has such forms goes through here and leaves out the ones it lacks with `if constexpr`.
template <class F>
void with_form(int blay, bool conja, bool conjb, F&& f)
{
    auto conj = [&](auto bl) {
        if (conja) { if (conjb) f(bl, std::true_type{}, std::true_type{}); else f(bl, std::true_type{}, std::false_type{}); }
        else { if (conjb) f(bl, std::false_type{}, std::true_type{}); else f(bl, std::false_type{}, std::false_type{}); }
    };
    if (blay) conj(std::integral_constant<int, 1>{}); else conj(std::integral_constant<int, 0>{});
}

struct ZgemmArgs {
    hipStream_t st; int M, N, K;
    const c128* A; long lda, sA; const c128* B; long ldb, sB; c128* C; long ldc, sC;
    double alpha; int beta, batch; const int* a_rows; const int* c_rows; long rows_stride; TCol tcol;
};

// The launch table: kind -> instantiation, each named once.  f(kernel, family, BM, BN, threads per workgroup) is called with the
// kernel of `kind` for this form; false where the form has none (the rule never asks for one: tests/test_zgemm_plan_host.py
// walks the rule through this table by way of maus_zgemm_plan).  zgemm_kernel and zgemm3m_dma_kernel take the same arguments, so
// every entry has the same type.  TILED (the LU form) has the plain layout only; the 128 x 64 DMA tile is its alone; the DMA
// kernel has no doubly conjugated form and the 4M tiles of the population products no plain one.
template <bool TILED, int BLAY, bool CONJA, bool CONJB, class F>
bool with_kernel(ZgemmKind kind, F&& f)
{
    constexpr bool PLAIN = BLAY == 0 && !CONJA && !CONJB, DMA_FORM = !(CONJA && CONJB);
    static_assert(PLAIN || !TILED, "tiled operands: plain layout only");
#define REG(BM, BN, WM, WN, MINW, M3) (f(zgemm_kernel<BM, BN, 16, WM, WN, BLAY, CONJA, CONJB, MINW, M3, TILED>, \
                                         M3 ? MAUS_ZGEMM_3M : MAUS_ZGEMM_4M, BM, BN, 64 * WM * WN), true)
#define DMA(MINW, MB, NB) (f(zgemm3m_dma_kernel<2, MINW, MB, NB, TILED, BLAY, CONJA, CONJB>, MAUS_ZGEMM_3M_DMA, 32 * MB, 32 * NB, 256), true)
    switch (kind) {                                          // no default: a kind without a case is a compiler warning
    case ZG_4M_128x16: if constexpr (PLAIN) return REG(128, 16, 4, 1, 4, false); break;
    case ZG_4M_16x128: if constexpr (PLAIN) return REG(16, 128, 1, 4, 3, false); break;
    case ZG_3M_32x64: if constexpr (PLAIN) return REG(32, 64, 1, 4, 4, true); break;
    case ZG_3M_64x32: if constexpr (PLAIN) return REG(64, 32, 2, 2, 4, true); break;
    case ZG_4M_64x64: if constexpr (!PLAIN) return REG(64, 64, 2, 2, 3, false); break;
    case ZG_4M_32x64: if constexpr (!PLAIN) return REG(32, 64, 1, 4, 4, false); break;
    case ZG_4M_32x32: if constexpr (!PLAIN) return REG(32, 32, 2, 2, 4, false); break;
    case ZG_DMA_64x32: if constexpr (DMA_FORM) return DMA(5, 2, 1); break;                     // five workgroups per CU
    case ZG_DMA_64x64: if constexpr (DMA_FORM) return DMA(3, 2, 2); break;                     // three
    case ZG_DMA_128x64: if constexpr (TILED) return DMA(2, 4, 2); break;                       // two
    }
#undef REG
#undef DMA
    return false;
}

// one grid of ceil(M / BM) x ceil(N / BN) tiles per matrix; a kind without a kernel for the form is an error, never another kernel
template <bool TILED, int BLAY, bool CONJA, bool CONJB>
void launch_kind(ZgemmKind kind, const ZgemmArgs& a)
{
    const bool found = with_kernel<TILED, BLAY, CONJA, CONJB>(kind, [&](auto kernel, int, int BM, int BN, int threads) {
        const int tiles_n = (a.N + BN - 1) / BN, nwg = (a.M + BM - 1) / BM * tiles_n;
        hipLaunchKernelGGL(kernel, dim3(nwg, a.batch), dim3(threads), 0, a.st, a.M, a.N, a.K, a.A, a.lda, a.sA, a.B, a.ldb, a.sB,
                           a.C, a.ldc, a.sC, a.alpha, a.beta, tiles_n, nwg, a.a_rows, a.c_rows, a.rows_stride, a.tcol);
    });
    if (!found) { fprintf(stderr, "zgemm: no kernel of kind %d for layout %d, conj %d %d\n", (int)kind, BLAY, CONJA, CONJB); abort(); }
}

}  // namespace

// Host-side launcher (device pointers).  batch matrices at element strides sA/sB/sC.
// a_rows / c_rows (device int arrays of length M, or null): row gather for A / row scatter
// for C -- the population's candidate vectors live in arbitrary slots of one array.
void maus_zgemm_launch_rows(hipStream_t st, int M, int N, int K, const c128* A, long lda, long sA,
                            const c128* B, long ldb, long sB, c128* C, long ldc, long sC,
                            double alpha, int beta, int batch, int blay, bool conja, bool conjb,
                            const int* a_rows, const int* c_rows, long rows_stride)
{
    if (M <= 0 || N <= 0 || batch <= 0) return;
    const ZgemmKind kind = zgemm_plan(MAUS_ZGEMM_ROWS, MAUS_LU_TILE_DEFAULT, M, N, K, batch, blay, conja, conjb);
    const ZgemmArgs a{st, M, N, K, A, lda, sA, B, ldb, sB, C, ldc, sC, alpha, beta, batch, a_rows, c_rows, rows_stride, TCol{0, 0, 0}};
    with_form(blay, conja, conjb, [&](auto bl, auto ca, auto cb) { launch_kind<false, decltype(bl)::value, decltype(ca)::value, decltype(cb)::value>(kind, a); });
}

// LU trailing update on the tile-major workspace (luws.h):  H[rows[m]][ccol + n] -= H[rows[m]][acol + k] * U[brow + k][ccol + n]
// for m < M, n < N, k < K, all `batch` matrices (element stride `stride`, `nrows` rows per 64-column tile); rows = the LU's
// per-matrix row permutation (rows_stride apart).
void maus_zgemm_launch_lu(hipStream_t st, int M, int N, int K, const c128* H, const c128* U, c128* Hc, long nrows, long stride,
                          int acol, int brow, int ccol, int batch, const int* rows, long rows_stride)
{
    if (M <= 0 || N <= 0 || K <= 0 || batch <= 0) return;
    const ZgemmKind kind = zgemm_plan(MAUS_ZGEMM_LU, lu_tile_mode(), M, N, K, batch, 0, false, false);
    launch_kind<true, 0, false, false>(kind, ZgemmArgs{st, M, N, K, H, nrows, stride, U, nrows, stride, Hc, nrows, stride, -1.0, 1, batch,
                                                        rows, rows, rows_stride, TCol{acol, brow, ccol}});
}

void maus_zgemm_launch_idx(hipStream_t st, int M, int N, int K, const c128* A, long lda, long sA,
                           const c128* B, long ldb, long sB, c128* C, long ldc, long sC,
                           double alpha, int beta, int batch, int blay, bool conja, bool conjb,
                           const int* a_rows, const int* c_rows)
{
    maus_zgemm_launch_rows(st, M, N, K, A, lda, sA, B, ldb, sB, C, ldc, sC, alpha, beta, batch, blay, conja, conjb, a_rows, c_rows, 0);
}

void maus_zgemm_launch(hipStream_t st, int M, int N, int K, const c128* A, long lda, long sA,
                       const c128* B, long ldb, long sB, c128* C, long ldc, long sC,
                       double alpha, int beta, int batch, int blay, bool conja, bool conjb)
{
    maus_zgemm_launch_idx(st, M, N, K, A, lda, sA, B, ldb, sB, C, ldc, sC, alpha, beta, batch, blay, conja, conjb, nullptr, nullptr);
}

// ---- few rows: the split-K method (kernels and rule above) ------------------------------------------------------------------
// S of a product under (method, forced slices), 0 where the default kernels run.  Host arithmetic only.
static int few_plan(int method, int forced, int M, int N, int K, int batch, int blay, bool conja, bool conjb)
{
    if (method != 1 || M < 1 || M > 32 || N < 1 || K < 1 || batch != 1) return 0;
    if (blay == 0 && !conja && !conjb) return 0;             // plain products keep the LU family's kernels
    int S = forced > 0 ? forced : few_rule(N, K, blay);
    if (S > K / 16) S = K / 16;                              // no slice shorter than 16
    return S >= 2 ? S : 0;
}

template <int BM, int BLAY, bool CONJA, bool CONJB>
static void launch_slices(hipStream_t st, int M, int N, int K, const c128* A, long lda, const c128* B, long ldb, c128* ws,
                          int tiles_n, int S, const int* a_rows)
{
    const int T = K / 16;
    hipLaunchKernelGGL((zgemm_slice_kernel<BM, BLAY, CONJA, CONJB>), dim3(tiles_n, S), dim3(256), 0, st,
                       M, N, K, A, lda, B, ldb, ws, T / S, T % S, a_rows);
}

// The population products of capi.hip go through here.  Split-K when the context's method is 1, M <= 32, batch = 1, the form
// is a dot-product layout or a conjugated operand, and the rule gives S >= 2; maus_zgemm_launch_idx, unchanged, otherwise.
// NOT routed here, on purpose: the GMRES products (gmres.hip pads them to 33 rows so that a candidate's iterate does not depend
// on how many others are still active), every LU, band, sparse (c->csr) and Lanczos path, and maus_herm_match_rows.  The
// kept-product stamps (capi.hip: av_family) are untouched: products of up to 32 rows leave none under either method.
int maus_zgemm_launch_few(maus_ctx* c, int M, int N, int K, const c128* A, long lda, long sA,
                          const c128* B, long ldb, long sB, c128* C, long ldc, long sC,
                          double alpha, int beta, int batch, int blay, bool conja, bool conjb,
                          const int* a_rows, const int* c_rows)
{
    const int S = few_plan(c->few_method, c->few_slices, M, N, K, batch, blay, conja, conjb);
    if (S == 0) {
        maus_zgemm_launch_idx(c->st, M, N, K, A, lda, sA, B, ldb, sB, C, ldc, sC, alpha, beta, batch, blay, conja, conjb, a_rows, c_rows);
        return 0;
    }
    // workspace: S slabs per column tile, sized from (S, N) alone -- never from ldp or the capacity, which a later
    // maus_set_matrix / maus_pop_reserve may change.  Grown when a call needs more, never shrunk, freed with the context.
    const int tiles_n = (N + FEW_BN - 1) / FEW_BN;
    const size_t need = (size_t)S * tiles_n * FEW_SLAB;
    if (need > c->few_ws_elems) {
        HIPCHK(c, hipStreamSynchronize(c->st));              // an earlier join may still read the old one
        if (c->few_ws) { (void)hipFree(c->few_ws); c->few_ws = nullptr; c->few_ws_elems = 0; }
        HIPCHK(c, hipMalloc((void**)&c->few_ws, sizeof(c128) * need));
        c->few_ws_elems = need;
        ++c->few_allocs;
    }
    with_form(blay, conja, conjb, [&](auto bl, auto ca, auto cb) {
        constexpr int BL = decltype(bl)::value; constexpr bool CA = decltype(ca)::value, CB = decltype(cb)::value;
        if constexpr (BL != 0 || CA || CB) {                 // few_plan: a plain product never gets here
            if (M <= 16) launch_slices<16, BL, CA, CB>(c->st, M, N, K, A, lda, B, ldb, c->few_ws, tiles_n, S, a_rows);
            else launch_slices<32, BL, CA, CB>(c->st, M, N, K, A, lda, B, ldb, c->few_ws, tiles_n, S, a_rows);
        }
    });
    hipLaunchKernelGGL(zgemm_join_kernel, dim3((N + 255) / 256, M), dim3(256), 0, c->st, M, N, S, tiles_n, c->few_ws, C, ldc, alpha, beta, c_rows);
    return 0;
}

extern "C" {

int maus_few_rows_set_method(maus_ctx* c, int method, int slices) {
    if (!c) return -1;
    if (method != 0 && method != 1) FAIL(c, "maus_few_rows_set_method: method must be 0 (default) or 1 (split-K)");
    if (slices < 0 || slices > 32) FAIL(c, "maus_few_rows_set_method: slices must be 0 (the rule) or 1..32");
    c->few_method = method;
    c->few_slices = slices;
    return 0;
}

int maus_few_rows_get_method(maus_ctx* c) { return c ? c->few_method : -1; }

int maus_few_rows_plan(int method, int slices, int M, int N, int K, int b_layout, int conj_a, int conj_b, int* slices_out) {
    if ((method != 0 && method != 1) || slices < 0 || slices > 32 || M < 1 || N < 1 || K < 1 || (b_layout != 0 && b_layout != 1)) return -1;
    const int S = few_plan(method, slices, M, N, K, 1, b_layout, conj_a != 0, conj_b != 0);
    if (slices_out) *slices_out = S ? S : 1;
    return S ? 1 : 0;
}

int maus_few_rows_kernel_for(maus_ctx* c, int M, int N, int K, int b_layout, int conj_a, int conj_b, int* slices_out) {
    if (!c) return -1;
    const int k = maus_few_rows_plan(c->few_method, c->few_slices, M, N, K, b_layout, conj_a, conj_b, slices_out);
    if (k < 0) FAIL(c, "maus_few_rows_kernel_for: bad sizes or layout");
    return k;
}

int maus_few_rows_workspace_allocs(maus_ctx* c) { return c ? c->few_allocs : -1; }

int maus_zgemm_plan(int form, int lu_tile, int M, int N, int K, int batch, int b_layout, int conj_a, int conj_b, int* bm_out, int* bn_out) {
    if ((form != MAUS_ZGEMM_ROWS && form != MAUS_ZGEMM_LU) || lu_tile < MAUS_LU_TILE_DEFAULT || lu_tile > MAUS_LU_TILE_128X64) return -1;
    if (M < 1 || N < 1 || K < 1 || batch < 1 || (b_layout != 0 && b_layout != 1)) return -1;
    if (form == MAUS_ZGEMM_LU && (b_layout || conj_a || conj_b)) return -1;
    // through the launch table, as the launchers go: -1 if it had no kernel of the plan's kind for this form
    const ZgemmKind kind = zgemm_plan(form, lu_tile, M, N, K, batch, b_layout, conj_a != 0, conj_b != 0);
    int family = -1;
    auto report = [&](auto, int fam, int bm, int bn, int) { family = fam; if (bm_out) *bm_out = bm; if (bn_out) *bn_out = bn; };
    if (form == MAUS_ZGEMM_LU) with_kernel<true, 0, false, false>(kind, report);
    else with_form(b_layout, conj_a != 0, conj_b != 0, [&](auto bl, auto ca, auto cb) {
        with_kernel<false, decltype(bl)::value, decltype(ca)::value, decltype(cb)::value>(kind, report); });
    return family;
}

}  // extern "C"
