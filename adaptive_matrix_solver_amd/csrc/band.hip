// Batched band LU with partial pivoting for sparse problem matrices above the dense LU's n (gfx950).
//
// A sparse matrix is bound once with an ordering perm (band.py: reverse Cuthill-McKee or the identity); B = A[perm][:, perm]
// has kl subdiagonals and ku superdiagonals.  Every solve of maus_band_solve
//     builds    H_k = B - lambda_k I + psi_k I  in LAPACK band storage (zgbtrf layout, ldab = 2 kl + ku + 1, column-major:
//               element (i, j) at row kv + i - j of column j, kv = kl + ku; the first kl rows take the fill of U),
//               and the permuted right-hand side X[slot][perm] (eigenproblems) or b[perm] (linear systems),
//     factors   it as zgbtf2 does (pivot = first maximum of |re| + |im| among the kl + 1 candidates of the column, ipiv and info
//               as LAPACK's), applying L to the right-hand side column by column as zgbtrs would afterwards,
//     solves    U x = y as ztbsv does and writes x back in the original order into W[slot].
//
// Schedule: one workgroup per matrix walks all n columns; the work of a column (pivot search, interchange of two rows over
// the columns the pivot row reaches, the kl x (kl + ku) rank-1 update) is spread over the workgroup.  Every element of the
// band is changed by exactly one thread at each column step, by one fused multiply-subtract, and the pivot search is an exact
// maximum with the lowest index among equals: there is no summation order that the workgroup size or the batch could change.
// The workgroup size is picked from (kl, ku) alone and only decides who does what.  A candidate's W row is therefore
// bit-identical alone, in any batch and in any chunking of the workspace (DESIGN §9's rule).
//
// That is the column kernel, the default.  maus_band_set_method(ctx, 1) selects the blocked method further down (zgbtrf's
// schedule, every step a launch over (matrix, tile)) for bands with BLK_MIN_KL <= kl <= BLK_MAX_KL; same storage, build kernel,
// pivot rule and status contract.  maus_band_set_method(ctx, 2) selects the tiled method after it (the blocked schedule with the
// block row and the trailing update as launches of their own over (column tile, row tile)) for kl up to TIL_MAX_KL.
// maus_band_set_method(ctx, 4) selects the wide method at the end (zgbtrf's two levels: outer blocks of 64 columns factored by
// the tiled steps, then one rank-64 update on the MFMA pipe) for WID_MIN_KL <= kl <= WID_MAX_KL.
// maus_band_set_method(ctx, 8) selects the narrow method (the column kernel's steps by one wave per matrix on an LDS ring of
// column slots, the band streamed through it in chunks) for kl <= NAR_MAX_KL, kl + ku <= NAR_MAX_KV; the column kernel's bits.
//
// Real arithmetic (maus_band_set_real(ctx, 1), DESIGN §11 "Band solves in real arithmetic"): the build and scan kernels, the
// column kernel, the narrow method and the split are one text over the scalar T, c128 or double.  A maus_band_solve call runs
// on T = double when band_real_rule holds for it -- a real CSR matrix with an ordering, rhs_mode 1 with a real b, real shifts,
// and a plan whose every kernel is one of those -- in the same workspace used as doubles; the T-dependent operations are the
// overloads of common.h, each the complex operation without the terms that multiply an exact zero, so x, ipiv, info and status
// are the complex path's values.  Population rows as right-hand sides (eigenvalue problems) and the blocked, tiled and wide
// kernels have no real instantiation and run complex as ever.
#include "ctx.h"
#include <climits>
#include <type_traits>
#include <utility>

namespace {

// T: the scalar of the band storage and of the right-hand side, c128, or double on the real path (maus_band_set_real)
template <class T>
struct BandArgsT {
    T* ab; T* x; int* ipiv; int* info; int* flags;
    int n, kl, ku, ldab;
};
using BandArgs = BandArgsT<c128>;

template <class T>
__device__ __forceinline__ long bix(const BandArgsT<T>& a, int g) { return (long)g * a.ldab * a.n; }

// ---- pieces that several kernels share: each rule is stated here, once ----------------------------------------------------
// Pivot across the workgroup: from each thread's first maximum (best, bidx) the index of the first maximum of all, the lowest
// index among equals, INT_MAX where none is finite.  One barrier (LDS_ONLY: lds_barrier()); s_best / s_idx are free after the next.
template <int NW, bool LDS_ONLY>
__device__ __forceinline__ int block_argmax(double best, int bidx, double (&s_best)[NW], int (&s_idx)[NW], int lane, int wave) {
    wave_argmax(best, bidx);
    if (lane == 0) { s_best[wave] = best; s_idx[wave] = bidx; }
    if constexpr (LDS_ONLY) lds_barrier(); else __syncthreads();
    double m = s_best[0]; int p = s_idx[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
        if (s_best[w] > m) { m = s_best[w]; p = s_idx[w]; }
        else if (s_best[w] == m) p = min(p, s_idx[w]);
    }
    return p;
}

__device__ __forceinline__ double lane_bcast(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ c128 lane_bcast(c128 v, int l) { return cmake(lane_bcast(v.x, l), lane_bcast(v.y, l)); }

// A block row keeps 2 NB elements of a column: slots 0 .. NB - 1 its rows j0 .. j0 + NB - 1, slot NB + jj the pivot row of
// column jj where that row lies below the block's jb rows; pivot rows that coincide share the first such slot.  Thread
// tid < NB writes the pivot row s_pr[tid] (relative to j0) and the slot s_sl[tid] of column tid; ip: ipiv of column j0.
template <int NB>
__device__ __forceinline__ void pivot_slots(const int* ip, int j0, int jb, int tid, int (&s_pr)[NB], int (&s_sl)[NB]) {
    if (tid >= NB) return;
    int pr = tid, sl = tid;
    if (tid < jb) {
        pr = ip[tid] - 1 - j0;
        sl = pr;
        if (pr >= jb) {
            sl = NB + tid;
            for (int k = tid - 1; k >= 0; --k) if (ip[k] - 1 - j0 == pr) sl = NB + k;
        }
    }
    s_pr[tid] = pr; s_sl[tid] = sl;
}

// L11 of a block step out of lw into LDS: NB x NB, column-major, strictly lower, zero elsewhere and from row jb on
template <int NB, int NT>
__device__ __forceinline__ void load_l11(c128* s_l11, const c128* lw, int lh, int jb, int tid) {
    for (int e = tid; e < NB * NB; e += NT) {
        const int r = e % NB, k = e / NB;
        s_l11[e] = (k < r && r < jb) ? lw[r + (long)k * lh] : cmake(0.0, 0.0);
    }
}

// U12 = L11^-1 A12 on columns in LDS, row r of column q at s_v[q * ld + r], owned by thread (q, r): one barrier per column of L11
template <int NB>
__device__ __forceinline__ void solve_l11(c128* s_v, int ld, const c128* s_l11, int jb, int ncol, int q, int r) {
    for (int k = 0; k + 1 < jb; ++k) {
        if (q < ncol && r > k && r < jb) cfms(s_v[q * ld + r], s_l11[r + k * NB], s_v[q * ld + k]);
        __syncthreads();
    }
}

// H_k = A[perm][:, perm] - lam_k I + psi_k I into zeroed band storage, one thread per row of the permuted matrix; the
// diagonal is (a - lam) + psi in NumPy's rounding order, with a = 0 where A stores none (as build_h_csr_kernel).  The permuted
// right-hand side goes to x.  flags |= 1 on any non-finite value.  T = double: the real parts of the same complex operands (the
// rule of the real path has found every imaginary part +-0), the diagonal the real half of the complex one.
__device__ __forceinline__ c128 band_diag(c128 v, c128 lam, double ps) {
    return cmake(__dadd_rn(__dsub_rn(v.x, lam.x), ps), __dadd_rn(__dsub_rn(v.y, lam.y), 0.0));
}
__device__ __forceinline__ double band_diag(double v, double lam, double ps) { return __dadd_rn(__dsub_rn(v, lam), ps); }

template <class T>
__global__ void __launch_bounds__(256)
band_build_csr_kernel(BandArgsT<T> a, const int* __restrict__ Ap, const int* __restrict__ Ai, const c128* __restrict__ Av,
                      const int* __restrict__ perm, const int* __restrict__ iperm,
                      const c128* __restrict__ shift, const double* __restrict__ psi,
                      int rhs_mode, const c128* __restrict__ X, long ldx, const int* __restrict__ slots, const c128* __restrict__ bvec)
{
    const int i = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
    bool bad = false;
    if (i < a.n) {
        T* ab = a.ab + bix(a, g);
        const int kv = a.kl + a.ku;
        const T lam = cnarrow<T>(shift[g]);
        const double ps = psi[g];
        auto diag = [&](T v) { return band_diag(v, lam, ps); };
        T h = diag(czero<T>());
        bad |= !cfinite(h);
        ab[kv + (long)i * a.ldab] = h;
        const int r = perm[i];
        for (int p = Ap[r]; p < Ap[r + 1]; ++p) {
            const int j = iperm[Ai[p]];
            h = (j == i) ? diag(cnarrow<T>(Av[p])) : cnarrow<T>(Av[p]);
            bad |= !cfinite(h);
            ab[kv + i - j + (long)j * a.ldab] = h;
        }
        const T v = cnarrow<T>((rhs_mode == 0) ? X[(long)slots[g] * ldx + r] : bvec[r]);
        bad |= !cfinite(v);
        a.x[(long)g * a.n + i] = v;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&a.flags[g], 1);
}

// band matrices and right-hand sides handed in by the caller (maus_band_lu_host): the non-finite scan only
template <class T>
__global__ void __launch_bounds__(256)
band_scan_kernel(BandArgsT<T> a)
{
    const int g = blockIdx.y;
    const long per = (long)a.ldab * a.n;
    bool bad = false;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < per; e += (long)gridDim.x * 256) {
        // element (i, j) of the matrix sits at row r = kv + i - j of column j; the first kl rows are workspace and the corners
        // outside 0 <= i < n are never read (zgbtrf)
        const int r = (int)(e % a.ldab);
        const long j = e / a.ldab, i = r - (a.kl + a.ku) + j;
        if (r >= a.kl && i >= 0 && i < a.n) bad |= !cfinite(a.ab[bix(a, g) + e]);
    }
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long)gridDim.x * 256) bad |= !cfinite(a.x[(long)g * a.n + i]);
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&a.flags[g], 1);
}

// zgbtf2 on matrix blockIdx.x with the forward half of zgbtrs folded in (see the file comment).  Column j of a step is not
// written before every thread has read its pivot and its old top entry: the interchange inside column j is carried by the
// multipliers' source (the row that receives the old top entry) and by one store of the pivot at the end of the step.
template <class T, int NT>
__global__ void __launch_bounds__(NT)
band_factor_kernel(BandArgsT<T> a)
{
    constexpr int NW = NT / 64;
    __shared__ double s_best[NW];
    __shared__ int s_idx[NW];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n, kl = a.kl, ku = a.ku, kv = kl + ku, ldab = a.ldab;
    T* ab = a.ab + bix(a, g);
    T* x = a.x + (long)g * n;
    int* ipiv = a.ipiv + (long)g * n;
    auto at = [&](int r, int j) -> T& { return ab[r + (long)j * ldab]; };
    // rows handled together in the update (a power of two from 64 to NT, so that it divides NT) and the column groups that
    // share them
    int RW = 64;
    while (RW < kl && RW < NT) RW *= 2;
    const int CG = NT / RW;
    const int pr = tid % RW, cg = tid / RW;
    // the fill-in rows of columns ku + 1 .. min(kv, n) - 1 start at zero (zgbtf2)
    for (int j = ku + 1; j < min(kv, n); ++j)
        for (int r = kv - j + tid; r < kl; r += NT) at(r, j) = czero<T>();
    int ju = 0, info = 0;
    for (int j = 0; j < n; ++j) {
        if (j + kv < n) for (int r = tid; r < kl; r += NT) at(r, j + kv) = czero<T>();
        const int km = min(kl, n - 1 - j);
        double best = -1.0; int bidx = INT_MAX;
        for (int p = tid; p <= km; p += NT) {
            const double v = cabs1(at(kv + p, j));
            if (v > best) { best = v; bidx = p; }                                                  // NaN never wins (izamax)
        }
        int jp = block_argmax<NW, false>(best, bidx, s_best, s_idx, lane, wave);
        if (jp == INT_MAX) jp = 0;
        const T piv = at(kv + jp, j), top = at(kv, j);
        if (tid == 0) ipiv[j] = j + jp + 1;                             // LAPACK's 1-based row
        if (ciszero(piv)) {
            if (info == 0) info = j + 1;
            __syncthreads();                                             // s_best / s_idx are written again by the next column
            continue;
        }
        ju = max(ju, min(j + ku + jp, n - 1));
        if (jp != 0) {
            for (int c = j + 1 + tid; c <= ju; c += NT) {
                const T t = at(kv + jp + j - c, c);
                at(kv + jp + j - c, c) = at(kv + j - c, c);
                at(kv + j - c, c) = t;
            }
            if (tid == 0) { const T t = x[j + jp]; x[j + jp] = x[j]; x[j] = t; }
        }
        __syncthreads();
        if (km > 0) {
            const T r = crecip(piv);
            const T xj = x[j];
            if (cg == 0)
                for (int p = pr; p < km; p += RW) {
                    const T l = cmul(p + 1 == jp ? top : at(kv + 1 + p, j), r);
                    at(kv + 1 + p, j) = l;
                    cfms(x[j + 1 + p], l, xj);
                }
            __syncthreads();
            const int ncol = ju - j;
            for (int p = pr; p < km; p += RW) {
                const T l = at(kv + 1 + p, j);
                for (int c = 1 + cg; c <= ncol; c += CG) cfms(at(kv + 1 + p - c, j + c), l, at(kv - c, j + c));
            }
        }
        if (tid == 0 && jp != 0) at(kv, j) = piv;
        __syncthreads();
    }
    if (tid == 0) a.info[g] = info;
}

// U x = y (ztbsv, upper, non-unit, k = kl + ku) on matrix blockIdx.x; x[j] goes to out[perm[j]] (out[j] without perm) once it
// is final.  Every thread forms x[j] itself (the same division of the same operands), so one barrier per column suffices.
// flags |= 2 on a non-finite result.
template <class T, int NT>
__global__ void __launch_bounds__(NT)
band_back_kernel(BandArgsT<T> a, c128* __restrict__ out, long ldo, const int* __restrict__ slots, const int* __restrict__ perm)
{
    const int g = blockIdx.x, tid = threadIdx.x;
    const int n = a.n, kv = a.kl + a.ku, ldab = a.ldab;
    const T* ab = a.ab + bix(a, g);
    T* x = a.x + (long)g * n;
    c128* o = out + (slots ? (long)slots[g] : (long)g) * ldo;
    bool bad = false;
    for (int j = n - 1; j >= 0; --j) {
        T xj = x[j];
        if (!ciszero(xj)) {
            xj = cdiv(xj, ab[kv + (long)j * ldab]);
            for (int i = max(0, j - kv) + tid; i < j; i += NT) cfms(x[i], xj, ab[kv + i - j + (long)j * ldab]);
        }
        if (tid == 0) { o[perm ? perm[j] : j] = cwiden(xj); bad |= !cfinite(xj); }
        __syncthreads();
    }
    if (tid == 0 && bad) atomicOr(&a.flags[g], 2);
}

// ---- the blocked method (maus_band_set_method(ctx, 1)) ------------------------------------------------------
// zgbtrf's schedule, BNB columns at a time, every step a launch over (matrix, tile):
//   panel    one workgroup per matrix holds the (kl + BNB) x BNB slice in registers (thread-owned rows, the pivot row and the
//            row it displaces through LDS, two LDS barriers per column).  Interchanges are applied across the whole slice, as
//            zgbtrf does inside a block, so L comes out in the block's final row order; it goes to a dense work array
//            lw[matrix][(kl + BNB) x BNB] -- nothing reads L after its own block step, because the right-hand side is a
//            column of the update below -- and U11 goes back into the band.
//   update   one workgroup per BTC columns right of the panel, up to the reach ju of the pivot rows (zgbtrf's ju), plus one
//            for the right-hand side: the tile goes through LDS once -- the BNB interchanges, U12 = L11^-1 A12, then
//            A22 -= L21 U12 with the thread's row of L21 in registers -- and back.  Every element is owned by one thread and
//            its BNB multiply-subtracts run in column order: no sum has an order that the grid or the batch could change.
//   back     U x = y in blocks of BNB by one workgroup per matrix: the BNB x BNB triangle in LDS, then one pass over the
//            kl + ku rows above it.
// The block width and the workgroup sizes follow from (kl, ku) alone.
constexpr int BNB = 16;                                 // columns per block step ...
constexpr int BNB_TALL = 8;                             // ... and where kl + BNB rows no longer fit two per thread of the panel
constexpr int BTC = 4;                                  // columns per update tile
constexpr int BLK_MIN_KL = 16;                          // narrower bands run the column kernel ...
constexpr int BLK_MAX_KL = 1024;                        // ... and so do bands too tall for the one-workgroup panel

// lw: the L of a block step, column-major with leading dimension lh, matrix g at lw + g * ls (blocked and tiled: lh = kl + nb,
// ls = lh * nb); ju: reach so far
struct BlkArgs { c128* lw; int* ju; int lh; long ls; };

bool band_runs_blocked(int kl) { return kl >= BLK_MIN_KL && kl <= BLK_MAX_KL; }
int band_nb(int kl) { return kl + BNB <= 1024 ? BNB : BNB_TALL; }

// the fill-in rows of the band storage start at zero (zgbtf2 clears them column by column as it goes)
__global__ void __launch_bounds__(256)
band_zero_fill_kernel(BandArgs a)
{
    const int g = blockIdx.y;
    const long per = (long)a.kl * a.n;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < per; e += (long)gridDim.x * 256)
        a.ab[bix(a, g) + e % a.kl + e / a.kl * a.ldab] = cmake(0.0, 0.0);
}

// Panel of block step j0 on matrix blockIdx.x: columns j0 .. j0 + jb - 1, rows j0 .. j0 + H - 1.  Thread t owns the slice's
// rows t, t + NT, ... (RP of them) in registers; the loop over the columns is unrolled so that every register index is static.
// Pivot rule, ipiv and info as band_factor_kernel.
template <int... I, class F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl(std::make_integer_sequence<int, N>{}, f); }

template <int NT, int RP, int NB>
__global__ void __launch_bounds__(NT)
band_panel_kernel(BandArgs a, BlkArgs w, int j0)
{
    constexpr int NW = NT / 64;
    __shared__ double s_best[NW];
    __shared__ int s_idx[NW];
    __shared__ c128 s_piv[NB], s_top[NB];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n, kl = a.kl, ku = a.ku, kv = kl + ku, ldab = a.ldab;
    c128* ab = a.ab + bix(a, g);
    c128* lw = w.lw + (long)g * w.ls;
    int* ipiv = a.ipiv + (long)g * n;
    const int jb = min(NB, n - j0), H = min(kl + jb, n - j0);
    auto at = [&](int r, int j) -> c128& { return ab[r + (long)j * ldab]; };
    c128 row[RP][NB];
    static_for<RP>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        const int r = tid + m * NT;
        static_for<NB>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            row[m][k] = (r < H && k < jb && r - k <= kl && k - r <= kv) ? at(kv + r - k, j0 + k) : cmake(0.0, 0.0);
        });
    });
    int ju = w.ju[g], info = 0;
    static_for<NB>([&](auto jc) {
        constexpr int jj = decltype(jc)::value;
        if (jj < jb) {
            const int j = j0 + jj, km = min(kl, n - 1 - j);
            double best = -1.0; int bidx = INT_MAX;
            static_for<RP>([&](auto mc) {
                constexpr int m = decltype(mc)::value;
                const int r = tid + m * NT;
                if (r >= jj && r <= jj + km) {
                    const double v = cabs1(row[m][jj]);
                    if (v > best) { best = v; bidx = r; }                                          // NaN never wins (izamax)
                }
            });
            int pr = block_argmax<NW, true>(best, bidx, s_best, s_idx, lane, wave);
            if (pr == INT_MAX) pr = jj;
            static_for<RP>([&](auto mc) {
                constexpr int m = decltype(mc)::value;
                const int r = tid + m * NT;
                if (r == pr) static_for<NB>([&](auto kc) { s_piv[decltype(kc)::value] = row[m][decltype(kc)::value]; });
                if (r == jj && pr != jj) static_for<NB>([&](auto kc) { s_top[decltype(kc)::value] = row[m][decltype(kc)::value]; });
            });
            lds_barrier();
            const c128 piv = s_piv[jj];
            const bool zero = piv.x == 0.0 && piv.y == 0.0;
            if (zero && info == 0) info = j + 1;
            // row jj of the slice is final: columns < jj of it are L11 in the block's row order, the others U11.  On a zero
            // pivot nothing moves (zgbtf2), so the row that stays is the top one.
            if (tid < jb) {
                const c128 v = (zero && pr != jj) ? s_top[tid] : s_piv[tid];
                if (tid < jj) lw[jj + (long)tid * w.lh] = v;
                else if (tid - jj <= kv) at(kv + jj - tid, j0 + tid) = v;
            }
            if (tid == 0) ipiv[j] = j0 + pr + 1;                        // LAPACK's 1-based row
            if (!zero) {
                ju = max(ju, min(j + ku + pr - jj, n - 1));
                const c128 rc = crecip(piv);
                static_for<RP>([&](auto mc) {
                    constexpr int m = decltype(mc)::value;
                    const int r = tid + m * NT;
                    if (pr != jj && r == pr) static_for<NB>([&](auto kc) { row[m][decltype(kc)::value] = s_top[decltype(kc)::value]; });
                    if (r > jj && r <= jj + km) {
                        const c128 l = cmul(row[m][jj], rc);
                        row[m][jj] = l;
                        static_for<NB - 1 - jj>([&](auto kc) {
                            constexpr int k = jj + 1 + decltype(kc)::value;
                            cfms(row[m][k], l, s_piv[k]);
                        });
                    }
                });
            }
        }
    });
    // rows below the block: L21
    static_for<RP>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        const int r = tid + m * NT;
        if (r >= jb && r < H)
            static_for<NB>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                if (k < jb) lw[r + (long)k * w.lh] = row[m][k];
            });
    });
    if (tid == 0) {
        w.ju[g] = ju;
        if (info && a.info[g] == 0) a.info[g] = info;
    }
}

// Block row and trailing update of block step j0: workgroup (t, g) takes columns c0 .. c0 + BTC - 1 right of the panel of
// matrix g, workgroup (ntile, g) its right-hand side.  Rows above a column's first stored row (i < c - kv) are zero and stay
// zero (a pivot row never reaches them), so they are read as zero and not written.
template <int NB>
__global__ void __launch_bounds__(256)
band_update_kernel(BandArgs a, BlkArgs w, int j0, int ntile)
{
    constexpr int NT = 256;
    extern __shared__ c128 s_v[];                                       // [BTC][lh]
    __shared__ c128 s_l11[NB * NB];
    __shared__ int s_pr[NB];
    const int t = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
    const int n = a.n, kl = a.kl, kv = kl + a.ku, ldab = a.ldab, lh = w.lh;
    const int jb = min(NB, n - j0), H = min(kl + jb, n - j0);
    const bool rhs = t == ntile;
    const int c0 = j0 + jb + t * BTC;
    int ncol = 1;
    if (!rhs) {
        const int ju = w.ju[g];
        if (c0 > ju) return;
        ncol = min(BTC, ju - c0 + 1);
    }
    c128* ab = a.ab + bix(a, g);
    const c128* lw = w.lw + (long)g * w.ls;
    // element i of column q at col(q)[i], stored from row lo(q) on
    auto col = [&](int q) -> c128* { return rhs ? a.x + (long)g * n : ab + (long)(c0 + q) * ldab + kv - (c0 + q); };
    auto lo = [&](int q) { return rhs ? 0 : c0 + q - kv; };
    for (int q = 0; q < ncol; ++q) {
        c128* p = col(q);
        const int l0 = lo(q);
        for (int r = tid; r < H; r += NT) s_v[q * lh + r] = (j0 + r >= l0) ? p[j0 + r] : cmake(0.0, 0.0);
    }
    if (tid < NB) s_pr[tid] = tid < jb ? a.ipiv[(long)g * n + j0 + tid] - 1 - j0 : tid;
    load_l11<NB, NT>(s_l11, lw, lh, jb, tid);
    __syncthreads();
    if (tid < ncol)
        for (int jj = 0; jj < jb; ++jj) {
            const int pr = s_pr[jj];
            if (pr != jj) { const c128 u = s_v[tid * lh + jj]; s_v[tid * lh + jj] = s_v[tid * lh + pr]; s_v[tid * lh + pr] = u; }
        }
    __syncthreads();
    {
        const int q = tid / NB, r = tid % NB;
        solve_l11<NB>(s_v, lh, s_l11, jb, ncol, q, r);
        if (q < ncol && r < jb && j0 + r >= lo(q)) col(q)[j0 + r] = s_v[q * lh + r];
    }
    for (int r = jb + tid; r < H; r += NT) {                            // rows below the block: jb = NB here
        c128 l[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) l[k] = lw[r + (long)k * lh];
        for (int q = 0; q < ncol; ++q) {
            c128 acc = s_v[q * lh + r];
#pragma unroll
            for (int k = 0; k < NB; ++k) cfms(acc, l[k], s_v[q * lh + k]);
            if (j0 + r >= lo(q)) col(q)[j0 + r] = acc;
        }
    }
}

// U x = y in blocks of BNB on matrix blockIdx.x, with the operations of band_back_kernel in its order; x[j] goes to
// out[perm[j]].  flags |= 2 on a non-finite result.
template <int NT>
__global__ void __launch_bounds__(NT)
band_back_blk_kernel(BandArgs a, c128* __restrict__ out, long ldo, const int* __restrict__ slots, const int* __restrict__ perm)
{
    __shared__ c128 s_u[BNB * BNB], s_y[BNB], s_x[BNB];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int n = a.n, kv = a.kl + a.ku, ldab = a.ldab;
    const c128* ab = a.ab + bix(a, g);
    c128* x = a.x + (long)g * n;
    c128* o = out + (slots ? (long)slots[g] : (long)g) * ldo;
    bool bad = false;
    for (int j0 = (n - 1) / BNB * BNB; j0 >= 0; j0 -= BNB) {
        const int jb = min(BNB, n - j0);
        if (tid < BNB * BNB) {
            const int r = tid & (BNB - 1), k = tid / BNB;
            s_u[tid] = (r <= k && k < jb && k - r <= kv) ? ab[kv + r - k + (long)(j0 + k) * ldab] : cmake(0.0, 0.0);
        }
        if (tid < jb) s_y[tid] = x[j0 + tid];
        __syncthreads();
        for (int k = jb - 1; k >= 0; --k) {
            c128 xk = s_y[k];
            const bool nz = xk.x != 0.0 || xk.y != 0.0;
            if (nz) xk = cdiv(xk, s_u[k + k * BNB]);
            if (nz && tid < k) cfms(s_y[tid], xk, s_u[tid + k * BNB]);
            if (tid == k) s_x[k] = xk;
            lds_barrier();
        }
        if (tid < jb) { const c128 xk = s_x[tid]; o[perm ? perm[j0 + tid] : j0 + tid] = xk; bad |= !cfinite(xk); }
        for (int i = max(0, j0 - kv) + tid; i < j0; i += NT) {
            c128 acc = x[i];
            for (int k = jb - 1; k >= 0; --k) {
                const c128 xk = s_x[k];
                const int c = j0 + k;
                if ((xk.x != 0.0 || xk.y != 0.0) && i >= c - kv) cfms(acc, xk, ab[kv + i - c + (long)c * ldab]);
            }
            x[i] = acc;
        }
        __syncthreads();
    }
    if (bad) atomicOr(&a.flags[g], 2);
}

// The launch queue of a solve of many block steps is bounded as maus_herm_tridiag bounds it: an event every 64 steps, wait
// for the one before last.
struct StepThrottle {
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t err = hipSuccess;                                        // of creating the events
    StepThrottle() { for (auto& e : ev) if (err == hipSuccess) err = hipEventCreateWithFlags(&e, hipEventDisableTiming); }
    ~StepThrottle() { for (auto& e : ev) if (e) (void)hipEventDestroy(e); }
    StepThrottle(const StepThrottle&) = delete;
    StepThrottle& operator=(const StepThrottle&) = delete;
    hipError_t before_step(int step) { return step % 64 == 0 && step >= 128 ? hipEventSynchronize(ev[(step / 64) & 1]) : hipSuccess; }
    hipError_t after_step(int step, hipStream_t st) {
        if (step % 64 != 63) return hipSuccess;
        const hipError_t e = hipGetLastError();
        return e == hipSuccess ? hipEventRecord(ev[(step / 64) & 1], st) : e;
    }
};

// the back substitution of the blocked, tiled and wide methods
hipError_t launch_back_blk(const BandArgs& a, int G, hipStream_t st, c128* out, long ldo, const int* slots, const int* perm) {
    if (a.kl + a.ku <= 256) hipLaunchKernelGGL((band_back_blk_kernel<256>), dim3(G), dim3(256), 0, st, a, out, ldo, slots, perm);
    else hipLaunchKernelGGL((band_back_blk_kernel<1024>), dim3(G), dim3(1024), 0, st, a, out, ldo, slots, perm);
    return hipGetLastError();
}

// ---- the tiled method (maus_band_set_method(ctx, 2)) --------------------------------------------------------
// The blocked method's schedule, storage, panel, pivot rule, status contract and back substitution, with the update split so
// that nothing of height kl goes through LDS and the panel is the only kernel whose reach is bounded (kl <= TIL_MAX_KL):
//   panel      band_panel_kernel with up to 9 rows per thread; above kl = 1024 the block width shrinks with the height of the
//              slice (band_tiled_nb) so that every instantiation stays in registers.
//   block row  one workgroup per 256 / nb columns right of the panel (plus the right-hand side): the interchanges and
//              U12 = L11^-1 A12 on the 2 nb elements of a column that they touch -- its top nb rows and its pivot rows.
//   trailing   one workgroup per (TCT columns, TRT rows) of A22 (plus the right-hand side): a thread keeps its row of L21 in
//              registers, U12 of the tile sits in LDS, every element is read once and written once.
// Every element is owned by one thread in each launch and its nb multiply-subtracts run in column order on the values the
// blocked update uses, so for a band that both methods take the results are the same bits.
constexpr int TIL_MIN_KL = BLK_MIN_KL;
constexpr int TIL_MAX_KL = 4096;                        // the register panel ends at 4608 rows (512 threads x 9 rows, nb = 4)
constexpr int TIL_NB16_H = 1536;                        // above kl = 1024: nb = 16 while kl + 16 rows fit three per thread ...
constexpr int TNB_MID = 8;                              // ... 8 while kl + 8 <= 3072 (six per thread) ...
constexpr int TNB_TALL = 4;                             // ... and 4 up to TIL_MAX_KL
constexpr int TCT = 16;                                 // columns per tile of the trailing update
constexpr int TRT = 256;                                // rows per tile of the trailing update: one per thread

bool band_runs_tiled(int kl) { return kl >= TIL_MIN_KL && kl <= TIL_MAX_KL; }
// up to BLK_MAX_KL the blocked method's width, so that both methods do the same arithmetic there; above it the widest block
// whose panel stays in registers (measured: DESIGN §11)
int band_tiled_nb(int kl) {
    if (kl <= BLK_MAX_KL) return band_nb(kl);
    return kl + BNB <= TIL_NB16_H ? BNB : (kl + TNB_MID <= 3072 ? TNB_MID : TNB_TALL);
}

// the wide method (maus_band_set_method(ctx, 4), further down): an outer block of NBO columns over the tiled method's steps
#ifndef MAUS_BAND_NBO
#define MAUS_BAND_NBO 64                                // 32 was timed and rejected; 64 is one lane per top row
#endif
constexpr int NBO = MAUS_BAND_NBO;                      // columns per outer block
static_assert(NBO == 64 || NBO == 32, "the outer block row maps the top rows of a column to the lanes of one wave");
constexpr int WID_MIN_KL = 64;                          // below it the outer block is wider than the band's reach: tiled runs
constexpr int WID_MAX_KL = TIL_MAX_KL;

bool band_runs_wide(int kl) { return kl >= WID_MIN_KL && kl <= WID_MAX_KL; }

// the narrow method (maus_band_set_method(ctx, 8), further down): the widest band whose live columns fit its LDS ring
constexpr int NAR_MAX_KL = 15;
constexpr int NAR_MAX_KV = 31;

bool band_runs_narrow(int kl, int ku) { return kl <= NAR_MAX_KL && kl + ku <= NAR_MAX_KV; }

// What a (kl, ku) band runs under `method`; the values are those of maus_band_set_method and maus_band_kernel_for.
enum BandKind : int { BK_COLUMN = 0, BK_BLOCKED = 1, BK_TILED = 2, BK_WIDE = 4, BK_NARROW = 8 };

bool band_method_ok(int m) { return m == BK_COLUMN || m == BK_BLOCKED || m == BK_TILED || m == BK_WIDE || m == BK_NARROW; }

// Everything the host side derives from (method, kl, ku): the only reader of the ranges above and of the method.
struct BandPlan {
    BandKind kind = BK_COLUMN;
    int nb = 1;                                         // (inner) block width; 1 for the column kernel and for narrow
    int nbo = 0;                                        // outer block width: NBO where the band runs wide
    bool panel = false;                                 // lw and ju exist: blocked, tiled and wide; column and narrow share one workspace
    size_t lw_small = 0, lw_outer = 0, lw = 0;          // elements of lw per solve: the (kl + BNB) x BNB panel of L, the wide
                                                        // method's LW, their sum; lw of G solves holds the G panels, then the G LW
    int cls = KC_BAND;                                  // ProfScope class
};

// Under method 4 a band with TIL_MIN_KL <= kl < WID_MIN_KL runs exactly what the tiled method runs.
BandPlan band_plan(int method, int kl, int ku) {
    BandPlan p;
    switch (method) {
    case BK_BLOCKED: if (band_runs_blocked(kl)) p.kind = BK_BLOCKED; break;
    case BK_TILED: if (band_runs_tiled(kl)) p.kind = BK_TILED; break;
    case BK_WIDE: if (band_runs_wide(kl)) p.kind = BK_WIDE; else if (kl < WID_MIN_KL && band_runs_tiled(kl)) p.kind = BK_TILED; break;
    case BK_NARROW: if (band_runs_narrow(kl, ku)) p.kind = BK_NARROW; break;
    default: break;
    }
    switch (p.kind) {
    case BK_BLOCKED: p.nb = band_nb(kl); p.cls = KC_BAND_BLOCKED; break;
    case BK_TILED: p.nb = band_tiled_nb(kl); p.cls = KC_BAND_TILED; break;
    case BK_WIDE: p.nb = band_tiled_nb(kl); p.cls = KC_BAND_WIDE; p.nbo = NBO; p.lw_outer = (size_t)(kl + NBO) * NBO; break;
    default: return p;
    }
    p.panel = true;
    p.lw_small = (size_t)(kl + BNB) * BNB;
    p.lw = p.lw_small + p.lw_outer;
    return p;
}

// Block row of block step j0: workgroup (t, g) takes the 256 / NB columns from c0 right of the panel of matrix g, workgroup
// (ntile, g) its right-hand side.  A column keeps 2 NB elements in LDS, in the slots of pivot_slots.  Rows above a column's
// first stored row are read as zero and not written, as band_update_kernel.
template <int NB>
__global__ void __launch_bounds__(256)
band_row_kernel(BandArgs a, BlkArgs w, int j0, int ntile, int cap)
{
    constexpr int NT = 256, RC = NT / NB, SL = 2 * NB;
    __shared__ c128 s_v[RC * SL];
    __shared__ c128 s_l11[NB * NB];
    __shared__ int s_pr[NB], s_sl[NB];
    const int t = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
    const int n = a.n, kl = a.kl, kv = kl + a.ku, ldab = a.ldab, lh = w.lh;
    const int jb = min(NB, n - j0), H = min(kl + jb, n - j0);
    const bool rhs = t == ntile;
    const int c0 = j0 + jb + t * RC;
    int ncol = 1;
    if (!rhs) {
        const int ju = min(w.ju[g], cap);                            // cap: INT_MAX, or the last column of the wide method's outer block
        if (c0 > ju) return;
        ncol = min(RC, ju - c0 + 1);
    }
    c128* ab = a.ab + bix(a, g);
    const c128* lw = w.lw + (long)g * w.ls;
    auto col = [&](int q) -> c128* { return rhs ? a.x + (long)g * n : ab + (long)(c0 + q) * ldab + kv - (c0 + q); };
    auto lo = [&](int q) { return rhs ? 0 : c0 + q - kv; };
    pivot_slots<NB>(a.ipiv + (long)g * n + j0, j0, jb, tid, s_pr, s_sl);
    load_l11<NB, NT>(s_l11, lw, lh, jb, tid);
    __syncthreads();
    for (int e = tid; e < ncol * SL; e += NT) {
        const int q = e / SL, s = e % SL;
        const int r = s < NB ? s : s_pr[s - NB];
        const bool used = (s < NB ? s : s - NB) < jb && r < H;
        s_v[e] = (used && j0 + r >= lo(q)) ? col(q)[j0 + r] : cmake(0.0, 0.0);
    }
    __syncthreads();
    if (tid < ncol)
        for (int jj = 0; jj < jb; ++jj) {
            const int sl = s_sl[jj];
            if (sl != jj) { const c128 u = s_v[tid * SL + jj]; s_v[tid * SL + jj] = s_v[tid * SL + sl]; s_v[tid * SL + sl] = u; }
        }
    __syncthreads();
    const int q = tid / NB, r = tid % NB;
    solve_l11<NB>(s_v, SL, s_l11, jb, ncol, q, r);
    if (q < ncol && r < jb) {
        if (j0 + r >= lo(q)) col(q)[j0 + r] = s_v[q * SL + r];
        const int pr = s_pr[r];
        if (s_sl[r] == NB + r && pr < H && j0 + pr >= lo(q)) col(q)[j0 + pr] = s_v[q * SL + NB + r];
    }
}

// Trailing update of block step j0 (a full block: jb = NB): workgroup (ct * nrt + rt, g) takes rows NB + rt TRT .. of the
// slice in the TCT columns from c0 right of the panel of matrix g, column tile ct = nct its right-hand side.  Along a column
// the band storage is contiguous in the row, so the loads and stores of a wave coalesce.
template <int NB>
__global__ void __launch_bounds__(TRT)
band_trail_kernel(BandArgs a, BlkArgs w, int j0, int nct, int nrt, int cap)
{
    __shared__ c128 s_u[TCT * NB];
    const int ct = blockIdx.x / nrt, rt = blockIdx.x % nrt, g = blockIdx.y, tid = threadIdx.x;
    const int n = a.n, kl = a.kl, kv = kl + a.ku, ldab = a.ldab, lh = w.lh;
    const int H = min(kl + NB, n - j0);
    const bool rhs = ct == nct;
    const int c0 = j0 + NB + ct * TCT;
    int ncol = 1;
    if (!rhs) {
        const int ju = min(w.ju[g], cap);
        if (c0 > ju) return;
        ncol = min(TCT, ju - c0 + 1);
    }
    c128* ab = a.ab + bix(a, g);
    const c128* lw = w.lw + (long)g * w.ls;
    auto col = [&](int q) -> c128* { return rhs ? a.x + (long)g * n : ab + (long)(c0 + q) * ldab + kv - (c0 + q); };
    auto lo = [&](int q) { return rhs ? 0 : c0 + q - kv; };
    for (int e = tid; e < ncol * NB; e += TRT) {
        const int q = e / NB, k = e % NB;
        s_u[e] = (j0 + k >= lo(q)) ? col(q)[j0 + k] : cmake(0.0, 0.0);
    }
    __syncthreads();
    const int r = NB + rt * TRT + tid;
    if (r >= H) return;
    c128 l[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) l[k] = lw[r + (long)k * lh];
#pragma unroll 4
    for (int q = 0; q < ncol; ++q) {
        const bool in = j0 + r >= lo(q);
        c128* p = col(q) + j0 + r;
        c128 acc = in ? *p : cmake(0.0, 0.0);
#pragma unroll
        for (int k = 0; k < NB; ++k) cfms(acc, l[k], s_u[q * NB + k]);
        if (in) *p = acc;
    }
}

template <int NB>
void launch_tiled_panel(const BandArgs& a, const BlkArgs& w, int G, hipStream_t st, int j0) {
    const int H = a.kl + NB;
    if constexpr (NB == BNB) {                                          // kl <= 1008 (the blocked method's panels), 1025 <= kl <= 1520
        if (H <= 256) hipLaunchKernelGGL((band_panel_kernel<256, 1, NB>), dim3(G), dim3(256), 0, st, a, w, j0);
        else if (H <= 512) hipLaunchKernelGGL((band_panel_kernel<512, 1, NB>), dim3(G), dim3(512), 0, st, a, w, j0);
        else if (H <= 1024) hipLaunchKernelGGL((band_panel_kernel<512, 2, NB>), dim3(G), dim3(512), 0, st, a, w, j0);
        else hipLaunchKernelGGL((band_panel_kernel<512, 3, NB>), dim3(G), dim3(512), 0, st, a, w, j0);
    } else if constexpr (NB == TNB_MID) {                               // 1009 <= kl <= 1024, 1521 <= kl <= 3064
        if (H <= 1536) hipLaunchKernelGGL((band_panel_kernel<512, 3, NB>), dim3(G), dim3(512), 0, st, a, w, j0);
        else if (H <= 2048) hipLaunchKernelGGL((band_panel_kernel<512, 4, NB>), dim3(G), dim3(512), 0, st, a, w, j0);
        else if (H <= 2560) hipLaunchKernelGGL((band_panel_kernel<512, 5, NB>), dim3(G), dim3(512), 0, st, a, w, j0);
        else hipLaunchKernelGGL((band_panel_kernel<512, 6, NB>), dim3(G), dim3(512), 0, st, a, w, j0);
    } else {                                                            // 3065 <= kl <= 4096
        if (H <= 4096) hipLaunchKernelGGL((band_panel_kernel<512, 8, NB>), dim3(G), dim3(512), 0, st, a, w, j0);
        else hipLaunchKernelGGL((band_panel_kernel<512, 9, NB>), dim3(G), dim3(512), 0, st, a, w, j0);
    }
}

// ---- the wide method (maus_band_set_method(ctx, 4)) ---------------------------------------------------------
// zgbtrf's two levels: an outer block of NBO columns is factored by the tiled method's steps of nb = band_tiled_nb columns,
// their block row and trailing update stopping at the outer block's last column (`cap`); the right-hand side goes with the
// inner steps as it does in the tiled method.  The L of the whole outer block is kept in LW[matrix][(kl + NBO) x NBO],
// column-major, in the block's final row order: the inner panels write their L straight into it (BlkArgs::lw offset by the
// step's place in the block) and the interchanges of a step are applied to the LW columns left of it (band_lw_swap_kernel,
// which also clears the few rows of the step's own columns that the panel does not reach).
// Then two launches take everything right of the block up to the reach ju:
//   outer row       one workgroup per ORC columns: the NBO interchanges in order and U12 = L11^-1 A12 on the 2 NBO elements
//                   of a column that they touch; a wave owns whole columns, a lane one of the NBO top rows, and row k reaches
//                   the others through v_readlane -- no barrier inside the solve.
//   outer trailing  A22 -= L21 U12 with K = NBO on v_mfma_f64_16x16x4_f64, one workgroup per (OCT columns, ORT rows), a wave
//                   32 rows x OCT columns.  In (row, column) coordinates the band storage is column-major with leading
//                   dimension ldab - 1, so the product is formed transposed -- U12^T as the MFMA's A operand out of LDS,
//                   L21^T as its B operand straight from LW -- and a result register holds 16 consecutive rows of one
//                   column.  4M: Cre += Ure (-Lre) + Uim Lim, Cim += Uim (-Lre) + Ure (-Lim), the accumulators start from
//                   A22 and k ascends; every element is owned by one wave and summed in that one order, whatever the grid,
//                   the batch or the chunk.
// A last block with fewer than NBO columns or no rows below it runs the tiled steps alone.
constexpr int ORC = 8;                                  // columns per workgroup of the outer block row: two per wave
constexpr int OCT = 32;                                 // columns ...
constexpr int ORT = 128;                                // ... and rows per workgroup of the outer trailing update

// After the panel of inner step d (columns J0 + d ..): its nb interchanges on the columns of LW left of it, one thread per
// column, and zeros in the rows of its own columns below the panel's slice (d + hin .. lh - 1, at most NBO - nb of them) --
// what the panel left there belongs to the outer block before, and the outer update and later interchanges read those rows.
// Everything else below the diagonal of LW is written by the panels, and nothing on or above it is ever read.
__global__ void __launch_bounds__(64)
band_lw_swap_kernel(BandArgs a, BlkArgs w, int J0, int d, int nb, int hin)
{
    const int g = blockIdx.x, k = threadIdx.x;
    c128* lw = w.lw + (long)g * w.ls;
    const int tail = w.lh - d - hin;
    for (int e = k; e < tail * nb; e += 64) lw[d + hin + e % tail + (long)(d + e / tail) * w.lh] = cmake(0.0, 0.0);
    if (k >= d) return;
    lw += (long)k * w.lh;
    const int* ip = a.ipiv + (long)g * a.n + J0 + d;
    for (int jj = 0; jj < nb; ++jj) {
        const int pr = ip[jj] - 1 - J0;
        if (pr != d + jj) { const c128 t = lw[d + jj]; lw[d + jj] = lw[pr]; lw[pr] = t; }
    }
}

// Outer block row of the block at J0 (a full one: NBO columns, rows below): workgroup (t, g) takes the ORC columns from c0
// right of the block of matrix g.  The slots of pivot_slots with jb = NB = NBO.  Rows above a column's first stored row are
// read as zero and not written.
__global__ void __launch_bounds__(256)
band_orow_kernel(BandArgs a, BlkArgs w, int J0)
{
    constexpr int SL = 2 * NBO;
    extern __shared__ c128 s_dyn[];
    c128* s_l11 = s_dyn;                                                // [NBO][NBO], column-major, strictly lower
    c128* s_v = s_dyn + NBO * NBO;                                      // [SL][ORC]
    __shared__ int s_pr[NBO], s_sl[NBO];
    const int t = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
    const int n = a.n, kl = a.kl, kv = kl + a.ku, ldab = a.ldab, lh = w.lh;
    const int H = min(kl + NBO, n - J0);
    const int c0 = J0 + NBO + t * ORC, ju = w.ju[g];
    if (c0 > ju) return;
    const int ncol = min(ORC, ju - c0 + 1);
    c128* ab = a.ab + bix(a, g);
    const c128* lw = w.lw + (long)g * w.ls;
    auto col = [&](int q) -> c128* { return ab + (long)(c0 + q) * ldab + kv - (c0 + q); };
    auto lo = [&](int q) { return c0 + q - kv; };
    pivot_slots<NBO>(a.ipiv + (long)g * n + J0, J0, NBO, tid, s_pr, s_sl);
    load_l11<NBO, 256>(s_l11, lw, lh, NBO, tid);
    __syncthreads();
    for (int e = tid; e < SL * ORC; e += 256) {
        const int q = e / SL, s = e % SL;
        const int r = s < NBO ? s : s_pr[s - NBO];
        s_v[s * ORC + q] = (q < ncol && r < H && J0 + r >= lo(q)) ? col(q)[J0 + r] : cmake(0.0, 0.0);
    }
    __syncthreads();
    if (tid < ncol)
        for (int jj = 0; jj < NBO; ++jj) {
            const int sl = s_sl[jj];
            if (sl != jj) { const c128 u = s_v[jj * ORC + tid]; s_v[jj * ORC + tid] = s_v[sl * ORC + tid]; s_v[sl * ORC + tid] = u; }
        }
    __syncthreads();
    // wave `wv` owns columns wv and wv + 4, lane r < NBO their row J0 + r
    const int r = tid & 63, wv = tid >> 6;
    const bool mine = r < NBO;
    c128 v0 = s_v[(mine ? r : 0) * ORC + wv], v1 = s_v[(mine ? r : 0) * ORC + wv + 4];
    for (int k = 0; k + 1 < NBO; ++k) {
        const c128 l = s_l11[(mine ? r : 0) + k * NBO];                 // zero for r <= k
        const c128 u0 = lane_bcast(v0, k), u1 = lane_bcast(v1, k);
        if (mine && r > k) { cfms(v0, l, u0); cfms(v1, l, u1); }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int q = wv + 4 * h;
        if (mine && q < ncol) {
            if (J0 + r >= lo(q)) col(q)[J0 + r] = h ? v1 : v0;
            const int pr = s_pr[r];
            if (s_sl[r] == NBO + r && pr < H && J0 + pr >= lo(q)) col(q)[J0 + pr] = s_v[(NBO + r) * ORC + q];
        }
    }
}

// Outer trailing update of the block at J0: workgroup (ct * nrt + rt, g) takes rows NBO + rt ORT .. of the slice in the OCT
// columns from c0 right of the block of matrix g; wave v its rows 32 v .. 32 v + 31 as 2 x 2 blocks of 16 x 16.  Lane maps of
// the MFMA as in csrc/zgemm.hip, with rows and columns exchanged: a = U12[k = 4 s + lane / 16][column lane % 16],
// b = L21[row lane % 16][k = 4 s + lane / 16], d[i] = C[row lane % 16][column lane / 16 + 4 i].  The whole rectangle is
// stored (c <= ju <= J0 + NBO - 1 + kv, r >= J0 + NBO), so only the edges at H and ju are masked: loads are clamped into the
// rectangle and feed elements that are not stored.
__global__ void __launch_bounds__(256)
band_otrail_kernel(BandArgs a, BlkArgs w, int J0, int nrt)
{
    __shared__ c128 s_u[NBO * OCT];                                     // [k][column ^ (k & 7)]: fragment reads and the transposing store conflict-free
    const int ct = blockIdx.x / nrt, rt = blockIdx.x % nrt, g = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = a.n, kl = a.kl, kv = kl + a.ku, lh = w.lh;
    const long ldc = a.ldab - 1;
    const int H = min(kl + NBO, n - J0);
    const int c0 = J0 + NBO + ct * OCT, ju = w.ju[g];
    if (c0 > ju) return;
    const int ncol = min(OCT, ju - c0 + 1);
    c128* cm = a.ab + bix(a, g) + kv;                                   // element (i, c) at cm[i + c * ldc]
    const c128* lw = w.lw + (long)g * w.ls;
    for (int e = tid; e < NBO * OCT; e += 256) {
        const int k = e % NBO, q = e / NBO;
        s_u[k * OCT + (q ^ (k & 7))] = (q < ncol && J0 + k >= c0 + q - kv) ? cm[J0 + k + (long)(c0 + q) * ldc] : cmake(0.0, 0.0);
    }
    __syncthreads();
    const int r0 = NBO + rt * ORT + wv * 32;
    if (r0 >= H) return;
    const int lr = lane & 15, lk = lane >> 4;
    int rr[2]; bool rok[2];
    d4 cre[2][2], cim[2][2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const int r = r0 + rb * 16 + lr;
        rok[rb] = r < H; rr[rb] = min(r, H - 1);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int q = min(cb * 16 + lk + 4 * i, ncol - 1);
                const c128 c = cm[J0 + rr[rb] + (long)(c0 + q) * ldc];
                cre[rb][cb][i] = c.x; cim[rb][cb][i] = c.y;
            }
    }
#pragma unroll 4
    for (int s = 0; s < NBO / 4; ++s) {
        const int k = 4 * s + lk;
        c128 l[2], u[2];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) l[rb] = lw[rr[rb] + (long)k * lh];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) u[cb] = s_u[k * OCT + ((cb * 16 + lr) ^ (k & 7))];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                cre[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(u[cb].x, -l[rb].x, cre[rb][cb], 0, 0, 0);
                cre[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(u[cb].y, l[rb].y, cre[rb][cb], 0, 0, 0);
                cim[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(u[cb].y, -l[rb].x, cim[rb][cb], 0, 0, 0);
                cim[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(u[cb].x, -l[rb].y, cim[rb][cb], 0, 0, 0);
            }
    }
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int q = cb * 16 + lk + 4 * i;
                if (rok[rb] && q < ncol) cm[J0 + rr[rb] + (long)(c0 + q) * ldc] = cmake(cre[rb][cb][i], cim[rb][cb][i]);
            }
}

// The whole blocked solve of G matrices on `st`: n / NB block steps of two launches each, then the back substitution.
template <int NB>
hipError_t launch_blocked_nb(const BandArgs& a, const BlkArgs& w, int G, hipStream_t st, c128* out, long ldo, const int* slots, const int* perm) {
    const int kv = a.kl + a.ku, H = a.kl + NB, ntile = (kv + BTC - 1) / BTC;
    const size_t lds = sizeof(c128) * (size_t)w.lh * BTC;
    // every call, for the device the call runs on: cheap beside the solve, and a refusal ends the solve here
    hipError_t err = hipFuncSetAttribute((const void*)band_update_kernel<NB>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    if (err == hipSuccess) err = hipMemsetAsync(w.ju, 0, sizeof(int) * G, st);
    StepThrottle th;
    if (err == hipSuccess) err = th.err;
    int step = 0;
    for (int j0 = 0; j0 < a.n && err == hipSuccess; j0 += NB, ++step) {
        if ((err = th.before_step(step)) != hipSuccess) break;
        if (H <= 256) hipLaunchKernelGGL((band_panel_kernel<256, 1, NB>), dim3(G), dim3(256), 0, st, a, w, j0);
        else if (H <= 512) hipLaunchKernelGGL((band_panel_kernel<512, 1, NB>), dim3(G), dim3(512), 0, st, a, w, j0);
        else if (H <= 1024) hipLaunchKernelGGL((band_panel_kernel<512, 2, NB>), dim3(G), dim3(512), 0, st, a, w, j0);
        else hipLaunchKernelGGL((band_panel_kernel<512, 3, NB>), dim3(G), dim3(512), 0, st, a, w, j0);
        hipLaunchKernelGGL(band_update_kernel<NB>, dim3(ntile + 1, G), dim3(256), lds, st, a, w, j0, ntile);
        err = th.after_step(step, st);
    }
    return err == hipSuccess ? launch_back_blk(a, G, st, out, ldo, slots, perm) : err;
}

// The whole tiled (lwo == nullptr) or wide solve of G matrices on `st`.  w.lw is the tiled method's panel of L (wide: short
// last blocks), lwo the LW of the outer blocks.  Per inner step three launches (the trailing update only where rows lie below
// the block), wide: plus the interchanges on LW; per outer block the two outer launches; then the blocked back substitution.
// Without lwo no block is `full`: every step runs uncapped over the whole reach kv, and since NBO is a multiple of every NB the
// steps j0 are 0, NB, 2 NB, ... -- the tiled method is the wide method without an outer block.
template <int NB>
hipError_t launch_tiled_nb(const BandArgs& a, const BlkArgs& w, c128* lwo, int G, hipStream_t st, c128* out, long ldo, const int* slots, const int* perm) {
    static_assert(NBO % NB == 0, "the inner steps tile an outer block");
    constexpr size_t orow_lds = sizeof(c128) * (NBO * NBO + 2 * NBO * ORC);
    const int kv = a.kl + a.ku, RC = 256 / NB, LH = a.kl + NBO;
    const long LS = (long)LH * NBO;
    // every call, for the device the call runs on: cheap beside the solve, and a refusal ends the solve here
    hipError_t err = lwo ? hipFuncSetAttribute((const void*)band_orow_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)orow_lds) : hipSuccess;
    if (err == hipSuccess) err = hipMemsetAsync(w.ju, 0, sizeof(int) * G, st);
    StepThrottle th;
    if (err == hipSuccess) err = th.err;
    int step = 0;
    for (int J0 = 0; J0 < a.n && err == hipSuccess; J0 += NBO) {
        const int HO = std::min(a.kl + NBO, a.n - J0);
        const bool full = lwo && a.n - J0 >= NBO && HO > NBO;
        for (int j0 = J0; j0 < std::min(J0 + NBO, a.n) && err == hipSuccess; j0 += NB, ++step) {
            if ((err = th.before_step(step)) != hipSuccess) break;
            const int d = j0 - J0;
            BlkArgs wi = w;
            if (full) { wi.lw = lwo + d + (long)d * LH; wi.lh = LH; wi.ls = LS; }
            const int cap = full ? J0 + NBO - 1 : INT_MAX;
            const int right = full ? NBO - d - NB : kv;                 // columns right of the panel that the step may reach
            const int ntile = (right + RC - 1) / RC, nct = (right + TCT - 1) / TCT;
            launch_tiled_panel<NB>(a, wi, G, st, j0);
            if (full) {
                BlkArgs wo = wi; wo.lw = lwo;
                hipLaunchKernelGGL(band_lw_swap_kernel, dim3(G), dim3(64), 0, st, a, wo, J0, d, NB, std::min(a.kl + NB, a.n - j0));
            }
            hipLaunchKernelGGL(band_row_kernel<NB>, dim3(ntile + 1, G), dim3(256), 0, st, a, wi, j0, ntile, cap);
            const int below = std::min(a.kl + NB, a.n - j0) - NB;           // rows of L21; none in a last, short block
            if (below > 0) {
                const int nrt = (below + TRT - 1) / TRT;
                hipLaunchKernelGGL(band_trail_kernel<NB>, dim3((nct + 1) * nrt, G), dim3(TRT), 0, st, a, wi, j0, nct, nrt, cap);
            }
            err = th.after_step(step, st);
        }
        if (full && err == hipSuccess) {
            BlkArgs wo = w; wo.lw = lwo; wo.lh = LH; wo.ls = LS;
            const int nrt = (HO - NBO + ORT - 1) / ORT;
            hipLaunchKernelGGL(band_orow_kernel, dim3((kv + ORC - 1) / ORC, G), dim3(256), orow_lds, st, a, wo, J0);
            hipLaunchKernelGGL(band_otrail_kernel, dim3((kv + OCT - 1) / OCT * nrt, G), dim3(256), 0, st, a, wo, J0, nrt);
        }
    }
    if (err == hipSuccess) err = hipGetLastError();
    return err == hipSuccess ? launch_back_blk(a, G, st, out, ldo, slots, perm) : err;
}

// ---- the narrow method (maus_band_set_method(ctx, 8)) -------------------------------------------------------
// The column kernel's steps on a band that never leaves the chip while it is live.  One wave per matrix; the columns a step
// can touch (j .. j + kv, kv <= NAR_MAX_KV) sit in an LDS ring of NAR_SLOTS column slots of NAR_LD rows, column c in slot
// c % NAR_SLOTS, the right-hand side beside them.  In zgbtf2 an interchange goes to the right only, so column j is final after
// step j: a column enters the ring once and leaves once, NAR_CH columns (one chunk, contiguous in band storage) at a time.
// At the top of the chunk of steps j0 .. j0 + 15:
//     enter   columns j0 + 32 .. j0 + 47 from the registers they were loaded into one chunk earlier (their fill rows zeroed,
//             as zgbtf2 zeroes them before a pivot row can reach them); columns j0 .. j0 + 47 are then resident, and the last
//             step of the chunk reaches column j0 + 15 + kv <= j0 + 46,
//     leave   columns j0 - 16 .. j0 - 1, x and ipiv with them, by coalesced stores,
//     load    columns j0 + 48 .. j0 + 63 into registers: in flight for the 16 steps of the chunk.
// A step is band_factor_kernel's, operation for operation: every element is changed by the same fused operation on the same
// operands and the pivot search is the same exact maximum, so x, ipiv, info and flags are the column kernel's bits.  Only who
// does what differs: the candidates of column j sit one per lane, so the pivot and the old top entry come by v_readlane; every
// lane of a row forms the row's multiplier itself (the same operation on the same operands) instead of reading it back; and
// the km x (ju - j) update is spread over all 64 lanes, RW (the power of two >= kl) rows by 64 / RW columns at a time.
// All barriers are lds_barrier(): the wave is alone in its workgroup and must not wait for its loads in flight.
constexpr int NAR_CH = 16;                              // columns per chunk
constexpr int NAR_SLOTS = 64;                           // column slots of the ring: four chunks
constexpr int NAR_LD = 48;                              // rows of a slot, >= ldab = 2 kl + ku + 1 <= 47
constexpr int NAR_EL = NAR_CH * NAR_LD / 64;            // elements of a chunk per lane
static_assert(NAR_CH + NAR_MAX_KV <= 3 * NAR_CH, "the last step of a chunk must stay inside the three resident chunks");
static_assert(2 * NAR_MAX_KL + (NAR_MAX_KV - NAR_MAX_KL) + 1 <= NAR_LD && NAR_MAX_KL + 1 <= 64, "slot height, one candidate per lane");

// Where element lane + 64 k of a chunk (16 columns of ldab rows, contiguous) sits relative to the chunk's first slot, or -1
// past the chunk's end.  Chunks start at multiples of 16 columns, so the map is the same for every chunk.
__device__ __forceinline__ void nar_chunk_map(int (&loff)[NAR_EL], int lane, int ldab) {
#pragma unroll
    for (int k = 0; k < NAR_EL; ++k) {
        const int e = lane + 64 * k;
        loff[k] = e < NAR_CH * ldab ? e / ldab * NAR_LD + e % ldab : -1;
    }
}

template <class T, int RW>
__global__ void __launch_bounds__(64)
band_narrow_factor_kernel(BandArgsT<T> a)
{
    constexpr int CG = 64 / RW;
    __shared__ T s_ab[NAR_SLOTS * NAR_LD];
    __shared__ T s_x[NAR_SLOTS];
    const int g = blockIdx.x, lane = threadIdx.x;
    const int n = a.n, kl = a.kl, ku = a.ku, kv = kl + ku, ldab = a.ldab;
    T* ab = a.ab + bix(a, g);
    T* x = a.x + (long)g * n;
    int* ipiv = a.ipiv + (long)g * n;
    const long end = (long)ldab * n;
    int loff[NAR_EL];
    nar_chunk_map(loff, lane, ldab);
    auto S = [&](int r, int c) -> T& { return s_ab[(c & (NAR_SLOTS - 1)) * NAR_LD + r]; };
    // columns c0 .. c0 + 15 and their x (c0 a multiple of 16; nothing is read at or past column n)
    auto load = [&](int c0, T (&v)[NAR_EL], T& vx) {
        const long e0 = (long)c0 * ldab + lane;
#pragma unroll
        for (int k = 0; k < NAR_EL; ++k) v[k] = (loff[k] >= 0 && e0 + 64 * k < end) ? ab[e0 + 64 * k] : czero<T>();
        vx = (lane < NAR_CH && c0 + lane < n) ? x[c0 + lane] : czero<T>();
    };
    // the fill-in rows of column c, kv - c <= r < kl, start at zero (zgbtf2: columns ku + 1 .. kv - 1 before the first step,
    // column j + kv at step j -- in both cases before a pivot row reaches the column)
    auto enter = [&](int c0, const T (&v)[NAR_EL], const T& vx) {
        const int s0 = (c0 & (NAR_SLOTS - 1)) * NAR_LD;
#pragma unroll
        for (int k = 0; k < NAR_EL; ++k)
            if (loff[k] >= 0) {
                const int r = loff[k] % NAR_LD, c = c0 + loff[k] / NAR_LD;
                s_ab[s0 + loff[k]] = (r < kl && r + c >= kv) ? czero<T>() : v[k];
            }
        if (lane < NAR_CH) s_x[(c0 & (NAR_SLOTS - 1)) + lane] = vx;
    };
    auto leave = [&](int c0, int pv) {
        const int s0 = (c0 & (NAR_SLOTS - 1)) * NAR_LD;
        const long e0 = (long)c0 * ldab + lane;
#pragma unroll
        for (int k = 0; k < NAR_EL; ++k)
            if (loff[k] >= 0 && e0 + 64 * k < end) ab[e0 + 64 * k] = s_ab[s0 + loff[k]];
        if (lane < NAR_CH && c0 + lane < n) { x[c0 + lane] = s_x[(c0 & (NAR_SLOTS - 1)) + lane]; ipiv[c0 + lane] = pv; }
    };
    T pre[NAR_EL], prex;
    load(0, pre, prex); enter(0, pre, prex);
    load(NAR_CH, pre, prex); enter(NAR_CH, pre, prex);
    load(2 * NAR_CH, pre, prex);
    int ju = 0, info = 0, pv = 0;                                       // pv: ipiv of column j0 + lane of the chunk
    for (int j0 = 0; j0 < n; j0 += NAR_CH) {
        enter(j0 + 2 * NAR_CH, pre, prex);
        if (j0 > 0) leave(j0 - NAR_CH, pv);
        load(j0 + 3 * NAR_CH, pre, prex);
        lds_barrier();
        const int je = min(j0 + NAR_CH, n);
        for (int j = j0; j < je; ++j) {
            const int km = min(kl, n - 1 - j);
            const T cand = lane <= km ? S(kv + lane, j) : czero<T>();
            double best = -1.0; int bidx = INT_MAX;
            if (lane <= km) {
                const double v = cabs1(cand);
                if (v > best) { best = v; bidx = lane; }                                           // NaN never wins (izamax)
            }
            wave_argmax(best, bidx);
            int jp = __builtin_amdgcn_readfirstlane(bidx);
            if (jp == INT_MAX) jp = 0;
            const T piv = lane_bcast(cand, jp), top = lane_bcast(cand, 0);
            if (lane == (j & (NAR_CH - 1))) pv = j + jp + 1;            // LAPACK's 1-based row
            if (ciszero(piv)) {
                if (info == 0) info = j + 1;
                continue;
            }
            ju = max(ju, min(j + ku + jp, n - 1));
            if (jp != 0) {
                const int c = j + 1 + lane;
                if (c <= ju) {
                    const T t = S(kv + jp + j - c, c);
                    S(kv + jp + j - c, c) = S(kv + j - c, c);
                    S(kv + j - c, c) = t;
                }
                if (lane == 0) {
                    T& xa = s_x[(j + jp) & (NAR_SLOTS - 1)];
                    T& xb = s_x[j & (NAR_SLOTS - 1)];
                    const T t = xa; xa = xb; xb = t;
                }
                lds_barrier();
            }
            if (km > 0) {
                const T r = crecip(piv);
                const T xj = s_x[j & (NAR_SLOTS - 1)];
                const int p = lane % RW, cg = lane / RW;
                if (p < km) {
                    const T own = S(kv + 1 + p, j);
                    const T l = cmul(p + 1 == jp ? top : own, r);
                    if (cg == 0) {
                        S(kv + 1 + p, j) = l;
                        cfms(s_x[(j + 1 + p) & (NAR_SLOTS - 1)], l, xj);
                    }
                    const int ncol = ju - j;
                    for (int c = 1 + cg; c <= ncol; c += CG) cfms(S(kv + 1 + p - c, j + c), l, S(kv - c, j + c));
                }
            }
            if (lane == 0 && jp != 0) S(kv, j) = piv;
            lds_barrier();
        }
    }
    leave((n - 1) / NAR_CH * NAR_CH, pv);
    if (lane == 0) a.info[g] = info;
}

// U x = y on matrix blockIdx.x by one wave, band_back_kernel's operations in its order, walking the chunks downwards.  The
// columns of the chunk at hand sit in LDS, the chunk below it is in flight in registers; x lives in a ring of NAR_SLOTS
// entries (a step reaches kv entries up, so the chunk at hand and the two below it are resident, the third below in flight).
// x[j] goes to out[perm[j]] a chunk at a time; flags |= 2 on a non-finite result.
template <class T>
__global__ void __launch_bounds__(64)
band_narrow_back_kernel(BandArgsT<T> a, c128* __restrict__ out, long ldo, const int* __restrict__ slots, const int* __restrict__ perm)
{
    __shared__ T s_u[NAR_CH * NAR_LD];
    __shared__ T s_x[NAR_SLOTS];
    const int g = blockIdx.x, lane = threadIdx.x;
    const int n = a.n, kv = a.kl + a.ku, ldab = a.ldab;
    const T* ab = a.ab + bix(a, g);
    const T* x = a.x + (long)g * n;
    c128* o = out + (slots ? (long)slots[g] : (long)g) * ldo;
    const long end = (long)ldab * n;
    int loff[NAR_EL];
    nar_chunk_map(loff, lane, ldab);
    // chunk k of the band (columns 16 k ..) and chunk k - 2 of x; nothing is read below index 0 or at or past n
    auto load = [&](int k, T (&v)[NAR_EL], T& vx) {
        const long e0 = (long)k * NAR_CH * ldab + lane;
#pragma unroll
        for (int q = 0; q < NAR_EL; ++q) v[q] = (k >= 0 && loff[q] >= 0 && e0 + 64 * q < end) ? ab[e0 + 64 * q] : czero<T>();
        const int i = (k - 2) * NAR_CH + lane;
        vx = (lane < NAR_CH && i >= 0 && i < n) ? x[i] : czero<T>();
    };
    auto enter = [&](int k, const T (&v)[NAR_EL], const T& vx) {
#pragma unroll
        for (int q = 0; q < NAR_EL; ++q) if (loff[q] >= 0) s_u[loff[q]] = v[q];
        if (lane < NAR_CH && k >= 2) s_x[((k - 2) * NAR_CH + lane) & (NAR_SLOTS - 1)] = vx;
    };
    const int K = (n - 1) / NAR_CH;
    {
        const int i = (K - 1) * NAR_CH + lane;                          // x of the last two chunks
        if (lane < 2 * NAR_CH && i >= 0 && i < n) s_x[i & (NAR_SLOTS - 1)] = x[i];
    }
    T pre[NAR_EL], prex;
    load(K, pre, prex);
    bool bad = false;
    for (int k = K; k >= 0; --k) {
        enter(k, pre, prex);
        load(k - 1, pre, prex);
        const int jo = k * NAR_CH + lane;                               // the entry of x this lane writes out
        const int po = (lane < NAR_CH && jo < n) ? (perm ? perm[jo] : jo) : 0;
        T xo = czero<T>();
        lds_barrier();
        for (int j = min(k * NAR_CH + NAR_CH, n) - 1; j >= k * NAR_CH; --j) {
            const T* u = s_u + (j & (NAR_CH - 1)) * NAR_LD + kv;        // the diagonal entry of column j
            T xj = s_x[j & (NAR_SLOTS - 1)];
            if (!ciszero(xj)) {
                xj = cdiv(xj, u[0]);
                const int i = j - 1 - lane;
                if (lane < kv && i >= 0) cfms(s_x[i & (NAR_SLOTS - 1)], xj, u[i - j]);
            }
            if (lane == (j & (NAR_CH - 1))) xo = xj;
            lds_barrier();
        }
        if (lane < NAR_CH && jo < n) { o[po] = cwiden(xo); bad |= !cfinite(xo); }
    }
    if (__any(bad) && lane == 0) atomicOr(&a.flags[g], 2);
}

template <class T>
void launch_narrow(const BandArgsT<T>& a, int G, hipStream_t st, c128* out, long ldo, const int* slots, const int* perm) {
    if (a.kl <= 1) hipLaunchKernelGGL((band_narrow_factor_kernel<T, 1>), dim3(G), dim3(64), 0, st, a);
    else if (a.kl <= 2) hipLaunchKernelGGL((band_narrow_factor_kernel<T, 2>), dim3(G), dim3(64), 0, st, a);
    else if (a.kl <= 4) hipLaunchKernelGGL((band_narrow_factor_kernel<T, 4>), dim3(G), dim3(64), 0, st, a);
    else if (a.kl <= 8) hipLaunchKernelGGL((band_narrow_factor_kernel<T, 8>), dim3(G), dim3(64), 0, st, a);
    else hipLaunchKernelGGL((band_narrow_factor_kernel<T, 16>), dim3(G), dim3(64), 0, st, a);
    hipLaunchKernelGGL(band_narrow_back_kernel<T>, dim3(G), dim3(64), 0, st, a, out, ldo, slots, perm);
}

// ---- the split method (maus_band_set_split(ctx, 1, part_len), DESIGN §11 "The split method") -----------------------------
// One narrow band spread over the device: Gaussian elimination with partial pivoting on H Q, where Q lists the interiors of p
// column partitions first and the separators between them last.  With w = kl + ku, partition i is the columns
// [i m, min((i + 1) m, n)); all but the last end in a separator S_i of w columns, the rest is the interior I_i = [a_i, b_i].
// The rows R_i = [i m - ku, (i + 1) m - ku) (cut to [0, n)) are the rows with an entry in I_i; they tile [0, n) and a row of
// R_i has entries in S_{i-1}, I_i and S_i only.
//   local    one group of GS lanes per (matrix, partition) eliminates the columns of I_i in ascending order, pivoting among the
//            rows of R_i not yet used (first maximum of |re| + |im| in row order, a NaN never wins, a zero pivot records the
//            column, the zero candidate nearest the diagonal leaves and the step goes on without an update).  The live rows (at most w + 1) sit in LDS, one column per lane:
//            lanes 0 .. w - 1 the columns of S_{i-1} (fill), lanes w .. 2 w the band columns c .. c + w of step c (column c'
//            in lane w + c' % (w + 1)), lane 2 w + 1 the right-hand side.  The pivot row of column c goes to pr[c][2 w + 2]
//            (S_{i-1}, then columns c .. c + w, then the right-hand side); the rows left over at the end -- kl, w or ku of
//            them, with entries in S_{i-1} and S_i only -- go straight into the band storage of the reduced system, in row
//            order, the leftovers of partition i after those of partition i - 1.
//   reduced  the leftover rows are a band matrix of order n_red = (p - 1) w in the separator unknowns with half-bandwidths
//            kl + w - 1 and ku + w - 1 (cut to n_red - 1): launch_solve factors and solves it by the plan the context's
//            method gives for that band.
//   back     one group per (matrix, partition) solves I_i in descending order from the stored pivot rows: lane k holds the
//            coefficient k of the row and the x it multiplies, the 2 w + 1 products are summed by a butterfly over the group
//            (one fixed order), and the x of the band columns move up one lane per step.
// Every choice is a function of (n, kl, ku, part_len) alone, and a group works on its own partition only: a system's bits do
// not depend on the batch or the chunking.
template <class T>
hipError_t launch_solve(const BandPlan& plan, const BandArgsT<T>& a, const BlkArgs& w, int G, hipStream_t st, c128* out, long ldo,
                        const int* slots, const int* perm);
size_t band_per_solve(const BandPlan& plan, int n, int kl, int ku);
double band_flops(int n, int kl, int ku, int G);
double band_bytes(const BandPlan& plan, int n, int kl, int ku, int G);

constexpr int SPL_MAX_KL = NAR_MAX_KL;
constexpr int SPL_MAX_W = NAR_MAX_KV;
constexpr int SPL_NOINFO = 0x7f7f7f7f;                  // linfo after memset 0x7f: no zero pivot in the local phase

struct SplitPlan {
    bool on = false;                                    // the split takes the band
    int w = 0, m = 0, p = 0, gs = 0;                    // kl + ku, partition length, partitions, lanes per group
    int n_red = 0, kl_red = 0, ku_red = 0;
    BandPlan rplan;                                     // of the reduced system under the context's method
    size_t bytes = 0;                                   // of the split's arrays per solve
};

// the rule: m = 64 ceil(sqrt(n w) / 64), at least 2 w + 2 (the local phase's m steps against the reduced system's n w / m)
int split_len(int n, int kl, int ku) {
    const long w = kl + ku, nw = (long)n * w;
    long s = (long)std::sqrt((double)nw);
    while (s * s < nw) ++s;
    while (s > 0 && (s - 1) * (s - 1) >= nw) --s;
    return (int)std::max<long>((s + 63) / 64 * 64, 2 * w + 2);
}

// mode: the switch; part_len: 0 for the rule.  Returns false for a forced length below 2 w + 2 on a band in range.
bool split_plan(int method, int mode, int part_len, int n, int kl, int ku, SplitPlan* sp) {
    *sp = SplitPlan();
    const int w = kl + ku;
    if (!mode || w < 1 || kl > SPL_MAX_KL || w > SPL_MAX_W || n < 1) return true;
    if (part_len && part_len < 2 * w + 2) return false;
    const int m = part_len ? part_len : split_len(n, kl, ku);
    if (n <= m) return true;                            // fewer than two partitions
    sp->on = true; sp->w = w; sp->m = m; sp->p = (n + m - 1) / m;
    sp->gs = 2 * w + 2 <= 8 ? 8 : (2 * w + 2 <= 16 ? 16 : (2 * w + 2 <= 32 ? 32 : 64));
    sp->n_red = (sp->p - 1) * w;
    sp->kl_red = std::min(kl + w - 1, sp->n_red - 1);
    sp->ku_red = std::min(ku + w - 1, sp->n_red - 1);
    sp->rplan = band_plan(method, sp->kl_red, sp->ku_red);
    // pr, the reduced system's band_per_solve, its solution, and info / flags / the local phase's info
    sp->bytes = sizeof(c128) * (size_t)n * (2 * w + 2) + band_per_solve(sp->rplan, sp->n_red, sp->kl_red, sp->ku_red)
              + sizeof(c128) * (size_t)sp->n_red + 3 * sizeof(int);
    return true;
}

// the split's arrays for G solves: pr[G][n][2 w + 2], the reduced system r (its x: the right-hand side), its solution
// xs[G][n_red], the local phase's info linfo[G] and the reduced plan's panel
template <class T>
struct SplitWsT { T* pr; BandArgsT<T> r; c128* xs; int* linfo; BlkArgs rw; };

template <class T>
size_t split_carve(const SplitPlan& sp, int n, int G, char* base, SplitWsT<T>* ws) {
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return base + o; };
    SplitWsT<T> s;
    s.r.n = sp.n_red; s.r.kl = sp.kl_red; s.r.ku = sp.ku_red; s.r.ldab = 2 * sp.kl_red + sp.ku_red + 1;
    s.pr = (T*)take(sizeof(T) * (size_t)n * (2 * sp.w + 2) * G);
    s.r.ab = (T*)take(sizeof(T) * (size_t)s.r.ldab * sp.n_red * G);
    s.r.x = (T*)take(sizeof(T) * (size_t)sp.n_red * G);
    s.xs = (c128*)take(sizeof(c128) * (size_t)sp.n_red * G);
    s.r.ipiv = (int*)take(sizeof(int) * (size_t)sp.n_red * G);
    s.r.info = (int*)take(sizeof(int) * G);
    s.r.flags = (int*)take(sizeof(int) * G);
    s.linfo = (int*)take(sizeof(int) * G);
    s.rw.lw = (c128*)take(sizeof(c128) * sp.rplan.lw * G);
    s.rw.ju = (int*)take(sp.rplan.panel ? sizeof(int) * G : 0);
    s.rw.lh = sp.kl_red + sp.rplan.nb; s.rw.ls = (long)s.rw.lh * sp.rplan.nb;
    if (ws) *ws = s;
    return off;
}

template <class T>
struct SplitArgsT { T* pr; int* linfo; int w, m, p; };

// the lane traffic of the split's back substitution, per component
__device__ __forceinline__ void lane_xor_add(c128& t, int off) { t.x += __shfl_xor(t.x, off, 64); t.y += __shfl_xor(t.y, off, 64); }
__device__ __forceinline__ void lane_xor_add(double& t, int off) { t += __shfl_xor(t, off, 64); }
__device__ __forceinline__ c128 lane_shfl(c128 v, int l) { return cmake(__shfl(v.x, l, 64), __shfl(v.y, l, 64)); }
__device__ __forceinline__ double lane_shfl(double v, int l) { return __shfl(v, l, 64); }
__device__ __forceinline__ c128 lane_shfl_up1(c128 v) { return cmake(__shfl_up(v.x, 1, 64), __shfl_up(v.y, 1, 64)); }
__device__ __forceinline__ double lane_shfl_up1(double v) { return __shfl_up(v, 1, 64); }

// interior columns of partition i, and the longest interior among the NG partitions of a wave (the wave's trip count)
__device__ __forceinline__ int split_ni(int p, int m, int w, int n, int i) { return i < p - 1 ? m - w : n - (p - 1) * m; }
template <int NG>
__device__ __forceinline__ int split_trips(int p, int m, int w, int n, int i0) {
    int T = 0;
    for (int q = 0; q < NG; ++q) if (i0 + q < p) T = max(T, split_ni(p, m, w, n, i0 + q));
    return T;
}

template <class T, int GS>
__global__ void __launch_bounds__(64)
band_split_local_kernel(BandArgsT<T> a, BandArgsT<T> r, SplitArgsT<T> s)
{
    constexpr int NG = 64 / GS, RS = GS / 2;
    __shared__ T s_win[NG * RS * GS];
    __shared__ T s_l[NG * RS];
    __shared__ int s_row[NG * RS];
    __shared__ int s_pv[NG];
    const int g = blockIdx.y, grp = threadIdx.x / GS, l = threadIdx.x % GS;
    const int i = blockIdx.x * NG + grp;
    const bool act = i < s.p;
    const int n = a.n, kl = a.kl, ku = a.ku, w = s.w, ldab = a.ldab, m = s.m;
    const T* ab = a.ab + bix(a, g);
    const T* x = a.x + (long)g * n;
    int* ipiv = a.ipiv + (long)g * n;
    T* pr = s.pr + (long)g * n * (2 * w + 2);
    const bool hasL = act && i > 0, hasR = act && i < s.p - 1;
    const int a0 = act ? i * m : 0, ni = act ? split_ni(s.p, m, w, n, i) : 0;
    const int rs0 = max(a0 - ku, 0), rend = hasR ? a0 + m - ku : n;     // R_i = [rs0, rend)
    const int trips = split_trips<NG>(s.p, m, w, n, blockIdx.x * NG);
    const bool bandl = l >= w && l <= 2 * w;
    T* S = s_win + (long)grp * RS * GS + l;                             // this lane's column: row slot q at S[q * GS]
    T* sl = s_l + grp * RS;
    int* srow = s_row + grp * RS;
    auto elem = [&](int rr, int cc) -> T {
        return (cc >= 0 && cc < n && rr - cc <= kl && cc - rr <= ku) ? ab[w + rr - cc + (long)cc * ldab] : czero<T>();
    };
    // this lane's element of row rr while it owns band column mc
    auto rowval = [&](int rr, int mc) -> T {
        if (l < w) return hasL ? elem(rr, a0 - w + l) : czero<T>();
        if (l <= 2 * w) return elem(rr, mc);
        return l == 2 * w + 1 ? x[rr] : czero<T>();
    };
    int mycol = 0;
    if (bandl) { const int sg = l - w, am = a0 % (w + 1); mycol = a0 + (sg - am + w + 1) % (w + 1); }
    // the rows above a0 + kl are live before the first step, in slots 0 ..
    const int ninit = act ? min(a0 + kl, rend) - rs0 : 0;
    unsigned live = 0;
    int fs = ninit;                                                     // the free slot the next row enters
    for (int q = 0; q <= w; ++q) {
        S[q * GS] = q < ninit ? rowval(rs0 + q, mycol) : czero<T>();
        if (l == 0) srow[q] = q < ninit ? rs0 + q : INT_MAX;
        if (q < ninit) live |= 1u << q;
    }
    T inc = (ni > 0 && a0 + kl < rend) ? rowval(a0 + kl, mycol) : czero<T>();           // the row that enters at the first step
    for (int j = 0; j < trips; ++j) {
        const bool on = j < ni;
        const int c = a0 + j;
        const bool pl = on && bandl && mycol == c;                      // the lane of the pivot column
        if (on) {
            const int re = c + kl;
            if (re < rend) { S[fs * GS] = inc; if (l == 0) srow[fs] = re; live |= 1u << fs; }
            inc = (j + 1 < ni && re + 1 < rend) ? rowval(re + 1, pl ? c + w + 1 : mycol) : czero<T>();
        }
        lds_barrier();
        if (pl) {
            double best = -1.0; int bs = -1, brow = INT_MAX;
            for (int q = 0; q <= w; ++q)
                if (live >> q & 1) {
                    const double v = cabs1(S[q * GS]);
                    const int row = srow[q];
                    if (v > best || (v == best && row < brow)) { best = v; bs = q; brow = row; }   // NaN never wins (izamax)
                }
            if (!(best > 0.0)) {
                // no pivot: the row that leaves is the zero candidate (any candidate where all are NaN) nearest the diagonal,
                // the lower of two -- the row zgbtf2 leaves in place
                int fd = INT_MAX; brow = INT_MAX;
                for (int q = 0; q <= w; ++q)
                    if ((live >> q & 1) && (best < 0.0 || cabs1(S[q * GS]) == 0.0)) {
                        const int row = srow[q], d = abs(row - c);
                        if (d < fd || (d == fd && row < brow)) { fd = d; bs = q; brow = row; }
                    }
            }
            const T piv = S[bs * GS];
            const bool zp = ciszero(piv);
            if (zp) atomicMin(&s.linfo[g], c + 1);
            const T rc = zp ? czero<T>() : crecip(piv);
            for (int q = 0; q <= w; ++q) {
                const bool upd = (live >> q & 1) && q != bs;
                sl[q] = (upd && !zp) ? cmul(S[q * GS], rc) : czero<T>();
                if (q != bs) S[q * GS] = czero<T>();                               // column c is eliminated: the slot becomes column c + w + 1
            }
            s_pv[grp] = bs;
        }
        lds_barrier();
        if (on) {
            const int bs = s_pv[grp];
            const T u = S[bs * GS];
            if (l <= 2 * w + 1) pr[(long)c * (2 * w + 2) + (bandl ? w + mycol - c : l)] = u;
            if (l == 0) ipiv[c] = srow[bs] + 1;                         // 1-based row of H, as LAPACK counts
            live &= ~(1u << bs);
            if (!pl)
                for (int q = 0; q <= w; ++q)
                    if (live >> q & 1) { T v = S[q * GS]; cfms(v, sl[q], u); S[q * GS] = v; }
            S[bs * GS] = czero<T>();
            fs = bs;
            if (pl) mycol += w + 1;
        }
    }
    lds_barrier();
    if (!act) return;
    // the rows left over, in row order, into the reduced system: columns of S_{i-1} at (i - 1) w .., of S_i at i w ..
    const int rho0 = i == 0 ? 0 : kl + (i - 1) * w, kvr = r.kl + r.ku;
    T* rab = r.ab + bix(r, g);
    int q_red = -1;
    if (l < w) { if (hasL) q_red = (i - 1) * w + l; }
    else if (bandl) { if (hasR && mycol < a0 + m) q_red = i * w + mycol - (a0 + m - w); }
    for (int q = 0; q <= w; ++q) {
        if (!(live >> q & 1)) continue;
        int rank = 0;
        for (int t = 0; t <= w; ++t) if ((live >> t & 1) && srow[t] < srow[q]) ++rank;
        const int rho = rho0 + rank;
        if (q_red >= 0) rab[kvr + rho - q_red + (long)q_red * r.ldab] = S[q * GS];
        else if (l == 2 * w + 1) r.x[(long)g * r.n + rho] = S[q * GS];
    }
}

template <class T, int GS>
__global__ void __launch_bounds__(64)
band_split_back_kernel(BandArgsT<T> a, SplitArgsT<T> s, const c128* __restrict__ xs, int n_red, c128* __restrict__ out, long ldo,
                       const int* __restrict__ slots, const int* __restrict__ perm)
{
    constexpr int NG = 64 / GS;
    const int g = blockIdx.y, grp = threadIdx.x / GS, l = threadIdx.x % GS;
    const int i = blockIdx.x * NG + grp;
    const bool act = i < s.p;
    const int n = a.n, w = s.w, m = s.m;
    const T* pr = s.pr + (long)g * n * (2 * w + 2);
    const c128* xg = xs + (long)g * n_red;
    c128* o = out + (slots ? (long)slots[g] : (long)g) * ldo;
    const bool hasL = act && i > 0, hasR = act && i < s.p - 1;
    const int a0 = act ? i * m : 0, ni = act ? split_ni(s.p, m, w, n, i) : 0, b0 = a0 + ni - 1;
    const int trips = split_trips<NG>(s.p, m, w, n, blockIdx.x * NG);
    const bool mult = l < 2 * w + 1 && l != w;                          // a coefficient that multiplies an x
    bool bad = false;
    // lane k < w: x of column k of S_{i-1}; lane w + d, 1 <= d <= w: x of column c + d, at the start the columns of S_i
    T xv = czero<T>();
    if (l < w) { if (hasL) xv = cnarrow<T>(xg[(i - 1) * w + l]); }
    else if (l > w && l <= 2 * w) { if (hasR) xv = cnarrow<T>(xg[i * w + l - w - 1]); }
    if (hasR && l < w) {                                                // the separator's own x
        const c128 v = xg[i * w + l];
        const int c = a0 + m - w + l;
        o[perm ? perm[c] : c] = v; bad |= !cfinite(v);
    }
    T cur = (ni > 0 && l <= 2 * w + 1) ? pr[(long)b0 * (2 * w + 2) + l] : czero<T>();
    for (int j = 0; j < trips; ++j) {
        const bool on = j < ni;
        const int c = b0 - j;
        const T nxt = (j + 1 < ni && l <= 2 * w + 1) ? pr[(long)(c - 1) * (2 * w + 2) + l] : czero<T>();
        T t = l == 2 * w + 1 ? cur : czero<T>();
        if (mult) cfms(t, cur, xv);
#pragma unroll
        for (int off = GS / 2; off > 0; off >>= 1) lane_xor_add(t, off);
        const T piv = lane_shfl(cur, grp * GS + w);
        const T xc = cdiv(t, piv);
        const T up = lane_shfl_up1(xv);
        if (on) {
            if (l == 0) { o[perm ? perm[c] : c] = cwiden(xc); bad |= !cfinite(xc); }
            if (l == w + 1) xv = xc; else if (l > w + 1 && l <= 2 * w) xv = up;
        }
        cur = nxt;
    }
    if (bad) atomicOr(&a.flags[g], 2);
}

// The split solve of G matrices on `st`: the reduced system is zeroed, filled by the local phase, solved by its own plan
// (no slots, no permutation: its x goes to xs), then the back substitution writes everything out.
template <class T>
hipError_t launch_split(const SplitPlan& sp, const BandArgsT<T>& a, const SplitWsT<T>& ws, int G, hipStream_t st, c128* out, long ldo,
                        const int* slots, const int* perm) {
    const SplitArgsT<T> s{ws.pr, ws.linfo, sp.w, sp.m, sp.p};
    const BandArgsT<T>& r = ws.r;
    hipError_t err = hipMemsetAsync(r.ab, 0, sizeof(T) * (size_t)r.ldab * r.n * G, st);
    if (err == hipSuccess) err = hipMemsetAsync(r.info, 0, sizeof(int) * G, st);
    if (err == hipSuccess) err = hipMemsetAsync(r.flags, 0, sizeof(int) * G, st);
    if (err == hipSuccess) err = hipMemsetAsync(ws.linfo, 0x7f, sizeof(int) * G, st);
    if (err != hipSuccess) return err;
    const int ng = 64 / sp.gs;
    const dim3 grid((sp.p + ng - 1) / ng, G);
    switch (sp.gs) {
    case 8: hipLaunchKernelGGL((band_split_local_kernel<T, 8>), grid, dim3(64), 0, st, a, r, s); break;
    case 16: hipLaunchKernelGGL((band_split_local_kernel<T, 16>), grid, dim3(64), 0, st, a, r, s); break;
    case 32: hipLaunchKernelGGL((band_split_local_kernel<T, 32>), grid, dim3(64), 0, st, a, r, s); break;
    default: hipLaunchKernelGGL((band_split_local_kernel<T, 64>), grid, dim3(64), 0, st, a, r, s); break;
    }
    if ((err = hipGetLastError()) != hipSuccess) return err;
    if ((err = launch_solve(sp.rplan, r, ws.rw, G, st, ws.xs, r.n, nullptr, nullptr)) != hipSuccess) return err;
    switch (sp.gs) {
    case 8: hipLaunchKernelGGL((band_split_back_kernel<T, 8>), grid, dim3(64), 0, st, a, s, ws.xs, r.n, out, ldo, slots, perm); break;
    case 16: hipLaunchKernelGGL((band_split_back_kernel<T, 16>), grid, dim3(64), 0, st, a, s, ws.xs, r.n, out, ldo, slots, perm); break;
    case 32: hipLaunchKernelGGL((band_split_back_kernel<T, 32>), grid, dim3(64), 0, st, a, s, ws.xs, r.n, out, ldo, slots, perm); break;
    default: hipLaunchKernelGGL((band_split_back_kernel<T, 64>), grid, dim3(64), 0, st, a, s, ws.xs, r.n, out, ldo, slots, perm); break;
    }
    return hipGetLastError();
}

// band-order column of unknown q of the reduced system
int split_sep_col(const SplitPlan& sp, int q) { return (q / sp.w + 1) * sp.m - sp.w + q % sp.w; }

// info of the whole solve from the two phases: 1 + the smallest band-order column with a zero pivot, 0 for none
int split_info(const SplitPlan& sp, int linfo, int rinfo) {
    int info = linfo == SPL_NOINFO ? 0 : linfo;
    if (rinfo > 0) { const int c = split_sep_col(sp, rinfo - 1) + 1; info = info ? std::min(info, c) : c; }
    return info;
}

// flops of the elimination run: per interior column w rows over 2 w + 2 columns and the row's 2 w + 1 products in the back
// substitution, plus the reduced system's; bytes: the band read once, pr written and read once, the reduced system's arrays
double split_flops(const SplitPlan& sp, int n, int G) {
    return 8.0 * G * (double)n * ((double)sp.w * (2 * sp.w + 2) + 2 * sp.w + 1) + band_flops(sp.n_red, sp.kl_red, sp.ku_red, G);
}
double split_bytes_moved(const SplitPlan& sp, int n, int kl, int ku, int G) {
    return 16.0 * G * (double)n * (2 * kl + ku + 1 + 2) + 32.0 * G * (double)n * (2 * sp.w + 2)
         + band_bytes(sp.rplan, sp.n_red, sp.kl_red, sp.ku_red, G);
}

// workgroup size from (kl, ku) alone: one wave for narrow bands, where the barriers of every column dominate
int band_threads(int kl, int ku) {
    const long w = (long)kl * (kl + ku);
    return w <= 512 ? 64 : (w <= 32768 ? 256 : 1024);
}

template <class T>
void launch_factor(const BandArgsT<T>& a, int G, hipStream_t st) {
    switch (band_threads(a.kl, a.ku)) {
    case 64: hipLaunchKernelGGL((band_factor_kernel<T, 64>), dim3(G), dim3(64), 0, st, a); break;
    case 256: hipLaunchKernelGGL((band_factor_kernel<T, 256>), dim3(G), dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL((band_factor_kernel<T, 1024>), dim3(G), dim3(1024), 0, st, a); break;
    }
}

template <class T>
void launch_back(const BandArgsT<T>& a, int G, hipStream_t st, c128* out, long ldo, const int* slots, const int* perm) {
    switch (band_threads(a.kl, a.ku)) {
    case 64: hipLaunchKernelGGL((band_back_kernel<T, 64>), dim3(G), dim3(64), 0, st, a, out, ldo, slots, perm); break;
    case 256: hipLaunchKernelGGL((band_back_kernel<T, 256>), dim3(G), dim3(256), 0, st, a, out, ldo, slots, perm); break;
    default: hipLaunchKernelGGL((band_back_kernel<T, 1024>), dim3(G), dim3(1024), 0, st, a, out, ldo, slots, perm); break;
    }
}

// The solve of G matrices on `st` by the schedule of the plan.  w is read where plan.panel; the LW of the wide method lies
// behind the G panels of lw.  The one-launch-per-phase schedules (column, narrow) report their errors at the caller's next check.
template <class T>
hipError_t launch_solve(const BandPlan& plan, const BandArgsT<T>& a, const BlkArgs& w, int G, hipStream_t st, c128* out, long ldo,
                        const int* slots, const int* perm) {
    switch (plan.kind) {
    case BK_COLUMN:
        launch_factor(a, G, st);
        launch_back(a, G, st, out, ldo, slots, perm);
        return hipSuccess;
    case BK_NARROW:
        launch_narrow(a, G, st, out, ldo, slots, perm);
        return hipSuccess;
    default:
        break;
    }
    // the panel methods have no real instantiation: band_real_kinds keeps a real call away from them
    if constexpr (!std::is_same_v<T, c128>) return hipErrorInvalidValue;
    else switch (plan.kind) {
    case BK_BLOCKED:
        return plan.nb == BNB ? launch_blocked_nb<BNB>(a, w, G, st, out, ldo, slots, perm)
                              : launch_blocked_nb<BNB_TALL>(a, w, G, st, out, ldo, slots, perm);
    default: {
        c128* lwo = plan.nbo ? w.lw + plan.lw_small * G : nullptr;
        switch (plan.nb) {
        case BNB: return launch_tiled_nb<BNB>(a, w, lwo, G, st, out, ldo, slots, perm);
        case TNB_MID: return launch_tiled_nb<TNB_MID>(a, w, lwo, G, st, out, ldo, slots, perm);
        default: return launch_tiled_nb<TNB_TALL>(a, w, lwo, G, st, out, ldo, slots, perm);
        }
    }
    }
}

// algorithmic flops of G solves: 8 n kl (kl + ku) for the factorisation, 8 n (2 kl + ku) for the solve
double band_flops(int n, int kl, int ku, int G) { return 8.0 * G * n * ((double)kl * (kl + ku) + 2.0 * kl + ku); }

// Bytes of G solves.
//   column, narrow  the band storage read and written once.
//   blocked  the band once per block step over the columns a pivot row can reach (kl + ku of them when every step pivots from
//            the bottom; ku when none does -- the reach is only known on the device, so this is the upper end), and once more
//            in the back substitution.
//   tiled    the same upper end of the band per block step, and L21 once per column tile of the trailing update.
//   wide     that upper end once per outer block step, LW once per column tile of the outer trailing update, and inside the
//            block the inner steps' share: the block's NBO columns over the slice's rows and L21 once per column tile of the
//            inner trailing update.  An upper end like the two above.
double band_bytes(const BandPlan& plan, int n, int kl, int ku, int G) {
    const int nb = plan.nb;
    const double back = 16.0 * G * (double)n * (kl + ku + 1);
    switch (plan.kind) {
    case BK_BLOCKED:
        return 32.0 * G * ((double)(n + nb - 1) / nb) * (kl + nb) * (double)(nb + kl + ku) + back;
    case BK_TILED: {
        const double steps = (double)(n + nb - 1) / nb, nct = (double)((kl + ku + TCT - 1) / TCT + 1);
        return G * steps * (32.0 * (kl + nb) * (double)(nb + kl + ku) + 16.0 * (kl + nb) * (double)nb * nct) + back;
    }
    case BK_WIDE: {
        const double outer = (double)(n + NBO - 1) / NBO, inner = (double)(n + nb - 1) / nb;
        const double octs = (double)((kl + ku + OCT - 1) / OCT), icts = (double)(NBO / TCT + 1);
        return G * outer * (32.0 * (kl + NBO) * (double)(NBO + kl + ku) + 16.0 * (kl + NBO) * (double)NBO * octs)
             + G * inner * (32.0 * (kl + nb) * (double)NBO + 16.0 * (kl + nb) * (double)nb * icts) + back;
    }
    default:
        return 32.0 * G * (double)(2 * kl + ku + 1) * n;
    }
}

// bytes of one solve in the workspace: the band storage, the right-hand side and the pivots; where the plan has a panel, lw
// and the reach as well
size_t band_per_solve(const BandPlan& plan, int n, int kl, int ku) {
    const size_t ldab = 2 * (size_t)kl + ku + 1;
    return sizeof(c128) * (ldab * n + n) + sizeof(int) * (size_t)n + (plan.panel ? sizeof(c128) * plan.lw + sizeof(int) : 0);
}

void band_ws_free(maus_ctx* c) {
    void* ps[] = {c->band_ab, c->band_x, c->band_ipiv, c->band_info, c->band_flags, c->band_lw, c->band_ju, c->band_sws};
    for (void* p : ps) if (p) (void)hipFree(p);
    c->band_lw = nullptr; c->band_ju = nullptr; c->band_sws = nullptr; c->band_ws_m = 0;
    c->band_ab = nullptr; c->band_x = nullptr; c->band_ipiv = nullptr; c->band_info = nullptr; c->band_flags = nullptr;
    c->band_g = 0; c->band_at_limit = false; c->band_ws_key = 0;
}

// Band workspace for `want` simultaneous solves of the bound ordering, sized as ensure_lu_ws sizes the dense one: announced
// once (maus_band_reserve), grown at most once more -- then to the cap (MAUS_BAND_BATCH, default 512, and 80 % of free
// memory) -- never shrunk; larger batches run in balanced chunks.
int ensure_band_ws(maus_ctx* c, int want) {
    const int n = c->band_n, ldab = 2 * c->band_kl + c->band_ku + 1;
    const BandPlan plan = band_plan(c->band_method, c->band_kl, c->band_ku);
    SplitPlan sp;
    if (!split_plan(c->band_method, c->band_split, c->band_split_len, n, c->band_kl, c->band_ku, &sp))
        FAIL(c, "band workspace: the partition length of maus_band_set_split is below 2 (kl + ku) + 2 for the bound band");
    const size_t per = band_per_solve(plan, n, c->band_kl, c->band_ku) + sp.bytes;
    const unsigned long long key = ((unsigned long long)n << 32) | ((unsigned long long)plan.panel << 31) | ((unsigned long long)(plan.nbo != 0) << 30)
                                 | ((unsigned long long)sp.on << 29) | ((unsigned long long)sp.rplan.panel << 28) | (unsigned)ldab;
    const bool same = c->band_ab && c->band_ws_key == key && c->band_ws_m == sp.m;
    if (same && (c->band_g >= want || c->band_at_limit)) return 0;
    size_t fr = 0, tot = 0;
    HIPCHK(c, hipMemGetInfo(&fr, &tot));
    if (same) fr += per * c->band_g;
    const int gmax = (int)std::max<size_t>(1, (size_t)(fr * 0.80) / per);
    const char* env = getenv("MAUS_BAND_BATCH");
    const int cap = env ? std::max(1, atoi(env)) : 512;
    int G = std::max(1, want);
    if (same) G = std::max(G, cap);                                     // a second allocation goes straight to the limit
    G = std::min(std::min(G, cap), gmax);
    if (same && c->band_g >= G) { c->band_at_limit = true; return 0; }
    HIPCHK(c, hipStreamSynchronize(c->st));
    band_ws_free(c);
    const int G_asked = G;
    while (hipMalloc((void**)&c->band_ab, sizeof(c128) * (size_t)ldab * n * G) != hipSuccess) {
        (void)hipGetLastError();
        c->band_ab = nullptr;
        if (G > 1) G = std::max(1, G * 3 / 4); else FAIL(c, "band workspace: hipMalloc failed even for one solve (out of device memory)");
    }
    HIPCHK(c, hipMalloc((void**)&c->band_x, sizeof(c128) * (size_t)n * G));
    HIPCHK(c, hipMalloc((void**)&c->band_ipiv, sizeof(int) * (size_t)n * G));
    HIPCHK(c, hipMalloc((void**)&c->band_info, sizeof(int) * G));
    HIPCHK(c, hipMalloc((void**)&c->band_flags, sizeof(int) * G));
    if (plan.panel) {
        HIPCHK(c, hipMalloc((void**)&c->band_lw, sizeof(c128) * plan.lw * G));
        HIPCHK(c, hipMalloc((void**)&c->band_ju, sizeof(int) * G));
    }
    if (sp.on) HIPCHK(c, hipMalloc((void**)&c->band_sws, split_carve<c128>(sp, n, G, nullptr, nullptr)));
    c->band_ws_m = sp.m;
    c->band_g = G; c->band_ws_key = key; c->band_allocs++;
    c->band_at_limit = same || G < G_asked || G >= std::min(cap, gmax);
    return 0;
}

// the workspace of the context as T: the real path uses the same allocation as doubles
template <class T>
BandArgsT<T> band_args(maus_ctx* c) {
    BandArgsT<T> a;
    a.ab = (T*)c->band_ab; a.x = (T*)c->band_x; a.ipiv = c->band_ipiv; a.info = c->band_info; a.flags = c->band_flags;
    a.n = c->band_n; a.kl = c->band_kl; a.ku = c->band_ku; a.ldab = 2 * a.kl + a.ku + 1;
    return a;
}

BlkArgs blk_args(const BandPlan& plan, int kl, c128* lw, int* ju) {
    BlkArgs w; w.lw = lw; w.ju = ju;
    w.lh = kl + plan.nb; w.ls = (long)w.lh * plan.nb;
    return w;
}

void band_status(int G, const int* info, const int* flags, int32_t* status) {
    for (int g = 0; g < G; ++g) {
        if (flags[g] & 1) status[g] = -1;
        else if (info[g] > 0) status[g] = info[g];
        else if (flags[g] & 2) status[g] = -2;
        else status[g] = 0;
    }
}

// the solve of G matrices by the split where its plan takes the band, else by the method's plan
template <class T>
hipError_t launch_any(const SplitPlan& sp, const SplitWsT<T>& ws, const BandPlan& plan, const BandArgsT<T>& a, const BlkArgs& w, int G, hipStream_t st,
                      c128* out, long ldo, const int* slots, const int* perm) {
    return sp.on ? launch_split(sp, a, ws, G, st, out, ldo, slots, perm) : launch_solve(plan, a, w, G, st, out, ldo, slots, perm);
}

// profile class and the scale of the complex flop (1 / 4) and byte (1 / 2) formulas on T
template <class T> int prof_class(const SplitPlan& sp, const BandPlan& plan) {
    return std::is_same_v<T, c128> ? (sp.on ? (int)KC_BAND_SPLIT : plan.cls) : (int)KC_BAND_REAL;
}
template <class T> double prof_scale(int by) { return std::is_same_v<T, c128> ? 1.0 : 1.0 / by; }

// Whether every kernel that a solve of an (n, kl, ku) band runs under (method, split) has a real instantiation: the column
// kernel and the narrow method have, for the band itself or for the split's reduced system.  False for a bad partition length.
bool band_real_kinds(int method, int split_mode, int part_len, int n, int kl, int ku, bool* real, int* kind, bool* split) {
    SplitPlan sp;
    if (!split_plan(method, split_mode, part_len, n, kl, ku, &sp)) return false;
    const BandPlan plan = band_plan(method, kl, ku);
    const BandKind k = sp.on ? sp.rplan.kind : plan.kind;
    *real = k == BK_COLUMN || k == BK_NARROW; *kind = plan.kind; *split = sp.on;
    return true;
}

// The rule of the real path, stated once: maus_band_solve decides by it and maus_band_real_plan reports it.  All or nothing
// per call.  MAUS_BAND_REAL_OK or the first condition that fails.
int band_real_rule(const maus_ctx* c, int rhs_mode, int count, const double* shift) {
    if (c->band_real != 1) return MAUS_BAND_REAL_OFF;
    if (!c->csr || c->rows != c->cols || !c->band_perm || c->band_n != c->rows) return MAUS_BAND_REAL_NOT_CSR;
    if (!c->A_real) return MAUS_BAND_REAL_MATRIX_COMPLEX;
    if (rhs_mode != 1) return MAUS_BAND_REAL_RHS_ROWS;
    if (!c->b || !c->b_real) return MAUS_BAND_REAL_RHS_COMPLEX;
    if (count > 0 && (!shift || !maus_real_flagged(shift, (size_t)count))) return MAUS_BAND_REAL_SHIFT_COMPLEX;
    bool real = false, split = false; int kind = 0;
    if (!band_real_kinds(c->band_method, c->band_split, c->band_split_len, c->band_n, c->band_kl, c->band_ku, &real, &kind, &split) || !real)
        return MAUS_BAND_REAL_NO_KERNELS;
    return MAUS_BAND_REAL_OK;
}

// maus_band_lu_host on T: ab and b are the caller's arrays as T (the real path: their real parts)
template <class T>
int band_lu_host_t(maus_ctx* c, int count, int n, int kl, int ku, const T* ab, const T* b, double* x_out,
                   int32_t* ipiv_out, int32_t* info_out) {
    BandArgsT<T> a;
    a.n = n; a.kl = kl; a.ku = ku; a.ldab = 2 * kl + ku + 1;
    const size_t abb = sizeof(T) * (size_t)a.ldab * n, xb = sizeof(T) * (size_t)n, ob = sizeof(c128) * (size_t)n, ib = sizeof(int) * (size_t)n;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const size_t o_ab = take(abb * count), o_x = take(xb * count), o_o = take(ob * count), o_p = take(ib * count),
                 o_i = take(sizeof(int) * count), o_f = take(sizeof(int) * count);
    const BandPlan plan = band_plan(c->band_method, kl, ku);
    const size_t o_l = take(sizeof(c128) * plan.lw * count), o_j = take(plan.panel ? sizeof(int) * count : 0);
    SplitPlan sp;
    if (!split_plan(c->band_method, c->band_split, c->band_split_len, n, kl, ku, &sp))
        FAIL(c, "maus_band_lu_host: the partition length of maus_band_set_split is below 2 (kl + ku) + 2 for this band");
    const size_t o_s = take(sp.on ? split_carve<T>(sp, n, count, nullptr, nullptr) : 0);
    if (ensure_scratch(c, off)) return -1;
    char* base = (char*)c->scratch;
    a.ab = (T*)(base + o_ab); a.x = (T*)(base + o_x); a.ipiv = (int*)(base + o_p); a.info = (int*)(base + o_i); a.flags = (int*)(base + o_f);
    c128* out = (c128*)(base + o_o);
    const BlkArgs w = blk_args(plan, kl, plan.panel ? (c128*)(base + o_l) : nullptr, plan.panel ? (int*)(base + o_j) : nullptr);
    SplitWsT<T> ws{};
    if (sp.on) split_carve(sp, n, count, base + o_s, &ws);
    if (maus_stage_h2d(c, a.ab, ab, abb * count, c->st)) return -1;
    if (maus_stage_h2d(c, a.x, b, xb * count, c->st)) return -1;
    HIPCHK(c, hipMemsetAsync(a.info, 0, sizeof(int) * count, c->st));
    HIPCHK(c, hipMemsetAsync(a.flags, 0, sizeof(int) * count, c->st));
    {
        ProfScope ps(c, prof_class<T>(sp, plan), prof_scale<T>(4) * (sp.on ? split_flops(sp, n, count) : band_flops(n, kl, ku, count)),
                     prof_scale<T>(2) * (sp.on ? split_bytes_moved(sp, n, kl, ku, count) : band_bytes(plan, n, kl, ku, count)));
        hipLaunchKernelGGL(band_scan_kernel<T>, dim3(64, count), dim3(256), 0, c->st, a);
        if constexpr (std::is_same_v<T, c128>)
            if (plan.panel && !sp.on) hipLaunchKernelGGL(band_zero_fill_kernel, dim3(64, count), dim3(256), 0, c->st, a);
        HIPCHK(c, launch_any(sp, ws, plan, a, w, count, c->st, out, n, nullptr, nullptr));
    }
    std::vector<int> h_info(count), h_flags(count), h_rinfo(sp.on ? count : 0), h_ripiv(sp.on && ipiv_out ? (size_t)sp.n_red * count : 0);
    if (maus_stage_d2h(c, x_out, out, ob * count, c->st)) return -1;
    if (ipiv_out && maus_stage_d2h(c, ipiv_out, a.ipiv, ib * count, c->st)) return -1;
    if (!h_ripiv.empty() && maus_stage_d2h(c, h_ripiv.data(), ws.r.ipiv, sizeof(int) * h_ripiv.size(), c->st)) return -1;
    if (maus_d2h(c, h_info.data(), sp.on ? ws.linfo : a.info, sizeof(int) * count, c->st)) return -1;
    if (sp.on && maus_d2h(c, h_rinfo.data(), ws.r.info, sizeof(int) * count, c->st)) return -1;
    if (maus_d2h(c, h_flags.data(), a.flags, sizeof(int) * count, c->st)) return -1;
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    if (sp.on) {
        for (int g = 0; g < count; ++g) h_info[g] = split_info(sp, h_info[g], h_rinfo[g]);
        // a separator column carries the pivot of its unknown of the reduced system (LAPACK's 1-based row of that system)
        if (ipiv_out)
            for (int g = 0; g < count; ++g)
                for (int q = 0; q < sp.n_red; ++q) ipiv_out[(size_t)g * n + split_sep_col(sp, q)] = h_ripiv[(size_t)g * sp.n_red + q];
    }
    band_status(count, h_info.data(), h_flags.data(), info_out);
    return 0;
}

// maus_band_solve on T (the caller has decided by band_real_rule): what the rule relies on is what the build kernel reads
template <class T>
int band_solve_t(maus_ctx* c, const int* slots, int count, const double* shift, const double* psi, int rhs_mode, int32_t* status) {
    if (!c->csr || !c->X) FAIL(c, "maus_band_solve: sparse matrix/population missing");
    if (!c->band_perm || c->band_n != c->rows) FAIL(c, "maus_band_solve: no ordering for the bound matrix (maus_band_prepare)");
    if (rhs_mode != 0 && rhs_mode != 1) FAIL(c, "maus_band_solve: rhs_mode must be 0 (X[slot]) or 1 (b)");
    if (rhs_mode == 1 && (!c->b || c->bn != c->rows)) FAIL(c, "maus_band_solve: rhs b not set");
    if (count == 0) return 0;
    if (check_slots(c, slots, count)) return -1;
    if (ensure_scalars(c, count)) return -1;
    if (ensure_band_ws(c, count)) return -1;
    const int nchunks = (count + c->band_g - 1) / c->band_g;            // balanced chunks, as maus_shifted_lu_solve
    const int Gmax = (count + nchunks - 1) / nchunks;
    std::vector<int> h_info(Gmax), h_flags(Gmax);
    const BandArgsT<T> a = band_args<T>(c);
    const BandPlan plan = band_plan(c->band_method, a.kl, a.ku);
    const BlkArgs w = blk_args(plan, a.kl, c->band_lw, c->band_ju);
    SplitPlan sp;
    SplitWsT<T> ws{};
    (void)split_plan(c->band_method, c->band_split, c->band_split_len, a.n, a.kl, a.ku, &sp);   // checked by ensure_band_ws
    if (sp.on) split_carve(sp, a.n, c->band_g, c->band_sws, &ws);
    std::vector<int> h_rinfo(sp.on ? Gmax : 0);
    for (int off = 0; off < count; off += Gmax) {
        const int G = std::min(Gmax, count - off);
        if (maus_h2d(c, c->d_slots, slots + off, sizeof(int) * G, c->st)) return -1;
        if (maus_h2d(c, c->d_c1, shift + 2 * (size_t)off, sizeof(c128) * G, c->st)) return -1;
        if (maus_h2d(c, c->d_r1, psi + off, sizeof(double) * G, c->st)) return -1;
        {
            ProfScope ps(c, prof_class<T>(sp, plan), prof_scale<T>(4) * (sp.on ? split_flops(sp, a.n, G) : band_flops(a.n, a.kl, a.ku, G)),
                         prof_scale<T>(2) * (sp.on ? split_bytes_moved(sp, a.n, a.kl, a.ku, G) : band_bytes(plan, a.n, a.kl, a.ku, G)));
            HIPCHK(c, hipMemsetAsync(a.info, 0, sizeof(int) * G, c->st));
            HIPCHK(c, hipMemsetAsync(a.flags, 0, sizeof(int) * G, c->st));
            HIPCHK(c, hipMemsetAsync(a.ab, 0, sizeof(T) * (size_t)a.ldab * a.n * G, c->st));
            hipLaunchKernelGGL(band_build_csr_kernel<T>, dim3((a.n + 255) / 256, G), dim3(256), 0, c->st, a, c->Acsr.ptr, c->Acsr.idx,
                               c->Acsr.val, c->band_perm, c->band_iperm, c->d_c1, c->d_r1, rhs_mode, c->X, c->ldp, c->d_slots, c->b);
            HIPCHK(c, launch_any(sp, ws, plan, a, w, G, c->st, c->W, c->ldp, c->d_slots, c->band_perm));
        }
        if (maus_d2h(c, h_info.data(), sp.on ? ws.linfo : a.info, sizeof(int) * G, c->st)) return -1;
        if (sp.on && maus_d2h(c, h_rinfo.data(), ws.r.info, sizeof(int) * G, c->st)) return -1;
        if (maus_d2h(c, h_flags.data(), a.flags, sizeof(int) * G, c->st)) return -1;
        HIPCHK(c, hipStreamSynchronize(c->st));
        HIPCHK(c, hipGetLastError());
        if (sp.on) for (int g = 0; g < G; ++g) h_info[g] = split_info(sp, h_info[g], h_rinfo[g]);
        band_status(G, h_info.data(), h_flags.data(), status + off);
    }
    return 0;
}

}  // namespace

void maus_band_drop(maus_ctx* c) {
    if (c->band_perm) (void)hipFree(c->band_perm);
    if (c->band_iperm) (void)hipFree(c->band_iperm);
    c->band_perm = nullptr; c->band_iperm = nullptr;
    c->band_n = 0; c->band_kl = -1; c->band_ku = -1;
    band_ws_free(c);
}

extern "C" {

int maus_sparse_max_n(void) { return 1 << 20; }

int maus_band_prepare(maus_ctx* c, const int32_t* perm, int n, int* kl_out, int* ku_out) {
    if (!c) return -1;
    if (!c->csr) FAIL(c, "maus_band_prepare: no sparse matrix bound (maus_set_matrix_csr)");
    if (c->rows != c->cols || n != c->rows) FAIL(c, "maus_band_prepare: the ordering must have the bound square matrix's n entries");
    if (!perm) FAIL(c, "maus_band_prepare: null ordering");
    if (n > maus_sparse_max_n()) FAIL(c, "maus_band_prepare: n exceeds maus_sparse_max_n()");
    std::vector<int> iperm((size_t)n, -1);
    for (int i = 0; i < n; ++i) {
        const int r = perm[i];
        if (r < 0 || r >= n || iperm[r] >= 0) FAIL(c, "maus_band_prepare: perm is not a permutation of 0..n-1");
        iperm[r] = i;
    }
    // kl / ku of A[perm][:, perm] from the pattern of the bound CSR matrix
    std::vector<int> ptr((size_t)n + 1), idx((size_t)c->Acsr.nnz);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(ptr.data(), c->Acsr.ptr, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost));
    if (c->Acsr.nnz) HIPCHK(c, hipMemcpy(idx.data(), c->Acsr.idx, sizeof(int) * (size_t)c->Acsr.nnz, hipMemcpyDeviceToHost));
    int kl = 0, ku = 0;
    for (int r = 0; r < n; ++r) {
        const int i = iperm[r];
        for (int p = ptr[r]; p < ptr[r + 1]; ++p) {
            const int d = i - iperm[idx[p]];
            kl = std::max(kl, d); ku = std::max(ku, -d);
        }
    }
    maus_band_drop(c);
    HIPCHK(c, hipMalloc((void**)&c->band_perm, sizeof(int) * (size_t)n));
    HIPCHK(c, hipMalloc((void**)&c->band_iperm, sizeof(int) * (size_t)n));
    HIPCHK(c, hipMemcpy(c->band_perm, perm, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->band_iperm, iperm.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    c->band_n = n; c->band_kl = kl; c->band_ku = ku;
    if (kl_out) *kl_out = kl;
    if (ku_out) *ku_out = ku;
    return 0;
}

int maus_band_reserve(maus_ctx* c, int count, int* capacity_out) {
    if (!c) return -1;
    if (!c->band_perm) FAIL(c, "maus_band_reserve: no ordering (maus_band_prepare)");
    if (count < 0) FAIL(c, "maus_band_reserve: bad count");
    if (count > 0 && ensure_band_ws(c, count)) return -1;
    if (capacity_out) *capacity_out = c->band_g;
    return 0;
}

int maus_band_solve(maus_ctx* c, const int* slots, int count, const double* shift, const double* psi, int rhs_mode, int32_t* status) {
    if (!c) return -1;
    maus_av_drop_all(c);
    // real or complex: one decision for the whole call (band_real_rule), also where the call then runs in chunks
    return band_real_rule(c, rhs_mode, count, shift) == MAUS_BAND_REAL_OK ? band_solve_t<double>(c, slots, count, shift, psi, rhs_mode, status)
                                                                          : band_solve_t<c128>(c, slots, count, shift, psi, rhs_mode, status);
}

int maus_band_workspace_allocs(maus_ctx* c) { return c ? c->band_allocs : -1; }

int maus_band_set_method(maus_ctx* c, int method) {
    if (!c) return -1;
    if (!band_method_ok(method))
        FAIL(c, "maus_band_set_method: method must be 0 (column), 1 (blocked), 2 (tiled), 4 (wide) or 8 (narrow)");
    c->band_method = method;                                            // the workspace follows at its next use (ensure_band_ws)
    return 0;
}

int maus_band_get_method(maus_ctx* c) { return c ? c->band_method : -1; }

int maus_band_kernel_for(maus_ctx* c, int n, int kl, int ku, int* nb_out) {
    if (!c) return -1;
    if (n <= 0 || kl < 0 || ku < 0) FAIL(c, "maus_band_kernel_for: bad sizes");
    const BandPlan plan = band_plan(c->band_method, kl, ku);
    if (nb_out) *nb_out = plan.nb;
    return plan.kind;
}

int maus_band_outer_nb(maus_ctx* c, int n, int kl, int ku) {
    if (!c) return -1;
    if (n <= 0 || kl < 0 || ku < 0) FAIL(c, "maus_band_outer_nb: bad sizes");
    return band_plan(c->band_method, kl, ku).nbo;
}

int maus_band_plan(int method, int n, int kl, int ku, int32_t* kind, int32_t* nb, int32_t* outer_nb, int64_t* ws_bytes_per_solve) {
    if (!band_method_ok(method) || n < 0 || kl < 0 || ku < 0) return -1;
    const BandPlan plan = band_plan(method, kl, ku);
    if (kind) *kind = plan.kind;
    if (nb) *nb = plan.nb;
    if (outer_nb) *outer_nb = plan.nbo;
    if (ws_bytes_per_solve) *ws_bytes_per_solve = (int64_t)band_per_solve(plan, n, kl, ku);
    return 0;
}

int maus_band_set_split(maus_ctx* c, int mode, int part_len) {
    if (!c) return -1;
    if ((mode != 0 && mode != 1) || part_len < 0)
        FAIL(c, "maus_band_set_split: mode must be 0 (off) or 1 (on), part_len 0 (the rule) or a partition length");
    c->band_split = mode; c->band_split_len = part_len;                 // the workspace follows at its next use (ensure_band_ws)
    return 0;
}

int maus_band_get_split(maus_ctx* c, int* part_len_out) {
    if (!c) return -1;
    if (part_len_out) *part_len_out = c->band_split_len;
    return c->band_split;
}

int maus_band_split_plan(int method, int n, int kl, int ku, int part_len, int32_t* takes, int32_t* part_len_out, int32_t* parts,
                         int32_t* n_red, int32_t* kl_red, int32_t* ku_red, int64_t* ws_bytes_per_solve) {
    if (!band_method_ok(method) || n < 0 || kl < 0 || ku < 0 || part_len < 0) return -1;
    SplitPlan sp;
    if (!split_plan(method, 1, part_len, n, kl, ku, &sp)) return -1;
    if (takes) *takes = sp.on;
    if (part_len_out) *part_len_out = sp.m;
    if (parts) *parts = sp.p;
    if (n_red) *n_red = sp.n_red;
    if (kl_red) *kl_red = sp.kl_red;
    if (ku_red) *ku_red = sp.ku_red;
    if (ws_bytes_per_solve) *ws_bytes_per_solve = (int64_t)sp.bytes;
    return 0;
}

int maus_band_lu_host(maus_ctx* c, int count, int n, int kl, int ku, const double* ab, const double* b, double* x_out,
                      int32_t* ipiv_out, int32_t* info_out) {
    if (!c) return -1;
    if (count <= 0 || n <= 0 || kl < 0 || ku < 0 || n > maus_sparse_max_n()) FAIL(c, "maus_band_lu_host: bad sizes");
    if (!ab || !b || !x_out || !info_out) FAIL(c, "maus_band_lu_host: null array");
    // the real path (maus_band_set_real): the plan has real kernels and every element handed in is flagged real
    bool real = false, split = false; int kind = 0;
    const size_t nab = (size_t)(2 * kl + ku + 1) * n * count, nb = (size_t)n * count;
    if (c->band_real == 1 && band_real_kinds(c->band_method, c->band_split, c->band_split_len, n, kl, ku, &real, &kind, &split) && real
        && maus_real_flagged(ab, nab) && maus_real_flagged(b, nb)) {
        std::vector<double> abr(nab), br(nb);
        for (size_t i = 0; i < nab; ++i) abr[i] = ab[2 * i];
        for (size_t i = 0; i < nb; ++i) br[i] = b[2 * i];
        return band_lu_host_t<double>(c, count, n, kl, ku, abr.data(), br.data(), x_out, ipiv_out, info_out);
    }
    return band_lu_host_t<c128>(c, count, n, kl, ku, (const c128*)ab, (const c128*)b, x_out, ipiv_out, info_out);
}

int maus_band_set_real(maus_ctx* c, int mode) {
    if (!c) return -1;
    if (mode != 0 && mode != 1) FAIL(c, "maus_band_set_real: mode must be 0 (complex arithmetic) or 1 (real arithmetic where the rule holds)");
    c->band_real = mode;
    return 0;
}

int maus_band_get_real(maus_ctx* c) { return c ? c->band_real : -1; }

int maus_band_real_plan(maus_ctx* c, int rhs_mode, int count, const double* shift, int32_t* out) {
    if (!c) return -1;
    if (count < 0 || (count > 0 && !shift) || !out) FAIL(c, "maus_band_real_plan: bad arguments");
    const int why = band_real_rule(c, rhs_mode, count, shift);
    bool real = false, split = false; int kind = 0;
    if (c->band_perm)
        (void)band_real_kinds(c->band_method, c->band_split, c->band_split_len, c->band_n, c->band_kl, c->band_ku, &real, &kind, &split);
    out[0] = why == MAUS_BAND_REAL_OK; out[1] = why; out[2] = kind; out[3] = split;
    return 0;
}

int maus_band_real_kinds(int method, int split_mode, int part_len, int n, int kl, int ku, int32_t* out) {
    if (!band_method_ok(method) || (split_mode != 0 && split_mode != 1) || part_len < 0 || n < 0 || kl < 0 || ku < 0 || !out) return -1;
    bool real = false, split = false; int kind = 0;
    if (!band_real_kinds(method, split_mode, part_len, n, kl, ku, &real, &kind, &split)) return -1;
    out[0] = real; out[1] = kind; out[2] = split;
    return 0;
}

}  // extern "C"
