// Sparse problem matrices: complex fp64 CSR times a gathered block of population rows, the diagonal of a CSR
// matrix, and the validation / upload behind maus_set_matrix_csr.
//
//     C[c_rows[k]][i] = sum_{p in row i} val[p] * B[a_rows[k]][idx[p]]        (k < count, i < nrows)
//
// The population is candidate-major (one row of ld elements per candidate), exactly as for maus_zgemm_launch_idx.  op(A) = A^H
// is the same product on the CSR of A^H, built once at bind time.
//
// Every output element is summed in one fixed order that depends on the matrix alone: the short-row schedule accumulates a
// row's nonzeros one after the other in CSR order; the long-row schedule gives lane l the nonzeros l, l + 64, ... of the row
// and joins the 64 partial sums by the fixed DPP tree of wave_sum_dpp.  Which candidates share a launch, how many there are and
// in which order they are gathered never enters the arithmetic, so a row's product is bit-identical alone, among 33 rows or
// among 256 -- what the kept-product stamps of capi.hip (av_*, ahu_*) rely on.  The schedule is chosen once per matrix from
// nnz / rows (csr_schedule) and reported by maus_matrix_is_sparse.
//
// Under maus_spmm_set_method(ctx, 1) an operand of the short-row schedule is also kept in sliced-ELL form (MausSell, built on the
// device at bind time) and spmm_sell_kernel reads that copy: the same lane per row, the same operations in the same order, the
// same bits, with coalesced operand loads and several nonzeros' gathers in flight.  spmm_kind states which operand takes it.
#include "ctx.h"
#include <cstring>

namespace {

constexpr int SP_CG = 8;          // candidates per thread: each nonzero (16 B value + 4 B index) is loaded once per 8 candidates
constexpr int SP_BT = 256;        // threads per block

// short rows (banded operators, up to ~32 nonzeros per row): one lane per row, so consecutive lanes gather neighbouring x[col]
// T = c128, or double for the real path (maus_real_set_method): the operand's real copy times rows of doubles, the same lane,
// the same order, one fma where the complex text has the two of a real part (common.h)
template <class T>
__global__ void __launch_bounds__(SP_BT)
spmm_rows_kernel(const int* __restrict__ ptr, const int* __restrict__ idx, const T* __restrict__ val, int nrows,
                 const T* __restrict__ B, long ldb, T* __restrict__ C, long ldc,
                 const int* __restrict__ a_rows, const int* __restrict__ c_rows, int count)
{
    const int i = blockIdx.x * SP_BT + threadIdx.x;
    const int k0 = blockIdx.y * SP_CG;
    if (i >= nrows) return;
    const int ng = min(SP_CG, count - k0);
    const T* b[SP_CG];
    T acc[SP_CG];
#pragma unroll
    for (int g = 0; g < SP_CG; ++g) {
        b[g] = B + (long)a_rows[k0 + (g < ng ? g : 0)] * ldb;
        acc[g] = czero<T>();
    }
    const int p1 = ptr[i + 1];
    for (int p = ptr[i]; p < p1; ++p) {
        const T a = val[p];
        const int j = idx[p];
#pragma unroll
        for (int g = 0; g < SP_CG; ++g)
            if (g < ng) cfma(acc[g], a, b[g][j]);
    }
#pragma unroll
    for (int g = 0; g < SP_CG; ++g)
        if (g < ng) C[(long)c_rows[k0 + g] * ldc + i] = acc[g];
}

// The lane-per-row product on the sliced-ELL copy of the operand (MausSell, maus_spmm_set_method(ctx, 1); DESIGN §10 "SpMM on a
// sliced-ELL copy").  Geometry and index lists are those of spmm_rows_kernel.  Entry p of the 64 rows of a slice is one
// contiguous run of 64 indices (256 B) and 64 values (1 KB), so a wave's operand load touches 4 + 16 cache lines where the CSR
// walk touches up to 64 + 64, and the loads of U consecutive entries and their U x ng gathers are issued before the first
// product needs them.  A lane adds the entries of its own row for p ascending, with cfma, onto a zero accumulator: the CSR
// kernel's operations in the CSR kernel's order, so the same bits.  A lane stops at its own length; lanes of a wave that are
// done sit out the rest of the wave's loop, and padding is neither loaded nor multiplied.
// The three constants can be set from the command line (make EXTRA=-DMAUS_SELL_U=2 ...) for the side-by-side builds of
// profiles/spmm_sell_variants.txt; the bits do not depend on them.
#ifndef MAUS_SELL_U
#define MAUS_SELL_U 4
#endif
#ifndef MAUS_SELL_U1
#define MAUS_SELL_U1 8
#endif
#ifndef MAUS_SELL_G1
#define MAUS_SELL_G1 1
#endif
constexpr int SELL_U = MAUS_SELL_U;     // entries in flight per lane, groups of 8 candidates (4: 189 VGPRs, 2 waves per SIMD)
constexpr int SELL_U_SHORT = 2;         // the same where no row has SELL_U entries (117 VGPRs, 4 waves per SIMD)
constexpr int SELL_U1 = MAUS_SELL_U1;   // the same for a lone candidate: Lanczos, one row of a population (8: 62 VGPRs, 8 waves per SIMD)
constexpr bool SELL_G1 = MAUS_SELL_G1;  // a lone candidate runs the instantiation with a group of 1

// W consecutive entries of the lane's row from entry p on: W index / value loads, then W x ng gathers, then the products for
// p ascending
template <class T, int CG, int W>
__device__ __forceinline__ void sell_chunk(T (&acc)[CG], const T* const (&b)[CG], int ng,
                                           const int* __restrict__ ji, const T* __restrict__ av, int p)
{
    int j[W];
    T a[W], x[W][CG];
#pragma unroll
    for (int u = 0; u < W; ++u) {
        j[u] = ji[(long)(p + u) * MAUS_WAVE];
        a[u] = av[(long)(p + u) * MAUS_WAVE];
    }
#pragma unroll
    for (int u = 0; u < W; ++u)
#pragma unroll
        for (int g = 0; g < CG; ++g)
            if (g < ng) x[u][g] = b[g][j[u]];
#pragma unroll
    for (int u = 0; u < W; ++u)
#pragma unroll
        for (int g = 0; g < CG; ++g)
            if (g < ng) cfma(acc[g], a[u], x[u][g]);
}

template <class T, int CG, int U>
__global__ void __launch_bounds__(SP_BT)
spmm_sell_kernel(const long* __restrict__ off, const int* __restrict__ len, const int* __restrict__ idx, const T* __restrict__ val,
                 int nrows, const T* __restrict__ B, long ldb, T* __restrict__ C, long ldc,
                 const int* __restrict__ a_rows, const int* __restrict__ c_rows, int count)
{
    const int i = blockIdx.x * SP_BT + threadIdx.x;
    const int k0 = blockIdx.y * CG;
    if (i >= nrows) return;
    const int ng = min(CG, count - k0);
    const T* b[CG];
    T acc[CG];
#pragma unroll
    for (int g = 0; g < CG; ++g) {
        b[g] = B + (long)a_rows[k0 + (g < ng ? g : 0)] * ldb;
        acc[g] = czero<T>();
    }
    const long base = off[i / MAUS_WAVE] + (i % MAUS_WAVE);
    const int* __restrict__ ji = idx + base;
    const T* __restrict__ av = val + base;
    const int n = len[i];
    int p = 0;
    for (; p + U <= n; p += U) sell_chunk<T, CG, U>(acc, b, ng, ji, av, p);
    // the row's last n % U entries, in chunks of 4, 2, 1: still p ascending
    if constexpr (U > 4) if (p + 4 <= n) { sell_chunk<T, CG, 4>(acc, b, ng, ji, av, p); p += 4; }
    if constexpr (U > 2) if (p + 2 <= n) { sell_chunk<T, CG, 2>(acc, b, ng, ji, av, p); p += 2; }
    if (p < n) sell_chunk<T, CG, 1>(acc, b, ng, ji, av, p);
#pragma unroll
    for (int g = 0; g < CG; ++g)
        if (g < ng) C[(long)c_rows[k0 + g] * ldc + i] = acc[g];
}

// Build of the sliced-ELL copy, step 1: len[r] of every row and, per slice (one wave), the longest of its 64 rows; rows past
// the end of the matrix count as empty
__global__ void __launch_bounds__(SP_BT)
sell_width_kernel(const int* __restrict__ ptr, int nrows, int nslices, int* __restrict__ len, int* __restrict__ width)
{
    const int r = blockIdx.x * SP_BT + threadIdx.x;
    int w = 0;
    if (r < nrows) { w = ptr[r + 1] - ptr[r]; len[r] = w; }
#pragma unroll
    for (int o = MAUS_WAVE / 2; o > 0; o >>= 1) w = max(w, __shfl_xor(w, o, MAUS_WAVE));
    if (r % MAUS_WAVE == 0 && r / MAUS_WAVE < nslices) width[r / MAUS_WAVE] = w;
}

// step 3 (step 2, the exclusive scan of 64 w_s into off, runs on the host): a thread per row copies its entries in CSR order and
// writes the rest of its lane of the slice as (index 0, value 0); one writer per slot, no atomics.  sidx == nullptr: the values
// alone (the real copy shares the indices of the complex one)
template <class T>
__global__ void __launch_bounds__(SP_BT)
sell_fill_kernel(const int* __restrict__ ptr, const int* __restrict__ idx, const T* __restrict__ val, int nrows, int nslices,
                 const long* __restrict__ off, int* __restrict__ sidx, T* __restrict__ sval)
{
    const int r = blockIdx.x * SP_BT + threadIdx.x;
    const int s = r / MAUS_WAVE;
    if (s >= nslices) return;
    const long base = off[s] + (r % MAUS_WAVE);
    const int w = (int)((off[s + 1] - off[s]) / MAUS_WAVE);
    const int p0 = r < nrows ? ptr[r] : 0;
    const int n = r < nrows ? ptr[r + 1] - p0 : 0;
    for (int p = 0; p < n; ++p) {
        if (sidx) sidx[base + (long)p * MAUS_WAVE] = idx[p0 + p];
        sval[base + (long)p * MAUS_WAVE] = val[p0 + p];
    }
    for (int p = n; p < w; ++p) {
        if (sidx) sidx[base + (long)p * MAUS_WAVE] = 0;
        sval[base + (long)p * MAUS_WAVE] = czero<T>();
    }
}

// long rows: one wave per row, lanes over the row's nonzeros, the partial sums joined by a fixed tree
__device__ __forceinline__ c128 sp_wave_sum(c128 v) { const double re = wave_sum_dpp(v.x), im = wave_sum_dpp(v.y); return cmake(re, im); }
__device__ __forceinline__ double sp_wave_sum(double v) { return wave_sum_dpp(v); }

template <class T>
__global__ void __launch_bounds__(SP_BT)
spmm_wave_kernel(const int* __restrict__ ptr, const int* __restrict__ idx, const T* __restrict__ val, int nrows,
                 const T* __restrict__ B, long ldb, T* __restrict__ C, long ldc,
                 const int* __restrict__ a_rows, const int* __restrict__ c_rows, int count)
{
    const int lane = threadIdx.x & (MAUS_WAVE - 1);
    const int i = blockIdx.x * (SP_BT / MAUS_WAVE) + threadIdx.x / MAUS_WAVE;
    const int k0 = blockIdx.y * SP_CG;
    if (i >= nrows) return;                       // whole waves leave together (i is uniform per wave)
    const int ng = min(SP_CG, count - k0);
    const T* b[SP_CG];
    T acc[SP_CG];
#pragma unroll
    for (int g = 0; g < SP_CG; ++g) {
        b[g] = B + (long)a_rows[k0 + (g < ng ? g : 0)] * ldb;
        acc[g] = czero<T>();
    }
    const int p1 = ptr[i + 1];
    for (int p = ptr[i] + lane; p < p1; p += MAUS_WAVE) {
        const T a = val[p];
        const int j = idx[p];
#pragma unroll
        for (int g = 0; g < SP_CG; ++g)
            if (g < ng) cfma(acc[g], a, b[g][j]);
    }
#pragma unroll
    for (int g = 0; g < SP_CG; ++g) {
        if (g >= ng) break;                       // ng is uniform per wave
        const T sum = sp_wave_sum(acc[g]);
        if (lane == 0) C[(long)c_rows[k0 + g] * ldc + i] = sum;
    }
}

// d[i] = A[i][i] (0 where the row stores no diagonal entry)
template <class T>
__global__ void __launch_bounds__(SP_BT)
csr_diag_kernel(const int* __restrict__ ptr, const int* __restrict__ idx, const T* __restrict__ val, int n, T* __restrict__ d)
{
    const int i = blockIdx.x * SP_BT + threadIdx.x;
    if (i >= n) return;
    T v = czero<T>();
    for (int p = ptr[i]; p < ptr[i + 1]; ++p)
        if (idx[p] == i) { v = val[p]; break; }
    d[i] = v;
}

// r[i] = Re z[i]: the real copy of values whose imaginary parts are all +-0 (maus_real_sync_*)
__global__ void __launch_bounds__(SP_BT)
real_part_kernel(const c128* __restrict__ z, double* __restrict__ r, long n)
{
    const long i = (long)blockIdx.x * SP_BT + threadIdx.x;
    if (i < n) r[i] = z[i].x;
}

// maus_real_spmm: R[k] = Re X[slots[k]] (and the row list 0 .. count - 1), and back, Y[slots[k]] = (Q[k], +0)
__global__ void __launch_bounds__(SP_BT)
real_rows_in_kernel(const c128* __restrict__ X, long ldx, const int* __restrict__ slots, int n, double* __restrict__ R, int* __restrict__ ident)
{
    const int i = blockIdx.x * SP_BT + threadIdx.x, k = blockIdx.y;
    if (i < n) R[(long)k * n + i] = X[(long)slots[k] * ldx + i].x;
    if (i == 0) ident[k] = k;
}
__global__ void __launch_bounds__(SP_BT)
real_rows_out_kernel(const double* __restrict__ Q, int n, const int* __restrict__ slots, c128* __restrict__ Y, long ldy)
{
    const int i = blockIdx.x * SP_BT + threadIdx.x, k = blockIdx.y;
    if (i < n) Y[(long)slots[k] * ldy + i] = cmake(Q[(long)k * n + i], 0.0);
}

}  // namespace

// One launch table for both scalar types: `val` / `sval` are the operand's values and those of its sliced-ELL copy in T
template <class T>
static void spmm_launch_t(hipStream_t st, const MausCsr& m, const T* val, const T* sval, int sched, const T* B, long ldb, T* C, long ldc,
                          const int* a_rows, const int* c_rows, int count) {
    if (count <= 0 || m.rows <= 0) return;
    const int groups = (count + SP_CG - 1) / SP_CG;
    const MausSell& s = m.sell;
    const dim3 rows_grid((m.rows + SP_BT - 1) / SP_BT, groups);
    if (SELL_G1 && sval && count == 1)                  // the copy exists only under the lane-per-row schedule of the matrix (spmm_kind)
        hipLaunchKernelGGL((spmm_sell_kernel<T, 1, SELL_U1>), rows_grid, dim3(SP_BT), 0, st,
                           s.off, s.len, s.idx, sval, m.rows, B, ldb, C, ldc, a_rows, c_rows, count);
    else if (sval && s.wmax < SELL_U)
        hipLaunchKernelGGL((spmm_sell_kernel<T, SP_CG, SELL_U_SHORT>), rows_grid, dim3(SP_BT), 0, st,
                           s.off, s.len, s.idx, sval, m.rows, B, ldb, C, ldc, a_rows, c_rows, count);
    else if (sval)
        hipLaunchKernelGGL((spmm_sell_kernel<T, SP_CG, SELL_U>), rows_grid, dim3(SP_BT), 0, st,
                           s.off, s.len, s.idx, sval, m.rows, B, ldb, C, ldc, a_rows, c_rows, count);
    else if (sched == MAUS_SPMM_WAVE)
        hipLaunchKernelGGL(spmm_wave_kernel<T>, dim3((m.rows + SP_BT / MAUS_WAVE - 1) / (SP_BT / MAUS_WAVE), groups), dim3(SP_BT), 0, st,
                           m.ptr, m.idx, val, m.rows, B, ldb, C, ldc, a_rows, c_rows, count);
    else
        hipLaunchKernelGGL(spmm_rows_kernel<T>, dim3((m.rows + SP_BT - 1) / SP_BT, groups), dim3(SP_BT), 0, st,
                           m.ptr, m.idx, val, m.rows, B, ldb, C, ldc, a_rows, c_rows, count);
}

void maus_spmm_launch(hipStream_t st, const MausCsr& m, int sched, const c128* B, long ldb, c128* C, long ldc,
                      const int* a_rows, const int* c_rows, int count) {
    spmm_launch_t<c128>(st, m, m.val, m.sell.val, sched, B, ldb, C, ldc, a_rows, c_rows, count);
}

// the real path: the operand's real copy (m.rval; m.sell.rval where the complex operand runs the sliced-ELL kernel) times rows
// of doubles -- the kernel, geometry and row lists that maus_spmm_launch picks for the same operand
void maus_spmm_launch_real(hipStream_t st, const MausCsr& m, int sched, const double* B, long ldb, double* C, long ldc,
                           const int* a_rows, const int* c_rows, int count) {
    spmm_launch_t<double>(st, m, m.rval, m.sell.val ? m.sell.rval : nullptr, sched, B, ldb, C, ldc, a_rows, c_rows, count);
}

void maus_csr_diag_launch(hipStream_t st, const MausCsr& m, int n, c128* d) {
    hipLaunchKernelGGL(csr_diag_kernel<c128>, dim3((n + SP_BT - 1) / SP_BT), dim3(SP_BT), 0, st, m.ptr, m.idx, m.val, n, d);
}

bool maus_real_flagged(const double* v, size_t count) {
    for (size_t i = 0; i < count; ++i) {
        uint64_t bits;
        memcpy(&bits, &v[2 * i + 1], sizeof bits);
        if (bits << 1) return false;            // anything but +0 / -0: a denormal, a NaN, a number
    }
    return true;
}

static int real_alloc(maus_ctx* c, double** p, size_t count) {
    HIPCHK(c, hipMalloc((void**)p, sizeof(double) * std::max<size_t>(1, count)));
    c->real_allocs += 1;
    return 0;
}
static void real_release(double*& p) { if (p) { (void)hipFree(p); p = nullptr; } }

// The operand's real copies: the CSR values (indices shared with the complex CSR), their sliced-ELL copy where the complex
// operand has one (the fill step of the build above on the real values; widths and offsets are the complex copy's), and the
// diagonal.  They exist only while the rule can hold for the bound matrix: method 1, a square CSR matrix flagged real.
int maus_real_sync_matrix(maus_ctx* c) {
    MausCsr& m = c->Acsr;
    if (!(c->real_method == 1 && c->csr && c->A_real && c->rows == c->cols)) {
        real_release(m.rval); real_release(m.sell.rval); real_release(c->Adiag_r);
        return 0;
    }
    const int n = c->rows;
    if (!m.rval) {
        if (real_alloc(c, &m.rval, (size_t)m.nnz)) return -1;
        if (m.nnz > 0)
            hipLaunchKernelGGL(real_part_kernel, dim3((unsigned)((m.nnz + SP_BT - 1) / SP_BT)), dim3(SP_BT), 0, c->st, m.val, m.rval, m.nnz);
    }
    if (!c->Adiag_r) {
        if (real_alloc(c, &c->Adiag_r, (size_t)n)) return -1;
        hipLaunchKernelGGL(csr_diag_kernel<double>, dim3((n + SP_BT - 1) / SP_BT), dim3(SP_BT), 0, c->st, m.ptr, m.idx, m.rval, n, c->Adiag_r);
    }
    if (!m.sell.val) real_release(m.sell.rval);
    else if (!m.sell.rval) {
        const MausSell& s = m.sell;
        if (real_alloc(c, &m.sell.rval, (size_t)s.padded)) return -1;
        hipLaunchKernelGGL(sell_fill_kernel<double>, dim3((s.slices * MAUS_WAVE + SP_BT - 1) / SP_BT), dim3(SP_BT), 0, c->st,
                           m.ptr, m.idx, m.rval, m.rows, s.slices, s.off, (int*)nullptr, m.sell.rval);
    }
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    return 0;
}

// The real copy of b, under method 1 for a b flagged real; refilled whenever b is set
int maus_real_sync_rhs(maus_ctx* c) {
    if (!(c->real_method == 1 && c->b && c->b_real)) { real_release(c->b_r); c->b_rn = 0; return 0; }
    if (c->b_rn != c->bn) { real_release(c->b_r); c->b_rn = 0; }
    if (!c->b_r) { if (real_alloc(c, &c->b_r, (size_t)c->bn)) return -1; c->b_rn = c->bn; }
    hipLaunchKernelGGL(real_part_kernel, dim3((c->bn + SP_BT - 1) / SP_BT), dim3(SP_BT), 0, c->st, c->b, c->b_r, (long)c->bn);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    return 0;
}

static void sell_free(MausSell& s) {
    if (s.val) (void)hipFree(s.val);
    if (s.rval) (void)hipFree(s.rval);
    if (s.idx) (void)hipFree(s.idx);
    if (s.len) (void)hipFree(s.len);
    if (s.off) (void)hipFree(s.off);
    s = MausSell();
}

void maus_csr_free(MausCsr& m) {
    sell_free(m.sell);
    if (m.ptr) (void)hipFree(m.ptr);
    if (m.idx) (void)hipFree(m.idx);
    if (m.val) (void)hipFree(m.val);
    if (m.rval) (void)hipFree(m.rval);
    m = MausCsr();
}

// nnz / rows above 32: a lane per row would walk a long row alone while its wave's other lanes wait on theirs
static int csr_schedule(int rows, long nnz) { return nnz > 32L * rows ? MAUS_SPMM_WAVE : MAUS_SPMM_ROWS; }

// Which kernel an operand runs, stated once (maus_spmm_plan / maus_spmm_kernel_for report it; tests ask them).  `sched` is the
// schedule of the bound MATRIX, from nnz and the rows of A: the CSR kernels run A and A^H under that one schedule, so it, and
// not the operand's own nnz / rows, decides whether the sliced-ELL kernel would give the CSR kernel's bits.  Under method 1 an
// operand of a lane-per-row matrix that stores something and whose padded size stays within the cap takes the copy.  The cap
// bounds memory (20 bytes per padded slot); it is not a tuned number.
constexpr int SELL_FILL_CAP = 200, SELL_CAP_MIN = 100, SELL_CAP_MAX = 1000000;
enum { MAUS_SPMM_SELL = 3 };
static bool spmm_setting_ok(int method, int cap) {
    return (method == 0 || method == 1) && (cap == 0 || (cap >= SELL_CAP_MIN && cap <= SELL_CAP_MAX));
}
static int spmm_kind(int method, int cap, int sched, long nnz, long padded) {
    if (method != 1 || sched != MAUS_SPMM_ROWS || nnz <= 0) return sched;
    // padded <= 64 * cols * slices < 2^53 and cap * nnz < 2^51: exact in double
    return 100.0 * (double)padded <= (double)(cap ? cap : SELL_FILL_CAP) * (double)nnz ? MAUS_SPMM_SELL : sched;
}

// The sliced-ELL copy of one bound operand under the context's method: slice widths on the device, their scan on the host
// (rows / 64 integers down and up), the fill on the device.  Leaves m.sell empty where the rule keeps the operand on CSR.
static int sell_build_into(maus_ctx* c, const MausCsr& m, MausSell& s, int*& d_width) {
    const int ns = (m.rows + MAUS_WAVE - 1) / MAUS_WAVE, blocks = (ns * MAUS_WAVE + SP_BT - 1) / SP_BT;
    HIPCHK(c, hipMalloc((void**)&s.len, sizeof(int) * m.rows));
    HIPCHK(c, hipMalloc((void**)&d_width, sizeof(int) * ns));
    hipLaunchKernelGGL(sell_width_kernel, dim3(blocks), dim3(SP_BT), 0, c->st, m.ptr, m.rows, ns, s.len, d_width);
    std::vector<int> width(ns);
    if (maus_stage_d2h(c, width.data(), d_width, sizeof(int) * ns, c->st)) return -1;
    std::vector<long> off((size_t)ns + 1, 0);
    for (int i = 0; i < ns; ++i) off[i + 1] = off[i] + (long)MAUS_WAVE * width[i];
    s.slices = ns; s.padded = off[ns]; s.wmax = *std::max_element(width.begin(), width.end());
    if (spmm_kind(c->spmm_method, c->spmm_fill_cap, c->csr_sched, m.nnz, s.padded) != MAUS_SPMM_SELL) return 1;
    HIPCHK(c, hipMalloc((void**)&s.off, sizeof(long) * (ns + 1)));
    HIPCHK(c, hipMalloc((void**)&s.idx, sizeof(int) * s.padded));
    HIPCHK(c, hipMalloc((void**)&s.val, sizeof(c128) * s.padded));
    if (maus_stage_h2d(c, s.off, off.data(), sizeof(long) * (ns + 1), c->st)) return -1;
    hipLaunchKernelGGL(sell_fill_kernel<c128>, dim3(blocks), dim3(SP_BT), 0, c->st, m.ptr, m.idx, m.val, m.rows, ns, s.off, s.idx, s.val);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    return 0;
}

static int sell_build(maus_ctx* c, MausCsr& m) {
    sell_free(m.sell);
    if (spmm_kind(c->spmm_method, c->spmm_fill_cap, c->csr_sched, m.nnz, 0) != MAUS_SPMM_SELL) return 0;   // no padded size passes
    MausSell s;
    int* d_width = nullptr;
    const int rc = sell_build_into(c, m, s, d_width);
    if (d_width) (void)hipFree(d_width);
    if (rc) { sell_free(s); return rc < 0 ? -1 : 0; }
    m.sell = s;
    return 0;
}

// Host-side checks of one CSR operand: indptr starts at 0, never decreases and ends at nnz; column indices lie in
// [0, cols) and increase strictly inside a row (sorted, no duplicates: the H build scatters one entry per position).
static const char* csr_check(int rows, int cols, long nnz, const int64_t* indptr, const int32_t* indices) {
    if (indptr[0] != 0) return "indptr[0] != 0";
    for (int i = 0; i < rows; ++i)                  // first the row pointers: the index loop below reads indices[indptr[i] ..)
        if (indptr[i + 1] < indptr[i]) return "indptr is not monotone";
    if (indptr[rows] != nnz) return "indptr[rows] != nnz";
    for (int i = 0; i < rows; ++i) {
        int prev = -1;
        for (int64_t p = indptr[i]; p < indptr[i + 1]; ++p) {
            const int j = indices[p];
            if (j < 0 || j >= cols) return "column index out of range";
            if (j <= prev) return "column indices of a row are not strictly increasing";
            prev = j;
        }
    }
    return nullptr;
}

static int csr_upload(maus_ctx* c, MausCsr& m, int rows, long nnz, const int64_t* indptr, const int32_t* indices, const double* values) {
    std::vector<int> p32(rows + 1);
    for (int i = 0; i <= rows; ++i) p32[i] = (int)indptr[i];
    HIPCHK(c, hipMalloc((void**)&m.ptr, sizeof(int) * (rows + 1)));
    HIPCHK(c, hipMalloc((void**)&m.idx, sizeof(int) * std::max(1L, nnz)));
    HIPCHK(c, hipMalloc((void**)&m.val, sizeof(c128) * std::max(1L, nnz)));
    m.rows = rows; m.nnz = nnz;
    if (maus_stage_h2d(c, m.ptr, p32.data(), sizeof(int) * (rows + 1), c->st)) return -1;
    if (nnz > 0) {
        if (maus_stage_h2d(c, m.idx, indices, sizeof(int) * nnz, c->st)) return -1;
        if (maus_stage_h2d(c, m.val, values, sizeof(c128) * nnz, c->st)) return -1;
    }
    return 0;
}

extern "C" {

int maus_set_matrix_csr(maus_ctx* c, int rows, int cols, int64_t nnz,
                        const int64_t* indptr, const int32_t* indices, const double* values_c128) {
    if (!c) return -1;
    if (rows <= 0 || cols <= 0 || nnz < 0 || nnz > INT32_MAX) FAIL(c, "maus_set_matrix_csr: bad sizes (rows, cols > 0, 0 <= nnz < 2^31)");
    if (!indptr || (nnz > 0 && (!indices || !values_c128))) FAIL(c, "maus_set_matrix_csr: null array");
    if (const char* e = csr_check(rows, cols, nnz, indptr, indices)) { c->err = std::string("maus_set_matrix_csr: ") + e; return -1; }
    // CSR of A^H by a counting sort over the columns: walking the rows of A in order leaves every row of A^H sorted
    std::vector<int64_t> hptr((size_t)cols + 1, 0);
    std::vector<int32_t> hidx((size_t)nnz);
    std::vector<double> hval(2 * (size_t)nnz);
    for (int64_t p = 0; p < nnz; ++p) hptr[(size_t)indices[p] + 1]++;
    for (int j = 0; j < cols; ++j) hptr[j + 1] += hptr[j];
    {
        std::vector<int64_t> next(hptr.begin(), hptr.end() - 1);
        for (int i = 0; i < rows; ++i)
            for (int64_t p = indptr[i]; p < indptr[i + 1]; ++p) {
                const int64_t q = next[indices[p]]++;
                hidx[q] = i;
                hval[2 * q] = values_c128[2 * p];
                hval[2 * q + 1] = -values_c128[2 * p + 1];
            }
    }
    // everything that belonged to the previous matrix goes (as maus_set_matrix); no dense copy is kept
    if (maus_matrix_reserve_csr(c, rows, cols)) return -1;
    if (csr_upload(c, c->Acsr, rows, nnz, indptr, indices, values_c128)) return -1;
    if (csr_upload(c, c->AHcsr, cols, nnz, hptr.data(), hidx.data(), hval.data())) return -1;
    c->csr_sched = csr_schedule(rows, nnz);
    if (rows == cols) {
        HIPCHK(c, hipMalloc((void**)&c->Adiag, sizeof(c128) * rows));
        maus_csr_diag_launch(c->st, c->Acsr, rows, c->Adiag);
    }
    c->csr = true;
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    if (sell_build(c, c->Acsr) || sell_build(c, c->AHcsr)) return -1;      // under maus_spmm_set_method(ctx, 1)
    c->A_real = maus_real_flagged(values_c128, (size_t)nnz);
    return maus_real_sync_matrix(c);                                       // under maus_real_set_method(ctx, 1)
}

int maus_matrix_is_sparse(maus_ctx* c) {
    if (!c) return -1;
    return c->csr ? c->csr_sched : 0;
}

int maus_spmm_set_method(maus_ctx* c, int method, int fill_cap_percent) {
    if (!c) return -1;
    if (!spmm_setting_ok(method, fill_cap_percent))
        FAIL(c, "maus_spmm_set_method: method must be 0 (CSR) or 1 (sliced ELL), fill_cap_percent 0 (the rule's 200) or 100..1000000");
    if (method == c->spmm_method && fill_cap_percent == c->spmm_fill_cap) return 0;
    if (!c->csr) { c->spmm_method = method; c->spmm_fill_cap = fill_cap_percent; return 0; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->st));                   // products in flight still read the copies
    const int old_method = c->spmm_method, old_cap = c->spmm_fill_cap;
    c->spmm_method = method; c->spmm_fill_cap = fill_cap_percent;
    if (sell_build(c, c->Acsr) || sell_build(c, c->AHcsr)) {
        // a failed build (device memory) leaves the previous setting: its copies are built again, and where that fails too the
        // operands run the CSR kernels, which give the same bits
        const std::string why = c->err;
        c->spmm_method = old_method; c->spmm_fill_cap = old_cap;
        if (sell_build(c, c->Acsr) || sell_build(c, c->AHcsr)) { sell_free(c->Acsr.sell); sell_free(c->AHcsr.sell); }
        c->err = why;
        (void)maus_real_sync_matrix(c);
        c->err = why;
        return -1;
    }
    return maus_real_sync_matrix(c);            // the real sliced-ELL values follow the copy they mirror
}

int maus_spmm_get_method(maus_ctx* c) { return c ? c->spmm_method : -1; }

int maus_real_set_method(maus_ctx* c, int method) {
    if (!c) return -1;
    if (method != 0 && method != 1) FAIL(c, "maus_real_set_method: method must be 0 (complex arithmetic) or 1 (real arithmetic where the rule holds)");
    if (method == c->real_method) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->st));
    const int old = c->real_method;
    c->real_method = method;
    if (maus_real_sync_matrix(c) || maus_real_sync_rhs(c)) {
        const std::string why = c->err;                        // device memory: back to the previous method, whose copies are smaller or none
        c->real_method = old;
        (void)maus_real_sync_matrix(c); (void)maus_real_sync_rhs(c);
        c->err = why;
        return -1;
    }
    return 0;
}

int maus_real_get_method(maus_ctx* c) { return c ? c->real_method : -1; }

int maus_real_values_flagged(const double* values_c128, int64_t count) {
    if (count < 0 || (count > 0 && !values_c128)) return -1;
    return maus_real_flagged(values_c128, (size_t)count) ? 1 : 0;
}

int maus_real_spmm(maus_ctx* c, const int* slots, int count) {
    if (!c) return -1;
    if (!c->csr || !c->Acsr.rval || !c->X) FAIL(c, "maus_real_spmm: needs method 1, a real square CSR matrix and a population");
    if (count < 0 || (count > 0 && !slots)) FAIL(c, "maus_real_spmm: bad arguments");
    if (count == 0) return 0;
    maus_av_drop_all(c);
    if (upload_slots(c, slots, count)) return -1;
    const int n = c->rows;
    const size_t rows = (sizeof(double) * (size_t)count * n + 255) / 256 * 256;
    if (ensure_scratch(c, 2 * rows + sizeof(int) * count)) return -1;
    double* R = (double*)c->scratch; double* Q = (double*)((char*)c->scratch + rows); int* ident = (int*)((char*)c->scratch + 2 * rows);
    const dim3 grid((n + SP_BT - 1) / SP_BT, count);
    hipLaunchKernelGGL(real_rows_in_kernel, grid, dim3(SP_BT), 0, c->st, c->X, c->ldp, c->d_slots, n, R, ident);
    { ProfScope ps(c, KC_SPMM_REAL, 2.0 * count * c->Acsr.nnz, maus_spmm_operand_bytes_real(c->Acsr) * ((count + 7) / 8) + 16.0 * count * n);
      maus_spmm_launch_real(c->st, c->Acsr, c->csr_sched, R, n, Q, n, ident, ident, count); }
    hipLaunchKernelGGL(real_rows_out_kernel, grid, dim3(SP_BT), 0, c->st, Q, n, c->d_slots, c->Y, c->ldp);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    return 0;
}

int maus_spmm_plan(int method, int fill_cap_percent, int rows, int64_t nnz, int64_t padded, int* kind_out) {
    if (!spmm_setting_ok(method, fill_cap_percent) || rows < 1 || nnz < 0 || padded < 0) return -1;
    if (kind_out) *kind_out = spmm_kind(method, fill_cap_percent, csr_schedule(rows, (long)nnz), (long)nnz, (long)padded);
    return 0;
}

int maus_spmm_kernel_for(maus_ctx* c, int adjoint) {
    if (!c) return -1;
    if (!c->csr) return 0;
    return (adjoint ? c->AHcsr : c->Acsr).sell.val ? MAUS_SPMM_SELL : c->csr_sched;
}

int maus_spmm_sell_info(maus_ctx* c, int adjoint, int* slices, int64_t* padded, int64_t* bytes) {
    if (!c) return -1;
    const MausCsr& m = adjoint ? c->AHcsr : c->Acsr;
    const MausSell& s = m.sell;
    const bool on = c->csr && s.val;
    if (slices) *slices = on ? s.slices : 0;
    if (padded) *padded = on ? s.padded : 0;
    if (bytes) *bytes = on ? (int64_t)(20 * s.padded + (long)sizeof(int) * m.rows + (long)sizeof(long) * (s.slices + 1)) : 0;
    return 0;
}

}  // extern "C"
