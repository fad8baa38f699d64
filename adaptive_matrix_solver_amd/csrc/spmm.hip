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
#include "ctx.h"

namespace {

constexpr int SP_CG = 8;          // candidates per thread: each nonzero (16 B value + 4 B index) is loaded once per 8 candidates
constexpr int SP_BT = 256;        // threads per block

// short rows (banded operators, up to ~32 nonzeros per row): one lane per row, so consecutive lanes gather neighbouring x[col]
__global__ void __launch_bounds__(SP_BT)
spmm_rows_kernel(const int* __restrict__ ptr, const int* __restrict__ idx, const c128* __restrict__ val, int nrows,
                 const c128* __restrict__ B, long ldb, c128* __restrict__ C, long ldc,
                 const int* __restrict__ a_rows, const int* __restrict__ c_rows, int count)
{
    const int i = blockIdx.x * SP_BT + threadIdx.x;
    const int k0 = blockIdx.y * SP_CG;
    if (i >= nrows) return;
    const int ng = min(SP_CG, count - k0);
    const c128* b[SP_CG];
    c128 acc[SP_CG];
#pragma unroll
    for (int g = 0; g < SP_CG; ++g) {
        b[g] = B + (long)a_rows[k0 + (g < ng ? g : 0)] * ldb;
        acc[g] = cmake(0.0, 0.0);
    }
    const int p1 = ptr[i + 1];
    for (int p = ptr[i]; p < p1; ++p) {
        const c128 a = val[p];
        const int j = idx[p];
#pragma unroll
        for (int g = 0; g < SP_CG; ++g)
            if (g < ng) cfma(acc[g], a, b[g][j]);
    }
#pragma unroll
    for (int g = 0; g < SP_CG; ++g)
        if (g < ng) C[(long)c_rows[k0 + g] * ldc + i] = acc[g];
}

// long rows: one wave per row, lanes over the row's nonzeros, the partial sums joined by a fixed tree
__global__ void __launch_bounds__(SP_BT)
spmm_wave_kernel(const int* __restrict__ ptr, const int* __restrict__ idx, const c128* __restrict__ val, int nrows,
                 const c128* __restrict__ B, long ldb, c128* __restrict__ C, long ldc,
                 const int* __restrict__ a_rows, const int* __restrict__ c_rows, int count)
{
    const int lane = threadIdx.x & (MAUS_WAVE - 1);
    const int i = blockIdx.x * (SP_BT / MAUS_WAVE) + threadIdx.x / MAUS_WAVE;
    const int k0 = blockIdx.y * SP_CG;
    if (i >= nrows) return;                       // whole waves leave together (i is uniform per wave)
    const int ng = min(SP_CG, count - k0);
    const c128* b[SP_CG];
    c128 acc[SP_CG];
#pragma unroll
    for (int g = 0; g < SP_CG; ++g) {
        b[g] = B + (long)a_rows[k0 + (g < ng ? g : 0)] * ldb;
        acc[g] = cmake(0.0, 0.0);
    }
    const int p1 = ptr[i + 1];
    for (int p = ptr[i] + lane; p < p1; p += MAUS_WAVE) {
        const c128 a = val[p];
        const int j = idx[p];
#pragma unroll
        for (int g = 0; g < SP_CG; ++g)
            if (g < ng) cfma(acc[g], a, b[g][j]);
    }
#pragma unroll
    for (int g = 0; g < SP_CG; ++g) {
        if (g >= ng) break;                       // ng is uniform per wave
        const double re = wave_sum_dpp(acc[g].x), im = wave_sum_dpp(acc[g].y);
        if (lane == 0) C[(long)c_rows[k0 + g] * ldc + i] = cmake(re, im);
    }
}

// d[i] = A[i][i] (0 where the row stores no diagonal entry)
__global__ void __launch_bounds__(SP_BT)
csr_diag_kernel(const int* __restrict__ ptr, const int* __restrict__ idx, const c128* __restrict__ val, int n, c128* __restrict__ d)
{
    const int i = blockIdx.x * SP_BT + threadIdx.x;
    if (i >= n) return;
    c128 v = cmake(0.0, 0.0);
    for (int p = ptr[i]; p < ptr[i + 1]; ++p)
        if (idx[p] == i) { v = val[p]; break; }
    d[i] = v;
}

}  // namespace

void maus_spmm_launch(hipStream_t st, const MausCsr& m, int sched, const c128* B, long ldb, c128* C, long ldc,
                      const int* a_rows, const int* c_rows, int count) {
    if (count <= 0 || m.rows <= 0) return;
    const int groups = (count + SP_CG - 1) / SP_CG;
    if (sched == MAUS_SPMM_WAVE)
        hipLaunchKernelGGL(spmm_wave_kernel, dim3((m.rows + SP_BT / MAUS_WAVE - 1) / (SP_BT / MAUS_WAVE), groups), dim3(SP_BT), 0, st,
                           m.ptr, m.idx, m.val, m.rows, B, ldb, C, ldc, a_rows, c_rows, count);
    else
        hipLaunchKernelGGL(spmm_rows_kernel, dim3((m.rows + SP_BT - 1) / SP_BT, groups), dim3(SP_BT), 0, st,
                           m.ptr, m.idx, m.val, m.rows, B, ldb, C, ldc, a_rows, c_rows, count);
}

void maus_csr_diag_launch(hipStream_t st, const MausCsr& m, int n, c128* d) {
    hipLaunchKernelGGL(csr_diag_kernel, dim3((n + SP_BT - 1) / SP_BT), dim3(SP_BT), 0, st, m.ptr, m.idx, m.val, n, d);
}

void maus_csr_free(MausCsr& m) {
    if (m.ptr) (void)hipFree(m.ptr);
    if (m.idx) (void)hipFree(m.idx);
    if (m.val) (void)hipFree(m.val);
    m = MausCsr();
}

// nnz / rows above 32: a lane per row would walk a long row alone while its wave's other lanes wait on theirs
static int csr_schedule(int rows, long nnz) { return nnz > 32L * rows ? MAUS_SPMM_WAVE : MAUS_SPMM_ROWS; }

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
    return 0;
}

int maus_matrix_is_sparse(maus_ctx* c) {
    if (!c) return -1;
    return c->csr ? c->csr_sched : 0;
}

}  // extern "C"
