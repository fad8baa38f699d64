// Sparse Hermitian shortcut at any size (AMS:186-216, DESIGN §10 "Lanczos"): thick-restart Lanczos on the CSR matrix for the k
// eigenpairs of largest |lambda|.  The host (engine.py) solves the projected ncv x ncv problem once per restart and decides;
// everything of length n stays here.
//
// The basis is ncv + 1 rows of n complex entries (one row per vector, the layout of the GMRES bases, so the SpMM's row-index
// lists address it).  One step j, all on the stream:
//     row j+1 = A row j                                        the CSR product of spmm.hip, one row
//     h  = V_j^H w,  w -= V_j^T h      (rows 0..j)             classical Gram-Schmidt, twice
//     alpha_j = Re(h1[j] + h2[j]),  beta_j = ||w||,  row j+1 = w / beta_j
// A workgroup owns a stretch of LZ_SPAN entries of n, keeps its piece of w in registers and streams the j + 1 basis pieces past
// it: 2 (j + 1) + 2 row reads/writes per pass, about 4 (j + 1) 16 n bytes per step.  Every sum has one fixed order: 64 lanes on
// the DPP tree of wave_sum_dpp, the four waves of a workgroup in index order, the workgroups' partial sums strided over 256
// threads and joined the same way.  No atomics: a run is bit-reproducible.
//
// A step whose beta is not above the caller's breakdown threshold leaves a zero row (and zero rows behind it): the host sees
// the small beta in the one read-back per sweep and continues from a fresh vector (maus_lanczos_inject).
#include "ctx.h"

namespace {

constexpr int LZ_BT = 256;                 // threads per workgroup
constexpr int LZ_E = 2;                    // entries of w per thread
constexpr int LZ_SPAN = LZ_BT * LZ_E;      // entries of n per workgroup
constexpr int LZ_MAXV = 32;                // largest ncv (SciPy's rule gives 20 from n = 20 up)
constexpr int LZ_H = LZ_MAXV + 1;          // coefficients per pass
constexpr int LZ_MAXK = 8;                 // largest number of Ritz rows a candidate is matched against (k <= 6)
constexpr int LZ_MSPAN = 4096;             // entries of n per workgroup of the match

__device__ __forceinline__ double lz_block_sum(double v, double* sbuf) {
    v = wave_sum_dpp(v);
    if ((threadIdx.x & 63) == 0) sbuf[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = (sbuf[0] + sbuf[1]) + (sbuf[2] + sbuf[3]);
    __syncthreads();
    return s;
}

// part[blk][i] = sum over the workgroup's stretch of conj(B[i][x]) w[x], i < cnt
__global__ void __launch_bounds__(LZ_BT)
lz_dots_kernel(const c128* __restrict__ B, long ld, int n, int cnt, const c128* __restrict__ w, c128* __restrict__ part)
{
    __shared__ c128 sred[LZ_H][LZ_BT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long x0 = (long)blockIdx.x * LZ_SPAN + threadIdx.x;
    c128 wr[LZ_E];
#pragma unroll
    for (int e = 0; e < LZ_E; ++e) { const long x = x0 + e * LZ_BT; wr[e] = x < n ? w[x] : cmake(0.0, 0.0); }
    for (int i = 0; i < cnt; ++i) {
        const c128* v = B + (long)i * ld;
        c128 acc = cmake(0.0, 0.0);
#pragma unroll
        for (int e = 0; e < LZ_E; ++e) { const long x = x0 + e * LZ_BT; if (x < n) cfma_conj(acc, v[x], wr[e]); }
        const double re = wave_sum_dpp(acc.x), im = wave_sum_dpp(acc.y);
        if (lane == 0) sred[i][wave] = cmake(re, im);
    }
    __syncthreads();
    if (threadIdx.x < cnt) {
        c128 s = sred[threadIdx.x][0];
#pragma unroll
        for (int k = 1; k < LZ_BT / 64; ++k) s = cadd(s, sred[threadIdx.x][k]);
        part[(long)blockIdx.x * LZ_H + threadIdx.x] = s;
    }
}

// h[i] = sum_blk part[blk][i]: workgroup i, thread t adds blk = t, t + 256, ... in that order, then the fixed tree
__global__ void __launch_bounds__(LZ_BT)
lz_reduce_kernel(const c128* __restrict__ part, int nblk, c128* __restrict__ h)
{
    __shared__ double sbuf[LZ_BT / 64];
    const int i = blockIdx.x;
    c128 acc = cmake(0.0, 0.0);
    for (int b = threadIdx.x; b < nblk; b += LZ_BT) acc = cadd(acc, part[(long)b * LZ_H + i]);
    const double re = lz_block_sum(acc.x, sbuf), im = lz_block_sum(acc.y, sbuf);
    if (threadIdx.x == 0) h[i] = cmake(re, im);
}

// w -= sum_{i < cnt} h[i] B[i]; npart[blk] = the stretch's share of ||w||^2 afterwards (npart may be null)
__global__ void __launch_bounds__(LZ_BT)
lz_update_kernel(const c128* __restrict__ B, long ld, int n, int cnt, c128* __restrict__ w, const c128* __restrict__ h,
                 double* __restrict__ npart)
{
    __shared__ double sbuf[LZ_BT / 64];
    const long x0 = (long)blockIdx.x * LZ_SPAN + threadIdx.x;
    c128 wr[LZ_E];
#pragma unroll
    for (int e = 0; e < LZ_E; ++e) { const long x = x0 + e * LZ_BT; wr[e] = x < n ? w[x] : cmake(0.0, 0.0); }
#pragma unroll 4
    for (int i = 0; i < cnt; ++i) {
        const c128* v = B + (long)i * ld;
        const c128 hi = h[i];
#pragma unroll
        for (int e = 0; e < LZ_E; ++e) { const long x = x0 + e * LZ_BT; if (x < n) cfms(wr[e], hi, v[x]); }
    }
    double ss = 0.0;
#pragma unroll
    for (int e = 0; e < LZ_E; ++e) {
        const long x = x0 + e * LZ_BT;
        if (x < n) { if (cnt > 0) w[x] = wr[e]; ss = fma(wr[e].x, wr[e].x, ss); ss = fma(wr[e].y, wr[e].y, ss); }
    }
    if (npart) {                                            // uniform per launch
        ss = lz_block_sum(ss, sbuf);
        if (threadIdx.x == 0) npart[blockIdx.x] = ss;
    }
}

// beta = sqrt(sum_blk npart[blk]); ab[j] = Re(h1[j] + h2[j]), ab[LZ_H + j] = beta (j >= 0); inv = 1 / beta where beta is above
// tol_abs, else 0: a broken-down (or non-finite) step leaves a zero row instead of amplified rounding noise
__global__ void __launch_bounds__(LZ_BT)
lz_final_kernel(const double* __restrict__ npart, int nblk, const c128* __restrict__ h, int j, double tol_abs,
                double* __restrict__ ab, double* __restrict__ inv)
{
    __shared__ double sbuf[LZ_BT / 64];
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblk; b += LZ_BT) acc += npart[b];
    acc = lz_block_sum(acc, sbuf);
    if (threadIdx.x == 0) {
        const double beta = sqrt(acc);
        if (j >= 0) { ab[j] = h[j].x + h[LZ_H + j].x; ab[LZ_H + j] = beta; }
        *inv = (beta > tol_abs) ? 1.0 / beta : 0.0;
    }
}

__global__ void __launch_bounds__(LZ_BT)
lz_scale_kernel(c128* __restrict__ w, int n, const double* __restrict__ inv)
{
    const long x = (long)blockIdx.x * LZ_BT + threadIdx.x;
    if (x >= n) return;
    const double s = *inv;
    const c128 a = w[x];
    w[x] = s == 0.0 ? cmake(0.0, 0.0) : cmake(a.x * s, a.y * s);
}

// out[i] = sum_{r < m} S[r][i] B[r], i < keep (S real, m x keep row-major), and, with copy_row, out[keep] = B[m].  A thread owns
// one entry of n and reads its whole column of the basis before it writes, so out may be the basis itself (the restart).
__global__ void __launch_bounds__(LZ_BT)
lz_combine_kernel(const c128* B, long ld, int n, int m, int keep, const double* __restrict__ S, c128* out, long ldo, int copy_row)
{
    __shared__ double sS[LZ_MAXV * LZ_MAXV];
    for (int t = threadIdx.x; t < m * keep; t += LZ_BT) sS[t] = S[t];
    __syncthreads();
    const long x = (long)blockIdx.x * LZ_BT + threadIdx.x;
    if (x >= n) return;
    c128 v[LZ_MAXV];
#pragma unroll
    for (int r = 0; r < LZ_MAXV; ++r) v[r] = r < m ? B[(long)r * ld + x] : cmake(0.0, 0.0);
    const c128 last = copy_row ? B[(long)m * ld + x] : cmake(0.0, 0.0);
    for (int i = 0; i < keep; ++i) {
        c128 acc = cmake(0.0, 0.0);
#pragma unroll
        for (int r = 0; r < LZ_MAXV; ++r)
            if (r < m) { const double s = sS[r * keep + i]; acc.x = fma(s, v[r].x, acc.x); acc.y = fma(s, v[r].y, acc.y); }
        out[(long)i * ldo + x] = acc;
    }
    if (copy_row) out[(long)keep * ldo + x] = last;
}

// np.argmax's order on |score| (popops.hip: herm_better): NaN before any number, then the larger value, then the smaller index
__device__ __forceinline__ bool lz_better(double v, int j, double best, int bidx) {
    const bool vn = v != v, bn = best != best;
    if (vn || bn) return vn && (!bn || j < bidx);
    return v > best || (v == best && j < bidx);
}

// AMS:197-202 in three kernels, n split over workgroups of LZ_MSPAN entries so that a handful of candidates fills the device.
// (1) workgroup (blk, g): its stretch's share of the k scores vdot(x_g, R[j]) and of the k squared norms ||R[j]||^2
__global__ void __launch_bounds__(LZ_BT)
lz_match_partial_kernel(const c128* __restrict__ R, long ldr, int k, int n, const c128* __restrict__ X, long ldx,
                        const int* __restrict__ slots, c128* __restrict__ spart, double* __restrict__ npart)
{
    __shared__ double sbuf[LZ_BT / 64];
    const c128* x = X + (long)slots[blockIdx.y] * ldx;
    const long lo = (long)blockIdx.x * LZ_MSPAN;
    const long hi = lo + LZ_MSPAN < n ? lo + LZ_MSPAN : n;
    c128 acc[LZ_MAXK];
    double nn[LZ_MAXK];
#pragma unroll
    for (int j = 0; j < LZ_MAXK; ++j) { acc[j] = cmake(0.0, 0.0); nn[j] = 0.0; }
    for (long i = lo + threadIdx.x; i < hi; i += LZ_BT) {
        const c128 xv = x[i];
#pragma unroll
        for (int j = 0; j < LZ_MAXK; ++j)
            if (j < k) { const c128 r = R[(long)j * ldr + i]; cfma_conj(acc[j], xv, r); nn[j] = fma(r.x, r.x, nn[j]); nn[j] = fma(r.y, r.y, nn[j]); }
    }
    const long o = ((long)blockIdx.y * gridDim.x + blockIdx.x) * LZ_MAXK;
#pragma unroll
    for (int j = 0; j < LZ_MAXK; ++j) {
        if (j >= k) break;                                  // k is uniform
        const double re = lz_block_sum(acc[j].x, sbuf), im = lz_block_sum(acc[j].y, sbuf), q = lz_block_sum(nn[j], sbuf);
        if (threadIdx.x == 0) { spart[o + j] = cmake(re, im); npart[o + j] = q; }
    }
}

// (2) workgroup g: the partial sums joined in one fixed order (thread t adds blk = t, t + 256, ..., then the tree); the first
// largest |score|; idx_out[g] = its row, norm_out[g] = that row's norm
__global__ void __launch_bounds__(LZ_BT)
lz_match_pick_kernel(const c128* __restrict__ spart, const double* __restrict__ npart, int nblk, int k,
                     int* __restrict__ idx_out, double* __restrict__ norm_out)
{
    __shared__ double sbuf[LZ_BT / 64];
    const long o = (long)blockIdx.x * nblk * LZ_MAXK;
    double best = -1.0, bnorm = 0.0; int bidx = 0x7fffffff;
    for (int j = 0; j < k; ++j) {
        double re = 0.0, im = 0.0, q = 0.0;
        for (int b = threadIdx.x; b < nblk; b += LZ_BT) { const c128 s = spart[o + (long)b * LZ_MAXK + j]; re += s.x; im += s.y; q += npart[o + (long)b * LZ_MAXK + j]; }
        re = lz_block_sum(re, sbuf); im = lz_block_sum(im, sbuf); q = lz_block_sum(q, sbuf);
        const double v = hypot(re, im);
        if (lz_better(v, j, best, bidx)) { best = v; bidx = j; bnorm = sqrt(q); }
    }
    if (threadIdx.x == 0) { idx_out[blockIdx.x] = bidx; norm_out[blockIdx.x] = bnorm; }
}

// (3) X[slot_g] <- R[idx_g] / norm_g
__global__ void __launch_bounds__(LZ_BT)
lz_match_copy_kernel(const c128* __restrict__ R, long ldr, int n, c128* __restrict__ X, long ldx, const int* __restrict__ slots,
                     const int* __restrict__ idx, const double* __restrict__ nrm)
{
    const long i = (long)blockIdx.x * LZ_BT + threadIdx.x;
    if (i >= n) return;
    const c128 a = R[(long)idx[blockIdx.y] * ldr + i];
    const double inv = 1.0 / nrm[blockIdx.y];
    X[(long)slots[blockIdx.y] * ldx + i] = cmake(a.x * inv, a.y * inv);
}

__global__ void lz_iota_kernel(int* p, int count) { const int i = blockIdx.x * blockDim.x + threadIdx.x; if (i < count) p[i] = i; }

void lz_free_basis(MausLanczos& z) {
    void** ps[] = {(void**)&z.B, (void**)&z.part, (void**)&z.h, (void**)&z.npart, (void**)&z.ab, (void**)&z.S, (void**)&z.ident};
    for (auto p : ps) if (*p) { (void)hipFree(*p); *p = nullptr; }
    z.ncv = 0; z.nblk = 0;
}

// classical Gram-Schmidt, twice, of row `wrow` of `base` against its rows 0 .. cnt - 1, then the norm, (alpha_j, beta_j) for
// j >= 0, and the scaling
void lz_orthonormalise(maus_ctx* c, c128* base, int wrow, int cnt, int j, double tol_abs) {
    MausLanczos& z = c->lz;
    const int n = z.n;
    c128* w = base + (long)wrow * n;
    ProfScope ps(c, KC_LANCZOS, 32.0 * cnt * n, (4.0 * cnt + 8.0) * 16.0 * n);
    for (int pass = 0; pass < 2; ++pass) {
        c128* h = z.h + pass * LZ_H;
        if (cnt > 0) {
            hipLaunchKernelGGL(lz_dots_kernel, dim3(z.nblk), dim3(LZ_BT), 0, c->st, base, (long)n, n, cnt, w, z.part);
            hipLaunchKernelGGL(lz_reduce_kernel, dim3(cnt), dim3(LZ_BT), 0, c->st, z.part, z.nblk, h);
        }
        if (cnt > 0 || pass == 1)
            hipLaunchKernelGGL(lz_update_kernel, dim3(z.nblk), dim3(LZ_BT), 0, c->st, base, (long)n, n, cnt, w, h, pass == 1 ? z.npart : nullptr);
    }
    hipLaunchKernelGGL(lz_final_kernel, dim3(1), dim3(LZ_BT), 0, c->st, z.npart, z.nblk, z.h, j, tol_abs, z.ab, z.ab + 2 * LZ_H);
    hipLaunchKernelGGL(lz_scale_kernel, dim3((n + LZ_BT - 1) / LZ_BT), dim3(LZ_BT), 0, c->st, w, n, z.ab + 2 * LZ_H);
}

const char* lz_no_matrix(const maus_ctx* c) {
    if (!c->csr) return "no CSR matrix is bound (maus_set_matrix_csr)";
    if (c->rows != c->cols) return "the matrix is not square";
    return nullptr;
}

}  // namespace

void maus_lanczos_drop(maus_ctx* c) {
    lz_free_basis(c->lz);
    if (c->lz.R) { (void)hipFree(c->lz.R); c->lz.R = nullptr; }
    c->lz.k = 0; c->lz.n = 0;
}

#define LZ_NEED_MATRIX(c, who) do { if (const char* e_ = lz_no_matrix(c)) { (c)->err = std::string(who ": ") + e_; return -1; } } while (0)
#define LZ_NEED_BASIS(c, who) do { LZ_NEED_MATRIX(c, who); if (!(c)->lz.B || (c)->lz.n != (c)->rows) FAIL(c, who ": no Lanczos basis (maus_lanczos_begin)"); } while (0)

extern "C" {

int maus_lanczos_inject(maus_ctx* c, int j, const double* v_c128) {
    if (!c) return -1;
    LZ_NEED_BASIS(c, "maus_lanczos_inject");
    MausLanczos& z = c->lz;
    if (j < 0 || j > z.ncv || !v_c128) FAIL(c, "maus_lanczos_inject: bad arguments");
    if (maus_stage_h2d(c, z.B + (long)j * z.n, v_c128, sizeof(c128) * (size_t)z.n, c->st)) return -1;
    lz_orthonormalise(c, z.B, j, j, -1, 0.0);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    return 0;
}

int maus_lanczos_begin(maus_ctx* c, const double* v0_c128, int ncv) {
    if (!c) return -1;
    LZ_NEED_MATRIX(c, "maus_lanczos_begin");
    const int n = c->rows;
    if (!v0_c128 || ncv < 1 || ncv > n || ncv > LZ_MAXV) FAIL(c, "maus_lanczos_begin: ncv must lie in [1, min(n, 32)]");
    HIPCHK(c, hipStreamSynchronize(c->st));
    maus_lanczos_drop(c);
    MausLanczos& z = c->lz;
    z.n = n; z.ncv = ncv; z.nblk = (n + LZ_SPAN - 1) / LZ_SPAN;
    HIPCHK(c, hipMalloc((void**)&z.B, sizeof(c128) * (size_t)(ncv + 1) * n));
    HIPCHK(c, hipMalloc((void**)&z.part, sizeof(c128) * (size_t)z.nblk * LZ_H));
    HIPCHK(c, hipMalloc((void**)&z.npart, sizeof(double) * (size_t)z.nblk));
    HIPCHK(c, hipMalloc((void**)&z.h, sizeof(c128) * 2 * LZ_H));
    HIPCHK(c, hipMalloc((void**)&z.ab, sizeof(double) * (2 * LZ_H + 1)));
    HIPCHK(c, hipMalloc((void**)&z.S, sizeof(double) * LZ_MAXV * LZ_MAXV));
    HIPCHK(c, hipMalloc((void**)&z.ident, sizeof(int) * (LZ_MAXV + 2)));
    hipLaunchKernelGGL(lz_iota_kernel, dim3(1), dim3(64), 0, c->st, z.ident, LZ_MAXV + 2);
    return maus_lanczos_inject(c, 0, v0_c128);
}

int maus_lanczos_extend(maus_ctx* c, int j0, int j1, double tol_abs, double* alpha_out, double* beta_out) {
    if (!c) return -1;
    LZ_NEED_BASIS(c, "maus_lanczos_extend");
    MausLanczos& z = c->lz;
    if (j0 < 0 || j0 >= j1 || j1 > z.ncv || !alpha_out || !beta_out || !(tol_abs >= 0.0)) FAIL(c, "maus_lanczos_extend: bad arguments");
    const int n = z.n;
    for (int j = j0; j < j1; ++j) {
        { ProfScope ps(c, KC_SPMM, 8.0 * c->Acsr.nnz, maus_spmm_operand_bytes(c->Acsr) + 32.0 * n);
          maus_spmm_launch(c->st, c->Acsr, c->csr_sched, z.B, (long)n, z.B, (long)n, z.ident + j, z.ident + j + 1, 1); }
        lz_orthonormalise(c, z.B, j + 1, j + 1, j, tol_abs);
    }
    if (maus_d2h(c, alpha_out, z.ab + j0, sizeof(double) * (j1 - j0), c->st)) return -1;
    if (maus_d2h(c, beta_out, z.ab + LZ_H + j0, sizeof(double) * (j1 - j0), c->st)) return -1;
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    return 0;
}

int maus_lanczos_restart(maus_ctx* c, const double* s_real, int m, int keep) {
    if (!c) return -1;
    LZ_NEED_BASIS(c, "maus_lanczos_restart");
    MausLanczos& z = c->lz;
    if (!s_real || m < 1 || m > z.ncv || keep < 1 || keep >= m) FAIL(c, "maus_lanczos_restart: need 1 <= keep < m <= ncv");
    if (maus_h2d(c, z.S, s_real, sizeof(double) * m * keep, c->st)) return -1;
    { ProfScope ps(c, KC_LANCZOS, 4.0 * m * keep * z.n, 16.0 * z.n * (m + keep + 2.0));
      hipLaunchKernelGGL(lz_combine_kernel, dim3((z.n + LZ_BT - 1) / LZ_BT), dim3(LZ_BT), 0, c->st, z.B, (long)z.n, z.n, m, keep, z.S, z.B, (long)z.n, 1); }
    // no synchronisation here: S left through the pinned ring, and the sweep that follows (maus_lanczos_extend) runs on the
    // same stream and ends in the one synchronisation of this restart
    HIPCHK(c, hipGetLastError());
    return 0;
}

int maus_lanczos_finish(maus_ctx* c, const double* s_real, int m, int k) {
    if (!c) return -1;
    LZ_NEED_BASIS(c, "maus_lanczos_finish");
    MausLanczos& z = c->lz;
    if (k == 0) {                                           // a run that did not converge: nothing is kept
        HIPCHK(c, hipStreamSynchronize(c->st));
        maus_lanczos_drop(c);
        return 0;
    }
    if (!s_real || m < 1 || m > z.ncv || k < 1 || k > m || k > LZ_MAXK) FAIL(c, "maus_lanczos_finish: need 1 <= k <= min(m, 8), m <= ncv");
    if (maus_h2d(c, z.S, s_real, sizeof(double) * m * k, c->st)) return -1;
    if (z.R) { HIPCHK(c, hipStreamSynchronize(c->st)); (void)hipFree(z.R); z.R = nullptr; }
    HIPCHK(c, hipMalloc((void**)&z.R, sizeof(c128) * (size_t)k * z.n));
    { ProfScope ps(c, KC_LANCZOS, 4.0 * m * k * z.n, 16.0 * z.n * (m + k));
      hipLaunchKernelGGL(lz_combine_kernel, dim3((z.n + LZ_BT - 1) / LZ_BT), dim3(LZ_BT), 0, c->st, z.B, (long)z.n, z.n, m, k, z.S, z.R, (long)z.n, 0); }
    // the kept vectors have been recombined once per restart and never against each other again: one more Gram-Schmidt sweep
    // over the k rows leaves them orthonormal to rounding (it moves a row by the few eps it had lost)
    for (int q = 0; q < k; ++q) lz_orthonormalise(c, z.R, q, q, -1, 0.0);
    z.k = k;
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    lz_free_basis(z);
    return 0;
}

int maus_herm_match_rows(maus_ctx* c, const int* slots, int count, int32_t* idx_out, double* norm_out) {
    if (!c) return -1;
    maus_av_drop_all(c);
    LZ_NEED_MATRIX(c, "maus_herm_match_rows");
    MausLanczos& z = c->lz;
    if (!z.R || z.n != c->rows || z.k < 1) FAIL(c, "maus_herm_match_rows: no Ritz rows (maus_lanczos_finish)");
    if (!c->X) FAIL(c, "maus_herm_match_rows: population missing");
    if (count == 0) return 0;
    if (upload_slots(c, slots, count)) return -1;
    const int n = z.n, nblk = (n + LZ_MSPAN - 1) / LZ_MSPAN;
    const int chunk = std::min(count, 32768);               // candidates per launch (the grid's second dimension)
    const size_t parts = (size_t)chunk * nblk * LZ_MAXK;
    if (ensure_scratch(c, parts * (sizeof(c128) + sizeof(double)))) return -1;
    c128* spart = (c128*)c->scratch; double* npart = (double*)(spart + parts);
    { ProfScope ps(c, KC_LANCZOS, 12.0 * count * z.k * n, 16.0 * count * n * (z.k + 3.0));
    for (int o = 0; o < count; o += chunk) {
        const int g = std::min(chunk, count - o);
        hipLaunchKernelGGL(lz_match_partial_kernel, dim3(nblk, g), dim3(LZ_BT), 0, c->st, z.R, (long)n, z.k, n, c->X, c->ldp, c->d_slots + o, spart, npart);
        hipLaunchKernelGGL(lz_match_pick_kernel, dim3(g), dim3(LZ_BT), 0, c->st, spart, npart, nblk, z.k, c->d_i1 + o, c->d_r1 + o);
        hipLaunchKernelGGL(lz_match_copy_kernel, dim3((n + LZ_BT - 1) / LZ_BT, g), dim3(LZ_BT), 0, c->st, z.R, (long)n, n, c->X, c->ldp, c->d_slots + o, c->d_i1 + o, c->d_r1 + o);
    } }
    if (maus_d2h(c, idx_out, c->d_i1, sizeof(int) * count, c->st)) return -1;
    if (maus_d2h(c, norm_out, c->d_r1, sizeof(double) * count, c->st)) return -1;
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    return 0;
}

int maus_get_ritz_rows(maus_ctx* c, double* rows_c128_out, int k, int n) {
    if (!c) return -1;
    MausLanczos& z = c->lz;
    if (!z.R || !rows_c128_out || k != z.k || n != z.n) FAIL(c, "maus_get_ritz_rows: no Ritz rows of that shape on the device");
    HIPCHK(c, hipStreamSynchronize(c->st));
    return maus_stage_d2h(c, rows_c128_out, z.R, sizeof(c128) * (size_t)k * n, c->st);
}

int maus_lanczos_get_basis(maus_ctx* c, int j0, int count, double* rows_c128_out) {
    if (!c) return -1;
    LZ_NEED_BASIS(c, "maus_lanczos_get_basis");
    MausLanczos& z = c->lz;
    if (j0 < 0 || count < 1 || count > z.ncv + 1 - j0 || !rows_c128_out) FAIL(c, "maus_lanczos_get_basis: need 0 <= j0, 1 <= count, j0 + count <= ncv + 1");
    HIPCHK(c, hipStreamSynchronize(c->st));
    return maus_stage_d2h(c, rows_c128_out, z.B + (long)j0 * z.n, sizeof(c128) * (size_t)count * z.n, c->st);
}

}  // extern "C"
