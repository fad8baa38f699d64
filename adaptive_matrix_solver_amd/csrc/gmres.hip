// Batched restarted GMRES with optional Jacobi (inverse-diagonal) left preconditioner (gfx950).
//
// Replaces, per candidate k, the reference's iterative branch (AMS:60-90):
//     spla.gmres(H_k, b, x0=b, tol=1e-8, maxiter=50, M=diag(1/diag(H_k)))   [tol -> rtol, SURVEY F2]
// whose algorithm is SciPy 1.15's scipy/sparse/linalg/_isolve/iterative.py:692-841: restart
// min(20, n), left preconditioning, modified Gram-Schmidt Arnoldi, Givens rotations in the
// LAPACK zlartg convention, adaptive inner tolerance `ptol`, true-residual exit
// ||b - H x|| <= rtol*||b||, info = maxiter when the restart cycles are exhausted.
//
// Shared-matrix mode (maus_gmres): H_k = A - shift_k I + psi_k I is never materialised: every inner iteration of ALL
// active candidates is ONE MFMA zgemm  Y = Z * A^T  (Z = the candidates' current Krylov vectors,
// gathered by row index) followed by a per-candidate kernel that adds (psi_k - shift_k) z,
// applies the Jacobi scale, orthogonalises (MGS, wavefront reductions), and runs the small
// Hessenberg / Givens / ptol state machine on one lane.  Each candidate advances through its
// own (cycle, column) state; the host only launches "ticks" until no candidate is active.
//
// Dense mode (maus_gmres_pert): the reference's H_solve of the GMRES branch also carries the random term
// 0.15 psi ((U1-.5) + i(U2-.5)) (AMS:49-52, 89).  At the default psi ~ 1e-19 that is below the rounding of one matvec
// and the shared-matrix mode is used; once psi has been escalated (attempt / stuck / aggression factors) it is not,
// and the candidates' H_k are materialised in the LU workspace (the same build kernels as the direct solve, i.e. the
// same bits as the reference's H_solve) -- the matvec is then one HBM-bound GEMV per candidate against its own H_k,
// and the Jacobi scale and its AMS:67-72 gate read diag(H_k) from the materialised matrix.
//
// The post step has two schedules for a CSR-bound matrix (maus_gmres_set_method): by default one workgroup per candidate
// (gmres_post_kernel with w in registers up to n = 16384, gmres_post_stream_kernel above); under method 1 the wide step further
// down (the gw_* kernels), which splits n over workgroups and joins every sum from per-piece partials in one fixed order.
// What the three schedules share is stated once: the rotation (zlartg), the decisions after a residual (resid_decide) and the
// one-lane Arnoldi tail (arnoldi_tail).  Their reductions are NOT shared: blk_sum and gw_block_sum / gw_join add in different
// orders, and each schedule's bits are those of its own order.  The vector bodies of the register and the streamed kernel are
// two texts on purpose (profiles/gmres_share.txt, section 5).
//
// Every kernel that touches a candidate's vectors is one text over their scalar type T: c128, or double on the real path
// (maus_real_set_method(ctx, 1)), which a maus_gmres call takes when maus_real_rule holds for it -- a CSR-bound matrix, the
// bound right-hand side and every shift of the call with imaginary parts of exactly +-0.  See "the scalar type T" below for
// why the two instantiations return the same bits, and for what differs on non-finite data.
#include "ctx.h"
#include <algorithm>
#include <cstring>

namespace {

constexpr int MAXR = 20;
constexpr int PAD_ROWS = 33;      // fewest rows for which the zgemm launcher picks the kernel family of a full population product
constexpr int GT = 256;
constexpr double EPS = 2.220446049250313e-16;

struct GState {
    int phase;        // 1: residual pending (z = x); 0: Arnoldi step pending (z = V[col]); 2: done
    int col, cycle, inner, info, breakdown, first, pad;
    double bnrm2, atol, ptol, pmf, presid, rnorm;
    double gc[MAXR];
    c128 gs[MAXR];
    c128 S[MAXR + 1];
    c128 h[MAXR][MAXR + 1];
};

template <int NT = GT>
__device__ __forceinline__ double blk_sum(double v, double* sbuf) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sbuf[wave] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) t += sbuf[w];
    return t;
}

// NumPy's complex reciprocal 1.0 / z  (Smith, as (1+0j)/z)
__device__ __forceinline__ c128 crecip_np(c128 z) {
    if (fabs(z.x) >= fabs(z.y)) {
        if (z.x == 0.0 && z.y == 0.0) return cmake(1.0 / fabs(z.x), 0.0 / fabs(z.y));   // inf, nan like NumPy
        const double rat = z.y / z.x, scl = 1.0 / (z.x + z.y * rat);
        return cmake(scl, -rat * scl);
    }
    const double rat = z.x / z.y, scl = 1.0 / (z.y + z.x * rat);
    return cmake(rat * scl, -scl);
}
__device__ __forceinline__ c128 cdiv_np(c128 a, c128 b) {
    if (fabs(b.x) >= fabs(b.y)) {
        const double rat = b.y / b.x, scl = 1.0 / (b.x + b.y * rat);
        return cmake((a.x + a.y * rat) * scl, (a.y - a.x * rat) * scl);
    }
    const double rat = b.x / b.y, scl = 1.0 / (b.y + b.x * rat);
    return cmake((a.x * rat + a.y) * scl, (a.y * rat - a.x) * scl);
}

// ---- the scalar type T of a solve's vectors: c128, or double on the real path (maus_real_set_method) ----
// The real path runs where the operand, b and every shift of the call have imaginary parts of exactly +-0; then so has every
// Krylov vector, every Hessenberg entry and the iterate of the complex solve.  Its kernels are the instantiation T = double of
// the texts below: rows of n doubles, and every vector operation the complex one with the terms that multiply an exact zero
// left out -- each of those adds +-0 to a sum and leaves it as it is -- in the same thread, the same order and through the same
// joins.  The helpers here state each such pair once.  Products and differences on the real side are single roundings by
// intrinsic, so that no contraction can fuse what the complex text rounds twice.  The one-lane state machine (zlartg,
// resid_decide, arnoldi_tail, GState) is NOT instantiated twice: both paths run the complex text on Hessenberg entries whose
// imaginary part is zero, so its decisions and rotations are the complex path's by construction (Smith's division by a real
// number is a multiplication by a reciprocal, which a real division would not reproduce).
// Non-finite data: 0 * Inf = NaN reaches the real part only through the terms left out, so the real path can hold Inf where the
// complex one holds NaN; what is finite or not, and with it info and status, is the same.
template <class T> __device__ __forceinline__ T sc_of(c128 z);                       // a Hessenberg-side scalar as T
template <> __device__ __forceinline__ c128 sc_of<c128>(c128 z) { return z; }
template <> __device__ __forceinline__ double sc_of<double>(c128 z) { return z.x; }
__device__ __forceinline__ c128 sc_c(c128 z) { return z; }                            // and back: imaginary part +0
__device__ __forceinline__ c128 sc_c(double r) { return cmake(r, 0.0); }
__device__ __forceinline__ void sc_abs2(double& s, c128 v) { s = fma(v.x, v.x, s); s = fma(v.y, v.y, s); }   // s += |v|^2
__device__ __forceinline__ void sc_abs2(double& s, double v) { s = fma(v, v, s); }
__device__ __forceinline__ c128 sc_scale(c128 v, double f) { return cmake(v.x * f, v.y * f); }
__device__ __forceinline__ double sc_scale(double v, double f) { return __dmul_rn(v, f); }
__device__ __forceinline__ c128 sc_sub(c128 a, c128 b) { return cmake(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double sc_sub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ c128 sc_add(c128 a, c128 b) { return cadd(a, b); }
__device__ __forceinline__ double sc_add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ bool sc_finite(c128 v) { return cfinite(v); }
__device__ __forceinline__ bool sc_finite(double v) { return isfinite(v); }
// psi - lambda, the shift behind the product
template <class T> __device__ __forceinline__ T sc_shift(double psi, c128 lam);
template <> __device__ __forceinline__ c128 sc_shift<c128>(double psi, c128 lam) { return cmake(psi - lam.x, -lam.y); }
template <> __device__ __forceinline__ double sc_shift<double>(double psi, c128 lam) { return __dsub_rn(psi, lam.x); }
// (1 / d) v, the Jacobi scale: crecip_np of a real d is 1 / d (1 / |d| for d = 0), its product with v one multiplication
__device__ __forceinline__ c128 sc_jacobi(c128 d, c128 v) { return cmul(crecip_np(d), v); }
__device__ __forceinline__ double sc_jacobi(double d, double v) { return __dmul_rn(d == 0.0 ? 1.0 / fabs(d) : 1.0 / d, v); }
// blk_sum of a T: the real part, then the imaginary part
template <int NT = GT> __device__ __forceinline__ c128 blk_sum_t(c128 v, double* sbuf) {
    const double re = blk_sum<NT>(v.x, sbuf), im = blk_sum<NT>(v.y, sbuf);
    return cmake(re, im);
}
template <int NT = GT> __device__ __forceinline__ double blk_sum_t(double v, double* sbuf) { return blk_sum<NT>(v, sbuf); }

// LAPACK 3.10+ zlartg, safe-range branches:  [c s; -conj(s) c] [f; g] = [r; 0], c real
// By value, every result component a scalar that is assigned once per branch, the call inlined: c, s and r stay in registers
// (reference parameters cost every calling kernel 24 bytes of scratch per lane, inlined or not).
struct Rot { double c, sx, sy, rx, ry; };
__device__ __forceinline__ Rot zlartg(c128 f, c128 g) {
    const double safmin = 2.2250738585072014e-308, rtmin = 1.4916681462400413e-154;
    Rot o;
    if (g.x == 0.0 && g.y == 0.0) { o.c = 1.0; o.sx = 0.0; o.sy = 0.0; o.rx = f.x; o.ry = f.y; return o; }
    if (f.x == 0.0 && f.y == 0.0) {
        const double d = (g.x == 0.0) ? fabs(g.y) : ((g.y == 0.0) ? fabs(g.x) : sqrt(g.x * g.x + g.y * g.y));
        o.c = 0.0; o.sx = g.x / d; o.sy = -g.y / d; o.rx = d; o.ry = 0.0; return o;
    }
    const double f2 = f.x * f.x + f.y * f.y, g2 = g.x * g.x + g.y * g.y, h2 = f2 + g2;
    const c128 gc_ = cconj(g);
    c128 sv;
    if (f2 >= h2 * safmin) {
        o.c = sqrt(f2 / h2);
        o.rx = f.x / o.c; o.ry = f.y / o.c;
        const double rtmax2 = 6.703903964971299e+153;    // 2 * sqrt(safmax/4)
        if (f2 > rtmin && h2 < rtmax2) { const double d = sqrt(f2 * h2); sv = cmul(gc_, cmake(f.x / d, f.y / d)); }
        else sv = cmul(gc_, cmake(o.rx / h2, o.ry / h2));
    } else {
        const double d = sqrt(f2 * h2);
        o.c = f2 / d;
        if (o.c >= safmin) { o.rx = f.x / o.c; o.ry = f.y / o.c; } else { const double q = h2 / d; o.rx = f.x * q; o.ry = f.y * q; }
        sv = cmul(gc_, cmake(f.x / d, f.y / d));
    }
    o.sx = sv.x; o.sy = sv.y;
    return o;
}

// The decisions after a residual r = b - H x of norm rnorm (iterative.py:737-748, 826-838): done with `info`, or a new restart
// cycle with the cycle count, ptol_max_factor and ptol it starts from.  Pure; the caller stores.
struct Resid { bool done; int info, cycle; double pmf, ptol; };
__device__ __forceinline__ Resid resid_decide(const GState& s, double rnorm, int maxiter) {
    Resid o;
    o.done = false; o.info = 0;
    o.pmf = s.pmf; o.ptol = s.ptol; o.cycle = s.cycle;
    if (!(rnorm == rnorm)) { o.done = true; o.info = maxiter; }              // NaN: can never pass a test
    else if (s.first) { if (rnorm < s.atol) { o.done = true; o.info = 0; } }
    else {
        if (rnorm <= s.atol) { o.done = true; o.info = 0; }
        else if (s.breakdown) { o.done = true; o.info = maxiter; }
        else {
            if (s.presid <= s.ptol) o.pmf = fmax(EPS, 0.25 * o.pmf); else o.pmf = fmin(1.0, 1.5 * o.pmf);
            o.ptol = s.presid * fmin(o.pmf, s.atol / rnorm);
            o.cycle += 1;
            if (o.cycle >= maxiter) { o.done = true; o.info = maxiter; }
        }
    }
    return o;
}

// The one-lane tail of an Arnoldi step (iterative.py:778-816).  h[0 .. col] holds the Gram-Schmidt coefficients of column col;
// h1 = ||w|| after them, brk the breakdown verdict.  Applies the earlier rotations, forms the new one, moves S, presid and the
// counters of GState on and, where the inner loop ends, solves for y[0 .. col] (the caller then adds y @ V[:col + 1] to x) and
// hands the candidate to phase 1; otherwise to column col + 1.  *end = whether the inner loop ended, stored where the verdict
// falls and not returned: with the store after the pseudo-solve gmres_post_kernel<32, 512> allocates its registers otherwise
// and the n = 12288 row is 1 % slower (profiles/gmres_share.txt, section 4).
__device__ __forceinline__ void arnoldi_tail(GState& s, c128* h, c128* y, int* end, int col, int R, bool brk, double h1) {
    h[col + 1] = cmake(brk ? 0.0 : h1, 0.0);
    for (int kk = 0; kk < col; ++kk) {
        const double c = s.gc[kk]; const c128 sg = s.gs[kk];
        const c128 n0 = h[kk], n1 = h[kk + 1];
        c128 a0 = cmake(c * n0.x, c * n0.y); cfma(a0, sg, n1);
        c128 a1 = cmake(c * n1.x, c * n1.y); cfms(a1, cconj(sg), n0);
        h[kk] = a0; h[kk + 1] = a1;
    }
    const Rot rot = zlartg(h[col], h[col + 1]);
    const double c = rot.c; const c128 sg = cmake(rot.sx, rot.sy), mag = cmake(rot.rx, rot.ry);
    s.gc[col] = c; s.gs[col] = sg;
    h[col] = mag; h[col + 1] = cmake(0.0, 0.0);
    const c128 Sc = s.S[col];
    const c128 tmp = cmul(cmake(-sg.x, sg.y), Sc);          // -conj(s) * S[col]
    s.S[col] = cmake(c * Sc.x, c * Sc.y);
    s.S[col + 1] = tmp;
    const double presid = hypot(tmp.x, tmp.y);
    s.presid = presid;
    s.inner += 1;
    for (int j = 0; j <= col + 1; ++j) s.h[col][j] = h[j];
    if (brk) s.breakdown = 1;
    const bool end_inner = (presid <= s.ptol) || brk || (col == R - 1);
    *end = end_inner ? 1 : 0;
    if (end_inner) {
        // y = trsv(h^T, S) with the pseudo-solve rules of iterative.py:806-816
        if (s.h[col][col].x == 0.0 && s.h[col][col].y == 0.0) s.S[col] = cmake(0.0, 0.0);
        for (int j = 0; j <= col; ++j) y[j] = s.S[j];
        for (int kk = col; kk > 0; --kk) {
            if (y[kk].x != 0.0 || y[kk].y != 0.0) {
                y[kk] = cdiv_np(y[kk], s.h[kk][kk]);
                const c128 t = y[kk];
                for (int j = 0; j < kk; ++j) cfms(y[j], t, s.h[kk][j]);
            }
        }
        if (y[0].x != 0.0 || y[0].y != 0.0) y[0] = cdiv_np(y[0], s.h[0][0]);
        s.phase = 1;
    } else {
        s.col = col + 1;
    }
}

// diag(H_k)[i] = (diag(A)[i] - lambda_k) + psi_k with the roundings of the build kernels of the direct solve
__device__ __forceinline__ c128 shifted_diag(c128 d, c128 lam, double ps) {
    return cmake(__dadd_rn(__dsub_rn(d.x, lam.x), ps), __dadd_rn(__dsub_rn(d.y, lam.y), 0.0));
}
__device__ __forceinline__ double shifted_diag(double d, c128 lam, double ps) { return __dadd_rn(__dsub_rn(d, lam.x), ps); }
// AMS:67-72: a diagonal entry rules the Jacobi scale out unless 1/d is finite and |d| > 1e-12
__device__ __forceinline__ bool jacobi_bad(c128 d) {
    const c128 inv = crecip_np(d);
    return !cfinite(inv) || !(hypot(d.x, d.y) > 1e-12);
}

__global__ void __launch_bounds__(256)
diag_kernel(const c128* __restrict__ A, int n, c128* __restrict__ d) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] = A[(long)i * n + i];
}

// AMS:67-72: ok iff every 1/diag(H) is finite and every |diag(H)| > 1e-12
__global__ void __launch_bounds__(GT)
jacobi_check_kernel(const c128* __restrict__ dA, int n, const c128* __restrict__ shift, const double* __restrict__ psi,
                    int* __restrict__ ok) {
    __shared__ int sbad;
    const int g = blockIdx.x;
    if (threadIdx.x == 0) sbad = 0;
    __syncthreads();
    const c128 lam = shift[g]; const double ps = psi[g];
    bool bad = false;
    for (int i = threadIdx.x; i < n; i += GT)
        if (jacobi_bad(shifted_diag(dA[i], lam, ps))) bad = true;
    if (bad) atomicOr(&sbad, 1);
    __syncthreads();
    if (threadIdx.x == 0) ok[g] = sbad ? 0 : 1;
}

template <class T>
struct GArgsT {
    int n, R, maxiter, rows_per;          // rows_per = R + 2 rows of the basis array per candidate
    double rtol;
    const T* dA; const c128* shift; const double* psi; const int* jac;
    const T* X; long ldx; const int* slots; const T* bvec; int rhs_mode;     // T = double: rhs_mode 1 only (the rule), X null
    T* Vb; T* Y; GState* st;
    const T* Hd; long ldh, strideH;       // dense mode: materialised H_k (null in shared-matrix mode)
};
using GArgs = GArgsT<c128>;

template <class T>
__device__ __forceinline__ const T* rhs_of(const GArgsT<T>& a, int k) {
    return a.rhs_mode == 0 ? a.X + (long)a.slots[k] * a.ldx : a.bvec;
}
template <class T>
__device__ __forceinline__ T psolve1(const GArgsT<T>& a, int k, int i, T v) {
    if (!a.jac[k]) return v;
    const T d = a.Hd ? a.Hd[(long)k * a.strideH + (long)i * a.ldh + i] : shifted_diag(a.dA[i], a.shift[k], a.psi[k]);
    return sc_jacobi(d, v);
}

// dense mode, AMS:65-86: Jacobi only where it was asked for AND every 1/diag(H_k) is finite and every |diag(H_k)| > 1e-12
__global__ void __launch_bounds__(GT)
jacobi_gate_dense_kernel(GArgs a, int* __restrict__ jac) {
    __shared__ int sbad;
    const int k = blockIdx.x;
    if (threadIdx.x == 0) sbad = 0;
    __syncthreads();
    bool bad = false;
    if (jac[k]) {
        for (int i = threadIdx.x; i < a.n; i += GT)
            if (jacobi_bad(a.Hd[(long)k * a.strideH + (long)i * a.ldh + i])) bad = true;
    }
    if (bad) atomicOr(&sbad, 1);
    __syncthreads();
    if (threadIdx.x == 0 && sbad) jac[k] = 0;
}

// dense mode matvec: Y[k] = H_k z_k for the active candidates.  One wave per matrix row at a time (a row is n x 16
// contiguous bytes), 16 rows per workgroup, z through L2: HBM-bound on H_k.
__global__ void __launch_bounds__(GT)
gemv_dense_kernel(GArgs a, const int* __restrict__ act, const int* __restrict__ zrow) {
    const int k = act[blockIdx.y];
    const c128* H = a.Hd + (long)k * a.strideH;
    const c128* z = a.Vb + (long)zrow[blockIdx.y] * a.n;
    c128* y = a.Y + (long)k * a.n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * 16 + wave * 4;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int i = r0 + rr;
        if (i >= a.n) break;
        const c128* row = H + (long)i * a.ldh;
        double sr = 0.0, si = 0.0;
        for (int j = lane; j < a.n; j += 64) {
            const c128 h = row[j], v = z[j];
            sr = fma(h.x, v.x, sr); sr = fma(-h.y, v.y, sr);
            si = fma(h.x, v.y, si); si = fma(h.y, v.x, si);
        }
        sr = wave_sum(sr); si = wave_sum(si);
        if (lane == 0) y[i] = cmake(sr, si);
    }
}

// x0 = b; norms; ptol (iterative.py:696-724)
template <class T>
__global__ void __launch_bounds__(GT)
gmres_init_kernel(GArgsT<T> a) {
    __shared__ double sbuf[GT / 64];
    const int k = blockIdx.x;
    const T* b = rhs_of(a, k);
    T* x = a.Vb + ((long)k * a.rows_per + a.R + 1) * a.n;
    double sb = 0.0, sm = 0.0;
    for (int i = threadIdx.x; i < a.n; i += GT) {
        const T v = b[i];
        x[i] = v;
        sc_abs2(sb, v);
        const T m = psolve1(a, k, i, v);
        sc_abs2(sm, m);
    }
    sb = blk_sum(sb, sbuf); sm = blk_sum(sm, sbuf);
    if (threadIdx.x == 0) {
        GState& s = a.st[k];
        s.bnrm2 = sqrt(sb);
        s.atol = fmax(0.0, a.rtol * s.bnrm2);
        s.pmf = 1.0;
        s.ptol = sqrt(sm) * fmin(1.0, s.atol / s.bnrm2);
        s.presid = 0.0; s.rnorm = 0.0;
        s.col = 0; s.cycle = 0; s.inner = 0; s.info = 0; s.breakdown = 0; s.first = 1;
        s.phase = (s.bnrm2 == 0.0) ? 2 : 1;             // b == 0 -> return b, info 0
    }
}

// Y[act[first + p]] = Y[act[0]] (see the first product of a linear system in maus_gmres_run)
__global__ void __launch_bounds__(256)
bcast_row_kernel(c128* __restrict__ Y, int n, const int* __restrict__ act, int first) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) Y[(long)act[first + blockIdx.y] * n + i] = Y[(long)act[0] * n + i];
}

// Rows nact .. to - 1 of the product's row lists repeat row 0 (see the dense shared product in maus_gmres_run): the product
// kernel then computes candidate act[0]'s row several times and every copy stores the same bits to the same row of Y.
__global__ void __launch_bounds__(64)
gmres_pad_rows_kernel(int* __restrict__ act, int* __restrict__ zrow, int nact, int to) {
    const int p = nact + threadIdx.x;
    if (p < to) { act[p] = act[0]; zrow[p] = zrow[0]; }
}

// what a tick's kernels of the wide step need of a candidate besides GState: phase and column as the compact kernel found them
// (the state kernel moves GState on while the finish kernel still needs them), the Hessenberg column under construction, and the
// state kernel's verdict for the finish kernel
struct WState {
    int phase, col, cont, end;        // cont: phase 1 goes on to a new cycle; end: the inner loop ended, x += y @ V[:col+1]
    double inv, pad;
    c128 hcol[MAXR + 2];
    c128 y[MAXR + 1];
};

// active list + the row of the basis array each active candidate multiplies next; out[0] = active candidates.  WIDE (the wide
// step): also the tick's (phase, col) of every active candidate into WState, and what the host needs to issue only the launches
// the tick has work for: out[1] = largest col among those in phase 0 (-1: none), out[2] = candidates in phase 1, out[3] = sum of
// col over phase 0 (the byte count of the profile class)
template <bool WIDE>
__global__ void __launch_bounds__(1024)
gmres_compact_kernel(const GState* __restrict__ st, int count, int rows_per, int R, int* __restrict__ act,
                     int* __restrict__ zrow, WState* __restrict__ ws, int* __restrict__ out) {
    __shared__ int scnt[16];
    __shared__ int sbase;
    __shared__ int smax, sp1, ssum;           // WIDE only
    if (threadIdx.x == 0) {
        sbase = 0;
        if (WIDE) { smax = -1; sp1 = 0; ssum = 0; }
    }
    __syncthreads();
    int mx = -1, p1 = 0, sum = 0;
    for (int k0 = 0; k0 < count; k0 += 1024) {
        const int k = k0 + threadIdx.x;
        const bool on = k < count && st[k].phase != 2;
        const unsigned long long m = __ballot(on);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) scnt[wave] = __popcll(m);
        __syncthreads();
        int off = sbase;
        for (int w = 0; w < wave; ++w) off += scnt[w];
        if (on) {
            const int p = off + __popcll(m & ((1ull << lane) - 1ull));
            const int ph = st[k].phase, col = st[k].col;
            act[p] = k;
            zrow[p] = k * rows_per + (ph == 1 ? R + 1 : col);
            if (WIDE) {
                ws[k].phase = ph; ws[k].col = col; ws[k].cont = 0; ws[k].end = 0;
                if (ph == 1) p1 += 1; else { mx = max(mx, col); sum += col; }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) { int t = 0; for (int w = 0; w < 16; ++w) t += scnt[w]; sbase += t; }
        __syncthreads();
    }
    if (WIDE) {
        atomicMax(&smax, mx); atomicAdd(&sp1, p1); atomicAdd(&ssum, sum);     // integers: any order gives the same result
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = sbase;
        if (WIDE) { out[1] = smax; out[2] = sp1; out[3] = ssum; }
    }
}

// EPT entries of the candidate's vectors per thread of an NT-thread workgroup: 256 threads up to n = 8192, 512 threads (EPT 32,
// the same 128 VGPRs of w) for 8192 < n <= 16384
template <class T, int EPT, int NT = GT>
__global__ void __launch_bounds__(NT)
gmres_post_kernel(GArgsT<T> a, const int* __restrict__ act) {
    __shared__ double sbuf[NT / 64];
    __shared__ c128 s_h[MAXR + 2];
    __shared__ c128 s_y[MAXR + 1];
    __shared__ int s_flag[2];                 // [0]: x update requested, [1]: candidate finished this tick
    const int k = act[blockIdx.x];
    GState& s = a.st[k];
    const int n = a.n, R = a.R, tid = threadIdx.x;
    const int phase = s.phase, col = s.col;
    T* Vk = a.Vb + (long)k * a.rows_per * n;
    T* x = Vk + (long)(R + 1) * n;
    const T* y = a.Y + (long)k * n;
    const c128 lam = a.shift[k];
    // H z = A z + (psi - lambda) z ; in dense mode the shift is part of the materialised H_k
    const T sh = a.Hd ? czero<T>() : sc_shift<T>(a.psi[k], lam);
    T w[EPT];

    if (phase == 1) {
        // ---- r = b - H x ; exit tests ; start of the next restart cycle (iterative.py:737-748, 826-838) ----
        const T* b = rhs_of(a, k);
        double ss = 0.0;
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int i = tid + e * NT;
            if (i < n) {
                T hx = y[i]; cfma(hx, sh, x[i]);
                const T r = sc_sub(b[i], hx);
                w[e] = r;
                sc_abs2(ss, r);
            }
        }
        const double rnorm = sqrt(blk_sum<NT>(ss, sbuf));
        const Resid d = resid_decide(s, rnorm, a.maxiter);
        if (d.done) {
            __syncthreads();
            if (tid == 0) { s.rnorm = rnorm; s.info = d.info; s.phase = 2; }
            return;
        }
        // V[0] = psolve(r) / ||psolve(r)||
        double sv = 0.0;
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int i = tid + e * NT;
            if (i < n) { w[e] = psolve1(a, k, i, w[e]); sc_abs2(sv, w[e]); }
        }
        const double tmp = sqrt(blk_sum<NT>(sv, sbuf));
        const double inv = 1.0 / tmp;
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int i = tid + e * NT;
            if (i < n) Vk[i] = sc_scale(w[e], inv);
        }
        if (tid == 0) {
            s.rnorm = rnorm; s.pmf = d.pmf; s.ptol = d.ptol; s.cycle = d.cycle; s.first = 0;
            for (int j = 0; j <= R; ++j) s.S[j] = cmake(0.0, 0.0);
            s.S[0] = cmake(tmp, 0.0);
            s.col = 0; s.breakdown = 0; s.phase = 0;
        }
        return;
    }

    // ---- Arnoldi step (iterative.py:751-800) ----
    const T* z = Vk + (long)col * n;
    double ss = 0.0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int i = tid + e * NT;
        if (i < n) {
            T av = y[i]; cfma(av, sh, z[i]);
            w[e] = psolve1(a, k, i, av);
            sc_abs2(ss, w[e]);
        }
    }
    const double h0 = sqrt(blk_sum<NT>(ss, sbuf));
    for (int kk = 0; kk <= col; ++kk) {                        // modified Gram-Schmidt
        const T* vk = Vk + (long)kk * n;
        T t = czero<T>();                                      // vdot(V[kk], w)
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int i = tid + e * NT;
            if (i < n) cfma_conj(t, vk[i], w[e]);
        }
        t = blk_sum_t<NT>(t, sbuf);
        if (tid == 0) s_h[kk] = sc_c(t);
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int i = tid + e * NT;
            if (i < n) cfms(w[e], t, vk[i]);
        }
    }
    ss = 0.0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int i = tid + e * NT;
        if (i < n) { sc_abs2(ss, w[e]); }
    }
    const double h1 = sqrt(blk_sum<NT>(ss, sbuf));
    const bool brk = h1 <= EPS * h0;
    {
        T* vn = Vk + (long)(col + 1) * n;
        const double inv = brk ? 1.0 : 1.0 / h1;
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int i = tid + e * NT;
            if (i < n) vn[i] = sc_scale(w[e], inv);
        }
    }
    if (tid == 0) arnoldi_tail(s, s_h, s_y, &s_flag[0], col, R, brk, h1);
    __syncthreads();
    if (s_flag[0]) {                                           // x += y @ V[:col+1]
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int i = tid + e * NT;
            if (i < n) {
                T acc = x[i];
                for (int j = 0; j <= col; ++j) cfma(acc, sc_of<T>(s_y[j]), Vk[(long)j * n + i]);
                x[i] = acc;
            }
        }
    }
}

// gmres_post_kernel for 16384 < n (CSR matrices only): w is not held in registers but streamed through the basis row it
// becomes, V[col + 1] (the Arnoldi step) or V[0] (the residual of a new cycle); thread t owns the entries t, t + NT, ... of
// every vector, as the register kernels do.  Same modified Gram-Schmidt order, state machine and exits; the variant is picked
// from n alone.  The vector loops below are gmres_post_kernel's line for line but for where w lives.
template <class T, int NT>
__global__ void __launch_bounds__(NT)
gmres_post_stream_kernel(GArgsT<T> a, const int* __restrict__ act) {
    __shared__ double sbuf[NT / 64];
    __shared__ c128 s_h[MAXR + 2];
    __shared__ c128 s_y[MAXR + 1];
    __shared__ int s_flag[2];
    const int k = act[blockIdx.x];
    GState& s = a.st[k];
    const int n = a.n, R = a.R, tid = threadIdx.x;
    const int phase = s.phase, col = s.col;
    T* Vk = a.Vb + (long)k * a.rows_per * n;
    T* x = Vk + (long)(R + 1) * n;
    const T* y = a.Y + (long)k * n;
    const c128 lam = a.shift[k];
    const T sh = a.Hd ? czero<T>() : sc_shift<T>(a.psi[k], lam);

    if (phase == 1) {
        const T* b = rhs_of(a, k);
        T* w = Vk;
        double ss = 0.0;
        for (int i = tid; i < n; i += NT) {
            T hx = y[i]; cfma(hx, sh, x[i]);
            const T r = sc_sub(b[i], hx);
            w[i] = r;
            sc_abs2(ss, r);
        }
        const double rnorm = sqrt(blk_sum<NT>(ss, sbuf));
        const Resid d = resid_decide(s, rnorm, a.maxiter);
        if (d.done) {
            __syncthreads();
            if (tid == 0) { s.rnorm = rnorm; s.info = d.info; s.phase = 2; }
            return;
        }
        double sv = 0.0;
        for (int i = tid; i < n; i += NT) {
            const T v = psolve1(a, k, i, w[i]);
            w[i] = v;
            sc_abs2(sv, v);
        }
        const double tmp = sqrt(blk_sum<NT>(sv, sbuf));
        const double inv = 1.0 / tmp;
        for (int i = tid; i < n; i += NT) w[i] = sc_scale(w[i], inv);
        if (tid == 0) {
            s.rnorm = rnorm; s.pmf = d.pmf; s.ptol = d.ptol; s.cycle = d.cycle; s.first = 0;
            for (int j = 0; j <= R; ++j) s.S[j] = cmake(0.0, 0.0);
            s.S[0] = cmake(tmp, 0.0);
            s.col = 0; s.breakdown = 0; s.phase = 0;
        }
        return;
    }

    const T* z = Vk + (long)col * n;
    T* w = Vk + (long)(col + 1) * n;
    double ss = 0.0;
    for (int i = tid; i < n; i += NT) {
        T av = y[i]; cfma(av, sh, z[i]);
        const T v = psolve1(a, k, i, av);
        w[i] = v;
        sc_abs2(ss, v);
    }
    const double h0 = sqrt(blk_sum<NT>(ss, sbuf));
    for (int kk = 0; kk <= col; ++kk) {                        // modified Gram-Schmidt
        const T* vk = Vk + (long)kk * n;
        T t = czero<T>();                                      // vdot(V[kk], w)
        for (int i = tid; i < n; i += NT) cfma_conj(t, vk[i], w[i]);
        t = blk_sum_t<NT>(t, sbuf);
        if (tid == 0) s_h[kk] = sc_c(t);
        for (int i = tid; i < n; i += NT) { T wi = w[i]; cfms(wi, t, vk[i]); w[i] = wi; }
    }
    ss = 0.0;
    for (int i = tid; i < n; i += NT) { const T wi = w[i]; sc_abs2(ss, wi); }
    const double h1 = sqrt(blk_sum<NT>(ss, sbuf));
    const bool brk = h1 <= EPS * h0;
    {
        const double inv = brk ? 1.0 : 1.0 / h1;
        for (int i = tid; i < n; i += NT) w[i] = sc_scale(w[i], inv);
    }
    if (tid == 0) arnoldi_tail(s, s_h, s_y, &s_flag[0], col, R, brk, h1);
    __syncthreads();
    if (s_flag[0]) {                                           // x += y @ V[:col+1]
        for (int i = tid; i < n; i += NT) {
            T acc = x[i];
            for (int j = 0; j <= col; ++j) cfma(acc, sc_of<T>(s_y[j]), Vk[(long)j * n + i]);
            x[i] = acc;
        }
    }
}

// ---- the wide step (maus_gmres_set_method(ctx, 1)): the post step of a CSR-bound solve over the whole device ----
// The arithmetic is gmres_post_stream_kernel's; the ownership is lanczos.hip's.  A workgroup of GW_BT threads owns GW_SPAN
// consecutive entries of ONE candidate's vectors, two per thread; workgroup q of a launch is piece q % np of active candidate
// q / np.  Every reduction goes through per-piece partial sums in memory and is joined in one fixed order by every workgroup
// that needs it (gw_join): thread t adds pieces t, t + 256, ..., then the 64 lanes on the DPP tree of wave_sum_dpp, then the
// four waves in index order.  All pieces of a candidate compute the same bits from the same partials; piece 0 keeps the value.
// No atomics on values, no workgroup waits for another: the launch boundaries of the stream are the only synchronisation.
// A candidate's sums depend on its own data and on n alone -- not on the batch, its order or its neighbours' states.
constexpr int GW_BT = 256;
constexpr int GW_E = 2;
constexpr int GW_SPAN = GW_BT * GW_E;

__device__ __forceinline__ c128 gw_block_sum(c128 v, c128* sbuf) {
    const double re = wave_sum_dpp(v.x), im = wave_sum_dpp(v.y);
    if ((threadIdx.x & 63) == 0) sbuf[threadIdx.x >> 6] = cmake(re, im);
    __syncthreads();
    const c128 s = cmake((sbuf[0].x + sbuf[1].x) + (sbuf[2].x + sbuf[3].x), (sbuf[0].y + sbuf[1].y) + (sbuf[2].y + sbuf[3].y));
    __syncthreads();
    return s;
}
// a sum of doubles: the real part of the same tree (the squared norms; every sum of the real path)
__device__ __forceinline__ double gw_block_sum(double v, c128* sbuf) {
    double* sb = (double*)sbuf;
    const double re = wave_sum_dpp(v);
    if ((threadIdx.x & 63) == 0) sb[threadIdx.x >> 6] = re;
    __syncthreads();
    const double s = (sb[0] + sb[1]) + (sb[2] + sb[3]);
    __syncthreads();
    return s;
}
template <class T>
__device__ __forceinline__ T gw_join(const T* __restrict__ part, int np, c128* sbuf) {
    T acc = czero<T>();
    for (int b = threadIdx.x; b < np; b += GW_BT) acc = sc_add(acc, part[b]);
    return gw_block_sum(acc, sbuf);
}

template <class T>
struct WArgsT {
    WState* ws; T* part0; T* part1; c128* pn;     // part0 / part1: the dot products, alternating by column; pn: the pair (|w|^2 before, after)
    int np;
};

// Form.  Phase 0: w = psolve(y + sh z) into V[col + 1], pn.x = the piece's share of ||w||^2, part0 = its share of vdot(V[0], w).
// Phase 1: r = b - (y + sh x) into V[0], pn.x = its share of ||r||^2.
template <class T>
__global__ void __launch_bounds__(GW_BT)
gw_form_kernel(GArgsT<T> a, const int* __restrict__ act, WArgsT<T> wa) {
    __shared__ c128 sbuf[GW_BT / 64];
    const int piece = blockIdx.x % wa.np, k = act[blockIdx.x / wa.np];
    const WState& W = wa.ws[k];
    const int n = a.n, phase = W.phase, col = W.col;
    T* Vk = a.Vb + (long)k * a.rows_per * n;
    const T* y = a.Y + (long)k * n;
    const c128 lam = a.shift[k];
    const T sh = sc_shift<T>(a.psi[k], lam);
    const int x0 = piece * GW_SPAN + threadIdx.x;
    const long o = (long)k * wa.np + piece;
    if (phase == 1) {
        const T* b = rhs_of(a, k);
        const T* x = Vk + (long)(a.R + 1) * n;
        double ss = 0.0;
#pragma unroll
        for (int e = 0; e < GW_E; ++e) {
            const int i = x0 + e * GW_BT;
            if (i < n) {
                T hx = y[i]; cfma(hx, sh, x[i]);
                const T r = sc_sub(b[i], hx);
                Vk[i] = r;
                sc_abs2(ss, r);
            }
        }
        const double s = gw_block_sum(ss, sbuf);
        if (threadIdx.x == 0) wa.pn[o].x = s;
        return;
    }
    const T* z = Vk + (long)col * n;
    const T* v0 = Vk;
    T* w = Vk + (long)(col + 1) * n;
    double ss = 0.0;
    T acc = czero<T>();
#pragma unroll
    for (int e = 0; e < GW_E; ++e) {
        const int i = x0 + e * GW_BT;
        if (i < n) {
            T av = y[i]; cfma(av, sh, z[i]);
            const T v = psolve1(a, k, i, av);
            w[i] = v;
            sc_abs2(ss, v);
            cfma_conj(acc, v0[i], v);
        }
    }
    const double s = gw_block_sum(ss, sbuf);
    const T d = gw_block_sum(acc, sbuf);
    if (threadIdx.x == 0) { wa.pn[o].x = s; wa.part0[o] = d; }
}

// Phase 1, the decisions of iterative.py:737-748 / 826-838 from the joined ||r||: done (phase 2) or a new cycle (cont)
template <class T>
__global__ void __launch_bounds__(GW_BT)
gw_resid_kernel(GArgsT<T> a, const int* __restrict__ act, WArgsT<T> wa) {
    __shared__ c128 sbuf[GW_BT / 64];
    const int k = act[blockIdx.x];
    WState& W = wa.ws[k];
    if (W.phase != 1) return;
    const double rnorm = sqrt(gw_join(wa.pn + (long)k * wa.np, wa.np, sbuf).x);
    if (threadIdx.x != 0) return;
    GState& s = a.st[k];
    const Resid d = resid_decide(s, rnorm, a.maxiter);
    if (d.done) { s.rnorm = rnorm; s.info = d.info; s.phase = 2; return; }
    s.rnorm = rnorm; s.pmf = d.pmf; s.ptol = d.ptol; s.cycle = d.cycle; s.first = 0;
    W.cont = 1;
}

// Phase 1, new cycle: V[0] = psolve(r), pn.y = the piece's share of its squared norm
template <class T>
__global__ void __launch_bounds__(GW_BT)
gw_psolve_kernel(GArgsT<T> a, const int* __restrict__ act, WArgsT<T> wa) {
    __shared__ c128 sbuf[GW_BT / 64];
    const int piece = blockIdx.x % wa.np, k = act[blockIdx.x / wa.np];
    const WState& W = wa.ws[k];
    if (W.phase != 1 || !W.cont) return;
    const int n = a.n;
    T* w = a.Vb + (long)k * a.rows_per * n;
    const int x0 = piece * GW_SPAN + threadIdx.x;
    double sv = 0.0;
#pragma unroll
    for (int e = 0; e < GW_E; ++e) {
        const int i = x0 + e * GW_BT;
        if (i < n) {
            const T v = psolve1(a, k, i, w[i]);
            w[i] = v;
            sc_abs2(sv, v);
        }
    }
    const double s = gw_block_sum(sv, sbuf);
    if (threadIdx.x == 0) wa.pn[(long)k * wa.np + piece].y = s;
}

// Phase 1, new cycle: V[0] /= ||V[0]||; piece 0 starts the cycle in GState (nothing of this tick reads GState after it)
template <class T>
__global__ void __launch_bounds__(GW_BT)
gw_start_kernel(GArgsT<T> a, const int* __restrict__ act, WArgsT<T> wa) {
    __shared__ c128 sbuf[GW_BT / 64];
    const int piece = blockIdx.x % wa.np, k = act[blockIdx.x / wa.np];
    const WState& W = wa.ws[k];
    if (W.phase != 1 || !W.cont) return;
    const int n = a.n;
    T* w = a.Vb + (long)k * a.rows_per * n;
    const double tmp = sqrt(gw_join(wa.pn + (long)k * wa.np, wa.np, sbuf).y);
    const double inv = 1.0 / tmp;
    const int x0 = piece * GW_SPAN + threadIdx.x;
#pragma unroll
    for (int e = 0; e < GW_E; ++e) {
        const int i = x0 + e * GW_BT;
        if (i < n) w[i] = sc_scale(w[i], inv);
    }
    if (piece == 0 && threadIdx.x == 0) {
        GState& s = a.st[k];
        for (int j = 0; j <= a.R; ++j) s.S[j] = cmake(0.0, 0.0);
        s.S[0] = cmake(tmp, 0.0);
        s.col = 0; s.breakdown = 0; s.phase = 0;
    }
}

// One column of the modified Gram-Schmidt sweep.  kk >= 1: candidates with col >= kk join dot kk - 1 (written by the launch
// before, or by the form kernel), apply w -= t V[kk - 1] and write their share of vdot(V[kk], w) from the w that leaves.
// kk == 0 is the tail: every phase-0 candidate joins its last dot (column col), applies the last subtraction and writes
// pn.y = its share of ||w||^2.
template <class T>
__global__ void __launch_bounds__(GW_BT)
gw_mgs_kernel(GArgsT<T> a, const int* __restrict__ act, WArgsT<T> wa, int kk) {
    __shared__ c128 sbuf[GW_BT / 64];
    const int piece = blockIdx.x % wa.np, k = act[blockIdx.x / wa.np];
    WState& W = wa.ws[k];
    if (W.phase != 0) return;
    const int col = W.col;
    const bool tail = kk == 0;
    if (tail) kk = col + 1; else if (kk > col) return;
    const int j = kk - 1, n = a.n;
    const long o = (long)k * wa.np;
    const T t = gw_join(((j & 1) ? wa.part1 : wa.part0) + o, wa.np, sbuf);
    if (piece == 0 && threadIdx.x == 0) W.hcol[j] = sc_c(t);
    T* Vk = a.Vb + (long)k * a.rows_per * n;
    const T* vj = Vk + (long)j * n;
    const T* vk = Vk + (long)kk * n;          // the tail never reads it (it is w)
    T* w = Vk + (long)(col + 1) * n;
    const int x0 = piece * GW_SPAN + threadIdx.x;
    T acc = czero<T>();
    double ss = 0.0;
#pragma unroll
    for (int e = 0; e < GW_E; ++e) {
        const int i = x0 + e * GW_BT;
        if (i < n) {
            T wi = w[i]; cfms(wi, t, vj[i]); w[i] = wi;
            if (tail) sc_abs2(ss, wi);
            else cfma_conj(acc, vk[i], wi);
        }
    }
    if (tail) {                                   // uniform over the workgroup
        const double s = gw_block_sum(ss, sbuf);
        if (threadIdx.x == 0) wa.pn[o + piece].y = s;
    } else {
        const T s = gw_block_sum(acc, sbuf);
        if (threadIdx.x == 0) ((kk & 1) ? wa.part1 : wa.part0)[o + piece] = s;
    }
}

// State: h0 and h1 from the joined partials, then arnoldi_tail on one lane per candidate, the Hessenberg column and y in WState
template <class T>
__global__ void __launch_bounds__(GW_BT)
gw_state_kernel(GArgsT<T> a, const int* __restrict__ act, WArgsT<T> wa) {
    __shared__ c128 sbuf[GW_BT / 64];
    const int k = act[blockIdx.x];
    WState& W = wa.ws[k];
    if (W.phase != 0) return;
    const c128 nn = gw_join(wa.pn + (long)k * wa.np, wa.np, sbuf);
    if (threadIdx.x != 0) return;
    GState& s = a.st[k];
    const double h0 = sqrt(nn.x), h1 = sqrt(nn.y);
    const bool brk = h1 <= EPS * h0;
    W.inv = brk ? 1.0 : 1.0 / h1;
    arnoldi_tail(s, W.hcol, W.y, &W.end, W.col, a.R, brk, h1);
}

// Finish: V[col + 1] = w * inv, and x += y @ V[:col + 1] where the inner loop ended
template <class T>
__global__ void __launch_bounds__(GW_BT)
gw_finish_kernel(GArgsT<T> a, const int* __restrict__ act, WArgsT<T> wa) {
    __shared__ c128 s_y[MAXR + 1];
    const int piece = blockIdx.x % wa.np, k = act[blockIdx.x / wa.np];
    const WState& W = wa.ws[k];
    if (W.phase != 0) return;
    const int n = a.n, col = W.col, end = W.end;
    const double inv = W.inv;
    if (end && threadIdx.x <= col) s_y[threadIdx.x] = W.y[threadIdx.x];
    __syncthreads();
    T* Vk = a.Vb + (long)k * a.rows_per * n;
    T* w = Vk + (long)(col + 1) * n;
    T* x = Vk + (long)(a.R + 1) * n;
    const int x0 = piece * GW_SPAN + threadIdx.x;
#pragma unroll
    for (int e = 0; e < GW_E; ++e) {
        const int i = x0 + e * GW_BT;
        if (i < n) {
            w[i] = sc_scale(w[i], inv);
            if (end) {
                T acc = x[i];
                for (int j = 0; j <= col; ++j) cfma(acc, sc_of<T>(s_y[j]), Vk[(long)j * n + i]);
                x[i] = acc;
            }
        }
    }
}

// W[slot] <- x ; outputs
template <class T>
__global__ void __launch_bounds__(GT)
gmres_finish_kernel(GArgsT<T> a, c128* __restrict__ W, long ldw, int* __restrict__ info, int* __restrict__ inner, int* __restrict__ status) {
    __shared__ int sbad;
    const int k = blockIdx.x;
    if (threadIdx.x == 0) sbad = 0;
    __syncthreads();
    const T* x = a.Vb + ((long)k * a.rows_per + a.R + 1) * a.n;
    c128* w = W + (long)a.slots[k] * ldw;
    bool bad = false;
    for (int i = threadIdx.x; i < a.n; i += GT) { const T v = x[i]; w[i] = sc_c(v); bad |= !sc_finite(v); }
    if (bad) atomicOr(&sbad, 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        const GState& s = a.st[k];
        info[k] = (s.phase == 2) ? s.info : a.maxiter;
        inner[k] = s.inner;
        status[k] = (info[k] == 0 && sbad) ? -2 : 0;
    }
}

// sparse matrix: every active candidate's product through the CSR operand (rows do not depend on the batch, so the shared first
// product A x0 of rhs_mode 1 needs no special case)
void csr_product(maus_ctx* c, const GArgsT<c128>& a, const int* zrow, const int* act, int nact) {
    const int n = a.n;
    ProfScope ps(c, KC_SPMM, 8.0 * nact * c->Acsr.nnz, maus_spmm_operand_bytes(c->Acsr) * ((nact + 7) / 8) + 32.0 * nact * n);
    maus_spmm_launch(c->st, c->Acsr, c->csr_sched, a.Vb, n, a.Y, n, zrow, act, nact);
}
// the real path: a quarter of the flops, 8 of the 16 bytes of every value and vector entry
void csr_product(maus_ctx* c, const GArgsT<double>& a, const int* zrow, const int* act, int nact) {
    const int n = a.n;
    ProfScope ps(c, KC_SPMM_REAL, 2.0 * nact * c->Acsr.nnz, maus_spmm_operand_bytes_real(c->Acsr) * ((nact + 7) / 8) + 16.0 * nact * n);
    maus_spmm_launch_real(c->st, c->Acsr, c->csr_sched, a.Vb, n, a.Y, n, zrow, act, nact);
}

// what a solve over T reads of the context, and the profile classes of its post step (one workgroup per candidate / wide)
template <class T> struct Bound;
template <> struct Bound<c128> {
    static const c128* diag(const maus_ctx* c) { return c->Adiag; }
    static const c128* rhs(const maus_ctx* c) { return c->b; }
    static const c128* pop(const maus_ctx* c) { return c->X; }
    enum { KC_POST = KC_VEC, KC_POST_WIDE = KC_GMRES_WIDE };
};
template <> struct Bound<double> {
    static const double* diag(const maus_ctx* c) { return c->Adiag_r; }
    static const double* rhs(const maus_ctx* c) { return c->b_r; }
    static const double* pop(const maus_ctx*) { return nullptr; }
    enum { KC_POST = KC_GMRES_REAL, KC_POST_WIDE = KC_GMRES_REAL };
};

}  // namespace

int maus_jacobi_check_run(maus_ctx* c, int count, const double* shift, const double* psi, int32_t* ok) {
    if (!maus_has_matrix(c) || c->rows != c->cols) FAIL(c, "maus_jacobi_check: square matrix required");
    if (count <= 0) return 0;
    const int n = c->rows;
    if (ensure_scalars(c, count)) return -1;
    if (ensure_scratch(c, sizeof(c128) * n)) return -1;
    c128* dA = (c128*)c->scratch;
    if (c->csr) HIPCHK(c, hipMemcpyAsync(dA, c->Adiag, sizeof(c128) * n, hipMemcpyDeviceToDevice, c->st));
    else hipLaunchKernelGGL(diag_kernel, dim3((n + 255) / 256), dim3(256), 0, c->st, c->A, n, dA);
    if (maus_h2d(c, c->d_c1, shift, sizeof(c128) * count, c->st)) return -1;
    if (maus_h2d(c, c->d_r1, psi, sizeof(double) * count, c->st)) return -1;
    hipLaunchKernelGGL(jacobi_check_kernel, dim3(count), dim3(GT), 0, c->st, dA, n, c->d_c1, c->d_r1, c->d_i1);
    if (maus_d2h(c, ok, c->d_i1, sizeof(int) * count, c->st)) return -1;
    HIPCHK(c, hipStreamSynchronize(c->st));
    return 0;
}

// The driver over the scalar type T of the vectors.  T = double: the real path -- maus_gmres_run has checked the rule, the
// matrix is CSR-bound, rhs_mode is 1 and Hdense is null; the scratch holds rows of n doubles, the states are the complex ones.
template <class T>
static int gmres_run_t(maus_ctx* c, const int* slots, int count, const double* shift, const double* psi, int rhs_mode,
                       const int32_t* use_jacobi, double rtol, int restart, int maxiter, int32_t* info_out, int32_t* inner_out,
                       int32_t* status, const T* Hdense, long ldh, long strideH, int32_t* jacobi_out) {
    constexpr bool CPLX = sizeof(T) == sizeof(c128);
    if (!maus_has_matrix(c) || !c->X) FAIL(c, "maus_gmres: matrix/population missing");
    if (c->csr && Hdense) FAIL(c, "maus_gmres: a sparse matrix has no random term (no materialised H)");
    if (c->rows != c->cols) FAIL(c, "maus_gmres: square matrix required");
    if (rhs_mode == 1 && (!c->b || c->bn != c->rows)) FAIL(c, "maus_gmres: rhs b not set");
    if (restart < 1 || restart > MAXR) FAIL(c, "maus_gmres: restart must be between 1 and 20 (the Krylov basis holds 20 vectors)");
    if (count <= 0) return 0;
    const int n = c->rows;
    if (n > maus_lu_max_n() && !c->csr) FAIL(c, "maus_gmres: n <= 16384 in this build (a CSR matrix: n <= maus_sparse_max_n())");
    if (n > maus_sparse_max_n()) FAIL(c, "maus_gmres: n exceeds maus_sparse_max_n()");
    const int R = std::min(restart, n);                      // SciPy: restart = min(restart, n)
    if (maxiter < 1) maxiter = 1;
    if (upload_slots(c, slots, count)) return -1;
    // scratch: diag | basis (count*(R+2) rows) | Y (count rows) | states | act | zrow | nact | jac | info/inner/status
    const size_t rows_per = (size_t)R + 2;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const size_t o_d = take(sizeof(T) * n), o_v = take(sizeof(T) * rows_per * count * n), o_y = take(sizeof(T) * (size_t)count * n),
                 o_s = take(sizeof(GState) * count), o_a = take(sizeof(int) * std::max(count, PAD_ROWS)),
                 o_z = take(sizeof(int) * std::max(count, PAD_ROWS)),
                 o_n = take(sizeof(int) * 4), o_j = take(sizeof(int) * count), o_o = take(sizeof(int) * 3 * count);
    // the wide step (method 1, CSR only): per-candidate tick state and three partial-sum buffers of one entry per piece (the
    // pair of squared norms, then the two dot products in T)
    const bool wide = c->gmres_method == 1 && c->csr && !Hdense;
    const int np = (n + GW_SPAN - 1) / GW_SPAN;
    const size_t o_w = wide ? take(sizeof(WState) * count) : 0, o_p = wide ? take((sizeof(T) * 2 + sizeof(c128)) * (size_t)count * np) : 0;
    if (wide && (size_t)count * np > 0x7fffffffull) FAIL(c, "maus_gmres: candidates x pieces of the wide step exceed a launch");
    if (ensure_scratch(c, off)) return -1;
    char* base = (char*)c->scratch;
    GArgsT<T> a;
    a.n = n; a.R = R; a.maxiter = maxiter; a.rows_per = (int)rows_per; a.rtol = rtol;
    a.dA = (T*)(base + o_d); a.Vb = (T*)(base + o_v); a.Y = (T*)(base + o_y); a.st = (GState*)(base + o_s);
    int* act = (int*)(base + o_a); int* zrow = (int*)(base + o_z); int* nact = (int*)(base + o_n);
    int* jac = (int*)(base + o_j); int* outs = (int*)(base + o_o);
    a.Hd = Hdense; a.ldh = ldh; a.strideH = strideH;
    a.shift = c->d_c1; a.psi = c->d_r1; a.jac = jac; a.X = Bound<T>::pop(c); a.ldx = c->ldp; a.slots = c->d_slots; a.bvec = Bound<T>::rhs(c); a.rhs_mode = rhs_mode;
    if (maus_h2d(c, c->d_c1, shift, sizeof(c128) * count, c->st)) return -1;
    if (maus_h2d(c, c->d_r1, psi, sizeof(double) * count, c->st)) return -1;
    if (maus_h2d(c, jac, use_jacobi, sizeof(int) * count, c->st)) return -1;
    if (c->csr) HIPCHK(c, hipMemcpyAsync(base + o_d, Bound<T>::diag(c), sizeof(T) * n, hipMemcpyDeviceToDevice, c->st));
    else hipLaunchKernelGGL(diag_kernel, dim3((n + 255) / 256), dim3(256), 0, c->st, c->A, n, (c128*)(base + o_d));
    if constexpr (CPLX) { if (Hdense) hipLaunchKernelGGL(jacobi_gate_dense_kernel, dim3(count), dim3(GT), 0, c->st, a, jac); }
    hipLaunchKernelGGL(gmres_init_kernel<T>, dim3(count), dim3(GT), 0, c->st, a);
    const long max_ticks = (long)maxiter * (R + 1) + 2;
    int h_nact = 0;
    WArgsT<T> wa;
    wa.ws = (WState*)(base + o_w); wa.pn = (c128*)(base + o_p); wa.part0 = (T*)(wa.pn + (size_t)count * np);
    wa.part1 = wa.part0 + (size_t)count * np; wa.np = np;
    for (long tick = 0; wide && tick < max_ticks; ++tick) {
        // one read-back per tick, as below: how many candidates are active, the largest column among those in phase 0 and how
        // many are in phase 1 -- the host issues only the launches this tick has work for
        int h[4] = {0, -1, 0, 0};
        hipLaunchKernelGGL(gmres_compact_kernel<true>, dim3(1), dim3(1024), 0, c->st, a.st, count, (int)rows_per, R, act, zrow, wa.ws, nact);
        if (maus_d2h(c, h, nact, sizeof(int) * 4, c->st)) return -1;
        HIPCHK(c, hipStreamSynchronize(c->st));
        h_nact = h[0];
        if (h_nact <= 0) break;
        const int maxcol = h[1], n1 = h[2], n0 = h_nact - n1;
        if (maxcol >= R || (n0 > 0) != (maxcol >= 0)) FAIL(c, "maus_gmres: inconsistent tick summary of the wide step");
        csr_product(c, a, zrow, act, h_nact);
        // bytes: form 64 n per candidate; a Gram-Schmidt column 64 n (w in and out, V[kk - 1], V[kk]), the tail 48 n; finish 32 n;
        // a new cycle 64 n (x += y @ V of the candidates whose inner loop ends is not counted)
        ProfScope ps(c, Bound<T>::KC_POST_WIDE, 0, (sizeof(T) / 16.0) * (double)n * (64.0 * h_nact + 64.0 * h[3] + 80.0 * n0 + 64.0 * n1));
        const dim3 gp((unsigned)((size_t)h_nact * np)), gc(h_nact), bt(GW_BT);
        hipLaunchKernelGGL(gw_form_kernel<T>, gp, bt, 0, c->st, a, act, wa);
        if (n1 > 0) {
            hipLaunchKernelGGL(gw_resid_kernel<T>, gc, bt, 0, c->st, a, act, wa);
            hipLaunchKernelGGL(gw_psolve_kernel<T>, gp, bt, 0, c->st, a, act, wa);
            hipLaunchKernelGGL(gw_start_kernel<T>, gp, bt, 0, c->st, a, act, wa);
        }
        if (n0 > 0) {
            for (int kk = 1; kk <= maxcol; ++kk) hipLaunchKernelGGL(gw_mgs_kernel<T>, gp, bt, 0, c->st, a, act, wa, kk);
            hipLaunchKernelGGL(gw_mgs_kernel<T>, gp, bt, 0, c->st, a, act, wa, 0);
            hipLaunchKernelGGL(gw_state_kernel<T>, gc, bt, 0, c->st, a, act, wa);
            hipLaunchKernelGGL(gw_finish_kernel<T>, gp, bt, 0, c->st, a, act, wa);
        }
    }
    for (long tick = 0; !wide && tick < max_ticks; ++tick) {
        hipLaunchKernelGGL(gmres_compact_kernel<false>, dim3(1), dim3(1024), 0, c->st, a.st, count, (int)rows_per, R, act, zrow, (WState*)nullptr, nact);
        if (maus_d2h(c, &h_nact, nact, sizeof(int), c->st)) return -1;
        HIPCHK(c, hipStreamSynchronize(c->st));
        if (h_nact <= 0) break;
        if (c->csr) csr_product(c, a, zrow, act, h_nact);
        else if constexpr (CPLX) {                                 // the dense products: complex only (the rule)
        if (Hdense) {
            ProfScope ps(c, KC_VEC, 0, 16.0 * h_nact * (double)n * n);
            hipLaunchKernelGGL(gemv_dense_kernel, dim3((n + 15) / 16, h_nact), dim3(GT), 0, c->st, a, act, zrow);
        } else
        if (tick == 0 && rhs_mode == 1 && h_nact > 33) {
            // The first product of a linear system is A x0 with x0 = b for EVERY candidate (AMS:85: x0 = b; the shift and psi come in
            // behind the product): 33 rows of it -- enough for the kernel family of the full product, so the same bits (round 4:
            // tests/test_gpu_kernels.py, rows do not depend on the batch) -- and a copy for the others, instead of the same
            // row of a 512-row product 512 times.
            { ProfScope ps(c, KC_GEMM, 8.0 * 33 * (double)n * n, 16.0 * ((double)n * n + 2.0 * 33 * n));
              maus_zgemm_launch_idx(c->st, 33, n, n, a.Vb, n, 0, c->A, n, 0, a.Y, n, 0, 1.0, 0, 1, 1, false, false, zrow, act); }
            hipLaunchKernelGGL(bcast_row_kernel, dim3((n + 255) / 256, h_nact - 33), dim3(256), 0, c->st, a.Y, n, act, 33);
        } else
        {
            // A candidate's product must not depend on how many others are still active.  The launcher takes the DMA-staged 3M
            // kernel from 33 rows on (K a multiple of 8, K >= 64) and 4M kernels below, and the two round differently: where the
            // 3M kernel applies, a product of fewer rows is padded to 33 with copies of its first row, so every product of a
            // solve -- alone or in any batch -- comes from the same kernel, whose rows do not depend on one another.
            int m = h_nact;
            if (m < PAD_ROWS && (n % 8) == 0 && n >= 64) {
                hipLaunchKernelGGL(gmres_pad_rows_kernel, dim3(1), dim3(64), 0, c->st, act, zrow, h_nact, PAD_ROWS);
                m = PAD_ROWS;
            }
            ProfScope ps(c, KC_GEMM, 8.0 * m * (double)n * n, 16.0 * ((double)n * n + 2.0 * m * n));
            maus_zgemm_launch_idx(c->st, m, n, n, a.Vb, n, 0, c->A, n, 0, a.Y, n, 0, 1.0, 0, 1, 1, false, false, zrow, act);
        }
        }
        { ProfScope ps(c, Bound<T>::KC_POST, 0, sizeof(T) * (double)h_nact * (double)n * (R + 4));
          if (n <= 4 * GT) hipLaunchKernelGGL((gmres_post_kernel<T, 4>), dim3(h_nact), dim3(GT), 0, c->st, a, act);
          else if (n <= 16 * GT) hipLaunchKernelGGL((gmres_post_kernel<T, 16>), dim3(h_nact), dim3(GT), 0, c->st, a, act);
          else if (n <= 32 * GT) hipLaunchKernelGGL((gmres_post_kernel<T, 32>), dim3(h_nact), dim3(GT), 0, c->st, a, act);
          else if (n <= 64 * GT) hipLaunchKernelGGL((gmres_post_kernel<T, 32, 2 * GT>), dim3(h_nact), dim3(2 * GT), 0, c->st, a, act);
          else hipLaunchKernelGGL((gmres_post_stream_kernel<T, 4 * GT>), dim3(h_nact), dim3(4 * GT), 0, c->st, a, act); }
    }
    hipLaunchKernelGGL(gmres_finish_kernel<T>, dim3(count), dim3(GT), 0, c->st, a, c->W, c->ldp, outs, outs + count, outs + 2 * count);
    if (maus_d2h(c, info_out, outs, sizeof(int) * count, c->st)) return -1;
    if (maus_d2h(c, inner_out, outs + count, sizeof(int) * count, c->st)) return -1;
    if (maus_d2h(c, status, outs + 2 * count, sizeof(int) * count, c->st)) return -1;
    if (jacobi_out) { if (maus_d2h(c, jacobi_out, jac, sizeof(int) * count, c->st)) return -1; }
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    return 0;
}

int maus_gmres_run(maus_ctx* c, const int* slots, int count, const double* shift, const double* psi, int rhs_mode,
                   const int32_t* use_jacobi, double rtol, int restart, int maxiter, int32_t* info_out, int32_t* inner_out,
                   int32_t* status, const c128* Hdense, long ldh, long strideH, int32_t* jacobi_out, bool real) {
    if (real) {
        // the caller decided by maus_real_rule for the whole call; what the rule relies on is checked again where it is used
        if (Hdense || !c->csr || rhs_mode != 1 || !c->Acsr.rval || !c->Adiag_r || !c->b_r || c->b_rn != c->rows)
            FAIL(c, "maus_gmres: the real path was chosen without its real copies");
        return gmres_run_t<double>(c, slots, count, shift, psi, rhs_mode, use_jacobi, rtol, restart, maxiter, info_out, inner_out,
                                   status, nullptr, 0, 0, jacobi_out);
    }
    return gmres_run_t<c128>(c, slots, count, shift, psi, rhs_mode, use_jacobi, rtol, restart, maxiter, info_out, inner_out,
                             status, Hdense, ldh, strideH, jacobi_out);
}

// The rule of the real path, stated once: maus_gmres decides by it and maus_real_plan reports it.  All or nothing per call.
int maus_real_rule(const maus_ctx* c, int rhs_mode, int count, const double* shift) {
    if (c->real_method != 1) return MAUS_REAL_METHOD_OFF;
    if (!c->csr || c->rows != c->cols) return MAUS_REAL_NOT_CSR;         // no square CSR matrix bound: no real copies either
    if (!c->A_real) return MAUS_REAL_MATRIX_COMPLEX;
    if (rhs_mode != 1) return MAUS_REAL_RHS_ROWS;
    if (!c->b || !c->b_real) return MAUS_REAL_RHS_COMPLEX;
    if (count > 0 && !maus_real_flagged(shift, (size_t)count)) return MAUS_REAL_SHIFT_COMPLEX;
    return MAUS_REAL_OK;
}

int maus_gmres_set_method(maus_ctx* c, int method) {
    if (!c) return -1;
    if (method != 0 && method != 1) FAIL(c, "maus_gmres_set_method: method must be 0 (default) or 1 (wide)");
    c->gmres_method = method;
    return 0;
}

int maus_gmres_get_method(maus_ctx* c) { return c ? c->gmres_method : -1; }

int maus_real_plan(maus_ctx* c, int rhs_mode, int count, const double* shift, int64_t* out) {
    if (!c) return -1;
    if (count < 0 || (count > 0 && !shift) || !out) FAIL(c, "maus_real_plan: bad arguments");
    const int why = maus_real_rule(c, rhs_mode, count, shift);
    const bool bound = c->csr && c->rows == c->cols;
    out[0] = why == MAUS_REAL_OK;
    out[1] = why;
    out[2] = bound ? maus_gmres_kernel_for(c, c->rows, 1) : -1;                                  // post schedule: 0 register, 1 stream, 2 wide
    out[3] = bound ? (c->Acsr.sell.val ? 3 : c->csr_sched) : 0;                                  // SpMM kernel, as maus_spmm_kernel_for
    out[4] = c->real_allocs;
    out[5] = (c->Acsr.rval ? 8 * std::max(1L, c->Acsr.nnz) : 0) + (c->Acsr.sell.rval ? 8 * c->Acsr.sell.padded : 0)
             + (c->Adiag_r ? 8L * c->rows : 0) + (c->b_r ? 8L * c->b_rn : 0);                     // bytes of the real copies held
    return 0;
}

int maus_gmres_kernel_for(maus_ctx* c, int n, int csr) {
    if (!c) return -1;
    if (n <= 0 || n > maus_sparse_max_n() || (!csr && n > maus_lu_max_n())) FAIL(c, "maus_gmres_kernel_for: bad size");
    if (csr && c->gmres_method == 1) return 2;
    return n <= 64 * GT ? 0 : 1;
}

size_t maus_gmres_wide_bytes_per_candidate(int n) {
    return sizeof(WState) + sizeof(c128) * 3 * (size_t)((n + GW_SPAN - 1) / GW_SPAN) + 512;
}
