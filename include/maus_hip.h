/* libmaus_hip -- C ABI of the MI355X (gfx950) hot path of MAUS.
 *
 * The reference (Kier73/Adaptive-Matrix-Solver, `Adaptive_Matrix_Solver_0.1.py`,
 * cited as AMS:line) is pure Python with no FFI layer; the boundary below is what
 * a ctypes binding of its per-candidate inner loop binds.
 * Each entry point names the reference lines it replaces.
 *
 * Conventions
 *  - Plain pointers and sizes only.  Complex data is interleaved (re, im) double,
 *    i.e. NumPy complex128, C-contiguous (row-major).
 *  - Every function returns 0 on success, <0 on an API/HIP error
 *    (maus_last_error() gives the text).  Nothing throws across the boundary.
 *  - NUMERICAL failures are not errors: they come back per candidate in
 *    `status[]` (0 ok; k>0 exact zero pivot at column k, LAPACK `info`
 *    convention, AMS:59 -> LinAlgError; -1 non-finite input matrix/rhs, -2
 *    non-finite result, AMS:94-95 -> ValueError), so the Python retry ladder
 *    (AMS:98-104) is reproduced exactly.
 *  - Host buffers are caller-owned and are only read / written by plain memcpy
 *    while a call is in progress: every transfer goes through a pinned buffer
 *    of the context (a caller array handed to the runtime would stay
 *    registered with the driver and stall the GPU queues when the caller frees
 *    it).  Device buffers are owned by the context.
 *  - One context per GPU, not thread-safe; calls are synchronous as seen by the
 *    caller (work is enqueued on the context's own HIP stream and joined before
 *    results are returned).
 *  - A "slot" is a row of the device-resident population arrays (one candidate
 *    vector per contiguous row).
 */
#ifndef MAUS_HIP_H
#define MAUS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct maus_ctx maus_ctx;

/* population arrays (`which`) */
enum { MAUS_POP_X = 0,   /* v_k (eig) / x_k (linear) / right_v_k (SVD)  AMS:120-121 */
       MAUS_POP_U = 1,   /* u_k (SVD)                                    AMS:121 */
       MAUS_POP_W = 2,   /* raw solver result new_vec_raw                AMS:278 */
       MAUS_POP_Y = 3 }; /* scratch: last A@X product */

/* residual kinds (AMS:295-301) */
enum { MAUS_EIG = 1, MAUS_LINEAR = 2, MAUS_SVD = 3 };

/* perturbation modes of the dense regulariser (AMS:49-50) */
enum { MAUS_PERT_NONE = 0,      /* reg = psi*I only (the 0.15*psi random term is dropped; the caller still
                                   advances the NumPy stream)                                              */
       MAUS_PERT_UNIFORM = 1,   /* caller supplies the two rand(N,N) draws; device forms
                                   ((U1-.5)+i(U2-.5))*psi*0.15 with the reference's rounding order       */
       MAUS_PERT_MT19937 = 2 }; /* device regenerates the legacy NumPy MT19937 stream from a supplied
                                   624-word state per candidate (bit-identical draws)                    */

/* MAUS_PERT_MT19937 descriptor: legacy NumPy RandomState (np.random.get_state()) + consumption pattern.
 * words_per_candidate and lead_words must be multiples of 2*n*n (one rand(N,N) draw). */
typedef struct {
    uint32_t key[624];
    int32_t pos;                    /* 0..624, as returned by get_state() */
    int32_t reserved;
    uint64_t words_per_candidate;   /* 4*n*n per dense attempt (8*n*n when a swallowed GMRES attempt draws first) */
    uint64_t lead_words;            /* words each candidate skips before the draws it uses */
    const int32_t* ordinals;        /* [count] position of each candidate in the run */
} maus_mt_desc;

/* ---- lifecycle ---------------------------------------------------------- */
int maus_ctx_create(int device, maus_ctx** out);
int maus_ctx_destroy(maus_ctx* ctx);
const char* maus_last_error(const maus_ctx* ctx);
/* name_len bytes of device name, CU count, total and free HBM bytes */
int maus_device_info(maus_ctx* ctx, char* name, int name_len, int* cus, size_t* hbm_total, size_t* hbm_free);
/* library ABI version (compile-time constant) */
int maus_abi_version(void);
/* largest n of the direct LU path (maus_shifted_lu_solve, maus_lu_solve_host, maus_lu_reserve) and of both GMRES modes
 * (maus_gmres, maus_gmres_pert) in this build: 16384 */
int maus_lu_max_n(void);

/* ---- problem data (AMS:343, 346: everything is complex128) -------------- */
/* Upload the rows x cols problem matrix.  Replaces passing `current_matrix_A`
 * by reference into every step (AMS:576). */
int maus_set_matrix(maus_ctx* ctx, const double* a_c128, int rows, int cols);

/* ---- sparse problem matrices (AMS:357-358, 380-392: the reference's CSC / spmatrix branch) ---------------------------
 * Upload a rows x cols matrix in CSR form: indptr[rows + 1] (int64, 0 .. nnz, non-decreasing), indices[nnz] (int32, in
 * [0, cols), strictly increasing inside a row) and values[nnz] complex128.  Malformed input returns -1 with a message and
 * leaves the device untouched.  The library keeps A and A^H in CSR (the latter built here) and the diagonal of A; no dense
 * copy is allocated.  Every product with the problem matrix (Rayleigh quotient AMS:264, residuals AMS:295-298, the SVD
 * power step AMS:228 / 240, the GMRES products of AMS:85) then runs as a CSR SpMM, and the direct solve builds H_k
 * = A - lambda_k I + psi_k I (AMS:46-47: no random term) straight from the CSR operand into the LU workspace.  Entry points
 * that need the dense matrix (maus_herm_tridiag, maus_gmres_pert, maus_comm_set_matrix) return an error.  nnz < 2^31.
 * maus_set_matrix replaces a CSR matrix again.
 * maus_matrix_is_sparse: 0 = dense matrix (or none), 1 = CSR with the lane-per-row SpMM schedule, 2 = CSR with the
 * wave-per-row schedule (nnz / rows > 32). */
int maus_set_matrix_csr(maus_ctx* ctx, int rows, int cols, int64_t nnz,
                        const int64_t* indptr, const int32_t* indices, const double* values_c128);
int maus_matrix_is_sparse(maus_ctx* ctx);

/* ---- band solves of a sparse matrix --------------------------
 * maus_sparse_max_n: the largest n of the CSR eigenvalue / linear path (1 << 20); maus_gmres accepts it for a CSR matrix,
 *   the dense modes keep maus_lu_max_n().
 * maus_band_prepare: the ordering perm[n] (a permutation of 0..n-1, checked on the host) of the bound square CSR matrix;
 *   returns kl / ku, the lower / upper half-bandwidths of A[perm][:, perm], computed from the bound pattern.  Bad input
 *   returns -1 and launches nothing.  Binding another matrix drops the ordering.
 * maus_band_reserve: the band workspace for `count` simultaneous solves, sized once as maus_lu_reserve sizes the dense one
 *   (MAUS_BAND_BATCH caps it, default 512); capacity_out (may be NULL): solves it holds.
 * maus_band_solve: the contract of maus_shifted_lu_solve with pert_mode NONE, on H_k = A - shift_k I + psi_k I in band
 *   storage: W[slot] = H_k^-1 (rhs_mode 0: X[slot], 1: b).  status[k]: 0, -1 non-finite H_k or right-hand side, > 0 the
 *   1-based column of the first exact zero pivot in the permuted order (zgbtrf's info), -2 non-finite solution.
 * maus_band_lu_host: `count` band matrices given in LAPACK's zgbtrf input layout, ab[count][n][ldab] (column j holds
 *   ldab = 2 kl + ku + 1 entries, A(i, j) at row kl + ku + i - j; the first kl rows are workspace), and b[count][n]:
 *   x_out[count][n], ipiv_out[count][n] (may be NULL; LAPACK's 1-based rows) and info_out[count] with the status values
 *   above.  Test entry point.
 * maus_band_workspace_allocs: (re-)allocations of the band workspace on this context.
 * maus_band_set_method: which kernels maus_band_solve, maus_band_reserve and maus_band_lu_host run on this context --
 *   0 the column kernel (one workgroup per matrix walks the columns; the default), 1 the blocked method (zgbtrf's
 *   schedule in blocks of 16 columns, every step a launch over (matrix, tile)), 2 the tiled method (the blocked
 *   schedule with the block row and the trailing update as launches of their own over (column tile, row tile); blocks of
 *   16, 8 or 4 columns by kl), 4 the wide method (zgbtrf's two levels: outer blocks of 64 columns factored by the
 *   tiled steps, then one rank-64 update of everything right of the block on the fp64 MFMA pipe), 8 the narrow method
 *   (the column kernel's steps by one wave per matrix, the live columns of the band in an LDS ring that the band streams
 *   through in chunks of 16 columns; same workspace as method 0).  There are no methods 3, 5, 6 and 7.
 *   Under method 1 a band with kl < 16 or kl > 1024 still runs the column kernel, under method 2 one with kl < 16 or
 *   kl > 4096; under method 4 a band with 64 <= kl <= 4096 runs wide, one with 16 <= kl < 64 exactly what method 2 runs
 *   and every other the column kernel; under method 8 a band with kl <= 15 and kl + ku <= 31 runs narrow and every other
 *   the column kernel.  For a band that both take, methods 1 and 2 give the same bits; method 8 gives the bits of method
 *   0 (x, ipiv, info and status) for every band.  The method outlives the bound matrix; same status contract in every
 *   method.
 * maus_band_get_method: the current method.
 * maus_band_kernel_for: what (n, kl, ku) runs under the current method: returns 0 (column kernel), 1 (blocked), 2 (tiled),
 *   4 (wide) or 8 (narrow); nb_out (may be NULL): the block width (wide: of the inner steps), 1 for the column kernel and
 *   for narrow.
 * maus_band_outer_nb: the width of the outer block (64) where (n, kl, ku) runs wide under the current method, 0 elsewhere.
 * maus_band_plan: the same answers for any `method`, without a context and without opening a device: kind and nb as
 *   maus_band_kernel_for, outer_nb as maus_band_outer_nb, ws_bytes_per_solve the workspace bytes of one solve (what
 *   maus_band_reserve allocates per solve).  Every out pointer may be NULL.  Returns 0, or -1 for a method that
 *   maus_band_set_method refuses or a negative size.
 * maus_band_set_split: a switch beside the method (DESIGN §11 "The split method"): mode 1 solves a band with
 *   1 <= kl + ku <= 31, kl <= 15 and n above one partition length by Gaussian elimination with partial pivoting on the
 *   column-reordered matrix -- the interiors of p column partitions first (one group of lanes per partition, all at once),
 *   then the (p - 1)(kl + ku) separator columns as a reduced band system that the method's own kernels factor and solve.
 *   Every other band runs exactly what the method runs.  part_len: 0 for the rule (64 ceil(sqrt(n (kl + ku)) / 64)), else
 *   the partition length, which must be at least 2 (kl + ku) + 2 -- checked where a band is solved or its workspace sized,
 *   which then fail.  mode 0 (the default) is the method alone, bit for bit.  A mode other than 0 / 1 or a negative
 *   part_len is refused and changes nothing.  Same status contract; a positive status is 1 + the smallest band-order column
 *   with a zero pivot in either phase.  The pivot order differs from zgbtrf's: x agrees to rounding, not bit for bit.
 *   Under the split, maus_band_lu_host's ipiv_out holds, for an interior column, the 1-based row of the matrix that was its
 *   pivot row, and for the separator column (i + 1) part_len - (kl + ku) + t of partition i (0 <= t < kl + ku) the
 *   1-based pivot row, in the reduced system's own row numbering, of its unknown i (kl + ku) + t (zgbtrf's ipiv of that
 *   system: row kl + (i - 1)(kl + ku) + s of it is the s-th leftover row, in row order, of partition i >= 1; the kl
 *   leftover rows of partition 0 come first).
 * maus_band_get_split: returns the mode; part_len_out (may be NULL): the forced partition length, 0 for the rule.
 * maus_band_split_plan: what the split would do with (n, kl, ku) under `method` and part_len, without a context or a
 *   device: takes (0 / 1), the partition length, the number of partitions, the reduced system's order and half-bandwidths,
 *   and the bytes of the split's arrays per solve (what the workspace adds to maus_band_plan's).  Where takes = 0 the rest
 *   are 0.  Every out pointer may be NULL.  Returns 0, or -1 for a bad method, a negative size, or a part_len below
 *   2 (kl + ku) + 2 on a band in the split's range.
 * maus_band_set_real: band solves in real arithmetic (DESIGN §11 "Band solves in real arithmetic"), a switch of its own beside
 *   maus_real_set_method and independent of it.  mode 0 (the default): complex arithmetic, today's path bit for bit.  mode 1:
 *   a maus_band_solve call runs on band storage, right-hand sides and ring slots of doubles when all of these hold -- a
 *   square CSR matrix with an ordering is bound and every stored value has an imaginary part of +-0; rhs_mode is 1 and b is
 *   real in the same sense; every shift of the call has an imaginary part of +-0 (maus_real_values_flagged); and the plan of
 *   the context's method for (kl, ku) is the column kernel or the narrow method, or the split takes the band and its reduced
 *   system's plan is one of those two.  All or nothing per call, also where the call runs in chunks.  Otherwise the call
 *   runs complex as ever: population rows as right-hand sides (eigenvalue problems) and the blocked, tiled and wide kernels
 *   have no real instantiation.  The real kernels are the complex text over T = double: geometry, ownership, pivot rule,
 *   chunks, ring slots, partition lengths and plans are the complex path's, and every operation is the complex one without
 *   the terms that multiply an exact zero.  For finite data x, ipiv, info and status are the complex path's under
 *   array_equal (zeros may differ in sign); a solution of a singular or non-finite system may hold Inf where the complex
 *   path holds NaN, with the same status.  W[slot] receives x with imaginary part +0.0.  No real copy of the operand is
 *   kept (the build kernel reads the real parts of the complex CSR values and of b) and nothing is allocated: the band
 *   workspace is used as doubles.  Counted in the profile class 21 ("band_real") and in no other band class.  Kept across
 *   matrices.  A mode other than 0 / 1 is refused and changes nothing.
 *   maus_band_lu_host follows the switch: under mode 1 it runs real when the plan qualifies and every element of ab and b
 *   handed in has an imaginary part of +-0 -- taken over the whole arrays on the host, fill rows and corners included, so a
 *   caller who leaves complex or NaN-imaginary workspace there gets the complex path.
 * maus_band_get_real: the mode.
 * maus_band_real_plan: what a maus_band_solve call with this rhs_mode and these `count` shifts does on the bound matrix,
 *   ordering and b: out[0] 1 = real, 0 = complex; out[1] MAUS_BAND_REAL_OK or the first condition of the rule that fails;
 *   out[2] the kernel kind as maus_band_kernel_for (0 without an ordering); out[3] 1 where the split takes the band.
 *   maus_band_solve decides by the same function.
 * maus_band_real_kinds: without a context or a device: out[0] 1 when every kernel that an (n, kl, ku) band runs under
 *   (method, split_mode, part_len) has a real instantiation, out[1] the kind as maus_band_plan, out[2] whether the split
 *   takes the band.  Returns 0, or -1 for bad arguments (as maus_band_split_plan). */
/* MAUS_BAND_REAL_NOT_CSR: no square CSR matrix with an ordering is bound; MAUS_BAND_REAL_NO_KERNELS: the method's plan for the
 * band (or for the split's reduced system) is the blocked, tiled or wide method */
enum { MAUS_BAND_REAL_OK = 0, MAUS_BAND_REAL_OFF = 1, MAUS_BAND_REAL_NOT_CSR = 2, MAUS_BAND_REAL_MATRIX_COMPLEX = 3,
       MAUS_BAND_REAL_RHS_ROWS = 4, MAUS_BAND_REAL_RHS_COMPLEX = 5, MAUS_BAND_REAL_SHIFT_COMPLEX = 6, MAUS_BAND_REAL_NO_KERNELS = 7 };
int maus_band_set_real(maus_ctx* ctx, int mode);
int maus_band_get_real(maus_ctx* ctx);
int maus_band_real_plan(maus_ctx* ctx, int rhs_mode, int count, const double* shift_c128, int32_t* out4);
int maus_band_real_kinds(int method, int split_mode, int part_len, int n, int kl, int ku, int32_t* out3);
int maus_sparse_max_n(void);
int maus_band_prepare(maus_ctx* ctx, const int32_t* perm, int n, int* kl_out, int* ku_out);
int maus_band_reserve(maus_ctx* ctx, int count, int* capacity_out);
int maus_band_solve(maus_ctx* ctx, const int* slots, int count, const double* shift_c128, const double* psi, int rhs_mode,
                    int32_t* status);
int maus_band_lu_host(maus_ctx* ctx, int count, int n, int kl, int ku, const double* ab_c128, const double* b_c128,
                      double* x_out_c128, int32_t* ipiv_out, int32_t* info_out);
int maus_band_workspace_allocs(maus_ctx* ctx);
int maus_band_set_method(maus_ctx* ctx, int method);
int maus_band_get_method(maus_ctx* ctx);
int maus_band_kernel_for(maus_ctx* ctx, int n, int kl, int ku, int* nb_out);
int maus_band_outer_nb(maus_ctx* ctx, int n, int kl, int ku);
int maus_band_plan(int method, int n, int kl, int ku, int32_t* kind, int32_t* nb, int32_t* outer_nb,
                   int64_t* ws_bytes_per_solve);
int maus_band_set_split(maus_ctx* ctx, int mode, int part_len);
int maus_band_get_split(maus_ctx* ctx, int* part_len_out);
int maus_band_split_plan(int method, int n, int kl, int ku, int part_len, int32_t* takes, int32_t* part_len_out, int32_t* parts,
                         int32_t* n_red, int32_t* kl_red, int32_t* ku_red, int64_t* ws_bytes_per_solve);

/* Upload b (AMS:146, 275). */
int maus_set_rhs(maus_ctx* ctx, const double* b_c128, int n);

/* ---- device-resident population ----------------------------------------- */
int maus_pop_reserve(maus_ctx* ctx, int capacity);
int maus_pop_capacity(maus_ctx* ctx);
/* host (count x len, C-contiguous complex128) -> slots[i] of array `which`; len = vector length */
int maus_pop_put(maus_ctx* ctx, int which, const int* slots, int count, const double* host_c128, int len);
int maus_pop_get(maus_ctx* ctx, int which, const int* slots, int count, double* host_c128, int len);

/* Device address of population array `which` (capacity x ld complex128 elements, row-major) after joining the context's
 * stream -- for a caller that exchanges candidate rows between GPUs with its own collective library (RCCL through
 * torch.distributed in dist.py) without bouncing them through the host.  The pointer is invalidated by
 * maus_pop_reserve / maus_set_matrix with a different vector length. */
int maus_pop_device_ptr(maus_ctx* ctx, int which, void** ptr_out, long* ld_out, int* capacity_out);

/* Device-side copy of the rows `slots` from population array which_src to which_dst (no host traffic).  Used to
 * snapshot the candidates of a speculative batch before the relaxed update overwrites them, so that a run can be
 * restarted behind an RNG event (E4 tiny-norm re-initialisation, AMS:283) exactly as the sequential reference
 * would continue. */
int maus_pop_copy(maus_ctx* ctx, int which_dst, int which_src, const int* slots, int count);

/* ---- device-backed history (AMS:126, 303-304: param_history keeps every iterate of every candidate) ---- */
/* Append the first `len` entries of rows `slots` of population array `which` to the context's history store
 * (device-to-device, no host traffic); the rows get consecutive indices starting at *first_index_out.  Beyond
 * MAUS_HIST_DEVICE_BYTES (default 8 GiB) the oldest rows are spilled to host memory.  maus_hist_get fetches rows by
 * index (from wherever they live) into host_c128[count][len]; maus_hist_clear drops everything. */
int maus_hist_append(maus_ctx* ctx, int which, const int* slots, int count, int len, int64_t* first_index_out);
int maus_hist_get(maus_ctx* ctx, const int64_t* indices, int count, int len, double* host_c128);
int maus_hist_clear(maus_ctx* ctx);
/* Generation of the history store: incremented whenever the store is dropped (maus_hist_clear, maus_set_matrix with a
 * different vector length).  A caller that keeps row indices (solver._HistRef) records the generation with them and
 * refuses to resolve an index of an older generation instead of reading somebody else's rows. */
int64_t maus_hist_generation(maus_ctx* ctx);

/* ---- phases of update_solution_step, batched over `count` candidates ---- */
/* Y[slot] = A @ X[slot]; num = vdot(v, A@v), den = vdot(v, v)      AMS:264-268.
 * num_c128: count complex; den_c128: count complex (imag is the rounded sum, ~0). */
int maus_matvec_rayleigh(maus_ctx* ctx, const int* slots, int count, double* num_c128, double* den_c128);

/* Psi-regularised direct solve, one LU per candidate            AMS:44-59 (+270):
 *   H_k = (A - shift_k I) + (psi_k I + pert_k);   solve H_k w = rhs;   W[slot] <- w
 * rhs_mode 0: rhs = X[slot] (eig, AMS:271); 1: rhs = b (linear, AMS:275).
 * shift_c128[count] complex (0 for linear), psi[count] real.
 * pert: see MAUS_PERT_*; `pert_data` is
 *   UNIFORM: host double[count][2][n][n]   (U1 then U2 per candidate)
 *   MT19937: host maus_mt_desc (below): the NumPy state at the start of the run and, per candidate,
 *            its ordinal in the run; candidate i uses the 4*n*n words starting at
 *            lead_words + ordinals[i] * words_per_candidate
 * status[count]: see conventions. */
int maus_shifted_lu_solve(maus_ctx* ctx, const int* slots, int count, const double* shift_c128,
                          const double* psi, int rhs_mode, int pert_mode, const void* pert_data,
                          int32_t* status);

/* Size the LU workspace ONCE for up to `count` simultaneous n x n systems (the reference's sla.solve allocates its
 * copy of H per call, AMS:59; here H_k of a whole batch are device-resident, 270 MB each at n = 4096, and re-allocating
 * ~100 GB costs seconds).  Capped by 80 % of the free HBM and MAUS_LU_BATCH (default 512); larger batches run in
 * chunks.  The workspace never shrinks; a batch beyond it makes it grow once, to the limit.  capacity_out (may be NULL):
 * matrices the workspace holds after the call. */
int maus_lu_reserve(maus_ctx* ctx, int n, int count, int* capacity_out);

/* Number of times the LU workspace has been (re-)allocated on this context (measurement: a timed region must not
 * contain one). */
int maus_lu_workspace_allocs(maus_ctx* ctx);

/* Robustness of the small-batch panel (no reference counterpart; the reference contract it protects is that every failed
 * solve surfaces to the retry ladder, AMS:94-104).  For batches that run on one stream the base panel of the LU may
 * spread over several workgroups per matrix that rendezvous once per pivot column; that needs all of them resident
 * at once, which holds only while this context has the device to itself.
 *  - maus_set_shared_device(ctx, 1): the caller knows the device is shared with other processes (several ranks of a
 *    `gloo` rehearsal on one GPU): the multi-workgroup panel is never used.
 *  - A rendezvous that times out marks the matrix (LAPACK-style info = INT_MIN).  The library then repeats the whole
 *    batch with one workgroup per matrix, switches the multi-workgroup panel off for the rest of the context's life and
 *    counts the event (maus_lu_mw_aborts).  If the repeat fails too the call returns -1 (maus_last_error: "LU panel
 *    rendezvous timed out"): a half-factored matrix is never reported as status 0. */
int maus_set_shared_device(maus_ctx* ctx, int shared);
int maus_lu_mw_aborts(maus_ctx* ctx);

/* X[slot] <- (1-alpha) X[slot] + alpha W[slot]; norm_out = ||X||_2; if normalise and
 * norm > 1e-10: X *= 1/norm                                        AMS:280-285.
 * alpha_c128[count] complex.  Slots whose norm test fails are left un-normalised (the
 * host re-initialises them, AMS:283). */
int maus_relax_normalise(maus_ctx* ctx, const int* slots, int count, const double* alpha_c128,
                         int normalise, double* norm_out);

/* residual_k and the finite check                                  AMS:295-301, 319-327.
 * kind EIG: ||A v - lam v||; LINEAR: ||A x - b||; SVD: ||A v - s u|| + ||A^H u - s v||
 * (lam_c128[count]: lambda or sigma+0i).  finite_out[i]=1 iff every entry of the
 * candidate's vectors is finite. */
int maus_residual(maus_ctx* ctx, int kind, const int* slots, int count, const double* lam_c128,
                  double* resid_out, int32_t* finite_out);

/* SVD alternating power step                                       AMS:233-242:
 * t = A v; sigma1 = ||t||; u = t / (sigma1 > 1e-10 ? sigma1 : 1); s = A^H u;
 * sigma2 = ||s||; v = s / (sigma2 > 1e-10 ? sigma2 : 1).
 * Outputs per candidate: norms[4] = {||v_in||, sigma1, ||u||, sigma2}. */
int maus_svd_power_step(maus_ctx* ctx, const int* slots, int count, double* norms_out);
/* The same step in two halves, for callers that run it speculatively over a whole population (the reference steps the
 * candidates one after the other, AMS:574-576, and a collapse -- AMS:229-232, 236-239 -- draws random numbers that the
 * candidates behind it must not have passed): propose computes the norms and leaves the candidates' vectors alone (the
 * proposed u in population array 3, the proposed v in array 2), commit makes the proposal the state of the listed
 * candidates.  maus_svd_power_step = propose + commit of the same list. */
int maus_svd_power_propose(maus_ctx* ctx, const int* slots, int count, double* norms_out);
int maus_svd_commit(maus_ctx* ctx, const int* slots, int count);

/* Hermitian shortcut                                               AMS:165-175:
 * given the eigenvector matrix V (n x n, columns = eigenvectors, uploaded once
 * per matrix version with maus_set_eigvecs) pick argmax_j |v^H V[:,j]| per
 * candidate, copy that column into X[slot], normalise.  idx_out[count]. */
int maus_set_eigvecs(maus_ctx* ctx, const double* v_c128, int n);
int maus_herm_match(maus_ctx* ctx, const int* slots, int count, int32_t* idx_out, double* norm_out);

/* The Hermitian eigendecomposition of AMS:161 (scipy.linalg.eigh = LAPACK zheevr: zhetrd -> dstemr -> zunmtr) with the
 * reduction and the back-transformation on the device, once per matrix:
 *   maus_herm_tridiag        A = Q T Q^H of the context's (Hermitian) matrix, zhetrd('L') semantics and reflector
 *                            conventions; d_out[n] / e_out[n-1]: diagonal / subdiagonal of the real T.  The reflectors stay
 *                            on the device until the back-transformation.  Only the lower triangle and the real part of the
 *                            diagonal are read.  A matrix whose largest entry lies outside [2^-400, 2^400) is reduced as its
 *                            multiple by a power of two (exact; d and e are multiplied back), the bound matrix stays as it is.
 *   maus_herm_tridiag_eig    eigenpairs (lambda, Z) of T on the device: bisection on the Sturm count, eigenvectors from the
 *                            twisted factorisation of T - lambda I (the getvec step of dstemr), no reorthogonalisation.
 *                            w_out[n] ascending; Z stays on the device for maus_herm_backtransform(ctx, NULL, 0).
 *                            diag_out[3] = {smallest eigenvalue gap / ||T||, largest residual component / ||T||, ||T||}: the
 *                            caller keeps the result only for well separated spectra with rounding-level residuals and
 *                            otherwise solves T on the host (scipy.linalg.eigh_tridiagonal = dstemr, the kernel zheevr uses)
 *                            and passes its Z.
 *   maus_herm_backtransform  V = Q Z (zunmtr semantics) from the real eigenvectors of T -- NULL (the device-resident Z of
 *                            maus_herm_tridiag_eig) or z_real[n][n] row-major (column k = k-th
 *                            eigenvector), or with col_major != 0 column-major as LAPACK returns them -- into the context's
 *                            eigenvector matrix, as if set by maus_set_eigvecs.
 * The first row of V is real (Q e_1 = e_1), LAPACK's phase convention. */
int maus_herm_tridiag(maus_ctx* ctx, double* d_out, double* e_out);
/* Tiles per workgroup (hch) of the reduction's lower-triangle matvec, for tests and timing:
 *   maus_herm_set_chunk   tiles = 0 (the default): the rule -- per column the largest of 16, 8, 4 that still gives 768 workgroups
 *                         for the column's T block rows, 4 where none does.  4, 8 or 16: that value for every column.  Anything
 *                         else is an error that changes nothing.  Kept across matrices.  The results of different values agree to
 *                         rounding, not bit for bit: the order of summation differs.
 *   maus_herm_chunk_plan  what column i of an order-n reduction launches under `forced` (0, 4, 8, 16), without a context or a
 *                         device: T_out = block rows of the 64 x 64 tile grid with rows > i, hch_out = tiles per workgroup,
 *                         ns_out = tile workgroups = sum_{tb < T} (tb / hch + 1).  All three are 0 for i = n - 1 (no matvec).
 *                         -1 for n < 1, i outside [0, n) or another `forced`. */
int maus_herm_set_chunk(maus_ctx* ctx, int tiles);
int maus_herm_chunk_plan(int n, int i, int forced, int* T_out, int* hch_out, int* ns_out);
/* Frees the reflector store / eigenvectors of T that maus_herm_tridiag(_eig) keep for maus_herm_backtransform: for callers that
 * only wanted the tridiagonal matrix or its eigenvalues (AMS:559, 567 reporting prologue; singular values of the start-up diagnostics). */
int maus_herm_release(maus_ctx* ctx);
/* the context's eigenvector matrix back on the host (v_out[n][n] complex128, row-major; tests, users of evolve()'s report) */
int maus_get_eigvecs(maus_ctx* ctx, double* v_c128_out, int n);
int maus_herm_backtransform(maus_ctx* ctx, const double* z_real, int col_major);
int maus_herm_tridiag_eig(maus_ctx* ctx, const double* d, const double* e, int n, double* w_out, double* diag_out);
/* the eigenvalues of T alone (bisection only, no n x n work arrays): singular values through the Hermitian embedding, spectra of
 * the reporting prologue (AMS:559 / 567) */
int maus_herm_tridiag_eigvals(maus_ctx* ctx, const double* d, const double* e, int n, double* w_out);

/* Sparse Hermitian shortcut at any size                            AMS:186-216:
 * eigsh(A, k = min(6, N - 1), which = 'LM', v0 = v_k, tol) is ARPACK's implicitly restarted Lanczos; here it is thick-restart
 * Lanczos (Wu and Simon: the same subspaces for a Hermitian operator) on the bound CSR matrix (maus_set_matrix_csr, square;
 * anything else is an error).  The basis lives on the device as ncv + 1 rows of n; the host solves the projected ncv x ncv
 * problem once per restart and decides (engine.py).  One synchronisation per restart, none per Lanczos step: maus_lanczos_restart
 * returns without one, the sweep that follows it (maus_lanczos_extend) ends in it.
 *   maus_lanczos_begin    room for the basis (1 <= ncv <= min(n, 32)); row 0 = v0_c128[n] / ||v0||.
 *   maus_lanczos_inject   row j = v_c128[n], orthogonalised against rows 0 .. j - 1 (classical Gram-Schmidt, twice) and
 *                         normalised: the vector a run continues from after a breakdown.
 *   maus_lanczos_extend   steps j = j0 .. j1 - 1 (j1 <= ncv): row j+1 = A row j, orthogonalised against rows 0 .. j (twice),
 *                         alpha_out[j - j0] = Re(row j . A row j), beta_out[j - j0] = the norm that is left, row j+1 scaled by
 *                         1 / beta.  A step whose beta is not above tol_abs (breakdown, or non-finite data) leaves a zero row.
 *   maus_lanczos_restart  rows 0 .. keep - 1 <- S^T rows 0 .. m - 1 (s_real[m][keep], the Ritz vectors that are kept), row
 *                         keep <- row m (the residual vector), 1 <= keep < m <= ncv.
 *   maus_lanczos_finish   the k Ritz rows S^T rows 0 .. m - 1 (s_real[m][k], k <= min(m, 8)), orthonormalised, stay resident as k rows
 *                         of n for maus_herm_match_rows until the matrix changes; the basis is freed.  k = 0 (a run that did
 *                         not converge) frees the basis and keeps nothing.
 *   maus_herm_match_rows  AMS:197-202, maus_herm_match for the resident rows: scores vdot(X[slot], row j), the first largest
 *                         |score| as np.argmax, X[slot] <- row j / ||row j||.  idx_out[count], norm_out[count].
 *   maus_get_ritz_rows    the k resident rows on the host (rows_c128_out[k][n]; tests, reports).
 *   maus_lanczos_get_basis rows j0 .. j0 + count - 1 of the live basis on the host (rows_c128_out[count][n], 0 <= j0, 1 <= count,
 *                         j0 + count <= ncv + 1; read-only, for tests); an error without a basis. */
int maus_lanczos_begin(maus_ctx* ctx, const double* v0_c128, int ncv);
int maus_lanczos_inject(maus_ctx* ctx, int j, const double* v_c128);
int maus_lanczos_extend(maus_ctx* ctx, int j0, int j1, double tol_abs, double* alpha_out, double* beta_out);
int maus_lanczos_restart(maus_ctx* ctx, const double* s_real, int m, int keep);
int maus_lanczos_finish(maus_ctx* ctx, const double* s_real, int m, int k);
int maus_herm_match_rows(maus_ctx* ctx, const int* slots, int count, int32_t* idx_out, double* norm_out);
int maus_get_ritz_rows(maus_ctx* ctx, double* rows_c128_out, int k, int n);
int maus_lanczos_get_basis(maus_ctx* ctx, int j0, int count, double* rows_c128_out);

/* Gram block of candidate vectors for the distinctness / redundancy tests      AMS:432-437, 443-451, 509-520:
 * out[i*count + j] = vdot(x_i, x_j) = sum_k conj(x_i[k]) x_j[k] over the first `len` entries of rows `slots`
 * of population array `which` (MAUS_POP_X / MAUS_POP_U).  Replaces the reference's pairwise np.vdot calls
 * between converged candidates; the host keeps the reference's greedy order and thresholds. */
int maus_gram(maus_ctx* ctx, int which, const int* slots, int count, int len, double* out_c128);

/* Batched restarted GMRES with optional Jacobi preconditioner       AMS:60-90 ->
 * scipy/sparse/linalg/_isolve/iterative.py:692-841 (restart 20, MGS, Givens, ptol).
 *   H_k = A - shift_k I + psi_k I (the random term of AMS:49-50 is left out: see maus_gmres_pert); x0 = rhs; W[slot] <- x
 * use_jacobi[count]: 1 -> M = diag(1/diag H_k) (caller applies AMS:65/72 gating via
 * maus_jacobi_check below).
 * info_out: 0 converged, maxiter otherwise (SciPy convention); inner_out: inner iterations.
 * restart: 1 .. 20 (the Krylov basis holds 20 vectors); anything else is an error -- no clamping, the call never runs another
 *   algorithm than the one asked for.  The cycle length is min(restart, n), as in SciPy.  maxiter < 1 counts as 1.
 * Non-finite data: maus_gmres does not scan the matrix or the right-hand sides.  A NaN or Inf in either makes the residual
 *   norm NaN, which passes no exit test: that candidate ends with info = maxiter, status = 0 (at once for a non-finite
 *   right-hand side, after one cycle for a non-finite matrix; SciPy reports the same after maxiter cycles of NaN), W[slot] then
 *   holds x0 or NaN.  status is never -1 here; -2: info = 0 although x is not finite (kept for the callers' AMS:94 test: with
 *   a finite ||b||^2 a converged residual implies a finite H x, so no finite system is known to reach it).
 * Range: norms are plain sums of squares (no scaling): right-hand sides and matrices must keep ||b||^2, ||M r||^2 and the
 *   squares of the Krylov vectors inside the double range -- entries of b between 1e-150 and 1e+150 in magnitude at unit-scale
 *   matrices; tested at |b| ~ 1e+-120.  Beyond that the norms overflow or underflow and the outcome is info = maxiter.
 * A candidate's x, info and inner count do not depend on the batch it is solved in (bit for bit): SpMM rows are independent,
 *   and a dense product of fewer than 33 rows is padded to 33 where the zgemm launcher would otherwise change from its 3M to its
 *   4M kernels (n a multiple of 8, n >= 64). */
int maus_gmres(maus_ctx* ctx, const int* slots, int count, const double* shift_c128, const double* psi,
               int rhs_mode, const int32_t* use_jacobi, double rtol, int restart, int maxiter,
               int32_t* info_out, int32_t* inner_out, int32_t* status);
/* The same solver against the reference's FULL H_solve of the GMRES branch (AMS:49-52, 89):
 *   H_k = A - shift_k I + psi_k I + 0.15 psi_k ((U1-.5) + i(U2-.5)),
 * materialised per candidate in the LU workspace by the build kernels of maus_shifted_lu_solve (pert_mode / pert_data
 * as there), matvec = one GEMV per candidate against its own H_k.  For escalated psi (retry ladder, large aggression /
 * stuck factors) where the random term is no longer below the rounding of a matvec; maus_gmres is the fast path below
 * that.  want_jacobi[count]: 1 -> use M = diag(1/diag H_k) provided the AMS:67-72 gate holds on diag(H_k) (evaluated on
 * the device; jacobi_out[count], may be NULL, reports whether it was used).  status -1: non-finite H_k or rhs (this entry
 * point scans both while it builds H_k, the AMS:94 analogue; maus_gmres never reports -1).  restart and the range of the data
 * as for maus_gmres.  A batch beyond the LU workspace capacity runs in chunks; a candidate's result does not depend on the
 * batch (one GEMV per candidate). */
int maus_gmres_pert(maus_ctx* ctx, const int* slots, int count, const double* shift_c128, const double* psi,
                    int rhs_mode, const int32_t* want_jacobi, int pert_mode, const void* pert_data,
                    double rtol, int restart, int maxiter,
                    int32_t* info_out, int32_t* inner_out, int32_t* status, int32_t* jacobi_out);
/* The schedule of maus_gmres's post step (scale, Gram-Schmidt, rotations, exits) for a CSR-bound matrix.
 *   maus_gmres_set_method  0 (the default): one workgroup per candidate holds or streams that candidate's vectors.
 *                          1 (wide): the entries of n are split over workgroups of 512, every reduction goes through per-piece
 *                          partial sums joined in one fixed order, about col + 6 launches per tick over the whole device.  The
 *                          algorithm, its exits and the status contract are the same; the dot products are summed in another
 *                          order, so x agrees with method 0 to rounding, not bit for bit.  A candidate's x, info and inner count
 *                          still depend on its own data and on n alone.  Under method 1 EVERY CSR-bound maus_gmres runs the wide
 *                          step, at any n >= 1; dense matrices and maus_gmres_pert ignore the method.  Kept across matrices.
 *   maus_gmres_get_method  the current method.
 *   maus_gmres_kernel_for  what the post step of an n x n matrix (csr != 0: CSR-bound) runs under the current method:
 *                          0 a register kernel (n <= 16384), 1 the stream kernel, 2 the wide step. */
int maus_gmres_set_method(maus_ctx* ctx, int method);
int maus_gmres_get_method(maus_ctx* ctx);
int maus_gmres_kernel_for(maus_ctx* ctx, int n, int csr);
/* Real arithmetic for maus_gmres on a real sparse system ("GMRES in real arithmetic").
 *   maus_real_set_method   0 (the default): every solve runs in complex arithmetic, nothing else is allocated.
 *                          1: a maus_gmres call runs on rows of n doubles, with a real copy of the operand values (8 bytes per
 *                          nonzero; the indices are the complex operand's), of the diagonal and of b, when ALL of these hold:
 *                          the matrix is CSR-bound and every stored value has an imaginary part of +0 or -0 (-0.0 counts as
 *                          real; 5e-324 and NaN do not); rhs_mode is 1 and b is real in the same sense; every shift of the call
 *                          has an imaginary part of +-0.  The flags are taken on the host when the arrays are bound.  Otherwise
 *                          the call runs the complex path unchanged: maus_gmres_pert, dense matrices, population rows as
 *                          right-hand sides, one complex shift among the call's.  Same algorithm, exits and status contract,
 *                          both post schedules (maus_gmres_set_method) and both SpMM kernels (maus_spmm_set_method).  For finite
 *                          data x, info, inner and status are those of the complex path bit for bit: every vector operation is
 *                          the complex one without the terms that multiply an exact zero, in the same order, and the one-lane
 *                          state machine is the complex one.  W[slot] receives x with imaginary part +0.0.  For non-finite data
 *                          info and status are the same, and x may hold Inf where the complex path holds NaN (0 * Inf).  Kept
 *                          across matrices; the real copies follow the bound matrix, b, and the SpMM method.
 *   maus_real_get_method   the current method.
 *   maus_real_plan         for the bound matrix and b: what a maus_gmres call with this rhs_mode and these `count` shifts does.
 *                          out[0] 1 = the real path, 0 = the complex path; out[1] MAUS_REAL_OK or the first condition that
 *                          fails; out[2] the post schedule as maus_gmres_kernel_for (-1: no square CSR matrix bound); out[3] the
 *                          SpMM kernel as maus_spmm_kernel_for; out[4] how often a real copy was allocated on this context;
 *                          out[5] the bytes of the real copies held now.  maus_gmres decides by the same function. */
/* MAUS_REAL_NOT_CSR: no square CSR matrix is bound (a dense matrix, or none) */
enum { MAUS_REAL_OK = 0, MAUS_REAL_METHOD_OFF = 1, MAUS_REAL_NOT_CSR = 2, MAUS_REAL_MATRIX_COMPLEX = 3, MAUS_REAL_RHS_ROWS = 4,
       MAUS_REAL_RHS_COMPLEX = 5, MAUS_REAL_SHIFT_COMPLEX = 6 };
int maus_real_set_method(maus_ctx* ctx, int method);
int maus_real_get_method(maus_ctx* ctx);
int maus_real_plan(maus_ctx* ctx, int rhs_mode, int count, const double* shift_c128, int64_t* out6);
/* The flag of the rule on `count` complex values: 1 when every imaginary part has the bits of +0.0 or -0.0, else 0 (-1: bad
 * arguments).  What maus_set_matrix_csr, maus_set_rhs and the shifts of a call are tested with; needs no context. */
int maus_real_values_flagged(const double* values_c128, int64_t count);
/* Y[slot] = A Re(X[slot]) by the SpMM kernels of the real path, the imaginary part +0.0: the product that a real solve runs on
 * its Krylov vectors, on population rows (tests, tools/real_rates.py).  Needs the real copy of the operand (method 1, a square
 * CSR matrix flagged real).  For rows with imaginary parts of +-0 the real part is that of the complex product, bit for bit. */
int maus_real_spmm(maus_ctx* ctx, const int* slots, int count);
/* Dense population products of at most 32 rows: A X of the Rayleigh quotient and the residuals (AMS:264-268, 295-301), the
 * score row conj(X) V of the Hermitian shortcut (AMS:165-175), the two products of the SVD power step (AMS:227-255) and the Gram
 * block of the converged candidates (AMS:432-451).  By default such a product runs ceil(N / 32) workgroups, each walking the whole
 * K alone; from 33 rows on other kernels fill the device.
 *   maus_few_rows_set_method  0 (the default): those kernels, bit for bit.  1 (split-K): K is cut into S slices, every (column
 *                          tile, slice) is a workgroup that writes its partial sums to a workspace of the context, and a second
 *                          launch adds the slices of an element in the order 0 .. S - 1 and applies alpha / beta.  Same four real
 *                          products per complex one, so the same componentwise bound, with other rounding than method 0; two runs
 *                          give the same bits (no atomics, nothing waits).  S depends on (N, K, layout) only, so a candidate's
 *                          row does not depend on how many others are multiplied with it.  `slices` 0: the library's rule;
 *                          1..32: that many slices (tests, timing), reduced so that none is shorter than 16; 1 is the default
 *                          kernels.  Applies to products with M <= 32 in dot-product layout or with a conjugated operand; plain
 *                          products, 33 rows and more, CSR-bound matrices, the GMRES products (padded to 33 rows so that an
 *                          iterate does not depend on the batch), the LU, band and Lanczos paths and maus_herm_match_rows never
 *                          take it.  Kept across matrices.  Anything else than 0 / 1, or slices outside 0..32: an error.
 *   maus_few_rows_get_method  the current method.
 *   maus_few_rows_kernel_for  what an M x N x K product of that form runs under the current method: 0 the default kernels
 *                          (slices_out = 1), 1 split-K with S in slices_out.  Host arithmetic, no launch.
 *   maus_few_rows_plan     the same for a given (method, slices), without a context or a device; -1 for bad arguments.
 *   maus_few_rows_workspace_allocs  how often the partial-sum workspace was (re)allocated: S * ceil(N / 64) * 32 * 64 complex
 *                          numbers, sized from the call's (S, N) alone, grown on demand, never shrunk. */
int maus_few_rows_set_method(maus_ctx* ctx, int method, int slices);
int maus_few_rows_get_method(maus_ctx* ctx);
int maus_few_rows_kernel_for(maus_ctx* ctx, int M, int N, int K, int b_layout, int conj_a, int conj_b, int* slices_out);
int maus_few_rows_plan(int method, int slices, int M, int N, int K, int b_layout, int conj_a, int conj_b, int* slices_out);
int maus_few_rows_workspace_allocs(maus_ctx* ctx);
/* Which kernel a dense product C[M,N] = op(A)[M,K] op(B)[K,N] on `batch` matrices runs: the library's dispatch rule (zgemm_plan
 * in csrc/zgemm.hip, the one place where it is stated), without a context or a device.
 *   form      MAUS_ZGEMM_ROWS: row-major operands in either B layout with either operand conjugated -- every product outside the
 *             LU factorisation (population products, GMRES, the Hermitian reduction, maus_zgemm_host).  MAUS_ZGEMM_LU: the
 *             trailing updates on the LU's tile-major workspace; plain layout only.
 *   lu_tile   what the environment variable MAUS_LU_TILE selects for the LU form (the library reads it once per process; this
 *             function never does): MAUS_LU_TILE_DEFAULT (unset), MAUS_LU_TILE_64X64, MAUS_LU_TILE_128X64.  Ignored by the rows form.
 * Returns the kernel family -- MAUS_ZGEMM_4M (register-staged, four real products per complex one), MAUS_ZGEMM_3M (register-
 * staged, three) or MAUS_ZGEMM_3M_DMA (three, operands staged by LDS-DMA) -- and the workgroup tile in bm_out x bn_out (either may
 * be NULL).  -1 for bad arguments: an unknown form or tile mode, a size or batch below 1, a layout other than 0 / 1, or a layout
 * or conjugation on the LU form.  (Products of at most 32 rows under maus_few_rows_set_method(ctx, 1): maus_few_rows_plan.) */
enum { MAUS_ZGEMM_ROWS = 0, MAUS_ZGEMM_LU = 1 };
enum { MAUS_LU_TILE_DEFAULT = 0, MAUS_LU_TILE_64X64 = 1, MAUS_LU_TILE_128X64 = 2 };
enum { MAUS_ZGEMM_4M = 0, MAUS_ZGEMM_3M = 1, MAUS_ZGEMM_3M_DMA = 2 };
int maus_zgemm_plan(int form, int lu_tile, int M, int N, int K, int batch, int b_layout, int conj_a, int conj_b,
                    int* bm_out, int* bn_out);
/* Products with a CSR-bound matrix (every one goes through the same launcher: the Rayleigh quotient, the residuals, the SVD power
 * step, the GMRES products, the Lanczos steps).  The lane-per-row schedule (maus_matrix_is_sparse = 1) can read its operand from a
 * second, sliced-ELL copy: rows in slices of 64, slice s as wide as its longest row, entry p of row r at off[s] + 64 p + (r & 63),
 * so that one wave-wide load of the operand is contiguous.  A lane still owns a row and adds its nonzeros in CSR order with the
 * same fused operations onto a zero accumulator: every output element is the number the CSR kernel gives, bit for bit, padding
 * is never read, and a row's product stays independent of the batch.  The CSR arrays stay resident beside the copy.
 *   maus_spmm_set_method   0 (the default): the CSR kernels.  1: the sliced-ELL copy for every operand (A and A^H are judged
 *                          separately) of a matrix of the lane-per-row schedule with nnz > 0 whose padded size sum(64 w_s) is at
 *                          most fill_cap_percent / 100 * nnz; every other operand runs the CSR kernels as under 0.  A build that
 *                          fails (device memory) is an error that leaves the previous method and cap.
 *                          fill_cap_percent 0: the library's 200 (a cap on memory, 20 bytes per padded slot); 100..1000000 for
 *                          tests and timing.  Another method or cap is an error that changes and launches nothing.  Kept across
 *                          matrices: with a CSR matrix bound the copies are built or freed at once, and maus_set_matrix_csr
 *                          builds them at bind time under method 1; maus_set_matrix, the next bind and maus_ctx_destroy free
 *                          them.  The build is three steps on the device without atomics (slice widths, their scan, the fill):
 *                          the same matrix gives the same arrays.
 *   maus_spmm_get_method   the current method.
 *   maus_spmm_kernel_for   what a product with the bound matrix (adjoint != 0: with A^H) runs under the current method: 0 no CSR
 *                          matrix is bound, 1 the lane-per-row CSR kernel, 2 the wave-per-row CSR kernel, 3 the sliced-ELL kernel.
 *   maus_spmm_plan         the same rule for a (method, fill_cap_percent), a matrix of `rows` rows and nnz entries and an
 *                          operand of it (A or A^H) with `padded` sliced-ELL slots, without a context or a device: kind_out =
 *                          1 / 2 / 3 as above.  `rows` is the row count of A for both operands: the schedule belongs to the
 *                          matrix (maus_matrix_is_sparse, nnz > 32 rows of A: a wave per row), the CSR kernels run A and A^H
 *                          under it, and only a lane-per-row matrix takes copies.  -1 for bad arguments (method, cap, rows < 1,
 *                          nnz < 0, padded < 0).
 *   maus_spmm_sell_info    what is resident for that operand: slices, padded slots, bytes (values, indices, row lengths and
 *                          slice offsets).  All zeros when the operand has no sliced-ELL copy.  Any of the three may be NULL. */
int maus_spmm_set_method(maus_ctx* ctx, int method, int fill_cap_percent);
int maus_spmm_get_method(maus_ctx* ctx);
int maus_spmm_kernel_for(maus_ctx* ctx, int adjoint);
int maus_spmm_plan(int method, int fill_cap_percent, int rows, int64_t nnz, int64_t padded, int* kind_out);
int maus_spmm_sell_info(maus_ctx* ctx, int adjoint, int* slices, int64_t* padded, int64_t* bytes);
/* AMS:67-72 gate: ok[i]=1 iff all 1/diag(H_k) finite and all |diag(H_k)| > 1e-12 */
int maus_jacobi_check(maus_ctx* ctx, int count, const double* shift_c128, const double* psi, int32_t* ok);

/* ---- population sharding over the GPUs of one node: RCCL over xGMI ------------------------------------------------
 * No reference counterpart: AMS:574-576 steps the candidates in one sequential loop.  Within an iteration a candidate's
 * step reads only (A, b, strategy) and its own state (AMS:576), so one process per GPU steps a contiguous block of the
 * active candidates and the only exchange is an all-gather -- of the per-candidate scalar records the host bookkeeping
 * consumes (AMS:424-475, 504-549: residual, stuckness, weight, status ...) and of the rows the owners updated.  librccl is
 * loaded on first use (dlopen); a process that never shards never needs it.  All calls are collective: every rank of
 * the communicator makes the same call with the same sizes.
 *   maus_device_count        HIP devices visible to this process (0 without a GPU; never fails).
 *   maus_comm_unique_id      ONE rank creates the 128-byte id (ncclGetUniqueId) and hands it to the others by any means
 *                            (dist.py: a socket on MASTER_ADDR).
 *   maus_comm_init           ncclCommInitRank on the context's device; one communicator per context.
 *   maus_comm_allgather_records   host buffers: recv[r] <- rank r's send (bytes_per_rank each), rank order.
 *   maus_comm_allgather_rows      device to device on population array `which`: slots[] lists the slots of every stepped
 *                            candidate grouped by owner rank (counts[r] per rank, the same list on every rank); on return
 *                            every rank holds every owner's rows.
 *   maus_comm_bcast          host buffer from `root` to all (start-up diagnostics, eigenvalues: computed by rank 0 only).
 *   maus_comm_bcast_eigvecs  the eigenvector matrix of the Hermitian shortcut (AMS:161; maus_set_eigvecs on `root` only),
 *                            device to device.
 *   maus_comm_set_matrix     maus_set_matrix for a sharded run (A replicated): `root` uploads `a` from the host, the
 *                            other ranks (a may be NULL there) receive it device to device; the root's failure is
 *                            everybody's.  Replaces N staged host copies of AMS:343's matrix by one.
 *   maus_comm_stats          collectives issued, payload bytes, host wall ms inside them (reset != 0 zeroes them). */
#define MAUS_COMM_ID_BYTES 128
int maus_device_count(void);
int maus_comm_unique_id(char* id_out /* MAUS_COMM_ID_BYTES */);
int maus_comm_init(maus_ctx* ctx, int rank, int world, const char* id /* MAUS_COMM_ID_BYTES */);
int maus_comm_destroy(maus_ctx* ctx);
int maus_comm_info(maus_ctx* ctx, int* rank_out, int* world_out);
int maus_comm_allgather_records(maus_ctx* ctx, const void* send, size_t bytes_per_rank, void* recv);
int maus_comm_allgather_rows(maus_ctx* ctx, int which, const int* slots, const int* counts, int len);
int maus_comm_bcast(maus_ctx* ctx, void* host_buf, size_t bytes, int root);
int maus_comm_bcast_eigvecs(maus_ctx* ctx, int n, int root);
int maus_comm_set_matrix(maus_ctx* ctx, const double* a, int rows, int cols, int root);
int maus_comm_stats(maus_ctx* ctx, long* calls_out, double* bytes_out, double* ms_out, int reset);

/* ---- plain batched GEMM on the context's stream (tests, Gram blocks) ----- */
/* C[M,N] = alpha * opA(A)[M,K] * opB(B) + beta * C, host in/out, row-major complex128.
 * b_layout 0: B is K x N; 1: B is N x K (dot-product form).  conj flags apply to A / B. */
int maus_zgemm_host(maus_ctx* ctx, int M, int N, int K, const double* A, const double* B, double* C,
                    int b_layout, int conj_a, int conj_b, double alpha, int beta);
/* LU factor + solve of `count` dense n x n systems given on the host (tests):
 * a_c128[count][n][n], b_c128[count][n] -> x_c128[count][n], status[count]. */
int maus_lu_solve_host(maus_ctx* ctx, int count, int n, const double* a_c128, const double* b_c128,
                       double* x_c128, int32_t* status, int32_t* ipiv_out /* count*n or NULL */);

/* ---- measurement --------------------------------------------------------- */
/* HIP-event timing on the context's stream. */
int maus_timer_start(maus_ctx* ctx);
int maus_timer_stop(maus_ctx* ctx, float* ms_out);
/* Per-kernel-class accounting (event pairs around each launch of the class while enabled).
 * classes: 0 zgemm (LU trailing update with K>=256 / A@X), 1 lu_panel, 2 trsm, 3 (unused since round 2: row-swap sweeps), 4 build_H, 5 backsolve,
 * 6 vector ops, 7..10 zgemm inside the LU recursion with K = 128 / 64 / 32 / 16, 11 CSR products, 12 band solves (the
 * column kernel and the narrow method: same flops and bytes),
 * 13 lanczos (reorthogonalisation, restart, match of the sparse Hermitian shortcut), 14 band solves by the blocked method
 * (maus_band_set_method; bytes: the band moved once per block step over the full reach kl + ku, not an MFMA class),
 * 15 band solves by the tiled method (bytes: as 14 plus L21 once per column tile of the trailing update)
 * 16 band solves by the wide method (bytes, an upper end: the band once per outer block of 64 columns over the full reach,
 *    LW once per column tile of the outer update, and the inner steps' bytes inside the block)
 * 17 the wide GMRES post step (maus_gmres_set_method; one bracket per tick around all its launches; flops 0, bytes 64 n per
 *    candidate and Gram-Schmidt column plus the form, tail, finish and new-cycle passes)
 * 19 the GMRES post step of the real path (maus_real_set_method), under either schedule: the brackets of class 6 / 17 with
 *    half the bytes; 20 the CSR products of the real path (12 bytes per nonzero or padded slot, 16 n per row).  Classes 6, 11
 *    and 17 count nothing of a call that runs real. */
/* on = 1: event pairs around every launch of every class; on = 2: around the K>=256 zgemm launches only (class 0;
 * long kernels, so cheap enough for a timed region -- full bracketing costs 3-5 % of throughput; MAUS_PROF_STRIDE
 * can thin them out, each sample then stands for `stride` launches); 0: off */
int maus_profile_enable(maus_ctx* ctx, int on);
int maus_profile_read(maus_ctx* ctx, int klass, int* launches, double* total_ms, double* flops, double* bytes);
/* ms during which at least one bracketed launch of the class was executing (union of their intervals over all
 * streams; equals total_ms when nothing overlaps) */
int maus_profile_union_ms(maus_ctx* ctx, int klass, double* union_ms);
int maus_sync(maus_ctx* ctx);

/* ---- legacy NumPy MT19937 stream helpers (host side) ----- */
/* Advance a 624-word MT19937 key + position by `nwords` 32-bit outputs without
 * materialising them (GF(2) jump polynomial; cached per nwords). */
int maus_mt19937_jump(uint32_t* key624, int32_t* pos, uint64_t nwords);

/* ---- candidate vectors drawn on the device from the NumPy stream (AMS:129-143, 544) ------------------------------
 * A new candidate's vector is normalise(np.random.rand(N) + 1j*np.random.rand(N)): two consecutive rand(N) draws, 4N words of
 * the legacy stream.  maus_pop_draw regenerates `count` such pairs on the device, bit for bit, from the state in `desc`
 * (desc->ordinals[k] = index of pair k in the stream counted from that state, need not be contiguous;
 * desc->words_per_candidate = 4*len, desc->lead_words = 0) and writes them into rows slots[k] of population array `which`.
 * The caller advances its own stream (maus_mt19937_jump by 4*len words per pair consumed).
 *   kinds[k]  MAUS_DRAW_RAW:  row = U1 + i U2, norm_out[k] = its 2-norm.
 *             MAUS_DRAW_UNIT: row = ((U1 + i U2) * (1 / norm)) * scale[k] component by component (NumPy's v / np.linalg.norm(v)
 *                             multiplies by the reciprocal); norm_out[k] = the norm before scaling.
 *             MAUS_DRAW_NORM: nothing is written and slots[k] is ignored; norm_out[k] = ||((U1 - .5) + i (U2 - .5)) * scale[k]||.
 *   scale     NULL: 1.0 for every draw.   substreams  0: the library's rule; 1..64 forces the sub-stream count (tests, timing).
 * A row's bits and norm_out depend on the state, the ordinal, the kind and the scale only: not on the sub-stream count, the
 * other draws of the call or the slot.  The squared norm is summed in chunks of 4992 elements in a fixed order, so it agrees
 * with NumPy's to rounding ((len + 2) 2^-53 relative), not bit for bit.  Elements of the row past `len` and all other rows
 * are untouched; the kept-product stamps are dropped.  len from maus_pop_draw_min_len() (1024) to maus_sparse_max_n(), at
 * most the population's row length; a shorter or longer len is an error.
 * maus_pop_draw_plan: the generator plan of such a call without a context or a device: S sub-streams of E elements per draw,
 * ngen = 2 * count * S generators, generator (k, sb, part) at index (k * S + sb) * 2 + part (part 0 = U1, 1 = U2) starts at
 * stream word 624 * ((2 * ordinals[k] + part) * dj + sb * dj2 + extra) + rpos counted from word 0 of the state's block;
 * extra_out / rpos_out (either may be NULL) are filled when ngen <= cap.  -1 for bad arguments. */
enum { MAUS_DRAW_RAW = 0, MAUS_DRAW_UNIT = 1, MAUS_DRAW_NORM = 2 };
#define MAUS_POP_DRAW_MIN_LEN 1024
int maus_pop_draw_min_len(void);
int maus_pop_draw(maus_ctx* ctx, int which, int len, int count, const int32_t* slots, const int32_t* kinds, const double* scale,
                  const maus_mt_desc* desc, int substreams /* 0 = the rule */, double* norm_out);
int maus_pop_draw_plan(int len, int count, const int32_t* ordinals, int pos, int substreams, int* s_out, int64_t* e_out,
                       int* ngen_out, int64_t* dj_out, int64_t* dj2_out, int32_t* extra_out, int32_t* rpos_out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* MAUS_HIP_H */
