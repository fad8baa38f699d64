// The zgemm launchers of zgemm.hip (device pointers; not part of the C ABI), declared once for every translation unit.
// C[M,N] = alpha * opA(A)[M,K] * opB(B)[K,N] + beta * C on `batch` matrices at element strides sA / sB / sC; blay 0: B is
// [k][n], 1: [n][k]; a_rows / c_rows (device int arrays of length M, or null): row gather for A / row scatter for C.
// Which kernel a product runs: zgemm_plan in zgemm.hip, exported as maus_zgemm_plan (include/maus_hip.h).
#pragma once
#include "common.h"

struct maus_ctx;

void maus_zgemm_launch(hipStream_t st, int M, int N, int K, const c128* A, long lda, long sA,
                       const c128* B, long ldb, long sB, c128* C, long ldc, long sC,
                       double alpha, int beta, int batch, int blay, bool conja, bool conjb);
// one row list for every matrix (population slots, Krylov rows)
void maus_zgemm_launch_idx(hipStream_t st, int M, int N, int K, const c128* A, long lda, long sA,
                           const c128* B, long ldb, long sB, c128* C, long ldc, long sC,
                           double alpha, int beta, int batch, int blay, bool conja, bool conjb,
                           const int* a_rows, const int* c_rows);
// one row list per matrix, rows_stride apart (0: the same list for all)
void maus_zgemm_launch_rows(hipStream_t st, int M, int N, int K, const c128* A, long lda, long sA,
                            const c128* B, long ldb, long sB, c128* C, long ldc, long sC,
                            double alpha, int beta, int batch, int blay, bool conja, bool conjb,
                            const int* a_rows, const int* c_rows, long rows_stride);
// LU trailing update on the tile-major workspace (luws.h):  H[rows[m]][ccol + n] -= H[rows[m]][acol + k] * U[brow + k][ccol + n]
void maus_zgemm_launch_lu(hipStream_t st, int M, int N, int K, const c128* H, const c128* U, c128* Hc, long nrows, long stride,
                          int acol, int brow, int ccol, int batch, const int* rows, long rows_stride);
// the product of maus_zgemm_launch_idx for the population products of capi.hip, split over K under maus_few_rows_set_method(ctx, 1)
int maus_zgemm_launch_few(maus_ctx* c, int M, int N, int K, const c128* A, long lda, long sA,
                          const c128* B, long ldb, long sB, c128* C, long ldc, long sC,
                          double alpha, int beta, int batch, int blay, bool conja, bool conjb,
                          const int* a_rows, const int* c_rows);
