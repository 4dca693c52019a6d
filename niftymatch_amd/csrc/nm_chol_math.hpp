// nm_chol_math.hpp -- the written-order Cholesky solve of a symmetric positive definite system, shared by the mosaic
// adjustment (nm_mosaic_adjust.hip) and the exposure gain solve (nm_mosaic_exposure.hip), device kernels and host twins
// alike. The system is M[N][ld] row-major fp64, ld > N: columns 0 .. N-1 hold the matrix (both triangles), column N the
// right-hand side. Left-looking by columns j = 0 .. N-1; element i of column j (i = j .. N; i = N is the right-hand side,
// whose row is the forward substitution) is ONE chain
//     v = M[j][i];  v = fma(-M[k][i], M[j][k], v) for k = 0 .. j-1 in order
// then M[j][j] = sqrt(v) for i = j (not positive or not finite: singular, the solve stops) and M[j][i] = M[i][j] = v / M[j][j]
// for i > j. Backward: x_i = (M[i][N] - chain) / M[i][i] for i = N-1 .. 0 with the chain v = fma(-M[i][k], x_k, v) for
// k = i+1 .. N-1 in order. Every element's chain is the same whoever runs it, so the lane-parallel device form and the
// serial host form agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace nmc {

// v - sum_{k < j} col[k * ld] row[k], in order
__host__ __device__ __forceinline__ double chol_chain(const double *col, int ld, const double *row, int j, double v)
{
#pragma unroll 8
    for (int k = 0; k < j; ++k) v = __builtin_fma(-col[(size_t)k * ld], row[k], v);
    return v;
}

// v - sum_{i < k < N} row[k] x[k], in order
__host__ __device__ __forceinline__ double back_chain(const double *row, const double *x, int i, int N, double v)
{
    for (int k = i + 1; k < N; ++k) v = __builtin_fma(-row[k], x[k], v);
    return v;
}

// The serial form (host twins). false: singular (x is then untouched; M is partly factored).
inline bool chol_solve_serial(double *M, int ld, int N, double *x)
{
    for (int j = 0; j < N; ++j) {
        double piv = 0.0;
        for (int i = j; i <= N; ++i) {
            const double v = chol_chain(M + i, ld, M + (size_t)j * ld, j, M[(size_t)j * ld + i]);
            if (i == j) {
                if (!(v > 0.0 && __builtin_isfinite(v))) return false;
                piv = __builtin_sqrt(v);
                M[(size_t)j * ld + j] = piv;
            } else {
                const double q = v / piv;
                M[(size_t)j * ld + i] = q;
                if (i < N) M[(size_t)i * ld + j] = q;
            }
        }
    }
    for (int i = N - 1; i >= 0; --i)
        x[i] = back_chain(M + (size_t)i * ld, x, i, N, M[(size_t)i * ld + N]) / M[(size_t)i * ld + i];
    return true;
}

// LDS of the workgroup form: MAXN >= N + 1
template <int MAXN> struct CholShared { double row[MAXN], x[MAXN], piv; int singular; };

// The workgroup form: thread i owns row i, thread N the right-hand side; every thread of a one-dimensional workgroup of
// more than N threads calls it, M is global or LDS memory visible to all of them and complete on entry (the caller's
// barrier). On return (behind a barrier) S.x[0 .. N) is the solution unless the result is false (singular).
template <int MAXN>
__device__ __forceinline__ bool chol_solve_block(double *M, int ld, int N, CholShared<MAXN> &S)
{
    const int tid = threadIdx.x;
    if (tid == 0) S.singular = 0;
    __syncthreads();
    for (int j = 0; j < N; ++j) {
        if (tid < j) S.row[tid] = M[(size_t)j * ld + tid];
        __syncthreads();
        double v = 0.0;
        if (tid >= j && tid <= N) v = chol_chain(M + tid, ld, S.row, j, M[(size_t)j * ld + tid]);
        if (tid == j) {
            if (!(v > 0.0 && __builtin_isfinite(v))) S.singular = 1;
            S.piv = __builtin_sqrt(v);
        }
        __syncthreads();
        if (S.singular) break;                                   // uniform
        if (tid == j) {
            M[(size_t)j * ld + j] = S.piv;
        } else if (tid > j && tid <= N) {
            const double q = v / S.piv;
            M[(size_t)j * ld + tid] = q;
            if (tid < N) M[(size_t)tid * ld + j] = q;
        }
        __syncthreads();
    }
    if (S.singular) return false;
    for (int i = N - 1; i >= 0; --i) {
        if (tid > i && tid < N) S.row[tid] = M[(size_t)i * ld + tid];
        __syncthreads();
        if (tid == 0) S.x[i] = back_chain(S.row, S.x, i, N, M[(size_t)i * ld + N]) / M[(size_t)i * ld + i];
        __syncthreads();
    }
    return true;
}
}  // namespace nmc
