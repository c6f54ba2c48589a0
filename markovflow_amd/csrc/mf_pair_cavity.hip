// The pair cavity of sparse power EP (markovflow/models/sparse_pep.py:251-293): for every pair (b, s) of a [B, S] batch, with the
// marginal N(m, Sig) of q on the pair, its site (nat1, nat2) and the fraction beta of the site to remove,
//   cav_cov  = (Sig^-1 + 2 beta sym(nat2))^-1          sym(X) = (X + X^T) / 2
//   cav_mean = cav_cov (Sig^-1 m - beta nat1)
//   gamma    = G(cav_mean, cav_cov) - G(m, Sig)        G(m, S) = (log det S + m^T S^-1 m) / 2
// computed WITHOUT an explicit inverse.  With Sig = L L^T, M = I + 2 beta L^T sym(nat2) L = C C^T and a = L^-1 m,
// u = a - beta L^T nat1, b = C^-1 u, W = L C^-T:
//   cav_cov = W W^T        cav_mean = W b        gamma = -sum_i log C_ii + (|b|^2 - |a|^2) / 2.
// M is positive definite exactly when the cavity precision is (Sig > 0 given), so a pivot of either factorisation that is not > 0
// (NaN included) makes all three outputs of THAT pair NaN; beta = 0 gives M = I exactly, the cavity equal to the marginal up to the
// rounding of L L^T, and gamma = 0 exactly.  Only the lower triangle of Sig is read, as torch.linalg.cholesky_ex does.
//
// Work split: a GROUP of GW = 4, 8, 16 or 32 lanes per pair (the least power of two above n), lane r < n owns ROW r of every n x n
// matrix in registers, and lane n owns the VECTOR that rides along as row n of the augmented matrix: a left-looking Cholesky that
// treats [Sig; m^T] as n + 1 rows leaves a^T = (L^-1 m)^T in row n at no extra step, and [M; u^T] leaves b^T.  A workgroup is ONE
// wavefront of 64 / GW pairs (16 ... 2), so every barrier below is a wait on the wavefront's own LDS traffic.
// Data movement: the workgroup's pairs are contiguous in all five inputs; they are staged with coalesced loads into three LDS tiles
// of (n + 1) rows of LD = n + 1 elements per pair - n + 1 is odd, and so is the tile (n + 1)^2: lane (pair p, row r) starts at
// (p (n + 1) + r) LD, on a bank of its own, for the row loads and stores; the column walk of L^T T reads consecutive addresses; every
// other LDS read is a broadcast within the group.  The tiles are reused in place (Sig, m -> L, a -> cav_cov, cav_mean; nat2, nat1
// -> C, b; T -> W) and the three outputs leave through LDS with coalesced stores.  No global scratch, no workspace, no atomics.
// Steps, all loops unrolled at compile time (n is a template parameter; the register arrays are indexed by constants):
//   1  rows of [Sig; m^T] -> L, a          column j: s = A_rj - sum_{k<j} L_rk L_jk (row j from LDS), the pivot s_jj by one
//                                          cross-lane move from lane j, L_rj = s / sqrt(s_jj); n divisions and n square roots
//   2  T = sym(nat2) L; lane n: nat1^T L   T_rc = sum_{k>=c} N_rk L_kc
//   3  M = I + 2 beta L^T T (lower);       M_rc = delta_rc + 2 beta sum_k L_kr T_kc;  lane n: u = a - beta (nat1^T L)
//   4  rows of [M; u^T] -> C, b            as step 1
//   5  W = L C^-T by forward substitution on the lane's own row of L; cav_mean_r = W_r . b
//   6  cav_cov_rc = sum_k W_rk W_ck        the same chain of fused multiply-adds for (r, c) and (c, r): symmetric bit for bit
// n (n + 1) + 2 n^2 fused multiply-adds per lane besides the two factorisations; nothing is a matrix-instruction tile at n <= 18.
// Instantiated for n = 2, 4, ..., 18 and both dtypes (float32 computes in float32).
#include "../../include/markovflow_amd.h"

#include "mf_lik_tile.hpp"

namespace {

constexpr int cavity_group(int n) { return n < 4 ? 4 : (n < 8 ? 8 : (n < 16 ? 16 : 32)); }     // lanes per pair: > n

// The factor of the group's N x N matrix, a lane per row (`r`; row N rides along and leaves as its forward substitution), left-looking.
// `row`: the lane's row, in (its lower triangle) and out (zero above the diagonal); `tile`: the group's LDS tile, whose rows are
// overwritten column by column with the finished factor (`writes`: this lane owns a row).  False if a pivot is not > 0.
template <typename T, int N, int GW>
__device__ __forceinline__ bool group_cholesky(T (&row)[N], T* tile, int r, bool writes) {
    constexpr int LD = N + 1;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        T s = row[j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= row[k] * tile[j * LD + k];
        const T piv = __shfl(s, j, GW);                // lane j holds the diagonal
        ok = ok && piv > T(0);
        const T d = sqrt(piv);
        row[j] = r == j ? d : (r > j ? s / d : T(0));
        if (writes) tile[r * LD + j] = row[j];
        __syncthreads();                               // row j + 1 is complete up to column j before column j + 1 reads it
    }
    return ok;
}

template <typename T, int N>
__global__ void __launch_bounds__(64) pair_cavity_kernel(long BS, const T* __restrict__ pair_mean, const T* __restrict__ pair_cov,
                                                         const T* __restrict__ nat1, const T* __restrict__ nat2,
                                                         const T* __restrict__ beta, T* __restrict__ cav_mean,
                                                         T* __restrict__ cav_cov, T* __restrict__ gamma) {
    constexpr int GW = cavity_group(N), PPB = 64 / GW, LD = N + 1, TILE = (N + 1) * LD, NN = N * N;
    __shared__ T sa[PPB * TILE];       // Sig, m  ->  L, a  ->  cav_cov, cav_mean
    __shared__ T sn[PPB * TILE];       // nat2, nat1  ->  C, b
    __shared__ T st[PPB * TILE];       // T  ->  W
    __shared__ T sg[PPB];              // gamma
    const int tid = threadIdx.x, p = tid / GW, lane = tid % GW;
    const int r = lane < N ? lane : N;                 // the lane's row: 0 .. N - 1 of the matrices, N the vector (the surplus
    const int cr = lane < N ? lane : 0;                // lanes repeat it and write nothing); its column where it has one
    const bool matrix = lane < N, writes = lane <= N;
    const long pair0 = (long)blockIdx.x * PPB;
    const int np = BS - pair0 < PPB ? int(BS - pair0) : PPB;           // the pairs of this workgroup (the last one: ragged)
    // ---- staging: np N^2 (N) contiguous elements per matrix (vector) input; a pair that does not exist is the identity with no site
    for (int idx = tid; idx < PPB * NN; idx += 64) {
        const int q = idx / NN, e = idx - q * NN, i = e / N, j = e - i * N;
        const bool there = idx < np * NN;
        sa[q * TILE + i * LD + j] = there ? pair_cov[pair0 * NN + idx] : T(i == j);
        sn[q * TILE + i * LD + j] = there ? nat2[pair0 * NN + idx] : T(0);
    }
    for (int idx = tid; idx < PPB * N; idx += 64) {
        const int q = idx / N, j = idx - q * N;
        const bool there = idx < np * N;
        sa[q * TILE + N * LD + j] = there ? pair_mean[pair0 * N + idx] : T(0);
        sn[q * TILE + N * LD + j] = there ? nat1[pair0 * N + idx] : T(0);
    }
    const T bt = p < np ? beta[pair0 + p] : T(0);
    __syncthreads();
    T* const ta = sa + p * TILE;
    T* const tn = sn + p * TILE;
    T* const tt = st + p * TILE;
    // ---- 1: [Sig; m^T] -> L, a
    T row[N];
#pragma unroll
    for (int k = 0; k < N; ++k) row[k] = ta[r * LD + k];
    const bool ok_s = group_cholesky<T, N, GW>(row, ta, r, writes);
    T aa = T(0);                                       // lane N: |a|^2
#pragma unroll
    for (int k = 0; k < N; ++k) aa += row[k] * row[k];
    // ---- 2: T = sym(nat2) L; lane N: nat1^T L
    T trow[N];
    {
        T ns[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const T x = tn[r * LD + k], y = tn[k * LD + cr];
            ns[k] = matrix ? T(0.5) * (x + y) : x;
        }
#pragma unroll
        for (int c = 0; c < N; ++c) {
            T acc = T(0);
#pragma unroll
            for (int k = c; k < N; ++k) acc += ns[k] * ta[k * LD + c];
            trow[c] = acc;
        }
    }
    if (matrix) {
#pragma unroll
        for (int c = 0; c < N; ++c) tt[r * LD + c] = trow[c];
    }
    __syncthreads();
    // ---- 3: M = I + 2 beta L^T T (the lower triangle is what step 4 reads); lane N: u = a - beta nat1^T L
    {
        T lcol[N];
#pragma unroll
        for (int k = 0; k < N; ++k) lcol[k] = ta[k * LD + cr];
#pragma unroll
        for (int c = 0; c < N; ++c) {
            T acc = T(0);
#pragma unroll
            for (int k = 0; k < N; ++k) acc += lcol[k] * tt[k * LD + c];
            row[c] = matrix ? T(c == r) + (T(2) * bt) * acc : row[c] - bt * trow[c];
        }
    }
    // ---- 4: [M; u^T] -> C, b (every read of nat2 and nat1 lies before the barrier of step 2)
    const bool ok_c = group_cholesky<T, N, GW>(row, tn, r, writes);
    T bb = T(0);                                       // lane N: |b|^2
#pragma unroll
    for (int k = 0; k < N; ++k) bb += row[k] * row[k];
    T logdet = matrix ? log(tn[cr * LD + cr]) : T(0);
#pragma unroll
    for (int m = GW / 2; m >= 1; m >>= 1) logdet += __shfl_xor(logdet, m, GW);
    const bool ok = ok_s && ok_c;
    // ---- 5: W = L C^-T, row by row: C w^T = l^T; cav_mean_r = w . b
    T w[N];
    T cm = T(0);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        T s = ta[r * LD + j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= w[k] * tn[j * LD + k];
        w[j] = s / tn[j * LD + j];
        cm += w[j] * tn[N * LD + j];
    }
    if (matrix) {
#pragma unroll
        for (int k = 0; k < N; ++k) tt[r * LD + k] = w[k];
    }
    __syncthreads();                                   // W is complete, and L has been read for the last time
    // ---- 6: cav_cov = W W^T into the tile of Sig, cav_mean into its row N, gamma
    const T nan = nan_of<T>();
#pragma unroll
    for (int c = 0; c < N; ++c) {
        T acc = T(0);
#pragma unroll
        for (int k = 0; k < N; ++k) acc += w[k] * tt[c * LD + k];
        if (matrix) ta[r * LD + c] = ok ? acc : nan;
    }
    if (matrix) ta[N * LD + r] = ok ? cm : nan;
    if (lane == N) sg[p] = ok ? T(0.5) * (bb - aa) - logdet : nan;
    __syncthreads();
    // ---- the outputs of the workgroup's pairs: contiguous again
    for (int idx = tid; idx < np * NN; idx += 64) {
        const int q = idx / NN, e = idx - q * NN, i = e / N, j = e - i * N;
        cav_cov[pair0 * NN + idx] = sa[q * TILE + i * LD + j];
    }
    for (int idx = tid; idx < np * N; idx += 64) {
        const int q = idx / N, j = idx - q * N;
        cav_mean[pair0 * N + idx] = sa[q * TILE + N * LD + j];
    }
    if (tid < np) gamma[pair0 + tid] = sg[tid];
}

template <typename T>
int run_pair_cavity(int64_t B, int64_t S, int n, const T* pair_mean, const T* pair_cov, const T* nat1, const T* nat2, const T* beta,
                    T* cav_mean, T* cav_cov, T* gamma, void* stream) {
    if (B < 0) return -1;
    if (S < 0 || (B > 0 && S > int64_t(0x7fffffff) / B)) return -2;
    if (n < 2 || n > 18 || (n & 1)) return -100;
    if (B == 0 || S == 0) return 0;
    if (const int bad = first_null(4, {pair_mean, pair_cov, nat1, nat2, beta, cav_mean, cav_cov, gamma})) return bad;
    return with_even_two_d<2>(n, -100, [&](auto D) {
        constexpr int N = decltype(D)::value, PPB = 64 / cavity_group(N);
        return launch(pair_cavity_kernel<T, N>, (B * S + PPB - 1) / PPB, 64, stream, B * S, pair_mean, pair_cov, nat1, nat2, beta,
                      cav_mean, cav_cov, gamma);
    });
}

}  // namespace

extern "C" {

int mf_pair_cavity_f64(int64_t B, int64_t S, int n, const double* pair_mean, const double* pair_cov, const double* nat1,
                           const double* nat2, const double* beta, double* cav_mean, double* cav_cov, double* gamma, void* stream) {
    return run_pair_cavity<double>(B, S, n, pair_mean, pair_cov, nat1, nat2, beta, cav_mean, cav_cov, gamma, stream);
}
int mf_pair_cavity_f32(int64_t B, int64_t S, int n, const float* pair_mean, const float* pair_cov, const float* nat1,
                           const float* nat2, const float* beta, float* cav_mean, float* cav_cov, float* gamma, void* stream) {
    return run_pair_cavity<float>(B, S, n, pair_mean, pair_cov, nat1, nat2, beta, cav_mean, cav_cov, gamma, stream);
}

}  // extern "C"
