/*
 * markovflow_amd - C ABI of the MI355X (gfx950) Kalman / block-tridiagonal hot path.
 *
 * This is the drop-in boundary.  In the reference the arithmetic of this path is reached through
 * eight Python imports from the third-party TensorFlow-op library banded_matrices
 * (/root/reference/markovflow/block_tri_diag.py:22-31) plus batched TensorFlow small-matrix ops
 * (markovflow/state_space_model.py:431-483, markovflow/kalman_filter.py:86-271).  Each entry point
 * below names the reference call it replaces.
 *
 * Conventions
 *   - every pointer is a caller-owned DEVICE pointer, contiguous row-major, layout exactly the
 *     reference's: matrices [B, T, d, d], vectors [B, T, d]; `sub` has T-1 blocks per series and
 *     block k couples block k+1 (row) with block k (column);
 *   - suffix _f32 / _f64 selects the scalar type; both are first class;
 *   - nothing is allocated inside: scratch comes from the caller (`*_workspace_bytes` + `ws`);
 *   - `stream` is a hipStream_t (passed as void*); all work is enqueued, nothing synchronises;
 *   - `info` (nullable) is a device int, zeroed by the caller, that the kernels raise on a non-positive pivot (LAPACK info > 0
 *     style; results are then NaN from the failing block on).  The word NAMES the first failing block where the raising kernel
 *     knows it - mf_info_flat_index(word) = series * blocks_per_series + block, the smallest such index over everything that
 *     raised on this word (the Cholesky and log-likelihood kernels of the lane, streamed and panel forms) - and is 1 where it does
 *     not (reduction levels, composite kernels): LAPACK's `info = 1 + flat index`, SURVEY 8(b), is `1 + mf_info_flat_index(word)`;
 *   - return value: 0 ok; -k = argument k (1-based) invalid; -100 = state dimension not instantiated for this entry
 *     point (register kernels 1..9, row kernels 10..15, wave / tile engines up to 64 in fp32 and 32 in fp64 - see
 *     mf_max_state_dim*, mf_row_operators_cover); -101 = this fused / streamed variant does not cover the call (the caller
 *     takes the general entry point); -1000 = launch failure;
 *   - re-entrant, no global state.
 */
#ifndef MARKOVFLOW_AMD_H
#define MARKOVFLOW_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Library / build identification. */
int mf_version(void);
/* Queues a 4-byte copy of the device word `info` into `host_mirror` (pinned host memory) on `stream`: after any synchronisation
 * with the stream the mirror holds the final word of every factorising launch queued before (the reference raises inside the
 * Cholesky op, block_tri_diag.py:423-436; here the failure crosses the bus in stream order, never outside it). */
int mf_info_mirror(int* host_mirror, const int* info, void* stream);
/* Flat index (series * blocks_per_series + block) of the first block whose elimination met a non-positive pivot, decoded from an
 * `info` word; -1 when the word is 0 (no failure) or 1 (a failure whose block the raising kernel could not name). */
int64_t mf_info_flat_index(int info_word);
int mf_max_state_dim(void);              /* every entry point, fp32 and fp64: register-resident kernels (9)       */
/* 1 when the register / row kernels run EVERY operator for this shape: d <= 9 always; 10 <= d <= 15 (row kernels only: one
 * 16-lane row per chunk; many series or short chains run them with one chunk per series) for every chain of at least two
 * blocks - otherwise, and for d >= 16, the LDS-tile / MFMA engine takes the call (same entry points; the chain-layout and
 * fused variants then return -100 / -101).  With more than four outputs the observation side (log-likelihood, precision
 * assembly, gradient step) goes to the tile engine at any d. */
int mf_row_operators_cover(int64_t B, int64_t T, int d, int elem_size);
int mf_max_state_dim_f32_loglik(void);   /* mf_kf_loglik_f32 only: LDS-tiled MFMA kernels for 10 <= d <= 64       */
int mf_max_state_dim_f64_loglik(void);   /* mf_kf_loglik_f64 only: f64 MFMA for 10 <= d <= 64 (panel kernels > 32) */
int mf_max_state_dim_f64_tile_ops(void); /* every other fp64 entry point on the MFMA engines: 10 <= d <= 32          */

/*
 * KalmanFilter.log_likelihood, per series, fully fused
 *   replaces markovflow/kalman_filter.py:184-255 and everything it calls:
 *   _k_inv_post (:86-101), StateSpaceModel._build_precision (state_space_model.py:431-483),
 *   SymmetricBlockTriDiagonal.cholesky (block_tri_diag.py:423-436 -> banded cholesky_band),
 *   marginal_means (state_space_model.py:232-251), LowerTriangularBlockTriDiagonal.solve
 *   (block_tri_diag.py:339-351 -> banded solve_triang_mat), abs_log_det (:353-366),
 *   log_det_precision (state_space_model.py:343-373).
 * Inputs: mu0 [B,d], cholP0 [B,d,d], A [B,T-1,d,d], b [B,T-1,d], cholQ [B,T-1,d,d],
 *         H [B,T,m,d], y [B,T,m], Rinv [m,m] (rinv_per_step=0, KalmanFilter) or [B,T,m,m]
 *         (rinv_per_step=1, KalmanFilterWithSites / WithSparseSites), 1 <= m <= 32 (up to four outputs: the register / row
 *         kernels; more: the LDS-tile kernels, at any state dimension).
 * State dimension: 1..9 in fp32 and fp64: one lane per (series, time-chunk) with the state in registers up to d = 6 (fp32: 8),
 *         above that one 16-lane DPP row per (series, time-chunk) with one matrix row per lane (csrc/mf_row.hpp -
 *         BASELINE config 4, d = 9) - the rows also take 10 <= d <= 15, there with up to EIGHT outputs; beyond that (and with
 *         more outputs than the register / row kernels take, at any d) 1 <= d <= 64 (fp32) or 32 (fp64) with 1 <= m <= 32 run one workgroup per (series,
 *         time-chunk) on LDS tiles and f32 / f64 MFMA (csrc/mf_big.hpp - BASELINE config 5, state_dim = 64).
 * Output: out[s] = add_const + term1 + term2 + 1/2 log|K^-1| - log|L|  (kalman_filter.py:233-253), i.e. the
 *         per-series log-likelihood; the terms that do not depend on the chain,
 *         -1/2 m T log(2 pi) + 1/2 log|Sigma^-1|  (kalman_filter.py:229-231,249-253), are passed in add_const.
 * chunks: number of time partitions per series (0 = choose automatically).
 * prof_start / prof_stop: optional hipEvent_t (NULL = off) recorded on `stream` immediately before and after
 *         the dominant (level-0) kernel, so a caller can time that kernel alone.
 */
size_t mf_kf_loglik_workspace_bytes(int64_t B, int64_t T, int d, int elem_size, int64_t chunks);
int mf_kf_loglik_f64(int64_t B, int64_t T, int d, int m, const double* mu0, const double* cholP0,
                     const double* A, const double* b, const double* cholQ, const double* H, const double* y,
                     const double* Rinv, int rinv_per_step, double add_const, double* out, void* ws,
                     size_t ws_bytes, int* info, int64_t chunks, void* prof_start, void* prof_stop, void* stream);
int mf_kf_loglik_f32(int64_t B, int64_t T, int d, int m, const float* mu0, const float* cholP0,
                     const float* A, const float* b, const float* cholQ, const float* H, const float* y,
                     const float* Rinv, int rinv_per_step, float add_const, float* out, void* ws,
                     size_t ws_bytes, int* info, int64_t chunks, void* prof_start, void* prof_stop, void* stream);

/*
 * SymmetricBlockTriDiagonal.cholesky  (block_tri_diag.py:423-436; banded cholesky_band +
 * block_to_band/band_to_block layout shuffles, which do not exist here).  Natural order:
 * L_0 = chol(D_0), W_{k-1} = S_{k-1} L_{k-1}^-T, L_k = chol(D_k - W_{k-1} W_{k-1}^T).
 * sub / lsub may be NULL (block-diagonal matrix).  Only the lower triangle of diag is read.
 * With many series one lane walks each chain.  With few, long chains (BASELINE config 3: B=1, T=100000) the
 * factorisation is parallelised in time by a multi-level partitioned elimination that still returns the
 * natural-order factor (csrc/mf_btd_par.hpp); that path needs scratch: ws_bytes >=
 * mf_btd_cholesky_workspace_bytes(...) (0 = the serial kernel will be used; ws may then be NULL).
 * The same holds for 10 <= d <= 64 (f32) / 32 (f64) on the LDS-tile / MFMA engine: few series are cut into chunks in time
 * (csrc/mf_bigpar_impl.hpp) - also for mf_btd_solve, mf_btd_diag_of_inverse, mf_btd_udl and mf_ssm_marginal_means, each with the
 * workspace its own query names; a NULL or short workspace selects the one-workgroup-per-series kernels, never an error.
 */
size_t mf_btd_cholesky_workspace_bytes(int64_t B, int64_t T, int d, int elem_size);
int mf_btd_cholesky_f64(int64_t B, int64_t T, int d, const double* diag, const double* sub, double* ldiag,
                        double* lsub, void* ws, size_t ws_bytes, int* info, void* stream);
int mf_btd_cholesky_f32(int64_t B, int64_t T, int d, const float* diag, const float* sub, float* ldiag,
                        float* lsub, void* ws, size_t ws_bytes, int* info, void* stream);

/*
 * LowerTriangularBlockTriDiagonal.solve  (block_tri_diag.py:339-351; banded solve_triang_mat):
 * out = L^-1 rhs (transpose=0) or L^-T rhs (transpose=1).  rhs/out are [Br,T,d]; rhs series r uses the
 * factor of series r % Bl (Br a multiple of Bl: extra leading dims, state_space_model.py:307-322).
 * Few, long chains are solved in parallel in time (the substitution is an affine recursion, composed per chunk
 * and scanned over the chunks); scratch as for the Cholesky: mf_btd_solve_workspace_bytes (0 = serial kernel).
 */
size_t mf_btd_solve_workspace_bytes(int64_t Bl, int64_t Br, int64_t T, int d, int elem_size);
int mf_btd_solve_f64(int64_t Bl, int64_t Br, int64_t T, int d, const double* ldiag, const double* lsub,
                     const double* rhs, double* out, int transpose, void* ws, size_t ws_bytes, void* stream);
int mf_btd_solve_f32(int64_t Bl, int64_t Br, int64_t T, int d, const float* ldiag, const float* lsub,
                     const float* rhs, float* out, int transpose, void* ws, size_t ws_bytes, void* stream);

/*
 * BlockTriDiagonal.dense_mult  (block_tri_diag.py:175-199; banded product_band_mat).
 * mode 0: M x for lower-triangular M; 1: M^T x; 2: symmetric M x (lower triangle mirrored).
 */
int mf_btd_matvec_f64(int64_t Bl, int64_t Br, int64_t T, int d, const double* diag, const double* sub,
                      const double* x, double* out, int mode, void* stream);
int mf_btd_matvec_f32(int64_t Bl, int64_t Br, int64_t T, int d, const float* diag, const float* sub,
                      const float* x, float* out, int mode, void* stream);

/* LowerTriangularBlockTriDiagonal.abs_log_det  (block_tri_diag.py:353-366): out [B]. */
int mf_btd_logdet_f64(int64_t B, int64_t T, int d, const double* ldiag, double* out, void* stream);
int mf_btd_logdet_f32(int64_t B, int64_t T, int d, const float* ldiag, float* out, void* stream);

/*
 * Fused scalar form of cholesky + solve + abs_log_det on an explicit (diag, sub, rhs):
 * out[s] = 1/2 |L^-1 rhs|^2 - log|L|, computed by partitioned (block cyclic reduction style)
 * elimination in time; this is what the log-likelihood of the sites variants reduces to.
 */
size_t mf_btd_logdet_quad_workspace_bytes(int64_t B, int64_t T, int d, int elem_size);
int mf_btd_logdet_quad_f64(int64_t B, int64_t T, int d, const double* diag, const double* sub, const double* rhs,
                           double* out, void* ws, size_t ws_bytes, int* info, void* stream);
int mf_btd_logdet_quad_f32(int64_t B, int64_t T, int d, const float* diag, const float* sub, const float* rhs,
                           float* out, void* ws, size_t ws_bytes, int* info, void* stream);

/*
 * LowerTriangularBlockTriDiagonal.block_diagonal_of_inverse  (block_tri_diag.py:318-337; banded
 * inverse_from_cholesky_band): diagonal blocks of (L L^T)^-1 into odiag [B,T,d,d]; if osub != NULL also
 * the sub-diagonal blocks [B,T-1,d,d] (what ssm_gaussian_transformations.py:453-458 reads).  The backward
 * (Takahashi) recursion is a congruence recursion Sigma_k = N_k + G_k^T Sigma_{k+1} G_k; for few series it is
 * composed per time-chunk and scanned (csrc/mf_btd_par.hpp), with scratch from the caller.
 */
size_t mf_btd_diag_of_inverse_workspace_bytes(int64_t B, int64_t T, int d, int elem_size);   /* 0 = serial kernel */
int mf_btd_diag_of_inverse_f64(int64_t B, int64_t T, int d, const double* ldiag, const double* lsub,
                               double* odiag, double* osub, void* ws, size_t ws_bytes, void* stream);
int mf_btd_diag_of_inverse_f32(int64_t B, int64_t T, int d, const float* ldiag, const float* lsub, float* odiag,
                               float* osub, void* ws, size_t ws_bytes, void* stream);

/*
 * StateSpaceModel.marginal_covariances and subsequent_covariances (markovflow/state_space_model.py:254-275, 326-341) in one
 * scan: Sigma_0 = P0, Sigma_{k+1} = A_k Sigma_k A_k^T + Q_k, out_sub[k] = Cov(x_{k+1}, x_k) = A_k Sigma_k (nullable).  The
 * reference takes the block diagonal of the inverse of the assembled precision; the forward recursion yields the same blocks
 * without assembling or factorising it.  Parallel in time for B < 4096 (workspace = the diag-of-inverse query), one lane per
 * series otherwise.  T >= 2.  State dimension 1..9 in registers; 10..64 (fp32) / 10..32 (fp64) on the LDS-tile / MFMA engine,
 * partitioned in time: chunk maps S -> M S M^T + N, a walk over the chunk boundaries, re-start per chunk (three launches;
 * workspace from the same query, one workgroup per series without it); -100 above.
 * cholP0 [B,d,d], A, cholQ [B,T-1,d,d]; out_cov [B,T,d,d], out_sub [B,T-1,d,d].
 */
int mf_ssm_marginal_covariances_f64(int64_t B, int64_t T, int d, const double* cholP0, const double* A, const double* cholQ,
                                    double* out_cov, double* out_sub, void* ws, size_t ws_bytes, void* stream);
int mf_ssm_marginal_covariances_f32(int64_t B, int64_t T, int d, const float* cholP0, const float* A, const float* cholQ,
                                    float* out_cov, float* out_sub, void* ws, size_t ws_bytes, void* stream);

/*
 * GaussMarkovDistribution.marginals (+ StateSpaceModel.subsequent_covariances)  (gauss_markov.py:107-117,
 * state_space_model.py:232-262,326-341) with ONE kernel writing all three: mu_{k+1} = A_k mu_k + b_k rides along the covariance
 * recursion of mf_ssm_marginal_covariances, A is read once.  Many series (B >= 4096) or a short chain (T < 64): one sweep per
 * series, no workspace.  Few long chains: the up / down sweeps of the two scans in time, then one emit kernel that restarts both
 * recursions at the chunk boundaries (workspace: mf_ssm_marginals_workspace_bytes; -101 without it - the caller then uses
 * mf_ssm_marginal_means + mf_ssm_marginal_covariances).  State dimension 10..64 (fp32) / 10..32 (fp64): the means ride along
 * the three passes of the time-partitioned covariance recursion (same workspace query).
 * mu0 [B,d], b [B,T-1,d]; out_mean [B,T,d], out_cov [B,T,d,d], out_sub [B,T-1,d,d] (nullable).
 */
size_t mf_ssm_marginals_workspace_bytes(int64_t B, int64_t T, int d, int elem_size);
int mf_ssm_marginals_f64(int64_t B, int64_t T, int d, const double* mu0, const double* cholP0, const double* A, const double* b,
                         const double* cholQ, double* out_mean, double* out_cov, double* out_sub, void* ws, size_t ws_bytes,
                         void* stream);
int mf_ssm_marginals_f32(int64_t B, int64_t T, int d, const float* mu0, const float* cholP0, const float* A, const float* b,
                         const float* cholQ, float* out_mean, float* out_cov, float* out_sub, void* ws, size_t ws_bytes,
                         void* stream);

/*
 * SymmetricBlockTriDiagonal.upper_diagonal_lower  (block_tri_diag.py:438-545, the tf.while_loop):
 * ut [B,T-1,d,d] = U_k^T, chol_d [B,T,d,d] = chol(Delta_k).
 * With eta != NULL ([B,T,d]) it additionally runs the rest of
 * BaseKalmanFilter.posterior_state_space_model (kalman_filter.py:159-174) in the same sweep:
 * m_post [B,T,d] = [mu0', b'_1...] and chol_dinv [B,T,d,d] = chol(Delta_k^-1) = [cholP0', cholQ'_1...].
 * chain_layout = 1 (needs eta; state dimension <= 9, else -101) writes the posterior chain the way StateSpaceModel takes it,
 * so that nothing has to be sliced, copied or negated afterwards: ut holds the posterior transitions A'_k = -(U_k^T), m_post
 * is [B*d values of mu0' | B*(T-1)*d values of b'] and chol_dinv [B*d*d values of cholP0' | B*(T-1)*d*d values of cholQ'];
 * chol_d may be NULL in this mode (the chain does not contain it: one d x d block per step less to write).
 * Few series: Delta_k are the natural-order pivots of the block-REVERSED matrix, so the parallel-in-time Cholesky
 * hierarchy is reused with reversed indexing, and the posterior offsets are an affine scan (scratch from the caller,
 * mf_btd_udl_workspace_bytes; 0 / NULL = one lane per series).
 */
size_t mf_btd_udl_workspace_bytes(int64_t B, int64_t T, int d, int elem_size);
int mf_btd_udl_f64(int64_t B, int64_t T, int d, const double* diag, const double* sub, double* ut, double* chol_d,
                   const double* eta, double* m_post, double* chol_dinv, int chain_layout, void* ws, size_t ws_bytes,
                   int* info, void* stream);
int mf_btd_udl_f32(int64_t B, int64_t T, int d, const float* diag, const float* sub, float* ut, float* chol_d,
                   const float* eta, float* m_post, float* chol_dinv, int chain_layout, void* ws, size_t ws_bytes,
                   int* info, void* stream);

/*
 * StateSpaceModel._build_precision (state_space_model.py:431-483), optionally + H^T R^-1 H
 * (kalman_filter.py:86-101) and the posterior information vector
 * eta = G^T Sigma^-1 y + K^-1 mu (kalman_filter.py:153-156).
 * H == NULL: prior precision only.  y == NULL: no observation term in eta.  eta == NULL: not computed
 * (mu0, b may then be NULL).  diag [B,T,d,d], sub [B,T-1,d,d], eta [B,T,d].
 */
int mf_ssm_precision_f64(int64_t B, int64_t T, int d, int m, const double* mu0, const double* cholP0,
                         const double* A, const double* b, const double* cholQ, const double* H, const double* y,
                         const double* Rinv, int rinv_per_step, double* diag, double* sub, double* eta,
                         void* stream);
int mf_ssm_precision_f32(int64_t B, int64_t T, int d, int m, const float* mu0, const float* cholP0, const float* A,
                         const float* b, const float* cholQ, const float* H, const float* y, const float* Rinv,
                         int rinv_per_step, float* diag, float* sub, float* eta, void* stream);

/*
 * StateSpaceModel.marginal_means / sample  (state_space_model.py:232-251,298-324): solves
 * (A^-1 block) x = offs, i.e. x_0 = offs_0, x_k = A_k x_{k-1} + offs_k.  offs/out [Br,T,d]; series r uses
 * the transitions of series r % Bl.  Scratch (parallel-in-time scan for few series): the size
 * mf_btd_solve_workspace_bytes(Bl, Br, T, d, elem_size) returns (0 / NULL = serial kernel).
 */
int mf_ssm_marginal_means_f64(int64_t Bl, int64_t Br, int64_t T, int d, const double* A, const double* offs,
                              double* out, void* ws, size_t ws_bytes, void* stream);
int mf_ssm_marginal_means_f32(int64_t Bl, int64_t Br, int64_t T, int d, const float* A, const float* offs,
                              float* out, void* ws, size_t ws_bytes, void* stream);

/*
 * Block-wise d x d products out[s,k] = X[s,k] Y[s,k] over [B, n] blocks; x_stride / y_stride = blocks per series in
 * the allocations of X / Y (>= n: a leading slice of a longer chain needs no copy).  Replaces the batched tf.matmul of
 * StateSpaceModel.subsequent_covariances (state_space_model.py:326-341), Cov(x_{k+1}, x_k) = A_k P_k.
 */
int mf_block_matmul_f64(int64_t B, int64_t n, int d, const double* X, int64_t x_stride, const double* Y,
                        int64_t y_stride, double* out, void* stream);
int mf_block_matmul_f32(int64_t B, int64_t n, int d, const float* X, int64_t x_stride, const float* Y,
                        int64_t y_stride, float* out, void* stream);

/*
 * SDE kernel -> state space model tensors on the device (the step right before the path).
 * For a concatenation (block-diagonal state: Sum / IndependentMultiOutput / a single kernel) of `ncomp` Matern components
 * of order orders[c] in {1, 3, 5} (Matern-1/2, 3/2, 5/2; state sizes 1, 2, 3) with lam = sqrt(order) / lengthscale and
 * variance var:  A[s,k] = exp(F dt[s,k]) in closed form (markovflow/kernels/matern.py:66-86,299-324,434-460, block diagonal
 * as kernels/sde_kernel.py:592-610), Q = Pinf - A Pinf A^T + jitter I (sde_kernel.py:421-446) and cholQ = its lower Cholesky
 * factor with an exactly zero Q passed through as zero (state_space_model.py:634-656).
 * orders is a HOST array of ncomp ints; lam / var are device arrays [ncomp] (per_series = 0) or [B, ncomp] (per_series = 1);
 * dt [B, n]; outputs A, cholQ (nullable), Q (nullable): [B, n, d, d] with d = sum of the component sizes.
 */
int mf_sde_matern_transitions_f64(int64_t B, int64_t n, int ncomp, const int* orders, const double* lam, const double* var,
                                  int per_series, const double* dt, double jitter, double* A, double* cholQ, double* Q,
                                  void* stream);
int mf_sde_matern_transitions_f32(int64_t B, int64_t n, int ncomp, const int* orders, const float* lam, const float* var,
                                  int per_series, const float* dt, float jitter, float* A, float* cholQ, float* Q,
                                  void* stream);

/*
 * Reverse mode of mf_sde_matern_transitions_* with respect to the hyper-parameters (the reference differentiates matern.py /
 * sde_kernel.py:421-446 and the Cholesky through TensorFlow: the GPR training step): for incoming gradients g_A, g_cholQ
 * [B,n,d,d] (either may be NULL) writes out[b, k, c, 0 / 1] = d/d lam_c, d/d var_c of <g_A[b,k], A_k> + <g_cholQ[b,k], chol Q_k>;
 * the caller sums over k (and over b for shared hyper-parameters).  One lane per (series, transition), the generator's closed
 * forms evaluated in forward mode (csrc/mf_sde.hip: Dual2).
 */
int mf_sde_matern_transitions_grad_f64(int64_t B, int64_t n, int ncomp, const int* orders, const double* lam, const double* var,
                                       int per_series, const double* dt, double jitter, const double* g_A, const double* g_cholQ,
                                       double* out, void* stream);
int mf_sde_matern_transitions_grad_f32(int64_t B, int64_t n, int ncomp, const int* orders, const float* lam, const float* var,
                                       int per_series, const float* dt, float jitter, const float* g_A, const float* g_cholQ,
                                       float* out, void* stream);
/* The same with the incoming gradients as packed records (see mf_gpr_matern_loglik_grad): only the entries the generator reads. */
int mf_sde_matern_transitions_grad_packed_f64(int64_t B, int64_t n, int ncomp, const int* orders, const double* lam,
                                              const double* var, int per_series, const double* dt, double jitter,
                                              const double* g_packed, double* out, void* stream);
int mf_sde_matern_transitions_grad_packed_f32(int64_t B, int64_t n, int ncomp, const int* orders, const float* lam,
                                              const float* var, int per_series, const float* dt, float jitter,
                                              const float* g_packed, float* out, void* stream);
/* The stationary prior of the same kernels, chol(Pinf + jitter) (markovflow/kernels/sde_kernel.py:402-419): out [B,ncomp,2] =
 * the contraction of g_cholP0 [B,d,d] (only the lower triangles of its diagonal blocks are read) with d chol / d (lam, var) of
 * every component - per series; a caller with shared hyper-parameters (per_series = 0) sums over the batch. */
int mf_sde_matern_prior_chol_grad_f64(int64_t B, int ncomp, const int* orders, const double* lam, const double* var, int per_series,
                                      double jitter, const double* g_cholP0, double* out, void* stream);
int mf_sde_matern_prior_chol_grad_f32(int64_t B, int ncomp, const int* orders, const float* lam, const float* var, int per_series,
                                      float jitter, const float* g_cholP0, float* out, void* stream);

/*
 * The generator for generalised components (markovflow/kernels/constant.py, periodic.py, sde_kernel.py:691-822): as
 * mf_sde_matern_transitions_*, with
 *   orders[c] in {0, 1, 3, 5}: order 0 is the constant component, A = [1], Pinf = [var], Q = jitter I exactly (lam[c] is ignored);
 *   osc[c] (HOST array of ncomp ints): 0 = no oscillator, 1 = A = A^M (x) R(omega dt), Pinf = Pinf^M (x) I2,
 *                                      2 = A = R(omega dt) (x) A^M, Pinf = I2 (x) Pinf^M,
 *     R(th) = [[cos th, -sin th], [sin th, cos th]]; an oscillator doubles the component's state size (1, 2, 3 -> 2, 4, 6);
 *   omega: device array shaped like lam / var ([ncomp] or [B, ncomp]), angular frequency 2 pi / period, ignored where osc[c] = 0
 *     (may be NULL when no component has an oscillator); var is the product of the factors' variances.
 * With every osc[c] = 0 and no order 0 the outputs are bit-identical to mf_sde_matern_transitions_*.
 * Errors: the negative position of the offending argument; -100 when the 64 d x d staging images exceed the LDS limit.
 */
int mf_sde_transitions_f64(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, const double* lam, const double* var,
                           const double* omega, int per_series, const double* dt, double jitter, double* A, double* cholQ, double* Q,
                           void* stream);
int mf_sde_transitions_f32(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, const float* lam, const float* var,
                           const float* omega, int per_series, const float* dt, float jitter, float* A, float* cholQ, float* Q,
                           void* stream);
/*
 * Reverse mode of mf_sde_transitions_*: out[b, k, c, 0 / 1 / 2] = d/d lam_c, d/d var_c, d/d omega_c of
 * <g_A[b,k], A_k> + <g_cholQ[b,k], chol Q_k> (g_A, g_cholQ [B,n,d,d], either may be NULL; out [B,n,ncomp,3]); d/d lam is zero
 * for order 0 and d/d omega where osc[c] = 0.  The same closed forms in forward mode with three tangents (csrc/mf_sde.hip: Dual3).
 */
int mf_sde_transitions_grad_f64(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, const double* lam,
                                const double* var, const double* omega, int per_series, const double* dt, double jitter,
                                const double* g_A, const double* g_cholQ, double* out, void* stream);
int mf_sde_transitions_grad_f32(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, const float* lam,
                                const float* var, const float* omega, int per_series, const float* dt, float jitter,
                                const float* g_A, const float* g_cholQ, float* out, void* stream);

/*
 * The generator for a PIECEWISE-stationary kernel (markovflow/kernels/piecewise_stationary.py): as mf_sde_transitions_*, with the
 * hyper-parameters of every step taken from the segment its start time lies in.
 *   nseg >= 1 segments, change_points [nseg-1] (device, sorted ascending, finite; may be NULL when nseg = 1), shared by all series;
 *   t_start [B,n]: the time every transition starts at (any order, -/+ 1e10 allowed); its segment is the number of change points
 *     <= t_start, compared in the call's precision - searchsorted(.., "right") - 1 on the -/+ inf augmented array of the
 *     reference: a start time exactly on a change point belongs to the segment AFTER it;
 *   lam, var, omega: [nseg, ncomp], or [B, nseg, ncomp] with per_series; dt [B,n];
 *   A, cholQ, Q [B,n,d,d] (the latter two optional), seg [B,n] int32 (optional): the segment of every step.
 * Q_k = Pinf(seg) - A_k Pinf(seg) A_k^T + jitter I with A_k from the SAME segment: a transition that crosses a change point is
 * generated entirely from the segment it starts in (the reference's behaviour; exact only when no transition crosses one).
 * The lookup runs in the kernel (up to 256 change points staged in LDS next to the staging image, a binary search in global
 * memory otherwise): nseg has no small cap.  With nseg = 1 the outputs are those of mf_sde_transitions_*.
 * Errors: the negative position of the offending argument, checked before any launch; -100 as for mf_sde_transitions_*; B = 0 or
 * n = 0 returns 0.
 */
int mf_sde_piecewise_transitions_f64(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, int nseg,
                                     const double* change_points, const double* lam, const double* var, const double* omega,
                                     int per_series, const double* t_start, const double* dt, double jitter, double* A, double* cholQ,
                                     double* Q, int* seg, void* stream);
int mf_sde_piecewise_transitions_f32(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, int nseg,
                                     const float* change_points, const float* lam, const float* var, const float* omega,
                                     int per_series, const float* t_start, const float* dt, float jitter, float* A, float* cholQ,
                                     float* Q, int* seg, void* stream);
/*
 * Reverse mode of mf_sde_piecewise_transitions_*: out[b, s, c, 0 / 1 / 2] = d/d lam, d/d var, d/d omega of component c in segment s
 * of  sum over the steps k of series b that start in segment s of  <g_A[b,k], A_k> + <g_cholQ[b,k], chol Q_k>  (g_A, g_cholQ
 * [B,n,d,d], either may be NULL; out [B,nseg,ncomp,3]).  A caller with shared hyper-parameters sums out over B.  The per-step
 * terms are those of mf_sde_transitions_grad_*; the sum over the steps of one (series, segment) runs on the device in a fixed
 * order without floating-point atomics (two launches: per block of 64 steps one partial sum per segment present, then the blocks
 * in order), so two calls agree bit for bit, for any order of t_start.  A segment without a step, d/d lam of an order-0
 * component and d/d omega of a component without an oscillator are exact zeros.
 * workspace: mf_sde_piecewise_transitions_grad_workspace_bytes(B, n, ncomp, sizeof(T)) bytes of device memory.
 */
size_t mf_sde_piecewise_transitions_grad_workspace_bytes(int64_t B, int64_t n, int ncomp, int elem_size);
int mf_sde_piecewise_transitions_grad_f64(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, int nseg,
                                          const double* change_points, const double* lam, const double* var, const double* omega,
                                          int per_series, const double* t_start, const double* dt, double jitter, const double* g_A,
                                          const double* g_cholQ, double* out, void* workspace, size_t workspace_bytes, void* stream);
int mf_sde_piecewise_transitions_grad_f32(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, int nseg,
                                          const float* change_points, const float* lam, const float* var, const float* omega,
                                          int per_series, const float* t_start, const float* dt, float jitter, const float* g_A,
                                          const float* g_cholQ, float* out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Impulse / step mean functions (markovflow/mean_function.py): the response of the kernel's own SDE to interventions at
 * action_times [B,K] (K >= 1, sorted ascending per series, ties allowed; not checked), evaluated at time_points [B,N] (any order).
 * Components as for mf_sde_transitions_* (orders, osc: HOST arrays; lam, omega: [ncomp], or [B,ncomp] with per_series; lam may be
 * NULL when every order is 0, omega when there is no oscillator; no var).  With j(t) = #{k : action_times[k] < t} (strict, in the
 * call's precision: a point exactly on an action time does not yet see that action):
 *   j = 0:  state = 0 and f = 0 EXACTLY (the product is skipped, so a point far before the first action gives no inf * 0);
 *   a NaN time point counts as j = K (it sorts last, as in torch.searchsorted): its gap is NaN, so its state and f are NaN, and in
 *   the reverse mode it makes g_r of its series (and bin K - 1 of g_a) NaN - a bad query time is not hidden;
 *   j > 0:  state(t) = a_k + exp(F (t - tau_k)) c_k,  k = j - 1,  with  c_0 = r_0,  c_k = exp(F (tau_k - tau_{k-1})) c_{k-1} + r_k;
 *   f[.., o] = the sum of the FIRST state of every component c with out_map[c] = o  (out_map: HOST array [ncomp], 0 <= . < m <= ncomp).
 * r [B,K,d]; a [B,K,d] or NULL (zero); f [B,N,m]; state [B,N,d] optional; c [B,K,d]: caller-owned scratch that receives the
 * coefficients.  Two launches: a scan sequential in K (one lane per (series, component)) and the evaluation (one lane per point;
 * every block of exp(F dt) is generated in registers, nothing d x d is held, so ncomp <= 16 is the only limit).
 * Errors: the negative position of the offending argument, checked before any launch; B = 0 or N = 0 returns 0 without a launch.
 */
int mf_mean_response_f64(int64_t B, int64_t K, int64_t N, int ncomp, const int* orders, const int* osc, const double* lam,
                         const double* omega, int per_series, const double* action_times, const double* r, const double* a,
                         const double* time_points, int m, const int* out_map, double* f, double* state, double* c, void* stream);
int mf_mean_response_f32(int64_t B, int64_t K, int64_t N, int ncomp, const int* orders, const int* osc, const float* lam,
                         const float* omega, int per_series, const float* action_times, const float* r, const float* a,
                         const float* time_points, int m, const int* out_map, float* f, float* state, float* c, void* stream);
/*
 * Reverse mode of mf_mean_response_*, the adjoint of the linear map (r, a) -> f: from g_f [B,N,m] to g_r [B,K,d] and g_a [B,K,d]
 * (g_a may be NULL).  Per point  exp(F (t - tau_k))^T H^T g_f  goes to bin k of g_c and  H^T g_f  to bin k of g_a; then
 * lambda_{K-1} = g_c_{K-1},  lambda_{k-1} = g_c_{k-1} + exp(F (tau_k - tau_{k-1}))^T lambda_k,  g_r = lambda.  The sums over the
 * points of one bin run in a fixed order without floating-point atomics (two launches: per block of 64 points one partial sum per
 * bin present, then every series' records in block order and the recurrence), so two calls agree bit for bit, for any order of
 * time_points.  N = 0 gives zeros.
 * workspace: mf_mean_response_grad_workspace_bytes(B, N, ncomp, d, sizeof(T)) bytes of device memory.
 */
size_t mf_mean_response_grad_workspace_bytes(int64_t B, int64_t N, int ncomp, int d, int elem_size);
int mf_mean_response_grad_f64(int64_t B, int64_t K, int64_t N, int ncomp, const int* orders, const int* osc, const double* lam,
                              const double* omega, int per_series, const double* action_times, const double* time_points, int m,
                              const int* out_map, const double* g_f, double* g_r, double* g_a, void* workspace,
                              size_t workspace_bytes, void* stream);
int mf_mean_response_grad_f32(int64_t B, int64_t K, int64_t N, int ncomp, const int* orders, const int* osc, const float* lam,
                              const float* omega, int per_series, const float* action_times, const float* time_points, int m,
                              const int* out_map, const float* g_f, float* g_r, float* g_a, void* workspace, size_t workspace_bytes,
                              void* stream);

/*
 * The generator of the LatentExponentiallyGenerated kernel (markovflow/kernels/latent_exp_generated.py): a dense feedback matrix
 * F [d,d] (per_series: [B,d,d]) with steady-state covariance I, 1 <= d <= 16; dt [B,n]; outputs [B,n,d,d], A required, cholQ and Q
 * optional:
 *   A_k = expm(dt_k F),  Q_k = I - A_k A_k^T + jitter I (symmetric),  cholQ_k its lower factor (upper triangle exactly zero).
 * Scaling and squaring with expm - I carried through the squarings, from which Q is formed without the cancellation of
 * I - A A^T at short gaps.  An all-zero Q passes through as a zero factor; a non-positive pivot gives NaN through the square root
 * (no info word); a step whose dt F is not finite gives NaN outputs for that step.  Any finite dt is covered (dt = 1e10: A -> 0).
 * Errors: the negative position of the offending argument, checked before any launch; -100 for d > 16; B = 0 or n = 0 returns 0
 * without a launch.
 */
int mf_sde_leg_transitions_f64(int64_t B, int64_t n, int d, const double* F, int per_series, const double* dt, double jitter,
                               double* A, double* cholQ, double* Q, void* stream);
int mf_sde_leg_transitions_f32(int64_t B, int64_t n, int d, const float* F, int per_series, const float* dt, float jitter, float* A,
                               float* cholQ, float* Q, void* stream);
/*
 * Reverse mode of mf_sde_leg_transitions_*: out[b] [d,d] = d/dF of  sum over the steps k of series b of
 * <g_A[b,k], A_k> + <g_cholQ[b,k], chol Q_k>  (g_A, g_cholQ [B,n,d,d], either may be NULL; only the lower triangle of g_cholQ is
 * read; out [B,d,d]).  A caller with a shared F sums out over B.  A step with an all-zero Q contributes through g_A only.  The sum
 * over the steps runs on the device in a fixed order without floating-point atomics (two launches), so two calls agree bit for bit.
 * workspace: mf_sde_leg_transitions_grad_workspace_bytes(B, n, d, sizeof(T)) bytes of device memory.
 */
size_t mf_sde_leg_transitions_grad_workspace_bytes(int64_t B, int64_t n, int d, int elem_size);
int mf_sde_leg_transitions_grad_f64(int64_t B, int64_t n, int d, const double* F, int per_series, const double* dt, double jitter,
                                    const double* g_A, const double* g_cholQ, double* out, void* workspace, size_t workspace_bytes,
                                    void* stream);
int mf_sde_leg_transitions_grad_f32(int64_t B, int64_t n, int d, const float* F, int per_series, const float* dt, float jitter,
                                    const float* g_A, const float* g_cholQ, float* out, void* workspace, size_t workspace_bytes,
                                    void* stream);

/*
 * GaussianProcessRegression.log_likelihood (markovflow/models/gaussian_process_regression.py:150-160) for a Matern kernel or
 * a Sum of two, with the kernel -> state-space-model step FUSED into the Kalman sweep: A_k and chol(Q_k) are generated in
 * registers from dt_k = t_{k+1} - t_k, so a step reads 16 bytes (t, y) instead of the materialised tensors.  One output,
 * zero mean function, H = [1 0 .. | 1 0 ..].  Arguments as for mf_sde_matern_transitions_* - orders: HOST array, ncomp <= 2 - plus
 * time points t [B,T] (strictly increasing), observations y [B,T], rinv [1] (device: 1 / noise variance); out[s] as
 * mf_kf_loglik_*: add_const carries -T/2 log 2 pi + T/2 log rinv.  Workspace: the size mf_kf_loglik_workspace_bytes returns.
 * Returns -101 when the component signature is not instantiated - supported: (1), (3), (5), (3,3), (5,3), (3,5), (5,5) on the
 * register kernels (d <= 6) and ANY concatenation of up to 15 components with 7 <= d <= 15 on the row kernels
 * (csrc/mf_row_gpr.hpp: every lane generates its own row of chol Q_k and column of A_k) - the caller then materialises the
 * model (mf_sde_matern_transitions + mf_kf_loglik).
 *
 * mf_gpr_matern_multi_loglik_*: the same for IndependentMultiOutput (kernels/sde_kernel.py:826-880: one output per component,
 * H[o] = e_{first state of component o}; BASELINE config 4 = three Matern-5/2 components, three outputs): y [B,T,m] with
 * m = ncomp <= 4 (<= 8 for d >= 10), rinv [m,m]; 7 <= d <= 15 (row kernels), -101 otherwise.
 */
int mf_gpr_matern_loglik_f64(int64_t B, int64_t T, int ncomp, const int* orders, const double* lam, const double* var,
                             int per_series, const double* t, const double* y, const double* rinv, double jitter,
                             double add_const, double* out, void* ws, size_t ws_bytes, int* info, int64_t chunks,
                             void* prof_start, void* prof_stop, void* stream);
int mf_gpr_matern_loglik_f32(int64_t B, int64_t T, int ncomp, const int* orders, const float* lam, const float* var,
                             int per_series, const float* t, const float* y, const float* rinv, float jitter,
                             float add_const, float* out, void* ws, size_t ws_bytes, int* info, int64_t chunks,
                             void* prof_start, void* prof_stop, void* stream);
int mf_gpr_matern_multi_loglik_f64(int64_t B, int64_t T, int ncomp, const int* orders, const double* lam, const double* var,
                                   int per_series, const double* t, const double* y, int m, const double* rinv, double jitter,
                                   double add_const, double* out, void* ws, size_t ws_bytes, int* info, int64_t chunks,
                                   void* prof_start, void* prof_stop, void* stream);
int mf_gpr_matern_multi_loglik_f32(int64_t B, int64_t T, int ncomp, const int* orders, const float* lam, const float* var,
                                   int per_series, const float* t, const float* y, int m, const float* rinv, float jitter,
                                   float add_const, float* out, void* ws, size_t ws_bytes, int* info, int64_t chunks,
                                   void* prof_start, void* prof_stop, void* stream);

/*
 * Last line of BaseKalmanFilter.log_likelihood (markovflow/kalman_filter.py:229-231,249-255) as ONE kernel:
 *   out[0] = sum_s per_series[s] + B * ( host_const - num_points * sum_i log chol_obs[i][i] + extra_const[0] )
 * per_series [B]: the output of the per-series entry point above; chol_obs [m,m] (nullable): Cholesky factor of the shared
 * observation covariance, contributing 1/2 T log|R^-1|; extra_const (nullable): one device scalar (e.g. the summed
 * log-determinants of per-step site precisions); host_const: -1/2 m T log(2 pi).  Accumulates in double.
 */
int mf_kf_loglik_total_f64(int64_t B, const double* per_series, int m, const double* chol_obs, int64_t num_points,
                           const double* extra_const, double host_const, double* out, void* stream);
int mf_kf_loglik_total_f32(int64_t B, const float* per_series, int m, const float* chol_obs, int64_t num_points,
                           const float* extra_const, float host_const, float* out, void* stream);

/*
 * Posterior prediction of the state at new time points: conditional_predict of
 * markovflow/conditionals.py:29-83 with _conditional_statistics_from_transitions (:122-203) and base_conditional_predict
 * (:380-420) fused, one lane per (series, new point).  idx [B,Np] (int64, device): insertion index of each new point
 * among the N training points (0..N); A_mt, Q_mt [B,Np,d,d]: transition from the previous training point (or from
 * "minus infinity") to the new point; A_tp, Q_tp: from the new point to the next training point (mf_sde_matern_transitions);
 * means [B,N,d], covs [B,N,d,d], subsequent_covs [B,N-1,d,d] = Cov(x_{k+1}, x_k): the posterior's marginals; prior_mean [B,d],
 * prior_cov [B,d,d]: the stationary state, used beyond both ends (pairwise_marginals, conditionals.py:424-485).
 * out_mean [B,Np,d], out_cov [B,Np,d,d] (NULL: means only).  State dimension 1..9.
 */
int mf_sde_conditional_predict_f64(int64_t B, int64_t N, int64_t Np, int d, const int64_t* idx, const double* A_mt,
                                   const double* Q_mt, const double* A_tp, const double* Q_tp, const double* means,
                                   const double* covs, const double* subsequent_covs, const double* prior_mean,
                                   const double* prior_cov, double* out_mean, double* out_cov, int* info, void* stream);
int mf_sde_conditional_predict_f32(int64_t B, int64_t N, int64_t Np, int d, const int64_t* idx, const float* A_mt,
                                   const float* Q_mt, const float* A_tp, const float* Q_tp, const float* means,
                                   const float* covs, const float* subsequent_covs, const float* prior_mean,
                                   const float* prior_cov, float* out_mean, float* out_cov, int* info, void* stream);

/*
 * conditional_statistics of markovflow/conditionals.py:87-120 (_conditional_statistics_from_transitions, :122-203): for every
 * new time point the statistics of p(x_t | x_-, x_+) = N(P_t [x_-, x_+], T_t) from the transitions x_- -> x_t (A_mt, Q_mt) and
 * x_t -> x_+ (A_tp, Q_tp), each [n, d, d]:  E = Q_mt A_tp^T (Q_tp + A_tp Q_mt A_tp^T)^-1,  D = A_mt - E A_tp A_mt,
 * projections = [D | E] ([n, d, 2d]),  covariances = T = Q_mt - Q_mt A_tp^T (...)^-1 A_tp Q_mt ([n, d, d]).  One lane per point,
 * d <= 9 (-100 beyond).  `info`: raised when Q_tp + A_tp Q_mt A_tp^T is not positive definite.
 */
int mf_sde_conditional_statistics_f64(int64_t n, int d, const double* A_mt, const double* Q_mt, const double* A_tp,
                                      const double* Q_tp, double* projections, double* covariances, int* info, void* stream);
int mf_sde_conditional_statistics_f32(int64_t n, int d, const float* A_mt, const float* Q_mt, const float* A_tp, const float* Q_tp,
                                      float* projections, float* covariances, int* info, void* stream);

/*
 * Reverse mode through the operators: banded_matrices registers a gradient for cholesky_band and inverse_from_cholesky_band
 * (markovflow/block_tri_diag.py:22-31), which is how the CVI models differentiate dist_p.precision -> naturals_to_ssm_params
 * (models/variational_cvi.py:105-136).
 *   mf_btd_cholesky_grad: (g_ldiag [B,T,d,d] lower | NULL, g_lsub [B,T-1,d,d] | NULL) = gradients w.r.t. the factor's blocks ->
 *     (g_diag [B,T,d,d] symmetric, g_sub [B,T-1,d,d]) = gradients w.r.t. the symmetric matrix' blocks.  Local adjoint of the
 *     dense Cholesky per block + the congruence recursion Z_k = C_k + G_k^T Z_{k+1} G_k, G_k = W_k L_k^-1 (parallel in time for
 *     few series) + an axpy.
 *   mf_btd_diag_of_inverse_grad: sigma = the forward's diagonal blocks of (L L^T)^-1; (g_diag | NULL, g_sub | NULL) = gradients
 *     w.r.t. the diagonal / sub-diagonal blocks of the inverse -> (g_ldiag lower, g_lsub).  The block Takahashi recursion run
 *     forward in reverse mode, A_{k+1} = Qbar_{k+1} + G_k A_k G_k^T, between two local kernels.
 * lsub == NULL: block-diagonal factor, B T independent blocks (every d <= 32).  Workspace: mf_btd_grad_workspace_bytes (0: state
 * dimension without these kernels, the entry points then return -100).  d <= 9: register kernels (the workspace is required);
 * 10 <= d <= 32 (round 6, csrc/mf_adj.hip, 16 x 16 MFMA register tiles; the reference differentiates these operators at
 * d = 30, T = 1001): with a workspace of mf_btd_grad_workspace_bytes and at least 32 blocks, terms local in time (a wavefront per
 * block) around one congruence recursion per adjoint, partitioned in time; otherwise (shorter chains, ws == NULL) one wavefront
 * per series walks the block recurrences.
 */
size_t mf_btd_grad_workspace_bytes(int64_t B, int64_t T, int d, int elem_size);
int mf_btd_cholesky_grad_f64(int64_t B, int64_t T, int d, const double* ldiag, const double* lsub, const double* g_ldiag,
                             const double* g_lsub, double* g_diag, double* g_sub, void* ws, size_t ws_bytes, void* stream);
int mf_btd_cholesky_grad_f32(int64_t B, int64_t T, int d, const float* ldiag, const float* lsub, const float* g_ldiag,
                             const float* g_lsub, float* g_diag, float* g_sub, void* ws, size_t ws_bytes, void* stream);
int mf_btd_diag_of_inverse_grad_f64(int64_t B, int64_t T, int d, const double* ldiag, const double* lsub, const double* sigma,
                                    const double* g_diag, const double* g_sub, double* g_ldiag, double* g_lsub, void* ws,
                                    size_t ws_bytes, void* stream);
int mf_btd_diag_of_inverse_grad_f32(int64_t B, int64_t T, int d, const float* ldiag, const float* lsub, const float* sigma,
                                    const float* g_diag, const float* g_sub, float* g_ldiag, float* g_lsub, void* ws,
                                    size_t ws_bytes, void* stream);

/*
 * Gradient of the Kalman log-likelihood with respect to every tensor of the model (the reference
 * gets it from TensorFlow's reverse mode over the banded ops: tests/integration/models/test_gaussian_process_regression.py:117-130,
 * markovflow/models/variational_cvi.py:138-161 for the sites variants).  Fisher's identity,
 * grad log p(y) = E_{x|y}[grad log p(x, y)], evaluated from the smoothed marginals the caller passes in:
 * post_mean [B,T,d], post_cov [B,T,d,d], post_cross [B,T-1,d,d] = Cov(x_{k+1}, x_k) - exact, local in time, one lane per
 * (series, time point).  Outputs, all per series (not summed over the batch): g_mu0 [B,d], g_cholP0 [B,d,d] (lower),
 * g_A [B,T-1,d,d], g_b [B,T-1,d], g_cholQ [B,T-1,d,d] (lower), g_H [B,T,m,d], g_y [B,T,m], and g_omega [B,T,m,m] =
 * E[r r^T] with r = y - H x: the derivative of the log-likelihood with respect to the observation PRECISION of time point k
 * is -1/2 g_omega[k] (+ 1/2 R_k from the log-determinant, which the caller owns).  Rinv: shared [m,m] (rinv_per_step = 0) or
 * [B,T,m,m] (1: KalmanFilterWithSites / WithSparseSites).  H = NULL: no emission model - the expected score of the bare chain
 * under the given moments (used for the q2 half of the KL gradient); y, Rinv, g_H, g_y, g_omega are then ignored.
 * weights [B] (nullable): the incoming gradient of every series' value, applied to all outputs (required for d > 9 or m > 4).
 * State dimension 1..9 with m <= 4: register kernels; 10..15 with m <= 4: row kernels; otherwise (d <= 64 fp32 / 32 fp64, m <= d
 * rounded up to 16) one LDS-tile workgroup per (series, time point) (csrc/mf_biggrad_impl.hpp).
 */
int mf_kf_loglik_grad_f64(int64_t B, int64_t T, int d, int m, const double* mu0, const double* cholP0, const double* A,
                          const double* b, const double* cholQ, const double* H, const double* y, const double* Rinv,
                          int rinv_per_step, const double* post_mean, const double* post_cov, const double* post_cross,
                          double* g_mu0, double* g_cholP0, double* g_A, double* g_b, double* g_cholQ, double* g_H,
                          double* g_y, double* g_omega, const double* weights, int* info, void* stream);
int mf_kf_loglik_grad_f32(int64_t B, int64_t T, int d, int m, const float* mu0, const float* cholP0, const float* A,
                          const float* b, const float* cholQ, const float* H, const float* y, const float* Rinv,
                          int rinv_per_step, const float* post_mean, const float* post_cov, const float* post_cross,
                          float* g_mu0, float* g_cholP0, float* g_A, float* g_b, float* g_cholQ, float* g_H, float* g_y,
                          float* g_omega, const float* weights, int* info, void* stream);

/*
 * The same gradients for FEW, LONG series WITHOUT the smoothed marginals in memory (csrc/mf_grad_lds.hpp): five streamed passes,
 * all partitioned in time - the three of the streamed posterior chain above: chunk summaries, scan, emit (only chol(Q') and b' of
 * the chain are read back), a scan that meets the two sides of every chunk boundary in the smoothed marginal of the chunk's first block,
 * and a forward pass per (series, chunk) that carries (m_k, S_k, Cov(x_{k+1}, x_k)) in registers and writes every gradient once.
 * Replaces mf_kf_posterior_chain -> mf_ssm_marginal_means / _covariances -> mf_kf_loglik_grad for state dimensions 1..6,
 * m <= 3 (per-step precision: m = 1) and 16-byte aligned A, cholQ, g_A, g_cholQ; -101: not this route's call (the caller keeps
 * the three-call route).  Outputs and weights as for mf_kf_loglik_grad; the upper triangles of g_cholP0, g_cholQ are zeros;
 * g_b, g_H, g_y, g_omega may be NULL (not wanted: not computed into memory - a tenth of the pass's traffic).
 * ws: mf_kf_loglik_grad_streamed_workspace_bytes (0: not this route's call); it holds the posterior chain, (4 d^2 + 3 d) s bytes
 * per step.  chunks: time partitions per series, 0 = automatic (>= 2).  prof_start / prof_stop: optional hipEvent_t recorded
 * around the kernels.
 * fwd_ws (nullable): the workspace of the mf_kf_loglik call that evaluated the SAME inputs, untouched since, together with the
 * partition mf_kf_loglik_plan reports for that call (path 2: the streaming level-0 kernel, whose per-chunk summaries are the
 * first thing in its workspace).  The Schur complement of a chunk's interior does not depend on the direction of the
 * elimination, so those summaries replace the first two passes and the boundary scan: three passes instead of five.
 * Reference: TensorFlow reverse mode through markovflow/kalman_filter.py:184-255.
 */
size_t mf_kf_loglik_grad_streamed_workspace_bytes(int64_t B, int64_t T, int d, int m, int rinv_per_step, int elem_size,
                                                  int64_t chunks);
int mf_kf_loglik_grad_streamed_f64(int64_t B, int64_t T, int d, int m, const double* mu0, const double* cholP0, const double* A,
                                   const double* b, const double* cholQ, const double* H, const double* y, const double* Rinv,
                                   int rinv_per_step, const double* weights, double* g_mu0, double* g_cholP0, double* g_A,
                                   double* g_b, double* g_cholQ, double* g_H, double* g_y, double* g_omega, void* ws,
                                   size_t ws_bytes, int* info, int64_t chunks, const void* fwd_ws, int64_t fwd_chunks_per_series,
                                   int64_t fwd_chunk_length, void* prof_start, void* prof_stop, void* stream);
int mf_kf_loglik_grad_streamed_f32(int64_t B, int64_t T, int d, int m, const float* mu0, const float* cholP0, const float* A,
                                   const float* b, const float* cholQ, const float* H, const float* y, const float* Rinv,
                                   int rinv_per_step, const float* weights, float* g_mu0, float* g_cholP0, float* g_A,
                                   float* g_b, float* g_cholQ, float* g_H, float* g_y, float* g_omega, void* ws,
                                   size_t ws_bytes, int* info, int64_t chunks, const void* fwd_ws, int64_t fwd_chunks_per_series,
                                   int64_t fwd_chunk_length, void* prof_start, void* prof_stop, void* stream);
/*
 * posterior_state_space_model AFTER log_likelihood on the same inputs - the smoother reuses the filter's pass: fwd_ws is the
 * workspace of that mf_kf_loglik call (untouched since; partition from mf_kf_loglik_plan, path 2), whose per-chunk summaries
 * replace the first pass of the streamed kernels (mf_kf_posterior_chain with a workspace): one scan over the summaries for the
 * boundary states, then the emit pass alone (3.9-5.4 ms instead of 5.4-6.7 at B=1024, T=10000, d=6 fp64).  Same outputs.
 * ws: mf_kf_posterior_chain_from_filter_workspace_bytes (0: not covered).  -101: not this route's call.
 */
size_t mf_kf_posterior_chain_from_filter_workspace_bytes(int64_t B, int64_t T, int d, int m, int rinv_per_step, int elem_size,
                                                         int64_t fwd_chunks_per_series);
int mf_kf_posterior_chain_from_filter_f64(int64_t B, int64_t T, int d, int m, const double* mu0, const double* cholP0,
                                          const double* A, const double* b, const double* cholQ, const double* H, const double* y,
                                          const double* Rinv, int rinv_per_step, double* a_post, double* mu0_post, double* b_post,
                                          double* cholP0_post, double* cholQ_post, void* ws, size_t ws_bytes, int* info,
                                          const void* fwd_ws, int64_t fwd_chunks_per_series, int64_t fwd_chunk_length,
                                          void* prof_start, void* prof_stop, void* stream);
int mf_kf_posterior_chain_from_filter_f32(int64_t B, int64_t T, int d, int m, const float* mu0, const float* cholP0,
                                          const float* A, const float* b, const float* cholQ, const float* H, const float* y,
                                          const float* Rinv, int rinv_per_step, float* a_post, float* mu0_post, float* b_post,
                                          float* cholP0_post, float* cholQ_post, void* ws, size_t ws_bytes, int* info,
                                          const void* fwd_ws, int64_t fwd_chunks_per_series, int64_t fwd_chunk_length,
                                          void* prof_start, void* prof_stop, void* stream);

/*
 * The posterior of the same GP-regression models as a state space model (markovflow/models/gaussian_process_regression.py:130-148
 * builds its posterior process from it) without materialising the prior's tensors: boundary states from the summaries the fused
 * forward mf_gpr_matern_loglik left in its workspace (explicit chunk count, partition as for mf_gpr_matern_loglik_grad), then the
 * emit pass of the streamed posterior chain with the transitions generated in registers (csrc/mf_gpr_grad.hpp).  Outputs as
 * mf_kf_posterior_chain.  ws: mf_gpr_matern_posterior_chain_workspace_bytes.  -101: signature or partition not covered.
 */
size_t mf_gpr_matern_posterior_chain_workspace_bytes(int64_t B, int64_t T, int d, int elem_size, int64_t fwd_chunks_per_series);
int mf_gpr_matern_posterior_chain_f64(int64_t B, int64_t T, int ncomp, const int* orders, const double* lam, const double* var,
                                      int per_series, const double* t, const double* y, const double* rinv, double jitter,
                                      double* a_post, double* mu0_post, double* b_post, double* cholP0_post, double* cholQ_post,
                                      void* ws, size_t ws_bytes, int* info, const void* fwd_ws, int64_t fwd_chunks_per_series,
                                      int64_t fwd_chunk_length, void* stream);
int mf_gpr_matern_posterior_chain_f32(int64_t B, int64_t T, int ncomp, const int* orders, const float* lam, const float* var,
                                      int per_series, const float* t, const float* y, const float* rinv, float jitter,
                                      float* a_post, float* mu0_post, float* b_post, float* cholP0_post, float* cholQ_post,
                                      void* ws, size_t ws_bytes, int* info, const void* fwd_ws, int64_t fwd_chunks_per_series,
                                      int64_t fwd_chunk_length, void* stream);

/*
 * The backward of the fused GP-regression log-likelihood mf_gpr_matern_loglik: a Sum of one or two Matern components, one output - the
 * training step
 * of markovflow/models/gaussian_process_regression.py:150-160 under a GradientTape - with the kernel -> state-space-model step
 * fused into its passes (csrc/mf_gpr_grad.hpp): the transitions are generated in registers from (t, hyper-parameters) inside the
 * emit pass and the gradient pass of the streamed backward, 16 bytes of model per step; the model tensors never exist.
 * fwd_ws: the workspace of the mf_gpr_matern_loglik call on the SAME inputs with an EXPLICIT chunk count C, untouched since;
 * its partition is fwd_chunk_length = ceil((T-1) / C), fwd_chunks_per_series = ceil((T-1) / fwd_chunk_length) >= 2.
 * Outputs: g_packed [B,T-1,rec] - the derivative of sum_s weights[s] log p(y_s) with respect to the transitions and the Cholesky
 * factors of the process covariances, ONE record per transition: [the k x k diagonal block of g_A of every component, row-major |
 * the lower triangle of the diagonal block of g_cholQ of every component, row-major], each part padded to 16 bytes (30 values at
 * d = 3 + 3 in fp64 instead of 72) - the input of mf_sde_matern_transitions_grad_packed, which reduces it to the hyper-parameters -,
 * g_cholP0 [B,d,d] (the stationary prior's factor), g_omega [B,T] (nullable; E[r^2] per time point: the
 * derivative with respect to the noise PRECISION is -1/2 of it, + 1/2 R from the log-determinant, which the caller owns).
 * ws: mf_gpr_matern_loglik_grad_workspace_bytes.  -101: signature or partition not covered (materialise instead).
 */
size_t mf_gpr_matern_loglik_grad_workspace_bytes(int64_t B, int64_t T, int d, int elem_size, int64_t fwd_chunks_per_series);
int mf_gpr_matern_loglik_grad_f64(int64_t B, int64_t T, int ncomp, const int* orders, const double* lam, const double* var,
                                  int per_series, const double* t, const double* y, const double* rinv, double jitter,
                                  const double* weights, double* g_packed, double* g_cholP0, double* g_omega,
                                  void* ws, size_t ws_bytes, int* info, const void* fwd_ws, int64_t fwd_chunks_per_series,
                                  int64_t fwd_chunk_length, void* stream);
int mf_gpr_matern_loglik_grad_f32(int64_t B, int64_t T, int ncomp, const int* orders, const float* lam, const float* var,
                                  int per_series, const float* t, const float* y, const float* rinv, float jitter,
                                  const float* weights, float* g_packed, float* g_cholP0, float* g_omega,
                                  void* ws, size_t ws_bytes, int* info, const void* fwd_ws, int64_t fwd_chunks_per_series,
                                  int64_t fwd_chunk_length, void* stream);
/* The level-0 kernel (path: 0 row kernels, 1 spike-in-LDS, 2 streaming, 3 direct loads) and time partition mf_kf_loglik chooses
 * for a call; aligned16: A and cholQ are 16-byte aligned. */
int mf_kf_loglik_plan(int64_t B, int64_t T, int d, int m, int rinv_per_step, int elem_size, int64_t chunks, int aligned16,
                      int* path, int64_t* chunks_per_series, int64_t* chunk_length);

/*
 * Gradient of  KL(q1 || q2)  between two state space models (markovflow/state_space_model.py:528-593; differentiated by
 * TensorFlow in the reference, pinned by tests/integration/models/test_variational.py:123-132) with respect to the parameters
 * of q1: the adjoints of q1's marginal mean and covariance, lam_k = n_k + A^T lam_{k+1}, M_k = N_k + A^T M_{k+1} A, in three
 * kernels - per-step inputs (parallel), a light sequential recursion per series, per-step parameter gradients (parallel);
 * csrc/mf_kl_grad.hpp.  ws: mf_ssm_adjoint_workspace_bytes.
 * means_1 [B,T,d], covs_1 [B,T,d,d]: marginals of q1 (mf_ssm_marginal_means / mf_ssm_marginal_covariances).  Outputs per series:
 * g_mu0 [B,d], g_cholP0 [B,d,d] (lower), g_A [B,T-1,d,d], g_b [B,T-1,d], g_cholQ [B,T-1,d,d] (lower), scaled by weights [B]
 * (nullable).  adj_N [B,T,d,d], adj_n [B,T,d] (both or neither): the inputs of the recursion when the forward kept them
 * (mf_ssm_kl_divergence: out_N, out_n); NULL: they are formed here.
 * The gradient with respect to q2 is MINUS mf_kf_loglik_grad with H = NULL, q2's parameters and q1's moments.
 * State dimension 1..9; 10..15 (row kernels) with adj_N / adj_n given only (-100 without them: the kernel that forms them is
 * not compiled in row form).
 */
int mf_ssm_kl_grad_f64(int64_t B, int64_t T, int d, const double* mu0_1, const double* cholP0_1, const double* A_1,
                       const double* b_1, const double* cholQ_1, const double* mu0_2, const double* cholP0_2, const double* A_2,
                       const double* b_2, const double* cholQ_2, const double* means_1, const double* covs_1,
                       const double* weights, const double* adj_N, const double* adj_n, double* g_mu0, double* g_cholP0,
                       double* g_A, double* g_b, double* g_cholQ, void* ws, size_t ws_bytes, int* info, void* stream);
int mf_ssm_kl_grad_f32(int64_t B, int64_t T, int d, const float* mu0_1, const float* cholP0_1, const float* A_1,
                       const float* b_1, const float* cholQ_1, const float* mu0_2, const float* cholP0_2, const float* A_2,
                       const float* b_2, const float* cholQ_2, const float* means_1, const float* covs_1, const float* weights,
                       const float* adj_N, const float* adj_n, float* g_mu0, float* g_cholP0, float* g_A, float* g_b,
                       float* g_cholQ, void* ws, size_t ws_bytes, int* info, void* stream);

/*
 * KalmanFilter._r_inv (markovflow/kalman_filter.py:341-348): R^-1 = (L L^T)^-1 from the Cholesky factor L [m,m] of the shared
 * observation covariance (the reference: tf.linalg.cholesky_solve against the identity), out [m,m].  m <= 32; one launch.
 */
int mf_obs_precision_from_chol_f64(int m, const double* chol, double* out, int* info, void* stream);
int mf_obs_precision_from_chol_f32(int m, const float* chol, float* out, int* info, void* stream);

/*
 * BaseKalmanFilter.posterior_state_space_model (markovflow/kalman_filter.py:109-182) fused: the posterior precision and the
 * information vector (state_space_model.py:431-483, kalman_filter.py:86-101,149-156) are assembled block by block INSIDE the
 * backward U D U^T recursion (block_tri_diag.py:438-545) and the five tensors of the posterior chain are written directly:
 * a_post [B,T-1,d,d] (= -U^T), mu0_post [B,d], b_post [B,T-1,d], cholP0_post [B,d,d], cholQ_post [B,T-1,d,d].  Nothing else
 * touches HBM: the precision, its factor and the solves of the reference's route (mf_ssm_precision + mf_btd_udl here) never exist.
 * Rinv shared [m,m] or per step [B,T,m,m]; m <= 4; state dimension 1..9.  Two forms:
 *   ws == NULL           one lane per series, ONE backward sweep: (4 d^2 + 3 d + m d + m) s bytes per step.  For batches that
 *                        fill the chip (thousands of series) and for short chains.
 *   ws != NULL           (mf_kf_posterior_chain_workspace_bytes > 0 and a workspace of that size; d <= 6, m <= 3 or m = 1 with
 *                        per-step precisions, 16-byte aligned tensors - otherwise the call quietly takes the first form):
 *                        partitioned in TIME like mf_kf_loglik and streamed by LDS-DMA (csrc/mf_post_lds.hpp).  Pass 1: a lane
 *                        per (series, chunk) eliminates its chunk backwards with the fill-in carried to the chunk's right end;
 *                        pass 2: a scan over the chunk summaries gives the recursion's state at every chunk boundary; pass 3:
 *                        every chunk restarts the recursion there and writes the chain.  The inputs are read twice, coalesced,
 *                        every output once.  `chunks` = chunks per series (0 = fill the chip); prof_start / prof_stop: optional
 *                        hipEvent_t recorded on `stream` around the three kernels.
 */
size_t mf_kf_posterior_chain_workspace_bytes(int64_t B, int64_t T, int d, int m, int rinv_per_step, int elem_size,
                                             int64_t chunks);
int mf_kf_posterior_chain_f64(int64_t B, int64_t T, int d, int m, const double* mu0, const double* cholP0, const double* A,
                              const double* b, const double* cholQ, const double* H, const double* y, const double* Rinv,
                              int rinv_per_step, double* a_post, double* mu0_post, double* b_post, double* cholP0_post,
                              double* cholQ_post, void* ws, size_t ws_bytes, int* info, int64_t chunks, void* prof_start,
                              void* prof_stop, void* stream);
int mf_kf_posterior_chain_f32(int64_t B, int64_t T, int d, int m, const float* mu0, const float* cholP0, const float* A,
                              const float* b, const float* cholQ, const float* H, const float* y, const float* Rinv,
                              int rinv_per_step, float* a_post, float* mu0_post, float* b_post, float* cholP0_post,
                              float* cholQ_post, void* ws, size_t ws_bytes, int* info, int64_t chunks, void* prof_start,
                              void* prof_stop, void* stream);

/*
 * KL(q1 || q2) between two state space models, one scalar per series (markovflow/state_space_model.py:528-593), fused: ONE
 * forward sweep per series carries q1's marginal mean and covariance in registers and accumulates the divergence from the
 * local form  1/2 sum_k [ tr(Q2^-1 Q1) + tr(Q2^-1 dA S_k dA^T) + eps_k^T Q2^-1 eps_k ] - T d / 2 + log-determinants
 * (csrc/mf_kl_grad.hpp) - the ten parameter tensors are read once and nothing else touches HBM.  One lane per series when the
 * batch fills the chip.  With few, long chains (mf_ssm_kl_workspace_bytes > 0 and a workspace of that size) q1's marginals come
 * from the scans in time and the same local terms are formed by one lane per (series, step) and summed per series; on that
 * route the marginals of q1 can be kept: out_means [B,T,d], out_covs [B,T,d,d], out_cross [B,T-1,d,d] = Cov(x_{k+1}, x_k) (means
 * and covariances together, the cross-covariances optionally on top; -15 otherwise) - exactly what mf_ssm_kl_grad /
 * mf_kf_loglik_grad need; the sweep per series carries the same quantities in registers and writes them on request.
 * out_N [B,T,d,d], out_n [B,T,d] (both or neither; either route): N_k = dA_k^T Q2_k^-1 dA_k, n_k = dA_k^T Q2_k^-1 eps_k, the
 * inputs of the adjoint recursion of mf_ssm_kl_grad - by-products of the forward sweep that save the backward a kernel.
 * State dimension 1..15 (10..15: where mf_row_operators_cover holds).
 * State dimension 16..32, T > 1, every by-product pointer NULL and a workspace of mf_ssm_kl_workspace_bytes: the value alone, in
 * the reference's operator form (the block rows of q2's precision against q1's marginal / subsequent covariances,
 * state_space_model.py:569-593) evaluated in ONE walk per (series, chunk of the time axis) on 16 x 16 MFMA register tiles
 * (csrc/mf_wave_ops.hpp, wave_kl_walk_kernel): q1's moment recursion, q2's means and the block terms together, neither the moments
 * nor the precision in memory; -100 with by-products requested (their consumers, mf_ssm_kl_grad_*, stop at d = 9), -15 without
 * the workspace.  `info` is not written on this route (a non-positive diagonal of a factor yields NaN in `out`).
 */
size_t mf_ssm_kl_workspace_bytes(int64_t B, int64_t T, int d, int elem_size);
int mf_ssm_kl_divergence_f64(int64_t B, int64_t T, int d, const double* mu0_1, const double* cholP0_1, const double* A_1,
                             const double* b_1, const double* cholQ_1, const double* mu0_2, const double* cholP0_2,
                             const double* A_2, const double* b_2, const double* cholQ_2, double* out, double* out_means,
                             double* out_covs, double* out_cross, double* out_N, double* out_n, void* ws, size_t ws_bytes,
                             int* info, void* stream);
int mf_ssm_kl_divergence_f32(int64_t B, int64_t T, int d, const float* mu0_1, const float* cholP0_1, const float* A_1,
                             const float* b_1, const float* cholQ_1, const float* mu0_2, const float* cholP0_2, const float* A_2,
                             const float* b_2, const float* cholQ_2, float* out, float* out_means, float* out_covs,
                             float* out_cross, float* out_N, float* out_n, void* ws, size_t ws_bytes, int* info, void* stream);

/*
 * KL(q1 || q2) for 16 <= d <= 32 from q1's MOMENTS (markovflow/state_space_model.py:528-593: the reference assembles q2's precision,
 * multiplies it block by block with q1's marginal / subsequent covariances and sums, :569-573).  One wavefront per (series, block)
 * forms block row k of q2's precision on register tiles (as mf_ssm_precision does) and reduces it on the spot against
 * covs_1 [B,T,d,d], cross_1 [B,T-1,d,d] = Cov(x_{k+1}, x_k) and mean_diff [B,T,d] = mu_2 - mu_1; the two log-determinants ride along
 * (q1's factors are read on their diagonals only); a second small kernel sums the T terms of a series in a fixed order.  q2's
 * precision never exists in memory.  ws: mf_ssm_kl_from_moments_workspace_bytes (B T scalars).  -100 outside 16 <= d <= 32.
 * The strict upper triangles of q2's factors are not read.  T = 1: cholQ_1, A_2, cholQ_2 and cross_1 may be NULL.
 * (StateSpaceModel.kl_divergence takes the one-walk kernel above at these state dimensions; this entry point stays as a tested
 * part of the C interface for callers that hold q1's moments already - tests/test_gpu_kl_from_moments.py.)
 */
size_t mf_ssm_kl_from_moments_workspace_bytes(int64_t B, int64_t T, int d, int elem_size);
int mf_ssm_kl_from_moments_f64(int64_t B, int64_t T, int d, const double* cholP0_1, const double* cholQ_1, const double* cholP0_2,
                               const double* A_2, const double* cholQ_2, const double* covs_1, const double* cross_1,
                               const double* mean_diff, double* out, void* ws, size_t ws_bytes, void* stream);
int mf_ssm_kl_from_moments_f32(int64_t B, int64_t T, int d, const float* cholP0_1, const float* cholQ_1, const float* cholP0_2,
                               const float* A_2, const float* cholQ_2, const float* covs_1, const float* cross_1,
                               const float* mean_diff, float* out, void* ws, size_t ws_bytes, void* stream);

/*
 * Adjoint of the marginal recursion  m_{k+1} = A_k m_k + b_k,  S_{k+1} = A_k S_k A_k^T + Q_k  (markovflow/state_space_model.py:232-262,
 * differentiated by TensorFlow in the reference: the expected log-likelihood of every variational model goes through
 * `marginals`, models/variational.py:150, models/sparse_variational.py:178-192).  Given the incoming gradients g_means [B,T,d] and
 * g_covs [B,T,d,d] (either may be NULL = zero) of a scalar with respect to the marginal means / covariances, and the
 * marginals themselves (means, covs), the gradients with respect to mu0, cholP0 (lower), A, b and cholQ (lower): the same
 * recursion as mf_ssm_kl_grad with (N_k, n_k) = (g_covs_k + g_covs_k^T, g_means_k), then a parallel kernel.  ws:
 * mf_ssm_adjoint_workspace_bytes.  State dimension 1..9.
 */
int mf_ssm_marginals_grad_f64(int64_t B, int64_t T, int d, const double* cholP0, const double* A, const double* cholQ,
                              const double* means, const double* covs, const double* g_means, const double* g_covs,
                              double* g_mu0, double* g_cholP0, double* g_A, double* g_b, double* g_cholQ, void* ws,
                              size_t ws_bytes, void* stream);
int mf_ssm_marginals_grad_f32(int64_t B, int64_t T, int d, const float* cholP0, const float* A, const float* cholQ,
                              const float* means, const float* covs, const float* g_means, const float* g_covs, float* g_mu0,
                              float* g_cholP0, float* g_A, float* g_b, float* g_cholQ, void* ws, size_t ws_bytes, void* stream);

/* Workspace of mf_ssm_kl_grad_* and mf_ssm_marginals_grad_*: per (series, block) the inputs (N_k, n_k) and the results
 * (M_k, lambda_k) of the adjoint recursion - (2 d^2 + 2 d) elements. */
size_t mf_ssm_adjoint_workspace_bytes(int64_t B, int64_t T, int d, int elem_size);

/*
 * Likelihoods of the CVI model (markovflow/models/variational_cvi.py:321-368 over gpflow's likelihoods; csrc/mf_lik.hip).  One
 * lane per data point, N points (a batch of series flattened).  `lik`: 0 Gaussian, params [variance]; 1 Bernoulli with gpflow's
 * probit link  p = 0.5 (1 + erf(f / sqrt 2)) (1 - 2e-3) + 1e-3, y in {0, 1}, no params; 2 Poisson with exp link and bin size 1,
 * no params; 3 Student-t, params [scale, df, lgamma((df + 1) / 2) - lgamma(df / 2) - log(df pi) / 2 - log(scale)].
 * `params`, `nodes` and `weights` are HOST arrays of doubles in both precisions (as `orders` / `osc` of mf_sde_transitions):
 * the nq <= 32 nodes and weights of a Gauss-Hermite rule (numpy.polynomial.hermite.hermgauss; weights sum to sqrt pi), which
 * travel by value in the kernel arguments.  Gaussian and Poisson expectations are closed forms; Bernoulli and Student-t are
 *   VE = sum w_i l(f_i),  dVE/dmu = sum w_i l'(f_i),  dVE/dvar = sum w_i l'(f_i) x_i / sqrt(2 var),   f_i = mu + sqrt(2 var) x_i,
 * w_i = weights_i / sqrt pi: the exact derivatives of the discretised sum.  A point with fvar <= 0 or NaN gets NaN in its own
 * outputs.  Returns 0, -(position of the offending argument) - unknown lik, nq outside 1..32, a missing or non-positive
 * parameter, a NULL array - or -1000 (launch failed); N = 0 returns 0 without a launch.
 *
 * mf_lik_variational_expectations: ve, g_mu, g_var [N], any of them may be NULL.
 * mf_lik_cvi_site_update: nat1, nat2 [N] updated IN PLACE with the gradient in the expectation parameters [mu, var + mu^2],
 *   g2 = dVE/dvar, g1 = dVE/dmu - 2 g2 mu, nat <- (1 - lr) nat + lr g  (0 <= lr <= 1); ve [N] optional.
 * mf_lik_predict_log_density: out [N] = log int p(y | f) N(f | mu, var) df - Gaussian in closed form, the others as a
 *   log-sum-exp over the nodes shifted by its maximum.
 */
int mf_lik_variational_expectations_f64(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                                        const double* fmu, const double* fvar, const double* y, double* ve, double* g_mu,
                                        double* g_var, void* stream);
int mf_lik_variational_expectations_f32(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                                        const float* fmu, const float* fvar, const float* y, float* ve, float* g_mu, float* g_var,
                                        void* stream);
int mf_lik_cvi_site_update_f64(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                               const double* fmu, const double* fvar, const double* y, double lr, double* nat1, double* nat2,
                               double* ve, void* stream);
int mf_lik_cvi_site_update_f32(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                               const float* fmu, const float* fvar, const float* y, float lr, float* nat1, float* nat2, float* ve,
                               void* stream);
int mf_lik_predict_log_density_f64(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                                   const double* fmu, const double* fvar, const double* y, double* out, void* stream);
int mf_lik_predict_log_density_f32(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                                   const float* fmu, const float* fvar, const float* y, float* out, void* stream);

/*
 * Power expectation propagation (markovflow/models/pep.py:99-215; csrc/mf_lik.hip).  N, lik, params, nq, nodes and weights as above;
 * alpha in (0, 1] is the power, lr in [0, 1] the damping.
 *
 * mf_lik_log_expected_density: led [N] = I(mu, var; alpha) = log int p(y | f)^alpha N(f | mu, var) df,  g1 = dI/dmu,  g2 = d2I/dmu2;
 *   any of the three may be NULL.  Gaussian in closed form, the others on the rule: with v_i = alpha l(f_i) + log w_i and
 *   p_i = softmax_i v_i,  I = logsumexp_i v_i,  g1 = sum p_i alpha l'(f_i),  g2 = sum p_i (alpha l''(f_i) + alpha^2 l'(f_i)^2) - g1^2
 *   - the exact derivatives of the discretised sum, accumulated in one pass under the running maximum.  Poisson's - lgamma(y + 1)
 *   enters multiplied by alpha.  At alpha = 1, led is mf_lik_predict_log_density's out.
 * mf_lik_pep_site_update: one step on the sites t(f) = exp(nat1 f + nat2 f^2 + log_norm), [N] each, IN PLACE, from the posterior
 *   marginals fmu, fvar of f:  cavity 1 / v_c = 1 / fvar + 2 alpha nat2,  mu_c = v_c (fmu / fvar - alpha nat1);  I, g1, g2 at the
 *   cavity;  den = 1 + v_c g2,  L2 = g2 / (2 den),  L1 = (g1 - mu_c g2) / den;  normaliser I + G(mu_c, v_c) - G(fmu, fvar) with
 *   G(mu, v) = (log v + mu^2 / v) / 2;  pep = (1 - alpha) old + (L1, L2, normaliser),  new = (1 - lr) old + lr pep.
 *   `update` [N] (bytes, may be NULL = every point): a point whose flag is 0 is left as it is, and so - all three numbers, bit for
 *   bit - is a point where fvar, 1 / v_c or den is not > 0 or a new value is not finite.  cav_mu, cav_var [N] (may be NULL) get the
 *   cavity of EVERY point, NaN where it does not exist.
 */
int mf_lik_log_expected_density_f64(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                                    double alpha, const double* fmu, const double* fvar, const double* y, double* led, double* g1,
                                    double* g2, void* stream);
int mf_lik_log_expected_density_f32(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                                    float alpha, const float* fmu, const float* fvar, const float* y, float* led, float* g1, float* g2,
                                    void* stream);
int mf_lik_pep_site_update_f64(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                               double alpha, double lr, const double* fmu, const double* fvar, const double* y,
                               const unsigned char* update, double* nat1, double* nat2, double* log_norm, double* cav_mu,
                               double* cav_var, void* stream);
int mf_lik_pep_site_update_f32(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                               float alpha, float lr, const float* fmu, const float* fvar, const float* y, const unsigned char* update,
                               float* nat1, float* nat2, float* log_norm, float* cav_mu, float* cav_var, void* stream);

/*
 * The segmented site update of the sparse CVI model (markovflow/models/sparse_variational_cvi.py:176-221; csrc/mf_lik.hip): B
 * series of N data points, S = M + 1 sites per series on the pairs of neighbouring inducing states, two_d = 2 d in 2, 4, ..., 18.
 *   seg_offsets [B, S + 1] int64  the points seg_offsets[b, s] <= k < seg_offsets[b, s + 1] of series b belong to site s
 *                                 (ascending, 0 first and N last; built by the caller, not validated on the device)
 *   w [B, N, 2d]                  H P_k, the projection of the pair [u_-, u_+] onto f_k
 *   c [B, N]                      H T_k H^T, the conditional variance of f_k given the pair
 *   y [B, N]                      observations
 *   pair_mean [B, S, 2d], pair_cov [B, S, 2d, 2d]   marginals of q on the pairs (conditionals.pairwise_marginals)
 *   nat1 [B, S, 2d], nat2 [B, S, 2d, 2d]            the sites, updated IN PLACE; BOTH NULL: projection only
 *   fmu, fvar, ve [B, N]          optional outputs, any of them may be NULL
 * Per point k of segment s:  fmu = w_k . m_s,  fvar = c_k + w_k^T S_s w_k,  (ve, gm, gv) as mf_lik_variational_expectations,
 * g2 = gv, g1 = gm - 2 gv fmu;  per segment  nat1_s <- (1 - lr) nat1_s + lr sum_k g1 w_k,
 * nat2_s <- (1 - lr) nat2_s + lr sum_k g2 w_k w_k^T  (an empty segment decays).  The sums run over the points in ascending order:
 * no floating-point atomics, the same bits on every launch and for a series alone or inside a batch.  A point with fvar <= 0 or
 * NaN gets NaN in its own fmu / fvar / ve and makes its segment's sites NaN; every other segment is untouched by it.
 * Returns 0, -(position of the offending argument in THIS signature: 1 B, 2 N, 3 S, 5 lik, 6 params, 7 nq, 8 nodes, 9 weights,
 * 10 ... 15 a NULL input, 16 lr outside [0, 1], 17 / 18 one of nat1 / nat2 NULL without the other), -100 for a two_d that is
 * odd, < 2 or > 18, or -1000 (launch failed).  Nothing is launched on an error, for B = 0, or when nothing is asked for.
 */
int mf_lik_sparse_cvi_site_update_f64(int64_t B, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq,
                                      const double* nodes, const double* weights, const int64_t* seg_offsets, const double* w,
                                      const double* c, const double* y, const double* pair_mean, const double* pair_cov, double lr,
                                      double* nat1, double* nat2, double* fmu, double* fvar, double* ve, void* stream);
int mf_lik_sparse_cvi_site_update_f32(int64_t B, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq,
                                      const double* nodes, const double* weights, const int64_t* seg_offsets, const float* w,
                                      const float* c, const float* y, const float* pair_mean, const float* pair_cov, float lr,
                                      float* nat1, float* nat2, float* fmu, float* fvar, float* ve, void* stream);

/*
 * The data term of the SVGP ELBO and its adjoint onto the pair marginals (markovflow/models/sparse_variational.py:149-192;
 * csrc/mf_lik.hip): B, N, S, two_d, the likelihood, the rule, seg_offsets, w, c, y, pair_mean and pair_cov as for
 * mf_lik_sparse_cvi_site_update_*.  Per point k of segment s:  fmu = w_k . m_s,  fvar = c_k + w_k^T S_s w_k,  (ve, gm, gv) as
 * mf_lik_variational_expectations;  per segment
 *   ve_sum [B, S]           sum_k ve_k
 *   g_mean [B, S, 2d]       sum_k gm_k w_k            d ve_sum_s / d m_s
 *   g_cov  [B, S, 2d, 2d]   sum_k gv_k w_k w_k^T      d ve_sum_s / d S_s for an unconstrained S_s (symmetric, both triangles written)
 * g_mean and g_cov BOTH NULL: the value only (the same bits); ve_sum may be NULL beside the gradients.
 * Two passes.  Pass 1 runs one wavefront per TILE - at most 64 consecutive points of one segment, tile j of a segment starting at
 * the segment's first point + 64 j - and leaves the tile's 2d (2d + 1) / 2 + 2d + 1 partial sums as one row of the workspace; pass
 * 2 adds a segment's rows in ascending tile order.  The caller supplies the tile table (int64, built from seg_offsets):
 *   num_tiles               sum over the segments of ceil(length / 64)
 *   tile_seg [num_tiles]    series * S + segment of every tile, ascending
 *   seg_tile [B S + 1]      the first tile of every segment (exclusive prefix sum; the last entry is num_tiles)
 * and the workspace, mf_lik_sparse_expectations_workspace_bytes(num_tiles, two_d, sizeof(T)) bytes (0 for num_tiles = 0).  The
 * table is clamped on the device, not validated: a wrong one gives wrong numbers and no access outside the buffers.
 * No floating-point atomics: every sum runs over the points in ascending order, the same bits on every launch and for a series
 * alone or inside a batch.  A point with fvar <= 0 or NaN makes the three outputs of ITS segment NaN; no other segment is touched.
 * An empty segment, and every segment for N = 0, gets zeros.  No allocation, no synchronisation.
 * Returns 0, -(position of the offending argument in THIS signature: 1 B, 2 N, 3 S, 5 lik, 6 params, 7 nq, 8 nodes, 9 weights,
 * 10 ... 15 a NULL input, 16 num_tiles negative, above 2^31 - 1 or non-zero for N = 0, 17 / 18 a NULL table, 19 a NULL workspace,
 * 20 a workspace that is too small, 22 / 23 one of g_mean / g_cov NULL without the other), -100 for a two_d that is odd, < 2 or
 * > 18, or -1000 (launch failed).  Nothing is launched on an error, for B = 0, or when every output is NULL.
 */
size_t mf_lik_sparse_expectations_workspace_bytes(int64_t num_tiles, int two_d, int elem_size);
int mf_lik_sparse_expectations_f64(int64_t B, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq,
                                   const double* nodes, const double* weights, const int64_t* seg_offsets, const double* w,
                                   const double* c, const double* y, const double* pair_mean, const double* pair_cov,
                                   int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* workspace,
                                   size_t workspace_bytes, double* ve_sum, double* g_mean, double* g_cov, void* stream);
int mf_lik_sparse_expectations_f32(int64_t B, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq,
                                   const double* nodes, const double* weights, const int64_t* seg_offsets, const float* w,
                                   const float* c, const float* y, const float* pair_mean, const float* pair_cov,
                                   int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* workspace,
                                   size_t workspace_bytes, float* ve_sum, float* g_mean, float* g_cov, void* stream);

/*
 * The data term of the SVGP ELBO for a likelihood with SEVERAL latent functions per observation, and its adjoint onto the pair
 * marginals (markovflow/models/sparse_variational.py:149-192 with markovflow/likelihoods/mutlistage_likelihood.py underneath;
 * csrc/mf_lik.hip).  B, N, S, two_d, the rule, seg_offsets, y, pair_mean, pair_cov, the tile table, the workspace and the three
 * outputs as for mf_lik_sparse_expectations_*; every point carries L = latent_dim DENSE projections of the pair,
 *   w [B, N, L, 2d]   row l: H_l P_k        c [B, N, L]   H_l T_k H_l^T (the diagonal of the output covariance)
 * Per point k of segment s and latent l:  mu_l = w_kl . m_s,  s2_l = c_kl + w_kl^T S_s w_kl;  (ve, gm_l, gv_l) of the likelihood
 * at (mu, s2, y_k);  per segment, over the points in ascending order and within a point over the latents in ascending order,
 *   ve_sum = sum_k ve_k      g_mean = sum_k sum_l gm_kl w_kl      g_cov = sum_k sum_l gv_kl w_kl w_kl^T
 * lik = 4, latent_dim = 3 is the multi-stage likelihood (no parameters: params is not read), with the Bernoulli's probit link and
 * the Poisson's exp link:  y == 0: B1(F0);  y == 1: B0(F0) + B1(F1);  y >= 2: B0(F0) + B0(F1) + Poisson(y - 2 | exp F2);  any other
 * y (a fraction, a negative number, NaN): exactly 0.  B1 = log sigma and B0 = log(1 - sigma) by the nq-point rule, the Poisson term
 * in closed form (float32: the link inside B1 / B0 is evaluated from its small side, 0.5 erfc(|f| / sqrt 2), so that the tails
 * keep their relative accuracy).  A latent that the point's branch does not read has gm = gv = 0 and its s2 is not examined; one that it reads
 * with s2 <= 0 or NaN makes the three outputs of the point's segment NaN.  Stages that are not read are not evaluated.
 * Pass 1 is one wavefront per tile of 64 points (LDS: 64 rows of L 2d + 1 elements, the pair marginal, 2 L + 1 rows of 64 values:
 * 34480 B at 2d = 18 in float64); the workspace row and pass 2 are those of mf_lik_sparse_expectations_*, and so is the size:
 * mf_lik_sparse_multi_expectations_workspace_bytes(num_tiles, two_d, sizeof(T)).  g_mean and g_cov BOTH NULL: the value only (the
 * same bits).  No floating-point atomics: the same bits on every launch and for a series alone or inside a batch.  The tile table
 * is clamped on the device, not validated.  No allocation, no synchronisation.
 * Returns 0, -(position of the offending argument in THIS signature: 1 B, 2 N, 3 S, 8 nq, 9 nodes, 10 weights, 11 ... 16 a NULL
 * input, 17 num_tiles negative, above 2^31 - 1 or non-zero for N = 0, 18 / 19 a NULL table, 20 a NULL workspace, 21 a workspace
 * that is too small, 23 / 24 one of g_mean / g_cov NULL without the other), -101 for a (two_d, latent_dim, lik) that is not
 * instantiated - two_d in 6, 8, ..., 18 with latent_dim = 3 and lik = 4 are - or -1000 (launch failed).  Nothing is launched on an
 * error, for B = 0, or when every output is NULL.
 */
size_t mf_lik_sparse_multi_expectations_workspace_bytes(int64_t num_tiles, int two_d, int elem_size);
int mf_lik_sparse_multi_expectations_f64(int64_t B, int64_t N, int64_t S, int two_d, int latent_dim, int lik, const double* params,
                                         int nq, const double* nodes, const double* weights, const int64_t* seg_offsets,
                                         const double* w, const double* c, const double* y, const double* pair_mean,
                                         const double* pair_cov, int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile,
                                         void* workspace, size_t workspace_bytes, double* ve_sum, double* g_mean, double* g_cov,
                                         void* stream);
int mf_lik_sparse_multi_expectations_f32(int64_t B, int64_t N, int64_t S, int two_d, int latent_dim, int lik, const double* params,
                                         int nq, const double* nodes, const double* weights, const int64_t* seg_offsets,
                                         const float* w, const float* c, const float* y, const float* pair_mean,
                                         const float* pair_cov, int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile,
                                         void* workspace, size_t workspace_bytes, float* ve_sum, float* g_mean, float* g_cov,
                                         void* stream);

/*
 * The multi-stage likelihood's variational expectations, element-wise (csrc/mf_lik.hip): a lane per point, fmu, fvar, g_mu and
 * g_var [N, 3], y and ve [N]; the formulas and the domain rule are those of mf_lik_sparse_multi_expectations_* (a point whose
 * branch reads a latent with fvar <= 0 or NaN gets NaN in ve and in that latent's two derivatives).  Any output may be NULL.
 * Returns 0, -(position: 1 N, 2 nq, 3 nodes, 4 weights, 5 ... 7 a NULL input) or -1000 (launch failed).
 */
int mf_lik_multistage_variational_expectations_f64(int64_t N, int nq, const double* nodes, const double* weights, const double* fmu,
                                                   const double* fvar, const double* y, double* ve, double* g_mu, double* g_var,
                                                   void* stream);
int mf_lik_multistage_variational_expectations_f32(int64_t N, int nq, const double* nodes, const double* weights, const float* fmu,
                                                   const float* fvar, const float* y, float* ve, float* g_mu, float* g_var,
                                                   void* stream);

/*
 * The data term of the SVGP ELBO under a FactorAnalysis emission, its adjoint onto the pair marginals and its adjoint onto the
 * mixing weights (markovflow/kernels/sde_kernel.py:881-941 under markovflow/models/sparse_variational.py:149-192;
 * csrc/mf_lik_factor.hip): P = num_outputs observed series, each with the scalar likelihood lik, mixed from L = latent_dim latent
 * processes, f_k = W_k g_k.  B, N, S, two_d, lik, params, the rule, seg_offsets, pair_mean, pair_cov, the tile table, the workspace and
 * the first three outputs as for mf_lik_sparse_expectations_*; every point carries
 *   wg  [B, N, L, 2d]  row l: H_inner,l P_k                 cg [B, N, L, L]  H_inner T_k H_inner^T (symmetric: the lower triangle is read)
 *   mix [B, N, P, L]   W_k = A(t_k) B                       y  [B, N, P]
 * Per point k of segment s:  mu_g = wg m_s,  Sig_g = cg + wg S_s wg^T;  per output p, ascending:  mu_p = W_p . mu_g,
 * s2_p = W_p Sig_g W_p^T,  (ve_p, gm_p, gv_p) of the likelihood at (mu_p, s2_p, y_kp);  a = W^T gm,  G = W^T diag(gv) W;  per segment,
 * over the points in ascending order and within a point over the pairs (l, l' <= l) in the order (0,0), (1,0), (1,1), (2,0), ...,
 * then over the latents in ascending order,
 *   ve_sum = sum_k sum_p ve_p      g_mean = sum_k wg^T a      g_cov = sum_k wg^T G wg
 * and per point, not summed (rows of points outside every segment are not written),
 *   g_w [B, N, P, L] = gm (x) mu_g + 2 diag(gv) W Sig_g       (may be NULL on its own)
 * An output with s2_p <= 0 or NaN makes the three outputs of its segment NaN, and row p of that point's g_w.
 * Pass 1 is one wavefront per tile of 64 points; the outputs are walked in chunks of 4 through LDS, whose footprint does not depend
 * on P (64 rows of L 2d + 1 elements, the pair marginal, 64 rows of 4 (L + 1) + 1, L (L + 1) / 2 + L + 1 rows of 64 values: 58544 B at
 * L = 4, 2d = 18 in float64).  The workspace row and pass 2 are those of mf_lik_sparse_expectations_*, and so is the size:
 * mf_lik_sparse_factor_expectations_workspace_bytes(num_tiles, two_d, sizeof(T)).  g_mean and g_cov BOTH NULL: the value (and g_w when
 * given) only, the same bits.  No floating-point atomics: the same bits on every launch and for a series alone or inside a batch.  The
 * tile table is clamped on the device, not validated.  No allocation, no synchronisation.
 * Returns 0, -(position of the offending argument in THIS signature: 1 B, 2 N, 3 S, 6 num_outputs < 1, 7 lik, 8 params, 9 nq, 10 nodes,
 * 11 weights, 12 ... 18 a NULL input, 19 num_tiles negative, above 2^31 - 1 or non-zero for N = 0, 20 / 21 a NULL table, 22 a NULL
 * workspace, 23 a workspace that is too small, 25 / 26 one of g_mean / g_cov NULL without the other), -101 for a signature that is
 * not instantiated - latent_dim in 2, 3, 4 with two_d even in 2 latent_dim ... 18 and num_outputs <= 1024 are - or -1000 (launch
 * failed).  Nothing is launched on an error, for B = 0, or when every output is NULL.
 */
size_t mf_lik_sparse_factor_expectations_workspace_bytes(int64_t num_tiles, int two_d, int elem_size);
int mf_lik_sparse_factor_expectations_f64(int64_t B, int64_t N, int64_t S, int two_d, int latent_dim, int64_t num_outputs, int lik,
                                          const double* params, int nq, const double* nodes, const double* weights,
                                          const int64_t* seg_offsets, const double* wg, const double* cg, const double* mix,
                                          const double* y, const double* pair_mean, const double* pair_cov, int64_t num_tiles,
                                          const int64_t* tile_seg, const int64_t* seg_tile, void* workspace, size_t workspace_bytes,
                                          double* ve_sum, double* g_mean, double* g_cov, double* g_w, void* stream);
int mf_lik_sparse_factor_expectations_f32(int64_t B, int64_t N, int64_t S, int two_d, int latent_dim, int64_t num_outputs, int lik,
                                          const double* params, int nq, const double* nodes, const double* weights,
                                          const int64_t* seg_offsets, const float* wg, const float* cg, const float* mix,
                                          const float* y, const float* pair_mean, const float* pair_cov, int64_t num_tiles,
                                          const int64_t* tile_seg, const int64_t* seg_tile, void* workspace, size_t workspace_bytes,
                                          float* ve_sum, float* g_mean, float* g_cov, float* g_w, void* stream);

/*
 * The data term of the SVGP ELBO for a likelihood with K = latent_dim latent functions per observation on K STACKED chains, and its
 * adjoints onto every chain's pair marginals (markovflow/kernels/sde_kernel.py:945-1279 and markovflow/emission_model.py:270-378
 * under markovflow/models/sparse_variational.py:149-192; csrc/mf_lik_stack.hip).  Every latent has a chain of its own - K is the last
 * batch dimension of the chains - and the K chains of a series share ONE segmentation: B series, N points, S = M + 1 segments,
 * two_d = 2 d (d the padded state dimension), the rule, seg_offsets [B, S + 1] and the tile table over the B S segments as for
 * mf_lik_sparse_expectations_*.  The data arrays are in the stacked layout, no transposes:
 *   w [B, K, N, 2d]  row n of chain k: H_k P_kn        c [B, K, N]  H_k T_kn H_k^T        y [B, N]
 *   pair_mean [B, K, S, 2d]        pair_cov [B, K, S, 2d, 2d]
 * Per point n of segment s and latent k, ascending:  mu_k = w_kn . m_ks,  s2_k = c_kn + w_kn^T S_ks w_kn;  (ve, gm_k, gv_k) of the
 * likelihood at (mu, s2, y_n);  per segment, over the points in ascending order,
 *   ve_sum [B, S] = sum ve      g_mean [B, K, S, 2d] = sum gm_k w_kn      g_cov [B, K, S, 2d, 2d] = sum gv_k w_kn w_kn^T
 * (g_cov symmetric, both triangles written from one sum).  lik = 4, latent_dim = 3 is the multi-stage likelihood of
 * mf_lik_sparse_multi_expectations_* (the same evaluation); lik = 5, latent_dim = 2 is the heteroscedastic Gaussian
 * y ~ N(F0, exp F1) in closed form: with e = exp(-mu_1 + s2_1 / 2) and E = e ((mu_0 - y)^2 + s2_0), ve = -(log 2 pi + mu_1 + E) / 2,
 * gm_0 = -e (mu_0 - y), gv_0 = -e / 2, gm_1 = -(1 - E) / 2, gv_1 = -E / 4 (the rule is checked, not used).  Neither has parameters:
 * params is not read.  A latent that the point's branch does not read has gm = gv = 0 and its s2 is not examined; one that it reads
 * with s2 <= 0 or NaN makes ve_sum [b, s], g_mean [b, :, s] and g_cov [b, :, s] NaN - all K chains of that segment, no other
 * segment.  The heteroscedastic Gaussian reads both latents at every point.  The zero columns of w in the padded state dimensions
 * of a chain shorter than d are multiplied through.
 * Pass 1 is one wavefront per tile of 64 points (LDS: 64 rows of K 2d + 1 elements, the K pair marginals, 2 K + 1 rows of 64 values:
 * 39952 B at K = 3, 2d = 18 in float64); a workspace row is K (2d (2d + 1) / 2 + 2d) + 1 values - per latent the lower triangle of
 * g_cov and g_mean, then sum ve - and pass 2 adds a segment's rows in ascending tile order.  The workspace holds
 * mf_lik_stack_expectations_workspace_bytes(num_tiles, two_d, latent_dim, sizeof(T)) bytes (0 for an argument out of range).
 * g_mean and g_cov BOTH NULL: the value only (the same bits); ve_sum NULL: the adjoints only (the same bits).  Empty segments and
 * N = 0 give exact zeros.  No floating-point atomics: the same bits on every launch and for a series alone or inside a batch.
 * The tile table is clamped on the device, not validated.  No allocation, no synchronisation.
 * Returns 0, -(position of the offending argument in THIS signature: 1 B, 3 N, 4 S, 8 nq, 9 nodes, 10 weights, 11 ... 16 a NULL
 * input, 17 num_tiles negative, above 2^31 - 1 or non-zero for N = 0, 18 / 19 a NULL table, 20 a NULL workspace, 21 a workspace
 * that is too small, 23 / 24 one of g_mean / g_cov NULL without the other), -101 for a (two_d, latent_dim, lik) that is not
 * instantiated - two_d in 2, 4, ..., 18 with (latent_dim, lik) = (3, 4) or (2, 5) are - or -1000 (launch failed).  Nothing is
 * launched and nothing written on an error, for B = 0, or when every output is NULL.
 */
size_t mf_lik_stack_expectations_workspace_bytes(int64_t num_tiles, int two_d, int latent_dim, int elem_size);
int mf_lik_stack_expectations_f64(int64_t B, int latent_dim, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq,
                                  const double* nodes, const double* weights, const int64_t* seg_offsets, const double* w,
                                  const double* c, const double* y, const double* pair_mean, const double* pair_cov,
                                  int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* workspace,
                                  size_t workspace_bytes, double* ve_sum, double* g_mean, double* g_cov, void* stream);
int mf_lik_stack_expectations_f32(int64_t B, int latent_dim, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq,
                                  const double* nodes, const double* weights, const int64_t* seg_offsets, const float* w,
                                  const float* c, const float* y, const float* pair_mean, const float* pair_cov,
                                  int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* workspace,
                                  size_t workspace_bytes, float* ve_sum, float* g_mean, float* g_cov, void* stream);

/*
 * The segmented site update of the sparse power-EP model (markovflow/models/sparse_pep.py:316-487; csrc/mf_lik.hip): B, N, S,
 * two_d, the likelihood, the rule, seg_offsets, w, c, y, the tile table and the workspace as for mf_lik_sparse_expectations_*;
 * alpha in (0, 1] is the power, lr in [0, 1] the damping.  The workspace row has the width of that entry point's, so its size is
 * mf_lik_sparse_expectations_workspace_bytes(num_tiles, two_d, sizeof(T)): there is no second size function.
 *   cav_mean [B, S, 2d], cav_cov [B, S, 2d, 2d]   the CAVITY of q on every pair (in place of pair_mean / pair_cov); NaN where it
 *                                                 does not exist
 *   seg_const [B, S]        added to the segment's summed log expected density before the blend; NULL: 0
 *   nat1 [B, S, 2d], nat2 [B, S, 2d, 2d], log_norm [B, S]   the sites, updated IN PLACE; ALL THREE NULL: evaluation only
 *   led_sum [B, S]          sum_k I_k of every segment (NaN for an undefined one); may be NULL
 *   fmu, fvar, led [B, N]   per point, any of them may be NULL
 * Pass 1, one wavefront per tile, per point k of segment s:  fmu = w_k . m_c,  fvar = c_k + w_k^T S_c w_k,  (I, g1, g2) as
 * mf_lik_log_expected_density at (fmu, fvar),  den = 1 + fvar g2 (Gaussian: (var / alpha) / (var / alpha + fvar), the same number
 * without the cancellation),  L2 = g2 / (2 den),  L1 = (g1 - fmu g2) / den.  A point is UNDEFINED when fvar or den is not > 0 or
 * one of L2, L1, I is not finite; it contributes NaN.  fmu and fvar are NaN where fvar is not > 0; led is I wherever fvar > 0.
 * The tile's sums  sum_k L2 w_k w_k^T (lower triangle),  sum_k L1 w_k,  sum_k I  are one row of the workspace.
 * Pass 2, one block per (series, segment), adds the rows in ascending tile order and, if every entry - the scalar one with
 * seg_const added - is finite, stores  pep = (1 - alpha) old + sum (+ seg_const),  new = (1 - lr) old + lr pep  into nat2 (both
 * triangles), nat1 and log_norm.  Otherwise the three site tensors of THIS segment are left as they are, bit for bit; no other
 * segment is touched.  An empty segment has sum 0: it decays by 1 - lr alpha.  led_sum gets the raw sum, without seg_const.
 * No floating-point atomics, the same bits on every launch, for a series alone or inside a batch, and in evaluation-only mode
 * beside the update; the tile table is clamped on the device, not validated.  No allocation, no synchronisation.
 * Returns 0, -(position of the offending argument in THIS signature: 1 B, 2 N, 3 S, 5 lik, 6 params, 7 nq, 8 nodes, 9 weights,
 * 10 alpha, 11 lr, 12 ... 17 a NULL input, 19 num_tiles negative, above 2^31 - 1 or non-zero for N = 0, 20 / 21 a NULL table, 22 a
 * NULL workspace, 23 a workspace that is too small, 24 / 25 / 26 the first of nat1 / nat2 / log_norm that is NULL beside a given
 * one), -100 for a two_d that is odd, < 2 or > 18, or -1000 (launch failed).  Nothing is launched on an error, for B = 0, or when
 * every output is NULL.
 */
int mf_lik_sparse_pep_site_update_f64(int64_t B, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq,
                                      const double* nodes, const double* weights, double alpha, double lr,
                                      const int64_t* seg_offsets, const double* w, const double* c, const double* y,
                                      const double* cav_mean, const double* cav_cov, const double* seg_const, int64_t num_tiles,
                                      const int64_t* tile_seg, const int64_t* seg_tile, void* workspace, size_t workspace_bytes,
                                      double* nat1, double* nat2, double* log_norm, double* led_sum, double* fmu, double* fvar,
                                      double* led, void* stream);
int mf_lik_sparse_pep_site_update_f32(int64_t B, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq,
                                      const double* nodes, const double* weights, float alpha, float lr,
                                      const int64_t* seg_offsets, const float* w, const float* c, const float* y,
                                      const float* cav_mean, const float* cav_cov, const float* seg_const, int64_t num_tiles,
                                      const int64_t* tile_seg, const int64_t* seg_tile, void* workspace, size_t workspace_bytes,
                                      float* nat1, float* nat2, float* log_norm, float* led_sum, float* fmu, float* fvar,
                                      float* led, void* stream);

/*
 * The data term of the log importance weights of importance-weighted VI and its adjoint onto the posterior draw at the inducing
 * points (markovflow/models/iwvi.py:109-173, markovflow/posterior.py:522-580; csrc/mf_lik.hip): K Monte-Carlo evaluations of
 * log p(y_n | f_n) at every data point.  B, N, S = M + 1, two_d = 2 d, the likelihood, seg_offsets, w = H [D E], y, the tile table
 * as for mf_lik_sparse_expectations_*; no quadrature rule - the density is evaluated point-wise; h [d] is the emission row.
 * u_post given ([K, B, M, d], the draw from q at the inducing points):
 *   states [K, B, N + M, d] is ONE prior draw on the merged, sorted time points: data point n of segment s sits at row n + s,
 *   inducing point m at row seg_offsets[b, m + 1] + m (points with x <= z_m precede z_m); per sample k, series b, point n of
 *   segment s, in this order of evaluation
 *     dL_i = s > 0 ? states[k, b, row(z_{s-1}), i] - u_post[k, b, s - 1, i] : 0
 *     dR_i = s < M ? states[k, b, row(z_s), i]     - u_post[k, b, s, i]     : 0
 *     f    = (sum_i h_i states[k, b, n + s, i] - sum_i w[b, n, i] dL_i) - sum_i w[b, n, d + i] dR_i
 *     l, l' = log p(y_n | f) and its derivative in f   (Poisson: with - lgamma(y + 1), computed once per point)
 *     log_lik [K, B, S]      sum over the points of segment s of l
 *     g_u     [K, B, M, d]   sum_{n in segment m} l'_n w[b, n, d + i] + sum_{n in segment m + 1} l'_n w[b, n, i]: the adjoint of
 *                            sum_s log_lik[k, b, s] with respect to u_post[k, b, m, i]
 * u_post NULL: states [K, B, N, d] holds final samples, point n at row n, f = sum_i h_i states[k, b, n, i]; w is not read and may
 * be NULL; g_u must be NULL.  Either output may be NULL; what is computed has the bits of the full call.
 * Two passes.  Pass 1 runs one wavefront per (tile, chunk of 8 samples), a lane per point: w, y and the Poisson constant are read
 * once and kept for the samples of the chunk, the prior draw is read exactly once, and the 2d + 1 partial sums of every
 * (tile, sample) - over the tile's points in ascending order - go to the workspace,
 * mf_lik_iw_log_weights_workspace_bytes(num_tiles, K, two_d, sizeof(T)) = num_tiles K (two_d + 1) sizeof(T) bytes (0 outside the
 * supported two_d, for num_tiles = 0 or K = 0).  Pass 2 adds per (k, b, s) that segment's tiles in ascending order into log_lik, and
 * per (k, b, m) the tiles of segment m, then those of segment m + 1, into g_u.  No atomics: the same bits on every launch, for a
 * series alone or inside a batch, for a sample alone or among K.  A non-finite f makes log_lik of ITS (k, b, s) and the g_u rows
 * that segment feeds non-finite; nothing else is touched.  An empty segment, and every segment for N = 0, gets zeros (N = 0
 * needs no input, table or workspace).  The offsets and the tile table are clamped on the device, not validated.  No allocation,
 * no synchronisation.
 * Returns 0, -(position of the offending argument in THIS signature: 1 B, 2 N, 3 S, 5 K negative or above 2^31 - 1, 6 lik,
 * 7 params, 8 seg_offsets NULL, 9 w NULL beside u_post, 10 / 11 / 12 y / h / states NULL, 14 num_tiles negative, above 2^31 - 1,
 * non-zero for N = 0 or with more than 2^31 - 1 blocks, 15 / 16 a NULL table, 17 a NULL workspace, 18 a workspace that is too
 * small, 20 g_u without u_post), -100 for a two_d that is odd, < 2 or > 18, or -1000 (launch failed).  Nothing is launched on an
 * error, for B = 0 or K = 0, or when both outputs are NULL.
 */
size_t mf_lik_iw_log_weights_workspace_bytes(int64_t num_tiles, int64_t K, int two_d, int elem_size);
int mf_lik_iw_log_weights_f64(int64_t B, int64_t N, int64_t S, int two_d, int64_t K, int lik, const double* params,
                              const int64_t* seg_offsets, const double* w, const double* y, const double* h, const double* states,
                              const double* u_post, int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile,
                              void* workspace, size_t workspace_bytes, double* log_lik, double* g_u, void* stream);
int mf_lik_iw_log_weights_f32(int64_t B, int64_t N, int64_t S, int two_d, int64_t K, int lik, const double* params,
                              const int64_t* seg_offsets, const float* w, const float* y, const float* h, const float* states,
                              const float* u_post, int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile,
                              void* workspace, size_t workspace_bytes, float* log_lik, float* g_u, void* stream);

/*
 * The data term of the VGP ELBO (markovflow/models/variational.py:129-152; csrc/mf_lik.hip), dense: q lives on the states at the data
 * points themselves, so point k of series b has its own emission row h [B, N, d], marginal mean means [B, N, d] and marginal
 * covariance covs [B, N, d, d].  1 <= d <= 12; the likelihood and the rule as for mf_lik_variational_expectations; y [B, N].
 * Per point:  fmu = h_k . m_k,  fvar = sum_i h_i (sum_j P_ij h_j) - the FULL matrix is read, both triangles, so the adjoint for an
 * unconstrained P is g_var h h^T -,  (ve, gm, gv) as mf_lik_variational_expectations;
 *   ve_sum [B]      sum_k ve_k
 *   g_mu   [B, N]   gm_k = d ve_k / d fmu_k          the compact form of the adjoint: 2 values per point, not d^2 + d;
 *   g_var  [B, N]   gv_k = d ve_k / d fvar_k         mf_lik_dense_expectations_adjoint_* expands them
 * g_mu and g_var BOTH NULL: the value only (the same bits); ve_sum may be NULL beside the gradients (no workspace is needed then).
 * THE ORDER OF THE SUMS, part of the contract: every sum starts from 0 and grows term by term, index ascending -
 *   t_i = sum_j P_ij h_j in j,  fvar = sum_i h_i t_i and fmu = sum_i h_i m_i in i,
 *   a TILE - points 64 t ... 64 t + 63 of a series - in its points (pass 1: one wavefront per tile, one partial per tile in the
 *   workspace), a series in its tiles (pass 2).  These two sums run in a double accumulator in float32 as well and are rounded once
 *   each, into the partial and into ve_sum.
 * No floating-point atomics: the same bits on every launch and for a series alone or inside a batch.  The workspace holds
 * mf_lik_dense_expectations_workspace_bytes(B, N, sizeof(T)) = B ceil(N / 64) sizeof(T) bytes (0 when B or N is 0).  A point with
 * fvar <= 0 or NaN makes ITS series' ve_sum and its own g_mu, g_var NaN; no other series or point changes.  N = 0 gives zeros.
 * No allocation, no synchronisation.
 * Returns 0, -(position of the offending argument in THIS signature: 1 B, 2 N (negative, or more than 2^31 - 1 tiles), 4 lik,
 * 5 params, 6 nq, 7 nodes, 8 weights, 9 ... 12 a NULL input, 13 a NULL workspace, 14 a workspace that is too small, 16 / 17 one of
 * g_mu / g_var NULL without the other), -100 for a d outside 1 ... 12, or -1000 (launch failed).  Nothing is launched on an error,
 * for B = 0, or when every output is NULL.
 */
size_t mf_lik_dense_expectations_workspace_bytes(int64_t B, int64_t N, int elem_size);
int mf_lik_dense_expectations_f64(int64_t B, int64_t N, int d, int lik, const double* params, int nq, const double* nodes,
                                  const double* weights, const double* h, const double* means, const double* covs, const double* y,
                                  void* workspace, size_t workspace_bytes, double* ve_sum, double* g_mu, double* g_var,
                                  void* stream);
int mf_lik_dense_expectations_f32(int64_t B, int64_t N, int d, int lik, const double* params, int nq, const double* nodes,
                                  const double* weights, const float* h, const float* means, const float* covs, const float* y,
                                  void* workspace, size_t workspace_bytes, float* ve_sum, float* g_mu, float* g_var, void* stream);

/*
 * The expansion of that adjoint onto the marginals, what mf_ssm_marginals_grad_* takes as g_means / g_covs (csrc/mf_lik.hip):
 *   g_means [B, N, d]      (weight_b g_mu[b, k]) h[b, k, i]
 *   g_covs  [B, N, d, d]   (weight_b (g_var[b, k] h[b, k, i])) h[b, k, j]
 * weight [B] is the incoming gradient of ve_sum; NULL means 1, with the bits a vector of ones gives.  One launch, store-bound:
 * consecutive lanes write consecutive elements.  Either output may be NULL.  1 <= d <= 12.
 * Returns 0, -(position: 1 B, 2 N, 4 h, 5 g_mu NULL beside g_means, 6 g_var NULL beside g_covs), -100 for a d outside 1 ... 12, or
 * -1000 (launch failed).  Nothing is launched on an error, for B = 0 or N = 0, or when both outputs are NULL.
 */
int mf_lik_dense_expectations_adjoint_f64(int64_t B, int64_t N, int d, const double* h, const double* g_mu, const double* g_var,
                                          const double* weight, double* g_means, double* g_covs, void* stream);
int mf_lik_dense_expectations_adjoint_f32(int64_t B, int64_t N, int d, const float* h, const float* g_mu, const float* g_var,
                                          const float* weight, float* g_means, float* g_covs, void* stream);

/*
 * The data term of the spatio-temporal sparse variational ELBO and its adjoints (markovflow/models/spatio_temporal_variational.py
 * :149-236; csrc/mf_st.hip).  The chain state is Ms copies of a temporal state of dimension d_t = two_dt / 2 (copy s in columns
 * s d_t ... (s + 1) d_t - 1), D = Ms d_t <= 64, and a pair of neighbouring inducing states has dimension n = 2 D <= 128.  B, N, S,
 * the likelihood, the rule, seg_offsets, c, y, pair_mean [B, S, n] and pair_cov [B, S, n, n] as for mf_lik_sparse_expectations_*;
 *   a  [B, N, Ms]      the spatial weights of every point, L^-1 K_s(Z_s, x_k)
 *   wt [B, N, two_dt]  the temporal projection of the pair onto the point, h P_k
 * The projection of the pair onto f_k is  W_k[half D + s d_t + i] = a_k[s] wt_k[half d_t + i]  (half in {0, 1}); it is never
 * written to memory.  pair_cov is read in full and symmetrised, Sbar = (S + S^T) / 2.  Per point k of segment s, with V_k = Sbar W_k:
 *   fmu = W_k . m_s,  fvar = c_k + W_k . V_k,  (ve, gm, gv) as mf_lik_variational_expectations
 * Outputs, each group optional, every combination with the same bits:
 *   ve_sum [B, S]                          sum_k ve_k
 *   g_mean [B, S, n], g_cov [B, S, n, n]   sum_k gm_k W_k,  sum_k gv_k W_k W_k^T (symmetric, both triangles written); both or neither
 *   g_a [B, N, Ms], g_wt [B, N, two_dt], g_c [B, N]     the adjoints of ve_k onto the point's own a, wt and c; all three or none:
 *                                          g_a[k, s]              = gm_k Ma[s] + 2 gv_k Va[s]
 *                                          g_wt[k, half d_t + i]  = gm_k Mwt[half d_t + i] + 2 gv_k Vwt[half d_t + i]
 *                                          g_c[k]                 = gv_k
 *                                          Xa[s] = sum_{half, i} X[half D + s d_t + i] wt_k[half d_t + i],
 *                                          Xwt[half d_t + i] = sum_s X[half D + s d_t + i] a_k[s]   for X = m_s (M) and X = V_k (V)
 *   fmu, fvar [B, N]                       the projection; with nothing else asked for y may be NULL
 * Two passes.  Pass 1 runs one workgroup per ROW - at most 256 consecutive points of one segment, row j of a segment starting at
 * the segment's first point + 256 j - and leaves the row's n (n + 1) / 2 + n + 1 partial sums in the workspace; pass 2 adds a
 * segment's rows in ascending order.  The caller supplies the row table in the form of the siblings' tile table, with 256 points per
 * tile: num_tiles = sum over the segments of ceil(length / 256), tile_seg [num_tiles], seg_tile [B S + 1]; and the workspace,
 * mf_lik_st_expectations_workspace_bytes(num_tiles, Ms, two_dt, sizeof(T)) = num_tiles (n (n + 1) / 2 + n + 1) sizeof(T) bytes
 * (0 outside the supported range or for num_tiles = 0; needed only beside ve_sum or g_mean).  The table is clamped on the device.
 * THE ORDER OF THE SUMS, part of the contract: every sum starts from 0 and grows by ONE fused multiply-add per term (the sums of
 * ve_k and of the rows: one addition), index ascending -
 *   V_k[i] in j;  fmu, W_k . V_k (then c_k is added), Ma, Va, Mwt, Vwt in the pair index j of their terms;
 *   g_a = fma(2 gv, Va, gm Ma), g_wt likewise;  a row's sums in its points, with (gv_k W_k[i]) W_k[j] for i >= j;  a segment's in
 *   its rows.
 * No floating-point atomics: the same bits on every launch and for a series alone or inside a batch.  A point with fvar <= 0 or
 * NaN gets NaN in its own fmu, fvar, g_a, g_wt, g_c and makes the three segment outputs of ITS segment NaN; nothing else changes.
 * An empty segment, and every segment for N = 0, gets zeros.  No allocation, no synchronisation.
 * Returns 0, -(position of the offending argument in THIS signature: 1 B, 2 N, 3 S, 6 lik, 7 params, 8 nq, 9 nodes, 10 weights,
 * 11 ... 14 a NULL input, 15 y NULL beside an output that needs the likelihood, 16 / 17 a NULL marginal, 18 num_tiles negative,
 * above 2^31 - 1 or non-zero for N = 0, 19 / 20 a NULL table, 21 a NULL workspace, 22 a workspace that is too small, 24 / 25 one of
 * g_mean / g_cov NULL without the other, 26 / 27 / 28 the first of g_a / g_wt / g_c that is NULL beside a given one), -100 for
 * Ms < 1, a two_dt that is odd or < 2, or Ms two_dt / 2 > 64, or -1000 (launch failed).  Nothing is launched on an error, for
 * B = 0, or when every output is NULL.
 */
size_t mf_lik_st_expectations_workspace_bytes(int64_t num_tiles, int Ms, int two_dt, int elem_size);
int mf_lik_st_expectations_f64(int64_t B, int64_t N, int64_t S, int Ms, int two_dt, int lik, const double* params, int nq,
                               const double* nodes, const double* weights, const int64_t* seg_offsets, const double* a,
                               const double* wt, const double* c, const double* y, const double* pair_mean, const double* pair_cov,
                               int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* workspace,
                               size_t workspace_bytes, double* ve_sum, double* g_mean, double* g_cov, double* g_a, double* g_wt,
                               double* g_c, double* fmu, double* fvar, void* stream);
int mf_lik_st_expectations_f32(int64_t B, int64_t N, int64_t S, int Ms, int two_dt, int lik, const double* params, int nq,
                               const double* nodes, const double* weights, const int64_t* seg_offsets, const float* a,
                               const float* wt, const float* c, const float* y, const float* pair_mean, const float* pair_cov,
                               int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* workspace,
                               size_t workspace_bytes, float* ve_sum, float* g_mean, float* g_cov, float* g_a, float* g_wt,
                               float* g_c, float* fmu, float* fvar, void* stream);

/*
 * One conjugate-computation VI step on the sites of the spatio-temporal sparse model, in place (markovflow/models/
 * spatio_temporal_variational.py:509-552; csrc/mf_st.hip).  Every input, the row table and the workspace as for
 * mf_lik_st_expectations_* (mf_lik_st_cvi_site_update_workspace_bytes returns the same number); the range is the same,
 * Ms >= 1, d_t >= 1, Ms d_t <= 64.  Per point k of segment s, with fmu, fvar and (ve, gm, gv) as there,
 *   g1_k = fma(-2 gv_k, fmu_k, gm_k)        the gradient of ve_k in the first expectation parameter; gv_k is the one in the second
 * and per segment
 *   theta1 = sum_k g1_k W_k,   theta2 = sum_k gv_k W_k W_k^T
 *   nat1 [B, S, n]     <-  fma(lr, theta1[j],      (1 - lr) nat1[j])
 *   nat2 [B, S, n, n]  <-  fma(lr, theta2[i][j],   (1 - lr) nat2[i][j])
 * with 1 - lr formed once in T.  theta2 is summed over its lower triangle only and both (i, j) and (j, i) take the entry
 * (max(i, j), min(i, j)), each blended with its own old value: a symmetric nat2 stays symmetric bit for bit.  nat1 and nat2 are
 * both required (mf_lik_st_expectations_* serves projection-only calls).  Optional outputs, every combination with the same bits in
 * nat1 and nat2:  ve_sum [B, S] = sum_k ve_k,  fmu, fvar [B, N].
 * Two passes: pass 1 is that of mf_lik_st_expectations_* with g1_k in place of gm_k in the vector sum, pass 2 adds a segment's rows
 * and blends.  THE ORDER OF THE SUMS, part of the contract: that of mf_lik_st_expectations_* -
 *   V_k[i] in j;  fmu and W_k . V_k (then c_k is added) in the pair index j;  a row's sums of ve_k, g1_k W_k[j] and
 *   (gv_k W_k[i]) W_k[j], i >= j, in its points, one fused multiply-add per term from 0;  a segment's in its rows, ascending from
 *   0, one addition per row;  then the blend above.
 * From zero sites at lr = 1, nat2 has the bits of g_cov, and ve_sum, fmu and fvar the bits they have there.  No floating-point
 * atomics.  A point with fvar <= 0 or NaN gets NaN in its own fmu and fvar and makes nat1, nat2 and ve_sum of ITS segment NaN; no
 * other segment changes.  An empty segment, and every segment for N = 0, has sums of exactly 0: its sites become (1 - lr) nat.
 * No allocation, no synchronisation.
 * Returns 0, -(position of the offending argument in THIS signature: 1 B, 2 N, 3 S, 6 lik, 7 params, 8 nq, 9 nodes, 10 weights,
 * 11 ... 17 a NULL input, 18 num_tiles negative, above 2^31 - 1 or non-zero for N = 0, 19 / 20 a NULL table, 21 a NULL workspace,
 * 22 a workspace that is too small, 23 a learning_rate outside [0, 1] or NaN, 24 / 25 a NULL nat1 / nat2), -100 for Ms < 1, a
 * two_dt that is odd or < 2, or Ms two_dt / 2 > 64, or -1000 (launch failed).  Nothing is launched on an error or for B = 0.
 */
size_t mf_lik_st_cvi_site_update_workspace_bytes(int64_t num_tiles, int Ms, int two_dt, int elem_size);
int mf_lik_st_cvi_site_update_f64(int64_t B, int64_t N, int64_t S, int Ms, int two_dt, int lik, const double* params, int nq,
                                  const double* nodes, const double* weights, const int64_t* seg_offsets, const double* a,
                                  const double* wt, const double* c, const double* y, const double* pair_mean,
                                  const double* pair_cov, int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile,
                                  void* workspace, size_t workspace_bytes, double learning_rate, double* nat1, double* nat2,
                                  double* ve_sum, double* fmu, double* fvar, void* stream);
int mf_lik_st_cvi_site_update_f32(int64_t B, int64_t N, int64_t S, int Ms, int two_dt, int lik, const double* params, int nq,
                                  const double* nodes, const double* weights, const int64_t* seg_offsets, const float* a,
                                  const float* wt, const float* c, const float* y, const float* pair_mean, const float* pair_cov,
                                  int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* workspace,
                                  size_t workspace_bytes, float learning_rate, float* nat1, float* nat2, float* ve_sum, float* fmu,
                                  float* fvar, void* stream);

/*
 * Non-linear SDEs  dx = f(x) dt + L dB  (markovflow/sde/sde.py, sde_utils.py; csrc/mf_nlsde.hip).  `drift`: 0 Ornstein-Uhlenbeck,
 * f(x) = -lambda x, params [lambda]; 1 double well, f(x) = 4 x (1 - x^2), no params (params may be NULL).  Both act element-wise
 * on the state.  `params`, `chol_l` of the simulation, `nodes` and `weights` are HOST arrays of doubles in both precisions.
 *
 * Euler-Maruyama: B paths of dimension 1 <= d <= 4 on a strictly increasing time_grid [T] whose first entry is the start time;
 * x0 [B, d], noise [B, T - 1, d] standard normal draws, chol_l the d (d + 1) / 2 entries of the lower triangle of L row by row;
 *   out [B, T, d]:  out[:, 0] = x0 (the same bits),  out[:, k + 1] = out[:, k] + f(out[:, k]) dt_k + sqrt(dt_k) L noise[:, k],
 * dt_k = time_grid[k + 1] - time_grid[k].  One launch for all T - 1 steps; no atomics, no workspace.  T = 1 writes x0 only.
 * Returns 0, -(position of the offending argument: 1 B, 2 T < 1, 3 d < 1, 4 drift, 5 params, 6 ... 10 a NULL array), -100 for
 * d > 4, or -1000 (launch failed); B = 0 returns 0 without a launch.
 */
int mf_nlsde_euler_maruyama_f64(int64_t B, int64_t T, int d, int drift, const double* params, const double* chol_l, const double* x0,
                                const double* time_grid, const double* noise, double* out, void* stream);
int mf_nlsde_euler_maruyama_f32(int64_t B, int64_t T, int d, int drift, const double* params, const double* chol_l, const float* x0,
                                const float* time_grid, const float* noise, float* out, void* stream);
/*
 * Linearisation along a Gaussian path, state dimension 1 (sde_utils.py:107-158): times [N + 1], mean and var [B, N] the marginals
 * N(m_k, S_k) of the path, chol_l the scalar L, an nq <= 32 point Gauss-Hermite rule as for mf_lik_variational_expectations.  With
 * E f = sum_i w_i f(x_i), E f' = sum_i w_i f'(x_i), x_i = m_k + sqrt(2 S_k) node_i, w_i = weights_i / sqrt pi, dt_k = times[k + 1] - times[k]:
 *   A [B, N] = 1 + E f' dt_k,   b [B, N] = (E f - E f' m_k) dt_k,   cholQ [B, N] = L sqrt(dt_k)
 * - the element counts of the [B, N, 1, 1], [B, N, 1], [B, N, 1, 1] tensors of a state space model.  A point with S_k <= 0 or NaN
 * gets NaN in its own A and b.  Returns 0, -(position: 1 B, 2 N, 3 drift, 4 params, 6 nq, 7 nodes, 8 weights, 9 ... 14 a NULL
 * array) or -1000; B = 0 or N = 0 returns 0 without a launch.
 */
int mf_nlsde_linearize_f64(int64_t B, int64_t N, int drift, const double* params, double chol_l, int nq, const double* nodes,
                           const double* weights, const double* times, const double* mean, const double* var, double* A, double* b,
                           double* cholQ, void* stream);
int mf_nlsde_linearize_f32(int64_t B, int64_t N, int drift, const double* params, float chol_l, int nq, const double* nodes,
                           const double* weights, const float* times, const float* mean, const float* var, float* A, float* b,
                           float* cholQ, void* stream);
/*
 * Expected squared drift difference along a Gaussian path, state dimension 1 (sde_utils.py:161-228): mean, var, A, b [B, N];
 * per point, with r_i = A_k x_i + b_k - f(x_i) at the nodes x_i above,
 *   v_k = scale / 2 sum_i w_i r_i^2                                   scale = dt / q
 *   g_b = scale sum_i w_i r_i,   g_A = scale sum_i w_i r_i x_i,   g_m = scale sum_i w_i r_i (A_k - f'(x_i)),
 *   g_S = scale sum_i w_i r_i (A_k - f'(x_i)) node_i / sqrt(2 S_k)    - the exact derivatives of the discretised v_k;
 * sum [B] = sum_k v_k (required); g_m, g_S, g_A, g_b [B, N], each may be NULL.  The sum runs in a fixed order in double in both
 * precisions - 256 points to one partial by a fixed tree, a series' partials ascending - without floating-point atomics: two calls
 * agree bit for bit, and so does a series alone and inside a batch.  A point with S_k <= 0 or NaN gets NaN in its own four
 * derivatives and makes the sum of ITS series NaN.  N = 0 writes zeros.  workspace: mf_nlsde_drift_difference_workspace_bytes
 * bytes of device memory, 8-byte aligned.  Returns 0, -(position: 1 B, 2 N, 3 drift, 4 params, 5 nq, 6 nodes, 7 weights, 9 ... 12 a
 * NULL input, 13 a NULL sum, 18 a NULL workspace, 19 one that is too small or misaligned) or -1000; B = 0 returns 0 without a launch.
 */
size_t mf_nlsde_drift_difference_workspace_bytes(int64_t B, int64_t N);
int mf_nlsde_drift_difference_f64(int64_t B, int64_t N, int drift, const double* params, int nq, const double* nodes,
                                  const double* weights, double scale, const double* mean, const double* var, const double* A,
                                  const double* b, double* sum, double* g_m, double* g_S, double* g_A, double* g_b, void* workspace,
                                  size_t workspace_bytes, void* stream);
int mf_nlsde_drift_difference_f32(int64_t B, int64_t N, int drift, const double* params, int nq, const double* nodes,
                                  const double* weights, float scale, const float* mean, const float* var, const float* A,
                                  const float* b, float* sum, float* g_m, float* g_S, float* g_A, float* g_b, void* workspace,
                                  size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MARKOVFLOW_AMD_H */
