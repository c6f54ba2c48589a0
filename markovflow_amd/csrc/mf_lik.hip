// Likelihoods for the CVI model (markovflow/models/variational_cvi.py:321-368 with gpflow's likelihoods underneath): per data
// point the expectation of log p(y | f) under N(f | mu, s2), its derivatives with respect to mu and s2, the natural-parameter
// site update built from them, and the log predictive density log E[p(y | f)].
//   lik 0  Gaussian            params [variance]             closed forms
//   lik 1  Bernoulli, probit   gpflow's inv_probit: p = 0.5 (1 + erf(f / sqrt 2)) (1 - 2e-3) + 1e-3
//   lik 2  Poisson, exp link   bin size 1                    closed forms (VE); quadrature (predictive density)
//   lik 3  Student-t           params [scale, df, const]     const = lgamma((df+1)/2) - lgamma(df/2) - log(df pi)/2 - log scale
// Bernoulli and Student-t use an nq-point Gauss-Hermite rule: f_i = mu + sqrt(2 s2) x_i,
//   VE = sum w_i l(f_i),  dVE/dmu = sum w_i l'(f_i),  dVE/ds2 = sum w_i l'(f_i) x_i / sqrt(2 s2)        (w_i = weight_i / sqrt pi)
// - the exact derivatives of the discretised sum, which is what the reference's tape through ndiagquad yields.
// Power expectation propagation (markovflow/models/pep.py) adds the log of the expected alpha-power density with its first two
// derivatives in the mean, and the fused site update built on it (cavity, gradient correction, site normaliser, power / damping step).
// Importance-weighted VI (markovflow/models/iwvi.py) adds the data term of the log importance weights: log p(y | f) itself, at K
// Monte-Carlo samples per point that are assembled in the kernel from one prior draw (no quadrature), with the adjoint onto the draw
// from q at the inducing points.
// The variational GP (markovflow/models/variational.py) adds the dense form of the ELBO's data term: every point has its own marginal
// and emission row, two derivatives per point are kept, and a second kernel expands them onto the marginals.
// One lane per data point; the rule travels by value in the kernel arguments and the loop over its nodes is wavefront-uniform, so
// nodes and weights are scalar loads; no LDS, no cross-lane traffic, no temporaries in memory.
#include "../../include/markovflow_amd.h"

// (the rule, the parameters, log p(y | f), the expectation of one point and the host side's argument checks: shared with mf_st.hip)
#include "mf_lik_math.hpp"
// (the front end of the tile-parallel kernels - tile locator, staging, workspace row -, pass 2 of the SVGP terms and the
// host side's dispatch and tile-table checks: shared with mf_lik_factor.hip, mf_lik_stack.hip and mf_st.hip)
#include "mf_lik_tile.hpp"
// (the multi-stage likelihood's expectation of one point: shared with mf_lik_stack.hip)
#include "mf_lik_multistage.hpp"

namespace {

// Variational expectations (nat1 == NULL) or the CVI site update (nat1, nat2 given): any of ve / g_mu / g_var may be NULL.
template <typename T, int LIK>
__global__ void __launch_bounds__(256) lik_ve_kernel(long N, Rule<T> q, Par<T> p, const T* __restrict__ fmu, const T* __restrict__ fvar,
                                                     const T* __restrict__ yobs, T lr, T* __restrict__ nat1, T* __restrict__ nat2,
                                                     T* __restrict__ out_ve, T* __restrict__ out_gm, T* __restrict__ out_gv) {
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= N) return;
    const T mu = fmu[id], s2 = fvar[id], y = yobs[id];
    T ve, gm, gv;
    if (s2 > T(0)) {
        expectations<T, LIK>(q, p, mu, s2, y, ve, gm, gv);
    } else {                                       // outside the domain (non-positive or NaN variance): NaN for this point only
        ve = gm = gv = nan_of<T>();
    }
    if (out_ve) out_ve[id] = ve;
    if (out_gm) out_gm[id] = gm;
    if (out_gv) out_gv[id] = gv;
    if (nat1) {
        // gradient with respect to the expectation parameters [mu, s2 + mu^2] (variational_cvi.py:448-460), then
        // theta <- (1 - lr) theta + lr g (:351-368)
        const T g1 = gm - T(2) * gv * mu;
        nat1[id] = (T(1) - lr) * nat1[id] + lr * g1;
        nat2[id] = (T(1) - lr) * nat2[id] + lr * gv;
    }
}

// ---- the front end of the two segmented kernels (sparse CVI's site update, SVGP's expected log-likelihood) -----------------------
// One wavefront works on a tile of at most 64 consecutive points of one (series, segment):
//   phase 1, a lane per point: the tile's rows of w travel through LDS, the segment's pair marginal (m_s, S_s) sits in LDS and is read
//            as broadcasts: fmu = w . m_s, fvar = c + w^T S_s w, then the expectations, which leave ROWS rows of 64 values in LDS.
//   phase 2, a lane per few entries of the accumulator - the lower triangle of a 2d x 2d matrix, a 2d vector and, with a third row,
//            one scalar - looping over the tile's points with broadcast LDS reads: entry (i, j) += (row0_k w_kj) w_ki; a vector
//            entry reads row1_k and the column of ones that pads every row of w, the scalar reads row2_k and the ones twice.
// The helpers take the LDS buffers as references to arrays and a point's c as a reference to global memory, not as pointers and a
// value: inlined, they then index and load exactly as the kernels would, and the register allocation stays what it was.

// (tri_decode and seg_entries - entry e of a packed lower triangle is (i, j <= i); the accumulator has the triangle, the vector and one
// scalar per row of LDS values beyond the first two - are in mf_lik_tile.hpp)

// accumulator entry e as (i, j, row of LDS values): e < TRI is (i, j <= i) of the matrix from row 0, then the vector's (j = D2: the
// column of ones) from row 1, then - ROWS = 3 only - the scalar (i = j = D2) from row 2.  A lane's surplus entry decodes as entry 0.
template <int D2, int ROWS>
__device__ __forceinline__ void entry_decode(int e, int& ei, int& ej, int& es) {
    constexpr int TRI = D2 * (D2 + 1) / 2, E = seg_entries(D2, ROWS);
    if (e >= E) e = 0;
    if (e < TRI) {
        tri_decode(e, ei, ej);
        es = 0;
    } else if (ROWS == 2 || e < TRI + D2) {
        ei = e - TRI;
        ej = D2;
        es = 64;
    } else {
        ei = D2;
        ej = D2;
        es = 128;
    }
}

// segment bs' pair marginal into LDS, and the ones that pad every row of w
template <typename T, int D2>
__device__ __forceinline__ void stage_pair(int lane, long bs, const T* pair_mean, const T* pair_cov, T (&ls)[D2 * D2], T (&lm)[D2],
                                           T (&lw)[64 * (D2 + 1)]) {
    for (int idx = lane; idx < D2 * D2; idx += 64) ls[idx] = pair_cov[bs * (D2 * D2) + idx];
    if (lane < D2) lm[lane] = pair_mean[bs * D2 + lane];
    lw[lane * (D2 + 1) + D2] = T(1);
}

// (stage_tile - npts rows of w into LDS at the odd row stride 2d + 1 - is in mf_lik_tile.hpp)

// this lane's point: mu = w . m_s, s2 = c + w^T S_s w
template <typename T, int D2>
__device__ __forceinline__ void project_point(int lane, const T (&lw)[64 * (D2 + 1)], const T (&ls)[D2 * D2], const T (&lm)[D2],
                                              const T& c, T& mu, T& s2) {
    T wr[D2];
#pragma unroll
    for (int i = 0; i < D2; ++i) wr[i] = lw[lane * (D2 + 1) + i];
    mu = T(0);
    s2 = c;
#pragma unroll
    for (int i = 0; i < D2; ++i) {
        T t = T(0);
#pragma unroll
        for (int j = 0; j < D2; ++j) t += ls[i * D2 + j] * wr[j];
        s2 += wr[i] * t;
        mu += wr[i] * lm[i];
    }
}

// phase 2: point k of the tile onto this lane's entries.  The kernels call it for k = 0, 1, ... - the sums run over the points in
// ascending order whatever the grid: the same bits on every launch, alone or inside a batch, and no floating-point atomics.  (The
// loop over the points stays in the kernels: inside a helper the compiler derives its trip count a second time, and the site kernel
// pays for that with five to eight scalar registers.)
template <typename T, int D2, int R, int NG>
__device__ __forceinline__ void accumulate_point(int k, const T (&lg)[NG], const T (&lw)[64 * (D2 + 1)], const int (&ei)[R],
                                                 const int (&ej)[R], const int (&es)[R], T (&part)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) part[r] += (lg[es[r] + k] * lw[k * (D2 + 1) + ej[r]]) * lw[k * (D2 + 1) + ei[r]];
}

// ---- sparse CVI: the segmented site update (markovflow/models/sparse_variational_cvi.py:176-221) ------------------------------
// One wavefront per (series, segment); the segment's points are walked in tiles of 64.  Phase 1 leaves g2 = gv and g1 = gm - 2 gv fmu
// in LDS; the accumulator is the lower triangle of nat2 and nat1, 2d (2d + 1) / 2 + 2d entries (90 at 2d = 12: two per lane, 189 at
// 2d = 18: three).  A tile's sum is formed on its own and then added to the segment's running sum.
// A point outside the domain (fvar <= 0 or NaN) leaves NaN in its own outputs and in its segment's sites.
template <typename T, int LIK, int D2>
__global__ void __launch_bounds__(64) sparse_site_kernel(long N, int S, Rule<T> q, Par<T> p, const long long* __restrict__ seg,
                                                         const T* __restrict__ w, const T* __restrict__ cvar,
                                                         const T* __restrict__ yobs, const T* __restrict__ pair_mean,
                                                         const T* __restrict__ pair_cov, T lr, T* __restrict__ nat1,
                                                         T* __restrict__ nat2, T* __restrict__ out_fmu, T* __restrict__ out_fvar,
                                                         T* __restrict__ out_ve) {
    constexpr int W = D2 + 1, TRI = D2 * (D2 + 1) / 2, E = seg_entries(D2, 2), R = (E + 63) / 64;
    __shared__ T lw[64 * W];
    __shared__ T ls[D2 * D2];
    __shared__ T lm[D2];
    __shared__ T lg[2 * 64];           // g2 of the tile's points, then g1
    const int lane = threadIdx.x;
    const long bs = blockIdx.x;        // series * S + segment
    const long b = bs / S;
    const long s = bs - b * S;
    long k_lo = (long)seg[b * (S + 1) + s], k_hi = (long)seg[b * (S + 1) + s + 1];
    clamp_range(k_lo, k_hi, N);
    int ei[R], ej[R], es[R];           // this lane's entries
    T acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        acc[r] = T(0);
        entry_decode<D2, 2>(lane + 64 * r, ei[r], ej[r], es[r]);
    }
    if (k_hi > k_lo) stage_pair<T, D2>(lane, bs, pair_mean, pair_cov, ls, lm, lw);
    for (long k0 = k_lo; k0 < k_hi; k0 += 64) {
        const int npts = k_hi - k0 < 64 ? int(k_hi - k0) : 64;
        __syncthreads();               // the previous tile's phase 2 has read lw and lg
        stage_tile<T, D2>(lane, npts, w + (b * N + k0) * D2, lw);
        __syncthreads();
        if (lane < npts) {
            const long id = b * N + k0 + lane;
            T mu, s2;
            project_point<T, D2>(lane, lw, ls, lm, cvar[id], mu, s2);
            const T y = yobs[id];
            T ve, gm, gv;
            if (s2 > T(0)) {
                expectations<T, LIK>(q, p, mu, s2, y, ve, gm, gv);
            } else {
                ve = gm = gv = mu = s2 = nan_of<T>();
            }
            if (out_fmu) out_fmu[id] = mu;
            if (out_fvar) out_fvar[id] = s2;
            if (out_ve) out_ve[id] = ve;
            if (nat1) {
                lg[lane] = gv;
                lg[64 + lane] = gm - T(2) * gv * mu;
            }
        }
        if (nat1) {
            __syncthreads();
            T part[R];                 // the tile's own sum first, then onto the running one: the rounding error grows with
#pragma unroll                         // 64 + the number of tiles, not with the length of the segment
            for (int r = 0; r < R; ++r) part[r] = T(0);
            for (int k = 0; k < npts; ++k) accumulate_point<T, D2, R>(k, lg, lw, ei, ej, es, part);
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] += part[r];
        }
    }
    if (nat1) {
        // theta <- (1 - lr) theta + lr sum_k g_k (:215-218); an empty segment just decays
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int e = lane + 64 * r;
            if (e >= E) continue;
            if (e < TRI) {
                T* blk = nat2 + bs * (D2 * D2);
                const int a = ei[r] * D2 + ej[r], t = ej[r] * D2 + ei[r];
                blk[a] = (T(1) - lr) * blk[a] + lr * acc[r];
                if (a != t) blk[t] = (T(1) - lr) * blk[t] + lr * acc[r];
            } else {
                T* v = nat1 + bs * D2 + ei[r];
                *v = (T(1) - lr) * *v + lr * acc[r];
            }
        }
    }
}

// ---- SVGP: the segmented expected log-likelihood and its adjoint onto the pair marginals (markovflow/models/sparse_variational.py
// :149-192, the data term of the ELBO) -----------------------------------------------------------------------------------------
// Two passes, tile-parallel: the grid of pass 1 is the number of TILES, so one long segment spreads over the whole device.
//   pass 1, one wavefront per tile: tile j of a segment starts at the segment's first point + 64 j (the tiling of a segment depends
//            on nothing but the segment).  Phase 1 leaves gv, gm and ve of the tile's points in LDS; the accumulator is the lower
//            triangle of g_cov, g_mean and ONE more entry, sum ve: 2d (2d + 1) / 2 + 2d + 1 entries.  The tile's sums go to the
//            workspace as one contiguous row (coalesced stores).
//   pass 2, one block per (series, segment), a lane per entry: the segment's rows are added in ascending tile order, the outputs
//            are written and the triangle mirrored.  An empty segment writes zeros.
// The tile table comes from the caller: tile_seg[t] = series * S + segment of tile t, seg_tile[series * S + segment] = the first
// tile of the segment (a prefix sum, B S + 1 entries).  It is clamped (locate_tile: mf_lik_tile.hpp), not trusted: a wrong table gives
// wrong numbers and no access outside the buffers.  No floating-point atomics; every sum's order is fixed by the point order alone.
template <typename T, int LIK, int D2>
__global__ void __launch_bounds__(64) sparse_expect_tile_kernel(long N, int S, long BS, Rule<T> q, Par<T> p,
                                                                const long long* __restrict__ seg,
                                                                const long long* __restrict__ tile_seg,
                                                                const long long* __restrict__ seg_tile, const T* __restrict__ w,
                                                                const T* __restrict__ cvar, const T* __restrict__ yobs,
                                                                const T* __restrict__ pair_mean, const T* __restrict__ pair_cov,
                                                                int grads, T* __restrict__ ws) {
    constexpr int W = D2 + 1, E = seg_entries(D2, 3), R = (E + 63) / 64;
    __shared__ T lw[64 * W];
    __shared__ T ls[D2 * D2];
    __shared__ T lm[D2];
    __shared__ T lg[3 * 64];           // gv of the tile's points, then gm, then ve
    const int lane = threadIdx.x;
    const long t = blockIdx.x;
    const TileAt at = locate_tile<64>(t, N, S, BS, seg, tile_seg, seg_tile);
    const long bs = at.bs, b = at.b, k0 = at.k0;
    const int npts = at.npts;
    int ei[R], ej[R], es[R];           // this lane's entries
    T part[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        part[r] = T(0);
        entry_decode<D2, 3>(lane + 64 * r, ei[r], ej[r], es[r]);
    }
    if (npts > 0) {
        stage_pair<T, D2>(lane, bs, pair_mean, pair_cov, ls, lm, lw);
        stage_tile<T, D2>(lane, npts, w + (b * N + k0) * D2, lw);
        __syncthreads();
        if (lane < npts) {
            const long id = b * N + k0 + lane;
            T mu, s2;
            project_point<T, D2>(lane, lw, ls, lm, cvar[id], mu, s2);
            const T y = yobs[id];
            T ve, gm, gv;
            if (s2 > T(0)) {
                expectations<T, LIK>(q, p, mu, s2, y, ve, gm, gv);
            } else {                               // outside the domain: NaN in all three sums of this point's segment
                ve = gm = gv = nan_of<T>();
            }
            lg[lane] = gv;
            lg[64 + lane] = gm;
            lg[128 + lane] = ve;
        }
        __syncthreads();
        if (grads) {
            for (int k = 0; k < npts; ++k) accumulate_point<T, D2, R>(k, lg, lw, ei, ej, es, part);
        } else if (lane == (E - 1) % 64) {         // value only: the one entry, with the bits it has beside the gradients
            for (int k = 0; k < npts; ++k) part[R - 1] += lg[128 + k];
        }
    }
    store_row<E>(ws + t * E, lane, part);
}

// (pass 2, expect_reduce_kernel at K = 1, is in mf_lik_tile.hpp: mf_lik_factor.hip and mf_lik_stack.hip launch it too)

// ---- the multi-stage likelihood: three latents per point, one observation (multistage_expectations: mf_lik_multistage.hpp) -------
// element-wise: a lane per point, fmu / fvar / g_mu / g_var [N, 3]
template <typename T>
__global__ void __launch_bounds__(256) multistage_ve_kernel(long N, Rule<T> q, const T* __restrict__ fmu, const T* __restrict__ fvar,
                                                            const T* __restrict__ yobs, T* __restrict__ out_ve,
                                                            T* __restrict__ out_gm, T* __restrict__ out_gv) {
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= N) return;
    T mu[MULTI_L], s2[MULTI_L], gm[MULTI_L], gv[MULTI_L], ve;
#pragma unroll
    for (int l = 0; l < MULTI_L; ++l) {
        mu[l] = fmu[id * MULTI_L + l];
        s2[l] = fvar[id * MULTI_L + l];
    }
    multistage_expectations<T>(q, yobs[id], mu, s2, ve, gm, gv);
    if (out_ve) out_ve[id] = ve;
#pragma unroll
    for (int l = 0; l < MULTI_L; ++l) {
        if (out_gm) out_gm[id * MULTI_L + l] = gm[l];
        if (out_gv) out_gv[id * MULTI_L + l] = gv[l];
    }
}

// The multi-latent SVGP data term: pass 1 of the tile-parallel pair above with L = 3 dense rows of w per point (w [B, N, L, 2d],
// c [B, N, L]); the tile table, the workspace row (lower triangle of g_cov, g_mean, sum ve) and pass 2 are those of
// sparse_expect_tile_kernel / expect_reduce_kernel.
//   phase 1, a lane per point: the tile's L rows per point travel through LDS as one row of L 2d + 1 elements (odd: the lanes' rows
//            start on distinct banks); per latent mu_l = w_l . m_s, s2_l = c_l + w_l^T S_s w_l; the multi-stage expectation leaves
//            gv_l (rows 0 .. L - 1 of lg), gm_l (rows L .. 2 L - 1) and ve (row 2 L) in LDS;
//   phase 2, a lane per accumulator entry: the points in ascending order and, within a point, the latents in ascending order:
//            g_cov (i, j) += (gv_l w_lj) w_li,  g_mean i += gm_l w_li,  ve_sum += ve.
// The rows are dense on purpose (a FactorAnalysis emission mixes the states): IndependentMultiOutput's zeros are multiplied through.
// LDS at L = 3, 2d = 18, fp64: 28160 + 2592 + 144 + 3584 B = 34480 B.
template <typename T, int D2>
__global__ void __launch_bounds__(64) sparse_multi_expect_tile_kernel(long N, int S, long BS, Rule<T> q,
                                                                      const long long* __restrict__ seg,
                                                                      const long long* __restrict__ tile_seg,
                                                                      const long long* __restrict__ seg_tile, const T* __restrict__ w,
                                                                      const T* __restrict__ cvar, const T* __restrict__ yobs,
                                                                      const T* __restrict__ pair_mean, const T* __restrict__ pair_cov,
                                                                      int grads, T* __restrict__ ws) {
    constexpr int L = MULTI_L, W = L * D2 + 1, TRI = D2 * (D2 + 1) / 2, E = expect_entries(1, D2), R = (E + 63) / 64;
    __shared__ T lw[64 * W];
    __shared__ T ls[D2 * D2];
    __shared__ T lm[D2];
    __shared__ T lg[(2 * L + 1) * 64];
    const int lane = threadIdx.x;
    const long t = blockIdx.x;
    const TileAt at = locate_tile<64>(t, N, S, BS, seg, tile_seg, seg_tile);
    const long bs = at.bs, b = at.b, k0 = at.k0;
    const int npts = at.npts;
    int ei[R], ej[R], kind[R];         // this lane's entries: kind 0 = (ei, ej) of the triangle, 1 = ei of the vector, 2 = the scalar,
    T part[R];                         // 3 = surplus
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = lane + 64 * r;
        part[r] = T(0);
        ei[r] = ej[r] = 0;
        kind[r] = e < TRI ? 0 : (e < TRI + D2 ? 1 : (e < E ? 2 : 3));
        if (kind[r] == 0) tri_decode(e, ei[r], ej[r]);
        if (kind[r] == 1) ei[r] = e - TRI;
    }
    if (npts > 0) {
        for (int idx = lane; idx < D2 * D2; idx += 64) ls[idx] = pair_cov[bs * (D2 * D2) + idx];
        if (lane < D2) lm[lane] = pair_mean[bs * D2 + lane];
        stage_tile<T, L * D2>(lane, npts, w + (b * N + k0) * (L * D2), lw);      // npts rows of L 2d elements
        __syncthreads();
        if (lane < npts) {
            const long id = b * N + k0 + lane;
            T wr[L][D2], mu[L], s2[L], gm[L], gv[L], ve;
#pragma unroll
            for (int l = 0; l < L; ++l) {
#pragma unroll
                for (int i = 0; i < D2; ++i) wr[l][i] = lw[lane * W + l * D2 + i];
                mu[l] = T(0);
                s2[l] = cvar[id * L + l];
            }
#pragma unroll 1
            for (int i = 0; i < D2; ++i) {         // (rolled: unrolled, the compiler keeps all of S_s in registers and spills)
                T acc[L];
#pragma unroll
                for (int l = 0; l < L; ++l) acc[l] = T(0);
#pragma unroll
                for (int c = 0; c < D2; ++c) {
                    const T sic = ls[i * D2 + c];
#pragma unroll
                    for (int l = 0; l < L; ++l) acc[l] += sic * wr[l][c];
                }
                const T mi = lm[i];
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    const T wi = lw[lane * W + l * D2 + i];
                    s2[l] += wi * acc[l];
                    mu[l] += wi * mi;
                }
            }
            multistage_expectations<T>(q, yobs[id], mu, s2, ve, gm, gv);
#pragma unroll
            for (int l = 0; l < L; ++l) {
                lg[l * 64 + lane] = gv[l];
                lg[(L + l) * 64 + lane] = gm[l];
            }
            lg[2 * L * 64 + lane] = ve;
        }
        __syncthreads();
        if (grads) {
            for (int k = 0; k < npts; ++k) {
#pragma unroll
                for (int l = 0; l < L; ++l) {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const T wi = lw[k * W + l * D2 + ei[r]];
                        if (kind[r] == 0) part[r] += (lg[l * 64 + k] * lw[k * W + l * D2 + ej[r]]) * wi;
                        if (kind[r] == 1) part[r] += lg[(L + l) * 64 + k] * wi;
                    }
                }
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (kind[r] == 2) part[r] += lg[2 * L * 64 + k];
            }
        } else if (lane == (E - 1) % 64) {         // value only: the one entry, with the bits it has beside the gradients
            for (int k = 0; k < npts; ++k) part[R - 1] += lg[2 * L * 64 + k];
        }
    }
    store_row<E>(ws + t * E, lane, part);
}

// log of the predictive density  log int p(y | f) N(f | mu, s2) df
template <typename T, int LIK>
__global__ void __launch_bounds__(256) lik_pld_kernel(long N, Rule<T> q, Par<T> p, const T* __restrict__ fmu, const T* __restrict__ fvar,
                                                      const T* __restrict__ yobs, T* __restrict__ out) {
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= N) return;
    const T mu = fmu[id], s2 = fvar[id], y = yobs[id];
    T res;
    if (!(s2 > T(0))) {
        res = nan_of<T>();
    } else if (LIK == 0) {
        constexpr T LOG_2PI = T(1.8378770664093454835606594728112);
        const T v = s2 + p.p0, r = y - mu;
        res = T(-0.5) * (LOG_2PI + m_log(v)) - T(0.5) * r * r / v;
    } else {
        // log-sum-exp over the nodes, shifted by the running maximum (q.w holds the LOG weights here)
        const T sd = m_sqrt(T(2) * s2);
        T m = -INFINITY, s = T(0), dl;
        for (int i = 0; i < q.nq; ++i) {
            const T v = log_prob<T, LIK, false>(mu + sd * q.x[i], y, p, dl) + q.w[i];
            if (v > m) {
                s = s * m_exp(m - v) + T(1);
                m = v;
            } else {
                s += v == -INFINITY ? T(0) : m_exp(v - m);      // (a NaN term lands here and makes the sum NaN)
            }
        }
        res = m + m_log(s);
        if (LIK == 2) res -= m_lgamma(y + T(1));       // the node-independent term of the Poisson log density, once
    }
    out[id] = res;
}

// ---- power expectation propagation (markovflow/models/pep.py:99-215) ----------------------------------------------------------
// I(mu, v; alpha) = log int p(y | f)^alpha N(f | mu, v) df with g1 = dI/dmu and g2 = d2I/dmu2 at one point (v > 0).  Gaussian: closed
// form.  The others: with v_i = alpha l(f_i) + log w_i (q.w holds the LOG weights), p_i = softmax_i v_i,
//   I = logsumexp_i v_i,   g1 = sum p_i alpha l'_i,   g2 = sum p_i (alpha l''_i + alpha^2 l'_i^2) - g1^2
// - the exact derivatives of the discretised sum.  ONE pass over the nodes: the three sums run under the running maximum m, and a
// node costs ONE exponential, exp(-|v - m|), which is the rescale of the sums when the maximum moves and the node's own weight when
// it does not (selects, no branch: the loop stays wavefront-uniform).  A node of weight exactly 0 (v = -inf: a Poisson rate that
// overflowed, whose l' is infinite too) contributes nothing; a NaN lands in the sum of weights and makes all three results NaN.
template <typename T, int LIK>
__device__ __forceinline__ void log_expected_density(const Rule<T>& q, const Par<T>& p, T alpha, T mu, T s2, T y, T& led, T& g1,
                                                     T& g2) {
    if (LIK == 0) {
        constexpr T LOG_2PI = T(1.8378770664093454835606594728112);
        const T sa = p.p0 / alpha, iv = T(1) / (sa + s2), r = y - mu;
        led = T(-0.5) * alpha * (LOG_2PI + m_log(p.p0)) + T(0.5) * (m_log(sa) + m_log(iv)) - T(0.5) * r * r * iv;
        g1 = r * iv;
        g2 = -iv;
    } else {
        const T sd = m_sqrt(T(2) * s2);
        T m = -INFINITY, s0 = T(0), s1 = T(0), sq = T(0);
        for (int i = 0; i < q.nq; ++i) {          // wavefront-uniform: q lives in the kernel arguments
            T dl, d2l;
            const T l = log_prob<T, LIK, true, true>(mu + sd * q.x[i], y, p, dl, d2l);
            const T v = alpha * l + q.w[i], a = alpha * dl, b = alpha * d2l + a * a;
            const bool up = v > m;
            const T e = v == -INFINITY ? T(0) : m_exp(up ? m - v : v - m);
            const T sc = up ? e : T(1), c = up ? T(1) : e;
            const bool live = c > T(0);
            s0 = s0 * sc + c;
            s1 = s1 * sc + (live ? c * a : T(0));
            sq = sq * sc + (live ? c * b : T(0));
            m = up ? v : m;
        }
        const T inv = T(1) / s0;
        // Poisson: the node-independent term of the log density, once.  It cancels against the log-sum-exp (y = 40: 107.8 - 110.3),
        // so the three terms meet in double in both precisions: float32 pays one rounding, of the result.  The float32 Poisson
        // instantiation therefore carries fp64 instructions ON PURPOSE - one double lgamma and two double adds per point, outside
        // the loop over the nodes
        led = LIK == 2 ? T(double(m) + double(m_log(s0)) - double(alpha) * lgamma(double(y) + 1.0)) : m + m_log(s0);
        g1 = s1 * inv;
        g2 = sq * inv - g1 * g1;
    }
}

template <typename T, int LIK>
__global__ void __launch_bounds__(256) lik_led_kernel(long N, Rule<T> q, Par<T> p, T alpha, const T* __restrict__ fmu,
                                                      const T* __restrict__ fvar, const T* __restrict__ yobs, T* __restrict__ out_led,
                                                      T* __restrict__ out_g1, T* __restrict__ out_g2) {
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= N) return;
    const T mu = fmu[id], s2 = fvar[id], y = yobs[id];
    T led, g1, g2;
    if (s2 > T(0)) {
        log_expected_density<T, LIK>(q, p, alpha, mu, s2, y, led, g1, g2);
    } else {                                       // outside the domain (non-positive or NaN variance): NaN for this point only
        led = g1 = g2 = nan_of<T>();
    }
    if (out_led) out_led[id] = led;
    if (out_g1) out_g1[id] = g1;
    if (out_g2) out_g2[id] = g2;
}

// One power-EP step on the sites t(f) = exp(n1 f + n2 f^2 + ln), in place (pep.py:179-215), from the posterior marginal N(m, s) of f:
//   cavity        1 / v_c = 1 / s + 2 alpha n2,   mu_c = v_c (m / s - alpha n1)      (the d x d route of pep.py:120-148 collapses to
//                 this by Sherman-Morrison: the site touches the state through f = h . s only)
//   correction    den = 1 + v_c g2,  L2 = g2 / (2 den),  L1 = (g1 - mu_c g2) / den   with I, g1, g2 at the cavity (pep.py:250-261)
//   normaliser    I + G(mu_c, v_c) - G(m, s),   G(mu, v) = (log v + mu^2 / v) / 2
//   step          pep = (1 - alpha) old + (L1, L2, normaliser),   new = (1 - lr) old + lr pep
// A point is SKIPPED - nothing is stored to its site - when its update flag is off, when s, 1 / v_c or den is not > 0, or when one of
// the new values is not finite.  The cavity goes out for every point (NaN where it does not exist).
template <typename T, int LIK>
__global__ void __launch_bounds__(256) lik_pep_kernel(long N, Rule<T> q, Par<T> p, T alpha, T lr, const T* __restrict__ fmu,
                                                      const T* __restrict__ fvar, const T* __restrict__ yobs,
                                                      const unsigned char* __restrict__ update, T* __restrict__ nat1,
                                                      T* __restrict__ nat2, T* __restrict__ log_norm, T* __restrict__ cav_mu,
                                                      T* __restrict__ cav_var) {
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= N) return;
    const T m = fmu[id], s = fvar[id], y = yobs[id];
    const T n1 = nat1[id], n2 = nat2[id], ln = log_norm[id];
    const T is = T(1) / s, pc = is + T(2) * alpha * n2;
    const bool cavity = s > T(0) && pc > T(0);
    const T vc = cavity ? T(1) / pc : nan_of<T>();
    const T mc = cavity ? vc * (m * is - alpha * n1) : nan_of<T>();
    if (cav_mu) cav_mu[id] = mc;
    if (cav_var) cav_var[id] = vc;
    if (!cavity || (update && !update[id])) return;       // (1 / v_c so small that v_c = inf: the finiteness check below)
    T led, g1, g2;
    log_expected_density<T, LIK>(q, p, alpha, mc, vc, y, led, g1, g2);
    // (Gaussian: den in closed form, free of the cancellation in 1 + v_c g2 - with lr = alpha = 1 the step then returns -1 / (2 s2))
    const T den = LIK == 0 ? (p.p0 / alpha) / (p.p0 / alpha + vc) : T(1) + vc * g2;
    const T l2 = T(0.5) * g2 / den, l1 = (g1 - mc * g2) / den;
    const T norm = led + T(0.5) * (m_log(vc) + mc * mc * pc) - T(0.5) * (m_log(s) + m * m * is);
    const T keep = T(1) - lr, decay = T(1) - alpha;
    const T new1 = keep * n1 + lr * (decay * n1 + l1);
    const T new2 = keep * n2 + lr * (decay * n2 + l2);
    const T newn = keep * ln + lr * (decay * ln + norm);
    if (!(den > T(0)) || !__builtin_isfinite(new1) || !__builtin_isfinite(new2) || !__builtin_isfinite(newn)) return;
    nat1[id] = new1;
    nat2[id] = new2;
    log_norm[id] = newn;
}

// ---- sparse power EP: the segmented site update (markovflow/models/sparse_pep.py:316-380, 473-487) ------------------------------
// The two-pass, tile-parallel layout of the SVGP kernels above, with the same front end at ROWS = 3 and the same tile table.  The
// caller supplies the CAVITY of every pair, N(m_c, S_c), where those kernels get the marginal.
//   pass 1, one wavefront per tile: per point fmu = w . m_c, fvar = c + w^T S_c w, then I, g1, g2 of the log expected alpha-power
//            density there and the gradient correction den = 1 + fvar g2, L2 = g2 / (2 den), L1 = (g1 - fmu g2) / den (Gaussian: den
//            in closed form, as in lik_pep_kernel).  L2, L1 and I are the three rows of LDS values; a point where fvar or den is not
//            > 0 or one of the three is not finite leaves NaN in all of them.  The tile's sums - sum L2 w w^T (lower triangle),
//            sum L1 w, sum I - go to the workspace as one row, as wide as the SVGP kernels' row.
//   pass 2, one block per (series, segment), a lane per entry (190 entries at 2d = 18): the segment's rows are added in ascending
//            tile order; then, if EVERY entry of the segment is finite (the scalar one with seg_const added),
//            pep = (1 - alpha) old + sum, new = (1 - lr) old + lr pep onto nat2 (both triangles), nat1 and log_norm; otherwise
//            nothing is stored to the three site tensors of this segment.  The decision is the block's and precedes every store.
// No floating-point atomics; every sum's order is fixed by the point order alone.  The tile table is clamped, not trusted.
template <typename T, int LIK, int D2>
__global__ void __launch_bounds__(64) sparse_pep_tile_kernel(long N, int S, long BS, Rule<T> q, Par<T> p, T alpha,
                                                             const long long* __restrict__ seg,
                                                             const long long* __restrict__ tile_seg,
                                                             const long long* __restrict__ seg_tile, const T* __restrict__ w,
                                                             const T* __restrict__ cvar, const T* __restrict__ yobs,
                                                             const T* __restrict__ cav_mean, const T* __restrict__ cav_cov,
                                                             int sites, T* __restrict__ ws, T* __restrict__ out_fmu,
                                                             T* __restrict__ out_fvar, T* __restrict__ out_led) {
    constexpr int W = D2 + 1, E = seg_entries(D2, 3), R = (E + 63) / 64;
    __shared__ T lw[64 * W];
    __shared__ T ls[D2 * D2];
    __shared__ T lm[D2];
    __shared__ T lg[3 * 64];           // L2 of the tile's points, then L1, then I
    const int lane = threadIdx.x;
    const long t = blockIdx.x;
    const TileAt at = locate_tile<64>(t, N, S, BS, seg, tile_seg, seg_tile);
    const long bs = at.bs, b = at.b, k0 = at.k0;
    const int npts = at.npts;
    int ei[R], ej[R], es[R];           // this lane's entries
    T part[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        part[r] = T(0);
        entry_decode<D2, 3>(lane + 64 * r, ei[r], ej[r], es[r]);
    }
    if (npts > 0) {
        stage_pair<T, D2>(lane, bs, cav_mean, cav_cov, ls, lm, lw);
        stage_tile<T, D2>(lane, npts, w + (b * N + k0) * D2, lw);
        __syncthreads();
        if (lane < npts) {
            const long id = b * N + k0 + lane;
            T mu, s2;
            project_point<T, D2>(lane, lw, ls, lm, cvar[id], mu, s2);
            const T y = yobs[id];
            T led, l1, l2;
            if (s2 > T(0)) {
                T g1, g2;
                log_expected_density<T, LIK>(q, p, alpha, mu, s2, y, led, g1, g2);
                const T den = LIK == 0 ? (p.p0 / alpha) / (p.p0 / alpha + s2) : T(1) + s2 * g2;
                l2 = T(0.5) * g2 / den;
                l1 = (g1 - mu * g2) / den;
                if (out_led) out_led[id] = led;
                if (!(den > T(0)) || !__builtin_isfinite(l2) || !__builtin_isfinite(l1) || !__builtin_isfinite(led))
                    led = l1 = l2 = nan_of<T>();
            } else {                               // outside the domain (a cavity that does not exist arrives as NaN)
                led = l1 = l2 = mu = s2 = nan_of<T>();
                if (out_led) out_led[id] = led;
            }
            if (out_fmu) out_fmu[id] = mu;
            if (out_fvar) out_fvar[id] = s2;
            lg[lane] = l2;
            lg[64 + lane] = l1;
            lg[128 + lane] = led;
        }
        __syncthreads();
        if (sites) {
            for (int k = 0; k < npts; ++k) accumulate_point<T, D2, R>(k, lg, lw, ei, ej, es, part);
        } else if (lane == (E - 1) % 64) {         // evaluation only: the one entry, with the bits it has beside the update
            for (int k = 0; k < npts; ++k) part[R - 1] += lg[128 + k];
        }
    }
    store_row<E>(ws + t * E, lane, part);
}

template <typename T, int D2>
__global__ void __launch_bounds__(256) sparse_pep_reduce_kernel(long num_tiles, const long long* __restrict__ seg_tile,
                                                                const T* __restrict__ ws, const T* __restrict__ seg_const, T alpha,
                                                                T lr, T* __restrict__ nat1, T* __restrict__ nat2,
                                                                T* __restrict__ log_norm, T* __restrict__ led_sum) {
    constexpr int TRI = D2 * (D2 + 1) / 2, E = seg_entries(D2, 3);
    static_assert(E <= 256, "one entry per lane");
    __shared__ int undefined;
    const long bs = blockIdx.x;
    const int e = threadIdx.x;
    long t_lo = 0, t_hi = 0;
    if (seg_tile) {                                // (NULL: no points at all)
        t_lo = (long)seg_tile[bs];
        t_hi = (long)seg_tile[bs + 1];
        clamp_range(t_lo, t_hi, num_tiles);
    }
    if (e == 0) undefined = 0;
    __syncthreads();
    T acc = T(0);
    if (e < E && (nat1 || e == E - 1)) {           // (evaluation only: pass 1 has summed the scalar entry alone)
        for (long t = t_lo; t < t_hi; ++t) acc += ws[t * E + e];
        if (e == E - 1) {
            if (led_sum) led_sum[bs] = acc;        // the raw sum, NaN included
            if (seg_const) acc += seg_const[bs];
        }
        if (!__builtin_isfinite(acc)) undefined = 1;
    }
    __syncthreads();
    if (!nat1 || undefined || e >= E) return;      // an undefined segment keeps its sites, bit for bit
    const T keep = T(1) - lr, decay = T(1) - alpha;
    if (e < TRI) {
        int i, c;
        tri_decode(e, i, c);
        T* blk = nat2 + bs * (D2 * D2);
        const int a = i * D2 + c, m = c * D2 + i;
        const T lo = blk[a], up = blk[m];
        blk[a] = keep * lo + lr * (decay * lo + acc);
        if (a != m) blk[m] = keep * up + lr * (decay * up + acc);
    } else if (e < E - 1) {
        T* v = nat1 + bs * D2 + (e - TRI);
        const T old = *v;
        *v = keep * old + lr * (decay * old + acc);
    } else {
        const T old = log_norm[bs];
        log_norm[bs] = keep * old + lr * (decay * old + acc);
    }
}

// ---- importance-weighted VI: the log importance weights' data term (markovflow/models/iwvi.py:109-173, posterior.py:522-580) ---------
// K Monte-Carlo evaluations of log p(y_n | f_n) at every data point, on samples assembled here from ONE prior draw on the merged,
// sorted time points (states [K, B, N + M, d]: data point n of segment s at row n + s, inducing point m at row offsets[m + 1] + m)
// and the posterior draw u_post [K, B, M, d] at the inducing points - Matheron's rule, whose correction only involves the two
// inducing states around a point:
//   dL = prior(z_{s-1}) - u_post_{s-1} (0 for s = 0),  dR = prior(z_s) - u_post_s (0 for s = M),
//   f = (h . prior(x_n) - w[n, :d] . dL) - w[n, d:] . dR,   l = log p(y_n | f),  l' = dl/df
// u_post == NULL: states [K, B, N, d] holds final samples, point n at row n, f = h . states(n) (w is not read and may be NULL).
// The two-pass, tile-parallel layout of the SVGP kernels, with the same tile table.
//   pass 1, one wavefront per (tile, chunk of IW_CHUNK samples), a lane per point: the tile's rows of w travel through LDS once and
//            stay in the lane's registers with y and the Poisson constant for every sample of the chunk; the chunk's (dL, dR) sit in
//            LDS and are read as broadcasts.  Per sample the tile's rows of the prior draw - npts d CONTIGUOUS values - come in
//            with coalesced loads (the next sample's are in flight while this one's density is evaluated), pass through LDS at an
//            odd row stride and leave l' and l there.  Then a lane per (sample, column) entry, 2d + 1 per sample: entry (k, c < 2d)
//            = sum_n l'_n w[n, c], entry (k, 2d) = sum_n l_n (through the column of ones that pads every row of w), over the
//            tile's points in ascending order.  The chunk's entries go to the workspace as one contiguous run, row (tile, sample).
//   pass 2, one block per (series, segment), a lane per (sample, output): log_lik[k, b, s] adds the segment's tiles in ascending
//            order; g_u[k, b, m, i] adds the tiles of segment m (column d + i), then those of segment m + 1 (column i).
// No atomics; every sum's order is fixed by the point order alone, and a sum never mixes samples or series: the same bits on every
// launch, for a series alone or in a batch, for a sample alone or among K.  The tile table and the offsets are clamped, not trusted.
constexpr int IW_CHUNK = 8;            // samples per block of pass 1

template <typename T, int LIK, int D2>
__global__ void __launch_bounds__(64) iw_tile_kernel(long N, int S, long BS, long B, long K, int chunks, Par<T> p,
                                                     const long long* __restrict__ seg, const long long* __restrict__ tile_seg,
                                                     const long long* __restrict__ seg_tile, const T* __restrict__ w,
                                                     const T* __restrict__ yobs, const T* __restrict__ h,
                                                     const T* __restrict__ states, const T* __restrict__ u_post, int grads,
                                                     T* __restrict__ ws) {
    constexpr int D = D2 / 2, W = D2 + 1, E = D2 + 1, DP = D | 1, LG = 129, R = (IW_CHUNK * E + 63) / 64;
    __shared__ T lw[64 * W];
    __shared__ T lx[64 * DP];          // the tile's rows of one sample of the prior draw
    __shared__ T ld[IW_CHUNK * D2];    // (dL, dR) of the chunk's samples
    __shared__ T lg[IW_CHUNK * LG];    // per sample l' of the tile's points, then l (stride 129: the samples start on distinct banks)
    const int lane = threadIdx.x;
    const long t = blockIdx.x / chunks;
    const long k_base = (blockIdx.x - t * chunks) * IW_CHUNK;
    const int kc = K - k_base < IW_CHUNK ? int(K - k_base) : IW_CHUNK;
    const TileAt at = locate_tile<64>(t, N, S, BS, seg, tile_seg, seg_tile);
    const long b = at.b, k_lo = at.k_lo, k_hi = at.k_hi, k0 = at.k0;
    const int s = int(at.s), npts = at.npts;
    const long rows = u_post ? N + (S - 1) : N;                     // rows of one (sample, series) of states
    const long row0 = u_post ? k0 + s : k0;                         // the row of the tile's first point
    T part[R];
#pragma unroll
    for (int r = 0; r < R; ++r) part[r] = T(0);
    if (npts > 0) {
        // (dL, dR) of every sample of the chunk; beyond both ends the correction vanishes
        for (int idx = lane; idx < kc * D2; idx += 64) {
            const int kk = idx / D2, c = idx - kk * D2, side = c / D, i = c - side * D;
            const long m = s - 1 + side;                            // the inducing point left (side 0) or right of the segment
            T delta = T(0);
            if (u_post && m >= 0 && m < S - 1) {
                const long kb = (k_base + kk) * B + b;
                const long zrow = (side ? k_hi : k_lo) + m;         // offsets[m + 1] + m
                delta = states[(kb * rows + zrow) * D + i] - u_post[(kb * (S - 1) + m) * D + i];
            }
            ld[idx] = delta;
        }
        lw[lane * W + D2] = T(1);
        if (u_post) {
            stage_tile<T, D2>(lane, npts, w + (b * N + k0) * D2, lw);
        } else {
            for (int idx = lane; idx < 64 * D2; idx += 64) lw[(idx / D2) * W + idx % D2] = T(0);
        }
        T xr[D];                       // this lane's share of the next sample's rows: elements lane, lane + 64, ...
        const T* src = states + ((k_base * B + b) * rows + row0) * D;
        const long k_stride = B * rows * D;
#pragma unroll
        for (int q = 0; q < D; ++q) xr[q] = lane + 64 * q < npts * D ? src[lane + 64 * q] : T(0);
        __syncthreads();
        T wr[D2], hr[D];
        T y = T(0), lgam = T(0);
#pragma unroll
        for (int i = 0; i < D2; ++i) wr[i] = lw[lane * W + i];
#pragma unroll
        for (int i = 0; i < D; ++i) hr[i] = h[i];
        if (lane < npts) {
            y = yobs[b * N + k0 + lane];
            if (LIK == 2) lgam = m_lgamma(y + T(1));                // once per point, not per sample
        }
        for (int kk = 0; kk < kc; ++kk) {
#pragma unroll
            for (int q = 0; q < D; ++q) {
                const int idx = lane + 64 * q;
                if (idx < npts * D) lx[(idx / D) * DP + idx % D] = xr[q];
            }
            __syncthreads();
            if (kk + 1 < kc) {
#pragma unroll
                for (int q = 0; q < D; ++q) xr[q] = lane + 64 * q < npts * D ? src[(kk + 1) * k_stride + lane + 64 * q] : T(0);
            }
            if (lane < npts) {
                T f = T(0);
#pragma unroll
                for (int i = 0; i < D; ++i) f += hr[i] * lx[lane * DP + i];
                if (u_post) {
                    T cl = T(0), cr = T(0);
#pragma unroll
                    for (int i = 0; i < D; ++i) cl += wr[i] * ld[kk * D2 + i];
#pragma unroll
                    for (int i = 0; i < D; ++i) cr += wr[D + i] * ld[kk * D2 + D + i];
                    f = (f - cl) - cr;
                }
                T dl;
                const T l = log_prob<T, LIK, true>(f, y, p, dl);
                lg[kk * LG + lane] = dl;
                lg[kk * LG + 64 + lane] = LIK == 2 ? l - lgam : l;
            }
            __syncthreads();           // lx is free for the next sample; after the last one l' and l are complete
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int e = lane + 64 * r, kk = e / E, c = e - kk * E;
            if (kk >= kc || !(grads || c == D2)) continue;
            const T* g = lg + kk * LG + (c == D2 ? 64 : 0);
            T acc = T(0);
            for (int n = 0; n < npts; ++n) acc += g[n] * lw[n * W + c];
            part[r] = acc;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = lane + 64 * r, kk = e / E, c = e - kk * E;
        if (kk < kc && (grads || c == D2)) ws[(t * K + k_base) * E + e] = part[r];
    }
}

template <typename T, int D2>
__global__ void __launch_bounds__(256) iw_reduce_kernel(long num_tiles, int S, long B, long K, const long long* __restrict__ seg_tile,
                                                        const T* __restrict__ ws, T* __restrict__ log_lik, T* __restrict__ g_u) {
    constexpr int D = D2 / 2, E = D2 + 1;
    const long bs = blockIdx.x;
    const long b = bs / S;
    const int s = int(bs - b * S), M = S - 1;
    long t_lo = 0, t_hi = 0, n_lo = 0, n_hi = 0;       // the tiles of this segment and of the next
    if (seg_tile) {                                    // (NULL: no points at all)
        t_lo = (long)seg_tile[bs];
        t_hi = (long)seg_tile[bs + 1];
        clamp_range(t_lo, t_hi, num_tiles);
        if (s < M) {
            n_lo = (long)seg_tile[bs + 1];
            n_hi = (long)seg_tile[bs + 2];
            clamp_range(n_lo, n_hi, num_tiles);
        }
    }
    for (long idx = threadIdx.x; idx < K * (D + 1); idx += 256) {
        const long k = idx / (D + 1);
        const int i = int(idx - k * (D + 1));
        T acc = T(0);
        if (i == D) {
            if (!log_lik) continue;
            for (long t = t_lo; t < t_hi; ++t) acc += ws[(t * K + k) * E + D2];
            log_lik[(k * B + b) * S + s] = acc;
        } else {
            if (!g_u || s >= M) continue;
            for (long t = t_lo; t < t_hi; ++t) acc += ws[(t * K + k) * E + D + i];       // inducing point s is this segment's right
            for (long t = n_lo; t < n_hi; ++t) acc += ws[(t * K + k) * E + i];           // neighbour and the next one's left
            g_u[((k * B + b) * M + s) * D + i] = acc;
        }
    }
}

// ---- VGP: the dense (unsegmented) expected log-likelihood and its adjoint onto the marginals of q (markovflow/models/variational.py
// :129-152, the data term of the ELBO) --------------------------------------------------------------------------------------------
// q lives on the states at the data points themselves: point k of series b has its own marginal (m_k [d], P_k [d, d]) and its own
// emission row h_k [d].  Two passes, tile-parallel; tile t of a series is its points 64 t ... 64 t + 63, so no table is needed.
//   pass 1, one wavefront per tile.  The tile's h, means and covs are CONTIGUOUS runs of 64 d, 64 d and 64 d^2 elements: they come in
//            with consecutive lanes on consecutive elements and pass through LDS at the odd row stride d | 1 (a row = d elements:
//            one point's h or m, one ROW of one point's P), so that lanes on consecutive rows start on distinct banks.  covs comes
//            in slabs of DENSE_SLAB_BYTES at the most (whole points: 64, 32, 16 or 8 of them), which bounds the LDS of a block
//            whatever d.  Per slab a lane per (point, row i): t_i = sum_j P_ij h_j into LDS.  Then a lane per point:
//            fmu = sum_i h_i m_i, fvar = sum_i h_i t_i, the expectations, g_mu and g_var stored (coalesced), ve through LDS to
//            lane 0, which adds the tile's points in ascending order and leaves ONE partial in the workspace.
//   pass 2, one lane per series: the series' partials are added in ascending tile order.  N = 0 writes zeros.
// THE ORDER OF THE SUMS IS PART OF THE CONTRACT (the float32 test helper repeats it): every sum starts from 0 and grows term by
// term with its index ascending - t_i in j, fmu and fvar in i (the full matrix is read, both triangles), a tile in its points, a
// series in its tiles; the last two run in a double accumulator in float32 too (one rounding into the workspace, one into ve_sum:
// a series of 10^4 points adds 157 partials, which a float accumulator would round 157 times).  No atomics: the same bits on every
// launch, for a series alone or inside a batch, with or without the gradients.  A point outside the domain (fvar <= 0 or NaN) leaves NaN in its g_mu, g_var and in its series' sum, nowhere else.
constexpr int DENSE_MAX_D = 12;
constexpr int DENSE_SLAB_BYTES = 16384;

// points per slab of covs: the most of 64, 32, 16, 8 whose padded rows fit DENSE_SLAB_BYTES (d = 12 in float64: 8 points, 9984 B)
template <typename T, int D>
constexpr int dense_slab_points() {
    int sp = 64;
    while (sp > 8 && size_t(sp) * D * (D | 1) * sizeof(T) > size_t(DENSE_SLAB_BYTES)) sp /= 2;
    return sp;
}

template <typename T, int LIK, int D>
__global__ void __launch_bounds__(64) dense_expect_tile_kernel(long N, long tiles_per_series, Rule<T> q, Par<T> p,
                                                               const T* __restrict__ h, const T* __restrict__ means,
                                                               const T* __restrict__ covs, const T* __restrict__ yobs,
                                                               T* __restrict__ ws, T* __restrict__ out_gm, T* __restrict__ out_gv) {
    constexpr int DP = D | 1, SP = dense_slab_points<T, D>();
    __shared__ T lh[64 * DP];          // the tile's rows of h
    __shared__ T lm[64 * DP];          // the tile's means
    __shared__ T lt[64 * DP];          // t_i = sum_j P_ij h_j of the tile's points
    __shared__ T lp[SP * D * DP];      // one slab of covs: row (point, i) at stride DP
    __shared__ T lv[64];               // ve of the tile's points
    const int lane = threadIdx.x;
    const long b = blockIdx.x / tiles_per_series;
    const long k0 = (blockIdx.x - b * tiles_per_series) * 64;
    const int npts = N - k0 < 64 ? int(N - k0) : 64;               // (>= 1: the grid has ceil(N / 64) tiles per series)
    const long first = b * N + k0;                                 // the tile's first point
    for (int idx = lane; idx < npts * D; idx += 64) {
        const int at = (idx / D) * DP + idx % D;
        lh[at] = h[first * D + idx];
        lm[at] = means[first * D + idx];
    }
    for (int s0 = 0; s0 < npts; s0 += SP) {
        const int sp = npts - s0 < SP ? npts - s0 : SP;
        const T* src = covs + (first + s0) * (D * D);
        __syncthreads();               // lh is staged; the previous slab's rows have been read
        for (int idx = lane; idx < sp * D * D; idx += 64) lp[(idx / D) * DP + idx % D] = src[idx];
        __syncthreads();
        for (int r = lane; r < sp * D; r += 64) {                  // row r of the slab: point s0 + r / D, row r % D of its P
            const int k = s0 + r / D;
            T t = T(0);
#pragma unroll
            for (int j = 0; j < D; ++j) t += lp[r * DP + j] * lh[k * DP + j];
            lt[k * DP + r % D] = t;
        }
    }
    __syncthreads();
    if (lane < npts) {
        T mu = T(0), s2 = T(0);
#pragma unroll
        for (int i = 0; i < D; ++i) {
            mu += lh[lane * DP + i] * lm[lane * DP + i];
            s2 += lh[lane * DP + i] * lt[lane * DP + i];
        }
        const T y = yobs[first + lane];
        T ve, gm, gv;
        if (s2 > T(0)) {
            expectations<T, LIK>(q, p, mu, s2, y, ve, gm, gv);
        } else {                                   // outside the domain: NaN for this point and its series' sum
            ve = gm = gv = nan_of<T>();
        }
        if (out_gm) {
            out_gm[first + lane] = gm;
            out_gv[first + lane] = gv;
        }
        lv[lane] = ve;
    }
    if (!ws) return;                               // (the gradients alone)
    __syncthreads();
    if (lane == 0) {
        double acc = 0.0;                          // (float32: the accumulator is a double, rounded once into the workspace)
        for (int k = 0; k < npts; ++k) acc += double(lv[k]);
        ws[blockIdx.x] = T(acc);
    }
}

template <typename T>
__global__ void __launch_bounds__(64) dense_expect_reduce_kernel(long B, long tiles_per_series, const T* __restrict__ ws,
                                                                 T* __restrict__ ve_sum) {
    const long b = (long)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double acc = 0.0;
    for (long t = 0; t < tiles_per_series; ++t) acc += double(ws[b * tiles_per_series + t]);
    ve_sum[b] = T(acc);
}

// The adjoint's expansion: g_means = (weight g_mu) h and g_covs = (weight (g_var h_i)) h_j, what mf_ssm_marginals_grad_* reads.  Pure
// stores: a lane per output element, consecutive lanes on consecutive elements of g_covs [B N d^2], then of g_means [B N d] (one
// index space, so one launch); the 2 + d values a point reads are shared by the d^2 + d lanes around it and come from the caches.
template <typename T, int D>
__global__ void __launch_bounds__(256) dense_adjoint_kernel(long BN, long N, const T* __restrict__ h, const T* __restrict__ g_mu,
                                                            const T* __restrict__ g_var, const T* __restrict__ weight,
                                                            T* __restrict__ g_means, T* __restrict__ g_covs) {
    const long n_cov = g_covs ? BN * (D * D) : 0, n_all = n_cov + (g_means ? BN * D : 0);
    const long stride = (long)gridDim.x * 256;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n_all; e += stride) {
        if (e < n_cov) {
            const long k = e / (D * D);
            const int r = int(e - k * (D * D)), i = r / D, j = r - i * D;
            const T w = weight ? weight[k / N] : T(1);
            g_covs[e] = (w * (g_var[k] * h[k * D + i])) * h[k * D + j];
        } else {
            const long m = e - n_cov, k = m / D;
            const T w = weight ? weight[k / N] : T(1);
            g_means[m] = (w * g_mu[k]) * h[m];
        }
    }
}

// (prepare, first_null and with_lik - the argument checks shared by every entry point - are in mf_lik_math.hpp)

// (with_even_two_d - the same as with_lik for the pair dimension of the segmented kernels - and launch - one launch, the arguments
// converted to the kernel's parameter types - are in mf_lik_tile.hpp)

// variational expectations (nat1 == NULL) or the CVI site update: the one kernel behind both
template <typename T>
int launch_ve(int64_t N, int lik, const Rule<T>& q, const Par<T>& p, const T* fmu, const T* fvar, const T* y, T lr, T* nat1, T* nat2,
              T* ve, T* g_mu, T* g_var, void* stream) {
    return with_lik(lik, [&](auto L) {
        return launch(lik_ve_kernel<T, decltype(L)::value>, (N + 255) / 256, 256, stream, N, q, p, fmu, fvar, y, lr, nat1, nat2, ve,
                      g_mu, g_var);
    });
}

template <typename T>
int run_ve(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights, const T* fmu, const T* fvar,
           const T* y, T* ve, T* g_mu, T* g_var, void* stream) {
    Rule<T> q;
    Par<T> p;
    int bad = prepare<T>(N, lik, params, nq, nodes, weights, false, q, p);
    if (bad) return bad;
    if (N == 0) return 0;
    if ((bad = first_null(7, {fmu, fvar, y}))) return bad;
    if (!ve && !g_mu && !g_var) return 0;          // nothing asked for
    return launch_ve<T>(N, lik, q, p, fmu, fvar, y, T(0), nullptr, nullptr, ve, g_mu, g_var, stream);
}

template <typename T>
int run_site(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights, const T* fmu, const T* fvar,
             const T* y, T lr, T* nat1, T* nat2, T* ve, void* stream) {
    Rule<T> q;
    Par<T> p;
    int bad = prepare<T>(N, lik, params, nq, nodes, weights, false, q, p);
    if (bad) return bad;
    if (!(lr >= T(0)) || !(lr <= T(1))) return -10;
    if (N == 0) return 0;
    if ((bad = first_null(7, {fmu, fvar, y}))) return bad;
    if ((bad = first_null(11, {nat1, nat2}))) return bad;
    return launch_ve<T>(N, lik, q, p, fmu, fvar, y, lr, nat1, nat2, ve, nullptr, nullptr, stream);
}

template <typename T>
int run_pld(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights, const T* fmu, const T* fvar,
            const T* y, T* out, void* stream) {
    Rule<T> q;
    Par<T> p;
    int bad = prepare<T>(N, lik, params, nq, nodes, weights, true, q, p);
    if (bad) return bad;
    if (N == 0) return 0;
    if ((bad = first_null(7, {fmu, fvar, y, out}))) return bad;
    return with_lik(lik, [&](auto L) {
        return launch(lik_pld_kernel<T, decltype(L)::value>, (N + 255) / 256, 256, stream, N, q, p, fmu, fvar, y, out);
    });
}

template <typename T>
int run_led(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights, T alpha, const T* fmu,
            const T* fvar, const T* y, T* led, T* g1, T* g2, void* stream) {
    Rule<T> q;
    Par<T> p;
    int bad = prepare<T>(N, lik, params, nq, nodes, weights, true, q, p);
    if (bad) return bad;
    if (!(alpha > T(0)) || !(alpha <= T(1))) return -7;
    if (N == 0) return 0;
    if ((bad = first_null(8, {fmu, fvar, y}))) return bad;
    if (!led && !g1 && !g2) return 0;              // nothing asked for
    return with_lik(lik, [&](auto L) {
        return launch(lik_led_kernel<T, decltype(L)::value>, (N + 255) / 256, 256, stream, N, q, p, alpha, fmu, fvar, y, led, g1, g2);
    });
}

template <typename T>
int run_pep(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights, T alpha, T lr, const T* fmu,
            const T* fvar, const T* y, const unsigned char* update, T* nat1, T* nat2, T* log_norm, T* cav_mu, T* cav_var,
            void* stream) {
    Rule<T> q;
    Par<T> p;
    int bad = prepare<T>(N, lik, params, nq, nodes, weights, true, q, p);
    if (bad) return bad;
    if (!(alpha > T(0)) || !(alpha <= T(1))) return -7;
    if (!(lr >= T(0)) || !(lr <= T(1))) return -8;
    if (N == 0) return 0;
    if ((bad = first_null(9, {fmu, fvar, y}))) return bad;
    if ((bad = first_null(13, {nat1, nat2, log_norm}))) return bad;       // (12 is update, which may be NULL)
    return with_lik(lik, [&](auto L) {
        return launch(lik_pep_kernel<T, decltype(L)::value>, (N + 255) / 256, 256, stream, N, q, p, alpha, lr, fmu, fvar, y, update,
                      nat1, nat2, log_norm, cav_mu, cav_var);
    });
}

// the leading argument checks of the segmented entry points: the (negative) position of the offending argument in THEIR
// signature (check_segmentation: mf_lik_tile.hpp), -100 for a two_d outside 2, 4, ..., 18
template <typename T>
int prepare_segmented(int64_t B, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq, const double* nodes,
                      const double* weights, Rule<T>& q, Par<T>& p, bool log_weights = false) {
    int bad = check_segmentation(B, N, S);
    if (bad) return bad;
    if (two_d < 2 || two_d > 18 || (two_d & 1)) return -100;
    bad = prepare<T>(0, lik, params, nq, nodes, weights, log_weights, q, p);                // -2 ... -6 there: arguments 5 ... 9 here
    return bad ? bad - 3 : 0;
}

template <typename T>
int run_sparse(int64_t B, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq, const double* nodes,
               const double* weights, const int64_t* seg, const T* w, const T* c, const T* y, const T* pm, const T* pc, T lr,
               T* nat1, T* nat2, T* fmu, T* fvar, T* ve, void* stream) {
    Rule<T> q;
    Par<T> p;
    int bad = prepare_segmented<T>(B, N, S, two_d, lik, params, nq, nodes, weights, q, p);
    if (bad) return bad;
    if (!(lr >= T(0)) || !(lr <= T(1))) return -16;
    if (!nat1 && nat2) return -17;
    if (nat1 && !nat2) return -18;
    if (B == 0) return 0;
    if (!nat1 && (N == 0 || (!fmu && !fvar && !ve))) return 0;      // nothing asked for
    if (!seg) return -10;
    if (N > 0 && (bad = first_null(11, {w, c, y, pm, pc}))) return bad;
    return with_even_two_d<2>(two_d, -100, [&](auto D) {
        return with_lik(lik, [&](auto L) {
            return launch(sparse_site_kernel<T, decltype(L)::value, decltype(D)::value>, B * S, 64, stream, N, S, q, p, ll(seg), w, c,
                          y, pm, pc, lr, nat1, nat2, fmu, fvar, ve);
        });
    });
}

// (expect_row, the workspace row of a tile, and check_tile_count / check_tile_table are in mf_lik_tile.hpp)

template <typename T>
int run_expect(int64_t B, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq, const double* nodes,
               const double* weights, const int64_t* seg, const T* w, const T* c, const T* y, const T* pm, const T* pc,
               int64_t tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* ws, size_t ws_bytes, T* ve_sum, T* g_mean,
               T* g_cov, void* stream) {
    Rule<T> q;
    Par<T> p;
    int bad = prepare_segmented<T>(B, N, S, two_d, lik, params, nq, nodes, weights, q, p);
    if (bad) return bad;
    if ((bad = check_tile_count(16, N, tiles))) return bad;
    if (!g_mean && g_cov) return -22;
    if (g_mean && !g_cov) return -23;
    if (B == 0 || (!ve_sum && !g_mean)) return 0;      // nothing asked for
    if (tiles > 0) {
        if ((bad = first_null(10, {seg, w, c, y, pm, pc}))) return bad;
        if ((bad = check_tile_table(16, tiles, tile_seg, seg_tile, ws, ws_bytes, expect_row(two_d), sizeof(T)))) return bad;
    }
    return with_even_two_d<2>(two_d, -100, [&](auto D) {
        constexpr int D2 = decltype(D)::value;
        if (tiles > 0) {
            const int rc = with_lik(lik, [&](auto L) {
                return launch(sparse_expect_tile_kernel<T, decltype(L)::value, D2>, tiles, 64, stream, N, S, B * S, q, p, ll(seg),
                              ll(tile_seg), ll(seg_tile), w, c, y, pm, pc, g_mean ? 1 : 0, ws);
            });
            if (rc) return rc;
        }
        return launch(expect_reduce_kernel<T, 1, D2>, B * S, 256, stream, tiles, S, tiles > 0 ? ll(seg_tile) : nullptr, ws, ve_sum,
                      g_mean, g_cov);
    });
}

// the multi-latent pair: instantiated for (two_d, latent_dim, lik) = (6 ... 18 even, 3, multi-stage), -101 for any other signature.
// The likelihood has no parameters (params is not read); the workspace row and pass 2 are the single-latent pair's.
template <typename T>
int run_multi_expect(int64_t B, int64_t N, int64_t S, int two_d, int latent_dim, int lik, int nq, const double* nodes,
                     const double* weights, const int64_t* seg, const T* w, const T* c, const T* y, const T* pm, const T* pc,
                     int64_t tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* ws, size_t ws_bytes, T* ve_sum, T* g_mean,
                     T* g_cov, void* stream) {
    Rule<T> q;
    Par<T> p;
    int bad = check_segmentation(B, N, S);
    if (bad) return bad;
    if (latent_dim != MULTI_L || lik != LIK_MULTISTAGE || two_d < 6 || two_d > 18 || (two_d & 1)) return -101;
    bad = prepare<T>(0, 1, nullptr, nq, nodes, weights, false, q, p);            // -4 ... -6 there: arguments 8 ... 10 here
    if (bad) return bad - 4;
    if ((bad = check_tile_count(17, N, tiles))) return bad;
    if (!g_mean && g_cov) return -23;
    if (g_mean && !g_cov) return -24;
    if (B == 0 || (!ve_sum && !g_mean)) return 0;      // nothing asked for
    if (tiles > 0) {
        if ((bad = first_null(11, {seg, w, c, y, pm, pc}))) return bad;
        if ((bad = check_tile_table(17, tiles, tile_seg, seg_tile, ws, ws_bytes, expect_row(two_d), sizeof(T)))) return bad;
    }
    return with_even_two_d<6>(two_d, -101, [&](auto D) {
        constexpr int D2 = decltype(D)::value;
        if (tiles > 0) {
            const int rc = launch(sparse_multi_expect_tile_kernel<T, D2>, tiles, 64, stream, N, S, B * S, q, ll(seg), ll(tile_seg),
                                  ll(seg_tile), w, c, y, pm, pc, g_mean ? 1 : 0, ws);
            if (rc) return rc;
        }
        return launch(expect_reduce_kernel<T, 1, D2>, B * S, 256, stream, tiles, S, tiles > 0 ? ll(seg_tile) : nullptr, ws, ve_sum,
                      g_mean, g_cov);
    });
}

template <typename T>
int run_multistage_ve(int64_t N, int nq, const double* nodes, const double* weights, const T* fmu, const T* fvar, const T* y, T* ve,
                      T* g_mu, T* g_var, void* stream) {
    Rule<T> q;
    Par<T> p;
    if (N < 0 || (N + 255) / 256 > int64_t(0x7fffffff)) return -1;
    const int bad = prepare<T>(0, 1, nullptr, nq, nodes, weights, false, q, p);  // -4 ... -6 there: arguments 2 ... 4 here
    if (bad) return bad + 2;
    if (N == 0) return 0;
    if (const int null = first_null(5, {fmu, fvar, y})) return null;
    if (!ve && !g_mu && !g_var) return 0;          // nothing asked for
    return launch(multistage_ve_kernel<T>, (N + 255) / 256, 256, stream, N, q, fmu, fvar, y, ve, g_mu, g_var);
}

// the sparse power-EP site update: the workspace row is the SVGP kernels' (expect_row), so is the workspace-size function
template <typename T>
int run_sparse_pep(int64_t B, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq, const double* nodes,
                   const double* weights, T alpha, T lr, const int64_t* seg, const T* w, const T* c, const T* y, const T* cm,
                   const T* cc, const T* seg_const, int64_t tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* ws,
                   size_t ws_bytes, T* nat1, T* nat2, T* log_norm, T* led_sum, T* fmu, T* fvar, T* led, void* stream) {
    Rule<T> q;
    Par<T> p;
    int bad = prepare_segmented<T>(B, N, S, two_d, lik, params, nq, nodes, weights, q, p, true);
    if (bad) return bad;
    if (!(alpha > T(0)) || !(alpha <= T(1))) return -10;
    if (!(lr >= T(0)) || !(lr <= T(1))) return -11;
    if ((bad = check_tile_count(19, N, tiles))) return bad;
    if (nat1 || nat2 || log_norm) {                // all three, or none (evaluation only)
        if ((bad = first_null(24, {nat1, nat2, log_norm}))) return bad;
    }
    if (B == 0 || (!nat1 && !led_sum && !fmu && !fvar && !led)) return 0;      // nothing asked for
    if (tiles > 0) {
        if ((bad = first_null(12, {seg, w, c, y, cm, cc}))) return bad;
        if ((bad = check_tile_table(19, tiles, tile_seg, seg_tile, ws, ws_bytes, expect_row(two_d), sizeof(T)))) return bad;
    }
    return with_even_two_d<2>(two_d, -100, [&](auto D) {
        constexpr int D2 = decltype(D)::value;
        if (tiles > 0) {
            const int rc = with_lik(lik, [&](auto L) {
                return launch(sparse_pep_tile_kernel<T, decltype(L)::value, D2>, tiles, 64, stream, N, S, B * S, q, p, alpha, ll(seg),
                              ll(tile_seg), ll(seg_tile), w, c, y, cm, cc, nat1 ? 1 : 0, ws, fmu, fvar, led);
            });
            if (rc) return rc;
        }
        if (!nat1 && !led_sum) return 0;           // per-point outputs only
        return launch(sparse_pep_reduce_kernel<T, D2>, B * S, 256, stream, tiles, tiles > 0 ? ll(seg_tile) : nullptr, ws, seg_const,
                      alpha, lr, nat1, nat2, log_norm, led_sum);
    });
}

// the log importance weights' data term: the workspace row of a (tile, sample) is the 2d column sums and the value sum
constexpr size_t iw_row(int two_d) { return size_t(two_d) + 1; }

template <typename T>
int run_iw(int64_t B, int64_t N, int64_t S, int two_d, int64_t K, int lik, const double* params, const int64_t* seg, const T* w,
           const T* y, const T* h, const T* states, const T* u_post, int64_t tiles, const int64_t* tile_seg, const int64_t* seg_tile,
           void* ws, size_t ws_bytes, T* log_lik, T* g_u, void* stream) {
    int bad = check_segmentation(B, N, S);
    if (bad) return bad;
    if (two_d < 2 || two_d > 18 || (two_d & 1)) return -100;
    if (K < 0 || K > int64_t(0x7fffffff)) return -5;
    Rule<T> q;                         // no quadrature: the density is evaluated point-wise (a one-node rule satisfies prepare)
    Par<T> p;
    const double node = 0.0, weight = 1.0;
    bad = prepare<T>(0, lik, params, 1, &node, &weight, false, q, p);          // -2, -3 there: arguments 6, 7 here
    if (bad) return bad - 4;
    const int64_t chunks = (K + IW_CHUNK - 1) / IW_CHUNK;
    if ((bad = check_tile_count(14, N, tiles, chunks))) return bad;            // (a block per tile and chunk of samples)
    if (g_u && !u_post) return -20;
    if (B == 0 || K == 0 || (!log_lik && !g_u)) return 0;      // nothing asked for
    if (tiles > 0) {
        if (!seg) return -8;
        if (u_post && !w) return -9;
        if ((bad = first_null(10, {y, h, states}))) return bad;
        if ((bad = check_tile_table(14, tiles, tile_seg, seg_tile, ws, ws_bytes, size_t(K) * iw_row(two_d), sizeof(T)))) return bad;
    }
    return with_even_two_d<2>(two_d, -100, [&](auto D) {
        constexpr int D2 = decltype(D)::value;
        if (tiles > 0) {
            const int rc = with_lik(lik, [&](auto L) {
                return launch(iw_tile_kernel<T, decltype(L)::value, D2>, tiles * chunks, 64, stream, N, S, B * S, B, K, chunks, p,
                              ll(seg), ll(tile_seg), ll(seg_tile), w, y, h, states, u_post, g_u ? 1 : 0, ws);
            });
            if (rc) return rc;
        }
        return launch(iw_reduce_kernel<T, D2>, B * S, 256, stream, tiles, S, B, K, tiles > 0 ? ll(seg_tile) : nullptr, ws, log_lik,
                      g_u);
    });
}

// the same for the state dimension of the dense kernels: 1 ... DENSE_MAX_D, -100 for any other
template <typename F>
int with_dense_d(int d, F&& f) {
    switch (d) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 9: return f(std::integral_constant<int, 9>{});
        case 10: return f(std::integral_constant<int, 10>{});
        case 11: return f(std::integral_constant<int, 11>{});
        case 12: return f(std::integral_constant<int, 12>{});
        default: return -100;
    }
}

// the leading argument checks of the two dense entry points; on success *tiles = ceil(N / 64)
inline int prepare_dense(int64_t B, int64_t N, int d, int64_t* tiles) {
    if (B < 0) return -1;
    if (N < 0) return -2;
    if (d < 1 || d > DENSE_MAX_D) return -100;
    *tiles = (N + 63) / 64;
    if (B > 0 && *tiles > int64_t(0x7fffffff) / B) return -2;      // one block per tile
    return 0;
}

template <typename T>
int run_dense_expect(int64_t B, int64_t N, int d, int lik, const double* params, int nq, const double* nodes, const double* weights,
                     const T* h, const T* means, const T* covs, const T* y, void* ws, size_t ws_bytes, T* ve_sum, T* g_mu, T* g_var,
                     void* stream) {
    Rule<T> q;
    Par<T> p;
    int64_t tiles = 0;
    int bad = prepare_dense(B, N, d, &tiles);
    if (bad) return bad;
    if ((bad = prepare<T>(0, lik, params, nq, nodes, weights, false, q, p))) return bad - 2;      // -2 ... -6 there: 4 ... 8 here
    if (!g_mu && g_var) return -16;
    if (g_mu && !g_var) return -17;
    if (B == 0 || (!ve_sum && !g_mu)) return 0;        // nothing asked for
    if (tiles > 0) {
        if ((bad = first_null(9, {h, means, covs, y}))) return bad;
        if (ve_sum && !ws) return -13;
        if (ve_sum && ws_bytes < size_t(B) * size_t(tiles) * sizeof(T)) return -14;
        const int rc = with_dense_d(d, [&](auto D) {
            return with_lik(lik, [&](auto L) {
                return launch(dense_expect_tile_kernel<T, decltype(L)::value, decltype(D)::value>, B * tiles, 64, stream, N, tiles, q,
                              p, h, means, covs, y, ve_sum ? ws : nullptr, g_mu, g_var);
            });
        });
        if (rc) return rc;
    }
    if (!ve_sum) return 0;
    return launch(dense_expect_reduce_kernel<T>, (B + 63) / 64, 64, stream, B, tiles, ws, ve_sum);
}

template <typename T>
int run_dense_adjoint(int64_t B, int64_t N, int d, const T* h, const T* g_mu, const T* g_var, const T* weight, T* g_means, T* g_covs,
                      void* stream) {
    int64_t tiles = 0;
    int bad = prepare_dense(B, N, d, &tiles);
    if (bad) return bad;
    if (B == 0 || N == 0 || (!g_means && !g_covs)) return 0;       // nothing asked for
    if (N > (int64_t(1) << 62) / (int64_t(d) * d + d) / B) return -2;
    if (!h) return -4;
    if (g_means && !g_mu) return -5;
    if (g_covs && !g_var) return -6;
    const int64_t n_all = B * N * ((g_covs ? int64_t(d) * d : 0) + (g_means ? d : 0));
    const int64_t blocks = (n_all + 255) / 256;
    constexpr int64_t MAX_BLOCKS = 256 * 64;           // beyond that a lane loops: 64 blocks on each of the 256 CUs
    return with_dense_d(d, [&](auto D) {
        return launch(dense_adjoint_kernel<T, decltype(D)::value>, blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS, 256, stream, B * N, N, h,
                      g_mu, g_var, weight, g_means, g_covs);
    });
}

}  // namespace

extern "C" {

size_t mf_lik_dense_expectations_workspace_bytes(int64_t B, int64_t N, int elem_size) {
    if (B <= 0 || N <= 0 || elem_size < 1) return 0;
    return size_t(B) * size_t((N + 63) / 64) * size_t(elem_size);
}
int mf_lik_dense_expectations_f64(int64_t B, int64_t N, int d, int lik, const double* params, int nq, const double* nodes,
                                  const double* weights, const double* h, const double* means, const double* covs, const double* y,
                                  void* workspace, size_t workspace_bytes, double* ve_sum, double* g_mu, double* g_var,
                                  void* stream) {
    return run_dense_expect<double>(B, N, d, lik, params, nq, nodes, weights, h, means, covs, y, workspace, workspace_bytes, ve_sum,
                                    g_mu, g_var, stream);
}
int mf_lik_dense_expectations_f32(int64_t B, int64_t N, int d, int lik, const double* params, int nq, const double* nodes,
                                  const double* weights, const float* h, const float* means, const float* covs, const float* y,
                                  void* workspace, size_t workspace_bytes, float* ve_sum, float* g_mu, float* g_var, void* stream) {
    return run_dense_expect<float>(B, N, d, lik, params, nq, nodes, weights, h, means, covs, y, workspace, workspace_bytes, ve_sum,
                                   g_mu, g_var, stream);
}
int mf_lik_dense_expectations_adjoint_f64(int64_t B, int64_t N, int d, const double* h, const double* g_mu, const double* g_var,
                                          const double* weight, double* g_means, double* g_covs, void* stream) {
    return run_dense_adjoint<double>(B, N, d, h, g_mu, g_var, weight, g_means, g_covs, stream);
}
int mf_lik_dense_expectations_adjoint_f32(int64_t B, int64_t N, int d, const float* h, const float* g_mu, const float* g_var,
                                          const float* weight, float* g_means, float* g_covs, void* stream) {
    return run_dense_adjoint<float>(B, N, d, h, g_mu, g_var, weight, g_means, g_covs, stream);
}

size_t mf_lik_iw_log_weights_workspace_bytes(int64_t num_tiles, int64_t K, int two_d, int elem_size) {
    if (num_tiles <= 0 || K <= 0 || two_d < 2 || two_d > 18 || (two_d & 1) || elem_size < 1) return 0;
    return size_t(num_tiles) * size_t(K) * iw_row(two_d) * size_t(elem_size);
}
int mf_lik_iw_log_weights_f64(int64_t B, int64_t N, int64_t S, int two_d, int64_t K, int lik, const double* params,
                              const int64_t* seg_offsets, const double* w, const double* y, const double* h, const double* states,
                              const double* u_post, int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile,
                              void* workspace, size_t workspace_bytes, double* log_lik, double* g_u, void* stream) {
    return run_iw<double>(B, N, S, two_d, K, lik, params, seg_offsets, w, y, h, states, u_post, num_tiles, tile_seg, seg_tile,
                          workspace, workspace_bytes, log_lik, g_u, stream);
}
int mf_lik_iw_log_weights_f32(int64_t B, int64_t N, int64_t S, int two_d, int64_t K, int lik, const double* params,
                              const int64_t* seg_offsets, const float* w, const float* y, const float* h, const float* states,
                              const float* u_post, int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile,
                              void* workspace, size_t workspace_bytes, float* log_lik, float* g_u, void* stream) {
    return run_iw<float>(B, N, S, two_d, K, lik, params, seg_offsets, w, y, h, states, u_post, num_tiles, tile_seg, seg_tile,
                         workspace, workspace_bytes, log_lik, g_u, stream);
}

size_t mf_lik_sparse_expectations_workspace_bytes(int64_t num_tiles, int two_d, int elem_size) {
    if (num_tiles <= 0 || two_d < 2 || two_d > 18 || (two_d & 1) || elem_size < 1) return 0;
    return size_t(num_tiles) * expect_row(two_d) * size_t(elem_size);
}
int mf_lik_sparse_expectations_f64(int64_t B, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq,
                                   const double* nodes, const double* weights, const int64_t* seg_offsets, const double* w,
                                   const double* c, const double* y, const double* pair_mean, const double* pair_cov,
                                   int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* workspace,
                                   size_t workspace_bytes, double* ve_sum, double* g_mean, double* g_cov, void* stream) {
    return run_expect<double>(B, N, S, two_d, lik, params, nq, nodes, weights, seg_offsets, w, c, y, pair_mean, pair_cov, num_tiles,
                              tile_seg, seg_tile, workspace, workspace_bytes, ve_sum, g_mean, g_cov, stream);
}
int mf_lik_sparse_expectations_f32(int64_t B, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq,
                                   const double* nodes, const double* weights, const int64_t* seg_offsets, const float* w,
                                   const float* c, const float* y, const float* pair_mean, const float* pair_cov,
                                   int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* workspace,
                                   size_t workspace_bytes, float* ve_sum, float* g_mean, float* g_cov, void* stream) {
    return run_expect<float>(B, N, S, two_d, lik, params, nq, nodes, weights, seg_offsets, w, c, y, pair_mean, pair_cov, num_tiles,
                             tile_seg, seg_tile, workspace, workspace_bytes, ve_sum, g_mean, g_cov, stream);
}

size_t mf_lik_sparse_multi_expectations_workspace_bytes(int64_t num_tiles, int two_d, int elem_size) {
    return mf_lik_sparse_expectations_workspace_bytes(num_tiles, two_d, elem_size);
}
int mf_lik_sparse_multi_expectations_f64(int64_t B, int64_t N, int64_t S, int two_d, int latent_dim, int lik, const double* params,
                                         int nq, const double* nodes, const double* weights, const int64_t* seg, const double* w,
                                         const double* c, const double* y, const double* pm, const double* pc, int64_t tiles,
                                         const int64_t* tile_seg, const int64_t* seg_tile, void* ws, size_t ws_bytes, double* ve_sum,
                                         double* g_mean, double* g_cov, void* stream) {
    (void)params;
    return run_multi_expect<double>(B, N, S, two_d, latent_dim, lik, nq, nodes, weights, seg, w, c, y, pm, pc, tiles, tile_seg,
                                    seg_tile, ws, ws_bytes, ve_sum, g_mean, g_cov, stream);
}
int mf_lik_sparse_multi_expectations_f32(int64_t B, int64_t N, int64_t S, int two_d, int latent_dim, int lik, const double* params,
                                         int nq, const double* nodes, const double* weights, const int64_t* seg, const float* w,
                                         const float* c, const float* y, const float* pm, const float* pc, int64_t tiles,
                                         const int64_t* tile_seg, const int64_t* seg_tile, void* ws, size_t ws_bytes, float* ve_sum,
                                         float* g_mean, float* g_cov, void* stream) {
    (void)params;
    return run_multi_expect<float>(B, N, S, two_d, latent_dim, lik, nq, nodes, weights, seg, w, c, y, pm, pc, tiles, tile_seg,
                                   seg_tile, ws, ws_bytes, ve_sum, g_mean, g_cov, stream);
}

int mf_lik_multistage_variational_expectations_f64(int64_t N, int nq, const double* nodes, const double* weights, const double* fmu,
                                                   const double* fvar, const double* y, double* ve, double* g_mu, double* g_var,
                                                   void* stream) {
    return run_multistage_ve<double>(N, nq, nodes, weights, fmu, fvar, y, ve, g_mu, g_var, stream);
}
int mf_lik_multistage_variational_expectations_f32(int64_t N, int nq, const double* nodes, const double* weights, const float* fmu,
                                                   const float* fvar, const float* y, float* ve, float* g_mu, float* g_var,
                                                   void* stream) {
    return run_multistage_ve<float>(N, nq, nodes, weights, fmu, fvar, y, ve, g_mu, g_var, stream);
}

int mf_lik_variational_expectations_f64(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                                        const double* fmu, const double* fvar, const double* y, double* ve, double* g_mu,
                                        double* g_var, void* stream) {
    return run_ve<double>(N, lik, params, nq, nodes, weights, fmu, fvar, y, ve, g_mu, g_var, stream);
}
int mf_lik_variational_expectations_f32(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                                        const float* fmu, const float* fvar, const float* y, float* ve, float* g_mu, float* g_var,
                                        void* stream) {
    return run_ve<float>(N, lik, params, nq, nodes, weights, fmu, fvar, y, ve, g_mu, g_var, stream);
}
int mf_lik_cvi_site_update_f64(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                               const double* fmu, const double* fvar, const double* y, double lr, double* nat1, double* nat2,
                               double* ve, void* stream) {
    return run_site<double>(N, lik, params, nq, nodes, weights, fmu, fvar, y, lr, nat1, nat2, ve, stream);
}
int mf_lik_cvi_site_update_f32(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                               const float* fmu, const float* fvar, const float* y, float lr, float* nat1, float* nat2, float* ve,
                               void* stream) {
    return run_site<float>(N, lik, params, nq, nodes, weights, fmu, fvar, y, lr, nat1, nat2, ve, stream);
}
int mf_lik_predict_log_density_f64(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                                   const double* fmu, const double* fvar, const double* y, double* out, void* stream) {
    return run_pld<double>(N, lik, params, nq, nodes, weights, fmu, fvar, y, out, stream);
}
int mf_lik_predict_log_density_f32(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                                   const float* fmu, const float* fvar, const float* y, float* out, void* stream) {
    return run_pld<float>(N, lik, params, nq, nodes, weights, fmu, fvar, y, out, stream);
}
int mf_lik_log_expected_density_f64(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                                    double alpha, const double* fmu, const double* fvar, const double* y, double* led, double* g1,
                                    double* g2, void* stream) {
    return run_led<double>(N, lik, params, nq, nodes, weights, alpha, fmu, fvar, y, led, g1, g2, stream);
}
int mf_lik_log_expected_density_f32(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                                    float alpha, const float* fmu, const float* fvar, const float* y, float* led, float* g1, float* g2,
                                    void* stream) {
    return run_led<float>(N, lik, params, nq, nodes, weights, alpha, fmu, fvar, y, led, g1, g2, stream);
}
int mf_lik_pep_site_update_f64(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                               double alpha, double lr, const double* fmu, const double* fvar, const double* y,
                               const unsigned char* update, double* nat1, double* nat2, double* log_norm, double* cav_mu,
                               double* cav_var, void* stream) {
    return run_pep<double>(N, lik, params, nq, nodes, weights, alpha, lr, fmu, fvar, y, update, nat1, nat2, log_norm, cav_mu, cav_var,
                           stream);
}
int mf_lik_pep_site_update_f32(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights,
                               float alpha, float lr, const float* fmu, const float* fvar, const float* y, const unsigned char* update,
                               float* nat1, float* nat2, float* log_norm, float* cav_mu, float* cav_var, void* stream) {
    return run_pep<float>(N, lik, params, nq, nodes, weights, alpha, lr, fmu, fvar, y, update, nat1, nat2, log_norm, cav_mu, cav_var,
                          stream);
}
int mf_lik_sparse_cvi_site_update_f64(int64_t B, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq,
                                      const double* nodes, const double* weights, const int64_t* seg_offsets, const double* w,
                                      const double* c, const double* y, const double* pair_mean, const double* pair_cov, double lr,
                                      double* nat1, double* nat2, double* fmu, double* fvar, double* ve, void* stream) {
    return run_sparse<double>(B, N, S, two_d, lik, params, nq, nodes, weights, seg_offsets, w, c, y, pair_mean, pair_cov, lr, nat1,
                              nat2, fmu, fvar, ve, stream);
}
int mf_lik_sparse_cvi_site_update_f32(int64_t B, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq,
                                      const double* nodes, const double* weights, const int64_t* seg_offsets, const float* w,
                                      const float* c, const float* y, const float* pair_mean, const float* pair_cov, float lr,
                                      float* nat1, float* nat2, float* fmu, float* fvar, float* ve, void* stream) {
    return run_sparse<float>(B, N, S, two_d, lik, params, nq, nodes, weights, seg_offsets, w, c, y, pair_mean, pair_cov, lr, nat1,
                             nat2, fmu, fvar, ve, stream);
}

int mf_lik_sparse_pep_site_update_f64(int64_t B, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq,
                                      const double* nodes, const double* weights, double alpha, double lr,
                                      const int64_t* seg_offsets, const double* w, const double* c, const double* y,
                                      const double* cav_mean, const double* cav_cov, const double* seg_const, int64_t num_tiles,
                                      const int64_t* tile_seg, const int64_t* seg_tile, void* workspace, size_t workspace_bytes,
                                      double* nat1, double* nat2, double* log_norm, double* led_sum, double* fmu, double* fvar,
                                      double* led, void* stream) {
    return run_sparse_pep<double>(B, N, S, two_d, lik, params, nq, nodes, weights, alpha, lr, seg_offsets, w, c, y, cav_mean, cav_cov,
                                  seg_const, num_tiles, tile_seg, seg_tile, workspace, workspace_bytes, nat1, nat2, log_norm, led_sum,
                                  fmu, fvar, led, stream);
}
int mf_lik_sparse_pep_site_update_f32(int64_t B, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq,
                                      const double* nodes, const double* weights, float alpha, float lr,
                                      const int64_t* seg_offsets, const float* w, const float* c, const float* y,
                                      const float* cav_mean, const float* cav_cov, const float* seg_const, int64_t num_tiles,
                                      const int64_t* tile_seg, const int64_t* seg_tile, void* workspace, size_t workspace_bytes,
                                      float* nat1, float* nat2, float* log_norm, float* led_sum, float* fmu, float* fvar,
                                      float* led, void* stream) {
    return run_sparse_pep<float>(B, N, S, two_d, lik, params, nq, nodes, weights, alpha, lr, seg_offsets, w, c, y, cav_mean, cav_cov,
                                 seg_const, num_tiles, tile_seg, seg_tile, workspace, workspace_bytes, nat1, nat2, log_norm, led_sum,
                                 fmu, fvar, led, stream);
}

}  // extern "C"
