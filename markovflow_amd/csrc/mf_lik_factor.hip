// The data term of the SVGP ELBO under a FactorAnalysis emission (markovflow/kernels/sde_kernel.py:881-941 under
// markovflow/models/sparse_variational.py:149-192): P observed series, each with a scalar likelihood, mixed from L latent processes,
//   f_k = W_k g_k,   g_k = H_inner x_k,   W_k = A(t_k) B   [P, L].
// Per point k of pair s, with wg_k [L, 2d] = H_inner P_k and Cg_k [L, L] = H_inner T_k H_inner^T (neither depends on B):
//   mu_g = wg m_s                    Sig_g = Cg + wg S_s wg^T                       (L and L x L: L projections, not P)
//   mu_p = W_p . mu_g                s2_p  = W_p Sig_g W_p^T                        p = 0 .. P - 1
//   (ve_p, gm_p, gv_p) = expectations<T, LIK>(mu_p, s2_p, y_kp)                     (mf_lik_math.hpp, unchanged)
//   a = W^T gm   G = W^T diag(gv) W                                                 (L and L x L, G symmetric)
//   ve_sum[s] = sum_k sum_p ve_p     g_mean[s] = sum_k wg^T a     g_cov[s] = sum_k wg^T G wg
//   g_w[k]    = gm (x) mu_g + 2 diag(gv) W Sig_g                                    ([P, L] per point: the adjoint onto W_k)
// Two passes, tile-parallel, as mf_lik_sparse_multi_expectations_* (mf_lik.hip): the tile table and its locator, the tile of 64 points
// per wavefront, the staging of wg, the workspace row and pass 2 at K = 1 (all in mf_lik_tile.hpp) are the siblings'.
// New is pass 1:
//   phase 1, a lane per point.  The point's L rows of wg travel through LDS as ONE row of L 2d + 1 elements (odd: the lanes' rows
//            start on distinct banks) into registers.  The projection is the rolled walk over the rows i of S_s:
//            acc_l = sum_c S_ic wg_lc (c ascending),  Sig_g[l][l'] += wg_l'i acc_l for l' <= l,  mu_g[l] += wg_li m_i,
//            with Sig_g started from the LOWER triangle of Cg (global memory; Cg is symmetric, its upper triangle is not read) and
//            mirrored at the end.
//            The outputs are walked in chunks of FACTOR_CHUNK = 4: a chunk's rows of W and its y are staged through LDS (a row of
//            4 (L + 1) + 1 elements per point: 4 L of W, 4 of y, one of padding - odd again), so the global loads are runs of 4 L
//            and 4 contiguous elements per point and the LDS footprint does not grow with P.  Per output p, ascending:
//            t = Sig_g W_p,  mu_p = W_p . mu_g,  s2_p = W_p . t,  the expectation;  ve += ve_p,  a_l += gm W_pl,
//            G[l][l'] += (gv W_pl) W_pl' (l' <= l);  when g_w is asked for, row p of it replaces W_p in the LDS slot and the chunk is
//            stored with the same contiguous runs.  Four is the largest chunk with which the L = 4, 2d = 18 float64 kernel stays
//            below 64 KB of static LDS (58544 B); a larger P only makes the loop longer.
//            The point leaves G (L (L + 1) / 2 rows of lg), a (L rows) and ve (one row) in LDS.
//   phase 2, a lane per accumulator entry.  The points in ascending order; within a point the pairs (l, l' <= l) in the order
//            (0,0), (1,0), (1,1), (2,0), ... :  g_cov (i, j) += G_ll (wg_lj wg_li)  or, l' < l,  G_ll' (wg_li wg_l'j + wg_l'i wg_lj);
//            then the latents ascending:  g_mean i += a_l wg_li;  then ve_sum += ve.  L (L + 1) / 2 rank-one terms per point, not P.
// Value only (g_mean and g_cov NULL): phase 2 adds ve alone, the same numbers in the same order.  No floating-point atomics.
// An output with s2_p <= 0 or NaN gets ve = gm = gv = NaN: the three sums of its segment and row p of the point's g_w are NaN.
// Instantiated: L in 2, 3, 4 and 2d even in 2 L ... 18, the four likelihoods, both dtypes; no instantiation uses scratch (compiler
// remarks: DESIGN.md 4.23), nothing was cut.  1 <= P <= FACTOR_MAX_OUTPUTS = 1024.
#include "../../include/markovflow_amd.h"

#include "mf_lik_tile.hpp"

namespace {

constexpr int FACTOR_CHUNK = 4;                // outputs per chunk of phase 1
constexpr int64_t FACTOR_MAX_OUTPUTS = 1024;   // P above it: -101

template <typename T, int LIK, int L, int D2>
__global__ void __launch_bounds__(64) sparse_factor_expect_tile_kernel(long N, int S, long BS, int P, Rule<T> q, Par<T> p,
                                                                       const long long* __restrict__ seg,
                                                                       const long long* __restrict__ tile_seg,
                                                                       const long long* __restrict__ seg_tile,
                                                                       const T* __restrict__ wg, const T* __restrict__ cg,
                                                                       const T* __restrict__ mix, const T* __restrict__ yobs,
                                                                       const T* __restrict__ pair_mean, const T* __restrict__ pair_cov,
                                                                       int grads, T* __restrict__ gw, T* __restrict__ ws) {
    constexpr int C = FACTOR_CHUNK, W = L * D2 + 1, CW = C * (L + 1) + 1, TL = L * (L + 1) / 2, NG = TL + L + 1;
    constexpr int TRI = D2 * (D2 + 1) / 2, E = expect_entries(1, D2), R = (E + 63) / 64;
    __shared__ T lw[64 * W];
    __shared__ T ls[D2 * D2];
    __shared__ T lm[D2];
    __shared__ T lc[64 * CW];          // a chunk of outputs: per point C rows of W, C values of y
    __shared__ T lg[NG * 64];          // G of the tile's points (TL rows), then a (L rows), then ve
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
        const long id0 = b * N + k0;                                 // the tile's first point
        for (int idx = lane; idx < D2 * D2; idx += 64) ls[idx] = pair_cov[bs * (D2 * D2) + idx];
        if (lane < D2) lm[lane] = pair_mean[bs * D2 + lane];
        stage_tile<T, L * D2>(lane, npts, wg + id0 * (L * D2), lw);  // npts rows of L 2d elements
        __syncthreads();
        T mug[L], sig[L][L], a[L], g[TL], ve_pt = T(0);
#pragma unroll
        for (int l = 0; l < L; ++l) {
            mug[l] = a[l] = T(0);
#pragma unroll
            for (int m = 0; m < L; ++m) sig[l][m] = T(0);
        }
#pragma unroll
        for (int e = 0; e < TL; ++e) g[e] = T(0);
        if (lane < npts) {
            T wr[L][D2];
#pragma unroll
            for (int l = 0; l < L; ++l) {
#pragma unroll
                for (int i = 0; i < D2; ++i) wr[l][i] = lw[lane * W + l * D2 + i];
#pragma unroll
                for (int m = 0; m <= l; ++m) sig[l][m] = cg[(id0 + lane) * (L * L) + l * L + m];
            }
#pragma unroll 1
            for (int i = 0; i < D2; ++i) {         // (rolled: unrolled, the compiler keeps all of S_s in registers and spills)
                T acc[L], wi[L];
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
                for (int l = 0; l < L; ++l) wi[l] = lw[lane * W + l * D2 + i];
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    mug[l] += wi[l] * mi;
#pragma unroll
                    for (int m = 0; m <= l; ++m) sig[l][m] += wi[m] * acc[l];
                }
            }
#pragma unroll
            for (int l = 0; l < L; ++l) {
#pragma unroll
                for (int m = 0; m < l; ++m) sig[m][l] = sig[l][m];
            }
        }
        for (int p0 = 0; p0 < P; p0 += C) {        // (P is a kernel argument: the trip count is the wavefront's)
            const int pc = P - p0 < C ? P - p0 : C;
            __syncthreads();                       // the previous chunk's store has read lc
            for (int idx = lane; idx < npts * pc * L; idx += 64) {
                const int k = idx / (pc * L), r = idx - k * (pc * L);
                lc[k * CW + r] = mix[((id0 + k) * P + p0) * L + r];
            }
            for (int idx = lane; idx < npts * pc; idx += 64) {
                const int k = idx / pc, r = idx - k * pc;
                lc[k * CW + C * L + r] = yobs[(id0 + k) * P + p0 + r];
            }
            __syncthreads();
            if (lane < npts) {
#pragma unroll 1
                for (int c = 0; c < pc; ++c) {
                    T wp[L], tv[L];
#pragma unroll
                    for (int l = 0; l < L; ++l) wp[l] = lc[lane * CW + c * L + l];
                    const T y = lc[lane * CW + C * L + c];
                    T mu = T(0), s2 = T(0);
#pragma unroll
                    for (int l = 0; l < L; ++l) {
                        tv[l] = T(0);
#pragma unroll
                        for (int m = 0; m < L; ++m) tv[l] += sig[l][m] * wp[m];
                        mu += wp[l] * mug[l];
                    }
#pragma unroll
                    for (int l = 0; l < L; ++l) s2 += wp[l] * tv[l];
                    T ve, gm, gv;
                    if (s2 > T(0)) {
                        expectations<T, LIK>(q, p, mu, s2, y, ve, gm, gv);
                    } else {                       // outside the domain: NaN in all three sums of this point's segment
                        ve = gm = gv = nan_of<T>();
                    }
                    ve_pt += ve;
                    int e = 0;
#pragma unroll
                    for (int l = 0; l < L; ++l) {
                        a[l] += gm * wp[l];
#pragma unroll
                        for (int m = 0; m <= l; ++m) g[e++] += (gv * wp[l]) * wp[m];
                    }
                    if (gw) {
#pragma unroll
                        for (int l = 0; l < L; ++l) lc[lane * CW + c * L + l] = gm * mug[l] + T(2) * gv * tv[l];
                    }
                }
            }
            if (gw) {
                __syncthreads();
                for (int idx = lane; idx < npts * pc * L; idx += 64) {
                    const int k = idx / (pc * L), r = idx - k * (pc * L);
                    gw[((id0 + k) * P + p0) * L + r] = lc[k * CW + r];
                }
            }
        }
        if (lane < npts) {
#pragma unroll
            for (int e = 0; e < TL; ++e) lg[e * 64 + lane] = g[e];
#pragma unroll
            for (int l = 0; l < L; ++l) lg[(TL + l) * 64 + lane] = a[l];
            lg[(TL + L) * 64 + lane] = ve_pt;
        }
        __syncthreads();
        if (grads) {
            for (int k = 0; k < npts; ++k) {
                int e = 0;
#pragma unroll
                for (int l = 0; l < L; ++l) {
#pragma unroll
                    for (int m = 0; m <= l; ++m) {
                        const T glm = lg[e * 64 + k];
                        ++e;
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            if (kind[r] == 0) {
                                const T wli = lw[k * W + l * D2 + ei[r]], wlj = lw[k * W + l * D2 + ej[r]];
                                if (m == l) {
                                    part[r] += (glm * wlj) * wli;
                                } else {
                                    part[r] += glm * (wli * lw[k * W + m * D2 + ej[r]] + lw[k * W + m * D2 + ei[r]] * wlj);
                                }
                            }
                        }
                    }
                }
#pragma unroll
                for (int l = 0; l < L; ++l) {
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (kind[r] == 1) part[r] += lg[(TL + l) * 64 + k] * lw[k * W + l * D2 + ei[r]];
                }
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (kind[r] == 2) part[r] += lg[(TL + L) * 64 + k];
            }
        } else if (lane == (E - 1) % 64) {         // value only: the one entry, with the bits it has beside the gradients
            for (int k = 0; k < npts; ++k) part[R - 1] += lg[(TL + L) * 64 + k];
        }
    }
    store_row<E>(ws + t * E, lane, part);
}

// (latent_dim, two_d) as compile-time constants: latent_dim in 2, 3, 4 and two_d even in 2 latent_dim ... 18; -101 for any other
template <typename F>
int with_factor_dims(int latent_dim, int two_d, F&& f) {
    auto at = [&](auto L) { return with_even_two_d<2 * decltype(L)::value>(two_d, -101, [&](auto D) { return f(L, D); }); };
    switch (latent_dim) {
        case 2: return at(std::integral_constant<int, 2>{});
        case 3: return at(std::integral_constant<int, 3>{});
        case 4: return at(std::integral_constant<int, 4>{});
        default: return -101;
    }
}

template <typename T>
int run_factor_expect(int64_t B, int64_t N, int64_t S, int two_d, int latent_dim, int64_t P, int lik, const double* params, int nq,
                      const double* nodes, const double* weights, const int64_t* seg, const T* wg, const T* cg, const T* mix,
                      const T* y, const T* pm, const T* pc, int64_t tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* ws,
                      size_t ws_bytes, T* ve_sum, T* g_mean, T* g_cov, T* g_w, void* stream) {
    Rule<T> q;
    Par<T> p;
    int bad = check_segmentation(B, N, S);
    if (bad) return bad;
    if (P < 1) return -6;
    if (latent_dim < 2 || latent_dim > 4 || two_d < 2 * latent_dim || two_d > 18 || (two_d & 1) || P > FACTOR_MAX_OUTPUTS) return -101;
    bad = prepare<T>(0, lik, params, nq, nodes, weights, false, q, p);           // -2 ... -6 there: arguments 7 ... 11 here
    if (bad) return bad - 5;
    if ((bad = check_tile_count(19, N, tiles))) return bad;
    if (!g_mean && g_cov) return -25;
    if (g_mean && !g_cov) return -26;
    if (B == 0 || (!ve_sum && !g_mean && !g_w)) return 0;      // nothing asked for
    if (tiles > 0) {
        if ((bad = first_null(12, {seg, wg, cg, mix, y, pm, pc}))) return bad;
        if ((bad = check_tile_table(19, tiles, tile_seg, seg_tile, ws, ws_bytes, expect_row(two_d), sizeof(T)))) return bad;
    }
    return with_factor_dims(latent_dim, two_d, [&](auto LL, auto D) {
        constexpr int L = decltype(LL)::value, D2 = decltype(D)::value;
        if (tiles > 0) {
            const int rc = with_lik(lik, [&](auto K) {
                return launch(sparse_factor_expect_tile_kernel<T, decltype(K)::value, L, D2>, tiles, 64, stream, N, S, B * S, P, q, p,
                              ll(seg), ll(tile_seg), ll(seg_tile), wg, cg, mix, y, pm, pc, g_mean ? 1 : 0, g_w, ws);
            });
            if (rc) return rc;
        }
        return launch(expect_reduce_kernel<T, 1, D2>, B * S, 256, stream, tiles, S, tiles > 0 ? ll(seg_tile) : nullptr, ws, ve_sum,
                      g_mean, g_cov);
    });
}

}  // namespace

extern "C" {

size_t mf_lik_sparse_factor_expectations_workspace_bytes(int64_t num_tiles, int two_d, int elem_size) {
    return mf_lik_sparse_expectations_workspace_bytes(num_tiles, two_d, elem_size);
}
int mf_lik_sparse_factor_expectations_f64(int64_t B, int64_t N, int64_t S, int two_d, int latent_dim, int64_t num_outputs, int lik,
                                          const double* params, int nq, const double* nodes, const double* weights,
                                          const int64_t* seg, const double* wg, const double* cg, const double* mix, const double* y,
                                          const double* pm, const double* pc, int64_t tiles, const int64_t* tile_seg,
                                          const int64_t* seg_tile, void* ws, size_t ws_bytes, double* ve_sum, double* g_mean,
                                          double* g_cov, double* g_w, void* stream) {
    return run_factor_expect<double>(B, N, S, two_d, latent_dim, num_outputs, lik, params, nq, nodes, weights, seg, wg, cg, mix, y,
                                     pm, pc, tiles, tile_seg, seg_tile, ws, ws_bytes, ve_sum, g_mean, g_cov, g_w, stream);
}
int mf_lik_sparse_factor_expectations_f32(int64_t B, int64_t N, int64_t S, int two_d, int latent_dim, int64_t num_outputs, int lik,
                                          const double* params, int nq, const double* nodes, const double* weights,
                                          const int64_t* seg, const float* wg, const float* cg, const float* mix, const float* y,
                                          const float* pm, const float* pc, int64_t tiles, const int64_t* tile_seg,
                                          const int64_t* seg_tile, void* ws, size_t ws_bytes, float* ve_sum, float* g_mean,
                                          float* g_cov, float* g_w, void* stream) {
    return run_factor_expect<float>(B, N, S, two_d, latent_dim, num_outputs, lik, params, nq, nodes, weights, seg, wg, cg, mix, y, pm,
                                    pc, tiles, tile_seg, seg_tile, ws, ws_bytes, ve_sum, g_mean, g_cov, g_w, stream);
}

}  // extern "C"
