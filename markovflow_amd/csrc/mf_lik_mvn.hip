// The data term of the SVGP ELBO under a MultivariateGaussian likelihood (markovflow/likelihoods/multivariate_gaussian.py under
// markovflow/models/sparse_variational.py:149-192): P observed series per point with noise that is correlated ACROSS the series,
//   p(y_k | f_k) = N(y_k; f_k, Sigma),   Sigma = L L^T,   Lam = Sigma^-1   [P, P], symmetric, ONE matrix for the whole launch.
// The term is closed-form (no quadrature) and not a sum over the outputs: it needs the full P x P marginal of f_k.  Per point k of
// pair s, with w_k [P, 2d] = H P_k and the FULL C_k [P, P] = H T_k H^T (symmetric: the lower triangle is read):
//   mu = w m_s          F = C + w S_s w^T          r = y - mu          v = Lam r          quad_k = r . v + <Lam, F>
//   quad_sum[s] = sum_k quad_k                     E_q log p = -(n_s (P log 2 pi + log det Sigma) + quad_sum[s]) / 2  (the caller's)
//   g_mean[s]   = sum_k w^T v                      the adjoint of -quad_sum / 2 onto m_s
//   g_cov[s]    = -1/2 sum_k w^T Lam w             ... onto S_s (symmetric)
//   m_sum[s]    = sum_k (r r^T + F)   [P, P]       -m_sum / 2 is the adjoint onto Lam: the likelihood's parameter trains in this launch
// Two passes, tile-parallel, as mf_lik_sparse_factor_expectations_* (mf_lik_factor.hip): the tile table and its locator, the tile of
// 64 points per wavefront, the staging of w and the store of a workspace row are mf_lik_tile.hpp's.  New is
//   pass 1, phase 1, a lane per point.  The point's P rows of w travel through LDS as ONE row of P 2d + 1 elements (odd: the lanes'
//            rows start on distinct banks) into registers.  The projection is the rolled walk over the rows i of S_s:
//            acc_p = sum_c S_ic w_pc (c ascending),  F[p][q] += w_qi acc_p for q <= p,  mu[p] += w_pi m_i,  with F started from the
//            LOWER triangle of C.  Lam is uniform over the launch: its lower triangle, P (P + 1) / 2 values, is read ONCE from
//            global memory into (scalar) registers, never from LDS per point.  Then, in this order:
//            r_p = y_p - mu_p;  v_p = sum_q Lam_pq r_q (q ascending);  quad = sum_p r_p v_p (p ascending), then over the pairs
//            (p, q <= p) in the order (0,0), (1,0), (1,1), ... :  quad += Lam_pp F_pp  or, q < p,  (2 Lam_pq) F_pq.
//            The point leaves in LDS, a row of 64 per quantity: v (P rows), r r^T + F (P (P + 1) / 2 rows), quad (one row).
//   pass 1, phase 2, a lane per accumulator entry: the triangle of g_cov, then g_mean, then the triangle of m_sum, then quad - a
//            workspace row of 2d (2d + 1) / 2 + 2d + P (P + 1) / 2 + 1 values.  The points in ascending order; within a point the
//            pairs (p, q <= p) in the order above:  g_cov (i, j) += (-Lam_pp / 2) (w_pi w_pj)  or, q < p,
//            (-Lam_pq / 2) (w_pi w_qj + w_qi w_pj);  then the outputs ascending:  g_mean i += v_p w_pi;  the entry of m_sum and quad
//            are plain adds from LDS.  Unlike the factor kernel's G, the pair coefficients are the SAME for every point: phase 2 reads
//            only w from LDS.
//   pass 2, one block per (series, segment), a lane per entry: the segment's rows are added in ascending tile order and both
//            triangles mirrored.  An empty segment writes exact zeros.  (Its own kernel: expect_reduce_kernel's row layout is its
//            siblings'.)
// Value only (g_mean, g_cov and m_sum NULL): phase 2 adds quad alone, the same numbers in the same order.  No floating-point atomics.
// Instantiated: P in 2, 3, 4 and 2d even in 2 ... 18, both dtypes: 54 kernels; none uses scratch (compiler remarks: DESIGN.md 4.26).
// NOT built: Lam w per point in a second LDS tile (it does not fit 64 KB at P = 4, 2d = 18 in float64) and the g_cov reduction on
// MFMA (nobody has measured whether phase 2 is the bottleneck).
#include "../../include/markovflow_amd.h"

#include "mf_lik_tile.hpp"

namespace {

constexpr int mvn_tri(int p) { return p * (p + 1) / 2; }
// a workspace row: the triangle of g_cov, g_mean, the triangle of m_sum, quad
constexpr int mvn_entries(int p, int d2) { return mvn_tri(d2) + d2 + mvn_tri(p) + 1; }

template <typename T, int P, int D2>
__global__ void __launch_bounds__(64) sparse_mvn_expect_tile_kernel(long N, int S, long BS, const long long* __restrict__ seg,
                                                                    const long long* __restrict__ tile_seg,
                                                                    const long long* __restrict__ seg_tile,
                                                                    const T* __restrict__ w, const T* __restrict__ c,
                                                                    const T* __restrict__ yobs, const T* __restrict__ prec,
                                                                    const T* __restrict__ pair_mean, const T* __restrict__ pair_cov,
                                                                    int grads, T* __restrict__ ws) {
    constexpr int W = P * D2 + 1, TP = mvn_tri(P), NG = P + TP + 1;
    constexpr int TRI = mvn_tri(D2), E = mvn_entries(P, D2), R = (E + 63) / 64;
    __shared__ T lw[64 * W];
    __shared__ T ls[D2 * D2];
    __shared__ T lm[D2];
    __shared__ T lg[NG * 64];          // of the tile's points: v (P rows), then r r^T + F (TP rows), then quad
    const int lane = threadIdx.x;
    const long t = blockIdx.x;
    const TileAt at = locate_tile<64>(t, N, S, BS, seg, tile_seg, seg_tile);
    const long bs = at.bs, b = at.b, k0 = at.k0;
    const int npts = at.npts;
    int ei[R], ej[R], kind[R];         // this lane's entries: kind 0 = (ei, ej) of g_cov's triangle, 1 = ei of g_mean, 2 = row ei of lg
    T part[R];                         // (an entry of m_sum, or quad), 3 = surplus
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = lane + 64 * r;
        part[r] = T(0);
        ei[r] = ej[r] = 0;
        kind[r] = e < TRI ? 0 : (e < TRI + D2 ? 1 : (e < E ? 2 : 3));
        if (kind[r] == 0) tri_decode(e, ei[r], ej[r]);
        if (kind[r] == 1) ei[r] = e - TRI;
        if (kind[r] == 2) ei[r] = P + (e - TRI - D2);
    }
    if (npts > 0) {
        const long id0 = b * N + k0;                                 // the tile's first point
        T lam[TP];                                                   // the lower triangle of Lam: uniform, read once
        {
            int e = 0;
#pragma unroll
            for (int p = 0; p < P; ++p) {
#pragma unroll
                for (int q = 0; q <= p; ++q) lam[e++] = prec[p * P + q];
            }
        }
        for (int idx = lane; idx < D2 * D2; idx += 64) ls[idx] = pair_cov[bs * (D2 * D2) + idx];
        if (lane < D2) lm[lane] = pair_mean[bs * D2 + lane];
        stage_tile<T, P * D2>(lane, npts, w + id0 * (P * D2), lw);   // npts rows of P 2d elements
        __syncthreads();
        if (lane < npts) {
            T wr[P][D2], mu[P], f[P][P];
#pragma unroll
            for (int p = 0; p < P; ++p) {
                mu[p] = T(0);
#pragma unroll
                for (int i = 0; i < D2; ++i) wr[p][i] = lw[lane * W + p * D2 + i];
#pragma unroll
                for (int q = 0; q <= p; ++q) f[p][q] = c[(id0 + lane) * (P * P) + p * P + q];
            }
#pragma unroll 1
            for (int i = 0; i < D2; ++i) {         // (rolled: unrolled, the compiler keeps all of S_s in registers and spills)
                T acc[P], wi[P];
#pragma unroll
                for (int p = 0; p < P; ++p) acc[p] = T(0);
#pragma unroll
                for (int cc = 0; cc < D2; ++cc) {
                    const T sic = ls[i * D2 + cc];
#pragma unroll
                    for (int p = 0; p < P; ++p) acc[p] += sic * wr[p][cc];
                }
                const T mi = lm[i];
#pragma unroll
                for (int p = 0; p < P; ++p) wi[p] = lw[lane * W + p * D2 + i];
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    mu[p] += wi[p] * mi;
#pragma unroll
                    for (int q = 0; q <= p; ++q) f[p][q] += wi[q] * acc[p];
                }
            }
            T r[P], quad = T(0);
#pragma unroll
            for (int p = 0; p < P; ++p) r[p] = yobs[(id0 + lane) * P + p] - mu[p];
#pragma unroll
            for (int p = 0; p < P; ++p) {
                T v = T(0);
#pragma unroll
                for (int q = 0; q < P; ++q) v += lam[q <= p ? mvn_tri(p) + q : mvn_tri(q) + p] * r[q];
                lg[p * 64 + lane] = v;
                quad += r[p] * v;
            }
            int e = 0;
#pragma unroll
            for (int p = 0; p < P; ++p) {
#pragma unroll
                for (int q = 0; q <= p; ++q) {
                    quad += (q == p ? lam[e] : T(2) * lam[e]) * f[p][q];
                    lg[(P + e) * 64 + lane] = r[p] * r[q] + f[p][q];
                    ++e;
                }
            }
            lg[(P + TP) * 64 + lane] = quad;
        }
        __syncthreads();
        if (grads) {
            for (int k = 0; k < npts; ++k) {
                int e = 0;
#pragma unroll
                for (int p = 0; p < P; ++p) {
#pragma unroll
                    for (int q = 0; q <= p; ++q) {
                        const T h = T(-0.5) * lam[e];
                        ++e;
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            if (kind[r] == 0) {
                                const T wpi = lw[k * W + p * D2 + ei[r]], wpj = lw[k * W + p * D2 + ej[r]];
                                if (q == p) {
                                    part[r] += h * (wpi * wpj);
                                } else {
                                    part[r] += h * (wpi * lw[k * W + q * D2 + ej[r]] + lw[k * W + q * D2 + ei[r]] * wpj);
                                }
                            }
                        }
                    }
                }
#pragma unroll
                for (int p = 0; p < P; ++p) {
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (kind[r] == 1) part[r] += lg[p * 64 + k] * lw[k * W + p * D2 + ei[r]];
                }
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (kind[r] == 2) part[r] += lg[ei[r] * 64 + k];
            }
        } else if (lane == (E - 1) % 64) {         // value only: the one entry, with the bits it has beside the adjoints
            for (int k = 0; k < npts; ++k) part[R - 1] += lg[(P + TP) * 64 + k];
        }
    }
    store_row<E>(ws + t * E, lane, part);
}

// pass 2: one block per (series, segment), a lane per entry of the workspace row
template <typename T, int P, int D2>
__global__ void __launch_bounds__(256) mvn_reduce_kernel(long num_tiles, const long long* __restrict__ seg_tile,
                                                         const T* __restrict__ ws, T* __restrict__ quad_sum, T* __restrict__ g_mean,
                                                         T* __restrict__ g_cov, T* __restrict__ m_sum) {
    constexpr int TRI = mvn_tri(D2), E = mvn_entries(P, D2);
    const long bs = blockIdx.x;
    long t_lo = 0, t_hi = 0;
    if (seg_tile) {                                // (NULL: no points at all)
        t_lo = (long)seg_tile[bs];
        t_hi = (long)seg_tile[bs + 1];
        clamp_range(t_lo, t_hi, num_tiles);
    }
    for (int e = threadIdx.x; e < E; e += 256) {
        if (e < TRI + D2 ? !g_mean : (e < E - 1 ? !m_sum : !quad_sum)) continue;
        T acc = T(0);
        for (long t = t_lo; t < t_hi; ++t) acc += ws[t * E + e];
        int i, j;
        if (e < TRI) {
            tri_decode(e, i, j);
            g_cov[bs * (D2 * D2) + i * D2 + j] = acc;
            g_cov[bs * (D2 * D2) + j * D2 + i] = acc;
        } else if (e < TRI + D2) {
            g_mean[bs * D2 + (e - TRI)] = acc;
        } else if (e < E - 1) {
            tri_decode(e - TRI - D2, i, j);
            m_sum[bs * (P * P) + i * P + j] = acc;
            m_sum[bs * (P * P) + j * P + i] = acc;
        } else {
            quad_sum[bs] = acc;
        }
    }
}

inline bool mvn_instantiated(int two_d, int outputs) {
    return outputs >= 2 && outputs <= 4 && two_d >= 2 && two_d <= 18 && !(two_d & 1);
}

// (num_outputs, two_d) as compile-time constants: num_outputs in 2, 3, 4 and two_d even in 2 ... 18; -101 for any other
template <typename F>
int with_mvn_dims(int outputs, int two_d, F&& f) {
    auto at = [&](auto P) { return with_even_two_d<2>(two_d, -101, [&](auto D) { return f(P, D); }); };
    switch (outputs) {
        case 2: return at(std::integral_constant<int, 2>{});
        case 3: return at(std::integral_constant<int, 3>{});
        case 4: return at(std::integral_constant<int, 4>{});
        default: return -101;
    }
}

template <typename T>
int run_mvn_expect(int64_t B, int64_t N, int64_t S, int two_d, int outputs, const int64_t* seg, const T* w, const T* c, const T* y,
                   const T* prec, const T* pm, const T* pc, int64_t tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* ws,
                   size_t ws_bytes, T* quad_sum, T* g_mean, T* g_cov, T* m_sum, void* stream) {
    int bad = check_segmentation(B, N, S);
    if (bad) return bad;
    if (!mvn_instantiated(two_d, outputs)) return -101;
    if ((bad = check_tile_count(13, N, tiles))) return bad;
    if (!g_mean && g_cov) return -19;
    if (g_mean && !g_cov) return -20;
    if (B == 0 || (!quad_sum && !g_mean && !m_sum)) return 0;  // nothing asked for
    if (tiles > 0) {
        if ((bad = first_null(6, {seg, w, c, y, prec, pm, pc}))) return bad;
        if ((bad = check_tile_table(13, tiles, tile_seg, seg_tile, ws, ws_bytes, size_t(mvn_entries(outputs, two_d)), sizeof(T))))
            return bad;
    }
    return with_mvn_dims(outputs, two_d, [&](auto PP, auto D) {
        constexpr int P = decltype(PP)::value, D2 = decltype(D)::value;
        if (tiles > 0) {
            const int rc = launch(sparse_mvn_expect_tile_kernel<T, P, D2>, tiles, 64, stream, N, S, B * S, ll(seg), ll(tile_seg),
                                  ll(seg_tile), w, c, y, prec, pm, pc, (g_mean || m_sum) ? 1 : 0, ws);
            if (rc) return rc;
        }
        return launch(mvn_reduce_kernel<T, P, D2>, B * S, 256, stream, tiles, tiles > 0 ? ll(seg_tile) : nullptr, ws, quad_sum, g_mean,
                      g_cov, m_sum);
    });
}

}  // namespace

extern "C" {

size_t mf_lik_sparse_mvn_expectations_workspace_bytes(int64_t num_tiles, int two_d, int num_outputs, int elem_size) {
    if (num_tiles <= 0 || two_d < 1 || num_outputs < 1 || elem_size < 1) return 0;
    return size_t(num_tiles) * size_t(mvn_entries(num_outputs, two_d)) * size_t(elem_size);
}
int mf_lik_sparse_mvn_expectations_f64(int64_t B, int64_t N, int64_t S, int two_d, int num_outputs, const int64_t* seg,
                                       const double* w, const double* c, const double* y, const double* prec, const double* pm,
                                       const double* pc, int64_t tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* ws,
                                       size_t ws_bytes, double* quad_sum, double* g_mean, double* g_cov, double* m_sum, void* stream) {
    return run_mvn_expect<double>(B, N, S, two_d, num_outputs, seg, w, c, y, prec, pm, pc, tiles, tile_seg, seg_tile, ws, ws_bytes,
                                  quad_sum, g_mean, g_cov, m_sum, stream);
}
int mf_lik_sparse_mvn_expectations_f32(int64_t B, int64_t N, int64_t S, int two_d, int num_outputs, const int64_t* seg, const float* w,
                                       const float* c, const float* y, const float* prec, const float* pm, const float* pc,
                                       int64_t tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* ws, size_t ws_bytes,
                                       float* quad_sum, float* g_mean, float* g_cov, float* m_sum, void* stream) {
    return run_mvn_expect<float>(B, N, S, two_d, num_outputs, seg, w, c, y, prec, pm, pc, tiles, tile_seg, seg_tile, ws, ws_bytes,
                                 quad_sum, g_mean, g_cov, m_sum, stream);
}

}  // extern "C"
