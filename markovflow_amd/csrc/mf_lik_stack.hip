// The data term of the SVGP ELBO for a likelihood with K latent functions per observation on K STACKED chains
// (markovflow/kernels/sde_kernel.py:945-1279 and markovflow/emission_model.py:270-378 under
// markovflow/models/sparse_variational.py:149-192): every latent has a chain of its own, K is the last batch dimension, the K chains
// of a series share one segmentation, and q is independent across the latents - K pair marginals of 2d per segment, not one of K 2d.
//   w [B, K, N, 2d]   c [B, K, N]   y [B, N]   pair_mean [B, K, S, 2d]   pair_cov [B, K, S, 2d, 2d]        (no transposes)
// Per point n of segment s and latent k, ascending:  mu_k = w_kn . m_ks,  s2_k = c_kn + w_kn^T S_ks w_kn;  (ve, gm_k, gv_k) of the
// likelihood at (mu, s2, y_n);  per segment, over the points in ascending order,
//   ve_sum = sum ve      g_mean[k] = sum gm_k w_kn      g_cov[k] = sum gv_k w_kn w_kn^T
// Two passes, tile-parallel, as mf_lik_sparse_multi_expectations_* (mf_lik.hip): the tile table and its locator, the tile of 64 points
// per wavefront, the staging of a chain's rows, the workspace row and pass 2 (mf_lik_tile.hpp) are the siblings' at K chains.
//   pass 1, phase 1, a lane per point.  The point's K rows of w travel through LDS as ONE row of K 2d + 1 elements (odd: the lanes'
//            rows start on distinct banks); a chain's npts rows are contiguous in global memory, so the loads are coalesced runs.
//            The latents are walked one after the other, so a lane holds ONE row of w in registers, not K: the rolled walk over the
//            rows i of S_ks,  acc = sum_c S_ic w_c (c ascending),  s2 += w_i acc,  mu += w_i m_i.  Then the likelihood's
//            expectation; gv_k (rows 0 .. K - 1 of lg), gm_k (rows K .. 2 K - 1) and ve (row 2 K) stay in LDS.
//   pass 1, phase 2, a lane per accumulator entry.  A workspace row is K (tri + 2d) + 1 values: per latent the lower triangle of
//            g_cov and g_mean, then sum ve.  The points in ascending order:  g_cov[k] (i, j) += (gv_k w_kj) w_ki,
//            g_mean[k] i += gm_k w_ki,  ve_sum += ve.
//   pass 2, one block per (series, segment), a lane per entry: the segment's rows are added in ascending tile order, the outputs are
//            written and every triangle mirrored.  An empty segment writes zeros.
// Value only (g_mean and g_cov NULL): phase 2 adds ve alone, the same numbers in the same order.  No floating-point atomics.
// A latent that the point's branch does not read has gm = gv = 0 and its s2 is not examined; one that is read with s2 <= 0 or NaN
// makes ve and ALL K latents' gm and gv of the point NaN, so the segment's ve_sum and its g_mean / g_cov on every chain are NaN.
// The zero columns of w in the padded state dimensions of a chain shorter than d are multiplied through.
// LDS at K = 3, 2d = 18, float64: 28160 (rows) + 7776 (S) + 432 (m) + 3584 (lg) = 39952 B.
// Instantiated: (K, lik) = (3, multi-stage) and (2, heteroscedastic Gaussian), 2d even in 2 ... 18, both dtypes.
#include "../../include/markovflow_amd.h"

#include "mf_lik_tile.hpp"
#include "mf_lik_multistage.hpp"

namespace {

constexpr int LIK_HETEROSCEDASTIC = 5;     // mean and log-variance latents, K = 2 (LIK_MULTISTAGE = 4 has K = 3)

// (a workspace row is expect_entries(K, 2d) values - per latent the triangle of g_cov and g_mean, then sum ve: mf_lik_tile.hpp)

template <int LIK> struct StackLatents;
template <> struct StackLatents<LIK_MULTISTAGE> { static constexpr int value = MULTI_L; };
template <> struct StackLatents<LIK_HETEROSCEDASTIC> { static constexpr int value = 2; };

// The heteroscedastic Gaussian  y ~ N(F0, exp F1)  in closed form: with e = exp(-m1 + v1 / 2) and E = e ((m0 - y)^2 + v0),
//   ve = -(log 2 pi + m1 + E) / 2,   d/dm0 = -e (m0 - y),   d/dv0 = -e / 2,   d/dm1 = -(1 - E) / 2,   d/dv1 = -E / 4.
template <typename T>
__device__ __forceinline__ void heteroscedastic_expectations(T y, const T (&mu)[2], const T (&s2)[2], T& ve, T (&gm)[2], T (&gv)[2]) {
    constexpr T LOG_2PI = T(1.8378770664093454835606594728112);
    const T r = mu[0] - y;
    const T e = m_exp(T(0.5) * s2[1] - mu[1]);
    const T big = e * (r * r + s2[0]);
    ve = T(-0.5) * (LOG_2PI + mu[1] + big);
    gm[0] = -e * r;
    gv[0] = T(-0.5) * e;
    gm[1] = T(-0.5) * (T(1) - big);
    gv[1] = T(-0.25) * big;
}

// the likelihood of one point on K marginals, with the domain rule of the stacked term: a latent that is read outside the domain
// poisons the value and the derivatives of EVERY latent of the point
template <typename T, int LIK, int K>
__device__ __forceinline__ void stack_expectations(const Rule<T>& q, T y, const T (&mu)[K], const T (&s2)[K], T& ve, T (&gm)[K],
                                                   T (&gv)[K]) {
    bool bad = false;
    if constexpr (LIK == LIK_MULTISTAGE) {
        const int stage = y == T(0) ? 0 : (y == T(1) ? 1 : (y >= T(2) ? 2 : -1));   // (multistage_expectations' own branch)
#pragma unroll
        for (int k = 0; k < K; ++k) bad = bad || (k <= stage && !(s2[k] > T(0)));
        multistage_expectations<T>(q, y, mu, s2, ve, gm, gv);
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) bad = bad || !(s2[k] > T(0));
        heteroscedastic_expectations<T>(y, mu, s2, ve, gm, gv);
    }
    if (bad) {
        ve = nan_of<T>();
#pragma unroll
        for (int k = 0; k < K; ++k) gm[k] = gv[k] = nan_of<T>();
    }
}

template <typename T, int LIK, int K, int D2>
__global__ void __launch_bounds__(64) stack_expect_tile_kernel(long N, int S, long BS, Rule<T> q, const long long* __restrict__ seg,
                                                               const long long* __restrict__ tile_seg,
                                                               const long long* __restrict__ seg_tile, const T* __restrict__ w,
                                                               const T* __restrict__ cvar, const T* __restrict__ yobs,
                                                               const T* __restrict__ pair_mean, const T* __restrict__ pair_cov,
                                                               int grads, T* __restrict__ ws) {
    constexpr int W = K * D2 + 1, TRI = D2 * (D2 + 1) / 2, PER = TRI + D2, E = expect_entries(K, D2), R = (E + 63) / 64;
    __shared__ T lw[64 * W];
    __shared__ T ls[K * D2 * D2];
    __shared__ T lm[K * D2];
    __shared__ T lg[(2 * K + 1) * 64];
    const int lane = threadIdx.x;
    const long t = blockIdx.x;
    const TileAt at = locate_tile<64>(t, N, S, BS, seg, tile_seg, seg_tile);
    const long b = at.b, s = at.s, k0 = at.k0;
    const int npts = at.npts;
    // this lane's entries: kind 0 = (oi, oj) of a triangle, 1 = oi of a vector, 2 = the scalar, 3 = surplus; oi / oj are offsets into
    // a point's row of lw (latent * 2d + state), og the row of lg that holds the entry's factor
    int oi[R], oj[R], og[R], kind[R];
    T part[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = lane + 64 * r;
        part[r] = T(0);
        oi[r] = oj[r] = og[r] = 0;
        kind[r] = e < E - 1 ? 0 : (e < E ? 2 : 3);
        if (kind[r] == 0) {
            const int k = e / PER, f = e - k * PER;
            if (f < TRI) {
                int i, c;
                tri_decode(f, i, c);
                oi[r] = k * D2 + i;
                oj[r] = k * D2 + c;
                og[r] = k * 64;
            } else {
                kind[r] = 1;
                oi[r] = k * D2 + (f - TRI);
                og[r] = (K + k) * 64;
            }
        }
    }
    if (npts > 0) {
        for (int idx = lane; idx < K * D2 * D2; idx += 64) {
            const int k = idx / (D2 * D2);
            ls[idx] = pair_cov[((b * K + k) * S + s) * (D2 * D2) + (idx - k * (D2 * D2))];
        }
        for (int idx = lane; idx < K * D2; idx += 64) {
            const int k = idx / D2;
            lm[idx] = pair_mean[((b * K + k) * S + s) * D2 + (idx - k * D2)];
        }
#pragma unroll
        for (int k = 0; k < K; ++k)                                   // npts rows of 2d elements of chain k, at column k 2d
            stage_tile<T, D2, W>(lane, npts, w + ((b * K + k) * N + k0) * D2, lw, k * D2);
        __syncthreads();
        if (lane < npts) {
            T mu[K], s2[K], gm[K], gv[K], ve;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                T wr[D2];
#pragma unroll
                for (int i = 0; i < D2; ++i) wr[i] = lw[lane * W + k * D2 + i];
                T m = T(0), v = cvar[(b * K + k) * N + k0 + lane];
#pragma unroll 1
                for (int i = 0; i < D2; ++i) {     // (rolled: unrolled, the compiler keeps all of S_ks in registers and spills)
                    T acc = T(0);
#pragma unroll
                    for (int c = 0; c < D2; ++c) acc += ls[(k * D2 + i) * D2 + c] * wr[c];
                    const T wi = lw[lane * W + k * D2 + i];
                    v += wi * acc;
                    m += wi * lm[k * D2 + i];
                }
                mu[k] = m;
                s2[k] = v;
            }
            stack_expectations<T, LIK, K>(q, yobs[b * N + k0 + lane], mu, s2, ve, gm, gv);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                lg[k * 64 + lane] = gv[k];
                lg[(K + k) * 64 + lane] = gm[k];
            }
            lg[2 * K * 64 + lane] = ve;
        }
        __syncthreads();
        if (grads) {
            for (int p = 0; p < npts; ++p) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (kind[r] == 0) part[r] += (lg[og[r] + p] * lw[p * W + oj[r]]) * lw[p * W + oi[r]];
                    if (kind[r] == 1) part[r] += lg[og[r] + p] * lw[p * W + oi[r]];
                    if (kind[r] == 2) part[r] += lg[2 * K * 64 + p];
                }
            }
        } else if (lane == (E - 1) % 64) {         // value only: the one entry, with the bits it has beside the gradients
            for (int p = 0; p < npts; ++p) part[R - 1] += lg[2 * K * 64 + p];
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {                  // (not store_row: through it four float64 instantiations spill two more SGPRs)
        const int e = lane + 64 * r;
        if (e < E) ws[t * E + e] = part[r];
    }
}

// (pass 2 is expect_reduce_kernel<T, K, D2> of mf_lik_tile.hpp)

inline bool stack_instantiated(int two_d, int latent_dim, int lik) {
    if (two_d < 2 || two_d > 18 || (two_d & 1)) return false;
    return (lik == LIK_MULTISTAGE && latent_dim == StackLatents<LIK_MULTISTAGE>::value) ||
           (lik == LIK_HETEROSCEDASTIC && latent_dim == StackLatents<LIK_HETEROSCEDASTIC>::value);
}

template <typename T>
int run_stack_expect(int64_t B, int latent_dim, int64_t N, int64_t S, int two_d, int lik, int nq, const double* nodes,
                     const double* weights, const int64_t* seg, const T* w, const T* c, const T* y, const T* pm, const T* pc,
                     int64_t tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* ws, size_t ws_bytes, T* ve_sum, T* g_mean,
                     T* g_cov, void* stream) {
    Rule<T> q;
    Par<T> p;
    int bad = check_segmentation(B, N, S, 3, 4);                                 // (latent_dim is the second argument here)
    if (bad) return bad;
    if (!stack_instantiated(two_d, latent_dim, lik)) return -101;
    bad = prepare<T>(0, 1, nullptr, nq, nodes, weights, false, q, p);            // -4 ... -6 there: arguments 8 ... 10 here
    if (bad) return bad - 4;
    if ((bad = check_tile_count(17, N, tiles))) return bad;
    if (!g_mean && g_cov) return -23;
    if (g_mean && !g_cov) return -24;
    if (B == 0 || (!ve_sum && !g_mean)) return 0;      // nothing asked for
    if (tiles > 0) {
        if ((bad = first_null(11, {seg, w, c, y, pm, pc}))) return bad;
        if ((bad = check_tile_table(17, tiles, tile_seg, seg_tile, ws, ws_bytes, size_t(expect_entries(latent_dim, two_d)), sizeof(T))))
            return bad;
    }
    return with_even_two_d<2>(two_d, -101, [&](auto D) {
        constexpr int D2 = decltype(D)::value;
        auto run = [&](auto LK) {
            constexpr int LIK = decltype(LK)::value, K = StackLatents<LIK>::value;
            if (tiles > 0) {
                const int rc = launch(stack_expect_tile_kernel<T, LIK, K, D2>, tiles, 64, stream, N, S, B * S, q, ll(seg),
                                      ll(tile_seg), ll(seg_tile), w, c, y, pm, pc, g_mean ? 1 : 0, ws);
                if (rc) return rc;
            }
            return launch(expect_reduce_kernel<T, K, D2>, B * S, 256, stream, tiles, S, tiles > 0 ? ll(seg_tile) : nullptr, ws,
                          ve_sum, g_mean, g_cov);
        };
        return lik == LIK_MULTISTAGE ? run(std::integral_constant<int, LIK_MULTISTAGE>{})
                                     : run(std::integral_constant<int, LIK_HETEROSCEDASTIC>{});
    });
}

}  // namespace

extern "C" {

size_t mf_lik_stack_expectations_workspace_bytes(int64_t num_tiles, int two_d, int latent_dim, int elem_size) {
    if (num_tiles <= 0 || two_d < 2 || two_d > 18 || (two_d & 1) || latent_dim < 1 || elem_size < 1) return 0;
    return size_t(num_tiles) * size_t(expect_entries(latent_dim, two_d)) * size_t(elem_size);
}
int mf_lik_stack_expectations_f64(int64_t B, int latent_dim, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq,
                                  const double* nodes, const double* weights, const int64_t* seg, const double* w, const double* c,
                                  const double* y, const double* pm, const double* pc, int64_t tiles, const int64_t* tile_seg,
                                  const int64_t* seg_tile, void* ws, size_t ws_bytes, double* ve_sum, double* g_mean, double* g_cov,
                                  void* stream) {
    (void)params;
    return run_stack_expect<double>(B, latent_dim, N, S, two_d, lik, nq, nodes, weights, seg, w, c, y, pm, pc, tiles, tile_seg,
                                    seg_tile, ws, ws_bytes, ve_sum, g_mean, g_cov, stream);
}
int mf_lik_stack_expectations_f32(int64_t B, int latent_dim, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq,
                                  const double* nodes, const double* weights, const int64_t* seg, const float* w, const float* c,
                                  const float* y, const float* pm, const float* pc, int64_t tiles, const int64_t* tile_seg,
                                  const int64_t* seg_tile, void* ws, size_t ws_bytes, float* ve_sum, float* g_mean, float* g_cov,
                                  void* stream) {
    (void)params;
    return run_stack_expect<float>(B, latent_dim, N, S, two_d, lik, nq, nodes, weights, seg, w, c, y, pm, pc, tiles, tile_seg,
                                   seg_tile, ws, ws_bytes, ve_sum, g_mean, g_cov, stream);
}

}  // extern "C"
