// The data term of the SVGP ELBO with the likelihood's parameter theta in DEVICE memory, one value per series or one for all, and the
// adjoint onto theta out of the same launch (gpflow's trainable Gaussian.variance / StudentT.scale under
// markovflow/models/sparse_variational.py:149-192).  mf_lik_sparse_expectations_* (mf_lik.hip) takes the parameter as a host double in
// the kernel arguments: a torch parameter fed that way costs a host read per step, and a parameter per series cannot be said at all.
//   lik 0  Gaussian    theta = variance    closed forms:  gt = (1 / 2 theta) ((r^2 + fvar) / theta - 1),  r = y - fmu
//   lik 3  Student-t   theta = scale       params [df, const],  const = lgamma((df+1)/2) - lgamma(df/2) - log(df pi)/2  (free of theta);
//                                          the nq-point rule with one more accumulator:  d l / d theta = (l'(f_i) r_i - 1) / theta,
//                                          since l' r = (df + 1) r^2 / (a + r^2), a = df theta^2, which the loop forms anyway
// Two passes, tile-parallel, on the front end of mf_lik_tile.hpp (tile table and locator, staging of w, store of a workspace row) and
// log_prob / expectations of mf_lik_math.hpp.  Of its own:
//   pass 1, one wavefront per tile of at most 64 points.  The tile's series b is wavefront-uniform: theta[b theta_stride] is ONE load
//            per tile and the Par<T> the point code reads (theta, df, const - log theta) is formed before the lanes part.
//            Phase 1, a lane per point: fmu = w . m_s, fvar = c + w^T S_s w, then (ve, gm, gv, gt); FOUR rows of 64 values in LDS,
//            gv, gm, ve, gt.  Phase 2, a lane per accumulator entry: the lower triangle of g_cov, g_mean, sum ve, sum gt -
//            2d (2d + 1) / 2 + 2d + 2 entries, 191 <= 3 . 64 at 2d = 18: as many entries per lane as the pair without theta at every 2d.
//            An entry is (row of LDS values, two columns of the point's padded row of w): the matrix reads gv and (i, j), the vector gm
//            and (i, the column of ones), each scalar its row and the ones twice - one multiply-add form for all four kinds, and a
//            times-one leaves the bits of a plain sum.  Without the pair adjoints (g_theta alone, the value alone) only the two
//            scalar entries are accumulated, as plain sums: the same bits.
//   pass 2, one block per (series, segment), a lane per entry: the segment's rows in ascending tile order, the triangle mirrored,
//            g_theta[b, s] written beside ve_sum[b, s].  It reads theta[b theta_stride] too: a theta that is not a positive finite
//            number makes ALL FOUR outputs of EVERY segment of that series NaN - the empty ones included, which have no tile to say
//            so - and no other series changes.  Nobody checks theta on the host: that would be a synchronisation.
// No floating-point atomics; every sum's order is fixed by the point order alone: the same bits on every launch, for a series alone
// or inside a batch, and for each output whichever of the others is asked for.
// Instantiated: lik in 0, 3 and 2d even in 2 ... 18, both dtypes; none uses scratch (compiler remarks: DESIGN.md 4.27).
#include "../../include/markovflow_amd.h"

#include <limits>

#include "mf_lik_tile.hpp"

namespace {

constexpr int theta_entries(int d2) { return seg_entries(d2, 4); }      // triangle, vector, sum ve, sum gt

// a theta the likelihood is defined for: positive and finite (NaN fails the first comparison)
template <typename T> __device__ __forceinline__ bool theta_valid(T th) { return th > T(0) && th <= std::numeric_limits<T>::max(); }

template <typename T, int LIK, int D2>
__global__ void __launch_bounds__(64) theta_expect_tile_kernel(long N, int S, long BS, Rule<T> q, T df, T lconst,
                                                               const T* __restrict__ theta, long theta_stride,
                                                               const long long* __restrict__ seg,
                                                               const long long* __restrict__ tile_seg,
                                                               const long long* __restrict__ seg_tile, const T* __restrict__ w,
                                                               const T* __restrict__ cvar, const T* __restrict__ yobs,
                                                               const T* __restrict__ pair_mean, const T* __restrict__ pair_cov,
                                                               int grads, T* __restrict__ ws) {
    constexpr int W = D2 + 1, TRI = D2 * (D2 + 1) / 2, E = theta_entries(D2), R = (E + 63) / 64;
    constexpr int GV = 0, GM = 64, VE = 128, GT = 192;      // the rows of lg
    __shared__ T lw[64 * W];           // the tile's rows of w, each padded with a one
    __shared__ T ls[D2 * D2];
    __shared__ T lm[D2];
    __shared__ T lg[4 * 64];
    const int lane = threadIdx.x;
    const long t = blockIdx.x;
    const TileAt at = locate_tile<64>(t, N, S, BS, seg, tile_seg, seg_tile);
    const int npts = at.npts;
    int ei[R], ej[R], es[R];           // this lane's entries: part += (lg[es + k] lw[k][ej]) lw[k][ei]; a surplus one decodes as entry 0
    T part[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = lane + 64 * r < E ? lane + 64 * r : 0;
        part[r] = T(0);
        ei[r] = ej[r] = D2;
        es[r] = e == E - 1 ? GT : VE;
        if (e < TRI) {
            tri_decode(e, ei[r], ej[r]);
            es[r] = GV;
        } else if (e < TRI + D2) {
            ei[r] = e - TRI;
            es[r] = GM;
        }
    }
    if (npts > 0) {
        const T th = theta[at.b * theta_stride];                    // wavefront-uniform: one load per tile
        Par<T> p;
        p.p0 = th;
        p.p1 = df;
        p.p2 = LIK == 3 ? lconst - m_log(th) : T(0);
        const T ith = T(1) / th;
        for (int idx = lane; idx < D2 * D2; idx += 64) ls[idx] = pair_cov[at.bs * (D2 * D2) + idx];
        if (lane < D2) lm[lane] = pair_mean[at.bs * D2 + lane];
        lw[lane * W + D2] = T(1);
        stage_tile<T, D2>(lane, npts, w + (at.b * N + at.k0) * D2, lw);
        __syncthreads();
        if (lane < npts) {
            const long id = at.b * N + at.k0 + lane;
            T wr[D2], mu = T(0), s2 = cvar[id];
#pragma unroll
            for (int i = 0; i < D2; ++i) wr[i] = lw[lane * W + i];
#pragma unroll
            for (int i = 0; i < D2; ++i) {
                T sw = T(0);
#pragma unroll
                for (int j = 0; j < D2; ++j) sw += ls[i * D2 + j] * wr[j];
                s2 += wr[i] * sw;
                mu += wr[i] * lm[i];
            }
            const T y = yobs[id];
            T ve, gm, gv, gt;
            if (!(s2 > T(0))) {                    // outside the domain: NaN in all four sums of this point's segment
                ve = gm = gv = gt = nan_of<T>();
            } else if (LIK == 0) {
                expectations<T, 0>(q, p, mu, s2, y, ve, gm, gv);
                const T r = y - mu;
                gt = T(0.5) * ith * ((r * r + s2) * ith - T(1));
            } else {
                const T sd = m_sqrt(T(2) * s2);
                T a0 = T(0), a1 = T(0), a2 = T(0), a3 = T(0);
                for (int i = 0; i < q.nq; ++i) {   // wavefront-uniform: q lives in the kernel arguments
                    const T x = q.x[i], wi = q.w[i], f = mu + sd * x;
                    T dl;
                    const T l = log_prob<T, 3, true>(f, y, p, dl);
                    a0 += wi * l;
                    a1 += wi * dl;
                    a2 += wi * dl * x;
                    a3 += wi * (dl * (y - f) - T(1));
                }
                ve = a0;
                gm = a1;
                gv = a2 / sd;
                gt = a3 * ith;
            }
            lg[GV + lane] = gv;
            lg[GM + lane] = gm;
            lg[VE + lane] = ve;
            lg[GT + lane] = gt;
        }
        __syncthreads();
        if (grads) {
            for (int k = 0; k < npts; ++k) {
#pragma unroll
                for (int r = 0; r < R; ++r) part[r] += (lg[es[r] + k] * lw[k * W + ej[r]]) * lw[k * W + ei[r]];
            }
        } else {                                   // the two scalar entries alone, with the bits they have beside the pair adjoints
            if (lane == (E - 2) % 64)
                for (int k = 0; k < npts; ++k) part[(E - 2) / 64] += lg[VE + k];
            if (lane == (E - 1) % 64)
                for (int k = 0; k < npts; ++k) part[(E - 1) / 64] += lg[GT + k];
        }
    }
    store_row<E>(ws + t * E, lane, part);
}

// pass 2: one block per (series, segment), a lane per entry of the workspace row
template <typename T, int D2>
__global__ void __launch_bounds__(256) theta_reduce_kernel(long num_tiles, int S, const long long* __restrict__ seg_tile,
                                                           const T* __restrict__ ws, const T* __restrict__ theta, long theta_stride,
                                                           T* __restrict__ ve_sum, T* __restrict__ g_mean, T* __restrict__ g_cov,
                                                           T* __restrict__ g_theta) {
    constexpr int TRI = D2 * (D2 + 1) / 2, E = theta_entries(D2);
    const long bs = blockIdx.x;
    const bool valid = theta_valid(theta[(bs / S) * theta_stride]);
    long t_lo = 0, t_hi = 0;
    if (seg_tile) {                                // (NULL: no points at all)
        t_lo = (long)seg_tile[bs];
        t_hi = (long)seg_tile[bs + 1];
        clamp_range(t_lo, t_hi, num_tiles);
    }
    for (int e = threadIdx.x; e < E; e += 256) {
        if (e < TRI + D2 ? !g_mean : (e == E - 2 ? !ve_sum : !g_theta)) continue;
        T acc = T(0);
        for (long t = t_lo; t < t_hi; ++t) acc += ws[t * E + e];
        if (!valid) acc = nan_of<T>();
        if (e < TRI) {
            int i, j;
            tri_decode(e, i, j);
            g_cov[bs * (D2 * D2) + i * D2 + j] = acc;
            g_cov[bs * (D2 * D2) + j * D2 + i] = acc;
        } else if (e < TRI + D2) {
            g_mean[bs * D2 + (e - TRI)] = acc;
        } else if (e == E - 2) {
            ve_sum[bs] = acc;
        } else {
            g_theta[bs] = acc;
        }
    }
}

inline bool theta_two_d(int two_d) { return two_d >= 2 && two_d <= 18 && !(two_d & 1); }

template <typename T>
int run_theta_expect(int64_t B, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq, const double* nodes,
                     const double* weights, const T* theta, int64_t theta_stride, const int64_t* seg, const T* w, const T* c,
                     const T* y, const T* pm, const T* pc, int64_t tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* ws,
                     size_t ws_bytes, T* ve_sum, T* g_mean, T* g_cov, T* g_theta, void* stream) {
    Rule<T> q;
    Par<T> unused;
    int bad = check_segmentation(B, N, S);
    if (bad) return bad;
    if (!theta_two_d(two_d)) return -100;
    if (lik != 0 && lik != 3) return -101;
    T df = T(0), lconst = T(0);
    if (lik == 3) {
        if (!params || !(params[0] > 0.0) || !std::isfinite(params[0]) || !std::isfinite(params[1])) return -6;
        df = T(params[0]);
        lconst = T(params[1]);
    }
    bad = prepare<T>(0, 1, nullptr, nq, nodes, weights, false, q, unused);       // -4 ... -6 there: arguments 7 ... 9 here
    if (bad) return bad - 3;
    if (theta_stride != 0 && theta_stride != 1) return -11;
    if ((bad = check_tile_count(18, N, tiles))) return bad;
    if (!g_mean && g_cov) return -24;
    if (g_mean && !g_cov) return -25;
    if (B == 0 || (!ve_sum && !g_mean && !g_theta)) return 0;       // nothing asked for
    if (!theta) return -10;                                         // (pass 2 reads it whatever N is)
    if (tiles > 0) {
        if ((bad = first_null(12, {seg, w, c, y, pm, pc}))) return bad;
        if ((bad = check_tile_table(18, tiles, tile_seg, seg_tile, ws, ws_bytes, size_t(theta_entries(two_d)), sizeof(T)))) return bad;
    }
    return with_even_two_d<2>(two_d, -100, [&](auto D) {
        constexpr int D2 = decltype(D)::value;
        if (tiles > 0) {
            const int grads = g_mean ? 1 : 0;
            const int rc = lik == 0 ? launch(theta_expect_tile_kernel<T, 0, D2>, tiles, 64, stream, N, S, B * S, q, df, lconst, theta,
                                             theta_stride, ll(seg), ll(tile_seg), ll(seg_tile), w, c, y, pm, pc, grads, ws)
                                    : launch(theta_expect_tile_kernel<T, 3, D2>, tiles, 64, stream, N, S, B * S, q, df, lconst, theta,
                                             theta_stride, ll(seg), ll(tile_seg), ll(seg_tile), w, c, y, pm, pc, grads, ws);
            if (rc) return rc;
        }
        return launch(theta_reduce_kernel<T, D2>, B * S, 256, stream, tiles, S, tiles > 0 ? ll(seg_tile) : nullptr, ws, theta,
                      theta_stride, ve_sum, g_mean, g_cov, g_theta);
    });
}

}  // namespace

extern "C" {

size_t mf_lik_sparse_expectations_theta_workspace_bytes(int64_t num_tiles, int two_d, int elem_size) {
    if (num_tiles <= 0 || !theta_two_d(two_d) || elem_size < 1) return 0;
    return size_t(num_tiles) * size_t(theta_entries(two_d)) * size_t(elem_size);
}
int mf_lik_sparse_expectations_theta_f64(int64_t B, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq,
                                         const double* nodes, const double* weights, const double* theta, int64_t theta_stride,
                                         const int64_t* seg_offsets, const double* w, const double* c, const double* y,
                                         const double* pair_mean, const double* pair_cov, int64_t num_tiles, const int64_t* tile_seg,
                                         const int64_t* seg_tile, void* workspace, size_t workspace_bytes, double* ve_sum,
                                         double* g_mean, double* g_cov, double* g_theta, void* stream) {
    return run_theta_expect<double>(B, N, S, two_d, lik, params, nq, nodes, weights, theta, theta_stride, seg_offsets, w, c, y,
                                    pair_mean, pair_cov, num_tiles, tile_seg, seg_tile, workspace, workspace_bytes, ve_sum, g_mean,
                                    g_cov, g_theta, stream);
}
int mf_lik_sparse_expectations_theta_f32(int64_t B, int64_t N, int64_t S, int two_d, int lik, const double* params, int nq,
                                         const double* nodes, const double* weights, const float* theta, int64_t theta_stride,
                                         const int64_t* seg_offsets, const float* w, const float* c, const float* y,
                                         const float* pair_mean, const float* pair_cov, int64_t num_tiles, const int64_t* tile_seg,
                                         const int64_t* seg_tile, void* workspace, size_t workspace_bytes, float* ve_sum, float* g_mean,
                                         float* g_cov, float* g_theta, void* stream) {
    return run_theta_expect<float>(B, N, S, two_d, lik, params, nq, nodes, weights, theta, theta_stride, seg_offsets, w, c, y,
                                   pair_mean, pair_cov, num_tiles, tile_seg, seg_tile, workspace, workspace_bytes, ve_sum, g_mean,
                                   g_cov, g_theta, stream);
}

}  // extern "C"
