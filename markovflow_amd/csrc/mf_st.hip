// The data term of the spatio-temporal sparse variational ELBO (markovflow/models/spatio_temporal_variational.py:149-236) and its
// adjoints, for a chain whose state is Ms copies of a d_t-dimensional temporal state: D = Ms d_t <= 64, pairs of dimension n = 2 D.
// The projection of a pair onto f_k is the Kronecker-structured row
//   W_k[half D + s d_t + i] = a_k[s] wt_k[half d_t + i]        (a_k [Ms] spatial weights, wt_k [2 d_t] temporal projection)
// which exists only in LDS.  Per point  V_k = Sbar W_k  (Sbar = (S + S^T) / 2, symmetrised while it is staged),  fmu = W_k . m,
// fvar = c_k + W_k . V_k,  (ve, gm, gv) as mf_lik_variational_expectations; the one mat-vec V_k serves the value, the quadratic form
// and the per-point adjoints onto a_k and wt_k.
//
// Pass 1, one workgroup of 256 threads per ROW - at most ST_TILE = 256 consecutive points of one (series, segment), walked as up to
// four GROUPS of 64 points, a lane per point:
//   stage    a and wt of the group transposed ([s][point]: a lane per point reads without bank conflicts), W [point][n padded to a
//            multiple of 16, + 1: odd stride]
//   mat-vec  Sbar travels through LDS in slabs of R rows (R = 32, 16 or 8, the largest that fits 160 KB; the choice changes no bit):
//            wave w owns R / 4 rows of the slab, its lanes the 64 points; S is read as LDS broadcasts, two columns per read.  After
//            every slab three waves fold its rows of V into  W . V  (wave 0),  Va[s] = sum_{half, i} V[j] wt[half d_t + i]  (wave 1)
//            and  Vwt[half d_t + i] = sum_s V[j] a[s]  (wave 2): V itself is never kept beyond a slab.
//   point    wave 0: fvar, the expectations, the per-point outputs
//   adjoint  g_a = gm Ma + 2 gv Va,  g_wt = gm Mwt + 2 gv Vwt  with Ma, Mwt the same contractions of m
//   sums     thread (ti, tj) of a 16 x 16 grid owns the entries (ti + 16 r, tj + 16 c), c <= r, of  sum_k gv_k W_k W_k^T  in
//            registers across the groups (36 accumulators; the lower triangle is what leaves), thread j < n entry j of
//            sum_k gm_k W_k, thread 0 sum_k ve_k: one workspace row of n (n + 1) / 2 + n + 1 values per workgroup.
// Pass 2, one block per (series, segment), adds a segment's rows in ascending order and mirrors the triangle.
// The CVI site update of the same model (spatio_temporal_variational.py:509-552, mf_lik_st_cvi_site_update_*) is pass 1 in the mode
// ST_WANT_SITES - g1 = gm - 2 gv fmu rides into the vector sum in place of gm - and a pass 2 of its own, st_cvi_reduce_kernel, which
// adds the rows in the same order and blends the sums into nat1 and nat2 in place.
// Every sum starts from 0 and grows by one fused multiply-add per term, index ascending (include/markovflow_amd.h has the list); no
// floating-point atomics.  The tile table is clamped (locate_tile at ST_TILE points a tile: mf_lik_tile.hpp), not trusted.
#include "../../include/markovflow_amd.h"

// (the tile locator and the checks of the segmentation: shared with the other tile-parallel kernels)
#include "mf_lik_tile.hpp"

namespace {

constexpr int ST_GROUP = 64;                  // points per group: a lane per point
constexpr int ST_TILE = 256;                  // points per workspace row: four groups
constexpr int ST_THREADS = 256;
constexpr int ST_MAX_D = 64;                  // Ms d_t
constexpr int ST_REG = 8;                     // a thread's entries per direction of the 16 x 16 grid
constexpr size_t ST_LDS_LIMIT = size_t(160) * 1024;

template <typename T> struct Pair2;
template <> struct Pair2<double> { using type = double2; };
template <> struct Pair2<float> { using type = float2; };

__device__ __forceinline__ float m_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double m_fma(double a, double b, double c) { return fma(a, b, c); }

// the LDS image in elements of T, the same on both sides of the launch
struct StLayout {
    int nr, ldw, lds;                         // 16-blocks of n, row stride of W (odd), row stride of the slab (even)
    int slab, w, a, wt, va, vwt, m, sc, vs, total;
};
__host__ __device__ inline StLayout st_layout(int Ms, int dt, int R) {
    StLayout L;
    const int n = 2 * Ms * dt;
    L.nr = (n + 15) / 16;
    L.ldw = 16 * L.nr + 1;
    L.lds = n + 2;
    L.slab = 0;                               // 16-byte aligned: read two columns at a time
    L.w = L.slab + R * L.lds;
    L.a = L.w + ST_GROUP * L.ldw;
    L.wt = L.a + ST_GROUP * Ms;
    L.va = L.wt + ST_GROUP * 2 * dt;
    L.vwt = L.va + ST_GROUP * Ms;
    L.m = L.vwt + ST_GROUP * 2 * dt;
    L.sc = L.m + n;
    L.vs = L.sc + 4 * ST_GROUP;               // fmu, ve, gm, gv of the group's points
    L.total = L.vs + R * ST_GROUP;
    return L;
}

// ST_WANT_SITES (with ST_WANT_GRADS): the value that rides with the point into the vector sum is g1 = gm - 2 gv fmu, the gradient in
// the first expectation parameter, in place of gm - the sums are then the CVI site targets (st_cvi_reduce_kernel)
constexpr int ST_WANT_VE = 1, ST_WANT_GRADS = 2, ST_WANT_SITES = 4;

template <typename T, int LIK>
__global__ void __launch_bounds__(ST_THREADS) st_expect_tile_kernel(
    long N, int S, long BS, int Ms, int dt, int R, Rule<T> q, Par<T> p, const long long* __restrict__ seg,
    const long long* __restrict__ tile_seg, const long long* __restrict__ seg_tile, const T* __restrict__ a, const T* __restrict__ wt,
    const T* __restrict__ cvar, const T* __restrict__ yobs, const T* __restrict__ pair_mean, const T* __restrict__ pair_cov,
    int want, T* __restrict__ ws, T* __restrict__ g_a, T* __restrict__ g_wt, T* __restrict__ g_c, T* __restrict__ fmu_out,
    T* __restrict__ fvar_out) {
    using T2 = typename Pair2<T>::type;
    extern __shared__ double2 st_lds_raw[];
    T* const lds = reinterpret_cast<T*>(st_lds_raw);
    const StLayout L = st_layout(Ms, dt, R);
    const int D = Ms * dt, n = 2 * D, two_dt = 2 * dt, nr = L.nr, ldw = L.ldw, lds_s = L.lds, RW = R >> 2;
    T* const slab = lds + L.slab;
    T* const lw = lds + L.w;
    T* const la = lds + L.a;
    T* const lwt = lds + L.wt;
    T* const lva = lds + L.va;
    T* const lvwt = lds + L.vwt;
    T* const lm = lds + L.m;
    T* const lsc = lds + L.sc;
    T* const lvs = lds + L.vs;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ti = tid >> 4, tj = tid & 15;
    const bool want_lik = want != 0 || g_a != nullptr;          // (g_a, g_wt, g_c come together)

    const long t = blockIdx.x;                                  // this row of the table: ST_TILE points a tile
    const TileAt at = locate_tile<ST_TILE>(t, N, S, BS, seg, tile_seg, seg_tile);
    const long bs = at.bs, b = at.b, k0 = at.k0;
    const int npts_row = at.npts;

    T acc[ST_REG * (ST_REG + 1) / 2];
#pragma unroll
    for (int e = 0; e < ST_REG * (ST_REG + 1) / 2; ++e) acc[e] = T(0);
    T accm = T(0), accv = T(0);

    const T* const Sg = pair_cov + bs * (long)n * n;
    for (int idx = tid; idx < n; idx += ST_THREADS) lm[idx] = pair_mean[bs * n + idx];

    for (int g0 = 0; g0 < npts_row; g0 += ST_GROUP) {
        const int npts = npts_row - g0 < ST_GROUP ? npts_row - g0 : ST_GROUP;
        const long pt0 = b * N + k0 + g0;                       // the group's first point
        __syncthreads();                                        // the group before has been read
        // ---- stage a and wt transposed; the rows of absent points are zero
        for (int idx = tid; idx < ST_GROUP * Ms; idx += ST_THREADS) {
            const int k = idx / Ms, s = idx - k * Ms;
            la[s * ST_GROUP + k] = idx < npts * Ms ? a[pt0 * Ms + idx] : T(0);
            lva[idx] = T(0);
        }
        for (int idx = tid; idx < ST_GROUP * two_dt; idx += ST_THREADS) {
            const int k = idx / two_dt, i = idx - k * two_dt;
            lwt[i * ST_GROUP + k] = idx < npts * two_dt ? wt[pt0 * two_dt + idx] : T(0);
            lvwt[idx] = T(0);
        }
        __syncthreads();
        // ---- W [point][j], zero beyond n
        for (int idx = tid; idx < ST_GROUP * 16 * nr; idx += ST_THREADS) {
            const int j = idx >> 6, k = idx & 63;               // (j is wavefront-uniform)
            T val = T(0);
            if (j < n) {
                const int half = j >= D ? 1 : 0, jj = j - half * D, s = jj / dt, i = jj - s * dt;
                val = la[s * ST_GROUP + k] * lwt[(half * dt + i) * ST_GROUP + k];
            }
            lw[k * ldw + j] = val;
        }
        __syncthreads();
        if (wave == 3) {                                        // fmu = W . m
            T fm = T(0);
            for (int j = 0; j < n; ++j) fm = m_fma(lw[lane * ldw + j], lm[j], fm);
            lsc[lane] = fm;
        }
        // ---- V = Sbar W, slab by slab
        T fv = T(0);
        for (int i0 = 0; i0 < n; i0 += R) {
            const int rows = n - i0 < R ? n - i0 : R;
            for (int idx = tid; idx < rows * n; idx += ST_THREADS) {          // the rows as they lie: consecutive lanes, columns
                const int r = idx / n, j = idx - r * n;
                slab[r * lds_s + j] = Sg[(long)(i0 + r) * n + j];
            }
            __syncthreads();
            for (int idx = tid; idx < rows * n; idx += ST_THREADS) {          // the columns: consecutive lanes, rows of the slab
                const int j = idx / rows, r = idx - j * rows;
                slab[r * lds_s + j] = T(0.5) * (slab[r * lds_s + j] + Sg[(long)j * n + i0 + r]);
            }
            __syncthreads();
            T v[ST_REG];
#pragma unroll
            for (int rr = 0; rr < ST_REG; ++rr) v[rr] = T(0);
            const int r0 = wave * RW;
            for (int j = 0; j < n; j += 2) {
                const T w0 = lw[lane * ldw + j], w1 = lw[lane * ldw + j + 1];
#pragma unroll
                for (int rr = 0; rr < ST_REG; ++rr) {
                    if (rr < RW) {
                        const T2 sv = *reinterpret_cast<const T2*>(&slab[(r0 + rr) * lds_s + j]);
                        v[rr] = m_fma(sv.x, w0, v[rr]);
                        v[rr] = m_fma(sv.y, w1, v[rr]);
                    }
                }
            }
#pragma unroll
            for (int rr = 0; rr < ST_REG; ++rr) {
                if (rr < RW && r0 + rr < rows) lvs[(r0 + rr) * ST_GROUP + lane] = v[rr];
            }
            __syncthreads();
            if (wave == 0) {
                for (int r = 0; r < rows; ++r) fv = m_fma(lw[lane * ldw + i0 + r], lvs[r * ST_GROUP + lane], fv);
            } else if (wave < 3 && g_a) {
                int half = i0 >= D ? 1 : 0, s = (i0 - half * D) / dt, i = i0 - half * D - s * dt;
                for (int r = 0; r < rows; ++r) {
                    const T vk = lvs[r * ST_GROUP + lane];
                    const int ia = s * ST_GROUP + lane, iw = (half * dt + i) * ST_GROUP + lane;
                    if (wave == 1) lva[ia] = m_fma(vk, lwt[iw], lva[ia]);
                    else lvwt[iw] = m_fma(vk, la[ia], lvwt[iw]);
                    if (++i == dt) {
                        i = 0;
                        if (++s == Ms) {
                            s = 0;
                            ++half;
                        }
                    }
                }
            }
        }
        // ---- the point itself
        if (wave == 0) {
            T ve = T(0), gm = T(0), gv = T(0);
            if (lane < npts) {
                const long id = pt0 + lane;
                const T mu = lsc[lane], s2 = cvar[id] + fv;
                const bool ok = s2 > T(0);                      // non-positive or NaN: NaN for this point and its segment
                if (fmu_out) fmu_out[id] = ok ? mu : nan_of<T>();
                if (fvar_out) fvar_out[id] = ok ? s2 : nan_of<T>();
                if (want_lik) {
                    if (ok) {
                        expectations<T, LIK>(q, p, mu, s2, yobs[id], ve, gm, gv);
                    } else {
                        ve = gm = gv = nan_of<T>();
                    }
                    if (g_c) g_c[id] = gv;
                    if (want & ST_WANT_SITES) gm = m_fma(T(-2) * gv, mu, gm);
                }
            }
            lsc[1 * ST_GROUP + lane] = ve;
            lsc[2 * ST_GROUP + lane] = gm;
            lsc[3 * ST_GROUP + lane] = gv;
        }
        if (!want_lik) continue;                                // projection only
        __syncthreads();
        // ---- the adjoints onto a and wt
        if (g_a) {
            for (int idx = tid; idx < ST_GROUP * Ms; idx += ST_THREADS) {
                const int k = idx & 63, s = idx >> 6;
                if (k < npts) {
                    T ma = T(0);
                    for (int half = 0; half < 2; ++half)
                        for (int i = 0; i < dt; ++i)
                            ma = m_fma(lm[half * D + s * dt + i], lwt[(half * dt + i) * ST_GROUP + k], ma);
                    const T gm = lsc[2 * ST_GROUP + k], gv = lsc[3 * ST_GROUP + k];
                    g_a[(pt0 + k) * Ms + s] = m_fma(T(2) * gv, lva[s * ST_GROUP + k], gm * ma);
                }
            }
            for (int idx = tid; idx < ST_GROUP * two_dt; idx += ST_THREADS) {
                const int k = idx & 63, qd = idx >> 6;
                if (k < npts) {
                    const int half = qd >= dt ? 1 : 0, i = qd - half * dt;
                    T mw = T(0);
                    for (int s = 0; s < Ms; ++s) mw = m_fma(lm[half * D + s * dt + i], la[s * ST_GROUP + k], mw);
                    const T gm = lsc[2 * ST_GROUP + k], gv = lsc[3 * ST_GROUP + k];
                    g_wt[(pt0 + k) * two_dt + qd] = m_fma(T(2) * gv, lvwt[qd * ST_GROUP + k], gm * mw);
                }
            }
        }
        // ---- the segment sums, point after point
        if (want) {
            for (int k = 0; k < npts; ++k) {
                if (tid == 0) accv += lsc[1 * ST_GROUP + k];
                if (want & ST_WANT_GRADS) {
                    const T gm = lsc[2 * ST_GROUP + k], gv = lsc[3 * ST_GROUP + k];
                    const T* const wk = lw + k * ldw;
                    if (tid < n) accm = m_fma(gm, wk[tid], accm);
                    T wi[ST_REG], wj[ST_REG];
#pragma unroll
                    for (int r = 0; r < ST_REG; ++r) {
                        if (r < nr) {
                            wi[r] = gv * wk[ti + 16 * r];
                            wj[r] = wk[tj + 16 * r];
                        }
                    }
#pragma unroll
                    for (int r = 0; r < ST_REG; ++r) {
                        if (r < nr) {
#pragma unroll
                            for (int c = 0; c <= r; ++c) acc[r * (r + 1) / 2 + c] = m_fma(wi[r], wj[c], acc[r * (r + 1) / 2 + c]);
                        }
                    }
                }
            }
        }
    }
    if (!want) return;
    // ---- the row: the lower triangle packed row by row, the vector, the scalar
    const long tri = (long)n * (n + 1) / 2;
    T* const row = ws + t * (tri + n + 1);
    if (want & ST_WANT_GRADS) {
#pragma unroll
        for (int r = 0; r < ST_REG; ++r) {
#pragma unroll
            for (int c = 0; c <= r; ++c) {
                const int i = ti + 16 * r, j = tj + 16 * c;
                if (i < n && j <= i) row[(long)i * (i + 1) / 2 + j] = acc[r * (r + 1) / 2 + c];
            }
        }
        if (tid < n) row[tri + tid] = accm;
    }
    if (tid == 0) row[tri + n] = accv;
}

template <typename T>
__global__ void __launch_bounds__(256) st_expect_reduce_kernel(long num_tiles, int n, const long long* __restrict__ seg_tile,
                                                               const T* __restrict__ ws, T* __restrict__ ve_sum,
                                                               T* __restrict__ g_mean, T* __restrict__ g_cov) {
    const long bs = blockIdx.x;
    long t_lo = 0, t_hi = 0;
    if (seg_tile) {                                // (NULL: no points at all)
        t_lo = (long)seg_tile[bs];
        t_hi = (long)seg_tile[bs + 1];
        clamp_range(t_lo, t_hi, num_tiles);
    }
    const long tri = (long)n * (n + 1) / 2, rowlen = tri + n + 1;
    if (g_mean) {
        for (int idx = threadIdx.x; idx < n * n; idx += 256) {
            const int i = idx / n, j = idx - i * n;
            if (j > i) continue;
            T acc = T(0);
            for (long t = t_lo; t < t_hi; ++t) acc += ws[t * rowlen + (long)i * (i + 1) / 2 + j];
            g_cov[bs * (long)n * n + (long)i * n + j] = acc;
            g_cov[bs * (long)n * n + (long)j * n + i] = acc;
        }
        for (int idx = threadIdx.x; idx < n; idx += 256) {
            T acc = T(0);
            for (long t = t_lo; t < t_hi; ++t) acc += ws[t * rowlen + tri + idx];
            g_mean[bs * n + idx] = acc;
        }
    }
    if (ve_sum && threadIdx.x == 0) {
        T acc = T(0);
        for (long t = t_lo; t < t_hi; ++t) acc += ws[t * rowlen + tri + n];
        ve_sum[bs] = acc;
    }
}

// Pass 2 of the CVI site update, one block per (series, segment): the segment's workspace rows are added in ascending row order
// from 0 (the sums of st_expect_reduce_kernel, entry by entry) - the packed lower triangle into LDS, consecutive lanes on consecutive
// entries of a row - and blended into the sites in place, nat <- fma(lr, sum, (1 - lr) nat).  nat2 is swept row by row, consecutive
// lanes on consecutive columns, one read and one write per entry; both triangles take the one sum of the lower triangle, each entry
// with its own old value.  n (n + 1) / 2 values of dynamic LDS.
template <typename T>
__global__ void __launch_bounds__(256) st_cvi_reduce_kernel(long num_tiles, int n, const long long* __restrict__ seg_tile,
                                                            const T* __restrict__ ws, T lr, T* __restrict__ nat1,
                                                            T* __restrict__ nat2, T* __restrict__ ve_sum) {
    extern __shared__ double2 st_cvi_lds_raw[];
    T* const lt = reinterpret_cast<T*>(st_cvi_lds_raw);
    const long bs = blockIdx.x;
    long t_lo = 0, t_hi = 0;
    if (seg_tile) {                                // (NULL: no points at all)
        t_lo = (long)seg_tile[bs];
        t_hi = (long)seg_tile[bs + 1];
        clamp_range(t_lo, t_hi, num_tiles);
    }
    const int tri = n * (n + 1) / 2;
    const long rowlen = (long)tri + n + 1;
    const T one_minus = T(1) - lr;
    for (int idx = threadIdx.x; idx < tri; idx += 256) {
        T acc = T(0);
        for (long t = t_lo; t < t_hi; ++t) acc += ws[t * rowlen + idx];
        lt[idx] = acc;
    }
    for (int idx = threadIdx.x; idx < n; idx += 256) {
        T acc = T(0);
        for (long t = t_lo; t < t_hi; ++t) acc += ws[t * rowlen + tri + idx];
        T* const dst = nat1 + bs * n + idx;
        *dst = m_fma(lr, acc, one_minus * *dst);
    }
    if (ve_sum && threadIdx.x == 0) {
        T acc = T(0);
        for (long t = t_lo; t < t_hi; ++t) acc += ws[t * rowlen + tri + n];
        ve_sum[bs] = acc;
    }
    __syncthreads();
    T* const dst2 = nat2 + bs * (long)n * n;
    for (int idx = threadIdx.x; idx < n * n; idx += 256) {
        const int i = idx / n, j = idx - i * n;
        const int hi = i > j ? i : j, lo = i > j ? j : i;
        dst2[idx] = m_fma(lr, lt[hi * (hi + 1) / 2 + lo], one_minus * dst2[idx]);
    }
}

inline bool st_in_range(int Ms, int two_dt) {
    return Ms >= 1 && two_dt >= 2 && !(two_dt & 1) && Ms <= ST_MAX_D && two_dt <= 2 * ST_MAX_D && Ms * (two_dt / 2) <= ST_MAX_D;
}

inline size_t st_row(int Ms, int two_dt) {
    const size_t n = size_t(Ms) * size_t(two_dt);
    return n * (n + 1) / 2 + n + 1;
}

// pass 1 on `tiles` > 0 rows: the slab height, the LDS limit and the launch
template <typename T>
int st_launch_tiles(int64_t B, int64_t N, int64_t S, int Ms, int two_dt, int lik, const Rule<T>& q, const Par<T>& p, const int64_t* seg,
                    const T* a, const T* wt, const T* c, const T* y, const T* pm, const T* pc, int64_t tiles, const int64_t* tile_seg,
                    const int64_t* seg_tile, int want, void* ws, T* g_a, T* g_wt, T* g_c, T* fmu, T* fvar, void* stream) {
    const int dt = two_dt / 2;
    int R = 32;
    while (R > 8 && size_t(st_layout(Ms, dt, R).total) * sizeof(T) > ST_LDS_LIMIT) R >>= 1;
    const size_t lds = size_t(st_layout(Ms, dt, R).total) * sizeof(T);
    if (lds > ST_LDS_LIMIT) return -100;
    return with_lik(lik, [&](auto L) {
        auto kernel = st_expect_tile_kernel<T, decltype(L)::value>;
        // past the 64 KB a kernel gets by default the limit is raised explicitly (gfx950: 160 KB per workgroup)
        if (lds > size_t(64) * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
                hipSuccess)
            return -1000;
        hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(ST_THREADS), lds, static_cast<hipStream_t>(stream), (long)N, (int)S,
                           (long)(B * S), Ms, dt, R, q, p, ll(seg), ll(tile_seg), ll(seg_tile), a, wt, c, y, pm, pc, want,
                           static_cast<T*>(ws), g_a, g_wt, g_c, fmu, fvar);
        return hipGetLastError() == hipSuccess ? 0 : -1000;
    });
}

// The CVI site update: pass 1 in the ST_WANT_SITES mode, then st_cvi_reduce_kernel.  Argument positions are those of
// mf_lik_st_cvi_site_update_*.
template <typename T>
int run_st_cvi(int64_t B, int64_t N, int64_t S, int Ms, int two_dt, int lik, const double* params, int nq, const double* nodes,
               const double* weights, const int64_t* seg, const T* a, const T* wt, const T* c, const T* y, const T* pm, const T* pc,
               int64_t tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* ws, size_t ws_bytes, double learning_rate, T* nat1,
               T* nat2, T* ve_sum, T* fmu, T* fvar, void* stream) {
    Rule<T> q;
    Par<T> p;
    int bad = check_segmentation(B, N, S);
    if (bad) return bad;
    if (!st_in_range(Ms, two_dt)) return -100;
    bad = prepare<T>(0, lik, params, nq, nodes, weights, false, q, p);          // -2 ... -6 there: arguments 6 ... 10 here
    if (bad) return bad - 4;
    if ((bad = check_tile_count(18, N, tiles))) return bad;
    if (!(learning_rate >= 0.0 && learning_rate <= 1.0)) return -23;           // (NaN fails both)
    if ((bad = first_null(24, {nat1, nat2}))) return bad;
    if (B == 0) return 0;
    if (tiles > 0) {
        if ((bad = first_null(11, {seg, a, wt, c, y, pm, pc}))) return bad;
        if ((bad = first_null(19, {tile_seg, seg_tile}))) return bad;
        if (!ws) return -21;
        if (ws_bytes < size_t(tiles) * st_row(Ms, two_dt) * sizeof(T)) return -22;
    }
    const int n = Ms * two_dt;
    const size_t lds2 = size_t(n) * (n + 1) / 2 * sizeof(T);
    auto reduce = st_cvi_reduce_kernel<T>;
    if (lds2 > size_t(64) * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(reduce), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2) != hipSuccess)
        return -1000;
    if (tiles > 0) {
        const int want = (ve_sum ? ST_WANT_VE : 0) | ST_WANT_GRADS | ST_WANT_SITES;
        const int rc = st_launch_tiles<T>(B, N, S, Ms, two_dt, lik, q, p, seg, a, wt, c, y, pm, pc, tiles, tile_seg, seg_tile, want, ws,
                                          nullptr, nullptr, nullptr, fmu, fvar, stream);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(reduce, dim3((unsigned)(B * S)), dim3(256), lds2, static_cast<hipStream_t>(stream), (long)tiles, n,
                       tiles > 0 ? ll(seg_tile) : nullptr, static_cast<const T*>(ws), T(learning_rate), nat1, nat2, ve_sum);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

template <typename T>
int run_st(int64_t B, int64_t N, int64_t S, int Ms, int two_dt, int lik, const double* params, int nq, const double* nodes,
           const double* weights, const int64_t* seg, const T* a, const T* wt, const T* c, const T* y, const T* pm, const T* pc,
           int64_t tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* ws, size_t ws_bytes, T* ve_sum, T* g_mean, T* g_cov,
           T* g_a, T* g_wt, T* g_c, T* fmu, T* fvar, void* stream) {
    Rule<T> q;
    Par<T> p;
    int bad = check_segmentation(B, N, S);
    if (bad) return bad;
    if (!st_in_range(Ms, two_dt)) return -100;
    bad = prepare<T>(0, lik, params, nq, nodes, weights, false, q, p);          // -2 ... -6 there: arguments 6 ... 10 here
    if (bad) return bad - 4;
    if ((bad = check_tile_count(18, N, tiles))) return bad;
    if (!g_mean && g_cov) return -24;
    if (g_mean && !g_cov) return -25;
    if (g_a || g_wt || g_c) {                      // all three, or none
        if ((bad = first_null(26, {g_a, g_wt, g_c}))) return bad;
    }
    const bool want_seg = ve_sum || g_mean, want_lik = want_seg || g_a;
    if (B == 0 || (!want_lik && !fmu && !fvar)) return 0;       // nothing asked for
    if (tiles > 0) {
        if ((bad = first_null(11, {seg, a, wt, c}))) return bad;
        if (want_lik && !y) return -15;
        if ((bad = first_null(16, {pm, pc}))) return bad;
        if ((bad = first_null(19, {tile_seg, seg_tile}))) return bad;
        if (want_seg) {
            if (!ws) return -21;
            if (ws_bytes < size_t(tiles) * st_row(Ms, two_dt) * sizeof(T)) return -22;
        }
    }
    const int n = Ms * two_dt;
    if (tiles > 0) {
        const int want = (ve_sum ? ST_WANT_VE : 0) | (g_mean ? ST_WANT_GRADS : 0);
        const int rc = st_launch_tiles<T>(B, N, S, Ms, two_dt, lik, q, p, seg, a, wt, c, y, pm, pc, tiles, tile_seg, seg_tile, want, ws,
                                          g_a, g_wt, g_c, fmu, fvar, stream);
        if (rc) return rc;
    }
    if (!want_seg) return 0;                       // per-point outputs only
    hipLaunchKernelGGL(st_expect_reduce_kernel<T>, dim3((unsigned)(B * S)), dim3(256), 0, static_cast<hipStream_t>(stream), (long)tiles,
                       n, tiles > 0 ? ll(seg_tile) : nullptr, static_cast<const T*>(ws), ve_sum, g_mean, g_cov);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace

extern "C" {

size_t mf_lik_st_expectations_workspace_bytes(int64_t num_tiles, int Ms, int two_dt, int elem_size) {
    if (num_tiles <= 0 || !st_in_range(Ms, two_dt) || (elem_size != 4 && elem_size != 8)) return 0;
    return size_t(num_tiles) * st_row(Ms, two_dt) * size_t(elem_size);
}

int mf_lik_st_expectations_f64(int64_t B, int64_t N, int64_t S, int Ms, int two_dt, int lik, const double* params, int nq,
                               const double* nodes, const double* weights, const int64_t* seg_offsets, const double* a,
                               const double* wt, const double* c, const double* y, const double* pair_mean, const double* pair_cov,
                               int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* workspace,
                               size_t workspace_bytes, double* ve_sum, double* g_mean, double* g_cov, double* g_a, double* g_wt,
                               double* g_c, double* fmu, double* fvar, void* stream) {
    return run_st<double>(B, N, S, Ms, two_dt, lik, params, nq, nodes, weights, seg_offsets, a, wt, c, y, pair_mean, pair_cov,
                          num_tiles, tile_seg, seg_tile, workspace, workspace_bytes, ve_sum, g_mean, g_cov, g_a, g_wt, g_c, fmu,
                          fvar, stream);
}
int mf_lik_st_expectations_f32(int64_t B, int64_t N, int64_t S, int Ms, int two_dt, int lik, const double* params, int nq,
                               const double* nodes, const double* weights, const int64_t* seg_offsets, const float* a,
                               const float* wt, const float* c, const float* y, const float* pair_mean, const float* pair_cov,
                               int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* workspace,
                               size_t workspace_bytes, float* ve_sum, float* g_mean, float* g_cov, float* g_a, float* g_wt,
                               float* g_c, float* fmu, float* fvar, void* stream) {
    return run_st<float>(B, N, S, Ms, two_dt, lik, params, nq, nodes, weights, seg_offsets, a, wt, c, y, pair_mean, pair_cov,
                         num_tiles, tile_seg, seg_tile, workspace, workspace_bytes, ve_sum, g_mean, g_cov, g_a, g_wt, g_c, fmu, fvar,
                         stream);
}

size_t mf_lik_st_cvi_site_update_workspace_bytes(int64_t num_tiles, int Ms, int two_dt, int elem_size) {
    return mf_lik_st_expectations_workspace_bytes(num_tiles, Ms, two_dt, elem_size);      // the same rows
}

int mf_lik_st_cvi_site_update_f64(int64_t B, int64_t N, int64_t S, int Ms, int two_dt, int lik, const double* params, int nq,
                                  const double* nodes, const double* weights, const int64_t* seg_offsets, const double* a,
                                  const double* wt, const double* c, const double* y, const double* pair_mean,
                                  const double* pair_cov, int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile,
                                  void* workspace, size_t workspace_bytes, double learning_rate, double* nat1, double* nat2,
                                  double* ve_sum, double* fmu, double* fvar, void* stream) {
    return run_st_cvi<double>(B, N, S, Ms, two_dt, lik, params, nq, nodes, weights, seg_offsets, a, wt, c, y, pair_mean, pair_cov,
                              num_tiles, tile_seg, seg_tile, workspace, workspace_bytes, learning_rate, nat1, nat2, ve_sum, fmu, fvar,
                              stream);
}
int mf_lik_st_cvi_site_update_f32(int64_t B, int64_t N, int64_t S, int Ms, int two_dt, int lik, const double* params, int nq,
                                  const double* nodes, const double* weights, const int64_t* seg_offsets, const float* a,
                                  const float* wt, const float* c, const float* y, const float* pair_mean, const float* pair_cov,
                                  int64_t num_tiles, const int64_t* tile_seg, const int64_t* seg_tile, void* workspace,
                                  size_t workspace_bytes, float learning_rate, float* nat1, float* nat2, float* ve_sum, float* fmu,
                                  float* fvar, void* stream) {
    return run_st_cvi<float>(B, N, S, Ms, two_dt, lik, params, nq, nodes, weights, seg_offsets, a, wt, c, y, pair_mean, pair_cov,
                             num_tiles, tile_seg, seg_tile, workspace, workspace_bytes, learning_rate, nat1, nat2, ve_sum, fmu, fvar,
                             stream);
}

}  // extern "C"
