// Transitions of the LatentExponentiallyGenerated kernel (markovflow/kernels/latent_exp_generated.py): per (series, step)
//     A = expm(dt F),  Q = I - A A^T + jitter I,  chol Q          F [d, d] shared or [B, d, d] per series, 1 <= d <= 16
// and the reverse mode, the gradient of  sum_k <gA_k, A_k> + <gC_k, chol Q_k>  with respect to F.  The arithmetic - scaling and
// squaring with expm - I carried through the squarings, the Cholesky factorisation and its adjoint, the Frechet derivative - is
// mf_leg_math.hpp, written against a group of lanes; this file supplies the group and the memory plumbing.
//
// Mapping: GW = the power of two >= d lanes form a group = one step, lane r of the group holds row r of every matrix in d
// registers; a wavefront works on 64 / GW steps at once.  A lane reads another row through ONE data-parallel move whose lane
// select is an immediate: quad_perm for GW <= 4, row_newbcast for GW = 16, two row_newbcast and a select for GW = 8.  The
// moves come from the compiler's builtin, so it places the wait states itself.  A d x d x d product is d*d moves and
// fused multiply-adds per lane; three live 16 x 16 double matrices are 96 registers a lane, not the 1536 of a lane per step.
//
// Steps of one wavefront need different numbers of squarings: the loops run to the wavefront's largest count and every step
// selects (mf_leg_math.hpp), so no cross-lane move sits under divergent control flow.  Outputs are staged per wavefront in LDS
// and leave as coalesced stores, as in sde_transitions_kernel (mf_sde.hip); the same tiles serve the two transpositions.
#include "../../include/markovflow_amd.h"

#include <hip/hip_runtime.h>

#include "mf_leg_math.hpp"

namespace {
using namespace mf;

constexpr int LEG_MAX_D = 16;
constexpr int LEG_STEPS_PER_GROUP = 8;        // reverse mode: consecutive rounds of a block, folded in registers (not tuned)

template <int CTRL> MF_DEV float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int CTRL> MF_DEV double dpp_mov(double v) {
    const unsigned long long x = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)x, CTRL, 0xf, 0xf, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(x >> 32), CTRL, 0xf, 0xf, true);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

constexpr int group_width(int d) { return d <= 1 ? 1 : d <= 2 ? 2 : d <= 4 ? 4 : d <= 8 ? 8 : 16; }

template <typename T_, int D_> struct DevGroup {
    using T = T_;
    static constexpr int D = D_, W = 1, GW = group_width(D_), TS = (D_ * D_) | 1;
    int r;          // lane's row
    T* tile;        // the group's LDS tile, TS elements

    MF_DEV int row(int) const { return r; }
    template <int K> MF_DEV T bc(const T (&m)[1][D], int j) const {
        static_assert(K < D, "broadcast from a lane without a row");
        if constexpr (GW == 1) return m[0][j];
        else if constexpr (GW == 2) return dpp_mov<K | (K << 2) | ((2 + K) << 4) | ((2 + K) << 6)>(m[0][j]);
        else if constexpr (GW == 4) return dpp_mov<K | (K << 2) | (K << 4) | (K << 6)>(m[0][j]);
        else if constexpr (GW == 8) {
            const T lo = dpp_mov<0x150 + K>(m[0][j]), hi = dpp_mov<0x150 + K + 8>(m[0][j]);
            return (threadIdx.x & 8) ? hi : lo;
        } else return dpp_mov<0x150 + K>(m[0][j]);
    }
    MF_DEV T max(const T (&v)[1]) const {
        T a = v[0];
        MF_UNROLL for (int m = GW / 2; m >= 1; m >>= 1) { const T o = __shfl_xor(a, m); a = o > a ? o : a; }
        return a;
    }
    MF_DEV bool all(const bool (&v)[1]) const {
        int a = v[0] ? 1 : 0;
        MF_UNROLL for (int m = GW / 2; m >= 1; m >>= 1) a &= __shfl_xor(a, m);
        return a != 0;
    }
    MF_DEV void transpose(const T (&m)[1][D], T (&out)[1][D]) const {
        if (r < D) { MF_UNROLL for (int j = 0; j < D; ++j) tile[r * D + j] = m[0][j]; }
        __syncthreads();
        MF_UNROLL for (int j = 0; j < D; ++j) out[0][j] = r < D ? tile[j * D + r] : T(0);
        __syncthreads();
    }
};

MF_DEV int wave_max(int v) {
    MF_UNROLL for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(v, m); v = o > v ? o : v; }
    return __builtin_amdgcn_readfirstlane(v);
}

// the wavefront's tiles of one output -> global memory, coalesced (the steps of a wavefront are contiguous in [B, n, d, d])
template <class G> MF_DEV void store_tiles(const G& g, const typename G::T (&m)[1][G::D], typename G::T* __restrict__ buf,
                                           typename G::T* __restrict__ dst, long base, long total) {
    constexpr int D = G::D, dd = D * D, SPW = 64 / G::GW;
    if (g.r < D) { MF_UNROLL for (int j = 0; j < D; ++j) g.tile[g.r * D + j] = m[0][j]; }
    __syncthreads();
    long nvalid = total - base;
    if (nvalid > SPW) nvalid = SPW;
    const int count = (int)nvalid * dd;
    typename G::T* gdst = dst + base * dd;
    for (int e = threadIdx.x; e < count; e += 64) gdst[e] = buf[(e / dd) * G::TS + (e % dd)];
    __syncthreads();
}

// rows of F and of F^T of a series into the lane's registers (lanes without a row: zero)
template <class G> MF_DEV void load_feedback(const G& g, const typename G::T* __restrict__ Fp, typename G::T (&Fr)[1][G::D],
                                             typename G::T (&Ft)[1][G::D]) {
    constexpr int D = G::D;
    MF_UNROLL for (int j = 0; j < D; ++j) {
        Fr[0][j] = g.r < D ? Fp[g.r * D + j] : typename G::T(0);
        Ft[0][j] = g.r < D ? Fp[j * D + g.r] : typename G::T(0);
    }
}

template <typename T, int D>
__global__ void __launch_bounds__(64) leg_transitions_kernel(long total, long n, const T* __restrict__ F, long fstride,
                                                             const T* __restrict__ dt, T jitter, T* __restrict__ A,
                                                             T* __restrict__ cholQ, T* __restrict__ Q) {
    using G = DevGroup<T, D>;
    constexpr int GW = G::GW, SPW = 64 / GW;
    __shared__ T buf[SPW * G::TS];
    const int lane = threadIdx.x, grp = lane / GW;
    G g{lane % GW, buf + grp * G::TS};
    const long base = (long)blockIdx.x * SPW, id = base + grp;
    const bool valid = id < total;
    const long series = valid ? id / n : 0;
    const T delta = valid ? dt[id] : T(0);
    T Fr[1][D], Ft[1][D], Y[1][D], E[1][D], M[1][D];
    load_feedback<G>(g, F + series * fstride, Fr, Ft);
    const int s = leg::scaled_argument<G>(Fr, leg::norm1_of_transposed<G>(g, Ft), delta, Y);
    const int smax = wave_max(s);
    leg::expm1_scaled<G>(g, Y, s, smax, E);
    leg::transition_of<G>(g, E, M);
    store_tiles<G>(g, M, buf, A, base, total);
    if (!cholQ && !Q) return;
    leg::process_covariance<G>(g, E, jitter, leg::is_skew<G>(g, Fr, Ft), M);
    if (Q) store_tiles<G>(g, M, buf, Q, base, total);
    if (!cholQ) return;
    bool zero;
    leg::cholesky<G>(g, M, E, zero);
    leg::zero_factor<G>(zero, E);
    store_tiles<G>(g, E, buf, cholQ, base, total);
}

// Reverse mode, launch 1 of 2: a block = one wavefront takes LEG_STEPS_PER_GROUP rounds of 64 / GW consecutive steps of ONE
// series; every group adds dt L_exp(dt F^T; G) of its steps in registers, in step order, then the block folds its groups in
// group order into one d x d record.  Launch 2 adds a series' records in block order: a fixed order throughout, no atomics.
template <typename T, int D>
__global__ void __launch_bounds__(64) leg_grad_steps_kernel(long n, long nblk, const T* __restrict__ F, long fstride,
                                                            const T* __restrict__ dt, T jitter, const T* __restrict__ gA,
                                                            const T* __restrict__ gC, T* __restrict__ rec) {
    using G = DevGroup<T, D>;
    constexpr int GW = G::GW, SPW = 64 / GW, dd = D * D;
    __shared__ T buf[SPW * G::TS];
    const int lane = threadIdx.x, grp = lane / GW;
    G g{lane % GW, buf + grp * G::TS};
    const long blk = blockIdx.x, b = blk / nblk, c = blk % nblk;
    T Fr[1][D], Ft[1][D], acc[1][D];
    load_feedback<G>(g, F + b * fstride, Fr, Ft);
    const T norm1 = leg::norm1_of_transposed<G>(g, Ft);
    const bool lossless = leg::is_skew<G>(g, Fr, Ft);
    MF_UNROLL for (int j = 0; j < D; ++j) acc[0][j] = T(0);
#pragma nounroll
    for (int it = 0; it < LEG_STEPS_PER_GROUP; ++it) {
        const long step = (c * LEG_STEPS_PER_GROUP + it) * SPW + grp;
        if ((c * LEG_STEPS_PER_GROUP + it) * SPW >= n) break;            // (uniform over the wavefront)
        const bool valid = step < n;
        const long id = b * n + (valid ? step : 0);
        const T delta = valid ? dt[id] : T(0);
        T Y[1][D], E[1][D], Aa[1][D], Qm[1][D], L[1][D], ga[1][D], gc[1][D];
        MF_UNROLL for (int j = 0; j < D; ++j) {
            const bool in = valid && g.r < D;
            ga[0][j] = (in && gA) ? gA[id * dd + g.r * D + j] : T(0);
            gc[0][j] = (in && gC) ? gC[id * dd + g.r * D + j] : T(0);
        }
        const int s = leg::scaled_argument<G>(Fr, norm1, delta, Y);
        const int smax = wave_max(s);
        leg::expm1_scaled<G>(g, Y, s, smax, E);
        leg::transition_of<G>(g, E, Aa);
        leg::process_covariance<G>(g, E, jitter, lossless, Qm);
        bool zero;
        leg::cholesky<G>(g, Qm, L, zero);
        leg::adjoint_seed<G>(g, Aa, L, zero, ga, gc, Qm);                 // Qm: the seed G
        MF_UNROLL for (int j = 0; j < D; ++j) Qm[0][j] = leg::t_ldexp<T>(Qm[0][j], -s);
        (void)leg::scaled_argument<G>(Ft, norm1, delta, Y);
        leg::frechet_scaled<G>(g, Y, Qm, s, smax, E);
        MF_UNROLL for (int j = 0; j < D; ++j) acc[0][j] = valid ? leg::t_fma<T>(delta, E[0][j], acc[0][j]) : acc[0][j];
    }
    if (g.r < D) { MF_UNROLL for (int j = 0; j < D; ++j) g.tile[g.r * D + j] = acc[0][j]; }
    __syncthreads();
    for (int e = lane; e < dd; e += 64) {
        T a = buf[e];
        for (int q = 1; q < SPW; ++q) a += buf[q * G::TS + e];
        rec[blk * dd + e] = a;
    }
}

template <typename T>
__global__ void __launch_bounds__(64) leg_grad_reduce_kernel(long B, long nblk, int dd, const T* __restrict__ rec, T* __restrict__ out) {
    const long id = (long)blockIdx.x * 64 + threadIdx.x;
    if (id >= B * dd) return;
    const long b = id / dd;
    const int e = (int)(id % dd);
    T a = T(0);
    for (long k = 0; k < nblk; ++k) a += rec[(b * nblk + k) * dd + e];
    out[id] = a;
}

inline long leg_grad_blocks(int64_t n, int d) {
    const long per = (long)(64 / group_width(d)) * LEG_STEPS_PER_GROUP;
    return (long)((n + per - 1) / per);
}

template <typename T, int D>
void launch_fwd(long total, long n, const T* F, long fstride, const T* dt, T jitter, T* A, T* cholQ, T* Q, hipStream_t st) {
    constexpr int SPW = 64 / group_width(D);
    hipLaunchKernelGGL((leg_transitions_kernel<T, D>), dim3((unsigned)((total + SPW - 1) / SPW)), dim3(64), 0, st, total, n, F,
                       fstride, dt, jitter, A, cholQ, Q);
}
template <typename T, int D>
void launch_grad(long B, long n, long nblk, const T* F, long fstride, const T* dt, T jitter, const T* gA, const T* gC, T* rec,
                 hipStream_t st) {
    hipLaunchKernelGGL((leg_grad_steps_kernel<T, D>), dim3((unsigned)(B * nblk)), dim3(64), 0, st, n, nblk, F, fstride, dt, jitter,
                       gA, gC, rec);
}

#define LEG_DISPATCH(d, CALL)                                                                                                      \
    switch (d) {                                                                                                                   \
        case 1: CALL(1); break;   case 2: CALL(2); break;   case 3: CALL(3); break;   case 4: CALL(4); break;                      \
        case 5: CALL(5); break;   case 6: CALL(6); break;   case 7: CALL(7); break;   case 8: CALL(8); break;                      \
        case 9: CALL(9); break;   case 10: CALL(10); break; case 11: CALL(11); break; case 12: CALL(12); break;                    \
        case 13: CALL(13); break; case 14: CALL(14); break; case 15: CALL(15); break; case 16: CALL(16); break;                    \
        default: return -100;                                                                                                      \
    }

// argument checks shared by the two entry points (the positions coincide up to `jitter`): 0, the negative position, or -100
inline int leg_spec(int64_t B, int64_t n, int d, const void* F, const void* dt, bool& empty) {
    if (B < 0) return -1;
    if (n < 0) return -2;
    if (d < 1) return -3;
    if (d > LEG_MAX_D) return -100;
    empty = B == 0 || n == 0;
    if (empty) return 0;
    if (!F) return -4;
    if (!dt) return -6;
    return 0;
}

template <typename T>
int run_leg(int64_t B, int64_t n, int d, const T* F, int per_series, const T* dt, T jitter, T* A, T* cholQ, T* Q, void* stream) {
    bool empty = false;
    const int bad = leg_spec(B, n, d, F, dt, empty);
    if (bad) return bad;
    if (empty) return 0;
    if (!A) return -8;
    const long fstride = per_series ? (long)d * d : 0L;
    hipStream_t st = static_cast<hipStream_t>(stream);
#define LEG_FWD(DD) launch_fwd<T, DD>((long)(B * n), (long)n, F, fstride, dt, jitter, A, cholQ, Q, st)
    LEG_DISPATCH(d, LEG_FWD)
#undef LEG_FWD
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

inline size_t leg_grad_workspace(int64_t B, int64_t n, int d, size_t elem) {
    if (B <= 0 || n <= 0 || d < 1 || d > LEG_MAX_D) return 0;
    return size_t(B) * size_t(leg_grad_blocks(n, d)) * size_t(d) * size_t(d) * elem;
}

template <typename T>
int run_leg_grad(int64_t B, int64_t n, int d, const T* F, int per_series, const T* dt, T jitter, const T* gA, const T* gC, T* out,
                 void* ws, size_t ws_bytes, void* stream) {
    bool empty = false;
    const int bad = leg_spec(B, n, d, F, dt, empty);
    if (bad) return bad;
    if (empty) return 0;
    if (!out) return -10;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!ws) return -11;
    if (ws_bytes < leg_grad_workspace(B, n, d, sizeof(T))) return -12;
    const long fstride = per_series ? (long)d * d : 0L;
    const long nblk = leg_grad_blocks(n, d);
    T* rec = static_cast<T*>(ws);
#define LEG_GRAD(DD) launch_grad<T, DD>((long)B, (long)n, nblk, F, fstride, dt, jitter, gA, gC, rec, st)
    LEG_DISPATCH(d, LEG_GRAD)
#undef LEG_GRAD
    if (hipGetLastError() != hipSuccess) return -1000;
    const long threads = (long)B * d * d;
    hipLaunchKernelGGL((leg_grad_reduce_kernel<T>), dim3((unsigned)((threads + 63) / 64)), dim3(64), 0, st, (long)B, nblk, d * d,
                       rec, out);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}
}   // namespace

extern "C" {
int mf_sde_leg_transitions_f64(int64_t B, int64_t n, int d, const double* F, int per_series, const double* dt, double jitter,
                               double* A, double* cholQ, double* Q, void* stream) {
    return run_leg<double>(B, n, d, F, per_series, dt, jitter, A, cholQ, Q, stream);
}
int mf_sde_leg_transitions_f32(int64_t B, int64_t n, int d, const float* F, int per_series, const float* dt, float jitter, float* A,
                               float* cholQ, float* Q, void* stream) {
    return run_leg<float>(B, n, d, F, per_series, dt, jitter, A, cholQ, Q, stream);
}
size_t mf_sde_leg_transitions_grad_workspace_bytes(int64_t B, int64_t n, int d, int elem_size) {
    return leg_grad_workspace(B, n, d, (size_t)elem_size);
}
int mf_sde_leg_transitions_grad_f64(int64_t B, int64_t n, int d, const double* F, int per_series, const double* dt, double jitter,
                                    const double* gA, const double* gC, double* out, void* ws, size_t ws_bytes, void* stream) {
    return run_leg_grad<double>(B, n, d, F, per_series, dt, jitter, gA, gC, out, ws, ws_bytes, stream);
}
int mf_sde_leg_transitions_grad_f32(int64_t B, int64_t n, int d, const float* F, int per_series, const float* dt, float jitter,
                                    const float* gA, const float* gC, float* out, void* ws, size_t ws_bytes, void* stream) {
    return run_leg_grad<float>(B, n, d, F, per_series, dt, jitter, gA, gC, out, ws, ws_bytes, stream);
}
}
