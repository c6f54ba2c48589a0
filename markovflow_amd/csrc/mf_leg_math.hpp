// Arithmetic of the LatentExponentiallyGenerated transition generator (markovflow/kernels/latent_exp_generated.py; Loper et al.
// 2020): F = -(N N^T + R - R^T) / 2, P_inf = I, and per (series, step) with X = dt F
//     A = expm(X),   Q = I - A A^T + jitter I,   chol Q
// and the reverse mode  d/dF of  <gA, A> + <gC, chol Q>.
//
// The matrix exponential is scaling and squaring around a Taylor polynomial: Y = X 2^-s with ||Y||_1 <= 1/2, degree 8 (float) or
// 15 (double) - remainder (1/2)^(m+1) / (m+1)! = 5e-9 / 7e-19 - then s squarings.  What is carried through the squarings is
// E = expm(.) - I  (E <- 2 E + E E), never expm itself, so that
//     Q = -(E + E^T + E E^T) + jitter I
// has no cancellation for a short gap, where I - A A^T loses eps / dt (float: a relative error of 1e-3 at dt = 1e-5, or no factor
// at all); A = I + E only at the very end.
//
// Layout: a GROUP of lanes shares one step, lane r holds row r of every D x D matrix in D registers.  Everything is written
// against a group type G that says how a lane reaches the other rows:
//     G::T, G::D, G::W               element type, state dimension, rows held HERE (device: 1, the lane's own; host: all D)
//     g.row(w)                       the matrix row that local row w is (device: the lane's index in its group)
//     g.template bc<K>(M, j)         M[K][j]: register j of the lane that holds row K (device: one DPP broadcast)
//     g.max(v), g.all(v)             reductions over the group's rows
//     g.transpose(M, out)            out = M^T (device: through the group's LDS tile)
// tests/host_sim/leg_sim.cpp supplies the host group and runs these very functions against the long-double reference; the
// device group is in mf_leg.hip.  Rules that keep both executions the same: a function never writes a matrix it broadcasts
// from inside the same loop over rows, and no broadcast sits under control flow that depends on the step (the squarings run to
// the largest count `smax` of the wavefront and every step selects its own).
#pragma once
#include <type_traits>
#include <utility>

#include "mf_small.hpp"

// On the device everything is inlined and unrolled (registers need static indices); the host build, whose group holds all D rows,
// keeps its loops - unrolled it is a hundred thousand multiply-adds per step function and minutes of compilation.
#if defined(__HIP_DEVICE_COMPILE__)
#define MF_LEG_HD __host__ __device__ __forceinline__
#define MF_LEG_UNROLL _Pragma("unroll")
#else
#define MF_LEG_HD __host__ __device__ inline
#define MF_LEG_UNROLL
#endif

namespace mf {
namespace leg {

template <int N, typename F, int... I> MF_LEG_HD void sfor_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
// f(integral_constant<int, i>) for i = 0..N-1 (the lane a broadcast reads is an immediate)
template <int N, typename F> MF_LEG_HD void sfor(F&& f) {
    if constexpr (N > 0) sfor_impl<N>(f, std::make_integer_sequence<int, N>{});
}

// The products below are issued one broadcast lane at a time: without a fence the scheduler hoists all D*D broadcasts of a product
// ahead of the multiply-adds and every one of them holds a register (d = 16, double: past the register file, into scratch).
#if defined(__HIP_DEVICE_COMPILE__)
#define MF_LEG_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define MF_LEG_FENCE() ((void)0)
#endif

template <typename T> struct Degree;
template <> struct Degree<float> { static constexpr int value = 8; };
template <> struct Degree<double> { static constexpr int value = 15; };

template <typename T> MF_LEG_HD T t_fma(T a, T b, T c);
template <> MF_LEG_HD float t_fma<float>(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
template <> MF_LEG_HD double t_fma<double>(double a, double b, double c) { return __builtin_fma(a, b, c); }
template <typename T> MF_LEG_HD T t_ldexp(T x, int e);
template <> MF_LEG_HD float t_ldexp<float>(float x, int e) { return __builtin_ldexpf(x, e); }
template <> MF_LEG_HD double t_ldexp<double>(double x, int e) { return __builtin_ldexp(x, e); }
template <typename T> MF_LEG_HD T t_nan();
template <> MF_LEG_HD float t_nan<float>() { return __builtin_nanf(""); }
template <> MF_LEG_HD double t_nan<double>() { return __builtin_nan(""); }
template <typename T> MF_LEG_HD bool t_finite(T x) { return __builtin_fabs((double)x) <= 1.7976931348623157e308 && x == x; }

// the number of squarings for ||X||_1 = norm: the smallest s >= 0 with norm 2^-s <= 1/2.  Bounded by the exponent range of T
// (130 / 1026); a norm that is not finite gives 0 - the caller poisons such a step instead of scaling it.
template <typename T> MF_LEG_HD int scale_count(T norm) {
    if (!(norm > T(0.5)) || !t_finite(norm)) return 0;
    int e = 0;
    if constexpr (std::is_same<T, float>::value) (void)__builtin_frexpf(norm, &e); else (void)__builtin_frexp(norm, &e);
    return e + 1;                                   // norm = m 2^e, m in [1/2, 1)
}

template <class G> using Mat = typename G::T[G::W][G::D];

template <class G> MF_LEG_HD void copy(const Mat<G>& a, Mat<G>& out) {
    MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) out[w][j] = a[w][j];
}
// out = P Q
template <class G> MF_LEG_HD void mul(const G& g, const Mat<G>& P, const Mat<G>& Q, Mat<G>& out) {
    using T = typename G::T;
    MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) out[w][j] = T(0);
    sfor<G::D>([&](auto k) {
        constexpr int kk = decltype(k)::value;
        MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) {
            const T q = g.template bc<kk>(Q, j);
            MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) out[w][j] = t_fma<T>(P[w][kk], q, out[w][j]);
        }
        MF_LEG_FENCE();
    });
}
// out = P Q^T
template <class G> MF_LEG_HD void mul_t(const G& g, const Mat<G>& P, const Mat<G>& Q, Mat<G>& out) {
    using T = typename G::T;
    MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) out[w][j] = T(0);
    sfor<G::D>([&](auto j) {
        constexpr int jj = decltype(j)::value;
        MF_LEG_UNROLL for (int k = 0; k < G::D; ++k) {
            const T q = g.template bc<jj>(Q, k);
            MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) out[w][jj] = t_fma<T>(P[w][k], q, out[w][jj]);
        }
        MF_LEG_FENCE();
    });
}

// ||F||_1, the largest absolute column sum, from the rows of F^T
template <class G> MF_LEG_HD typename G::T norm1_of_transposed(const G& g, const Mat<G>& Ft) {
    using T = typename G::T;
    T v[G::W];
    MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) {
        v[w] = T(0);
        MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) v[w] += Ft[w][j] < T(0) ? -Ft[w][j] : Ft[w][j];
        v[w] = v[w] == v[w] ? v[w] : T(1) / T(0);          // (a NaN must not get lost in the maximum)
    }
    return g.max(v);
}

// Y = dt M 2^-s for M = F or F^T with s = scale_count(|dt| ||F||_1), returned.  Where dt F is not finite Y is NaN throughout:
// every output of that step is NaN and no trip count depends on it.
template <class G> MF_LEG_HD int scaled_argument(const Mat<G>& M, typename G::T norm1, typename G::T dt, Mat<G>& Y) {
    using T = typename G::T;
    const T norm = (dt < T(0) ? -dt : dt) * norm1;
    const bool ok = t_finite(norm);
    const int s = scale_count<T>(norm);
    MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j)
        Y[w][j] = ok ? t_ldexp<T>(dt * M[w][j], -s) : t_nan<T>();
    return s;
}

// E = expm(Y 2^s) - I from the scaled Y: the Taylor terms, then `smax` squaring rounds of which this step takes the first s
template <class G> MF_LEG_HD void expm1_scaled(const G& g, const Mat<G>& Y, int s, int smax, Mat<G>& E) {
    using T = typename G::T;
    Mat<G> Tk, Tn;
    copy<G>(Y, Tk);
    copy<G>(Y, E);
#pragma nounroll
    for (int k = 2; k <= Degree<T>::value; ++k) {
        mul<G>(g, Y, Tk, Tn);          // (Y T_k, not T_k Y: a broadcast of the loop-invariant Y would be hoisted, all D*D of it)
        const T inv = T(1) / T(k);
        MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) {
            Tk[w][j] = Tn[w][j] * inv;
            E[w][j] += Tk[w][j];
        }
    }
#pragma nounroll
    for (int t = 0; t < smax; ++t) {
        // A step past its own count squares a zero matrix and adds itself back: plain data flow.  (A select of the finished
        // product is turned into a branch around the multiply-adds, across which all D*D broadcasts stay live.)
        const bool on = t < s;
        MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) Tk[w][j] = on ? E[w][j] : T(0);
        mul<G>(g, Tk, E, Tn);
        MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j)
            E[w][j] = t_fma<T>(T(2), Tk[w][j], Tn[w][j]) + (on ? T(0) : E[w][j]);
    }
}

// A = I + E
template <class G> MF_LEG_HD void transition_of(const G& g, const Mat<G>& E, Mat<G>& A) {
    using T = typename G::T;
    MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j)
        A[w][j] = E[w][j] + (g.row(w) == j ? T(1) : T(0));
}

// true when F + F^T is exactly zero (N = 0): expm(dt F) is orthogonal and the process noise vanishes identically
template <class G> MF_LEG_HD bool is_skew(const G& g, const Mat<G>& F, const Mat<G>& Ft) {
    using T = typename G::T;
    bool z[G::W];
    MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) {
        z[w] = true;
        MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) z[w] &= (F[w][j] + Ft[w][j] == T(0));
    }
    return g.all(z);
}

// Q = -(E + E^T + E E^T) + jitter I, exactly symmetric: with M = E + E E^T / 2 it is -(M + M^T).  For a skew F (`lossless`) the
// bracket is zero in exact arithmetic and is taken as such - by a product with 0 / 1, so that a NaN step stays NaN.
template <class G>
MF_LEG_HD void process_covariance(const G& g, const Mat<G>& E, typename G::T jitter, bool lossless, Mat<G>& Q) {
    using T = typename G::T;
    Mat<G> M, Mt;
    mul_t<G>(g, E, E, M);
    MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) M[w][j] = t_fma<T>(T(0.5), M[w][j], E[w][j]);
    g.transpose(M, Mt);
    const T keep = lossless ? T(0) : T(1);
    MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j)
        Q[w][j] = keep * -(M[w][j] + Mt[w][j]) + (g.row(w) == j ? jitter : T(0));
}

// L = chol Q, right-looking (Q is consumed).  comp_chol's convention (mf_sde.hip): a non-positive pivot gives NaN through the
// square root, the upper triangle is exactly zero, and an all-zero Q is reported (`zero`) - it is factorised as if it were I, so
// that the adjoint's solves stay finite; zero_factor() turns that into the zero factor that is passed on.
template <class G> MF_LEG_HD void cholesky(const G& g, Mat<G>& Q, Mat<G>& L, bool& zero) {
    using T = typename G::T;
    bool z[G::W];
    MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) {
        z[w] = true;
        MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) z[w] &= (Q[w][j] == T(0));
    }
    zero = g.all(z);
    MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j)
        Q[w][j] = (zero && g.row(w) == j) ? T(1) : Q[w][j];
    sfor<G::D>([&](auto j) {
        constexpr int jj = decltype(j)::value;
        const T ljj = t_sqrt<T>(g.template bc<jj>(Q, jj));
        const T inv = T(1) / ljj;
        MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) {
            const int r = g.row(w);
            L[w][jj] = r > jj ? Q[w][jj] * inv : (r == jj ? ljj : T(0));
        }
        sfor<G::D>([&](auto k) {
            constexpr int kk = decltype(k)::value;
            if constexpr (kk > jj) {
                const T lk = g.template bc<kk>(L, jj);
                MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) Q[w][kk] = t_fma<T>(-L[w][jj], lk, Q[w][kk]);
            }
        });
        MF_LEG_FENCE();
    });
}
// the factor that leaves: exact zeros for an all-zero Q (a product with 0 / 1, not a select of the factorisation's result)
template <class G> MF_LEG_HD void zero_factor(bool zero, Mat<G>& L) {
    using T = typename G::T;
    const T keep = zero ? T(0) : T(1);
    MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) L[w][j] *= keep;
}

// The seed of the exponential's adjoint: G = gA - 2 gQ A, where gQ = L^-T sym(Phi(L^T tril(gC))) L^-1 is the Cholesky
// factorisation's reverse mode (Phi: lower triangle, diagonal halved) - zero for a step whose Q is all zero.
// Only the lower triangle of gC is read.
template <class G>
MF_LEG_HD void adjoint_seed(const G& g, const Mat<G>& A, const Mat<G>& L, bool zero, const Mat<G>& gA, const Mat<G>& gC, Mat<G>& Gs) {
    using T = typename G::T;
    Mat<G> LT, P, Pt, U;
    g.transpose(L, LT);
    MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) U[w][j] = j <= g.row(w) ? gC[w][j] : T(0);
    mul<G>(g, LT, U, P);
    MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) {
        const int r = g.row(w);
        P[w][j] = j < r ? P[w][j] : (j == r ? T(0.5) * P[w][j] : T(0));
    }
    g.transpose(P, Pt);
    MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) P[w][j] = T(0.5) * (P[w][j] + Pt[w][j]);
    // U = P L^-1: every row solves  u L = p  from the last column back
    sfor<G::D>([&](auto jr) {
        constexpr int jj = G::D - 1 - decltype(jr)::value;
        const T inv = T(1) / g.template bc<jj>(L, jj);
        MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) U[w][jj] = P[w][jj] * inv;
        MF_LEG_UNROLL for (int k = 0; k < jj; ++k) {
            const T l = g.template bc<jj>(L, k);
            MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) P[w][k] = t_fma<T>(-U[w][jj], l, P[w][k]);
        }
        MF_LEG_FENCE();
    });
    // gQ = L^-T U in place: row i is final once the rows below it have been eliminated
    sfor<G::D>([&](auto ir) {
        constexpr int ii = G::D - 1 - decltype(ir)::value;
        const T inv = T(1) / g.template bc<ii>(L, ii);
        MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j)
            U[w][j] = g.row(w) == ii ? U[w][j] * inv : U[w][j];
        MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) {
            const T sj = g.template bc<ii>(U, j);
            MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) P[w][j] = g.row(w) < ii ? t_fma<T>(-LT[w][ii], sj, U[w][j]) : U[w][j];
        }
        copy<G>(P, U);
        MF_LEG_FENCE();
    });
    const T keep = zero ? T(0) : T(1);               // (L is cholesky()'s factor, I for an all-zero Q: U is finite there)
    MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) U[w][j] *= keep;
    mul<G>(g, U, A, P);
    MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) Gs[w][j] = t_fma<T>(T(-2), P[w][j], gA[w][j]);
}

// Lx = L_exp(Z 2^s; Gd 2^s): the Frechet derivative of the exponential at the scaled Z in the scaled direction Gd - the
// derivative recurrences D_k = (Z D_{k-1} + Gd T_{k-1}) / k beside the Taylor terms T_k, then per squaring
// Lx <- B Lx + Lx B = 2 Lx + Eb Lx + Lx Eb  with B = I + Eb the exponential so far.  With Z = (Y)^T this is the adjoint of expm at Y.
template <class G> MF_LEG_HD void frechet_scaled(const G& g, const Mat<G>& Z, const Mat<G>& Gd, int s, int smax, Mat<G>& Lx) {
    using T = typename G::T;
    Mat<G> Tk, Dk, Eb, Tn, Dn;
    copy<G>(Z, Tk);
    copy<G>(Z, Eb);
    copy<G>(Gd, Dk);
    copy<G>(Gd, Lx);
#pragma nounroll
    for (int k = 2; k <= Degree<T>::value; ++k) {
        const T inv = T(1) / T(k);
        mul<G>(g, Z, Dk, Dn);
        mul<G>(g, Gd, Tk, Tn);
        MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) {
            Dk[w][j] = (Dn[w][j] + Tn[w][j]) * inv;
            Lx[w][j] += Dk[w][j];
        }
        mul<G>(g, Z, Tk, Tn);
        MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) {
            Tk[w][j] = Tn[w][j] * inv;
            Eb[w][j] += Tk[w][j];
        }
    }
#pragma nounroll
    for (int t = 0; t < smax; ++t) {
        const bool on = t < s;                       // (masked operands, no select of a product: see expm1_scaled)
        MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j) {
            Tk[w][j] = on ? Eb[w][j] : T(0);
            Dk[w][j] = on ? Lx[w][j] : T(0);
        }
        mul<G>(g, Tk, Lx, Dn);
        mul<G>(g, Dk, Eb, Tn);
        MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j)
            Lx[w][j] = t_fma<T>(T(2), Dk[w][j], Dn[w][j] + Tn[w][j]) + (on ? T(0) : Lx[w][j]);
        mul<G>(g, Tk, Eb, Tn);
        MF_LEG_UNROLL for (int w = 0; w < G::W; ++w) MF_LEG_UNROLL for (int j = 0; j < G::D; ++j)
            Eb[w][j] = t_fma<T>(T(2), Tk[w][j], Tn[w][j]) + (on ? T(0) : Eb[w][j]);
    }
}

}   // namespace leg
}   // namespace mf
