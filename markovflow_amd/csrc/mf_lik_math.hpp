// What the likelihood translation units (mf_lik.hip, mf_st.hip) share: the quadrature rule and the likelihood parameters as they
// travel in the kernel arguments, log p(y | f) with its derivatives, the variational expectation of one point, and the host side's
// argument checks and launch helper.  See mf_lik.hip for the likelihoods themselves.
#pragma once

#include <cmath>
#include <initializer_list>
#include <type_traits>
#include <hip/hip_runtime.h>

namespace {

constexpr int MAXQ = 32;

template <typename T> struct Rule {
    int nq;
    T x[MAXQ];     // nodes
    T w[MAXQ];     // weights / sqrt(pi)  (variational expectations)  or  log(weights / sqrt(pi))  (predictive density)
};
template <typename T> struct Par { T p0, p1, p2; };

__device__ __forceinline__ float m_exp(float x) { return expf(x); }
__device__ __forceinline__ double m_exp(double x) { return exp(x); }
__device__ __forceinline__ float m_log(float x) { return logf(x); }
__device__ __forceinline__ double m_log(double x) { return log(x); }
__device__ __forceinline__ float m_log1p(float x) { return log1pf(x); }
__device__ __forceinline__ double m_log1p(double x) { return log1p(x); }
__device__ __forceinline__ float m_erf(float x) { return erff(x); }
__device__ __forceinline__ double m_erf(double x) { return erf(x); }
__device__ __forceinline__ float m_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double m_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ float m_lgamma(float x) { return lgammaf(x); }
__device__ __forceinline__ double m_lgamma(double x) { return lgamma(x); }

template <typename T> __device__ __forceinline__ T nan_of() { return T(NAN); }

// log p(y | f) and, when asked, its first (DERIV) and second (DERIV2, which implies the first) derivative in f.  Poisson: WITHOUT
// - lgamma(y + 1), which does not depend on f; the caller subtracts it once per point, outside its loop over the nodes.
//   Bernoulli: with p' = (1 - 2e-3) phi(f) and p'' = -f p',  l'' = -f l' - p'^2 (y / p^2 + (1 - y) / (1 - p)^2)
//   Student-t: l'' = -(df + 1) (a - r^2) / (a + r^2)^2,  a = df scale^2,  r = y - f
template <typename T, int LIK, bool DERIV, bool DERIV2 = false>
__device__ __forceinline__ T log_prob(T f, T y, const Par<T>& p, T& dl, T& d2l) {
    constexpr T LOG_2PI = T(1.8378770664093454835606594728112);
    if (LIK == 0) {
        const T r = y - f, iv = T(1) / p.p0;
        if (DERIV || DERIV2) dl = r * iv;
        if (DERIV2) d2l = -iv;
        return T(-0.5) * (LOG_2PI + m_log(p.p0)) - T(0.5) * r * r * iv;
    } else if (LIK == 1) {
        constexpr T JIT = T(1e-3), INV_SQRT2 = T(0.70710678118654752440084436210485), INV_SQRT_2PI = T(0.3989422804014326779399460599343);
        const T pr = T(0.5) * (T(1) + m_erf(f * INV_SQRT2)) * (T(1) - T(2) * JIT) + JIT;
        if (DERIV || DERIV2) {
            const T dp = (T(1) - T(2) * JIT) * INV_SQRT_2PI * m_exp(T(-0.5) * f * f);
            dl = dp * (y / pr - (T(1) - y) / (T(1) - pr));
            if (DERIV2) {
                const T q1 = T(1) - pr;
                d2l = -f * dl - dp * dp * (y / (pr * pr) + (T(1) - y) / (q1 * q1));
            }
        }
        return y * m_log(pr) + (T(1) - y) * m_log1p(-pr);
    } else if (LIK == 2) {
        const T e = m_exp(f);
        if (DERIV || DERIV2) dl = y - e;
        if (DERIV2) d2l = -e;
        return y * f - e;
    } else {
        const T r = y - f, a = p.p1 * p.p0 * p.p0, r2 = r * r;      // a = df scale^2
        if (DERIV || DERIV2) dl = (p.p1 + T(1)) * r / (a + r2);
        if (DERIV2) d2l = -(p.p1 + T(1)) * (a - r2) / ((a + r2) * (a + r2));
        return p.p2 - T(0.5) * (p.p1 + T(1)) * m_log1p(r2 / a);
    }
}
template <typename T, int LIK, bool DERIV>
__device__ __forceinline__ T log_prob(T f, T y, const Par<T>& p, T& dl) {
    T unused;
    return log_prob<T, LIK, DERIV, false>(f, y, p, dl, unused);
}

// the expectation and its two derivatives at one point (fvar > 0)
template <typename T, int LIK>
__device__ __forceinline__ void expectations(const Rule<T>& q, const Par<T>& p, T mu, T s2, T y, T& ve, T& gm, T& gv) {
    if (LIK == 0) {
        constexpr T LOG_2PI = T(1.8378770664093454835606594728112);
        const T r = y - mu, iv = T(1) / p.p0;
        ve = T(-0.5) * (LOG_2PI + m_log(p.p0)) - T(0.5) * (r * r + s2) * iv;
        gm = r * iv;
        gv = T(-0.5) * iv;
    } else if (LIK == 2) {
        const T e = m_exp(mu + T(0.5) * s2);
        ve = y * mu - e - m_lgamma(y + T(1));
        gm = y - e;
        gv = T(-0.5) * e;
    } else {
        const T sd = m_sqrt(T(2) * s2);
        T a0 = T(0), a1 = T(0), a2 = T(0);
        for (int i = 0; i < q.nq; ++i) {          // wavefront-uniform: q lives in the kernel arguments
            const T x = q.x[i], w = q.w[i];
            T dl;
            const T l = log_prob<T, LIK, true>(mu + sd * x, y, p, dl);             // (Poisson never gets here)
            a0 += w * l;
            a1 += w * dl;
            a2 += w * dl * x;
        }
        ve = a0;
        gm = a1;
        gv = a2 / sd;
    }
}

// a range [lo, hi) of offsets that the caller built, clamped into 0 <= lo <= hi <= n and not trusted: a bad one reads nothing, gives
// wrong numbers and no access outside the buffers
__device__ __forceinline__ void clamp_range(long& lo, long& hi, long n) {
    lo = lo < 0 ? 0 : (lo > n ? n : lo);
    hi = hi < lo ? lo : (hi > n ? n : hi);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// argument checks shared by every entry point: 0, or the (negative) position of the offending argument
template <typename T>
int prepare(int64_t N, int lik, const double* params, int nq, const double* nodes, const double* weights, bool log_weights,
            Rule<T>& q, Par<T>& p) {
    if (N < 0 || (N + 255) / 256 > int64_t(0x7fffffff)) return -1;
    if (lik < 0 || lik > 3) return -2;
    p.p0 = p.p1 = p.p2 = T(0);
    if (lik == 0) {
        if (!params || !(params[0] > 0.0)) return -3;
        p.p0 = T(params[0]);
    } else if (lik == 3) {
        if (!params || !(params[0] > 0.0) || !(params[1] > 0.0) || !std::isfinite(params[2])) return -3;
        p.p0 = T(params[0]);
        p.p1 = T(params[1]);
        p.p2 = T(params[2]);
    }
    if (nq < 1 || nq > MAXQ) return -4;
    if (!nodes) return -5;
    if (!weights) return -6;
    const double inv_sqrt_pi = 0.56418958354775628694807945156077;
    q.nq = nq;
    for (int i = 0; i < MAXQ; ++i) {
        const double w = i < nq ? weights[i] * inv_sqrt_pi : 0.0;
        if (i < nq && !(weights[i] > 0.0)) return -6;
        q.x[i] = i < nq ? T(nodes[i]) : T(0);
        q.w[i] = i < nq ? T(log_weights ? std::log(w) : w) : T(0);
    }
    return 0;
}

// null-pointer checks of a run of arguments whose first has position `first`: 0, or the (negative) position of the first null one
inline int first_null(int first, std::initializer_list<const void*> ptrs) {
    for (const void* ptr : ptrs) {
        if (!ptr) return -first;
        ++first;
    }
    return 0;
}

// the runtime likelihood id (0 ... 3: prepare has checked it) as a compile-time constant: f(std::integral_constant<int, LIK>)
template <typename F>
int with_lik(int lik, F&& f) {
    switch (lik) {
        case 0: return f(std::integral_constant<int, 0>{});
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        default: return f(std::integral_constant<int, 3>{});
    }
}

inline const long long* ll(const int64_t* x) { return reinterpret_cast<const long long*>(x); }

}  // namespace
