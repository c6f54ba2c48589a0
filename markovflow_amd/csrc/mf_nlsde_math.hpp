// Arithmetic of the non-linear SDE kernels (mf_nlsde.hip; markovflow/sde/sde.py, sde_utils.py): the drift and its derivative by
// id, one Euler-Maruyama step, and the Gauss-Hermite sums of the linearisation and of the drift difference.  Plain C++ that also
// compiles for the host without the HIP headers: tests/host_sim/nlsde_sim.cpp runs these very functions on the CPU.
//   drift 0  Ornstein-Uhlenbeck   f(x) = -lambda x            params [lambda]
//   drift 1  double well          f(x) = 4 x (1 - x^2)        no params
// Both act element-wise on the state; the diffusion is a constant lower-triangular L (packed row by row).
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define MF_NLSDE_HD __host__ __device__ __forceinline__
#else
#define MF_NLSDE_HD inline
#endif

namespace mf {
namespace nlsde {

constexpr int MAXQ = 32;       // nodes of a rule (it travels in the kernel arguments)
constexpr int MAX_D = 4;       // state dimension of the Euler-Maruyama kernel
constexpr int NUM_DRIFTS = 2;

template <typename T> struct Rule {
    int nq;
    T x[MAXQ];     // nodes
    T w[MAXQ];     // weights / sqrt(pi)
};
template <typename T> struct Par { T p0; };
template <typename T> struct Chol { T l[MAX_D * (MAX_D + 1) / 2]; };      // lower triangle, row by row

MF_NLSDE_HD float t_sqrt(float x) { return sqrtf(x); }
MF_NLSDE_HD double t_sqrt(double x) { return sqrt(x); }
template <typename T> MF_NLSDE_HD T t_nan() { return T(NAN); }

template <typename T, int DRIFT> MF_NLSDE_HD T drift(T x, const Par<T>& p) {
    if (DRIFT == 0) return -p.p0 * x;
    return T(4) * x * (T(1) - x * x);
}
template <typename T, int DRIFT> MF_NLSDE_HD T drift_prime(T x, const Par<T>& p) {
    if (DRIFT == 0) return -p.p0;
    return T(4) - T(12) * x * x;
}

// x <- x + f(x) dt + sq (L xi), sq = sqrt(dt): every component from the OLD state
template <typename T, int D, int DRIFT>
MF_NLSDE_HD void em_step(T (&x)[D], const T (&xi)[D], T dt, T sq, const Chol<T>& L, const Par<T>& p) {
    T nx[D];
    for (int i = 0; i < D; ++i) {
        T lx = T(0);
        for (int j = 0; j <= i; ++j) lx += L.l[i * (i + 1) / 2 + j] * xi[j];
        nx[i] = x[i] + drift<T, DRIFT>(x[i], p) * dt + sq * lx;
    }
    for (int i = 0; i < D; ++i) x[i] = nx[i];
}

// E f and E f' under N(m, S), S > 0: sum_i w_i f(x_i), x_i = m + sqrt(2 S) node_i, the nodes in ascending index
template <typename T, int DRIFT>
MF_NLSDE_HD void gh_drift_moments(const Rule<T>& q, const Par<T>& p, T m, T S, T& ef, T& efp) {
    const T sd = t_sqrt(T(2) * S);
    T a0 = T(0), a1 = T(0);
    for (int i = 0; i < q.nq; ++i) {
        const T xi = m + sd * q.x[i];
        a0 += q.w[i] * drift<T, DRIFT>(xi, p);
        a1 += q.w[i] * drift_prime<T, DRIFT>(xi, p);
    }
    ef = a0;
    efp = a1;
}

// one step of the linearised chain (sde_utils.py:146-157, drift.py:93-100, state_dim 1); S <= 0 or NaN: A and b are NaN
template <typename T, int DRIFT>
MF_NLSDE_HD void linearize_point(const Rule<T>& q, const Par<T>& p, T l, T m, T S, T dt, T& A, T& b, T& cq) {
    cq = l * t_sqrt(dt);
    if (!(S > T(0))) {
        A = b = t_nan<T>();
        return;
    }
    T ef, efp;
    gh_drift_moments<T, DRIFT>(q, p, m, S, ef, efp);
    A = T(1) + efp * dt;
    b = (ef - efp * m) * dt;
}

// val = scale / 2 sum_i w_i r_i^2,  r_i = A x_i + b - f(x_i),  with the exact derivatives of that sum in m, S, A and b
// (sde_utils.py:161-228 per point; scale = dt / q).  S <= 0 or NaN: all five are NaN.
template <typename T, int DRIFT>
MF_NLSDE_HD void gh_drift_difference(const Rule<T>& q, const Par<T>& p, T m, T S, T A, T b, T scale, T& val, T& gm, T& gS, T& gA,
                                     T& gb) {
    if (!(S > T(0))) {
        val = gm = gS = gA = gb = t_nan<T>();
        return;
    }
    const T sd = t_sqrt(T(2) * S);
    T a0 = T(0), am = T(0), as = T(0), aa = T(0), ab = T(0);
    for (int i = 0; i < q.nq; ++i) {
        const T node = q.x[i], xi = m + sd * node;
        const T r = (A * xi + b) - drift<T, DRIFT>(xi, p);
        const T wr = q.w[i] * r, wrs = wr * (A - drift_prime<T, DRIFT>(xi, p));
        a0 += wr * r;
        ab += wr;
        aa += wr * xi;
        am += wrs;
        as += wrs * node;
    }
    val = T(0.5) * a0 * scale;
    gb = ab * scale;
    gA = aa * scale;
    gm = am * scale;
    gS = as / sd * scale;
}

// the rule as the kernels carry it: 0, or the offset (0, 1, 2) of the offending one of (nq, nodes, weights)
template <typename T>
inline int make_rule(int nq, const double* nodes, const double* weights, Rule<T>& q) {
    if (nq < 1 || nq > MAXQ) return 1;
    if (!nodes) return 2;
    if (!weights) return 3;
    const double inv_sqrt_pi = 0.56418958354775628694807945156077;
    q.nq = nq;
    for (int i = 0; i < MAXQ; ++i) {
        if (i < nq && !(weights[i] > 0.0)) return 3;
        q.x[i] = i < nq ? T(nodes[i]) : T(0);
        q.w[i] = i < nq ? T(weights[i] * inv_sqrt_pi) : T(0);
    }
    return 0;
}

// drift id and parameters: 0, 1 (unknown id) or 2 (missing or non-finite parameter)
template <typename T>
inline int make_par(int drift_id, const double* params, Par<T>& p) {
    if (drift_id < 0 || drift_id >= NUM_DRIFTS) return 1;
    p.p0 = T(0);
    if (drift_id == 0) {
        if (!params || !std::isfinite(params[0])) return 2;
        p.p0 = T(params[0]);
    }
    return 0;
}

}  // namespace nlsde
}  // namespace mf
