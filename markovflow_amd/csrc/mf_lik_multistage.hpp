// The multi-stage likelihood's expectation at one point, shared by the translation units that evaluate it: mf_lik.hip (the
// element-wise kernel and the multi-latent SVGP data term on one concatenated chain) and mf_lik_stack.hip (the same data term on
// stacked chains).  Moved here verbatim from mf_lik.hip; the quadrature itself is mf_lik_math.hpp's.
#pragma once

#include "mf_lik_math.hpp"

namespace {

// ---- the multi-stage likelihood (markovflow/likelihoods/mutlistage_likelihood.py): three latents per point, one observation -----
// A decision tree over the latents: y == 0 reads latent 0 (log sigma), y == 1 latents 0 (log(1 - sigma)) and 1 (log sigma), y >= 2
// latents 0 and 1 (log(1 - sigma) each) and 2 (Poisson of y - 2); sigma is the Bernoulli's probit link, jitter included.  Any other
// y - a fraction, a negative number, NaN - reads nothing and contributes exactly 0.  A latent that is not read has derivative 0
// and its variance is not looked at; one that is read outside the domain (s2 <= 0 or NaN) makes the value and its own two
// derivatives NaN.  Only the stages that are read are evaluated: one quadrature for y == 0, two otherwise, plus the closed form
// (bernoulli_stage below; the Poisson stage is expectations<T, 2>).
// The value is summed over the latents in ascending order.
constexpr int MULTI_L = 3;         // latents per point
constexpr int LIK_MULTISTAGE = 4;  // the likelihood id of the multi-latent entry points

__device__ __forceinline__ float m_erfc(float x) { return erfcf(x); }
__device__ __forceinline__ double m_erfc(double x) { return erfc(x); }

// One Bernoulli stage: the nq-point expectation of log sigma(f) (hit) or log(1 - sigma(f)) (miss) with its two derivatives, s2 > 0.
// The formulas are expectations<T, 1>'s with y = 1 or 0; the link is evaluated from its SMALL side, 0.5 erfc(|u|), u = f / sqrt 2:
// sigma = small for u < 0 and 1 - small otherwise, 1 - sigma the other way round.  1 + erf(u) and 1 - sigma cancel in the tails,
// where an erf good to an ulp of 1 leaves the quotient p' / sigma good to 1e-5 only in float32 (sigma is 1e-3 there, the jitter);
// a point of this likelihood reads up to two such stages, and the sums of the float32 kernel then miss what the same formulas give
// with a correctly rounded erf by more than the single-latent kernels do.  erfc keeps the small side to an ulp of ITSELF.
// Used in float32 only.  In float64 the same cancellation costs 1e-13, far below what a model resolves, and the stage is
// expectations<T, 1>: what the Bernoulli kernels, the torch route and the tests' closed forms evaluate, operation for operation.
template <typename T>
__device__ __forceinline__ void bernoulli_stage(const Rule<T>& q, T mu, T s2, bool hit, T& ve, T& gm, T& gv) {
    constexpr T JIT = T(1e-3), INV_SQRT2 = T(0.70710678118654752440084436210485), INV_SQRT_2PI = T(0.3989422804014326779399460599343);
    const T sd = m_sqrt(T(2) * s2);
    T a0 = T(0), a1 = T(0), a2 = T(0);
    for (int i = 0; i < q.nq; ++i) {              // wavefront-uniform: q lives in the kernel arguments
        const T x = q.x[i], w = q.w[i];
        const T f = mu + sd * x, u = f * INV_SQRT2;
        const T small = T(0.5) * m_erfc(u < T(0) ? -u : u) * (T(1) - T(2) * JIT) + JIT;
        const T pr = (u < T(0)) == hit ? small : T(1) - small;      // sigma for a hit, 1 - sigma for a miss
        const T dp = (T(1) - T(2) * JIT) * INV_SQRT_2PI * m_exp(T(-0.5) * f * f);
        const T dl = hit ? dp / pr : -dp / pr;
        a0 += w * m_log(pr);
        a1 += w * dl;
        a2 += w * dl * x;
    }
    ve = a0;
    gm = a1;
    gv = a2 / sd;
}

template <typename T>
__device__ __forceinline__ void multistage_expectations(const Rule<T>& q, T y, const T (&mu)[MULTI_L], const T (&s2)[MULTI_L], T& ve,
                                                        T (&gm)[MULTI_L], T (&gv)[MULTI_L]) {
    const Par<T> none = {T(0), T(0), T(0)};
    const int stage = y == T(0) ? 0 : (y == T(1) ? 1 : (y >= T(2) ? 2 : -1));
    ve = T(0);
#pragma unroll
    for (int l = 0; l < MULTI_L; ++l) gm[l] = gv[l] = T(0);
#pragma unroll
    for (int l = 0; l < 2; ++l) {
        if (l <= stage) {
            if (s2[l] > T(0)) {
                T v;
                if constexpr (std::is_same<T, float>::value) {
                    bernoulli_stage<T>(q, mu[l], s2[l], l == stage, v, gm[l], gv[l]);
                } else {                           // float64: the Bernoulli kernels' own evaluation, the bits of lik 1
                    expectations<T, 1>(q, none, mu[l], s2[l], l == stage ? T(1) : T(0), v, gm[l], gv[l]);
                }
                ve += v;
            } else {
                ve = gm[l] = gv[l] = nan_of<T>();
            }
        }
    }
    if (stage == 2) {
        if (s2[2] > T(0)) {
            T v;
            expectations<T, 2>(q, none, mu[2], s2[2], y - T(2), v, gm[2], gv[2]);
            ve += v;
        } else {
            ve = gm[2] = gv[2] = nan_of<T>();
        }
    }
}

}  // namespace
