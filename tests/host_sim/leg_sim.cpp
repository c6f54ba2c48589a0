// CPU build of the arithmetic of the LatentExponentiallyGenerated transition kernels (markovflow_amd/csrc/mf_leg_math.hpp): the
// host group holds all D rows of a step, a broadcast is an array read, and a step runs through the very functions and the very
// order of calls of leg_transitions_kernel / leg_grad_steps_kernel (mf_leg.hip).  `extra` squaring rounds beyond the step's own
// count stand for a wavefront whose other steps need more: they must not change the result.  Test infrastructure
// (tests/test_leg_host_sim.py compares with tests/helpers/leg_closed_forms.py); plain host compilation, nothing preloaded.
#include "../../markovflow_amd/csrc/mf_leg_math.hpp"

#include <cstdint>

namespace {
using namespace mf;

template <typename T_, int D_> struct HostGroup {
    using T = T_;
    static constexpr int D = D_, W = D_;
    int row(int w) const { return w; }
    template <int K> T bc(const T (&m)[W][D], int j) const { return m[K][j]; }
    T max(const T (&v)[W]) const {
        T a = v[0];
        for (int w = 1; w < W; ++w) a = v[w] > a ? v[w] : a;
        return a;
    }
    bool all(const bool (&v)[W]) const {
        bool a = true;
        for (int w = 0; w < W; ++w) a = a && v[w];
        return a;
    }
    void transpose(const T (&m)[W][D], T (&out)[W][D]) const {
        for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) out[i][j] = m[j][i];
    }
};

template <typename T, int D>
void run(long K, const T* F, const T* dt, T jitter, int extra, T* A, T* Q, T* L, const T* gA, const T* gC, T* terms) {
    using G = HostGroup<T, D>;
    G g;
    T Fr[D][D], Ft[D][D];
    for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) { Fr[i][j] = F[i * D + j]; Ft[i][j] = F[j * D + i]; }
    const T norm1 = leg::norm1_of_transposed<G>(g, Ft);
    const bool lossless = leg::is_skew<G>(g, Fr, Ft);
    for (long k = 0; k < K; ++k) {
        T Y[D][D], E[D][D], Aa[D][D], Qm[D][D], Lr[D][D], Lz[D][D], ga[D][D], gc[D][D], Gs[D][D], Lx[D][D];
        const int s = leg::scaled_argument<G>(Fr, norm1, dt[k], Y);
        const int smax = s + extra;
        leg::expm1_scaled<G>(g, Y, s, smax, E);
        leg::transition_of<G>(g, E, Aa);
        leg::process_covariance<G>(g, E, jitter, lossless, Qm);
        for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) { A[(k * D + i) * D + j] = Aa[i][j]; Q[(k * D + i) * D + j] = Qm[i][j]; }
        bool zero;
        leg::cholesky<G>(g, Qm, Lr, zero);
        leg::copy<G>(Lr, Lz);
        leg::zero_factor<G>(zero, Lz);
        for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) L[(k * D + i) * D + j] = Lz[i][j];
        if (!terms) continue;
        for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) {
            ga[i][j] = gA ? gA[(k * D + i) * D + j] : T(0);
            gc[i][j] = gC ? gC[(k * D + i) * D + j] : T(0);
        }
        leg::adjoint_seed<G>(g, Aa, Lr, zero, ga, gc, Gs);
        for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) Gs[i][j] = leg::t_ldexp<T>(Gs[i][j], -s);
        (void)leg::scaled_argument<G>(Ft, norm1, dt[k], Y);
        leg::frechet_scaled<G>(g, Y, Gs, s, smax, Lx);
        for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) terms[(k * D + i) * D + j] = dt[k] * Lx[i][j];
    }
}

template <typename T>
int dispatch(int d, long K, const T* F, const T* dt, T jitter, int extra, T* A, T* Q, T* L, const T* gA, const T* gC, T* terms) {
    switch (d) {
        case 1: run<T, 1>(K, F, dt, jitter, extra, A, Q, L, gA, gC, terms); return 0;
        case 2: run<T, 2>(K, F, dt, jitter, extra, A, Q, L, gA, gC, terms); return 0;
        case 6: run<T, 6>(K, F, dt, jitter, extra, A, Q, L, gA, gC, terms); return 0;
        case 7: run<T, 7>(K, F, dt, jitter, extra, A, Q, L, gA, gC, terms); return 0;
        case 16: run<T, 16>(K, F, dt, jitter, extra, A, Q, L, gA, gC, terms); return 0;
        default: return -100;
    }
}
}   // namespace

extern "C" {
int mf_leg_host_sim_f64(int d, int64_t K, const double* F, const double* dt, double jitter, int extra, double* A, double* Q, double* L,
                        const double* gA, const double* gC, double* terms) {
    return dispatch<double>(d, (long)K, F, dt, jitter, extra, A, Q, L, gA, gC, terms);
}
int mf_leg_host_sim_f32(int d, int64_t K, const float* F, const float* dt, float jitter, int extra, float* A, float* Q, float* L,
                        const float* gA, const float* gC, float* terms) {
    return dispatch<float>(d, (long)K, F, dt, jitter, extra, A, Q, L, gA, gC, terms);
}
}
