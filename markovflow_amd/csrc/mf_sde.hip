// SDE kernel -> state space model on the device: for a concatenation (block-diagonal state) of
// Matern-1/2, 3/2, 5/2 components, the transition matrices A_k = exp(F dt_k) in closed form and the Cholesky factors of
// the process covariances Q_k = Pinf - A_k Pinf A_k^T (+ jitter I), written straight into the [B, T-1, d, d] tensors
// StateSpaceModel takes.  Replaces, for these kernels, the TensorFlow graph of
//   markovflow/kernels/matern.py:66-86 (Matern12), :299-324,:343-356 (Matern32), :434-460,:485-501 (Matern52),
//   markovflow/kernels/sde_kernel.py:421-446 (transition_statistics: Q = Pinf - A Pinf A^T + jitter),
//   markovflow/kernels/sde_kernel.py:592-610,644-658 (ConcatKernel: block-diagonal A and Pinf),
//   markovflow/state_space_model.py:634-656 (cholesky_or_zero: an all-zero covariance passes through as zero).
// One lane per (series, transition); every component is at most 3 x 3, so everything is register resident.
// mf_sde_transitions_* (further down) adds the order-0 component (Constant) and an oscillator factor (HarmonicOscillator,
// Matern * HarmonicOscillator: blocks up to 6 x 6) in a kernel of its own; the Matern entry points are untouched by it.
#include "../../include/markovflow_amd.h"

// No fused-multiply-add contraction in this file: Q = Pinf - A Pinf A^T must come out EXACTLY zero for a zero time gap
// (the all-zero pass-through of cholesky_or_zero), which a contracted `P - fma(...)` breaks by one rounding error.
#pragma STDC FP_CONTRACT OFF

#include <hip/hip_runtime.h>

namespace {

constexpr int MAXC = 16;   // components per kernel
struct Spec {
    int ncomp, d;
    int order[MAXC];       // 1, 3 or 5  (Matern-order/2)
    int off[MAXC];         // first state index of the component
};

template <typename T> __device__ __forceinline__ T t_exp(T x);
template <> __device__ __forceinline__ float t_exp<float>(float x) { return expf(x); }
template <> __device__ __forceinline__ double t_exp<double>(double x) { return exp(x); }
template <typename T> __device__ __forceinline__ T t_sqrt_(T x);
template <> __device__ __forceinline__ float t_sqrt_<float>(float x) { return sqrtf(x); }
template <> __device__ __forceinline__ double t_sqrt_<double>(double x) { return sqrt(x); }

// Forward-mode derivative carrier with two tangents (d/d lam, d/d var): the gradient kernel below instantiates the SAME closed
// forms (Comp::build, comp_chol) with it, so the derivative cannot drift from the value code.
template <typename T> struct Dual2 {
    T v, a, b;
    __device__ __forceinline__ Dual2() {}
    __device__ __forceinline__ Dual2(T x) : v(x), a(T(0)), b(T(0)) {}
    __device__ __forceinline__ Dual2(T x, T da, T db) : v(x), a(da), b(db) {}
};
template <typename T> __device__ __forceinline__ Dual2<T> operator+(Dual2<T> x, Dual2<T> y) { return {x.v + y.v, x.a + y.a, x.b + y.b}; }
template <typename T> __device__ __forceinline__ Dual2<T> operator-(Dual2<T> x, Dual2<T> y) { return {x.v - y.v, x.a - y.a, x.b - y.b}; }
template <typename T> __device__ __forceinline__ Dual2<T> operator-(Dual2<T> x) { return {-x.v, -x.a, -x.b}; }
template <typename T> __device__ __forceinline__ Dual2<T> operator*(Dual2<T> x, Dual2<T> y) {
    return {x.v * y.v, x.a * y.v + x.v * y.a, x.b * y.v + x.v * y.b};
}
template <typename T> __device__ __forceinline__ Dual2<T> operator/(Dual2<T> x, Dual2<T> y) {
    const T r = T(1) / y.v, q = x.v * r;          // ONE division (an fp64 division is a dozen quarter-rate instructions)
    return {q, (x.a - q * y.a) * r, (x.b - q * y.b) * r};
}
template <typename T> __device__ __forceinline__ Dual2<T>& operator+=(Dual2<T>& x, Dual2<T> y) { x = x + y; return x; }
template <typename T> __device__ __forceinline__ Dual2<T>& operator-=(Dual2<T>& x, Dual2<T> y) { x = x - y; return x; }
template <typename T> __device__ __forceinline__ bool operator==(Dual2<T> x, Dual2<T> y) { return x.v == y.v; }
template <> __device__ __forceinline__ Dual2<float> t_exp<Dual2<float>>(Dual2<float> x) { const float e = expf(x.v); return {e, e * x.a, e * x.b}; }
template <> __device__ __forceinline__ Dual2<double> t_exp<Dual2<double>>(Dual2<double> x) { const double e = exp(x.v); return {e, e * x.a, e * x.b}; }
template <> __device__ __forceinline__ Dual2<float> t_sqrt_<Dual2<float>>(Dual2<float> x) {
    const float r = sqrtf(x.v), h = 0.5f / r;
    return {r, h * x.a, h * x.b};
}
template <> __device__ __forceinline__ Dual2<double> t_sqrt_<Dual2<double>>(Dual2<double> x) {
    const double r = sqrt(x.v), h = 0.5 / r;
    return {r, h * x.a, h * x.b};
}

// A (K x K) and Pinf (K x K) of one Matern component; lam = sqrt(order) / lengthscale
template <typename T, int K> struct Comp {
    T A[K][K], P[K][K];
    __device__ __forceinline__ void build(T lam, T var, T dt) {
        const T e = t_exp<T>(-lam * dt);
        for (int i = 0; i < K; ++i) for (int j = 0; j < K; ++j) P[i][j] = T(0);
        if (K == 1) {
            A[0][0] = e;
            P[0][0] = var;
        } else if (K == 2) {
            // F = [[0, 1], [-lam^2, -2 lam]],  A = e^{-lam dt} (I + (F + lam I) dt)        (matern.py:316-320)
            A[0][0] = e * (T(1) + lam * dt);
            A[0][1] = e * dt;
            A[1][0] = -e * lam * lam * dt;
            A[1][1] = e * (T(1) - lam * dt);
            P[0][0] = var;
            P[1][1] = var * lam * lam;
        } else {
            // F = [[0,1,0],[0,0,1],[-lam^3,-3 lam^2,-3 lam]],  N = F + lam I is nilpotent: A = e^{-lam dt}(I + N dt + N^2 dt^2/2)
            const T l2 = lam * lam, l3 = l2 * lam;
            const T N[3][3] = {{lam, T(1), T(0)}, {T(0), lam, T(1)}, {-l3, -T(3) * l2, -T(2) * lam}};
            T N2[3][3];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    T a = T(0);
                    for (int l = 0; l < 3; ++l) a += N[i][l] * N[l][j];
                    N2[i][j] = a;
                }
            const T h = T(0.5) * dt * dt;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) A[i][j] = e * ((i == j ? T(1) : T(0)) + N[i][j] * dt + N2[i][j] * h);
            const T l23 = l2 / T(3);                                                        // matern.py:494-500
            P[0][0] = var;
            P[0][2] = -var * l23;
            P[2][0] = -var * l23;
            P[1][1] = var * l23;
            P[2][2] = var * l2 * l2;
        }
    }
};

// Q = Pinf - A Pinf A^T + jitter (symmetrised) and its lower Cholesky factor L (an exactly zero Q passes through as a zero factor:
// `zero`)
template <typename T, int K>
__device__ __forceinline__ void comp_chol(const Comp<T, K>& c, T jitter, T (&Q)[K][K], T (&L)[K][K], bool& zero, bool want_chol) {
    T AP[K][K];
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) {
            T a = T(0);
            for (int l = 0; l < K; ++l) a += c.A[i][l] * c.P[l][j];
            AP[i][j] = a;
        }
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) {
            T a = T(0);
            for (int l = 0; l < K; ++l) a += AP[i][l] * c.A[j][l];
            Q[i][j] = c.P[i][j] - a + (i == j ? jitter : T(0));
        }
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < i; ++j) { const T m = T(0.5) * (Q[i][j] + Q[j][i]); Q[i][j] = m; Q[j][i] = m; }
    zero = true;
    for (int i = 0; i < K; ++i) for (int j = 0; j < K; ++j) { zero &= (Q[i][j] == T(0)); L[i][j] = T(0); }
    if (!want_chol || zero) return;
    for (int j = 0; j < K; ++j) {
        T s = Q[j][j];
        for (int l = 0; l < j; ++l) s -= L[j][l] * L[j][l];
        const T ljj = t_sqrt_<T>(s);
        L[j][j] = ljj;
        for (int i = j + 1; i < K; ++i) {
            T v = Q[i][j];
            for (int l = 0; l < j; ++l) v -= L[i][l] * L[j][l];
            L[i][j] = v / ljj;
        }
    }
}

// the component's blocks of ONE of A / chol(Q) / Q (which = 0 / 1 / 2) into a d x d image `blk`
template <typename T, int K>
__device__ __forceinline__ void emit(const Comp<T, K>& c, T jitter, int d, int off, int which, T* __restrict__ blk) {
    if (which == 0) {
        for (int i = 0; i < K; ++i) for (int j = 0; j < K; ++j) blk[(off + i) * d + off + j] = c.A[i][j];
        return;
    }
    T Q[K][K], L[K][K];
    bool zero;
    comp_chol<T, K>(c, jitter, Q, L, zero, which == 1);
    for (int i = 0; i < K; ++i) for (int j = 0; j < K; ++j) blk[(off + i) * d + off + j] = which == 2 ? Q[i][j] : L[i][j];
}

// One wavefront per 64 consecutive (series, transition) pairs: every lane builds its d x d block in an LDS slice (odd
// stride: conflict-free), then the wave writes the 64 blocks - contiguous in the [B, n, d, d] tensor - with coalesced
// stores.  Per-lane scattered 8-byte stores reached 0.6 TB/s; this form writes at several TB/s.
template <typename T>
__global__ void __launch_bounds__(64) matern_transitions_kernel(long B, long n, Spec sp, const T* __restrict__ lam,
                                                                const T* __restrict__ var, long hstride,
                                                                const T* __restrict__ dt, T jitter, T* __restrict__ A,
                                                                T* __restrict__ cholQ, T* __restrict__ Q) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* buf = reinterpret_cast<T*>(smem_raw);
    const long base = (long)blockIdx.x * 64, total = B * n;
    const long id = base + threadIdx.x;
    const bool valid = id < total;
    const int d = sp.d, dd = d * d, stride = dd | 1;
    const long s = valid ? id / n : 0;
    const T delta = valid ? dt[id] : T(1);
    T* mine = buf + threadIdx.x * stride;
    T* outs[3] = {A, cholQ, Q};
    for (int which = 0; which < 3; ++which) {
        T* dst = outs[which];
        if (!dst) continue;
        for (int e = 0; e < dd; ++e) mine[e] = T(0);
        for (int c = 0; c < sp.ncomp; ++c) {
            const T l = lam[s * hstride + c], v = var[s * hstride + c];
            if (sp.order[c] == 1) { Comp<T, 1> k; k.build(l, v, delta); emit<T, 1>(k, jitter, d, sp.off[c], which, mine); }
            else if (sp.order[c] == 3) { Comp<T, 2> k; k.build(l, v, delta); emit<T, 2>(k, jitter, d, sp.off[c], which, mine); }
            else { Comp<T, 3> k; k.build(l, v, delta); emit<T, 3>(k, jitter, d, sp.off[c], which, mine); }
        }
        __syncthreads();
        long nvalid = total - base;
        if (nvalid > 64) nvalid = 64;
        const long count = nvalid * dd;
        T* gdst = dst + base * dd;
        for (long e = threadIdx.x; e < count; e += 64) gdst[e] = buf[(e / dd) * stride + (e % dd)];
        __syncthreads();
    }
}

template <typename T>
int run(int64_t B, int64_t n, int ncomp, const int* orders, const T* lam, const T* var, int per_series, const T* dt, T jitter,
        T* A, T* cholQ, T* Q, void* stream) {
    if (B < 0) return -1;
    if (n < 0) return -2;
    if (ncomp < 1 || ncomp > MAXC) return -3;
    if (!orders) return -4;
    Spec sp;
    sp.ncomp = ncomp;
    int off = 0;
    for (int c = 0; c < ncomp; ++c) {
        if (orders[c] != 1 && orders[c] != 3 && orders[c] != 5) return -4;
        sp.order[c] = orders[c];
        sp.off[c] = off;
        off += (orders[c] + 1) / 2;
    }
    sp.d = off;
    if (B == 0 || n == 0) return 0;
    if (!lam) return -5;
    if (!var) return -6;
    if (!dt) return -8;
    if (!A) return -10;
    const long total = B * n;
    const size_t lds = size_t(64) * size_t((sp.d * sp.d) | 1) * sizeof(T);
    // one wave's staging image: past the 64 KB a kernel gets by default the limit is raised explicitly (gfx950: 160 KB per
    // workgroup); past that the state dimension is not supported by this kernel
    if (lds > size_t(160) * 1024) return -100;
    if (lds > size_t(64) * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(&matern_transitions_kernel<T>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return -100;
    hipLaunchKernelGGL((matern_transitions_kernel<T>), dim3((unsigned)((total + 63) / 64)), dim3(64), lds,
                       static_cast<hipStream_t>(stream), (long)B, (long)n, sp, lam, var, per_series ? (long)ncomp : 0L, dt,
                       jitter, A, cholQ, Q);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// ---- reverse mode of the generator: d/d(lam, var) of  sum_k <gA_k, A_k> + <gC_k, chol Q_k> ----------------------------------------------
// (the hyper-parameter gradient of GaussianProcessRegression.log_likelihood: the reference differentiates matern.py / sde_kernel.py
// :421-446 and the banded Cholesky through TensorFlow; here gA, gC come from the Fisher-identity backward of the log-likelihood.)
// One lane per (series, transition): the component's closed forms in forward mode (Dual2: tangents d/d lam, d/d var), contracted
// with the incoming gradients' diagonal blocks; out [B, n, ncomp, 2] - summed over the transitions by the caller (deterministic).
// (gA / gC point at the component's own block: dense tensors with row stride ld, or - packed - the K x K block row-major and the
// lower triangle of the factor's block row-major)
template <typename T, int K>
__device__ __forceinline__ void grad_component(T lam, T var, T dt, T jitter, int ld, bool packed, const T* __restrict__ gA,
                                               const T* __restrict__ gC, T& g_lam, T& g_var) {
    using Du = Dual2<T>;
    Comp<Du, K> c;
    c.build(Du(lam, T(1), T(0)), Du(var, T(0), T(1)), Du(dt));
    g_lam = T(0);
    g_var = T(0);
    if (gA) {
        for (int i = 0; i < K; ++i)
            for (int j = 0; j < K; ++j) {
                const T g = gA[i * (packed ? K : ld) + j];
                g_lam += g * c.A[i][j].a;
                g_var += g * c.A[i][j].b;
            }
    }
    if (gC) {
        Du Q[K][K], L[K][K];
        bool zero;
        comp_chol<Du, K>(c, Du(jitter), Q, L, zero, true);
        if (!zero) {
            for (int i = 0; i < K; ++i)
                for (int j = 0; j <= i; ++j) {
                    const T g = packed ? gC[i * (i + 1) / 2 + j] : gC[i * ld + j];
                    g_lam += g * L[i][j].a;
                    g_var += g * L[i][j].b;
                }
        }
    }
}
// packed = 0: gA, gC are the dense [B, n, d, d] tensors.  packed = 1: gA is ONE record per transition of `rec` elements -
// [the K x K block of g_A of every component | the lower triangle of the block of g_cholQ of every component], what
// mf_gpr_matern_loglik_grad writes (csrc/mf_gpr_grad.hpp) - and gC is ignored.
template <typename T>
__global__ void __launch_bounds__(64) matern_transitions_grad_kernel(long B, long n, Spec sp, const T* __restrict__ lam,
                                                                     const T* __restrict__ var, long hstride,
                                                                     const T* __restrict__ dt, T jitter, const T* __restrict__ gA,
                                                                     const T* __restrict__ gC, int packed, int rec,
                                                                     T* __restrict__ out) {
    const long id = (long)blockIdx.x * 64 + threadIdx.x;
    if (id >= B * n) return;
    const long s = id / n;
    const int d = sp.d;
    const T delta = dt[id];
    int na = 0;
    for (int c = 0; c < sp.ncomp; ++c) { const int k = (sp.order[c] + 1) / 2; na += k * k; }
    int pa = 0, pc = (int)(((na * sizeof(T) + 15) / 16) * 16 / sizeof(T));      // the factor's part starts on a 16-byte unit
    for (int c = 0; c < sp.ncomp; ++c) {
        const T l = lam[s * hstride + c], v = var[s * hstride + c];
        const int k = (sp.order[c] + 1) / 2, off = sp.off[c];
        const T* ga = packed ? gA + id * rec + pa : (gA ? gA + id * d * d + off * d + off : nullptr);
        const T* gc = packed ? gA + id * rec + pc : (gC ? gC + id * d * d + off * d + off : nullptr);
        pa += k * k;
        pc += k * (k + 1) / 2;
        T gl, gv;
        if (sp.order[c] == 1) grad_component<T, 1>(l, v, delta, jitter, d, packed != 0, ga, gc, gl, gv);
        else if (sp.order[c] == 3) grad_component<T, 2>(l, v, delta, jitter, d, packed != 0, ga, gc, gl, gv);
        else grad_component<T, 3>(l, v, delta, jitter, d, packed != 0, ga, gc, gl, gv);
        out[(id * sp.ncomp + c) * 2] = gl;
        out[(id * sp.ncomp + c) * 2 + 1] = gv;
    }
}

// The stationary prior's factor chol(Pinf + jitter), block by block: out[s, c, :] = <g_cholP0 block c, d chol / d (lam, var)>.
// (Comp::build with the transition zeroed: Q = Pinf + jitter.)
template <typename T, int K>
__device__ __forceinline__ void prior_component(T lam, T var, T jitter, int ld, const T* __restrict__ gC, T& g_lam, T& g_var) {
    using Du = Dual2<T>;
    Comp<Du, K> c;
    c.build(Du(lam, T(1), T(0)), Du(var, T(0), T(1)), Du(T(1)));
    for (int i = 0; i < K; ++i) for (int j = 0; j < K; ++j) c.A[i][j] = Du(T(0));
    Du Q[K][K], L[K][K];
    bool zero;
    comp_chol<Du, K>(c, Du(jitter), Q, L, zero, true);
    g_lam = T(0);
    g_var = T(0);
    if (zero) return;
    for (int i = 0; i < K; ++i)
        for (int j = 0; j <= i; ++j) {
            const T g = gC[i * ld + j];
            g_lam += g * L[i][j].a;
            g_var += g * L[i][j].b;
        }
}
template <typename T>
__global__ void __launch_bounds__(64) matern_prior_grad_kernel(long B, Spec sp, const T* __restrict__ lam, const T* __restrict__ var,
                                                               long hstride, T jitter, const T* __restrict__ gC0, T* __restrict__ out) {
    const long s = (long)blockIdx.x * 64 + threadIdx.x;
    if (s >= B) return;
    const int d = sp.d;
    for (int c = 0; c < sp.ncomp; ++c) {
        const T l = lam[s * hstride + c], v = var[s * hstride + c];
        const int off = sp.off[c];
        const T* gc = gC0 + s * d * d + off * d + off;
        T gl, gv;
        if (sp.order[c] == 1) prior_component<T, 1>(l, v, jitter, d, gc, gl, gv);
        else if (sp.order[c] == 3) prior_component<T, 2>(l, v, jitter, d, gc, gl, gv);
        else prior_component<T, 3>(l, v, jitter, d, gc, gl, gv);
        out[(s * sp.ncomp + c) * 2] = gl;
        out[(s * sp.ncomp + c) * 2 + 1] = gv;
    }
}
template <typename T>
int run_prior_grad(int64_t B, int ncomp, const int* orders, const T* lam, const T* var, int per_series, T jitter, const T* gC0, T* out,
                   void* stream) {
    if (B < 0) return -1;
    if (ncomp < 1 || ncomp > MAXC) return -2;
    if (!orders) return -3;
    Spec sp;
    sp.ncomp = ncomp;
    int off = 0;
    for (int c = 0; c < ncomp; ++c) {
        if (orders[c] != 1 && orders[c] != 3 && orders[c] != 5) return -3;
        sp.order[c] = orders[c];
        sp.off[c] = off;
        off += (orders[c] + 1) / 2;
    }
    sp.d = off;
    if (B == 0) return 0;
    if (!lam) return -4;
    if (!var) return -5;
    if (!gC0) return -8;
    if (!out) return -9;
    hipLaunchKernelGGL((matern_prior_grad_kernel<T>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream),
                       (long)B, sp, lam, var, per_series ? (long)ncomp : 0L, jitter, gC0, out);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

template <typename T>
int run_grad(int64_t B, int64_t n, int ncomp, const int* orders, const T* lam, const T* var, int per_series, const T* dt, T jitter,
             const T* gA, const T* gC, int packed, T* out, void* stream) {
    if (B < 0) return -1;
    if (n < 0) return -2;
    if (ncomp < 1 || ncomp > MAXC) return -3;
    if (!orders) return -4;
    Spec sp;
    sp.ncomp = ncomp;
    int off = 0;
    for (int c = 0; c < ncomp; ++c) {
        if (orders[c] != 1 && orders[c] != 3 && orders[c] != 5) return -4;
        sp.order[c] = orders[c];
        sp.off[c] = off;
        off += (orders[c] + 1) / 2;
    }
    sp.d = off;
    if (B == 0 || n == 0) return 0;
    if (!lam) return -5;
    if (!var) return -6;
    if (!dt) return -8;
    if (!out) return -12;
    if (packed && !gA) return -10;
    int ra = 0, rc = 0;               // elements of a packed record: blocks of g_A | lower triangles of g_cholQ, each padded to 16 bytes
    for (int c = 0; c < ncomp; ++c) { const int k = (orders[c] + 1) / 2; ra += k * k; rc += k * (k + 1) / 2; }
    const int rec = (int)((((ra * sizeof(T) + 15) / 16) * 16 + ((rc * sizeof(T) + 15) / 16) * 16) / sizeof(T));
    const long total = B * n;
    hipLaunchKernelGGL((matern_transitions_grad_kernel<T>), dim3((unsigned)((total + 63) / 64)), dim3(64), 0,
                       static_cast<hipStream_t>(stream), (long)B, (long)n, sp, lam, var, per_series ? (long)ncomp : 0L, dt, jitter,
                       gA, gC, packed, rec, out);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// ---- generalised components: order 0 (Constant) and an oscillator factor (HarmonicOscillator, Matern * HarmonicOscillator) ----------
// (markovflow/kernels/constant.py, periodic.py, sde_kernel.py:691-822 (Product): A = A^M (x) R(omega dt) or R (x) A^M,
// Pinf = Pinf^M (x) I2 or I2 (x) Pinf^M, with R(th) = [[cos th, -sin th], [sin th, cos th]].)  Order 0 is the Matern-1/2 form at
// lam = 0: A = [1], Pinf = [var]; its Q is jitter I EXACTLY (constant.py:86-102, periodic.py:135-154), not the rounding noise of
// var (I - R R^T).  The Matern factor comes from Comp::build and Q / chol Q from comp_chol, so a component without an oscillator is
// computed by the very instructions of matern_transitions_kernel.
struct GSpec {
    int ncomp, d;
    int order[MAXC];       // 0, 1, 3 or 5
    int osc[MAXC];         // 0 = no oscillator, 1 = Matern (x) R, 2 = R (x) Matern
    int off[MAXC];
};

// accurate sin / cos (not the fast intrinsics): cos 0 = 1 and sin 0 = 0 exactly, which the zero-gap pass-through relies on
template <typename T> __device__ __forceinline__ T t_sin(T x);
template <> __device__ __forceinline__ float t_sin<float>(float x) { return sinf(x); }
template <> __device__ __forceinline__ double t_sin<double>(double x) { return sin(x); }
template <typename T> __device__ __forceinline__ T t_cos(T x);
template <> __device__ __forceinline__ float t_cos<float>(float x) { return cosf(x); }
template <> __device__ __forceinline__ double t_cos<double>(double x) { return cos(x); }

// Dual2 with a third tangent (d/d lam, d/d var, d/d omega): the carrier of the generalised generator's reverse mode
template <typename T> struct Dual3 {
    T v, a, b, c;
    __device__ __forceinline__ Dual3() {}
    __device__ __forceinline__ Dual3(T x) : v(x), a(T(0)), b(T(0)), c(T(0)) {}
    __device__ __forceinline__ Dual3(T x, T da, T db, T dc) : v(x), a(da), b(db), c(dc) {}
};
template <typename T> __device__ __forceinline__ Dual3<T> operator+(Dual3<T> x, Dual3<T> y) { return {x.v + y.v, x.a + y.a, x.b + y.b, x.c + y.c}; }
template <typename T> __device__ __forceinline__ Dual3<T> operator-(Dual3<T> x, Dual3<T> y) { return {x.v - y.v, x.a - y.a, x.b - y.b, x.c - y.c}; }
template <typename T> __device__ __forceinline__ Dual3<T> operator-(Dual3<T> x) { return {-x.v, -x.a, -x.b, -x.c}; }
template <typename T> __device__ __forceinline__ Dual3<T> operator*(Dual3<T> x, Dual3<T> y) {
    return {x.v * y.v, x.a * y.v + x.v * y.a, x.b * y.v + x.v * y.b, x.c * y.v + x.v * y.c};
}
template <typename T> __device__ __forceinline__ Dual3<T> operator/(Dual3<T> x, Dual3<T> y) {
    const T r = T(1) / y.v, q = x.v * r;
    return {q, (x.a - q * y.a) * r, (x.b - q * y.b) * r, (x.c - q * y.c) * r};
}
template <typename T> __device__ __forceinline__ Dual3<T>& operator+=(Dual3<T>& x, Dual3<T> y) { x = x + y; return x; }
template <typename T> __device__ __forceinline__ Dual3<T>& operator-=(Dual3<T>& x, Dual3<T> y) { x = x - y; return x; }
template <typename T> __device__ __forceinline__ bool operator==(Dual3<T> x, Dual3<T> y) { return x.v == y.v; }
template <> __device__ __forceinline__ Dual3<float> t_exp<Dual3<float>>(Dual3<float> x) { const float e = expf(x.v); return {e, e * x.a, e * x.b, e * x.c}; }
template <> __device__ __forceinline__ Dual3<double> t_exp<Dual3<double>>(Dual3<double> x) { const double e = exp(x.v); return {e, e * x.a, e * x.b, e * x.c}; }
template <> __device__ __forceinline__ Dual3<float> t_sqrt_<Dual3<float>>(Dual3<float> x) {
    const float r = sqrtf(x.v), h = 0.5f / r;
    return {r, h * x.a, h * x.b, h * x.c};
}
template <> __device__ __forceinline__ Dual3<double> t_sqrt_<Dual3<double>>(Dual3<double> x) {
    const double r = sqrt(x.v), h = 0.5 / r;
    return {r, h * x.a, h * x.b, h * x.c};
}
template <> __device__ __forceinline__ Dual3<float> t_sin<Dual3<float>>(Dual3<float> x) {
    const float s = sinf(x.v), c = cosf(x.v);
    return {s, c * x.a, c * x.b, c * x.c};
}
template <> __device__ __forceinline__ Dual3<double> t_sin<Dual3<double>>(Dual3<double> x) {
    const double s = sin(x.v), c = cos(x.v);
    return {s, c * x.a, c * x.b, c * x.c};
}
template <> __device__ __forceinline__ Dual3<float> t_cos<Dual3<float>>(Dual3<float> x) {
    const float s = -sinf(x.v), c = cosf(x.v);
    return {c, s * x.a, s * x.b, s * x.c};
}
template <> __device__ __forceinline__ Dual3<double> t_cos<Dual3<double>>(Dual3<double> x) {
    const double s = -sin(x.v), c = cos(x.v);
    return {c, s * x.a, s * x.b, s * x.c};
}

// A and Pinf of (a Matern factor of KM states) x (the oscillator): RF = false: Matern (x) R, true: R (x) Matern
template <typename T, int KM, bool RF>
__device__ __forceinline__ void build_osc(T lam, T var, T omega, T dt, Comp<T, 2 * KM>& out) {
    Comp<T, KM> m;
    m.build(lam, var, dt);
    const T th = omega * dt;
    const T c = t_cos<T>(th), s = t_sin<T>(th);
    const T R[2][2] = {{c, -s}, {s, c}};
    for (int i = 0; i < KM; ++i)
        for (int j = 0; j < KM; ++j)
            for (int p = 0; p < 2; ++p)
                for (int q = 0; q < 2; ++q) {
                    const int row = RF ? p * KM + i : i * 2 + p, col = RF ? q * KM + j : j * 2 + q;
                    out.A[row][col] = m.A[i][j] * R[p][q];
                    out.P[row][col] = p == q ? m.P[i][j] : T(0);
                }
}

// emit() for a component that may be of order 0, whose Q is jitter I exactly
template <typename T, int K>
__device__ __forceinline__ void emit_g(const Comp<T, K>& c, bool order0, T jitter, int d, int off, int which, T* __restrict__ blk) {
    if (which == 0 || !order0) { emit<T, K>(c, jitter, d, off, which, blk); return; }
    const T v = which == 2 ? jitter : t_sqrt_<T>(jitter);
    for (int i = 0; i < K; ++i) for (int j = 0; j < K; ++j) blk[(off + i) * d + off + j] = i == j ? v : T(0);
}

// matern_transitions_kernel for generalised components: the same staging and stores, the component's block up to 6 x 6
template <typename T>
__global__ void __launch_bounds__(64) sde_transitions_kernel(long B, long n, GSpec sp, const T* __restrict__ lam,
                                                             const T* __restrict__ var, const T* __restrict__ omega, long hstride,
                                                             const T* __restrict__ dt, T jitter, T* __restrict__ A,
                                                             T* __restrict__ cholQ, T* __restrict__ Q) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* buf = reinterpret_cast<T*>(smem_raw);
    const long base = (long)blockIdx.x * 64, total = B * n;
    const long id = base + threadIdx.x;
    const bool valid = id < total;
    const int d = sp.d, dd = d * d, stride = dd | 1;
    const long s = valid ? id / n : 0;
    const T delta = valid ? dt[id] : T(1);
    T* mine = buf + threadIdx.x * stride;
    T* outs[3] = {A, cholQ, Q};
    for (int which = 0; which < 3; ++which) {
        T* dst = outs[which];
        if (!dst) continue;
        for (int e = 0; e < dd; ++e) mine[e] = T(0);
        for (int c = 0; c < sp.ncomp; ++c) {
            const int order = sp.order[c], osc = sp.osc[c], off = sp.off[c];
            const T l = order == 0 ? T(0) : lam[s * hstride + c], v = var[s * hstride + c];
            if (osc == 0) {
                if (order <= 1) { Comp<T, 1> k; k.build(l, v, delta); emit_g<T, 1>(k, order == 0, jitter, d, off, which, mine); }
                else if (order == 3) { Comp<T, 2> k; k.build(l, v, delta); emit<T, 2>(k, jitter, d, off, which, mine); }
                else { Comp<T, 3> k; k.build(l, v, delta); emit<T, 3>(k, jitter, d, off, which, mine); }
                continue;
            }
            const T w = omega[s * hstride + c];
            if (order <= 1) {          // (one Matern state: both Kronecker orders coincide)
                Comp<T, 2> k;
                build_osc<T, 1, false>(l, v, w, delta, k);
                emit_g<T, 2>(k, order == 0, jitter, d, off, which, mine);
            } else if (order == 3) {
                Comp<T, 4> k;
                if (osc == 1) build_osc<T, 2, false>(l, v, w, delta, k); else build_osc<T, 2, true>(l, v, w, delta, k);
                emit<T, 4>(k, jitter, d, off, which, mine);
            } else {
                Comp<T, 6> k;
                if (osc == 1) build_osc<T, 3, false>(l, v, w, delta, k); else build_osc<T, 3, true>(l, v, w, delta, k);
                emit<T, 6>(k, jitter, d, off, which, mine);
            }
        }
        __syncthreads();
        long nvalid = total - base;
        if (nvalid > 64) nvalid = 64;
        const long count = nvalid * dd;
        T* gdst = dst + base * dd;
        for (long e = threadIdx.x; e < count; e += 64) gdst[e] = buf[(e / dd) * stride + (e % dd)];
        __syncthreads();
    }
}

// argument checks shared by the two generalised entry points: 0, or the (negative) position of the offending argument
inline int g_spec(int ncomp, const int* orders, const int* osc, GSpec& sp, bool& any_osc) {
    if (ncomp < 1 || ncomp > MAXC) return -3;
    if (!orders) return -4;
    if (!osc) return -5;
    sp.ncomp = ncomp;
    any_osc = false;
    int off = 0;
    for (int c = 0; c < ncomp; ++c) {
        if (orders[c] != 0 && orders[c] != 1 && orders[c] != 3 && orders[c] != 5) return -4;
        if (osc[c] < 0 || osc[c] > 2) return -5;
        sp.order[c] = orders[c];
        sp.osc[c] = osc[c];
        sp.off[c] = off;
        off += (orders[c] == 0 ? 1 : (orders[c] + 1) / 2) * (osc[c] ? 2 : 1);
        any_osc |= osc[c] != 0;
    }
    sp.d = off;
    return 0;
}

template <typename T>
int run_g(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, const T* lam, const T* var, const T* omega,
          int per_series, const T* dt, T jitter, T* A, T* cholQ, T* Q, void* stream) {
    if (B < 0) return -1;
    if (n < 0) return -2;
    GSpec sp;
    bool any_osc;
    const int bad = g_spec(ncomp, orders, osc, sp, any_osc);
    if (bad) return bad;
    if (B == 0 || n == 0) return 0;
    if (!lam) return -6;
    if (!var) return -7;
    if (any_osc && !omega) return -8;
    if (!dt) return -10;
    if (!A) return -12;
    const long total = B * n;
    const size_t lds = size_t(64) * size_t((sp.d * sp.d) | 1) * sizeof(T);
    if (lds > size_t(160) * 1024) return -100;              // (the limit of run(): d <= 17 in fp64)
    if (lds > size_t(64) * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(&sde_transitions_kernel<T>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return -100;
    hipLaunchKernelGGL((sde_transitions_kernel<T>), dim3((unsigned)((total + 63) / 64)), dim3(64), lds,
                       static_cast<hipStream_t>(stream), (long)B, (long)n, sp, lam, var, omega, per_series ? (long)ncomp : 0L, dt,
                       jitter, A, cholQ, Q);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// reverse mode: grad_component with the third tangent.  g[0..2] = d/d (lam, var, omega) of <gA, A> + <gC, chol Q> over the
// component's K x K block of the dense [.., d, d] gradients (row stride ld)
template <typename T, int K>
__device__ void contract3(const Comp<Dual3<T>, K>& c, bool order0, T jitter, int ld, const T* __restrict__ gA,
                          const T* __restrict__ gC, T (&g)[3]) {
    using Du = Dual3<T>;
    g[0] = g[1] = g[2] = T(0);
    if (gA) {
        for (int i = 0; i < K; ++i)
            for (int j = 0; j < K; ++j) {
                const T w = gA[i * ld + j];
                g[0] += w * c.A[i][j].a;
                g[1] += w * c.A[i][j].b;
                g[2] += w * c.A[i][j].c;
            }
    }
    if (gC && !order0) {               // (order 0: chol Q = sqrt(jitter) I does not depend on the hyper-parameters)
        Du Q[K][K], L[K][K];
        bool zero;
        comp_chol<Du, K>(c, Du(jitter), Q, L, zero, true);
        if (!zero) {
            for (int i = 0; i < K; ++i)
                for (int j = 0; j <= i; ++j) {
                    const T w = gC[i * ld + j];
                    g[0] += w * L[i][j].a;
                    g[1] += w * L[i][j].b;
                    g[2] += w * L[i][j].c;
                }
        }
    }
}
template <typename T>
__global__ void __launch_bounds__(64) sde_transitions_grad_kernel(long B, long n, GSpec sp, const T* __restrict__ lam,
                                                                  const T* __restrict__ var, const T* __restrict__ omega, long hstride,
                                                                  const T* __restrict__ dt, T jitter, const T* __restrict__ gA,
                                                                  const T* __restrict__ gC, T* __restrict__ out) {
    using Du = Dual3<T>;
    const long id = (long)blockIdx.x * 64 + threadIdx.x;
    if (id >= B * n) return;
    const long s = id / n;
    const int d = sp.d;
    const Du delta(dt[id]);
    for (int c = 0; c < sp.ncomp; ++c) {
        const int order = sp.order[c], osc = sp.osc[c], off = sp.off[c];
        const Du l(order == 0 ? T(0) : lam[s * hstride + c], T(1), T(0), T(0)), v(var[s * hstride + c], T(0), T(1), T(0));
        const T* ga = gA ? gA + id * d * d + off * d + off : nullptr;
        const T* gc = gC ? gC + id * d * d + off * d + off : nullptr;
        T g[3];
        if (osc == 0) {
            if (order <= 1) { Comp<Du, 1> k; k.build(l, v, delta); contract3<T, 1>(k, order == 0, jitter, d, ga, gc, g); }
            else if (order == 3) { Comp<Du, 2> k; k.build(l, v, delta); contract3<T, 2>(k, false, jitter, d, ga, gc, g); }
            else { Comp<Du, 3> k; k.build(l, v, delta); contract3<T, 3>(k, false, jitter, d, ga, gc, g); }
        } else {
            const Du w(omega[s * hstride + c], T(0), T(0), T(1));
            if (order <= 1) {
                Comp<Du, 2> k;
                build_osc<Du, 1, false>(l, v, w, delta, k);
                contract3<T, 2>(k, order == 0, jitter, d, ga, gc, g);
            } else if (order == 3) {
                Comp<Du, 4> k;
                if (osc == 1) build_osc<Du, 2, false>(l, v, w, delta, k); else build_osc<Du, 2, true>(l, v, w, delta, k);
                contract3<T, 4>(k, false, jitter, d, ga, gc, g);
            } else {
                Comp<Du, 6> k;
                if (osc == 1) build_osc<Du, 3, false>(l, v, w, delta, k); else build_osc<Du, 3, true>(l, v, w, delta, k);
                contract3<T, 6>(k, false, jitter, d, ga, gc, g);
            }
        }
        T* o = out + (id * sp.ncomp + c) * 3;
        o[0] = order == 0 ? T(0) : g[0];      // (order 0 has no lam)
        o[1] = g[1];
        o[2] = osc == 0 ? T(0) : g[2];
    }
}

template <typename T>
int run_g_grad(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, const T* lam, const T* var, const T* omega,
               int per_series, const T* dt, T jitter, const T* gA, const T* gC, T* out, void* stream) {
    if (B < 0) return -1;
    if (n < 0) return -2;
    GSpec sp;
    bool any_osc;
    const int bad = g_spec(ncomp, orders, osc, sp, any_osc);
    if (bad) return bad;
    if (B == 0 || n == 0) return 0;
    if (!lam) return -6;
    if (!var) return -7;
    if (any_osc && !omega) return -8;
    if (!dt) return -10;
    if (!out) return -14;
    const long total = B * n;
    hipLaunchKernelGGL((sde_transitions_grad_kernel<T>), dim3((unsigned)((total + 63) / 64)), dim3(64), 0,
                       static_cast<hipStream_t>(stream), (long)B, (long)n, sp, lam, var, omega, per_series ? (long)ncomp : 0L, dt,
                       jitter, gA, gC, out);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// ---- piecewise-stationary kernels: the hyper-parameters of a step are those of the segment its START TIME lies in -------------------
// (markovflow/kernels/piecewise_stationary.py: searchsorted(change points augmented by -/+ inf, t, "right") - 1, dynamic_partition,
// one generator call per segment, concat.)  Here every lane looks its own segment up - the number of change points <= t_start,
// compared in T - and reads lam / var / omega of that segment ([nseg, ncomp] or [B, nseg, ncomp]); A_k, Pinf and hence Q_k all
// come from that ONE segment, also when t_start + dt lies beyond the next change point (the reference's behaviour).  The block
// arithmetic is the device code above (Comp::build, build_osc, emit, emit_g, comp_chol, contract3); sde_transitions_kernel and its
// reverse mode are left as they are, so the dispatch over (order, osc) is repeated in the two helpers below.

constexpr int PW_LDS_CHANGE_POINTS = 256;   // staged in LDS up to here (2 KB in fp64); not tuned: only K <= 15 has been timed

// number of change points <= t (cp sorted ascending, LDS or global): in [0, ncp] for ANY t, NaN included
template <typename T> __device__ __forceinline__ int segment_of(const T* __restrict__ cp, int ncp, T t) {
    int lo = 0, hi = ncp;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cp[mid] <= t) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the blocks of ONE of A / chol Q / Q of every component into the lane's d x d image; l / v / w: the segment's hyper-parameters
template <typename T>
__device__ __forceinline__ void emit_components(const GSpec& sp, const T* __restrict__ l_, const T* __restrict__ v_,
                                                const T* __restrict__ w_, T delta, T jitter, int which, T* __restrict__ mine) {
    const int d = sp.d;
    for (int c = 0; c < sp.ncomp; ++c) {
        const int order = sp.order[c], osc = sp.osc[c], off = sp.off[c];
        const T l = order == 0 ? T(0) : l_[c], v = v_[c];
        if (osc == 0) {
            if (order <= 1) { Comp<T, 1> k; k.build(l, v, delta); emit_g<T, 1>(k, order == 0, jitter, d, off, which, mine); }
            else if (order == 3) { Comp<T, 2> k; k.build(l, v, delta); emit<T, 2>(k, jitter, d, off, which, mine); }
            else { Comp<T, 3> k; k.build(l, v, delta); emit<T, 3>(k, jitter, d, off, which, mine); }
            continue;
        }
        const T w = w_[c];
        if (order <= 1) {
            Comp<T, 2> k;
            build_osc<T, 1, false>(l, v, w, delta, k);
            emit_g<T, 2>(k, order == 0, jitter, d, off, which, mine);
        } else if (order == 3) {
            Comp<T, 4> k;
            if (osc == 1) build_osc<T, 2, false>(l, v, w, delta, k); else build_osc<T, 2, true>(l, v, w, delta, k);
            emit<T, 4>(k, jitter, d, off, which, mine);
        } else {
            Comp<T, 6> k;
            if (osc == 1) build_osc<T, 3, false>(l, v, w, delta, k); else build_osc<T, 3, true>(l, v, w, delta, k);
            emit<T, 6>(k, jitter, d, off, which, mine);
        }
    }
}

// sde_transitions_kernel with the segment lookup: the same staging and coalesced stores; the change points sit behind the
// staging image in LDS when `cp_lds`, otherwise the binary search reads them from global memory (L2-resident: every lane
// of the grid walks the same few lines)
template <typename T>
__global__ void __launch_bounds__(64) piecewise_transitions_kernel(long B, long n, GSpec sp, int nseg, const T* __restrict__ cp,
                                                                   int cp_lds, const T* __restrict__ lam, const T* __restrict__ var,
                                                                   const T* __restrict__ omega, long hstride,
                                                                   const T* __restrict__ t_start, const T* __restrict__ dt, T jitter,
                                                                   T* __restrict__ A, T* __restrict__ cholQ, T* __restrict__ Q,
                                                                   int* __restrict__ seg_out) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* buf = reinterpret_cast<T*>(smem_raw);
    const long base = (long)blockIdx.x * 64, total = B * n;
    const long id = base + threadIdx.x;
    const bool valid = id < total;
    const int d = sp.d, dd = d * d, stride = dd | 1, ncp = nseg - 1;
    const T* cps = cp;
    if (cp_lds) {
        T* stage = buf + 64 * stride;
        for (int e = threadIdx.x; e < ncp; e += 64) stage[e] = cp[e];
        __syncthreads();
        cps = stage;
    }
    const long s = valid ? id / n : 0;
    const T delta = valid ? dt[id] : T(1);
    const int seg = valid ? segment_of<T>(cps, ncp, t_start[id]) : 0;
    if (valid && seg_out) seg_out[id] = seg;
    const long h = s * hstride + (long)seg * sp.ncomp;
    T* mine = buf + threadIdx.x * stride;
    T* outs[3] = {A, cholQ, Q};
    for (int which = 0; which < 3; ++which) {
        T* dst = outs[which];
        if (!dst) continue;
        for (int e = 0; e < dd; ++e) mine[e] = T(0);
        emit_components<T>(sp, lam + h, var + h, omega ? omega + h : nullptr, delta, jitter, which, mine);
        __syncthreads();
        long nvalid = total - base;
        if (nvalid > 64) nvalid = 64;
        const long count = nvalid * dd;
        T* gdst = dst + base * dd;
        for (long e = threadIdx.x; e < count; e += 64) gdst[e] = buf[(e / dd) * stride + (e % dd)];
        __syncthreads();
    }
}

// argument checks shared by the two piecewise entry points (positions in THEIR signatures)
inline int pw_spec(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, int nseg, const void* cp, const void* lam,
                   const void* var, const void* omega, const void* t_start, const void* dt, GSpec& sp, bool& empty) {
    if (B < 0) return -1;
    if (n < 0) return -2;
    bool any_osc;
    const int bad = g_spec(ncomp, orders, osc, sp, any_osc);
    if (bad) return bad;
    if (nseg < 1) return -6;
    empty = B == 0 || n == 0;
    if (empty) return 0;
    if (nseg > 1 && !cp) return -7;
    if (!lam) return -8;
    if (!var) return -9;
    if (any_osc && !omega) return -10;
    if (!t_start) return -12;
    if (!dt) return -13;
    return 0;
}

template <typename T>
int run_pw(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, int nseg, const T* cp, const T* lam, const T* var,
           const T* omega, int per_series, const T* t_start, const T* dt, T jitter, T* A, T* cholQ, T* Q, int* seg, void* stream) {
    GSpec sp;
    bool empty = false;
    const int bad = pw_spec(B, n, ncomp, orders, osc, nseg, cp, lam, var, omega, t_start, dt, sp, empty);
    if (bad) return bad;
    if (empty) return 0;
    if (!A) return -15;
    const long total = B * n;
    const size_t image = size_t(64) * size_t((sp.d * sp.d) | 1) * sizeof(T);
    if (image > size_t(160) * 1024) return -100;            // (the limit of run_g())
    // up to PW_LDS_CHANGE_POINTS change points ride behind the staging image (every block copies ALL of them, while a lane's search
    // reads about log2(nseg): past a few hundred the copy costs more than it saves, and a large copy takes LDS from the occupancy),
    // as long as the two stay inside what a kernel gets without asking (64 KB), or inside the raised limit once the image alone is
    // past it; beyond that the lookup reads global memory
    const size_t cpb = size_t(nseg - 1) * sizeof(T);
    const size_t room = (image > size_t(64) * 1024 ? size_t(160) : size_t(64)) * 1024;
    const int cp_lds = nseg > 1 && nseg - 1 <= PW_LDS_CHANGE_POINTS && image + cpb <= room;
    const size_t lds = image + (cp_lds ? cpb : 0);
    if (lds > size_t(64) * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(&piecewise_transitions_kernel<T>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return -100;
    hipLaunchKernelGGL((piecewise_transitions_kernel<T>), dim3((unsigned)((total + 63) / 64)), dim3(64), lds,
                       static_cast<hipStream_t>(stream), (long)B, (long)n, sp, nseg, cp, cp_lds, lam, var, omega,
                       per_series ? (long)nseg * ncomp : 0L, t_start, dt, jitter, A, cholQ, Q, seg);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// Reverse mode, launch 1 of 2.  One wavefront per 64 consecutive steps OF ONE SERIES (the grid is B x ceil(n / 64)): a lane forms
// its step's contributions g[c][0..2] exactly as sde_transitions_grad_kernel does (contract3 on the Dual3 closed forms, with the
// hyper-parameters of the step's segment), parks them in LDS, and the wave folds the lanes of equal segment together: the lowest
// lane of every segment present ("slot" r, in order of first appearance) receives the sum over its lanes IN LANE ORDER, component
// value `lane` summed by lane `lane`.  Record r of block (b, k) is (segment, nv = 3 ncomp sums); cnt[b, k] records are written.
// No atomics: a segment appears in at most one record per block, and launch 2 walks the blocks in order.
template <typename T>
__device__ __forceinline__ void grad_components(const GSpec& sp, const T* __restrict__ l_, const T* __restrict__ v_,
                                                const T* __restrict__ w_, T dt, T jitter, const T* __restrict__ gA,
                                                const T* __restrict__ gC, T* __restrict__ o) {
    using Du = Dual3<T>;
    const int d = sp.d;
    const Du delta(dt);
    for (int c = 0; c < sp.ncomp; ++c) {
        const int order = sp.order[c], osc = sp.osc[c], off = sp.off[c];
        const Du l(order == 0 ? T(0) : l_[c], T(1), T(0), T(0)), v(v_[c], T(0), T(1), T(0));
        const T* ga = gA ? gA + off * d + off : nullptr;
        const T* gc = gC ? gC + off * d + off : nullptr;
        T g[3];
        if (osc == 0) {
            if (order <= 1) { Comp<Du, 1> k; k.build(l, v, delta); contract3<T, 1>(k, order == 0, jitter, d, ga, gc, g); }
            else if (order == 3) { Comp<Du, 2> k; k.build(l, v, delta); contract3<T, 2>(k, false, jitter, d, ga, gc, g); }
            else { Comp<Du, 3> k; k.build(l, v, delta); contract3<T, 3>(k, false, jitter, d, ga, gc, g); }
        } else {
            const Du w(w_[c], T(0), T(0), T(1));
            if (order <= 1) {
                Comp<Du, 2> k;
                build_osc<Du, 1, false>(l, v, w, delta, k);
                contract3<T, 2>(k, order == 0, jitter, d, ga, gc, g);
            } else if (order == 3) {
                Comp<Du, 4> k;
                if (osc == 1) build_osc<Du, 2, false>(l, v, w, delta, k); else build_osc<Du, 2, true>(l, v, w, delta, k);
                contract3<T, 4>(k, false, jitter, d, ga, gc, g);
            } else {
                Comp<Du, 6> k;
                if (osc == 1) build_osc<Du, 3, false>(l, v, w, delta, k); else build_osc<Du, 3, true>(l, v, w, delta, k);
                contract3<T, 6>(k, false, jitter, d, ga, gc, g);
            }
        }
        o[c * 3] = order == 0 ? T(0) : g[0];      // (order 0 has no lam)
        o[c * 3 + 1] = g[1];
        o[c * 3 + 2] = osc == 0 ? T(0) : g[2];
    }
}

template <typename T>
__global__ void __launch_bounds__(64) piecewise_grad_steps_kernel(long n, long nblk, GSpec sp, int nseg, const T* __restrict__ cp,
                                                                  const T* __restrict__ lam, const T* __restrict__ var,
                                                                  const T* __restrict__ omega, long hstride,
                                                                  const T* __restrict__ t_start, const T* __restrict__ dt, T jitter,
                                                                  const T* __restrict__ gA, const T* __restrict__ gC,
                                                                  T* __restrict__ rec_val, int* __restrict__ rec_seg,
                                                                  int* __restrict__ rec_cnt) {
    __shared__ T park[64 * (3 * MAXC + 1)];
    const int lane = threadIdx.x, nv = 3 * sp.ncomp, pstride = nv | 1;
    const long blk = blockIdx.x, b = blk / nblk, k = blk % nblk;
    const long step = k * 64 + lane;
    const bool valid = step < n;
    int seg = -1;
    if (valid) {
        const long id = b * n + step;
        const long dd = (long)sp.d * sp.d;
        seg = segment_of<T>(cp, nseg - 1, t_start[id]);
        const long h = b * hstride + (long)seg * sp.ncomp;
        grad_components<T>(sp, lam + h, var + h, omega ? omega + h : nullptr, dt[id], jitter, gA ? gA + id * dd : nullptr,
                           gC ? gC + id * dd : nullptr, park + lane * pstride);
    }
    __syncthreads();
    unsigned long long remaining = __ballot(valid);
    int slot = 0;
    while (remaining) {                                   // (wave-uniform: one round per segment present in this block)
        const int leader = __ffsll(remaining) - 1;
        const int sl = __shfl(seg, leader);
        const unsigned long long members = __ballot(valid && seg == sl);
        if (lane < nv) {
            T acc = T(0);
            for (unsigned long long m = members; m; m &= m - 1) acc += park[(__ffsll(m) - 1) * pstride + lane];
            rec_val[(blk * 64 + slot) * nv + lane] = acc;
        }
        if (lane == 0) rec_seg[blk * 64 + slot] = sl;
        remaining &= ~members;
        ++slot;
    }
    if (lane == 0) rec_cnt[blk] = slot;
}

// Launch 2 of 2: one thread per (series, segment, value) adds the records of its segment over the series' blocks in block order -
// a fixed order, so two runs agree bit for bit; a segment without a step keeps the exact zero it starts from.
template <typename T>
__global__ void __launch_bounds__(64) piecewise_grad_reduce_kernel(long B, long nblk, int nseg, int nv, const T* __restrict__ rec_val,
                                                                   const int* __restrict__ rec_seg, const int* __restrict__ rec_cnt,
                                                                   T* __restrict__ out) {
    const long id = (long)blockIdx.x * 64 + threadIdx.x;
    if (id >= B * nseg * nv) return;
    const int v = (int)(id % nv), sg = (int)((id / nv) % nseg);
    const long b = id / ((long)nv * nseg);
    T acc = T(0);
    for (long k = 0; k < nblk; ++k) {
        const long blk = b * nblk + k;
        const int cnt = rec_cnt[blk];
        for (int r = 0; r < cnt; ++r)
            if (rec_seg[blk * 64 + r] == sg) { acc += rec_val[(blk * 64 + r) * nv + v]; break; }
    }
    out[id] = acc;
}

// workspace of the reverse mode: per block of 64 steps up to 64 records of nv values | their segments | the record count
inline size_t pw_grad_workspace(int64_t B, int64_t n, int ncomp, size_t elem) {
    if (B <= 0 || n <= 0 || ncomp < 1 || ncomp > MAXC) return 0;
    const size_t blocks = size_t(B) * size_t((n + 63) / 64);
    return blocks * (size_t(64) * 3 * ncomp * elem + 64 * sizeof(int) + sizeof(int));
}

template <typename T>
int run_pw_grad(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, int nseg, const T* cp, const T* lam,
                const T* var, const T* omega, int per_series, const T* t_start, const T* dt, T jitter, const T* gA, const T* gC,
                T* out, void* ws, size_t ws_bytes, void* stream) {
    GSpec sp;
    bool empty = false;
    const int bad = pw_spec(B, n, ncomp, orders, osc, nseg, cp, lam, var, omega, t_start, dt, sp, empty);
    if (bad) return bad;
    if (empty) return 0;
    if (!out) return -17;
    if (!ws) return -18;
    if (ws_bytes < pw_grad_workspace(B, n, ncomp, sizeof(T))) return -19;
    const long nblk = (long)((n + 63) / 64), blocks = (long)B * nblk;
    const int nv = 3 * ncomp;
    T* rec_val = static_cast<T*>(ws);
    int* rec_seg = reinterpret_cast<int*>(rec_val + (size_t)blocks * 64 * nv);
    int* rec_cnt = rec_seg + (size_t)blocks * 64;
    hipLaunchKernelGGL((piecewise_grad_steps_kernel<T>), dim3((unsigned)blocks), dim3(64), 0, static_cast<hipStream_t>(stream),
                       (long)n, nblk, sp, nseg, cp, lam, var, omega, per_series ? (long)nseg * ncomp : 0L, t_start, dt, jitter, gA, gC,
                       rec_val, rec_seg, rec_cnt);
    if (hipGetLastError() != hipSuccess) return -1000;
    const long threads = (long)B * nseg * nv;
    hipLaunchKernelGGL((piecewise_grad_reduce_kernel<T>), dim3((unsigned)((threads + 63) / 64)), dim3(64), 0,
                       static_cast<hipStream_t>(stream), (long)B, nblk, nseg, nv, rec_val, rec_seg, rec_cnt, out);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// ---- mean functions: the response of the kernel's own SDE to impulses / steps at given action times -----------------------------------
// (markovflow/mean_function.py:117-413.)  For one series with actions at tau_0 <= ... <= tau_{K-1}: j(t) = #{k : tau_k < t}, the state
// mean is EXACTLY zero for j = 0 and  s(t) = a_k + exp(F (t - tau_k)) c_k  with k = j - 1 otherwise, the coefficients following the
// affine recurrence  c_0 = r_0,  c_k = exp(F (tau_k - tau_{k-1})) c_{k-1} + r_k  (impulse: r = u, a = 0; step: a = -F^-1 u,
// r_k = a_{k-1} - a_k).  f(t) = H s(t), H selecting the first state of every component into the component's output.  The reference
// materialises [.., K, d, d] and [.., N, d, d] transition tensors for this; here every exp(F dt) block lives in the registers of the
// lane that multiplies with it, built by Comp::build / build_osc above.

// fn(the component's transition block at gap `delta`): THE dispatch over (order, osc) of the kernels below.  Pinf is not used (the
// compiler drops it)
template <typename T, typename Fn>
__device__ __forceinline__ void with_transition(int order, int osc, T l, T w, T delta, Fn&& fn) {
    const T v = T(1);
    if (osc == 0) {
        if (order <= 1) { Comp<T, 1> k; k.build(l, v, delta); fn(k); }
        else if (order == 3) { Comp<T, 2> k; k.build(l, v, delta); fn(k); }
        else { Comp<T, 3> k; k.build(l, v, delta); fn(k); }
    } else if (order <= 1) {
        Comp<T, 2> k;
        build_osc<T, 1, false>(l, v, w, delta, k);
        fn(k);
    } else if (order == 3) {
        Comp<T, 4> k;
        if (osc == 1) build_osc<T, 2, false>(l, v, w, delta, k); else build_osc<T, 2, true>(l, v, w, delta, k);
        fn(k);
    } else {
        Comp<T, 6> k;
        if (osc == 1) build_osc<T, 3, false>(l, v, w, delta, k); else build_osc<T, 3, true>(l, v, w, delta, k);
        fn(k);
    }
}
#define MF_COMP_DIM(k) int(sizeof((k).A) / sizeof((k).A[0]))

struct MSpec : GSpec {
    int out[MAXC];         // the output that the component's first state is added to (H is a 0/1 selector)
};

__host__ __device__ inline int comp_states(int order, int osc) { return (order == 0 ? 1 : (order + 1) / 2) * (osc ? 2 : 1); }

// number of action times < t (tau sorted ascending): in [0, K] for ANY t.  A NaN time sorts last, as in torch.searchsorted: it
// lands in the last bin, where its gap t - tau is NaN, so that a bad query time comes out as NaN (and poisons the gradients of its
// series) instead of hiding behind the exact zero of the points before the first action
template <typename T> __device__ __forceinline__ int actions_before(const T* __restrict__ tau, int K, T t) {
    if (t != t) return K;
    int lo = 0, hi = K;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tau[mid] < t) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Forward, launch 1 of 2: the coefficient scan.  F is block diagonal, so the recurrence decouples by component: one lane per
// (series, component), sequential in K (the number of interventions - small next to N), at most 6 values in registers.
template <typename T>
__global__ void __launch_bounds__(64) mean_scan_kernel(long B, long K, MSpec sp, const T* __restrict__ lam, const T* __restrict__ omega,
                                                       long hstride, const T* __restrict__ tau, const T* __restrict__ r,
                                                       T* __restrict__ c) {
    const long id = (long)blockIdx.x * 64 + threadIdx.x;
    if (id >= B * sp.ncomp) return;
    const long b = id / sp.ncomp;
    const int cc = (int)(id % sp.ncomp);
    const int order = sp.order[cc], osc = sp.osc[cc], off = sp.off[cc], d = sp.d, kk = comp_states(order, osc);
    const T l = order == 0 ? T(0) : lam[b * hstride + cc], w = osc ? omega[b * hstride + cc] : T(0);
    const T* tb = tau + b * K;
    T cur[6];
    for (int i = 0; i < 6; ++i) cur[i] = i < kk ? r[(b * K) * d + off + i] : T(0);
    for (int i = 0; i < kk; ++i) c[(b * K) * d + off + i] = cur[i];
    for (long k = 1; k < K; ++k) {
        const T* rk = r + (b * K + k) * d + off;
        T* ck = c + (b * K + k) * d + off;
        with_transition<T>(order, osc, l, w, tb[k] - tb[k - 1], [&](const auto& blk) {
            constexpr int KK = MF_COMP_DIM(blk);
            T nxt[KK];
            for (int i = 0; i < KK; ++i) {
                T acc = T(0);
                for (int j = 0; j < KK; ++j) acc += blk.A[i][j] * cur[j];
                nxt[i] = acc + rk[i];
            }
            for (int i = 0; i < KK; ++i) { cur[i] = nxt[i]; ck[i] = nxt[i]; }
        });
    }
}

// Forward, launch 2 of 2: one lane per (series, time point).  The lane finds its bin by a binary search of the series' action times
// (global memory, L2-resident: the lanes of a block walk the same few lines), builds every component's block of exp(F (t - tau_k)) in
// registers, multiplies with the slice of c_k, adds a_k and accumulates the first state into the component's output.  State and f
// go through an LDS image (odd stride per lane: conflict-free) and leave with coalesced stores, as in sde_transitions_kernel.
template <typename T>
__global__ void __launch_bounds__(64) mean_eval_kernel(long B, long K, long N, MSpec sp, int m, const T* __restrict__ lam,
                                                       const T* __restrict__ omega, long hstride, const T* __restrict__ tau,
                                                       const T* __restrict__ c, const T* __restrict__ a, const T* __restrict__ tp,
                                                       T* __restrict__ f, T* __restrict__ state) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* buf = reinterpret_cast<T*>(smem_raw);
    const long base = (long)blockIdx.x * 64, total = B * N;
    const long id = base + threadIdx.x;
    const bool valid = id < total;
    const int d = sp.d, stride = (d + m) | 1;
    T* mine = buf + threadIdx.x * stride;       // [state d | f m]
    for (int e = 0; e < d + m; ++e) mine[e] = T(0);
    if (valid) {
        const long b = id / N;
        const T t = tp[id];
        const int j = actions_before<T>(tau + b * K, (int)K, t);
        if (j > 0) {
            const long row = (b * K + (j - 1)) * d;
            const T delta = t - tau[b * K + (j - 1)];
            for (int cc = 0; cc < sp.ncomp; ++cc) {
                const int order = sp.order[cc], osc = sp.osc[cc], off = sp.off[cc];
                const T l = order == 0 ? T(0) : lam[b * hstride + cc], w = osc ? omega[b * hstride + cc] : T(0);
                const T* ck = c + row + off;
                const T* ak = a ? a + row + off : nullptr;
                T* fo = mine + d + sp.out[cc];
                with_transition<T>(order, osc, l, w, delta, [&](const auto& blk) {
                    constexpr int KK = MF_COMP_DIM(blk);
                    T cv[KK];
                    for (int i = 0; i < KK; ++i) cv[i] = ck[i];
                    for (int i = 0; i < KK; ++i) {
                        T acc = T(0);
                        for (int jj = 0; jj < KK; ++jj) acc += blk.A[i][jj] * cv[jj];
                        if (ak) acc = ak[i] + acc;
                        mine[off + i] = acc;
                        if (i == 0) *fo += acc;
                    }
                });
            }
        }
    }
    __syncthreads();
    long nvalid = total - base;
    if (nvalid > 64) nvalid = 64;
    if (nvalid < 0) nvalid = 0;
    for (long e = threadIdx.x; e < nvalid * m; e += 64) f[base * m + e] = buf[(e / m) * stride + d + (e % m)];
    if (state)
        for (long e = threadIdx.x; e < nvalid * d; e += 64) state[base * d + e] = buf[(e / d) * stride + (e % d)];
}

// argument checks shared by the two mean-response entry points (positions in THEIR signatures: both start
// B, K, N, ncomp, orders, osc, lam, omega, per_series, action_times)
inline int mean_spec(int64_t B, int64_t K, int64_t N, int ncomp, const int* orders, const int* osc, const void* lam,
                     const void* omega, const void* tau, MSpec& sp) {
    if (B < 0) return -1;
    if (K < 1 || K > (int64_t(1) << 30)) return -2;
    if (N < 0) return -3;
    bool any_osc, any_lam = false;
    const int bad = g_spec(ncomp, orders, osc, sp, any_osc);
    if (bad) return bad - 1;                                 // (g_spec numbers ncomp, orders, osc 3, 4, 5; here they are 4, 5, 6)
    for (int c = 0; c < ncomp; ++c) any_lam |= orders[c] != 0;
    if (B == 0) return 0;
    if (any_lam && !lam) return -7;
    if (any_osc && !omega) return -8;
    if (!tau) return -10;
    return 0;
}
inline int mean_out_map(int ncomp, int m, const int* out_map, int pos_m, MSpec& sp) {
    if (m < 1 || m > ncomp) return -pos_m;
    if (!out_map) return -(pos_m + 1);
    for (int c = 0; c < ncomp; ++c) {
        if (out_map[c] < 0 || out_map[c] >= m) return -(pos_m + 1);
        sp.out[c] = out_map[c];
    }
    return 0;
}

template <typename T>
int run_mean(int64_t B, int64_t K, int64_t N, int ncomp, const int* orders, const int* osc, const T* lam, const T* omega,
             int per_series, const T* tau, const T* r, const T* a, const T* tp, int m, const int* out_map, T* f, T* state, T* c,
             void* stream) {
    MSpec sp;
    int bad = mean_spec(B, K, N, ncomp, orders, osc, lam, omega, tau, sp);
    if (bad) return bad;
    bad = mean_out_map(ncomp, m, out_map, 14, sp);
    if (bad) return bad;
    if (B == 0 || N == 0) return 0;
    if (!r) return -11;
    if (!tp) return -13;
    if (!f) return -16;
    if (!c) return -18;
    const long hstride = per_series ? (long)ncomp : 0L;
    hipLaunchKernelGGL((mean_scan_kernel<T>), dim3((unsigned)((B * ncomp + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream),
                       (long)B, (long)K, sp, lam, omega, hstride, tau, r, c);
    if (hipGetLastError() != hipSuccess) return -1000;
    const size_t lds = size_t(64) * size_t((sp.d + m) | 1) * sizeof(T);      // (at most 64 x 113 x 8 B = 57 KB: inside the default 64 KB)
    hipLaunchKernelGGL((mean_eval_kernel<T>), dim3((unsigned)((B * N + 63) / 64)), dim3(64), lds, static_cast<hipStream_t>(stream),
                       (long)B, (long)K, (long)N, sp, m, lam, omega, hstride, tau, c, a, tp, f, state);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// Reverse mode (the adjoint of the linear map (r, a) -> f), launch 1 of 2.  One wavefront per 64 consecutive points OF ONE SERIES
// (the grid is B x ceil(N / 64)): a lane parks  v = exp(F delta)^T H^T g  (d values: per component g times the first row of its
// block) and the component's g itself (ncomp values: the rows of H^T g that are not zero) in LDS, and the wave folds the lanes of
// equal bin together as piecewise_grad_steps_kernel does: record r of block (b, q) is (bin, nv = d + ncomp sums over its lanes IN
// LANE ORDER); cnt[b, q] records are written.  A point before the first action belongs to no bin.  No atomics.
template <typename T>
__global__ void __launch_bounds__(64) mean_grad_points_kernel(long K, long N, long nblk, MSpec sp, int m, const T* __restrict__ lam,
                                                              const T* __restrict__ omega, long hstride, const T* __restrict__ tau,
                                                              const T* __restrict__ tp, const T* __restrict__ gf,
                                                              T* __restrict__ rec_val, int* __restrict__ rec_bin,
                                                              int* __restrict__ rec_cnt) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* park = reinterpret_cast<T*>(smem_raw);
    const int lane = threadIdx.x, d = sp.d, nv = d + sp.ncomp, pstride = nv | 1;
    const long blk = blockIdx.x, b = blk / nblk, q = blk % nblk;
    const long point = q * 64 + lane;
    int bin = -1;
    if (point < N) {
        const long id = b * N + point;
        const T t = tp[id];
        bin = actions_before<T>(tau + b * K, (int)K, t) - 1;
        if (bin >= 0) {
            const T delta = t - tau[b * K + bin];
            T* mine = park + lane * pstride;
            for (int cc = 0; cc < sp.ncomp; ++cc) {
                const int order = sp.order[cc], osc = sp.osc[cc], off = sp.off[cc];
                const T l = order == 0 ? T(0) : lam[b * hstride + cc], w = osc ? omega[b * hstride + cc] : T(0);
                const T g = gf[id * m + sp.out[cc]];
                mine[d + cc] = g;
                with_transition<T>(order, osc, l, w, delta, [&](const auto& tr) {
                    constexpr int KK = MF_COMP_DIM(tr);
                    for (int i = 0; i < KK; ++i) mine[off + i] = tr.A[0][i] * g;
                });
            }
        }
    }
    __syncthreads();
    const bool binned = bin >= 0;
    unsigned long long remaining = __ballot(binned);
    int slot = 0;
    while (remaining) {                                   // (wave-uniform: one round per bin present in this block)
        const int leader = __ffsll(remaining) - 1;
        const int bl = __shfl(bin, leader);
        const unsigned long long members = __ballot(binned && bin == bl);
        for (int v = lane; v < nv; v += 64) {
            T acc = T(0);
            for (unsigned long long mm = members; mm; mm &= mm - 1) acc += park[(__ffsll(mm) - 1) * pstride + v];
            rec_val[(blk * 64 + slot) * nv + v] = acc;
        }
        if (lane == 0) rec_bin[blk * 64 + slot] = bl;
        remaining &= ~members;
        ++slot;
    }
    if (lane == 0) rec_cnt[blk] = slot;
}

// Launch 2 of 2: one lane per (series, component).  It clears its slice of g_r (and of g_a), walks the series' blocks ONCE and adds
// every record into its bin - O(records), in block and slot order: a fixed order, so two runs agree bit for bit - and then runs the
// reverse recurrence  lambda_{K-1} = g_c_{K-1},  lambda_{k-1} = g_c_{k-1} + A_k^T lambda_k  in place: g_r = lambda.
template <typename T>
__global__ void __launch_bounds__(64) mean_grad_scan_kernel(long B, long K, long nblk, MSpec sp, const T* __restrict__ lam,
                                                            const T* __restrict__ omega, long hstride, const T* __restrict__ tau,
                                                            const T* __restrict__ rec_val, const int* __restrict__ rec_bin,
                                                            const int* __restrict__ rec_cnt, T* g_r, T* g_a) {
    const long id = (long)blockIdx.x * 64 + threadIdx.x;
    if (id >= B * sp.ncomp) return;
    const long b = id / sp.ncomp;
    const int cc = (int)(id % sp.ncomp);
    const int order = sp.order[cc], osc = sp.osc[cc], off = sp.off[cc], d = sp.d, kk = comp_states(order, osc), nv = d + sp.ncomp;
    for (long k = 0; k < K; ++k)
        for (int i = 0; i < kk; ++i) {
            g_r[(b * K + k) * d + off + i] = T(0);
            if (g_a) g_a[(b * K + k) * d + off + i] = T(0);
        }
    for (long q = 0; q < nblk; ++q) {
        const long blk = b * nblk + q;
        const int cnt = rec_cnt[blk];
        for (int s = 0; s < cnt; ++s) {
            const long row = (b * K + rec_bin[blk * 64 + s]) * d + off;
            const T* rv = rec_val + (blk * 64 + s) * nv;
            for (int i = 0; i < kk; ++i) g_r[row + i] += rv[off + i];
            if (g_a) g_a[row] += rv[d + cc];
        }
    }
    const T l = order == 0 ? T(0) : lam[b * hstride + cc], w = osc ? omega[b * hstride + cc] : T(0);
    const T* tb = tau + b * K;
    T cur[6];
    for (int i = 0; i < 6; ++i) cur[i] = i < kk ? g_r[(b * K + K - 1) * d + off + i] : T(0);
    for (long k = K - 1; k >= 1; --k) {
        T* gk = g_r + (b * K + k - 1) * d + off;
        with_transition<T>(order, osc, l, w, tb[k] - tb[k - 1], [&](const auto& tr) {
            constexpr int KK = MF_COMP_DIM(tr);
            T nxt[KK];
            for (int jj = 0; jj < KK; ++jj) {
                T acc = T(0);
                for (int i = 0; i < KK; ++i) acc += tr.A[i][jj] * cur[i];
                nxt[jj] = gk[jj] + acc;
            }
            for (int i = 0; i < KK; ++i) { cur[i] = nxt[i]; gk[i] = nxt[i]; }
        });
    }
}

// workspace of the reverse mode: per block of 64 points up to 64 records of d + ncomp values | their bins | the record count
inline size_t mean_grad_workspace(int64_t B, int64_t N, int ncomp, int d, size_t elem) {
    if (B <= 0 || N <= 0 || ncomp < 1 || ncomp > MAXC || d < ncomp || d > 6 * MAXC) return 0;
    const size_t blocks = size_t(B) * size_t((N + 63) / 64);
    return blocks * (size_t(64) * size_t(d + ncomp) * elem + 64 * sizeof(int) + sizeof(int));
}

template <typename T>
int run_mean_grad(int64_t B, int64_t K, int64_t N, int ncomp, const int* orders, const int* osc, const T* lam, const T* omega,
                  int per_series, const T* tau, const T* tp, int m, const int* out_map, const T* gf, T* g_r, T* g_a, void* ws,
                  size_t ws_bytes, void* stream) {
    MSpec sp;
    int bad = mean_spec(B, K, N, ncomp, orders, osc, lam, omega, tau, sp);
    if (bad) return bad;
    bad = mean_out_map(ncomp, m, out_map, 12, sp);
    if (bad) return bad;
    if (B == 0) return 0;
    if (!g_r) return -15;
    const long hstride = per_series ? (long)ncomp : 0L;
    const long nblk = (long)((N + 63) / 64), blocks = (long)B * nblk;
    T* rec_val = static_cast<T*>(ws);
    int* rec_bin = nullptr;
    int* rec_cnt = nullptr;
    if (N > 0) {
        if (!tp) return -11;
        if (!gf) return -14;
        if (!ws) return -17;
        if (ws_bytes < mean_grad_workspace(B, N, ncomp, sp.d, sizeof(T))) return -18;
        const int nv = sp.d + ncomp;
        rec_bin = reinterpret_cast<int*>(rec_val + (size_t)blocks * 64 * nv);
        rec_cnt = rec_bin + (size_t)blocks * 64;
        const size_t lds = size_t(64) * size_t(nv | 1) * sizeof(T);
        hipLaunchKernelGGL((mean_grad_points_kernel<T>), dim3((unsigned)blocks), dim3(64), lds, static_cast<hipStream_t>(stream),
                           (long)K, (long)N, nblk, sp, m, lam, omega, hstride, tau, tp, gf, rec_val, rec_bin, rec_cnt);
        if (hipGetLastError() != hipSuccess) return -1000;
    }
    hipLaunchKernelGGL((mean_grad_scan_kernel<T>), dim3((unsigned)((B * ncomp + 63) / 64)), dim3(64), 0,
                       static_cast<hipStream_t>(stream), (long)B, (long)K, nblk, sp, lam, omega, hstride, tau, rec_val, rec_bin,
                       rec_cnt, g_r, g_a);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// R^-1 = (L L^T)^-1 from the Cholesky factor of the observation covariance (KalmanFilter._r_inv, kalman_filter.py:341-348: a
// tf.linalg.cholesky_solve against the identity).  m <= 32: one wavefront, thread j solves column j of L^-1 by forward
// substitution, then the threads share the m^2 entries of L^-T L^-1.  ONE launch instead of the eleven small torch / rocBLAS
// kernels of an identity + two triangular solves (4.6 us each: 6 % of an evaluation at BASELINE config 4).
template <typename T>
__global__ void __launch_bounds__(64) obs_precision_kernel(int m, const T* __restrict__ chol, T* __restrict__ out, int* info) {
    __shared__ T L[32 * 33], Li[32 * 33];
    const int t = threadIdx.x;
    for (int e = t; e < m * m; e += 64) L[(e / m) * 33 + (e % m)] = chol[e];
    __syncthreads();
    if (t < m) {
        // column t of L^-1: x_t = 1 / L_tt, x_i = -(sum_{k<i} L_ik x_k) / L_ii for i > t
        for (int i = 0; i < m; ++i) {
            T acc = (i == t) ? T(1) : T(0);
            for (int k = t; k < i; ++k) acc -= L[i * 33 + k] * Li[k * 33 + t];
            Li[i * 33 + t] = i < t ? T(0) : acc / L[i * 33 + i];
        }
        if (!(L[t * 33 + t] != T(0)) && info) __hip_atomic_store(info, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __syncthreads();
    for (int e = t; e < m * m; e += 64) {
        const int i = e / m, j = e % m;
        T acc = T(0);
        for (int k = (i > j ? i : j); k < m; ++k) acc += Li[k * 33 + i] * Li[k * 33 + j];
        out[e] = acc;
    }
}

template <typename T> int obs_precision(int m, const T* chol, T* out, int* info, void* stream) {
    if (m < 1 || m > 32) return -1;
    if (!chol) return -2;
    if (!out) return -3;
    hipLaunchKernelGGL((obs_precision_kernel<T>), dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), m, chol, out, info);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace

extern "C" {

int mf_obs_precision_from_chol_f64(int m, const double* chol, double* out, int* info, void* stream) {
    return obs_precision<double>(m, chol, out, info, stream);
}
int mf_obs_precision_from_chol_f32(int m, const float* chol, float* out, int* info, void* stream) {
    return obs_precision<float>(m, chol, out, info, stream);
}

int mf_sde_matern_transitions_f64(int64_t B, int64_t n, int ncomp, const int* orders, const double* lam, const double* var,
                                  int per_series, const double* dt, double jitter, double* A, double* cholQ, double* Q,
                                  void* stream) {
    return run<double>(B, n, ncomp, orders, lam, var, per_series, dt, jitter, A, cholQ, Q, stream);
}
int mf_sde_matern_transitions_f32(int64_t B, int64_t n, int ncomp, const int* orders, const float* lam, const float* var,
                                  int per_series, const float* dt, float jitter, float* A, float* cholQ, float* Q,
                                  void* stream) {
    return run<float>(B, n, ncomp, orders, lam, var, per_series, dt, jitter, A, cholQ, Q, stream);
}

int mf_sde_transitions_f64(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, const double* lam, const double* var,
                           const double* omega, int per_series, const double* dt, double jitter, double* A, double* cholQ, double* Q,
                           void* stream) {
    return run_g<double>(B, n, ncomp, orders, osc, lam, var, omega, per_series, dt, jitter, A, cholQ, Q, stream);
}
int mf_sde_transitions_f32(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, const float* lam, const float* var,
                           const float* omega, int per_series, const float* dt, float jitter, float* A, float* cholQ, float* Q,
                           void* stream) {
    return run_g<float>(B, n, ncomp, orders, osc, lam, var, omega, per_series, dt, jitter, A, cholQ, Q, stream);
}
int mf_sde_transitions_grad_f64(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, const double* lam,
                                const double* var, const double* omega, int per_series, const double* dt, double jitter,
                                const double* g_A, const double* g_cholQ, double* out, void* stream) {
    return run_g_grad<double>(B, n, ncomp, orders, osc, lam, var, omega, per_series, dt, jitter, g_A, g_cholQ, out, stream);
}
int mf_sde_transitions_grad_f32(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, const float* lam,
                                const float* var, const float* omega, int per_series, const float* dt, float jitter,
                                const float* g_A, const float* g_cholQ, float* out, void* stream) {
    return run_g_grad<float>(B, n, ncomp, orders, osc, lam, var, omega, per_series, dt, jitter, g_A, g_cholQ, out, stream);
}

int mf_sde_piecewise_transitions_f64(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, int nseg,
                                     const double* change_points, const double* lam, const double* var, const double* omega,
                                     int per_series, const double* t_start, const double* dt, double jitter, double* A, double* cholQ,
                                     double* Q, int* seg, void* stream) {
    return run_pw<double>(B, n, ncomp, orders, osc, nseg, change_points, lam, var, omega, per_series, t_start, dt, jitter, A, cholQ, Q,
                          seg, stream);
}
int mf_sde_piecewise_transitions_f32(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, int nseg,
                                     const float* change_points, const float* lam, const float* var, const float* omega,
                                     int per_series, const float* t_start, const float* dt, float jitter, float* A, float* cholQ,
                                     float* Q, int* seg, void* stream) {
    return run_pw<float>(B, n, ncomp, orders, osc, nseg, change_points, lam, var, omega, per_series, t_start, dt, jitter, A, cholQ, Q,
                         seg, stream);
}
size_t mf_sde_piecewise_transitions_grad_workspace_bytes(int64_t B, int64_t n, int ncomp, int elem_size) {
    return (elem_size == 4 || elem_size == 8) ? pw_grad_workspace(B, n, ncomp, (size_t)elem_size) : 0;
}
int mf_sde_piecewise_transitions_grad_f64(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, int nseg,
                                          const double* change_points, const double* lam, const double* var, const double* omega,
                                          int per_series, const double* t_start, const double* dt, double jitter, const double* g_A,
                                          const double* g_cholQ, double* out, void* workspace, size_t workspace_bytes, void* stream) {
    return run_pw_grad<double>(B, n, ncomp, orders, osc, nseg, change_points, lam, var, omega, per_series, t_start, dt, jitter, g_A,
                               g_cholQ, out, workspace, workspace_bytes, stream);
}
int mf_sde_piecewise_transitions_grad_f32(int64_t B, int64_t n, int ncomp, const int* orders, const int* osc, int nseg,
                                          const float* change_points, const float* lam, const float* var, const float* omega,
                                          int per_series, const float* t_start, const float* dt, float jitter, const float* g_A,
                                          const float* g_cholQ, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    return run_pw_grad<float>(B, n, ncomp, orders, osc, nseg, change_points, lam, var, omega, per_series, t_start, dt, jitter, g_A,
                              g_cholQ, out, workspace, workspace_bytes, stream);
}

int mf_mean_response_f64(int64_t B, int64_t K, int64_t N, int ncomp, const int* orders, const int* osc, const double* lam,
                         const double* omega, int per_series, const double* action_times, const double* r, const double* a,
                         const double* time_points, int m, const int* out_map, double* f, double* state, double* c, void* stream) {
    return run_mean<double>(B, K, N, ncomp, orders, osc, lam, omega, per_series, action_times, r, a, time_points, m, out_map, f, state,
                            c, stream);
}
int mf_mean_response_f32(int64_t B, int64_t K, int64_t N, int ncomp, const int* orders, const int* osc, const float* lam,
                         const float* omega, int per_series, const float* action_times, const float* r, const float* a,
                         const float* time_points, int m, const int* out_map, float* f, float* state, float* c, void* stream) {
    return run_mean<float>(B, K, N, ncomp, orders, osc, lam, omega, per_series, action_times, r, a, time_points, m, out_map, f, state,
                           c, stream);
}
size_t mf_mean_response_grad_workspace_bytes(int64_t B, int64_t N, int ncomp, int d, int elem_size) {
    return (elem_size == 4 || elem_size == 8) ? mean_grad_workspace(B, N, ncomp, d, (size_t)elem_size) : 0;
}
int mf_mean_response_grad_f64(int64_t B, int64_t K, int64_t N, int ncomp, const int* orders, const int* osc, const double* lam,
                              const double* omega, int per_series, const double* action_times, const double* time_points, int m,
                              const int* out_map, const double* g_f, double* g_r, double* g_a, void* workspace,
                              size_t workspace_bytes, void* stream) {
    return run_mean_grad<double>(B, K, N, ncomp, orders, osc, lam, omega, per_series, action_times, time_points, m, out_map, g_f, g_r,
                                 g_a, workspace, workspace_bytes, stream);
}
int mf_mean_response_grad_f32(int64_t B, int64_t K, int64_t N, int ncomp, const int* orders, const int* osc, const float* lam,
                              const float* omega, int per_series, const float* action_times, const float* time_points, int m,
                              const int* out_map, const float* g_f, float* g_r, float* g_a, void* workspace, size_t workspace_bytes,
                              void* stream) {
    return run_mean_grad<float>(B, K, N, ncomp, orders, osc, lam, omega, per_series, action_times, time_points, m, out_map, g_f, g_r,
                                g_a, workspace, workspace_bytes, stream);
}

int mf_sde_matern_transitions_grad_f64(int64_t B, int64_t n, int ncomp, const int* orders, const double* lam, const double* var,
                                       int per_series, const double* dt, double jitter, const double* g_A, const double* g_cholQ,
                                       double* out, void* stream) {
    return run_grad<double>(B, n, ncomp, orders, lam, var, per_series, dt, jitter, g_A, g_cholQ, 0, out, stream);
}
int mf_sde_matern_transitions_grad_f32(int64_t B, int64_t n, int ncomp, const int* orders, const float* lam, const float* var,
                                       int per_series, const float* dt, float jitter, const float* g_A, const float* g_cholQ,
                                       float* out, void* stream) {
    return run_grad<float>(B, n, ncomp, orders, lam, var, per_series, dt, jitter, g_A, g_cholQ, 0, out, stream);
}
int mf_sde_matern_transitions_grad_packed_f64(int64_t B, int64_t n, int ncomp, const int* orders, const double* lam,
                                              const double* var, int per_series, const double* dt, double jitter,
                                              const double* g_packed, double* out, void* stream) {
    return run_grad<double>(B, n, ncomp, orders, lam, var, per_series, dt, jitter, g_packed, nullptr, 1, out, stream);
}
int mf_sde_matern_transitions_grad_packed_f32(int64_t B, int64_t n, int ncomp, const int* orders, const float* lam,
                                              const float* var, int per_series, const float* dt, float jitter,
                                              const float* g_packed, float* out, void* stream) {
    return run_grad<float>(B, n, ncomp, orders, lam, var, per_series, dt, jitter, g_packed, nullptr, 1, out, stream);
}
int mf_sde_matern_prior_chol_grad_f64(int64_t B, int ncomp, const int* orders, const double* lam, const double* var, int per_series,
                                      double jitter, const double* g_cholP0, double* out, void* stream) {
    return run_prior_grad<double>(B, ncomp, orders, lam, var, per_series, jitter, g_cholP0, out, stream);
}
int mf_sde_matern_prior_chol_grad_f32(int64_t B, int ncomp, const int* orders, const float* lam, const float* var, int per_series,
                                      float jitter, const float* g_cholP0, float* out, void* stream) {
    return run_prior_grad<float>(B, ncomp, orders, lam, var, per_series, jitter, g_cholP0, out, stream);
}

}  // extern "C"
