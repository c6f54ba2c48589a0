// Non-linear SDEs dx = f(x) dt + L dB (markovflow/sde/sde.py, sde_utils.py): Euler-Maruyama simulation, the linearisation along a
// Gaussian path, and the expected squared drift difference (the Girsanov KL term) with its derivatives.  The arithmetic lives in
// mf_nlsde_math.hpp, which tests/host_sim/nlsde_sim.cpp also compiles for the CPU.
//
// Euler-Maruyama: one launch for all T - 1 steps, a lane per path, the state in D <= 4 registers.  With a lane per path the address
// of out[b, k, :] is strided by T D across lanes, so neither stream touches global memory from the recurrence: a block of 64 paths
// walks the time axis in tiles of 256 / (D sizeof(T)) steps, and a tile - 64 rows of at most 256 contiguous bytes - passes through LDS.
//   load   16 lanes per row, a lane per 16-byte chunk, consecutive lanes on consecutive chunks of ONE path; 4 rows per instruction.
//          The chunks are the 16-byte ALIGNED chunks of global memory inside the row (a row starts wherever (b (T - 1) + k0) D
//          falls): each is one 16-byte load.  What a row has in front of its first boundary and behind its last, fewer than 16
//          bytes each, is fetched element by element by the lane that owns the row - a fixed 2 (16 / sizeof(T) - 1) predicated
//          loads per tile, no divergent second walk.  The next tile is fetched into registers before this tile's steps run.
//   steps  lane r walks its row (odd row stride: lanes on distinct banks), reads xi, and writes the new state over it IN PLACE:
//          the noise tile of steps k0 ... k0 + n - 1 becomes the path tile of columns k0 + 1 ... k0 + n.
//   store  the same walk over the rows of `out`.
// dt_k and sqrt(dt_k) of a tile's steps are computed by the first n lanes once and read as LDS broadcasts.  No atomics.
// (B = 65536 paths are 1024 wavefronts, one per SIMD of the device: the prefetch is what hides the load latency, not occupancy.)
//
// The two quadrature kernels follow mf_lik.hip: a lane per point, the rule by value in the kernel arguments, the loop over the
// nodes wavefront-uniform, no [.., nq] temporaries.  The per-series sum of the drift difference is two passes in a fixed order:
// a block of 256 points leaves ONE double partial (a fixed tree in LDS) in a [tile][series] workspace, then a lane per series adds
// its partials in ascending tile order, consecutive lanes reading consecutive doubles - the same bits on every launch, no
// floating-point atomics.
#include "../../include/markovflow_amd.h"

#include <cstdint>
#include <type_traits>
#include <hip/hip_runtime.h>

#include "mf_nlsde_math.hpp"

namespace {
using namespace mf::nlsde;

constexpr int EM_ROW_BYTES = 256;      // a path's row of a tile, at the most: 16 chunks of 16 bytes
constexpr int DD_BLOCK = 256;          // points per partial of the drift difference

template <typename T> struct Vec16;
template <> struct Vec16<double> { typedef double type __attribute__((ext_vector_type(2))); };
template <> struct Vec16<float> { typedef float type __attribute__((ext_vector_type(4))); };

// Where the 16-byte chunks of global memory lie in one row of a tile: the row is the `len` elements from element g0 of an array
// whose first element is `mis` elements past a 16-byte boundary.
template <typename T>
struct Row {
    static constexpr int VEC = 16 / sizeof(T);
    int head;       // elements in front of the first boundary (all of the row if it ends before it)
    int nfull;      // whole chunks behind them; the rest, fewer than VEC elements, is the tail
    __device__ __forceinline__ Row(long g0, int mis, int len) {
        head = (VEC - int((g0 + mis) % VEC)) % VEC;
        head = head < len ? head : len;
        nfull = (len - head) / VEC;
    }
    __device__ __forceinline__ int tail() const { return head + nfull * VEC; }
};

template <typename T, int D, int DRIFT>
__global__ void __launch_bounds__(64) em_kernel(long B, long Tn, Par<T> p, Chol<T> L, int mis_noise, int mis_out,
                                                const T* __restrict__ x0, const T* __restrict__ grid, const T* __restrict__ noise,
                                                T* __restrict__ out) {
    using V = typename Vec16<T>::type;
    constexpr int VEC = Row<T>::VEC, CH = EM_ROW_BYTES / 16;         // whole chunks per row, at the most
    constexpr int TS = CH * VEC / D, RS = (CH * VEC) | 1;            // steps per tile; the odd row stride in LDS
    static_assert(CH == 16, "a quarter of the wavefront walks a row");
    __shared__ T tile[64 * RS];
    __shared__ T ldt[TS], lsq[TS];
    const int lane = threadIdx.x, sub = lane >> 4, c = lane & 15;    // chunk c of rows sub, sub + 4, ...
    const long b0 = (long)blockIdx.x * 64, b = b0 + lane, steps = Tn - 1;
    const int nrows = B - b0 < 64 ? int(B - b0) : 64;
    T x[D];
#pragma unroll
    for (int i = 0; i < D; ++i) x[i] = T(0);
    if (b < B) {
#pragma unroll
        for (int i = 0; i < D; ++i) {
            x[i] = x0[b * D + i];
            out[b * Tn * D + i] = x[i];
        }
    }
    V body[CH];                        // the next tile of noise: this lane's chunk of 16 rows, and the two ends of row `lane`
    T ends[2][VEC - 1];
    auto fetch = [&](long k0, int len) {
        const long row0 = (b0 * steps + k0) * D, stride = steps * D;
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            const int r = 4 * q + sub;
            body[q] = V(T(0));
            if (r >= nrows) continue;
            const long g0 = row0 + r * stride;
            const Row<T> w(g0, mis_noise, len);
            if (c < w.nfull) body[q] = *reinterpret_cast<const V*>(noise + g0 + w.head + c * VEC);
        }
        const long g0 = row0 + lane * stride;
        const Row<T> w(g0, mis_noise, len);
#pragma unroll
        for (int v = 0; v < VEC - 1; ++v) {
            ends[0][v] = lane < nrows && v < w.head ? noise[g0 + v] : T(0);
            ends[1][v] = lane < nrows && w.tail() + v < len ? noise[g0 + w.tail() + v] : T(0);
        }
    };
    if (steps > 0) fetch(0, (steps < TS ? int(steps) : TS) * D);
    for (long k0 = 0; k0 < steps; k0 += TS) {
        const int n = steps - k0 < TS ? int(steps - k0) : TS, len = n * D;
        __syncthreads();               // the previous tile's store has read the rows
        {
            const long row0 = (b0 * steps + k0) * D, stride = steps * D;
#pragma unroll
            for (int q = 0; q < CH; ++q) {
                const int r = 4 * q + sub;
                if (r >= nrows) continue;
                const Row<T> w(row0 + r * stride, mis_noise, len);
                if (c < w.nfull) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) tile[r * RS + w.head + c * VEC + v] = body[q][v];
                }
            }
            if (lane < nrows) {
                const Row<T> w(row0 + lane * stride, mis_noise, len);
#pragma unroll
                for (int v = 0; v < VEC - 1; ++v) {
                    if (v < w.head) tile[lane * RS + v] = ends[0][v];
                    if (w.tail() + v < len) tile[lane * RS + w.tail() + v] = ends[1][v];
                }
            }
        }
        if (lane < n) {
            const T dt = grid[k0 + lane + 1] - grid[k0 + lane];
            ldt[lane] = dt;
            lsq[lane] = t_sqrt(dt);
        }
        __syncthreads();
        if (k0 + TS < steps) fetch(k0 + TS, (steps - k0 - TS < TS ? int(steps - k0 - TS) : TS) * D);
        if (b < B) {
            for (int s = 0; s < n; ++s) {
                T xi[D];
#pragma unroll
                for (int i = 0; i < D; ++i) xi[i] = tile[lane * RS + s * D + i];
                em_step<T, D, DRIFT>(x, xi, ldt[s], lsq[s], L, p);
#pragma unroll
                for (int i = 0; i < D; ++i) tile[lane * RS + s * D + i] = x[i];
            }
        }
        __syncthreads();
        {
            const long row0 = (b0 * Tn + k0 + 1) * D, stride = Tn * D;
#pragma unroll
            for (int q = 0; q < CH; ++q) {
                const int r = 4 * q + sub;
                if (r >= nrows) continue;
                const long g0 = row0 + r * stride;
                const Row<T> w(g0, mis_out, len);
                if (c < w.nfull) {
                    V val;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) val[v] = tile[r * RS + w.head + c * VEC + v];
                    *reinterpret_cast<V*>(out + g0 + w.head + c * VEC) = val;
                }
            }
            if (lane < nrows) {
                const long g0 = row0 + lane * stride;
                const Row<T> w(g0, mis_out, len);
#pragma unroll
                for (int v = 0; v < VEC - 1; ++v) {
                    if (v < w.head) out[g0 + v] = tile[lane * RS + v];
                    if (w.tail() + v < len) out[g0 + w.tail() + v] = tile[lane * RS + w.tail() + v];
                }
            }
        }
    }
}

template <typename T, int DRIFT>
__global__ void __launch_bounds__(256) linearize_kernel(long total, long N, Rule<T> q, Par<T> p, T l, const T* __restrict__ times,
                                                        const T* __restrict__ mean, const T* __restrict__ var, T* __restrict__ A,
                                                        T* __restrict__ bo, T* __restrict__ cq) {
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const long k = id % N;
    T a, b, c;
    linearize_point<T, DRIFT>(q, p, l, mean[id], var[id], times[k + 1] - times[k], a, b, c);
    A[id] = a;
    bo[id] = b;
    cq[id] = c;
}

template <typename T, int DRIFT>
__global__ void __launch_bounds__(DD_BLOCK) drift_difference_kernel(long B, long N, long tiles, Rule<T> q, Par<T> p, T scale,
                                                                    const T* __restrict__ mean, const T* __restrict__ var,
                                                                    const T* __restrict__ A, const T* __restrict__ bi,
                                                                    T* __restrict__ g_m, T* __restrict__ g_S, T* __restrict__ g_A,
                                                                    T* __restrict__ g_b, double* __restrict__ ws) {
    __shared__ double lv[DD_BLOCK];
    const int tid = threadIdx.x;
    const long series = blockIdx.x / tiles, k = (blockIdx.x - series * tiles) * DD_BLOCK + tid;
    double mine = 0.0;
    if (k < N) {
        const long id = series * N + k;
        T val, gm, gS, gA, gb;
        gh_drift_difference<T, DRIFT>(q, p, mean[id], var[id], A[id], bi[id], scale, val, gm, gS, gA, gb);
        if (g_m) g_m[id] = gm;
        if (g_S) g_S[id] = gS;
        if (g_A) g_A[id] = gA;
        if (g_b) g_b[id] = gb;
        mine = double(val);
    }
    lv[tid] = mine;
    __syncthreads();
    for (int s = DD_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) lv[tid] += lv[tid + s];
        __syncthreads();
    }
    if (tid == 0) ws[(blockIdx.x - series * tiles) * B + series] = lv[0];      // [tile][series]: pass 2 reads it coalesced
}

template <typename T>
__global__ void __launch_bounds__(64) drift_difference_sum_kernel(long B, long tiles, const double* __restrict__ ws, T* __restrict__ out) {
    const long series = (long)blockIdx.x * 64 + threadIdx.x;
    if (series >= B) return;
    double acc = 0.0;
    for (long t = 0; t < tiles; ++t) acc += ws[t * B + series];      // consecutive lanes on consecutive doubles
    out[series] = T(acc);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
inline int misalignment(const void* ptr, size_t elem) { return int((reinterpret_cast<uintptr_t>(ptr) % 16) / elem); }

template <typename T, int D>
int launch_em(int drift, long B, long Tn, const Par<T>& p, const Chol<T>& L, const T* x0, const T* grid, const T* noise, T* out,
              hipStream_t st) {
    const dim3 blocks((unsigned)((B + 63) / 64));
    const int mn = misalignment(noise, sizeof(T)), mo = misalignment(out, sizeof(T));
    if (drift == 0)
        hipLaunchKernelGGL((em_kernel<T, D, 0>), blocks, dim3(64), 0, st, B, Tn, p, L, mn, mo, x0, grid, noise, out);
    else
        hipLaunchKernelGGL((em_kernel<T, D, 1>), blocks, dim3(64), 0, st, B, Tn, p, L, mn, mo, x0, grid, noise, out);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

template <typename T>
int run_em(int64_t B, int64_t Tn, int d, int drift, const double* params, const double* chol_l, const T* x0, const T* grid,
           const T* noise, T* out, void* stream) {
    if (B < 0 || (B + 63) / 64 > int64_t(0x7fffffff)) return -1;
    if (Tn < 1) return -2;
    if (d < 1) return -3;
    if (d > MAX_D) return -100;
    Par<T> p;
    const int bad = make_par<T>(drift, params, p);
    if (bad) return -(3 + bad);
    if (!chol_l) return -6;
    Chol<T> L;
    for (int i = 0; i < MAX_D * (MAX_D + 1) / 2; ++i) L.l[i] = i < d * (d + 1) / 2 ? T(chol_l[i]) : T(0);
    if (B == 0) return 0;
    if (!x0) return -7;
    if (Tn > 1 && !grid) return -8;
    if (Tn > 1 && !noise) return -9;
    if (!out) return -10;
    if (reinterpret_cast<uintptr_t>(noise) % sizeof(T) || reinterpret_cast<uintptr_t>(out) % sizeof(T)) return -10;
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (d) {
        case 1: return launch_em<T, 1>(drift, B, Tn, p, L, x0, grid, noise, out, st);
        case 2: return launch_em<T, 2>(drift, B, Tn, p, L, x0, grid, noise, out, st);
        case 3: return launch_em<T, 3>(drift, B, Tn, p, L, x0, grid, noise, out, st);
        default: return launch_em<T, 4>(drift, B, Tn, p, L, x0, grid, noise, out, st);
    }
}

template <typename T>
int run_linearize(int64_t B, int64_t N, int drift, const double* params, T chol_l, int nq, const double* nodes, const double* weights,
                  const T* times, const T* mean, const T* var, T* A, T* b, T* cholQ, void* stream) {
    if (B < 0) return -1;
    if (N < 0 || (B > 0 && N > int64_t(0x7fffffff) * 256 / B)) return -2;
    Par<T> p;
    int bad = make_par<T>(drift, params, p);
    if (bad) return -(2 + bad);
    Rule<T> q;
    bad = make_rule<T>(nq, nodes, weights, q);
    if (bad) return -(5 + bad);
    if (B == 0 || N == 0) return 0;
    const void* ptrs[] = {times, mean, var, A, b, cholQ};
    for (int i = 0; i < 6; ++i)
        if (!ptrs[i]) return -(9 + i);
    const long total = (long)B * N;
    const dim3 blocks((unsigned)((total + 255) / 256));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (drift == 0)
        hipLaunchKernelGGL((linearize_kernel<T, 0>), blocks, dim3(256), 0, st, total, (long)N, q, p, chol_l, times, mean, var, A, b, cholQ);
    else
        hipLaunchKernelGGL((linearize_kernel<T, 1>), blocks, dim3(256), 0, st, total, (long)N, q, p, chol_l, times, mean, var, A, b, cholQ);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

inline long dd_tiles(int64_t N) { return (long)((N + DD_BLOCK - 1) / DD_BLOCK); }

inline size_t dd_workspace(int64_t B, int64_t N) {
    if (B <= 0 || N <= 0) return 0;
    return size_t(B) * size_t(dd_tiles(N)) * sizeof(double);
}

template <typename T>
int run_drift_difference(int64_t B, int64_t N, int drift, const double* params, int nq, const double* nodes, const double* weights,
                         T scale, const T* mean, const T* var, const T* A, const T* b, T* sum, T* g_m, T* g_S, T* g_A, T* g_b,
                         void* ws, size_t ws_bytes, void* stream) {
    if (B < 0 || (B + 63) / 64 > int64_t(0x7fffffff)) return -1;
    if (N < 0 || (B > 0 && dd_tiles(N) > int64_t(0x7fffffff) / B)) return -2;
    Par<T> p;
    int bad = make_par<T>(drift, params, p);
    if (bad) return -(2 + bad);
    Rule<T> q;
    bad = make_rule<T>(nq, nodes, weights, q);
    if (bad) return -(4 + bad);
    if (B == 0) return 0;
    if (!sum) return -13;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long tiles = dd_tiles(N);
    if (N > 0) {
        const void* ptrs[] = {mean, var, A, b};
        for (int i = 0; i < 4; ++i)
            if (!ptrs[i]) return -(9 + i);
        if (!ws) return -18;
        if (ws_bytes < dd_workspace(B, N) || reinterpret_cast<uintptr_t>(ws) % sizeof(double)) return -19;
        const dim3 blocks((unsigned)(B * tiles));
        double* part = static_cast<double*>(ws);
        if (drift == 0)
            hipLaunchKernelGGL((drift_difference_kernel<T, 0>), blocks, dim3(DD_BLOCK), 0, st, (long)B, (long)N, tiles, q, p, scale, mean, var, A,
                               b, g_m, g_S, g_A, g_b, part);
        else
            hipLaunchKernelGGL((drift_difference_kernel<T, 1>), blocks, dim3(DD_BLOCK), 0, st, (long)B, (long)N, tiles, q, p, scale, mean, var, A,
                               b, g_m, g_S, g_A, g_b, part);
        if (hipGetLastError() != hipSuccess) return -1000;
    }
    hipLaunchKernelGGL((drift_difference_sum_kernel<T>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, (long)B, tiles,
                       static_cast<const double*>(ws), sum);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}
}   // namespace

extern "C" {
int mf_nlsde_euler_maruyama_f64(int64_t B, int64_t T, int d, int drift, const double* params, const double* chol_l, const double* x0,
                                const double* time_grid, const double* noise, double* out, void* stream) {
    return run_em<double>(B, T, d, drift, params, chol_l, x0, time_grid, noise, out, stream);
}
int mf_nlsde_euler_maruyama_f32(int64_t B, int64_t T, int d, int drift, const double* params, const double* chol_l, const float* x0,
                                const float* time_grid, const float* noise, float* out, void* stream) {
    return run_em<float>(B, T, d, drift, params, chol_l, x0, time_grid, noise, out, stream);
}
int mf_nlsde_linearize_f64(int64_t B, int64_t N, int drift, const double* params, double chol_l, int nq, const double* nodes,
                           const double* weights, const double* times, const double* mean, const double* var, double* A, double* b,
                           double* cholQ, void* stream) {
    return run_linearize<double>(B, N, drift, params, chol_l, nq, nodes, weights, times, mean, var, A, b, cholQ, stream);
}
int mf_nlsde_linearize_f32(int64_t B, int64_t N, int drift, const double* params, float chol_l, int nq, const double* nodes,
                           const double* weights, const float* times, const float* mean, const float* var, float* A, float* b,
                           float* cholQ, void* stream) {
    return run_linearize<float>(B, N, drift, params, chol_l, nq, nodes, weights, times, mean, var, A, b, cholQ, stream);
}
size_t mf_nlsde_drift_difference_workspace_bytes(int64_t B, int64_t N) { return dd_workspace(B, N); }
int mf_nlsde_drift_difference_f64(int64_t B, int64_t N, int drift, const double* params, int nq, const double* nodes,
                                  const double* weights, double scale, const double* mean, const double* var, const double* A,
                                  const double* b, double* sum, double* g_m, double* g_S, double* g_A, double* g_b, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    return run_drift_difference<double>(B, N, drift, params, nq, nodes, weights, scale, mean, var, A, b, sum, g_m, g_S, g_A, g_b,
                                        workspace, workspace_bytes, stream);
}
int mf_nlsde_drift_difference_f32(int64_t B, int64_t N, int drift, const double* params, int nq, const double* nodes,
                                  const double* weights, float scale, const float* mean, const float* var, const float* A,
                                  const float* b, float* sum, float* g_m, float* g_S, float* g_A, float* g_b, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    return run_drift_difference<float>(B, N, drift, params, nq, nodes, weights, scale, mean, var, A, b, sum, g_m, g_S, g_A, g_b,
                                       workspace, workspace_bytes, stream);
}
}
