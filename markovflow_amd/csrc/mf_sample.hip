// StateSpaceModel.sample (markovflow/state_space_model.py:298-324) in one call on the chain's own leaves:
//   x_0 = mu0 + cholP0 eps_0,   x_k = A_{k-1} x_{k-1} + b_{k-1} + cholQ_{k-1} eps_k,
// the FULL stored d x d blocks of cholP0 / cholQ multiplied, trajectory r = s B + series on the chain of series r % B.
//
// Work split.  A UNIT is (series, chunk of L consecutive steps); a GROUP of G lanes (G = 1, 16 or 64) walks one unit, its lanes are
// G samples of that series; a wavefront holds 64 / G groups on consecutive units.  All lanes of a group are at the same step of the
// same chain, so A_k, b_k, cholQ_k reach them as UNIFORM-ADDRESS loads: one request per group and instruction (G = 64: the address is
// a function of blockIdx alone and the compiler reads the chain through the constant cache), and the chain is read once per
// (series, chunk, block of G samples), not once per sample.  x, the row of eps and - in the summarising pass - one column of the
// chunk's transition product live in registers (at most 3 d + d scalars); no scratch, no atomics.
//
// eps and out.  A lane owns a row of d values per step, strided by T d across the lanes, so neither stream is touched from the
// recurrence: the wavefront walks time in tiles of TS = 240 / (d sizeof(T)) steps, and a tile - 64 rows of at most 240 contiguous
// bytes - passes through LDS (mf_nlsde.hip's scheme).  16 lanes per row, a lane per 16-byte ALIGNED chunk of global memory that
// meets the row (240 bytes from any element boundary meet at most 16 of them), consecutive lanes on consecutive chunks of ONE
// trajectory, 4 rows per instruction.  A chunk that lies inside the row is one 16-byte access; the two chunks that straddle a
// row's ends move element by element under a predicate.  The next tile is fetched into registers before this tile's steps run;
// lane r then walks row r (odd row stride), and in the emitting pass writes x over eps IN PLACE: the tile that came in as noise
// goes out as states by the same walk over `out`.
//
// Two regimes.  One sweep per trajectory (a single launch of the emitting pass, chunks = 1, no workspace) when S B fills the
// machine or the chain is short.  Few long trajectories are partitioned in time:
//   1. summarise   per unit the zero-start end state v of every sample (chunk 0: the true end state) and the chunk's transition
//                  product Phi, column j carried by lane j of the group through the same A_k the lane has loaded for x
//                  (hence G >= 16 > d): reads eps and the chain, writes the workspace only;
//   2. scan        a lane per trajectory, x_in(c + 1) = Phi_c x_in(c) + v_c over the chunk ends, workspace [chunk][entry][index]
//                  so that consecutive lanes read consecutive scalars;
//   3. emit        every chunk restarted from its x_in: reads eps and the chain again, writes `out` once.
// The result depends on `chunks` (another association) and on nothing else: the same bits on every launch.
#include "../../include/markovflow_amd.h"

#include <cstdint>
#include <hip/hip_runtime.h>

namespace {
constexpr int MAX_D = 9;
constexpr int ROW_BYTES = 240;         // a trajectory's row of a tile, at the most: it meets 16 aligned chunks wherever it starts
constexpr long SWEEP_TRAJECTORIES = 65536;   // chunks = 0: from here on one lane per trajectory fills the device (1024 wavefronts)
constexpr long TARGET_WAVES = 2048;          // chunks = 0: wavefronts the partitioned passes aim at (two per SIMD)
constexpr long MIN_CHUNK = 32;               // chunks = 0: steps per chunk, at the least

template <typename T> struct Vec16;
template <> struct Vec16<double> { typedef double type __attribute__((ext_vector_type(2))); };
template <> struct Vec16<float> { typedef float type __attribute__((ext_vector_type(4))); };

template <typename T>
struct Args {
    long B, S, Tn, R;                  // R = S B trajectories
    long L, CU;                        // steps per chunk; chunks per series that this launch walks (the summary skips the last)
    long sblocks;                      // blocks of G samples
    const T *mu0, *cholP0, *A, *b, *cholQ, *eps;
    T* out;
    T *phi, *v, *xin;                  // [chunk - 1][d d][series], [chunk][d][trajectory], [chunk - 1][d][trajectory]
    int mis_eps, mis_out;              // elements between the last 16-byte boundary and eps / out
};

// Offset IN THE ROW of the first element of aligned chunk c: the row starts at element g0 of an array whose first element lies
// `mis` elements past a 16-byte boundary.  Above -VEC; chunk 0 is the one that holds the row's first element.
template <typename T>
__device__ __forceinline__ int chunk_offset(long g0, int mis, int c) {
    constexpr int VEC = 16 / sizeof(T);
    return c * VEC - int((g0 + mis) % VEC);
}

// MODE 0: emit (the sweep when there is one chunk), 1: summarise.
template <typename T, int D, int G, int MODE>
__global__ void __launch_bounds__(64) walk_kernel(Args<T> a) {
    using V = typename Vec16<T>::type;
    constexpr int VEC = 16 / sizeof(T), CH = 16, NG = 64 / G;
    constexpr int TS = ROW_BYTES / int(sizeof(T)) / D, RS = (TS * D) | 1;      // steps per tile; the odd row stride in LDS
    static_assert(MODE == 0 || G > D, "lane j of a group carries column j of the transition product");
    __shared__ T tile[64 * RS];
    __shared__ long rbase[64];         // element of eps / out at which row r starts (both are [S, B, T, d])
    __shared__ int rlen[64];           // steps of row r
    const int lane = threadIdx.x, sub = lane >> 4, c = lane & 15;              // chunk c of rows sub, sub + 4, ...
    const int g = lane / G, j = lane % G;
    const long ublock = blockIdx.x / a.sblocks, sblock = blockIdx.x - ublock * a.sblocks;
    const long u = ublock * NG + g, s = sblock * G + j;
    const bool unit = u < a.B * a.CU, valid = unit && s < a.S;
    const long series = unit ? u / a.CU : 0, chunk = unit ? u - series * a.CU : 0;
    const long traj = s * a.B + series, k0 = chunk * a.L;
    const int len = unit ? int(a.Tn - k0 < a.L ? a.Tn - k0 : a.L) : 0;
    // a lane without a sample still walks the chain where the group needs its column of the product (S < d)
    const int own_len = valid || (MODE == 1 && unit && sblock == 0 && j < D) ? len : 0;
    rbase[lane] = (traj * a.Tn + k0) * D;
    rlen[lane] = valid ? len : 0;

    T x[D], p[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        x[i] = T(0);
        p[i] = i == j ? T(1) : T(0);
    }
    if (MODE == 0 && valid && chunk > 0) {
#pragma unroll
        for (int i = 0; i < D; ++i) x[i] = a.xin[((chunk - 1) * D + i) * a.R + traj];
    }
    __syncthreads();

    auto steps_of = [&](int r, long t0) {
        const long n = rlen[r] - t0;
        return n < 0 ? 0 : n < TS ? int(n) : TS;
    };
    V body[CH];                        // the next tile of eps: this lane's chunk of 16 rows
    auto fetch = [&](long t0) {
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            const int r = 4 * q + sub, n = steps_of(r, t0) * D;
            body[q] = V(T(0));
            const long g0 = rbase[r] + t0 * D;
            const int e0 = chunk_offset<T>(g0, a.mis_eps, c);
            if (e0 >= n) continue;
            if (e0 >= 0 && e0 + VEC <= n) {
                body[q] = *reinterpret_cast<const V*>(a.eps + g0 + e0);
            } else {
#pragma unroll
                for (int w = 0; w < VEC; ++w)
                    if (e0 + w >= 0 && e0 + w < n) body[q][w] = a.eps[g0 + e0 + w];
            }
        }
    };
    fetch(0);
    for (long t0 = 0; t0 < a.L; t0 += TS) {
        __syncthreads();               // the previous tile's store has read the rows
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            const int r = 4 * q + sub, n = steps_of(r, t0) * D;
            const int e0 = chunk_offset<T>(rbase[r] + t0 * D, a.mis_eps, c);
#pragma unroll
            for (int w = 0; w < VEC; ++w)
                if (e0 + w >= 0 && e0 + w < n) tile[r * RS + e0 + w] = body[q][w];
        }
        __syncthreads();
        if (t0 + TS < a.L) fetch(t0 + TS);
        const int n_own = own_len - t0 < 0 ? 0 : own_len - t0 < TS ? int(own_len - t0) : TS;
        for (int st = 0; st < n_own; ++st) {
            const long k = k0 + t0 + st;
            T xi[D], y[D];
#pragma unroll
            for (int i = 0; i < D; ++i) xi[i] = tile[lane * RS + st * D + i];
            if (k > 0) {
                const long ci = series * (a.Tn - 1) + k - 1;
                const T* __restrict__ Ak = a.A + ci * (D * D);
                const T* __restrict__ bk = a.b + ci * D;
                const T* __restrict__ Qk = a.cholQ + ci * (D * D);
                T pn[D];
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    T acc = bk[i], pa = T(0);
#pragma unroll
                    for (int l = 0; l < D; ++l) acc += Qk[i * D + l] * xi[l];
#pragma unroll
                    for (int l = 0; l < D; ++l) {
                        const T ail = Ak[i * D + l];
                        acc += ail * x[l];
                        if (MODE == 1) pa += ail * p[l];
                    }
                    y[i] = acc;
                    pn[i] = pa;
                }
                if (MODE == 1) {
#pragma unroll
                    for (int i = 0; i < D; ++i) p[i] = pn[i];
                }
            } else {                   // the initial state: no transition in front of it
                const T* __restrict__ m0 = a.mu0 + series * D;
                const T* __restrict__ P0 = a.cholP0 + series * (D * D);
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    T acc = m0[i];
#pragma unroll
                    for (int l = 0; l < D; ++l) acc += P0[i * D + l] * xi[l];
                    y[i] = acc;
                }
            }
#pragma unroll
            for (int i = 0; i < D; ++i) {
                x[i] = y[i];
                if (MODE == 0) tile[lane * RS + st * D + i] = y[i];
            }
        }
        if (MODE == 0) {
            __syncthreads();
#pragma unroll
            for (int q = 0; q < CH; ++q) {
                const int r = 4 * q + sub, n = steps_of(r, t0) * D;
                const long g0 = rbase[r] + t0 * D;
                const int e0 = chunk_offset<T>(g0, a.mis_out, c);
                if (e0 >= n) continue;
                if (e0 >= 0 && e0 + VEC <= n) {
                    V val;
#pragma unroll
                    for (int w = 0; w < VEC; ++w) val[w] = tile[r * RS + e0 + w];
                    *reinterpret_cast<V*>(a.out + g0 + e0) = val;
                } else {
#pragma unroll
                    for (int w = 0; w < VEC; ++w)
                        if (e0 + w >= 0 && e0 + w < n) a.out[g0 + e0 + w] = tile[r * RS + e0 + w];
                }
            }
        }
    }
    if (MODE == 1 && valid) {
#pragma unroll
        for (int i = 0; i < D; ++i) a.v[(chunk * D + i) * a.R + traj] = x[i];
    }
    if (MODE == 1 && unit && sblock == 0 && j < D && chunk > 0) {
#pragma unroll
        for (int i = 0; i < D; ++i) a.phi[((chunk - 1) * (D * D) + i * D + j) * a.B + series] = p[i];
    }
}

// x_in(1) = v_0 (chunk 0 starts at the initial state: its summary is its true end), x_in(c + 1) = Phi_c x_in(c) + v_c.
template <typename T, int D>
__global__ void __launch_bounds__(64) scan_kernel(long B, long R, long C, const T* __restrict__ phi, const T* __restrict__ v,
                                                  T* __restrict__ xin) {
    const long r = (long)blockIdx.x * 64 + threadIdx.x;
    if (r >= R) return;
    const long series = r % B;
    T x[D];
#pragma unroll
    for (int i = 0; i < D; ++i) x[i] = v[i * R + r];
#pragma unroll 2
    for (long c = 1; c < C; ++c) {
#pragma unroll
        for (int i = 0; i < D; ++i) xin[((c - 1) * D + i) * R + r] = x[i];
        if (c == C - 1) break;
        T y[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            T acc = v[(c * D + i) * R + r];
#pragma unroll
            for (int l = 0; l < D; ++l) acc += phi[((c - 1) * (D * D) + i * D + l) * B + series] * x[l];
            y[i] = acc;
        }
#pragma unroll
        for (int i = 0; i < D; ++i) x[i] = y[i];
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct Plan {
    long C, L;                         // chunks per series (1: the sweep) and steps per chunk
    int G;                             // lanes of a group
};

inline long ceil_div(long a, long b) { return (a + b - 1) / b; }

inline int group_lanes(long S, bool partitioned) { return S > 16 ? 64 : (S > 1 || partitioned) ? 16 : 1; }

// chunks: 0 automatic, 1 the sweep, >= 2 that many partitions (clamped to T; the chunks are ceil(T / chunks) steps long, and a
// request that this length cannot honour exactly is rounded down to the number of chunks that are not empty).
inline Plan make_plan(long B, long S, long Tn, long chunks) {
    long C = chunks;
    if (chunks == 0) {
        const int G = group_lanes(S, true);
        const long waves = ceil_div(B, 64 / G) * ceil_div(S, G);               // per chunk of the time axis
        C = ceil_div(TARGET_WAVES, waves);
        if (C > Tn / MIN_CHUNK) C = Tn / MIN_CHUNK;
        if (S * B >= SWEEP_TRAJECTORIES || C < 2) C = 1;
    }
    if (C > Tn) C = Tn;
    Plan p;
    p.L = ceil_div(Tn, C);
    p.C = ceil_div(Tn, p.L);
    p.G = group_lanes(S, p.C > 1);
    return p;
}

template <typename T>
inline size_t workspace_elems(long B, long S, int d, const Plan& p) {
    if (p.C < 2) return 0;
    return size_t(p.C - 1) * (size_t(d) * d * B + 2 * size_t(d) * S * B);
}

inline int misalignment(const void* ptr, size_t elem) { return int((reinterpret_cast<uintptr_t>(ptr) % 16) / elem); }

template <typename T, int D, int G, int MODE>
int launch_walk(Args<T> a, long chunks_walked, hipStream_t st) {
    a.CU = chunks_walked;
    a.sblocks = ceil_div(a.S, G);
    const long blocks = ceil_div(a.B * a.CU, 64 / G) * a.sblocks;
    if (blocks > 0x7fffffffL) return -1;
    hipLaunchKernelGGL((walk_kernel<T, D, G, MODE>), dim3((unsigned)blocks), dim3(64), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

template <typename T, int D>
int launch_d(const Args<T>& a, const Plan& p, hipStream_t st) {
    if (p.C < 2) {
        if (p.G == 1) return launch_walk<T, D, 1, 0>(a, 1, st);
        if (p.G == 16) return launch_walk<T, D, 16, 0>(a, 1, st);
        return launch_walk<T, D, 64, 0>(a, 1, st);
    }
    int rc = p.G == 16 ? launch_walk<T, D, 16, 1>(a, p.C - 1, st) : launch_walk<T, D, 64, 1>(a, p.C - 1, st);
    if (rc) return rc;
    hipLaunchKernelGGL((scan_kernel<T, D>), dim3((unsigned)ceil_div(a.R, 64)), dim3(64), 0, st, a.B, a.R, p.C, a.phi, a.v, a.xin);
    if (hipGetLastError() != hipSuccess) return -1000;
    return p.G == 16 ? launch_walk<T, D, 16, 0>(a, p.C, st) : launch_walk<T, D, 64, 0>(a, p.C, st);
}

template <typename T>
int run_sample(int64_t B, int64_t S, int64_t Tn, int d, const T* mu0, const T* cholP0, const T* A, const T* b, const T* cholQ,
               const T* eps, T* out, void* ws, size_t ws_bytes, int64_t chunks, void* stream) {
    if (B < 0) return -1;
    if (S < 0 || (B > 0 && S > int64_t(0x7fffffff) * 64 / B)) return -2;
    if (Tn < 1) return -3;
    if (d < 1) return -4;
    if (chunks < 0) return -14;
    if (d > MAX_D) return -100;
    if (B == 0 || S == 0) return 0;
    if (!mu0) return -5;
    if (!cholP0) return -6;
    if (Tn > 1 && !A) return -7;
    if (Tn > 1 && !b) return -8;
    if (Tn > 1 && !cholQ) return -9;
    if (!eps || reinterpret_cast<uintptr_t>(eps) % sizeof(T)) return -10;
    if (!out || reinterpret_cast<uintptr_t>(out) % sizeof(T)) return -11;
    Plan p = make_plan(B, S, Tn, chunks);
    const size_t need = workspace_elems<T>(B, S, d, p) * sizeof(T);
    if (p.C > 1 && (!ws || ws_bytes < need || reinterpret_cast<uintptr_t>(ws) % sizeof(T))) p = make_plan(B, S, Tn, 1);
    Args<T> a;
    a.B = B, a.S = S, a.Tn = Tn, a.R = S * B, a.L = p.L, a.CU = 0, a.sblocks = 0;
    a.mu0 = mu0, a.cholP0 = cholP0, a.A = A, a.b = b, a.cholQ = cholQ, a.eps = eps, a.out = out;
    a.phi = static_cast<T*>(ws);
    a.v = a.phi + (p.C > 1 ? size_t(p.C - 1) * d * d * B : 0);
    a.xin = a.v + (p.C > 1 ? size_t(p.C - 1) * d * a.R : 0);
    a.mis_eps = misalignment(eps, sizeof(T)), a.mis_out = misalignment(out, sizeof(T));
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (d) {
        case 1: return launch_d<T, 1>(a, p, st);
        case 2: return launch_d<T, 2>(a, p, st);
        case 3: return launch_d<T, 3>(a, p, st);
        case 4: return launch_d<T, 4>(a, p, st);
        case 5: return launch_d<T, 5>(a, p, st);
        case 6: return launch_d<T, 6>(a, p, st);
        case 7: return launch_d<T, 7>(a, p, st);
        case 8: return launch_d<T, 8>(a, p, st);
        default: return launch_d<T, 9>(a, p, st);
    }
}
}   // namespace

extern "C" {
size_t mf_ssm_sample_workspace_bytes(int64_t B, int64_t S, int64_t T, int d, int elem_size, int64_t chunks) {
    if (B <= 0 || S <= 0 || T < 1 || d < 1 || d > MAX_D || chunks < 0 || (elem_size != 4 && elem_size != 8)) return 0;
    const Plan p = make_plan(B, S, T, chunks);
    return workspace_elems<double>(B, S, d, p) * size_t(elem_size);
}
int mf_ssm_sample_f64(int64_t B, int64_t S, int64_t T, int d, const double* mu0, const double* cholP0, const double* A, const double* b,
                      const double* cholQ, const double* eps, double* out, void* ws, size_t ws_bytes, int64_t chunks, void* stream) {
    return run_sample<double>(B, S, T, d, mu0, cholP0, A, b, cholQ, eps, out, ws, ws_bytes, chunks, stream);
}
int mf_ssm_sample_f32(int64_t B, int64_t S, int64_t T, int d, const float* mu0, const float* cholP0, const float* A, const float* b,
                      const float* cholQ, const float* eps, float* out, void* ws, size_t ws_bytes, int64_t chunks, void* stream) {
    return run_sample<float>(B, S, T, d, mu0, cholP0, A, b, cholQ, eps, out, ws, ws_bytes, chunks, stream);
}
}
