// StateSpaceModel.log_pdf (markovflow/state_space_model.py:485-526) and its adjoints on the chain's own leaves: with
//   r_0 = x_0 - mu0,   r_k = x_k - (b_{k-1} + A_{k-1} x_{k-1}),   z_k = L_k^-1 r_k,   u_k = L_k^-T z_k
// (L_k the LOWER TRIANGLE of cholP0 for k = 0 and of cholQ_{k-1} after it; nothing above the diagonal is read),
//   out[s, b]  = sum_k ( -1/2 |z_k|^2 - sum_i log|L_k,ii| ) - 1/2 T d log 2 pi,
//   g_x_k      = -g (u_k - A_k^T u_{k+1}),          g_mu0 / g_b_{k-1} = sum_s g u_k,        g_A_{k-1} = sum_s g u_k x_{k-1}^T,
//   g_L_k      = tril(sum_s g u_k z_k^T) - diag((sum_s g) / L_k,ii).
//
// Work split (mf_sample.hip's).  A UNIT is (series, chunk of L consecutive factors); a GROUP of G lanes (16 for S <= 16, else 64 - a
// function of S alone) walks one unit, its lanes are G samples of that series; a wavefront holds 64 / G groups on consecutive units and a
// block is one wavefront.  There is NO recurrence: factor k needs x_{k-1}, x_k and block k only, so chunks need no summaries - a chunk
// reads one LEAD row (x_{k0-1}) in front of its own and, for the adjoint, one TRAIL row behind them, whose factor it evaluates a second
// time for A^T u alone.  A_k, b_k, L_k reach a group as uniform-address loads, the reciprocals of the diagonal are formed once per step,
// and the two triangular solves run in the lane's registers with x_{k-1} carried.
//
// States and g_x.  The rows are T d apart across lanes, so they move through LDS tiles by mf_sample.hip's front end: tiles of
// TS = 240 / (d sizeof) steps, 16 lanes per row, a lane per 16-byte ALIGNED piece, element-wise at the straddling ends, odd row stride, the
// next tile fetched into registers before this tile's steps run.  The adjoint writes g_x IN PLACE over x, one slot LATE: row k is
// complete only after factor k + 1 has added A_k^T g u_{k+1}, so a tile's rows land in slots 1 ... TS, slot 0 holds the last row of
// the tile before (carried in registers across the barrier), and the store walk writes slots 0 ... TS - 1 (and the chunk's final row).
//
// Sums.  The value: a lane adds its factors in ascending k and leaves one partial per (sample, chunk); a second launch adds a
// trajectory's chunks in ascending order (one chunk: the walk writes `out` itself).  It depends on `chunks` and on nothing else.
// Parameter adjoints are sums over SAMPLES: per step the lanes leave g u, z and x_{k-1} in LDS and a lane per output entry
// (2 d^2 + d of them per group: A, the square of L with zeros above the diagonal, b) adds the block's samples in ascending order from
// LDS broadcasts; with more than one block of G samples each block writes its own slab of the workspace and a second launch adds
// the slabs in ascending order.  No atomics: every output has the same bits on every launch, whatever else is asked for, and a
// series alone gives the bits it gives in a batch (G and the slabs depend on S alone; the adjoints do not depend on `chunks`).
#include "../../include/markovflow_amd.h"

#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

namespace {
constexpr int MAX_D = 9;
constexpr int ROW_BYTES = 240;         // a trajectory's row of a tile, at the most: it meets 16 aligned pieces wherever it starts
constexpr long TARGET_WAVES = 2048;    // chunks = 0: wavefronts the walk aims at (two per SIMD)
constexpr long MIN_CHUNK = 8;          // chunks = 0: factors per chunk, at the least (a chunk re-reads one or two rows)

template <typename T> struct Vec16;
template <> struct Vec16<double> { typedef double type __attribute__((ext_vector_type(2))); };
template <> struct Vec16<float> { typedef float type __attribute__((ext_vector_type(4))); };

__device__ __forceinline__ double log_abs(double v) { return log(fabs(v)); }
__device__ __forceinline__ float log_abs(float v) { return logf(fabsf(v)); }

template <typename T>
struct Args {
    long B, S, Tn, R;                  // R = S B trajectories
    long L, C;                         // factors per chunk, chunks per series
    long sblocks;                      // blocks of G samples
    const T *mu0, *cholP0, *A, *b, *cholQ, *x, *g;
    T *out, *part;                     // value: [S, B] (one chunk) or the partials [chunk][trajectory]
    T cst;                             // -1/2 T d log 2 pi
    T *gx, *g_mu0, *g_P0, *g_A, *g_b, *g_Q;
    long slab;                         // elements between the parameter adjoints of consecutive sample blocks (0: one block, the outputs)
    int mis_x, mis_gx;                 // elements between the last 16-byte boundary and x / g_x
};

// Offset IN THE ROW of the first element of aligned piece c: the row starts at element g0 >= 0 of an array whose first element lies
// `mis` elements past a 16-byte boundary.  Above -VEC; piece 0 is the one that holds the row's first element.
template <typename T>
__device__ __forceinline__ int piece_offset(long g0, int mis, int c) {
    constexpr int VEC = 16 / sizeof(T);
    return c * VEC - int((g0 + mis) % VEC);
}

// MODE 0: the value, 1: the adjoints (g_x and / or the five parameter adjoints: uniform run-time choices, one code path).
template <typename T, int D, int G, int MODE>
__global__ void __launch_bounds__(64) walk_kernel(Args<T> a) {
    using V = typename Vec16<T>::type;
    constexpr int VEC = 16 / sizeof(T), CH = 16, NG = 64 / G;
    constexpr int TS = ROW_BYTES / int(sizeof(T)) / D, SH = MODE, RS = ((TS + SH) * D) | 1;   // steps per tile; slots shifted; odd stride
    constexpr int SD = D | 1, E = 2 * D * D + D;                                              // per-sample stride; entries per group and step
    __shared__ T tile[64 * RS];
    __shared__ long rbase[64];         // element of x / g_x at which row r starts (its lead row when it has one)
    __shared__ int rrows[64], rlead[64], rlen[64];                   // rows of row r in all, its lead rows (0 / 1), its own factors
    __shared__ T su[MODE ? 64 * SD : 1], sz[MODE ? 64 * SD : 1], sx[MODE ? 64 * SD : 1], sg[MODE ? 64 : 1];
    __shared__ long gfirst[NG], gseries[NG];                         // per group: step of its row 0, its series
    const int lane = threadIdx.x, sub = lane >> 4, c = lane & 15;    // piece c of rows sub, sub + 4, ...
    const int grp = lane / G, j = lane % G;
    const long ublock = blockIdx.x / a.sblocks, sblock = blockIdx.x - ublock * a.sblocks;
    const long u = ublock * NG + grp, s = sblock * G + j;
    const bool unit = u < a.B * a.C, valid = unit && s < a.S;
    const long series = unit ? u / a.C : 0, chunk = unit ? u - series * a.C : 0;
    const long traj = valid ? s * a.B + series : 0, k0 = chunk * a.L;
    const int len = unit ? int(a.Tn - k0 < a.L ? a.Tn - k0 : a.L) : 0;
    const int lead = k0 > 0 ? 1 : 0, trail = MODE == 1 && unit && k0 + len < a.Tn ? 1 : 0;
    const int nrows = valid ? lead + len + trail : 0;
    const long kfirst = k0 - lead;
    const bool want_x = MODE == 1 && a.gx != nullptr, want_p = MODE == 1 && a.g_mu0 != nullptr;
    rbase[lane] = valid ? (traj * a.Tn + kfirst) * D : 0;
    rrows[lane] = nrows, rlead[lane] = lead, rlen[lane] = valid ? len : 0;
    if (j == 0) gfirst[grp] = kfirst, gseries[grp] = series;
    T gval = T(0);
    if (MODE == 1) {
        if (valid) gval = a.g[traj];
        sg[lane] = gval;
    }
    __syncthreads();
    int bmax = 0;                      // rows of the block's longest unit (lane 0 of a group has a sample whenever the unit exists)
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) bmax = rrows[gi * G] > bmax ? rrows[gi * G] : bmax;
    const int ns = int(a.S - sblock * G < G ? a.S - sblock * G : G);

    auto steps_of = [&](int r, int t0) {
        const int n = rrows[r] - t0;
        return n < 0 ? 0 : n < TS ? n : TS;
    };
    V body[CH];                        // the next tile of x: this lane's piece of 16 rows
    auto fetch = [&](int t0) {
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            const int r = 4 * q + sub, n = steps_of(r, t0) * D;
            body[q] = V(T(0));
            const long g0 = rbase[r] + long(t0) * D;
            const int e0 = piece_offset<T>(g0, a.mis_x, c);
            if (e0 >= n) continue;
            if (e0 >= 0 && e0 + VEC <= n) {
                body[q] = *reinterpret_cast<const V*>(a.x + g0 + e0);
            } else {
#pragma unroll
                for (int w = 0; w < VEC; ++w)
                    if (e0 + w >= 0 && e0 + w < n) body[q][w] = a.x[g0 + e0 + w];
            }
        }
    };

    T xp[D], pend[D], acc = T(0);      // x_{k-1}; the tile's last row of g_x, complete after the next tile's first factor
#pragma unroll
    for (int i = 0; i < D; ++i) xp[i] = pend[i] = T(0);
    fetch(0);
    // the adjoint runs one tile past the rows: the chunk's final row leaves through slot 0 when the rows fill their last tile
    for (int t0 = 0; t0 < bmax + SH; t0 += TS) {
        __syncthreads();               // the previous tile's store has read the rows
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            const int r = 4 * q + sub, n = steps_of(r, t0) * D;
            const int e0 = piece_offset<T>(rbase[r] + long(t0) * D, a.mis_x, c);
#pragma unroll
            for (int w = 0; w < VEC; ++w)
                if (e0 + w >= 0 && e0 + w < n) tile[r * RS + SH * D + e0 + w] = body[q][w];
        }
        if (MODE == 1) {
#pragma unroll
            for (int i = 0; i < D; ++i) tile[lane * RS + i] = pend[i];
        }
        __syncthreads();
        if (t0 + TS < bmax) fetch(t0 + TS);
        const int n_own = steps_of(lane, t0);
        int nmax = 0;
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) nmax = steps_of(gi * G, t0) > nmax ? steps_of(gi * G, t0) : nmax;
        for (int st = 0; st < nmax; ++st) {
            const int rho = t0 + st;
            const bool row = st < n_own, fac = row && rho >= lead, own = fac && rho < lead + len;
            const long k = kfirst + rho;
            T xi[D], z[D], gu[D];
#pragma unroll
            for (int i = 0; i < D; ++i) xi[i] = row ? tile[lane * RS + (SH + st) * D + i] : T(0), z[i] = gu[i] = T(0);
            if (fac) {
                const long ci = k > 0 ? series * (a.Tn - 1) + k - 1 : 0;
                const T* __restrict__ Lk = k > 0 ? a.cholQ + ci * (D * D) : a.cholP0 + series * (D * D);
                const T* __restrict__ Ak = a.A + ci * (D * D);
                T rinv[D], ld = T(0), q = T(0);
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    const T lii = Lk[i * D + i];
                    rinv[i] = T(1) / lii;
                    if (MODE == 0) ld += log_abs(lii);
                }
#pragma unroll
                for (int i = 0; i < D; ++i) {          // r, then z by forward substitution
                    T m;
                    if (k > 0) {
                        m = a.b[ci * D + i];
#pragma unroll
                        for (int l = 0; l < D; ++l) m += Ak[i * D + l] * xp[l];
                    } else {
                        m = a.mu0[series * D + i];
                    }
                    T v = xi[i] - m;
#pragma unroll
                    for (int l = 0; l < i; ++l) v -= Lk[i * D + l] * z[l];
                    z[i] = v * rinv[i];
                    q += z[i] * z[i];
                }
                if (MODE == 0) acc += T(-0.5) * q - ld;
                if (MODE == 1) {
#pragma unroll
                    for (int i = D - 1; i >= 0; --i) {  // u by back substitution with the same triangle
                        T v = z[i];
#pragma unroll
                        for (int l = i + 1; l < D; ++l) v -= Lk[l * D + i] * gu[l];
                        gu[i] = v * rinv[i];
                    }
#pragma unroll
                    for (int i = 0; i < D; ++i) gu[i] *= gval;
                    if (want_x) {
                        if (own) {
#pragma unroll
                            for (int i = 0; i < D; ++i) tile[lane * RS + (SH + st) * D + i] = -gu[i];
                        }
                        if (k > 0 && rho > lead) {     // the row before this one is the chunk's own: its second term
#pragma unroll
                            for (int l = 0; l < D; ++l) {
                                T t = T(0);
#pragma unroll
                                for (int i = 0; i < D; ++i) t += Ak[i * D + l] * gu[i];
                                tile[lane * RS + st * D + l] += t;
                            }
                        }
                    }
                }
            }
            if (want_p) {
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    su[lane * SD + i] = own ? gu[i] : T(0);
                    sz[lane * SD + i] = own ? z[i] : T(0);
                    sx[lane * SD + i] = own ? xp[i] : T(0);
                }
                __syncthreads();
                for (int o = lane; o < NG * E; o += 64) {
                    const int gi = o / E, e = o - gi * E, r0 = gi * G;
                    if (rho < rlead[r0] || rho >= rlead[r0] + rlen[r0]) continue;
                    const long ko = gfirst[gi] + rho, so = gseries[gi];
                    const int kind = e < D * D ? 0 : e < 2 * D * D ? 1 : 2;
                    const int e1 = e - kind * D * D, i = kind == 2 ? e1 : e1 / D, l = kind == 2 ? 0 : e1 % D;
                    if (kind == 0 && ko == 0) continue;
                    const long co = ko > 0 ? so * (a.Tn - 1) + ko - 1 : so;
                    T* dst;
                    if (kind == 0) dst = a.g_A + (co * D + i) * D + l;
                    else if (kind == 1) dst = (ko > 0 ? a.g_Q : a.g_P0) + (co * D + i) * D + l;
                    else dst = (ko > 0 ? a.g_b : a.g_mu0) + co * D + i;
                    T sum = T(0);
                    if (!(kind == 1 && l > i)) {
                        const T* second = kind == 0 ? sx : sz;
                        for (int sm = 0; sm < ns; ++sm) {
                            const T v = kind == 2 ? T(1) : second[(r0 + sm) * SD + l];
                            sum += su[(r0 + sm) * SD + i] * v;
                        }
                        if (kind == 1 && l == i) {
                            T gs = T(0);
                            for (int sm = 0; sm < ns; ++sm) gs += sg[r0 + sm];
                            sum -= gs / (ko > 0 ? a.cholQ : a.cholP0)[(co * D + i) * D + i];
                        }
                    }
                    dst[sblock * a.slab] = sum;
                }
                __syncthreads();
            }
            if (row) {
#pragma unroll
                for (int i = 0; i < D; ++i) xp[i] = xi[i];
            }
        }
        if (MODE == 1) {
            if (n_own == TS) {
#pragma unroll
                for (int i = 0; i < D; ++i) pend[i] = tile[lane * RS + TS * D + i];
            }
            if (want_x) {
                __syncthreads();
#pragma unroll
                for (int q = 0; q < CH; ++q) {
                    // slots 0 ... m - 1 are rows t0 - 1 ... t0 + m - 2; the chunk's own rows among them leave
                    const int r = 4 * q + sub, nr = steps_of(r, t0), m = nr < TS ? nr + 1 : TS;
                    const int sa = rlead[r] - (t0 - 1) > 0 ? rlead[r] - (t0 - 1) : 0;
                    const int sb = rlead[r] + rlen[r] - (t0 - 1) < m ? rlead[r] + rlen[r] - (t0 - 1) : m;
                    if (sb <= sa) continue;
                    const long g0 = rbase[r] + long(t0 - 1 + sa) * D;
                    const int n = (sb - sa) * D, toff = r * RS + sa * D;
                    const int e0 = piece_offset<T>(g0, a.mis_gx, c);
                    if (e0 >= n) continue;
                    if (e0 >= 0 && e0 + VEC <= n) {
                        V val;
#pragma unroll
                        for (int w = 0; w < VEC; ++w) val[w] = tile[toff + e0 + w];
                        *reinterpret_cast<V*>(a.gx + g0 + e0) = val;
                    } else {
#pragma unroll
                        for (int w = 0; w < VEC; ++w)
                            if (e0 + w >= 0 && e0 + w < n) a.gx[g0 + e0 + w] = tile[toff + e0 + w];
                    }
                }
            }
        }
    }
    if (MODE == 0 && valid) {
        if (a.C == 1) a.out[traj] = acc + a.cst;
        else a.part[chunk * a.R + traj] = acc;
    }
}

// out = ((p_0 + p_1) + ...) + cst over a trajectory's chunks, a lane per trajectory.
template <typename T>
__global__ void __launch_bounds__(64) chunk_sum_kernel(long R, long C, T cst, const T* __restrict__ part, T* __restrict__ out) {
    const long r = (long)blockIdx.x * 64 + threadIdx.x;
    if (r >= R) return;
    T sum = part[r];
    for (long c = 1; c < C; ++c) sum += part[c * R + r];
    out[r] = sum + cst;
}

// The parameter adjoints from the slabs of the sample blocks, ascending; a slab is the five outputs one behind the other.
template <typename T>
struct Slabs {
    long n[5], blocks, slab;
    const T* ws;
    T* dst[5];
};
template <typename T>
__global__ void __launch_bounds__(64) slab_sum_kernel(Slabs<T> s) {
    const long idx = (long)blockIdx.x * 64 + threadIdx.x;
    if (idx >= s.slab) return;
    T sum = s.ws[idx];
    for (long p = 1; p < s.blocks; ++p) sum += s.ws[p * s.slab + idx];
    long off = idx;
    int which = 0;
    while (off >= s.n[which]) off -= s.n[which++];
    s.dst[which][off] = sum;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct Plan {
    long C, L;                         // chunks per series and factors per chunk
    int G;                             // lanes of a group
};

inline long ceil_div(long a, long b) { return (a + b - 1) / b; }

// chunks: 0 automatic (enough chunks of at least MIN_CHUNK factors for TARGET_WAVES wavefronts), >= 1 that many, clamped to T; chunks
// of ceil(T / chunks) factors, a request that this length cannot honour exactly rounded down to the chunks that are not empty.
inline Plan make_plan(long B, long S, long Tn, long chunks) {
    Plan p;
    p.G = S > 16 ? 64 : 16;
    long C = chunks;
    if (chunks == 0) {
        const long waves = ceil_div(B, 64 / p.G) * ceil_div(S, p.G);
        C = ceil_div(TARGET_WAVES, waves);
        if (C > Tn / MIN_CHUNK) C = Tn / MIN_CHUNK;
        if (C < 1) C = 1;
    }
    if (C > Tn) C = Tn;
    p.L = ceil_div(Tn, C);
    p.C = ceil_div(Tn, p.L);
    return p;
}

inline size_t slab_elems(long B, long Tn, int d) { return size_t(B) * (d + d * d) + size_t(B) * (Tn - 1) * (2 * d * d + d); }

inline int misalignment(const void* ptr, size_t elem) { return int((reinterpret_cast<uintptr_t>(ptr) % 16) / elem); }

template <typename T, int D, int MODE>
int launch_walk(Args<T> a, const Plan& p, hipStream_t st) {
    a.sblocks = ceil_div(a.S, p.G);
    const long blocks = ceil_div(a.B * a.C, 64 / p.G) * a.sblocks;
    if (blocks > 0x7fffffffL) return -1;
    if (p.G == 16) hipLaunchKernelGGL((walk_kernel<T, D, 16, MODE>), dim3((unsigned)blocks), dim3(64), 0, st, a);
    else hipLaunchKernelGGL((walk_kernel<T, D, 64, MODE>), dim3((unsigned)blocks), dim3(64), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

template <typename T, int MODE>
int launch_d(int d, const Args<T>& a, const Plan& p, hipStream_t st) {
    switch (d) {
        case 1: return launch_walk<T, 1, MODE>(a, p, st);
        case 2: return launch_walk<T, 2, MODE>(a, p, st);
        case 3: return launch_walk<T, 3, MODE>(a, p, st);
        case 4: return launch_walk<T, 4, MODE>(a, p, st);
        case 5: return launch_walk<T, 5, MODE>(a, p, st);
        case 6: return launch_walk<T, 6, MODE>(a, p, st);
        case 7: return launch_walk<T, 7, MODE>(a, p, st);
        case 8: return launch_walk<T, 8, MODE>(a, p, st);
        default: return launch_walk<T, 9, MODE>(a, p, st);
    }
}

// The checks the two entry points share; 1 when there is nothing to do, 0 to go on.
template <typename T>
int check_chain(int64_t B, int64_t S, int64_t Tn, int d, const T* mu0, const T* cholP0, const T* A, const T* b, const T* cholQ,
                const T* states, int64_t chunks, int chunks_pos) {
    if (B < 0) return -1;
    if (S < 0 || (B > 0 && S > int64_t(0x7fffffff) * 16 / B)) return -2;
    if (Tn < 1) return -3;
    if (d < 1) return -4;
    if (chunks < 0) return -chunks_pos;
    if (d > MAX_D) return -100;
    if (B == 0 || S == 0) return 1;
    if (!mu0) return -5;
    if (!cholP0) return -6;
    if (Tn > 1 && !A) return -7;
    if (Tn > 1 && !b) return -8;
    if (Tn > 1 && !cholQ) return -9;
    if (!states || reinterpret_cast<uintptr_t>(states) % sizeof(T)) return -10;
    return 0;
}

template <typename T>
Args<T> chain_args(int64_t B, int64_t S, int64_t Tn, const Plan& p, const T* mu0, const T* cholP0, const T* A, const T* b, const T* cholQ,
                   const T* states) {
    Args<T> a = {};
    a.B = B, a.S = S, a.Tn = Tn, a.R = S * B, a.L = p.L, a.C = p.C;
    a.mu0 = mu0, a.cholP0 = cholP0, a.A = A, a.b = b, a.cholQ = cholQ, a.x = states;
    a.mis_x = misalignment(states, sizeof(T));
    return a;
}

template <typename T>
int run_value(int64_t B, int64_t S, int64_t Tn, int d, const T* mu0, const T* cholP0, const T* A, const T* b, const T* cholQ,
              const T* states, T* out, void* ws, size_t ws_bytes, int64_t chunks, void* stream) {
    const int rc = check_chain(B, S, Tn, d, mu0, cholP0, A, b, cholQ, states, chunks, 14);
    if (rc) return rc < 0 ? rc : 0;
    if (!out) return 0;
    const Plan p = make_plan(B, S, Tn, chunks);
    if (p.C > 1) {
        if (!ws || reinterpret_cast<uintptr_t>(ws) % sizeof(T)) return -12;
        if (ws_bytes < size_t(p.C) * S * B * sizeof(T)) return -13;
    }
    Args<T> a = chain_args(B, S, Tn, p, mu0, cholP0, A, b, cholQ, states);
    a.out = out, a.part = static_cast<T*>(ws);
    a.cst = T(-0.5 * double(Tn) * d * 1.8378770664093454835606594728112);       // log 2 pi
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int lrc = launch_d<T, 0>(d, a, p, st);
    if (lrc || p.C == 1) return lrc;
    hipLaunchKernelGGL((chunk_sum_kernel<T>), dim3((unsigned)ceil_div(a.R, 64)), dim3(64), 0, st, a.R, p.C, a.cst, a.part, out);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

template <typename T>
int run_grad(int64_t B, int64_t S, int64_t Tn, int d, const T* mu0, const T* cholP0, const T* A, const T* b, const T* cholQ,
             const T* states, const T* g, T* g_states, T* g_mu0, T* g_cholP0, T* g_A, T* g_b, T* g_cholQ, void* ws, size_t ws_bytes,
             int64_t chunks, void* stream) {
    const int rc = check_chain(B, S, Tn, d, mu0, cholP0, A, b, cholQ, states, chunks, 20);
    if (rc) return rc < 0 ? rc : 0;
    T* const params[5] = {g_mu0, g_cholP0, g_A, g_b, g_cholQ};
    const int np = Tn > 1 ? 5 : 2;     // without a transition there is nothing behind g_A, g_b, g_cholQ
    int wanted = 0;
    for (int i = 0; i < np; ++i) wanted += params[i] != nullptr;
    if (!g_states && wanted == 0) return 0;
    if (!g) return -11;
    if (g_states && reinterpret_cast<uintptr_t>(g_states) % sizeof(T)) return -12;
    for (int i = 0; i < np; ++i)       // all five or none
        if (wanted && !params[i]) return -(13 + i);
    const Plan p = make_plan(B, S, Tn, chunks);
    const long sblocks = ceil_div(S, p.G);
    const size_t slab = slab_elems(B, Tn, d);
    const bool slabs = wanted && sblocks > 1;
    if (slabs) {
        if (!ws || reinterpret_cast<uintptr_t>(ws) % sizeof(T)) return -18;
        if (ws_bytes < size_t(sblocks) * slab * sizeof(T)) return -19;
    }
    Args<T> a = chain_args(B, S, Tn, p, mu0, cholP0, A, b, cholQ, states);
    a.g = g, a.gx = g_states, a.mis_gx = misalignment(g_states, sizeof(T));
    Slabs<T> sl = {};
    sl.n[0] = B * d, sl.n[1] = B * d * d, sl.n[2] = B * (Tn - 1) * d * d, sl.n[3] = B * (Tn - 1) * d, sl.n[4] = sl.n[2];
    sl.blocks = sblocks, sl.slab = long(slab), sl.ws = static_cast<const T*>(ws);
    for (int i = 0; i < 5; ++i) sl.dst[i] = params[i];
    if (wanted) {
        T* base = static_cast<T*>(ws);
        a.slab = slabs ? long(slab) : 0;
        a.g_mu0 = slabs ? base : g_mu0;
        a.g_P0 = slabs ? base + sl.n[0] : g_cholP0;
        a.g_A = slabs ? base + sl.n[0] + sl.n[1] : g_A;
        a.g_b = slabs ? base + sl.n[0] + sl.n[1] + sl.n[2] : g_b;
        a.g_Q = slabs ? base + sl.n[0] + sl.n[1] + sl.n[2] + sl.n[3] : g_cholQ;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int lrc = launch_d<T, 1>(d, a, p, st);
    if (lrc || !slabs) return lrc;
    if (ceil_div(long(slab), 64) > 0x7fffffffL) return -1;
    hipLaunchKernelGGL((slab_sum_kernel<T>), dim3((unsigned)ceil_div(long(slab), 64)), dim3(64), 0, st, sl);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

inline bool query_ok(int64_t B, int64_t S, int64_t T, int d, int elem_size, int64_t chunks) {
    return B > 0 && S > 0 && T >= 1 && d >= 1 && d <= MAX_D && chunks >= 0 && (elem_size == 4 || elem_size == 8);
}
}   // namespace

extern "C" {
size_t mf_ssm_log_pdf_workspace_bytes(int64_t B, int64_t S, int64_t T, int d, int elem_size, int64_t chunks) {
    if (!query_ok(B, S, T, d, elem_size, chunks)) return 0;
    const Plan p = make_plan(B, S, T, chunks);
    return p.C > 1 ? size_t(p.C) * S * B * size_t(elem_size) : 0;
}
int mf_ssm_log_pdf_f64(int64_t B, int64_t S, int64_t T, int d, const double* mu0, const double* cholP0, const double* A, const double* b,
                       const double* cholQ, const double* states, double* out, void* ws, size_t ws_bytes, int64_t chunks, void* stream) {
    return run_value<double>(B, S, T, d, mu0, cholP0, A, b, cholQ, states, out, ws, ws_bytes, chunks, stream);
}
int mf_ssm_log_pdf_f32(int64_t B, int64_t S, int64_t T, int d, const float* mu0, const float* cholP0, const float* A, const float* b,
                       const float* cholQ, const float* states, float* out, void* ws, size_t ws_bytes, int64_t chunks, void* stream) {
    return run_value<float>(B, S, T, d, mu0, cholP0, A, b, cholQ, states, out, ws, ws_bytes, chunks, stream);
}
size_t mf_ssm_log_pdf_grad_workspace_bytes(int64_t B, int64_t S, int64_t T, int d, int elem_size, int64_t chunks) {
    if (!query_ok(B, S, T, d, elem_size, chunks)) return 0;
    const long sblocks = ceil_div(S, make_plan(B, S, T, chunks).G);
    return sblocks > 1 ? size_t(sblocks) * slab_elems(B, T, d) * size_t(elem_size) : 0;
}
int mf_ssm_log_pdf_grad_f64(int64_t B, int64_t S, int64_t T, int d, const double* mu0, const double* cholP0, const double* A,
                            const double* b, const double* cholQ, const double* states, const double* g, double* g_states, double* g_mu0,
                            double* g_cholP0, double* g_A, double* g_b, double* g_cholQ, void* ws, size_t ws_bytes, int64_t chunks,
                            void* stream) {
    return run_grad<double>(B, S, T, d, mu0, cholP0, A, b, cholQ, states, g, g_states, g_mu0, g_cholP0, g_A, g_b, g_cholQ, ws, ws_bytes,
                            chunks, stream);
}
int mf_ssm_log_pdf_grad_f32(int64_t B, int64_t S, int64_t T, int d, const float* mu0, const float* cholP0, const float* A, const float* b,
                            const float* cholQ, const float* states, const float* g, float* g_states, float* g_mu0, float* g_cholP0,
                            float* g_A, float* g_b, float* g_cholQ, void* ws, size_t ws_bytes, int64_t chunks, void* stream) {
    return run_grad<float>(B, S, T, d, mu0, cholP0, A, b, cholQ, states, g, g_states, g_mu0, g_cholP0, g_A, g_b, g_cholQ, ws, ws_bytes,
                           chunks, stream);
}
}
