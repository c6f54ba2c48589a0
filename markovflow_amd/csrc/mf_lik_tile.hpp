// What the tile-parallel data terms share (mf_lik.hip: the single-latent and multi-latent SVGP pairs, sparse power EP, the importance
// weights; mf_lik_factor.hip; mf_lik_stack.hip; mf_st.hip): the front end of pass 1 - the tile locator that clamps the caller's table,
// the staging of a tile's rows of w, the store of a workspace row -, pass 2 of the SVGP terms, and on the host side the launch helper,
// the switch over two_d and the argument checks of the segmentation and the tile table.
// The helpers take the LDS buffers and a lane's entries as references to arrays, and the loops over a tile's points stay in the
// kernels: inlined, they then index and load exactly as the kernels would, and the register allocation stays what it was.  What is
// NOT here is the `kind` table of a lane's entries in the multi-latent, factor and stack kernels: moved into a helper - as a whole, entry
// by entry, or at K = 1 only - it costs the float64 instantiations two to twelve more spilled SGPRs
// (profiles/lik_tile_front_end_resources_and_ab.txt), so each of the three kernels keeps its own lines.
#pragma once

#include "mf_lik_math.hpp"

namespace {

// ---- device side -----------------------------------------------------------------------------------------------------------------
// Tile t of the caller's table: tile_seg[t] = series * S + segment, seg_tile[series * S + segment] = the first tile of the segment (a
// prefix sum, B S + 1 entries); tile j of a segment starts at the segment's first point + TILE j.  The table and the offsets are
// clamped here, not trusted: a wrong one gives npts = 0 or wrong numbers and no access outside the buffers.
struct TileAt {
    long bs, b, s;                     // series * S + segment, and the two
    long k_lo, k_hi;                   // the segment's points
    long k0;                           // the tile's first point
    int npts;                          // (0 only for a table that disagrees with the offsets)
};
template <int TILE>
__device__ __forceinline__ TileAt locate_tile(long t, long N, int S, long BS, const long long* seg, const long long* tile_seg,
                                              const long long* seg_tile) {
    TileAt a;
    a.bs = (long)tile_seg[t];
    a.bs = a.bs < 0 ? 0 : (a.bs >= BS ? BS - 1 : a.bs);
    a.b = a.bs / S;
    a.s = a.bs - a.b * S;
    a.k_lo = (long)seg[a.b * (S + 1) + a.s];
    a.k_hi = (long)seg[a.b * (S + 1) + a.s + 1];
    clamp_range(a.k_lo, a.k_hi, N);
    const long j = t - (long)seg_tile[a.bs];                        // this tile's number within its segment
    a.k0 = (j >= 0 && j <= (a.k_hi - a.k_lo) / TILE) ? a.k_lo + TILE * j : a.k_hi;
    a.npts = a.k_hi - a.k0 < TILE ? int(a.k_hi - a.k0) : TILE;
    return a;
}

// entry e of a packed lower triangle is (i, j <= i)
__device__ __forceinline__ void tri_decode(int e, int& i, int& j) {
    i = 0;
    while ((i + 1) * (i + 2) / 2 <= e) ++i;
    j = e - i * (i + 1) / 2;
}

// the accumulator has the triangle, the vector and one scalar per row of LDS values beyond the first two
constexpr int seg_entries(int d2, int rows) { return d2 * (d2 + 1) / 2 + d2 + rows - 2; }

// a workspace row of the SVGP terms: per chain the triangle of g_cov and g_mean, then sum ve (k = 1: seg_entries(d2, 3))
constexpr int expect_entries(int k, int d2) { return k * (d2 * (d2 + 1) / 2 + d2) + 1; }
constexpr size_t expect_row(int two_d) { return size_t(expect_entries(1, two_d)); }

// npts rows of RW elements into LDS at column col0 of rows of STRIDE elements: coalesced global loads; STRIDE is odd (RW + 1 for a
// row on its own), so the lanes' rows start on distinct banks
template <typename T, int RW, int STRIDE = RW + 1, int NW>
__device__ __forceinline__ void stage_tile(int lane, int npts, const T* wt, T (&lw)[NW], int col0 = 0) {
    for (int idx = lane; idx < npts * RW; idx += 64) lw[(idx / RW) * STRIDE + col0 + idx % RW] = wt[idx];
}

// this lane's entries into the tile's workspace row of E values: one contiguous row, coalesced stores
template <int E, typename T, int R>
__device__ __forceinline__ void store_row(T* ws_row, int lane, const T (&part)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = lane + 64 * r;
        if (e < E) ws_row[e] = part[r];
    }
}

//   pass 2 of the SVGP terms, one block per (series, segment), a lane per entry: the segment's rows are added in ascending tile
//            order, the outputs are written - chain k of K to row (series * K + k) * S + segment of g_mean / g_cov - and every
//            triangle mirrored.  An empty segment writes zeros.
template <typename T, int K, int D2>
__global__ void __launch_bounds__(256) expect_reduce_kernel(long num_tiles, int S, const long long* __restrict__ seg_tile,
                                                            const T* __restrict__ ws, T* __restrict__ ve_sum, T* __restrict__ g_mean,
                                                            T* __restrict__ g_cov) {
    constexpr int TRI = D2 * (D2 + 1) / 2, PER = TRI + D2, E = expect_entries(K, D2);
    const long bs = blockIdx.x;
    const long b = bs / S;
    const long s = bs - b * S;
    long t_lo = 0, t_hi = 0;
    if (seg_tile) {                                // (NULL: no points at all)
        t_lo = (long)seg_tile[bs];
        t_hi = (long)seg_tile[bs + 1];
        clamp_range(t_lo, t_hi, num_tiles);
    }
    for (int e = threadIdx.x; e < E; e += 256) {
        if (e < E - 1 ? !g_mean : !ve_sum) continue;
        T acc = T(0);
        for (long t = t_lo; t < t_hi; ++t) acc += ws[t * E + e];
        if (e == E - 1) {
            ve_sum[bs] = acc;
            continue;
        }
        const int k = e / PER, f = e - k * PER;
        const long row = K == 1 ? bs : (b * K + k) * S + s;        // (K = 1: b S + s is bs itself)
        if (f < TRI) {
            int i, c;
            tri_decode(f, i, c);
            g_cov[row * (D2 * D2) + i * D2 + c] = acc;
            g_cov[row * (D2 * D2) + c * D2 + i] = acc;
        } else {
            g_mean[row * D2 + (f - TRI)] = acc;
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// one launch; the arguments are converted to the kernel's parameter types (NULL to a typed pointer, int64_t to long or int)
template <typename... Params, typename... Args>
int launch(void (*kernel)(Params...), int64_t grid, unsigned block, void* stream, const Args&... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(block), 0, static_cast<hipStream_t>(stream), static_cast<Params>(args)...);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

// the pair dimension as a compile-time constant: f(std::integral_constant<int, two_d>) for an even two_d in MIN ... 18, `err` for any
// other; nothing is instantiated below MIN
template <int MIN, typename F>
int with_even_two_d(int two_d, int err, F&& f) {
    auto at = [&](auto D) -> int {
        if constexpr (decltype(D)::value >= MIN) return f(D);
        else return err;
    };
    switch (two_d) {
        case 2: return at(std::integral_constant<int, 2>{});
        case 4: return at(std::integral_constant<int, 4>{});
        case 6: return at(std::integral_constant<int, 6>{});
        case 8: return at(std::integral_constant<int, 8>{});
        case 10: return at(std::integral_constant<int, 10>{});
        case 12: return at(std::integral_constant<int, 12>{});
        case 14: return at(std::integral_constant<int, 14>{});
        case 16: return at(std::integral_constant<int, 16>{});
        case 18: return at(std::integral_constant<int, 18>{});
        default: return err;
    }
}

// The checks of a segmented entry point's leading arguments: 0, or the (negative) position of the offending one in ITS signature -
// B is the first everywhere, N and S sit at pos_n and pos_s.
inline int check_segmentation(int64_t B, int64_t N, int64_t S, int pos_n = 2, int pos_s = 3) {
    if (B < 0) return -1;
    if (N < 0) return -pos_n;
    if (S < 1 || (B > 0 && S > int64_t(0x7fffffff) / B)) return -pos_s;
    return 0;
}

// The checks of the tile table, in two steps because the entry points check their outputs in between.  `pos` is the position of
// num_tiles in the entry point's signature; tile_seg, seg_tile, workspace and workspace_bytes follow it there.
//   the count: in range - one block per tile, or blocks_per_tile of them -, and no tiles without points
inline int check_tile_count(int pos, int64_t N, int64_t tiles, int64_t blocks_per_tile = 1) {
    if (tiles < 0 || tiles > int64_t(0x7fffffff) || (N == 0 && tiles != 0) ||
        (blocks_per_tile > 0 && tiles > int64_t(0x7fffffff) / blocks_per_tile))
        return -pos;
    return 0;
}
//   the table of tiles > 0 tiles: the three pointers, and the workspace's size against `row` values of elem_size bytes per tile
inline int check_tile_table(int pos, int64_t tiles, const void* tile_seg, const void* seg_tile, const void* ws, size_t ws_bytes,
                            size_t row, size_t elem_size) {
    if (const int bad = first_null(pos + 1, {tile_seg, seg_tile, ws})) return bad;
    return ws_bytes < size_t(tiles) * row * elem_size ? -(pos + 4) : 0;
}

}  // namespace
