// What the tile-parallel SVGP data terms (mf_lik.hip: the single-latent and the multi-latent pair; mf_lik_factor.hip: the factor-
// analysis pair) share: the packed accumulator row a tile of pass 1 leaves in the workspace - the lower triangle of g_cov, g_mean and
// sum ve - pass 2, which adds a segment's rows in ascending tile order, and the launch helper.
#pragma once

#include "mf_lik_math.hpp"

namespace {

// entry e of a packed lower triangle is (i, j <= i)
__device__ __forceinline__ void tri_decode(int e, int& i, int& j) {
    i = 0;
    while ((i + 1) * (i + 2) / 2 <= e) ++i;
    j = e - i * (i + 1) / 2;
}

// the accumulator has the triangle, the vector and one scalar per row of LDS values beyond the first two
constexpr int seg_entries(int d2, int rows) { return d2 * (d2 + 1) / 2 + d2 + rows - 2; }

// the workspace row of a tile: the triangle of g_cov, g_mean, sum ve
constexpr size_t expect_row(int two_d) { return size_t(seg_entries(two_d, 3)); }

//   pass 2, one block per (series, segment), a lane per entry: the segment's rows are added in ascending tile order, the outputs
//            are written and the triangle mirrored.  An empty segment writes zeros.
template <typename T, int D2>
__global__ void __launch_bounds__(256) sparse_expect_reduce_kernel(long num_tiles, const long long* __restrict__ seg_tile,
                                                                   const T* __restrict__ ws, T* __restrict__ ve_sum,
                                                                   T* __restrict__ g_mean, T* __restrict__ g_cov) {
    constexpr int TRI = D2 * (D2 + 1) / 2, E = seg_entries(D2, 3);
    const long bs = blockIdx.x;
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
        if (e < TRI) {
            int i, c;
            tri_decode(e, i, c);
            g_cov[bs * (D2 * D2) + i * D2 + c] = acc;
            g_cov[bs * (D2 * D2) + c * D2 + i] = acc;
        } else if (e < E - 1) {
            g_mean[bs * D2 + (e - TRI)] = acc;
        } else {
            ve_sum[bs] = acc;
        }
    }
}

// one launch; the arguments are converted to the kernel's parameter types (NULL to a typed pointer, int64_t to long or int)
template <typename... Params, typename... Args>
int launch(void (*kernel)(Params...), int64_t grid, unsigned block, void* stream, const Args&... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(block), 0, static_cast<hipStream_t>(stream), static_cast<Params>(args)...);
    return hipGetLastError() == hipSuccess ? 0 : -1000;
}

}  // namespace
