// Does a NARROW stream over-fetch?  Every lane owns `steps` consecutive rows of ROWB bytes (as a lane of the streaming
// log-likelihood kernel owns a time chunk of b or H: 48-B rows) and reads one whole row per step with 16-B loads; the buffer
// (65 536 lanes x steps rows) is walked exactly once and lies far beyond the 256 MiB Infinity Cache.  Under
//     rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR -- ./narrow_fetch
// (a counter pass of its own) the counter per kernel, in KiB, against the bytes printed here gives the factor by which FETCH_SIZE
// has to be scaled for such a stream.  walk_rows<48> is the narrow case, walk_rows<288> the wide one (a row of A) for comparison,
// walk_rows<128> whole lines.
// Build: hipcc --offload-arch=gfx950 -O3 -o narrow_fetch narrow_fetch.hip
#include <hip/hip_runtime.h>
#include <cstdio>

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <int ROWB> __global__ void __launch_bounds__(64) walk_rows(const u32x4* __restrict__ buf, long lanes, int steps, unsigned* sink) {
    constexpr int U = ROWB / 16;
    const long lane = (long)blockIdx.x * 64 + threadIdx.x;
    if (lane >= lanes) return;
    const u32x4* p = buf + lane * (long)steps * U;
    unsigned acc = 0;
    for (int j = 0; j < steps; ++j, p += U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u32x4 v = __builtin_nontemporal_load(p + u);
            acc += v.x ^ v.y ^ v.z ^ v.w;
        }
    }
    if (acc == 0x12345678u) *sink = acc;
}

template <int ROWB> static void run(const u32x4* buf, long lanes, int steps, unsigned* sink) {
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, 0);
    hipLaunchKernelGGL(walk_rows<ROWB>, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, 0, buf, lanes, steps, sink);
    (void)hipEventRecord(e1, 0);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    const double bytes = (double)lanes * steps * ROWB;
    printf("walk_rows<%d>: lanes %ld steps %d  bytes %.0f (%.1f KiB, %.3f GB)  %.3f ms  %.0f GB/s\n", ROWB, lanes, steps, bytes,
           bytes / 1024.0, bytes / 1e9, ms, bytes / ms / 1e6);
}

int main() {
    const long lanes = 65536;
    const int steps = 157;
    const size_t bytes = (size_t)lanes * steps * 288;          // 2.96 GB: the widest case; the narrow one walks its first 494 MB
    u32x4* buf;
    unsigned* sink;
    if (hipMalloc(&buf, bytes) != hipSuccess || hipMalloc(&sink, 4) != hipSuccess) return 1;
    (void)hipMemset(buf, 1, bytes);
    (void)hipDeviceSynchronize();
    run<288>(buf, lanes, steps, sink);      // (first, so that the narrow walk below finds nothing of its range in any cache)
    run<128>(buf, lanes, steps, sink);
    run<48>(buf, lanes, steps, sink);
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
