// rt_rngtable.hip — the table of a pixel's scatter draws (option rng_table).
//
// A path's random numbers do not depend on the scene or the camera: the seed starts as y * width + x, the
// primary ray takes two draws, and every bounce that scatters takes exactly one rnd_in_sphere, whatever the
// material (a path that does not scatter ends).  So the point a path uses at bounce b and the seed it leaves
// behind are a function of the pixel and b alone, the same in every frame of a resolution.  This kernel
// computes them once, one lane per pixel, with the frame kernels' own pcg / rnd / rnd_in_sphere (rt_rng.h),
// the kMaxRejectTriples give-up included.
#include "rt_internal.h"
#include "rt_rng.h"

namespace rtamd {

namespace {

__global__ __launch_bounds__(256) void fill_rng_table(float4* __restrict__ table, unsigned n_px, int k_planes) {
    const unsigned s0 = blockIdx.x * 256u + threadIdx.x;
    if (s0 >= n_px) return;
    uint32_t seed = s0;
    (void)rnd(seed);                     // the primary ray's jitter pair
    (void)rnd(seed);
    for (int k = 0; k < k_planes; ++k) {
        const V3 p = rnd_in_sphere(seed);
        table[(size_t)k * n_px + s0] = make_float4(p.x, p.y, p.z, __uint_as_float(seed));
    }
}

}  // namespace

hipError_t launch_rng_table(float4* table, int width, int height, int k, hipStream_t stream) {
    if (!table || rng_table_bytes(width, height, k) == 0) return hipErrorInvalidValue;
    const unsigned n_px = (unsigned)((uint64_t)width * (uint64_t)height);   // <= 2^27: rng_table_bytes
    hipLaunchKernelGGL(fill_rng_table, dim3((n_px + 255u) / 256u), dim3(256), 0, stream, table, n_px, k);
    return hipGetLastError();
}

}  // namespace rtamd
