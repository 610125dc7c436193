// rt_rng.h — the shader's random numbers (compute_dynamic_ray.comp:52-70), written once for the frame
// kernels (rt_trace.hip) and for the kernel that tables a pixel's scatter draws (rt_rngtable.hip;
// DESIGN.md §4o): both compile these very functions, so their bits agree by construction.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace rtamd {

namespace {

constexpr int kMaxRejectTriples = 1 << 16; // bound on the rejection loop (:65-68), see DESIGN.md

struct V3 { float x, y, z; };

__device__ __forceinline__ float vdot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// pcg (compute_dynamic_ray.comp:52-56) and randomFloat (:58-61).
__device__ __forceinline__ uint32_t pcg(uint32_t v) {
    const uint32_t s = v * 747796405u + 2891336453u;
    const uint32_t w = ((s >> ((s >> 28u) + 4u)) ^ s) * 277803737u;
    return (w >> 22u) ^ w;
}
__device__ __forceinline__ float rnd(uint32_t& seed) {
    seed = pcg(seed);
    return (float)seed / 4294967296.0f;   // float(0xFFFFFFFFu) rounds to 2^32
}

// randomVec3InUnitSphere (:63-70): three draws are made and discarded, then
// rejection sampling of 2*rand3-1 until dot(p,p) < 1.
__device__ __forceinline__ V3 rnd_in_sphere(uint32_t& seed) {
    seed = pcg(pcg(pcg(seed)));
    for (int it = 0; it < kMaxRejectTriples; ++it) {
        const float a = rnd(seed);
        const float b = rnd(seed);
        const float c = rnd(seed);
        const V3 p = {a * 2.0f - 1.0f, b * 2.0f - 1.0f, c * 2.0f - 1.0f};
        if (vdot(p, p) < 1.0f) return p;
    }
    return {0.0f, 0.0f, 0.0f};
}

}  // namespace

}  // namespace rtamd
