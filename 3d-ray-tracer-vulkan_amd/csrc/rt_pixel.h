// rt_pixel.h — the per-pixel device helpers every kernel file shares: the
// RGBA8 quantisation, the luminance, a dot product in the order the parity
// documents write it, the filters' tap kernels and the display store.  Device
// code only; each function has this one definition.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rtamd {

// VkFormat R8G8B8A8_UNORM store: clamp to [0,1], round to nearest even.
__device__ __forceinline__ uint8_t unorm8(float c) {
    return c > 0.0f ? (c < 1.0f ? (uint8_t)__builtin_rintf(c * 255.0f) : (uint8_t)255) : (uint8_t)0;
}

__device__ __forceinline__ float lum_of(float r, float g, float b) {
    return (0.2126f * r + 0.7152f * g) + 0.0722f * b;
}

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

// the 3x3 window's binomial B = [1/2, 1/4] and the B3 spline h = [3/8, 1/4, 1/16], by |offset|;
// the products of two are exact
constexpr float b2(int o) { return o == 0 ? 0.5f : 0.25f; }
constexpr float b3(int o) { return o == 0 ? 0.375f : ((o == 1 || o == -1) ? 0.25f : 0.0625f); }

// What a frame shows of the linear colour (r, g, b) of pixel p: g = sqrt(c) as
// 3 floats and quantised as the render quantises it.  Either output may be null.
__device__ __forceinline__ void store_display(uchar4* out_rgba, float* out_rad, size_t p, float r, float g, float b) {
    const float sr = sqrtf(r), sg = sqrtf(g), sb = sqrtf(b);
    if (out_rgba) out_rgba[p] = make_uchar4(unorm8(sr), unorm8(sg), unorm8(sb), 255);
    if (out_rad) {
        out_rad[3 * p + 0] = sr;
        out_rad[3 * p + 1] = sg;
        out_rad[3 * p + 2] = sb;
    }
}

}  // namespace rtamd
