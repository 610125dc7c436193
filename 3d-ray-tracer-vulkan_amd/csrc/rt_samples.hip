// rt_samples.hip — the resolve of a samples launch (rtamd.h "samples",
// DESIGN.md §4k).
//
// A samples launch traces S consecutive samples of one camera as the S frames
// of a batch launch and leaves their linear colours, one frame after another,
// in the call's workspace.  This kernel folds them into the running sum: per
// channel s = the old sum (or slice 0 when the call starts a new sum, which is
// then never read), then s = s + slice f for f in increasing order, one
// rounded add each, exactly the adds extension bit 4 makes frame by frame.  On
// the call's last chunk it also writes what bit 4's last frame would show:
// fin = s / n, g = sqrt(fin), and g quantised as the render quantises it.  The
// library is built with -ffp-contract=off and `/` and sqrtf are correctly
// rounded, so the bits are the CPU oracle's.
//
// Bandwidth bound: S + 1 float images in (S when the sum starts over), up to
// three images out.  No atomics, no LDS: every element belongs to one lane.
// Two forms:
//   wide   : a lane folds 4 pixels (12 floats) with three 16-byte accesses per
//            image and writes its four RGBA8 pixels with one; every base
//            must lie on the 16-byte grid, so 3 * n_px * 4 bytes must be a
//            multiple of 16 (n_px a multiple of 4) and so must every pointer
//   scalar : a lane folds one pixel with 4-byte accesses; any size (slice f of
//            a frame of 2553 floats starts 12 * f bytes off the grid)
#include "rt_internal.h"
#include "rt_pixel.h"

namespace rtamd {
namespace {

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 div4(float4 a, float d) { return make_float4(a.x / d, a.y / d, a.z / d, a.w / d); }
__device__ __forceinline__ float4 sqrt4(float4 a) { return make_float4(sqrtf(a.x), sqrtf(a.y), sqrtf(a.z), sqrtf(a.w)); }
__device__ __forceinline__ unsigned pack_rgba(float r, float g, float b) {
    return (unsigned)unorm8(r) | (unsigned)unorm8(g) << 8 | (unsigned)unorm8(b) << 16 | 255u << 24;
}

__global__ __launch_bounds__(256) void samples_resolve_wide(SamplesArgs a) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;     // 4 pixels: floats [12 q, 12 q + 12)
    if (q >= a.n_px / 4) return;
    const size_t stride4 = a.n_px / 4 * 3;                       // float4 per image
    const float4* in = reinterpret_cast<const float4*>(a.slices) + 3 * q;
    float4* sum = reinterpret_cast<float4*>(a.sum) + 3 * q;
    float4 s0, s1, s2;
    int f = 0;
    if (a.load_sum) {
        s0 = sum[0]; s1 = sum[1]; s2 = sum[2];
    } else {
        s0 = in[0]; s1 = in[1]; s2 = in[2];
        f = 1;
    }
    for (; f < a.n_slices; ++f) {
        const float4* p = in + (size_t)f * stride4;
        s0 = add4(s0, p[0]); s1 = add4(s1, p[1]); s2 = add4(s2, p[2]);
    }
    sum[0] = s0; sum[1] = s1; sum[2] = s2;
    if (!a.finish) return;
    const float4 g0 = sqrt4(div4(s0, a.divisor)), g1 = sqrt4(div4(s1, a.divisor)), g2 = sqrt4(div4(s2, a.divisor));
    if (a.out_rad) {
        float4* o = reinterpret_cast<float4*>(a.out_rad) + 3 * q;
        o[0] = g0; o[1] = g1; o[2] = g2;
    }
    if (a.out_rgba)      // pixels 4 q .. 4 q + 3: (g0.xyz) (g0.w g1.xy) (g1.zw g2.x) (g2.yzw)
        reinterpret_cast<uint4*>(a.out_rgba)[q] = make_uint4(pack_rgba(g0.x, g0.y, g0.z), pack_rgba(g0.w, g1.x, g1.y),
                                                             pack_rgba(g1.z, g1.w, g2.x), pack_rgba(g2.y, g2.z, g2.w));
}

__global__ __launch_bounds__(256) void samples_resolve_scalar(SamplesArgs a) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;     // one pixel
    if (p >= a.n_px) return;
    const size_t stride = a.n_px * 3;
    const float* in = a.slices + 3 * p;
    float* sum = a.sum + 3 * p;
    float r, g, b;
    int f = 0;
    if (a.load_sum) {
        r = sum[0]; g = sum[1]; b = sum[2];
    } else {
        r = in[0]; g = in[1]; b = in[2];
        f = 1;
    }
    for (; f < a.n_slices; ++f) {
        const float* q = in + (size_t)f * stride;
        r = r + q[0]; g = g + q[1]; b = b + q[2];
    }
    sum[0] = r; sum[1] = g; sum[2] = b;
    if (!a.finish) return;
    const float gr = sqrtf(r / a.divisor), gg = sqrtf(g / a.divisor), gb = sqrtf(b / a.divisor);
    if (a.out_rad) {
        a.out_rad[3 * p + 0] = gr;
        a.out_rad[3 * p + 1] = gg;
        a.out_rad[3 * p + 2] = gb;
    }
    if (a.out_rgba) a.out_rgba[p] = make_uchar4(unorm8(gr), unorm8(gg), unorm8(gb), 255);
}

}  // namespace

hipError_t launch_samples_resolve(const SamplesArgs& r, hipStream_t stream) {
    const uintptr_t bases = (uintptr_t)r.slices | (uintptr_t)r.sum | (uintptr_t)r.out_rgba | (uintptr_t)r.out_rad;
    const bool wide = r.form == 0 && r.n_px % 4 == 0 && (bases & 15u) == 0;
    if (!wide) {
        hipLaunchKernelGGL(samples_resolve_scalar, dim3((unsigned)((r.n_px + 255) / 256)), dim3(256), 0, stream, r);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(samples_resolve_wide, dim3((unsigned)((r.n_px / 4 + 255) / 256)), dim3(256), 0, stream, r);
    return hipGetLastError();
}

}  // namespace rtamd

extern "C" {

size_t rt_samples_workspace_bytes(int width, int height, int frames) {
    if (width < 1 || height < 1 || (int64_t)width * (int64_t)height > (int64_t)1 << 31) return 0;
    if (frames < 1 || frames > rtamd::kMaxBatch) return 0;
    return (size_t)frames * (size_t)width * (size_t)height * 12;
}

}  // extern "C"
