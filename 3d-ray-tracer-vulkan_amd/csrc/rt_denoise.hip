// rt_denoise.hip — the edge-avoiding a-trous denoiser of 1-sample frames
// (rtamd.h "denoise").
//
// A 5x5 B3-spline wavelet filter, step 2^i in pass i, whose tap weights fall
// with the angle between the first-hit normals, with the tap's distance from
// the centre pixel's tangent plane and with the luminance difference.  The
// guides are the rt_hit records rt_render_hits_device writes.  All arithmetic
// is IEEE binary32 in the order DESIGN.md §4g writes it (the library is built
// with -ffp-contract=off, `/` and sqrtf are correctly rounded, fmaxf drops a
// NaN operand), so tests/denoise_ref.py restates it bit for bit.
//
// Pass 0 reads the render's 12-byte radiance (g, squared on the fly); the
// passes between ping-pong float4(c.rgb, luminance) through the two halves of
// the caller's workspace, so a pixel's luminance is computed once, by its
// writer; the last pass writes sqrt(c) and the RGBA8 pixels.
//
// Two forms of a pass:
//   plain : one lane per pixel, a wave on 64 consecutive pixels of a row; the
//           25 taps are read from global memory (contiguous across the wave at
//           every step size).
//   tiled : a 256-thread workgroup filters 32 x 8 pixels of ONE residue class
//           (x mod step, y mod step), whose taps are neighbours in that class:
//           the 36 x 12 halo tile is staged once in LDS as three 16-byte
//           planes (20,736 B), and the taps are ds_read_b128 of consecutive
//           16-byte slots (conflict-free; a 48-byte record's 12-dword stride
//           would touch 16 of the 64 banks).
// Which form a step size gets by default was measured (kTiledByStep below).
#include "rt_internal.h"

#include <cmath>

namespace rtamd {
namespace {

struct PassArgs {
    int W, H, step;
    const float*  in_rad;     // pass 0: the render's radiance, 3 floats per pixel (else null)
    const float4* in_c;       // later passes: (c.rgb, luminance)
    const float4* hits;       // rt_hit as 2 float4: (t, tri, n.xy), (n.z, pos.xyz)
    float4*       out_c;      // every pass but the last (else null)
    uchar4*       out_rgba;   // last pass, nullable
    float*        out_rad;    // last pass, nullable
    float         kd;         // sigma_depth
    float         isc;        // step / sigma_color
    int           npow;       // normal_power_log2
};

__device__ __forceinline__ float lum_of(float r, float g, float b) {
    return (0.2126f * r + 0.7152f * g) + 0.0722f * b;
}

__device__ __forceinline__ uint8_t unorm8(float c) {   // the render's store (rt_trace.hip)
    return c > 0.0f ? (c < 1.0f ? (uint8_t)__builtin_rintf(c * 255.0f) : (uint8_t)255) : (uint8_t)0;
}

// (c.rgb, luminance) of pixel q of this pass's input
__device__ __forceinline__ float4 load_c(const PassArgs& a, size_t q) {
    if (a.in_rad) {
        const float gr = a.in_rad[3 * q + 0], gg = a.in_rad[3 * q + 1], gb = a.in_rad[3 * q + 2];
        const float r = gr * gr, g = gg * gg, b = gb * gb;
        return make_float4(r, g, b, lum_of(r, g, b));
    }
    return a.in_c[q];
}

__device__ __forceinline__ void store_px(const PassArgs& a, size_t p, float r, float g, float b) {
    if (a.out_c) {
        a.out_c[p] = make_float4(r, g, b, lum_of(r, g, b));
        return;
    }
    const float sr = sqrtf(r), sg = sqrtf(g), sb = sqrtf(b);
    if (a.out_rgba) a.out_rgba[p] = make_uchar4(unorm8(sr), unorm8(sg), unorm8(sb), 255);
    if (a.out_rad) {
        a.out_rad[3 * p + 0] = sr;
        a.out_rad[3 * p + 1] = sg;
        a.out_rad[3 * p + 2] = sb;
    }
}

// The centre pixel's side of a tap weight, and the running sums.
struct Centre {
    float nx, ny, nz, px, py, pz, lum, kz;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, ws = 0.0f;
};

// One tap: hh = h[|dx|] * h[|dy|]; q0 / q1 the tap's hit record, cq its (c.rgb, luminance).
// A tap outside the frame or without a hit (tri < 0) leaves the sums as they are.
__device__ __forceinline__ void tap(Centre& c, const PassArgs& a, float hh, float4 q0, float4 q1, float4 cq,
                                    bool inside) {
    float nd = __builtin_fmaxf(0.0f, (c.nx * q0.z + c.ny * q0.w) + c.nz * q1.x);
    for (int k = 0; k < a.npow; ++k) nd = nd * nd;
    const float ex = q1.y - c.px, ey = q1.z - c.py, ez = q1.w - c.pz;
    const float d = __builtin_fabsf((c.nx * ex + c.ny * ey) + c.nz * ez);
    const float x = d * c.kz;
    const float y = __builtin_fabsf(c.lum - cq.w) * a.isc;
    const float w = (hh * nd) / ((1.0f + x * x) * (1.0f + y * y));
    const bool take = inside && __float_as_int(q0.y) >= 0;
    c.sr = take ? c.sr + w * cq.x : c.sr;
    c.sg = take ? c.sg + w * cq.y : c.sg;
    c.sb = take ? c.sb + w * cq.z : c.sb;
    c.ws = take ? c.ws + w : c.ws;
}

__device__ __forceinline__ Centre centre_of(const PassArgs& a, float4 p0, float4 p1, float4 cp) {
    Centre c;
    c.nx = p0.z; c.ny = p0.w; c.nz = p1.x;
    c.px = p1.y; c.py = p1.z; c.pz = p1.w;
    c.lum = cp.w;
    c.kz = 1.0f / (a.kd * p0.x);
    return c;
}

__device__ __forceinline__ void finish(const PassArgs& a, size_t p, const Centre& c, float4 cp) {
    const bool ok = c.ws > 0.0f;                   // NaN or zero: the pixel passes through
    store_px(a, p, ok ? c.sr / c.ws : cp.x, ok ? c.sg / c.ws : cp.y, ok ? c.sb / c.ws : cp.z);
}

// the B3 spline h = [3/8, 1/4, 1/16] by |offset|; the products of two are exact
constexpr float b3(int o) { return o == 0 ? 0.375f : ((o == 1 || o == -1) ? 0.25f : 0.0625f); }

// ---- plain: one lane per pixel, 64 x 4 pixels per workgroup, taps from global memory
__global__ __launch_bounds__(256, 4) void denoise_plain(PassArgs a, int tiles_x) {
    const int bx = (int)(blockIdx.x % (unsigned)tiles_x), by = (int)(blockIdx.x / (unsigned)tiles_x);
    const int x = bx * 64 + (int)(threadIdx.x & 63u), y = by * 4 + (int)(threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * (size_t)a.W + (size_t)x;
    const float4 p0 = a.hits[2 * p], p1 = a.hits[2 * p + 1];
    const float4 cp = load_c(a, p);
    if (__float_as_int(p0.y) < 0) {                // sky / invalid: pass through
        store_px(a, p, cp.x, cp.y, cp.z);
        return;
    }
    Centre c = centre_of(a, p0, p1, cp);
    // a row of taps at a time: its 15 loads are in flight together, the next row's wait (registers)
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * a.step, qy = y + dy * a.step;
            const bool inside = qx >= 0 && qx < a.W && qy >= 0 && qy < a.H;
            const size_t q = inside ? (size_t)qy * (size_t)a.W + (size_t)qx : p;   // a safe address either way
            tap(c, a, b3(dx) * b3(dy), a.hits[2 * q], a.hits[2 * q + 1], load_c(a, q), inside);
        }
    }
    finish(a, p, c, cp);
}

// ---- tiled: 32 x 8 pixels of one residue class per workgroup, the halo tile in LDS
constexpr int kTileX = 32, kTileY = 8, kHaloX = kTileX + 4, kHaloY = kTileY + 4;

__global__ __launch_bounds__(256, 4) void denoise_tiled(PassArgs a, int tiles_x) {
    __shared__ float4 s_c[kHaloX * kHaloY], s_h0[kHaloX * kHaloY], s_h1[kHaloX * kHaloY];
    const unsigned s = (unsigned)a.step;
    unsigned id = blockIdx.x;                      // ((by * tiles_x + bx) * s + ry) * s + rx
    const int rx = (int)(id % s); id /= s;
    const int ry = (int)(id % s); id /= s;
    const int bx = (int)(id % (unsigned)tiles_x), by = (int)(id / (unsigned)tiles_x);
    // class coordinates (cx, cy) are pixel (rx + step * cx, ry + step * cy); 64-bit: step * cx may pass 2^31
    const long long W = a.W, H = a.H, st = a.step;
    if (rx + st * (bx * kTileX) >= W || ry + st * (by * kTileY) >= H) return;   // this class ends before the tile
    for (int e = (int)threadIdx.x; e < kHaloX * kHaloY; e += 256) {
        const int i = e % kHaloX, j = e / kHaloX;
        const long long x = rx + st * (bx * kTileX - 2 + i), y = ry + st * (by * kTileY - 2 + j);
        float4 cq = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q0 = make_float4(0.0f, __int_as_float(-1), 0.0f, 0.0f),
               q1 = cq;                            // outside the frame: a tap without a hit
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const size_t q = (size_t)y * (size_t)W + (size_t)x;
            cq = load_c(a, q);
            q0 = a.hits[2 * q];
            q1 = a.hits[2 * q + 1];
        }
        s_c[e] = cq;
        s_h0[e] = q0;
        s_h1[e] = q1;
    }
    __syncthreads();
    const int i = (int)(threadIdx.x & 31u), j = (int)(threadIdx.x >> 5);
    const long long x = rx + st * (bx * kTileX + i), y = ry + st * (by * kTileY + j);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    const int e0 = (j + 2) * kHaloX + (i + 2);
    const float4 p0 = s_h0[e0], p1 = s_h1[e0], cp = s_c[e0];
    if (__float_as_int(p0.y) < 0) {
        store_px(a, p, cp.x, cp.y, cp.z);
        return;
    }
    Centre c = centre_of(a, p0, p1, cp);
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int e = e0 + dy * kHaloX + dx;
            tap(c, a, b3(dx) * b3(dy), s_h0[e], s_h1[e], s_c[e], true);
        }
    }
    finish(a, p, c, cp);
}

// The form each step size 2^i takes by default: the faster one of
// tools/denoise_bench.py's per-pass times on config 3 at 1920x1080
// (profiles/denoise): tiled 0.075 / 0.079 / 0.091 ms against
// plain 0.092 / 0.094 / 0.100 at steps 1 / 2 / 4, tiled 0.134 against plain
// 0.096 at step 8 (a residue class's tile rows lie 8 pixels apart, so its
// staging loads use 16 bytes of every 128 fetched).  Steps 16 and 32 keep the
// plain form; their times are in DESIGN.md §4g.
constexpr bool kTiledByStep[6] = {true, true, true, false, false, false};

}  // namespace

hipError_t launch_denoise(const DenoiseArgs& d, hipStream_t stream) {
    const size_t px = (size_t)d.width * (size_t)d.height;
    float4* half[2] = {d.workspace, d.workspace + px};
    for (int i = 0; i < d.iterations; ++i) {
        if (d.only_pass >= 0 && i != d.only_pass) continue;
        PassArgs a;
        a.W = d.width; a.H = d.height; a.step = 1 << i;
        a.in_rad = i == 0 ? d.radiance : nullptr;
        a.in_c = i == 0 ? nullptr : half[(i - 1) & 1];
        a.hits = d.hits;
        const bool last = i == d.iterations - 1;
        a.out_c = last ? nullptr : half[i & 1];
        a.out_rgba = last ? d.out_rgba : nullptr;
        a.out_rad = last ? d.out_rad : nullptr;
        a.kd = d.sigma_depth;
        a.isc = d.inv_sigma_color * (float)a.step;
        a.npow = d.normal_power_log2;
        // tiles of a residue class: ceil(ceil(W / step) / 32) x ceil(ceil(H / step) / 8), for step^2 classes
        const size_t cw = ((size_t)d.width + a.step - 1) / a.step, ch = ((size_t)d.height + a.step - 1) / a.step;
        const size_t ttx = (cw + kTileX - 1) / kTileX, tty = (ch + kTileY - 1) / kTileY;
        const size_t tiled_blocks = ttx * tty * (size_t)a.step * (size_t)a.step;
        bool tiled = d.form == 2 || (d.form == 0 && kTiledByStep[i]);
        if (tiled_blocks > 0x7FFFFFFFull) tiled = false;             // past a 1-D grid: the plain form
        if (tiled) {
            hipLaunchKernelGGL(denoise_tiled, dim3((unsigned)tiled_blocks), dim3(256), 0, stream, a, (int)ttx);
        } else {
            const size_t ptx = ((size_t)d.width + 63) / 64, pty = ((size_t)d.height + 3) / 4;
            hipLaunchKernelGGL(denoise_plain, dim3((unsigned)(ptx * pty)), dim3(256), 0, stream, a, (int)ptx);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace rtamd

extern "C" {

void rt_denoise_default_params(rt_denoise_params* out) {
    if (!out) return;
    out->iterations = 4;
    out->normal_power_log2 = 7;
    out->sigma_depth = 0.005f;
    out->sigma_color = 0.5f;
}

size_t rt_denoise_workspace_bytes(int width, int height) {
    if (width < 1 || height < 1 || (int64_t)width * (int64_t)height > (int64_t)1 << 31) return 0;
    return (size_t)2 * (size_t)width * (size_t)height * 16;
}

}  // extern "C"
