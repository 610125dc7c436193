// rt_denoise_history.hip — the history-adaptive a-trous filter that follows
// temporal accumulation (rtamd.h "denoise", rt_denoise_history_device;
// DESIGN.md §4i).
//
// rt_denoise.hip's 5x5 B3-spline wavelet filter with the history's sample count
// n in three places: a pixel with n samples is filtered in the first
// max(0, iterations - floor(log2 n)) passes only and passes through the rest,
// its colour tolerance tightens by n, and a tap counts n_q times.  A pixel
// without a hit or with n < 1 (or NaN) is never filtered and never a tap.  All
// arithmetic is IEEE binary32 in the order DESIGN.md §4i writes it (the library
// is built with -ffp-contract=off, `/` and sqrtf are correctly rounded, fmaxf
// drops a NaN operand), so tests/denoise_history_ref.py restates it bit for bit.
//
// Every pass reads and every pass but the last writes the history's own record
// format, float4(c.rgb, n): pass 0 reads the caller's history, the passes
// between ping-pong through the two halves of the workspace, the last pass
// writes sqrt(c) and the RGBA8 pixels.  The luminance of a record is recomputed
// where it is needed (three multiplications and two additions of the stored
// colour: the same bits wherever it is done).
//
// Two forms of a pass, as in rt_denoise.hip:
//   plain : one lane per pixel, a wave on 64 consecutive pixels of a row; the
//           25 taps are read from global memory, their luminance computed per
//           tap.
//   tiled : a 256-thread workgroup filters 32 x 8 pixels of ONE residue class
//           (x mod step, y mod step); the 36 x 12 halo tile is staged once in
//           LDS as three 16-byte planes and a 4-byte plane of luminances
//           (22,464 B), each luminance computed once, by the lane that stages
//           the record.  A lane whose pixel passes through still stages its
//           share and leaves only after the barrier.
// Which form a step size gets by default was measured (kTiledByStep below).
#include "rt_internal.h"

#include <cmath>

namespace rtamd {
namespace {

struct PassArgs {
    int W, H, step;
    const float4* in;         // (c.rgb, n): pass 0 the history, later passes the workspace
    const float4* hits;       // rt_hit as 2 float4: (t, tri, n.xy), (n.z, pos.xyz)
    float4*       out_c;      // every pass but the last (else null)
    uchar4*       out_rgba;   // last pass, nullable
    float*        out_rad;    // last pass, nullable
    float         kd;         // sigma_depth
    float         isc;        // step / sigma_color
    int           npow;       // normal_power_log2
    int           left;       // iterations - pass index: a pixel is filtered while floor(log2 n) < left
};

__device__ __forceinline__ float lum_of(float r, float g, float b) {
    return (0.2126f * r + 0.7152f * g) + 0.0722f * b;
}

__device__ __forceinline__ uint8_t unorm8(float c) {   // the render's store (rt_trace.hip)
    return c > 0.0f ? (c < 1.0f ? (uint8_t)__builtin_rintf(c * 255.0f) : (uint8_t)255) : (uint8_t)0;
}

// a record that is filtered at all and serves as a tap: a hit with n >= 1 (a NaN n fails)
__device__ __forceinline__ bool live(float tri_bits, float n) { return __float_as_int(tri_bits) >= 0 && n >= 1.0f; }

// a live pixel is filtered in this pass while floor(log2 n), its unbiased exponent, is below `left`
__device__ __forceinline__ bool filtered(const PassArgs& a, float tri_bits, float n) {
    const int e = ((__float_as_int(n) >> 23) & 0xFF) - 127;
    return live(tri_bits, n) && e < a.left;
}

__device__ __forceinline__ void store_px(const PassArgs& a, size_t p, float r, float g, float b, float n) {
    if (a.out_c) {
        a.out_c[p] = make_float4(r, g, b, n);
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
    float nx, ny, nz, px, py, pz, lum, kz, isc;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, ws = 0.0f;
};

// One tap: hh = h[|dx|] * h[|dy|]; q0 / q1 the tap's hit record, cq its (c.rgb, n), lq its luminance.
// A tap outside the frame or not live leaves the sums as they are.
__device__ __forceinline__ void tap(Centre& c, const PassArgs& a, float hh, float4 q0, float4 q1, float4 cq, float lq,
                                    bool inside) {
    float nd = __builtin_fmaxf(0.0f, (c.nx * q0.z + c.ny * q0.w) + c.nz * q1.x);
    for (int k = 0; k < a.npow; ++k) nd = nd * nd;
    const float ex = q1.y - c.px, ey = q1.z - c.py, ez = q1.w - c.pz;
    const float d = __builtin_fabsf((c.nx * ex + c.ny * ey) + c.nz * ez);
    const float x = d * c.kz;
    const float y = __builtin_fabsf(c.lum - lq) * c.isc;
    const float w = ((hh * nd) * cq.w) / ((1.0f + x * x) * (1.0f + y * y));
    const bool take = inside && live(q0.y, cq.w);
    c.sr = take ? c.sr + w * cq.x : c.sr;
    c.sg = take ? c.sg + w * cq.y : c.sg;
    c.sb = take ? c.sb + w * cq.z : c.sb;
    c.ws = take ? c.ws + w : c.ws;
}

__device__ __forceinline__ Centre centre_of(const PassArgs& a, float4 p0, float4 p1, float4 cp, float lum) {
    Centre c;
    c.nx = p0.z; c.ny = p0.w; c.nz = p1.x;
    c.px = p1.y; c.py = p1.z; c.pz = p1.w;
    c.lum = lum;
    c.kz = 1.0f / (a.kd * p0.x);
    c.isc = a.isc * cp.w;                          // (isc * step) * n_p
    return c;
}

__device__ __forceinline__ void finish(const PassArgs& a, size_t p, const Centre& c, float4 cp) {
    const bool ok = c.ws > 0.0f;                   // NaN or zero: the pixel passes through
    store_px(a, p, ok ? c.sr / c.ws : cp.x, ok ? c.sg / c.ws : cp.y, ok ? c.sb / c.ws : cp.z, cp.w);
}

// the B3 spline h = [3/8, 1/4, 1/16] by |offset|; the products of two are exact
constexpr float b3(int o) { return o == 0 ? 0.375f : ((o == 1 || o == -1) ? 0.25f : 0.0625f); }

// ---- plain: one lane per pixel, 64 x 4 pixels per workgroup, taps from global memory
__global__ __launch_bounds__(256, 4) void denoise_history_plain(PassArgs a, int tiles_x) {
    const int bx = (int)(blockIdx.x % (unsigned)tiles_x), by = (int)(blockIdx.x / (unsigned)tiles_x);
    const int x = bx * 64 + (int)(threadIdx.x & 63u), y = by * 4 + (int)(threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * (size_t)a.W + (size_t)x;
    const float4 p0 = a.hits[2 * p];
    const float4 cp = a.in[p];
    if (!filtered(a, p0.y, cp.w)) {                // sky, no sample, or history long enough: pass through
        store_px(a, p, cp.x, cp.y, cp.z, cp.w);
        return;
    }
    Centre c = centre_of(a, p0, a.hits[2 * p + 1], cp, lum_of(cp.x, cp.y, cp.z));
    // a row of taps at a time: its 15 loads are in flight together, the next row's wait (registers)
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * a.step, qy = y + dy * a.step;
            const bool inside = qx >= 0 && qx < a.W && qy >= 0 && qy < a.H;
            const size_t q = inside ? (size_t)qy * (size_t)a.W + (size_t)qx : p;   // a safe address either way
            const float4 cq = a.in[q];
            tap(c, a, b3(dx) * b3(dy), a.hits[2 * q], a.hits[2 * q + 1], cq, lum_of(cq.x, cq.y, cq.z), inside);
        }
    }
    finish(a, p, c, cp);
}

// ---- tiled: 32 x 8 pixels of one residue class per workgroup, the halo tile in LDS
constexpr int kTileX = 32, kTileY = 8, kHaloX = kTileX + 4, kHaloY = kTileY + 4;

__global__ __launch_bounds__(256, 4) void denoise_history_tiled(PassArgs a, int tiles_x) {
    __shared__ float4 s_c[kHaloX * kHaloY], s_h0[kHaloX * kHaloY], s_h1[kHaloX * kHaloY];
    __shared__ float s_lum[kHaloX * kHaloY];
    const unsigned s = (unsigned)a.step;
    unsigned id = blockIdx.x;                      // ((by * tiles_x + bx) * s + ry) * s + rx
    const int rx = (int)(id % s); id /= s;
    const int ry = (int)(id % s); id /= s;
    const int bx = (int)(id % (unsigned)tiles_x), by = (int)(id / (unsigned)tiles_x);
    // class coordinates (cx, cy) are pixel (rx + step * cx, ry + step * cy); 64-bit: step * cx may pass 2^31
    const long long W = a.W, H = a.H, st = a.step;
    // this class ends before the tile: the whole workgroup leaves, before any barrier
    if (rx + st * (bx * kTileX) >= W || ry + st * (by * kTileY) >= H) return;
    for (int e = (int)threadIdx.x; e < kHaloX * kHaloY; e += 256) {
        const int i = e % kHaloX, j = e / kHaloX;
        const long long x = rx + st * (bx * kTileX - 2 + i), y = ry + st * (by * kTileY - 2 + j);
        float4 cq = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q0 = make_float4(0.0f, __int_as_float(-1), 0.0f, 0.0f),
               q1 = cq;                            // outside the frame: a tap without a hit and without a sample
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const size_t q = (size_t)y * (size_t)W + (size_t)x;
            cq = a.in[q];
            q0 = a.hits[2 * q];
            q1 = a.hits[2 * q + 1];
        }
        s_c[e] = cq;
        s_h0[e] = q0;
        s_h1[e] = q1;
        s_lum[e] = lum_of(cq.x, cq.y, cq.z);
    }
    __syncthreads();                               // every lane of the workgroup arrives: no lane has left yet
    const int i = (int)(threadIdx.x & 31u), j = (int)(threadIdx.x >> 5);
    const long long x = rx + st * (bx * kTileX + i), y = ry + st * (by * kTileY + j);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    const int e0 = (j + 2) * kHaloX + (i + 2);
    const float4 p0 = s_h0[e0], cp = s_c[e0];
    if (!filtered(a, p0.y, cp.w)) {
        store_px(a, p, cp.x, cp.y, cp.z, cp.w);
        return;
    }
    Centre c = centre_of(a, p0, s_h1[e0], cp, s_lum[e0]);
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int e = e0 + dy * kHaloX + dx;
            tap(c, a, b3(dx) * b3(dy), s_h0[e], s_h1[e], s_c[e], s_lum[e], true);
        }
    }
    finish(a, p, c, cp);
}

// The form each step size 2^i takes by default, from tools/adaptive_bench.py's
// per-pass times on config 3 at 1920x1080 (profiles/adaptive).
// With one sample everywhere the passes cost what rt_denoise.hip's cost and
// the same forms win: tiled 0.070 / 0.076 / 0.088 ms against plain 0.089 /
// 0.094 / 0.100 at steps 1 / 2 / 4, plain 0.096 against tiled 0.134 at step 8.
// After 8 frames only pass 0 still filters every hit pixel.  The later passes
// mostly pass through, and there the plain form wins by far: a wave whose 64
// pixels all pass through leaves after two loads and a store each, while a
// tile stages its halo whatever its pixels do.  Plain 0.019 against tiled
// 0.046 / 0.074 / 0.124 at steps 2 / 4 / 8 with a static camera, 0.035 / 0.034
// / 0.032 against 0.053 / 0.081 / 0.134 orbiting 1 degree per frame.  The long
// history is the state a sequence spends its time in, so steps 2 and 4 take
// the plain form: the whole filter takes 0.03 ms more on a sequence's first
// frame and 0.06 to 0.08 ms less on every frame from the eighth on.
constexpr bool kTiledByStep[6] = {true, false, false, false, false, false};

}  // namespace

hipError_t launch_denoise_history(const DenoiseArgs& d, const float4* hist, hipStream_t stream) {
    const size_t px = (size_t)d.width * (size_t)d.height;
    float4* half[2] = {d.workspace, d.workspace + px};
    for (int i = 0; i < d.iterations; ++i) {
        if (d.only_pass >= 0 && i != d.only_pass) continue;
        PassArgs a;
        a.W = d.width; a.H = d.height; a.step = 1 << i;
        a.in = i == 0 ? hist : half[(i - 1) & 1];
        a.hits = d.hits;
        const bool last = i == d.iterations - 1;
        a.out_c = last ? nullptr : half[i & 1];
        a.out_rgba = last ? d.out_rgba : nullptr;
        a.out_rad = last ? d.out_rad : nullptr;
        a.kd = d.sigma_depth;
        a.isc = d.inv_sigma_color * (float)a.step;
        a.npow = d.normal_power_log2;
        a.left = d.iterations - i;
        // tiles of a residue class: ceil(ceil(W / step) / 32) x ceil(ceil(H / step) / 8), for step^2 classes
        const size_t cw = ((size_t)d.width + a.step - 1) / a.step, ch = ((size_t)d.height + a.step - 1) / a.step;
        const size_t ttx = (cw + kTileX - 1) / kTileX, tty = (ch + kTileY - 1) / kTileY;
        const size_t tiled_blocks = ttx * tty * (size_t)a.step * (size_t)a.step;
        bool tiled = d.form == 2 || (d.form == 0 && kTiledByStep[i]);
        if (tiled_blocks > 0x7FFFFFFFull) tiled = false;             // past a 1-D grid: the plain form
        if (tiled) {
            hipLaunchKernelGGL(denoise_history_tiled, dim3((unsigned)tiled_blocks), dim3(256), 0, stream, a, (int)ttx);
        } else {
            const size_t ptx = ((size_t)d.width + 63) / 64, pty = ((size_t)d.height + 3) / 4;
            hipLaunchKernelGGL(denoise_history_plain, dim3((unsigned)(ptx * pty)), dim3(256), 0, stream, a, (int)ptx);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace rtamd
