// rt_variance.hip — the variance-guided a-trous filter and the temporal
// accumulation that feeds it luminance moments (rtamd.h "variance",
// rt_temporal_moments_device and rt_denoise_variance_device).
//
// Three kernels beside the ones they are modelled on, which stay as they are:
//
//   temporal_moments : rt_temporal.hip's kernel with a second history buffer,
//       (m1, m2) = the accumulated means of the samples' luminance and of its
//       square, gathered through the same taps with the same weights.  The
//       colour's operations are rt_temporal.hip's in the same order: the same
//       history, radiance and RGBA8 bits.
//   variance_estimate : one lane per pixel writes the filter's first record
//       (c.rgb, v), v = the variance of the pixel's mean: the temporal one,
//       max(0, m2 - m1^2) / max(n - 1, 1), where the history has min_history
//       samples, else the larger of it and a 7x7 spatial estimate weighted by
//       the guides.  v = -1 marks a pixel that is never filtered and never a
//       tap (no hit, or n < 1).  Only the lanes with a short history walk the
//       49 taps: a wave without one leaves after its own loads.
//   variance pass, two forms as in rt_denoise_history.hip: rt_denoise.hip's
//       5x5 B3-spline pass whose luminance tolerance is sigma_lum times the
//       pixel's own standard deviation, sqrt of v under a 3x3 binomial window
//       (always at step 1), and which filters v along with the colour
//       (weights squared), so the tolerance tightens pass by pass.  A pixel
//       with n samples is filtered in the first max(0, iterations -
//       floor(log2 n)) passes only (§4i's count, n read from the history).
//       plain : one lane per pixel, taps from global memory, any step.
//       tiled : step 1 only, 32 x 8 pixels per workgroup, the 36 x 12 halo in
//               LDS (22,464 B as §4i's): at step 1 the 25 taps and the 3x3
//               window both lie inside it.
//
// All arithmetic is IEEE binary32 in the order DESIGN.md §4j writes it (the
// library is built with -ffp-contract=off, `/` and sqrtf are correctly
// rounded, fmaxf / fminf drop a NaN operand), so tests/variance_ref.py
// restates it bit for bit.
#include "rt_internal.h"

#include <cmath>

namespace rtamd {
namespace {

__device__ __forceinline__ float lum_of(float r, float g, float b) {
    return (0.2126f * r + 0.7152f * g) + 0.0722f * b;
}

__device__ __forceinline__ uint8_t unorm8(float c) {   // the render's store (rt_trace.hip)
    return c > 0.0f ? (c < 1.0f ? (uint8_t)__builtin_rintf(c * 255.0f) : (uint8_t)255) : (uint8_t)0;
}

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

// ---------------------------------------------------------------- moments --
// project(C, P) of DESIGN.md §4h
__device__ __forceinline__ bool project(const TemporalBasis& c, float px, float py, float pz, float& u, float& v) {
    const float wx = px - c.ox, wy = py - c.oy, wz = pz - c.oz;
    const float dn = dot3(wx, wy, wz, c.nx, c.ny, c.nz);
    u = dot3(wx, wy, wz, c.ax, c.ay, c.az) / dn;
    v = dot3(wx, wy, wz, c.bx, c.by, c.bz) / dn;
    return dn * c.det > 0.0f;
}

// rt_temporal.hip's kernel, line for line, with the moments beside the colour:
// a tap costs 8 B more, a pixel writes 8 B more.
template <bool TILES>
__global__ __launch_bounds__(256) void temporal_moments_kernel(TemporalArgs a, const float2* mom_prev, float2* mom_out,
                                                               int tiles_x) {
    const int bx = (int)(blockIdx.x % (unsigned)tiles_x), by = (int)(blockIdx.x / (unsigned)tiles_x);
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int x = bx * 64 + (TILES ? (int)(wave * 16u + (lane & 15u)) : (int)lane);
    const int y = by * 4 + (TILES ? (int)(lane >> 4) : (int)wave);
    if (x >= a.width || y >= a.height) return;
    const int W = a.width, H = a.height;
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    const float4 p0 = a.hits[2 * p], p1 = a.hits[2 * p + 1];      // (t, tri, n.xy), (n.z, pos.xyz)
    const float gr = a.radiance[3 * p + 0], gg = a.radiance[3 * p + 1], gb = a.radiance[3 * p + 2];
    const float cr = gr * gr, cg = gg * gg, cb = gb * gb;
    const float l = lum_of(cr, cg, cb), l2 = l * l;
    const bool hit = __float_as_int(p0.y) >= 0;
    float orr = cr, og = cg, ob = cb, on = hit ? 1.0f : 0.0f;      // sky / invalid: passes through with n = 0
    float o1 = l, o2 = l2;
    if (hit && a.hist_prev) {
        const float nx = p0.z, ny = p0.w, nz = p1.x, qx = p1.y, qy = p1.z, qz = p1.w;
        float uc, vc, up, vp;
        const bool fc = project(a.cur, qx, qy, qz, uc, vc);
        const bool fp = project(a.prev, qx, qy, qz, up, vp);
        const float fW = (float)W, fH = (float)H;
        const float fx = (float)x + (up - uc) * fW, fy = (float)y + (vc - vp) * fH;
        if (fc && fp && fx > -1.0f && fx < fW && fy > -1.0f && fy < fH) {      // (a NaN fails)
            const float x0 = __builtin_floorf(fx), y0 = __builtin_floorf(fy);
            const float ax = fx - x0, ay = fy - y0, tol = a.plane_tol * p0.x;
            const int ix = (int)x0, iy = (int)y0;
            // the four taps' loads first, from addresses inside the frame either way
            float4 h0[4], h1[4], hc[4];
            float2 hm[4];
            bool inside[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int tx = ix + (k & 1), ty = iy + (k >> 1);
                inside[k] = tx >= 0 && tx < W && ty >= 0 && ty < H;
                const size_t q = inside[k] ? (size_t)ty * (size_t)W + (size_t)tx : p;
                h0[k] = a.hits_prev[2 * q];
                h1[k] = a.hits_prev[2 * q + 1];
                hc[k] = a.hist_prev[q];
                hm[k] = mom_prev[q];
            }
            float sr = 0.0f, sg = 0.0f, sb = 0.0f, ws = 0.0f, nm = __builtin_inff(), s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {                       // j outer, i inner
                const float wt = ((k & 1) ? ax : 1.0f - ax) * ((k >> 1) ? ay : 1.0f - ay);
                const float nd = dot3(nx, ny, nz, h0[k].z, h0[k].w, h1[k].x);
                const float pd = __builtin_fabsf(dot3(nx, ny, nz, h1[k].y - qx, h1[k].z - qy, h1[k].w - qz));
                const bool take = inside[k] && __float_as_int(h0[k].y) >= 0 && hc[k].w > 0.0f && wt > 0.0f &&
                                  nd >= a.normal_min && pd <= tol;
                sr = take ? sr + wt * hc[k].x : sr;
                sg = take ? sg + wt * hc[k].y : sg;
                sb = take ? sb + wt * hc[k].z : sb;
                ws = take ? ws + wt : ws;
                nm = take ? __builtin_fminf(nm, hc[k].w) : nm;
                s1 = take ? s1 + wt * hm[k].x : s1;
                s2 = take ? s2 + wt * hm[k].y : s2;
            }
            if (ws > 0.0f) {
                const float hr = sr / ws, hg = sg / ws, hb = sb / ws;
                const float nn = __builtin_fminf(nm + 1.0f, a.max_history), inv = 1.0f / nn;
                orr = hr + (cr - hr) * inv;
                og = hg + (cg - hg) * inv;
                ob = hb + (cb - hb) * inv;
                on = nn;
                const float h1m = s1 / ws, h2m = s2 / ws;
                o1 = h1m + (l - h1m) * inv;
                o2 = h2m + (l2 - h2m) * inv;
            }
        }
    }
    a.hist_out[p] = make_float4(orr, og, ob, on);
    mom_out[p] = make_float2(o1, o2);
    if (a.out_rgba || a.out_rad) {
        const float rr = sqrtf(orr), rg = sqrtf(og), rb = sqrtf(ob);
        if (a.out_rgba) a.out_rgba[p] = make_uchar4(unorm8(rr), unorm8(rg), unorm8(rb), 255);
        if (a.out_rad) {
            a.out_rad[3 * p + 0] = rr;
            a.out_rad[3 * p + 1] = rg;
            a.out_rad[3 * p + 2] = rb;
        }
    }
}

// option temporal_tile 0: rt_temporal.hip's shipped mapping, a wave on 64 pixels of a row
constexpr int kShippedMapping = 1;

// ----------------------------------------------------------------- filter --
// a record that is filtered at all and serves as a tap: a hit with n >= 1 (a NaN n fails)
__device__ __forceinline__ bool live(float tri_bits, float n) { return __float_as_int(tri_bits) >= 0 && n >= 1.0f; }

// max(0, n_p . n_q)^(2^npow) and the tap's distance from the centre's tangent plane, in sigma_depth * t_p
struct Guide {
    float nx, ny, nz, px, py, pz, kz;
};
__device__ __forceinline__ Guide guide_of(float4 p0, float4 p1, float kd) {
    return Guide{p0.z, p0.w, p1.x, p1.y, p1.z, p1.w, 1.0f / (kd * p0.x)};
}
__device__ __forceinline__ void guide_terms(const Guide& c, int npow, float4 q0, float4 q1, float& nd, float& x) {
    nd = __builtin_fmaxf(0.0f, (c.nx * q0.z + c.ny * q0.w) + c.nz * q1.x);
    for (int k = 0; k < npow; ++k) nd = nd * nd;
    const float ex = q1.y - c.px, ey = q1.z - c.py, ez = q1.w - c.pz;
    x = __builtin_fabsf((c.nx * ex + c.ny * ey) + c.nz * ez) * c.kz;
}

struct EstimateArgs {
    int W, H;
    const float4* hist;       // (c.rgb, n)
    const float2* mom;        // (m1, m2)
    const float4* hits;
    float4*       out;        // (c.rgb, v)
    float         kd;         // sigma_depth
    int           npow;       // normal_power_log2
    float         min_history;
};

__global__ __launch_bounds__(256) void variance_estimate(EstimateArgs a, int tiles_x) {
    const int bx = (int)(blockIdx.x % (unsigned)tiles_x), by = (int)(blockIdx.x / (unsigned)tiles_x);
    const int x = bx * 64 + (int)(threadIdx.x & 63u), y = by * 4 + (int)(threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * (size_t)a.W + (size_t)x;
    const float4 p0 = a.hits[2 * p];
    const float4 cp = a.hist[p];
    const float2 m = a.mom[p];
    if (!live(p0.y, cp.w)) {
        a.out[p] = make_float4(cp.x, cp.y, cp.z, -1.0f);
        return;
    }
    const float vt = __builtin_fmaxf(0.0f, m.y - m.x * m.x) / __builtin_fmaxf(cp.w - 1.0f, 1.0f);
    float v = vt;
    if (!(cp.w >= a.min_history)) {                // a short history: the spatial estimate too
        const Guide c = guide_of(p0, a.hits[2 * p + 1], a.kd);
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
        // a row of taps at a time, its 21 loads in flight together
#pragma unroll 1
        for (int dy = -3; dy <= 3; ++dy) {
#pragma unroll
            for (int dx = -3; dx <= 3; ++dx) {
                const int qx = x + dx, qy = y + dy;
                const bool inside = qx >= 0 && qx < a.W && qy >= 0 && qy < a.H;
                const size_t q = inside ? (size_t)qy * (size_t)a.W + (size_t)qx : p;   // a safe address either way
                const float4 q0 = a.hits[2 * q], q1 = a.hits[2 * q + 1], cq = a.hist[q];
                float nd, xx;
                guide_terms(c, a.npow, q0, q1, nd, xx);
                const float w = nd / (1.0f + xx * xx);
                const float lq = lum_of(cq.x, cq.y, cq.z);
                const float wl = w * lq;
                const bool take = inside && live(q0.y, cq.w);
                s0 = take ? s0 + w : s0;
                s1 = take ? s1 + wl : s1;
                s2 = take ? s2 + wl * lq : s2;
            }
        }
        const float mu = s1 / s0;
        const float vs = __builtin_fmaxf(0.0f, s2 / s0 - mu * mu);
        v = s0 > 0.0f ? __builtin_fmaxf(vs, vt) : vt;
    }
    a.out[p] = make_float4(cp.x, cp.y, cp.z, v);
}

struct PassArgs {
    int W, H, step;
    const float4* in;         // (c.rgb, v): the estimate's or the previous pass's half of the workspace
    const float*  hist;       // the history, read for n alone (4 floats per pixel)
    const float4* hits;
    float4*       out_c;      // every pass but the last (else null)
    uchar4*       out_rgba;   // last pass, nullable
    float*        out_rad;    // last pass, nullable
    float         kd;         // sigma_depth
    float         sl;         // sigma_lum
    int           npow;       // normal_power_log2
    int           left;       // iterations - pass index: a pixel is filtered while floor(log2 n) < left
};

// a tap-worthy pixel (v < 0 fails, a NaN v passes) is filtered in this pass while floor(log2 n) < left
__device__ __forceinline__ bool filtered(const PassArgs& a, float v, float n) {
    const int e = ((__float_as_int(n) >> 23) & 0xFF) - 127;
    return !(v < 0.0f) && e < a.left;
}

__device__ __forceinline__ void store_px(const PassArgs& a, size_t p, float r, float g, float b, float v) {
    if (a.out_c) {
        a.out_c[p] = make_float4(r, g, b, v);
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

// the 3x3 window's binomial B = [1/2, 1/4] and the B3 spline h = [3/8, 1/4, 1/16], by |offset|
constexpr float b2(int o) { return o == 0 ? 0.5f : 0.25f; }
constexpr float b3(int o) { return o == 0 ? 0.375f : ((o == 1 || o == -1) ? 0.25f : 0.0625f); }

struct Sums {
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, ws = 0.0f, vs = 0.0f;
};

// 1 / (sigma_lum * the blurred standard deviation + 1e-6)
__device__ __forceinline__ float inv_tolerance(const PassArgs& a, float g, float gw) {
    return 1.0f / ((a.sl * sqrtf(g / gw)) + 1e-6f);
}

// One tap: hh = h[|dx|] * h[|dy|]; q0 / q1 the tap's hit record, cq its (c.rgb, v), lq its luminance.
__device__ __forceinline__ void tap(Sums& s, const Guide& c, const PassArgs& a, float lum, float isl, float hh, float4 q0,
                                    float4 q1, float4 cq, float lq, bool inside) {
    float nd, x;
    guide_terms(c, a.npow, q0, q1, nd, x);
    const float y = __builtin_fabsf(lum - lq) * isl;
    const float w = (hh * nd) / ((1.0f + x * x) * (1.0f + y * y));
    const bool take = inside && cq.w >= 0.0f;
    s.sr = take ? s.sr + w * cq.x : s.sr;
    s.sg = take ? s.sg + w * cq.y : s.sg;
    s.sb = take ? s.sb + w * cq.z : s.sb;
    s.ws = take ? s.ws + w : s.ws;
    s.vs = take ? s.vs + (w * w) * cq.w : s.vs;
}

__device__ __forceinline__ void finish(const PassArgs& a, size_t p, const Sums& s, float4 cp) {
    const bool ok = s.ws > 0.0f;                   // NaN or zero: the pixel passes through
    store_px(a, p, ok ? s.sr / s.ws : cp.x, ok ? s.sg / s.ws : cp.y, ok ? s.sb / s.ws : cp.z,
             ok ? s.vs / (s.ws * s.ws) : cp.w);
}

// ---- plain: one lane per pixel, 64 x 4 pixels per workgroup, taps from global memory
__global__ __launch_bounds__(256, 4) void denoise_variance_plain(PassArgs a, int tiles_x) {
    const int bx = (int)(blockIdx.x % (unsigned)tiles_x), by = (int)(blockIdx.x / (unsigned)tiles_x);
    const int x = bx * 64 + (int)(threadIdx.x & 63u), y = by * 4 + (int)(threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * (size_t)a.W + (size_t)x;
    const float4 cp = a.in[p];
    if (!filtered(a, cp.w, a.hist[4 * p + 3])) {   // not a tap, or history long enough: pass through
        store_px(a, p, cp.x, cp.y, cp.z, cp.w);
        return;
    }
    // the 3x3 window, always at step 1: the records' fourth words
    float g = 0.0f, gw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx, qy = y + dy;
            const bool inside = qx >= 0 && qx < a.W && qy >= 0 && qy < a.H;
            const size_t q = inside ? (size_t)qy * (size_t)a.W + (size_t)qx : p;
            const float vq = reinterpret_cast<const float*>(a.in)[4 * q + 3];
            const bool take = inside && vq >= 0.0f;
            g = take ? g + (b2(dx) * b2(dy)) * vq : g;
            gw = take ? gw + b2(dx) * b2(dy) : gw;
        }
    }
    const float isl = inv_tolerance(a, g, gw);
    const Guide c = guide_of(a.hits[2 * p], a.hits[2 * p + 1], a.kd);
    const float lum = lum_of(cp.x, cp.y, cp.z);
    Sums s;
    // a row of taps at a time: its 15 loads are in flight together, the next row's wait (registers)
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * a.step, qy = y + dy * a.step;
            const bool inside = qx >= 0 && qx < a.W && qy >= 0 && qy < a.H;
            const size_t q = inside ? (size_t)qy * (size_t)a.W + (size_t)qx : p;   // a safe address either way
            const float4 cq = a.in[q];
            tap(s, c, a, lum, isl, b3(dx) * b3(dy), a.hits[2 * q], a.hits[2 * q + 1], cq, lum_of(cq.x, cq.y, cq.z),
                inside);
        }
    }
    finish(a, p, s, cp);
}

// ---- tiled, step 1: 32 x 8 pixels per workgroup, the halo tile in LDS
constexpr int kTileX = 32, kTileY = 8, kHaloX = kTileX + 4, kHaloY = kTileY + 4;

__global__ __launch_bounds__(256, 4) void denoise_variance_tiled(PassArgs a, int tiles_x) {
    __shared__ float4 s_c[kHaloX * kHaloY], s_h0[kHaloX * kHaloY], s_h1[kHaloX * kHaloY];
    __shared__ float s_lum[kHaloX * kHaloY];
    const int bx = (int)(blockIdx.x % (unsigned)tiles_x), by = (int)(blockIdx.x / (unsigned)tiles_x);
    const int W = a.W, H = a.H;
    for (int e = (int)threadIdx.x; e < kHaloX * kHaloY; e += 256) {
        const int i = e % kHaloX, j = e / kHaloX;
        const int x = bx * kTileX - 2 + i, y = by * kTileY - 2 + j;
        float4 cq = make_float4(0.0f, 0.0f, 0.0f, -1.0f), q0 = make_float4(0.0f, __int_as_float(-1), 0.0f, 0.0f),
               q1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // outside the frame: not a tap
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
    const int x = bx * kTileX + i, y = by * kTileY + j;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    const int e0 = (j + 2) * kHaloX + (i + 2);
    const float4 cp = s_c[e0];
    if (!filtered(a, cp.w, a.hist[4 * p + 3])) {
        store_px(a, p, cp.x, cp.y, cp.z, cp.w);
        return;
    }
    float g = 0.0f, gw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const float vq = s_c[e0 + dy * kHaloX + dx].w;
            const bool take = vq >= 0.0f;          // (a record outside the frame holds -1)
            g = take ? g + (b2(dx) * b2(dy)) * vq : g;
            gw = take ? gw + b2(dx) * b2(dy) : gw;
        }
    }
    const float isl = inv_tolerance(a, g, gw);
    const Guide c = guide_of(s_h0[e0], s_h1[e0], a.kd);
    const float lum = s_lum[e0];
    Sums s;
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int e = e0 + dy * kHaloX + dx;
            tap(s, c, a, lum, isl, b3(dx) * b3(dy), s_h0[e], s_h1[e], s_c[e], s_lum[e], true);
        }
    }
    finish(a, p, s, cp);
}

// The form step 1 takes by default (option denoise_kernel 0), from
// tools/variance_bench.py's per-pass times on config 3 at 1920x1080
// (profiles/variance).  Pass 0 filters every live pixel whatever
// the history's length (floor(log2 n) < iterations up to n = 2^iterations - 1),
// so the tile's staging is never wasted there: tiled 0.0745 / 0.0760 / 0.0781 ms
// against plain 0.0972 / 0.0976 / 0.0981 after 1 frame / 8 static frames / 8
// frames orbiting 1 degree per frame.
constexpr bool kTiledAtStep1 = true;

}  // namespace

hipError_t launch_temporal_moments(const TemporalArgs& t, const float2* mom_prev, float2* mom_out, hipStream_t stream) {
    const size_t tx = ((size_t)t.width + 63) / 64, ty = ((size_t)t.height + 3) / 4;   // <= 2^29 workgroups
    const int form = t.form ? t.form : kShippedMapping;
    if (form == 2)
        hipLaunchKernelGGL(temporal_moments_kernel<true>, dim3((unsigned)(tx * ty)), dim3(256), 0, stream, t, mom_prev,
                           mom_out, (int)tx);
    else
        hipLaunchKernelGGL(temporal_moments_kernel<false>, dim3((unsigned)(tx * ty)), dim3(256), 0, stream, t, mom_prev,
                           mom_out, (int)tx);
    return hipGetLastError();
}

hipError_t launch_denoise_variance(const VarianceArgs& d, hipStream_t stream) {
    const size_t px = (size_t)d.width * (size_t)d.height;
    float4* half[2] = {d.workspace, d.workspace + px};
    const size_t ptx = ((size_t)d.width + 63) / 64, pty = ((size_t)d.height + 3) / 4;
    if (d.only_pass < 0) {
        EstimateArgs e;
        e.W = d.width; e.H = d.height;
        e.hist = d.hist; e.mom = d.mom; e.hits = d.hits;
        e.out = half[0];
        e.kd = d.sigma_depth;
        e.npow = d.normal_power_log2;
        e.min_history = (float)d.min_history;
        hipLaunchKernelGGL(variance_estimate, dim3((unsigned)(ptx * pty)), dim3(256), 0, stream, e, (int)ptx);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    if (d.stage == 0) return hipSuccess;           // option variance_stage 0: the estimate alone (timing)
    for (int i = 0; i < d.iterations; ++i) {
        if (d.only_pass >= 0 && i != d.only_pass) continue;
        PassArgs a;
        a.W = d.width; a.H = d.height; a.step = 1 << i;
        a.in = half[i & 1];
        a.hist = reinterpret_cast<const float*>(d.hist);
        a.hits = d.hits;
        const bool last = i == d.iterations - 1;
        a.out_c = last ? nullptr : half[(i + 1) & 1];
        a.out_rgba = last ? d.out_rgba : nullptr;
        a.out_rad = last ? d.out_rad : nullptr;
        a.kd = d.sigma_depth;
        a.sl = d.sigma_lum;
        a.npow = d.normal_power_log2;
        a.left = d.iterations - i;
        const size_t ttx = ((size_t)d.width + kTileX - 1) / kTileX, tty = ((size_t)d.height + kTileY - 1) / kTileY;
        bool tiled = i == 0 && (d.form == 2 || (d.form == 0 && kTiledAtStep1));
        if (ttx * tty > 0x7FFFFFFFull) tiled = false;                // past a 1-D grid: the plain form
        if (tiled)
            hipLaunchKernelGGL(denoise_variance_tiled, dim3((unsigned)(ttx * tty)), dim3(256), 0, stream, a, (int)ttx);
        else
            hipLaunchKernelGGL(denoise_variance_plain, dim3((unsigned)(ptx * pty)), dim3(256), 0, stream, a, (int)ptx);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

}  // namespace rtamd

extern "C" {

void rt_variance_default_params(rt_variance_params* out) {
    if (!out) return;
    out->iterations = 4;
    out->normal_power_log2 = 7;
    out->sigma_depth = 0.005f;
    out->sigma_lum = 1.0f;
    out->min_history = 4;
    out->reserved[0] = out->reserved[1] = out->reserved[2] = 0;
}

}  // extern "C"
