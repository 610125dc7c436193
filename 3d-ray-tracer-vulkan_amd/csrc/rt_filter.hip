// rt_filter.hip — the edge-avoiding a-trous filters (rtamd.h "denoise" and
// "variance").
//
// One 5x5 B3-spline wavelet pass, step 2^i in pass i, whose tap weights fall
// with the angle between the first-hit normals, with the tap's distance from
// the centre pixel's tangent plane and with the luminance difference.  The
// guides are the rt_hit records rt_render_hits_device writes.  Three filters
// take this pass, each a compile-time policy of the two kernel templates:
//
//   Radiance (rt_denoise_device, §4g): a 1-sample frame.  Pass 0 reads the
//       render's 12-byte radiance (g, squared on the fly); the passes between
//       keep float4(c.rgb, luminance), so a pixel's luminance is computed once,
//       by its writer.  A pixel without a hit passes through.
//   History (rt_denoise_history_device, §4i): records (c.rgb, n) of a history.
//       A pixel with n samples is filtered in the first max(0, iterations -
//       floor(log2 n)) passes only, its colour tolerance tightens by n, and a
//       tap counts n_q times.  A pixel without a hit or with n < 1 (or NaN) is
//       never filtered and never a tap.
//   Variance (rt_denoise_variance_device, §4j): records (c.rgb, v), v the
//       variance of the pixel's mean, written first by variance_estimate below
//       (v = -1: never filtered, never a tap).  The luminance tolerance is
//       sigma_lum times the pixel's own standard deviation, sqrt of v under a
//       3x3 binomial window (always at step 1), and v is filtered along with
//       the colour (weights squared).  §4i's count of passes, n read from the
//       history.
// A fourth policy, Albedo (rt_denoise_albedo_device, §4p), is Radiance on the
// illumination: its pass 0 divides the colour by the first-hit albedo buffer
// (written by first_hit_albedo below, rt_albedo_device), its last pass
// multiplies the centre's result back, and the passes between are Radiance's.
//
// Every pass but the last writes its filter's record into the other half of
// the caller's workspace; the last writes sqrt(c) and the RGBA8 pixels.  All
// arithmetic is IEEE binary32 in the order DESIGN.md writes it (the library is
// built with -ffp-contract=off, `/` and sqrtf are correctly rounded, fmaxf /
// fminf drop a NaN operand), so tests/denoise_ref.py, denoise_history_ref.py
// and variance_ref.py restate it bit for bit.
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
//           would touch 16 of the 64 banks).  The History and Variance records
//           hold no luminance: theirs is a fourth, 4-byte plane (22,464 B in
//           all), each computed once, by the lane that stages the record.  The
//           Variance filter's 3x3 window is at pixel step 1 and lies inside a
//           class's tile at step 1 only, so that filter is tiled at step 1
//           alone.
// Which form a step size gets by default was measured (kTiledByStep below).
#include "rt_internal.h"
#include "rt_pixel.h"

#include <type_traits>

namespace rtamd {
namespace {

struct PassArgs {
    int W, H, step;
    const float4* in;         // this pass's records (Radiance, pass 0: null)
    const float*  side;       // Radiance, pass 0: the render's radiance, 3 floats per pixel (else null);
                              //   Variance: the history, read for n alone (4 floats per pixel)
    const float4* hits;       // rt_hit as 2 float4: (t, tri, n.xy), (n.z, pos.xyz)
    float4*       out_c;      // every pass but the last (else null)
    uchar4*       out_rgba;   // last pass, nullable
    float*        out_rad;    // last pass, nullable
    float         kd;         // sigma_depth
    float         tol;        // Radiance, History: step / sigma_color; Variance: sigma_lum
    int           npow;       // normal_power_log2
    int           left;       // iterations - pass index: a pixel is filtered while floor(log2 n) < left
};

// a record that is filtered at all and serves as a tap: a hit with n >= 1 (a NaN n fails)
__device__ __forceinline__ bool live(float tri_bits, float n) { return __float_as_int(tri_bits) >= 0 && n >= 1.0f; }

// floor(log2 n), n's unbiased exponent: a pixel is still filtered in a pass while it is below PassArgs::left
__device__ __forceinline__ int log2_floor(float n) { return ((__float_as_int(n) >> 23) & 0xFF) - 127; }

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

// The centre pixel's own record and hit record.
struct Centre {
    float4 c, h0, h1;
};

struct Sums {
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, ws = 0.0f, vs = 0.0f;
};

// ---- the three filters: what a pass does not share.
// kLumPlane   : the tiled form stages a plane of luminances (else the record's fourth word is one)
// kOutsideW   : the fourth word of the record staged for a tap outside the frame
// kTiledStep1 : the tiled form exists at step 1 alone
// kFiltersW   : the record's fourth word is filtered along with the colour, its weights squared
// load        : the record of pixel q
// lum         : a record's luminance
// test        : reads the pixel's record c() into o.c and what of its hit record (h0(), h1(): its halves) the
//               test needs, in the order this filter's loads have always had, and says whether the pixel
//               passes through this pass unfiltered (having read no more than that)
// kTestPasses : the sense of test's answer: true = passes through, false = is filtered.  The same test stated
//               the other way round compiles to another block order and measured 0.5 to 3 % slower per pass
//               (profiles/filters): each filter keeps the sense its kernels have always had
// kWindow     : the kernels sum the fourth words of the pixel's 3x3 neighbourhood (g, weights gw) for tolerance
// tolerance   : the factor on the centre's luminance difference
// weight      : a tap's weight before the guides' and the luminance's denominators
// is_tap      : whether a record inside the frame counts
// fourth      : the fourth word stored with the colour (r, g, b); w = the centre's own, or with kFiltersW
//               the filtered one
// Args        : the kernels' first argument, PassArgs or a struct derived from it
// display     : what the last pass does to the centre's colour before the display store
struct Radiance {
    using Args = PassArgs;
    static constexpr bool  kLumPlane = false;
    static constexpr float kOutsideW = 0.0f;
    static constexpr bool  kTiledStep1 = false;
    static constexpr bool  kFiltersW = false;
    static constexpr bool  kWindow = false;
    static constexpr bool  kTestPasses = true;
    __device__ static __forceinline__ float4 load(const PassArgs& a, size_t q) {
        if (a.side) {
            const float gr = a.side[3 * q + 0], gg = a.side[3 * q + 1], gb = a.side[3 * q + 2];
            const float r = gr * gr, g = gg * gg, b = gb * gb;
            return make_float4(r, g, b, lum_of(r, g, b));
        }
        return a.in[q];
    }
    __device__ static __forceinline__ float lum(float4 c) { return c.w; }
    template <class C, class H0, class H1>
    __device__ static __forceinline__ bool test(const PassArgs&, size_t, C c, H0 h0, H1 h1, Centre& o) {
        o.h0 = h0();
        o.h1 = h1();
        o.c = c();
        return __float_as_int(o.h0.y) < 0;         // sky / invalid
    }
    template <class H0, class H1>
    __device__ static __forceinline__ Guide guide(const PassArgs& a, H0, H1, const Centre& o) {
        return guide_of(o.h0, o.h1, a.kd);
    }
    __device__ static __forceinline__ float4 load_tap(const PassArgs& a, size_t q, float4& q0, float4& q1) {
        q0 = a.hits[2 * q];
        q1 = a.hits[2 * q + 1];
        return load(a, q);
    }
    __device__ static __forceinline__ float tolerance(const PassArgs& a, float4, float, float) { return a.tol; }
    __device__ static __forceinline__ float weight(float hn, float4) { return hn; }
    __device__ static __forceinline__ bool is_tap(float4 q0, float4) { return __float_as_int(q0.y) >= 0; }
    __device__ static __forceinline__ float fourth(float r, float g, float b, float) { return lum_of(r, g, b); }
    __device__ static __forceinline__ void display(const PassArgs&, size_t, float&, float&, float&) {}
};

struct History {
    using Args = PassArgs;
    static constexpr bool  kLumPlane = true;
    static constexpr float kOutsideW = 0.0f;       // without a sample
    static constexpr bool  kTiledStep1 = false;
    static constexpr bool  kFiltersW = false;
    static constexpr bool  kWindow = false;
    static constexpr bool  kTestPasses = false;
    __device__ static __forceinline__ float4 load(const PassArgs& a, size_t q) { return a.in[q]; }
    __device__ static __forceinline__ float lum(float4 c) { return lum_of(c.x, c.y, c.z); }
    template <class C, class H0, class H1>
    __device__ static __forceinline__ bool test(const PassArgs& a, size_t, C c, H0 h0, H1, Centre& o) {
        o.h0 = h0();
        o.c = c();
        const int e = log2_floor(o.c.w);
        return live(o.h0.y, o.c.w) && e < a.left;       // (else: sky, no sample, or history long enough)
    }
    template <class H0, class H1>
    __device__ static __forceinline__ Guide guide(const PassArgs& a, H0, H1 h1, const Centre& o) {
        return guide_of(o.h0, h1(), a.kd);
    }
    __device__ static __forceinline__ float4 load_tap(const PassArgs& a, size_t q, float4& q0, float4& q1) {
        const float4 cq = a.in[q];
        q0 = a.hits[2 * q];
        q1 = a.hits[2 * q + 1];
        return cq;
    }
    __device__ static __forceinline__ float tolerance(const PassArgs& a, float4 cp, float, float) {
        return a.tol * cp.w;                       // (isc * step) * n_p
    }
    __device__ static __forceinline__ float weight(float hn, float4 cq) { return hn * cq.w; }
    __device__ static __forceinline__ bool is_tap(float4 q0, float4 cq) { return live(q0.y, cq.w); }
    __device__ static __forceinline__ float fourth(float, float, float, float n) { return n; }
    __device__ static __forceinline__ void display(const PassArgs&, size_t, float&, float&, float&) {}
};

struct Variance {
    using Args = PassArgs;
    static constexpr bool  kLumPlane = true;
    static constexpr float kOutsideW = -1.0f;      // not a tap
    static constexpr bool  kTiledStep1 = true;
    static constexpr bool  kFiltersW = true;
    static constexpr bool  kWindow = true;
    static constexpr bool  kTestPasses = false;
    __device__ static __forceinline__ float4 load(const PassArgs& a, size_t q) { return a.in[q]; }
    __device__ static __forceinline__ float lum(float4 c) { return lum_of(c.x, c.y, c.z); }
    // a tap-worthy pixel (v < 0 fails, a NaN v passes) is filtered in this pass while floor(log2 n) < left
    template <class C, class H0, class H1>
    __device__ static __forceinline__ bool test(const PassArgs& a, size_t p, C c, H0, H1, Centre& o) {
        o.c = c();
        const int e = log2_floor(a.side[4 * p + 3]);
        return !(o.c.w < 0.0f) && e < a.left;
    }
    template <class H0, class H1>
    __device__ static __forceinline__ Guide guide(const PassArgs& a, H0 h0, H1 h1, const Centre&) {
        return guide_of(h0(), h1(), a.kd);
    }
    __device__ static __forceinline__ float4 load_tap(const PassArgs& a, size_t q, float4& q0, float4& q1) {
        const float4 cq = a.in[q];
        q0 = a.hits[2 * q];
        q1 = a.hits[2 * q + 1];
        return cq;
    }
    // 1 / (sigma_lum * the blurred standard deviation + 1e-6): the 3x3 window, always at step 1
    __device__ static __forceinline__ float tolerance(const PassArgs& a, float4, float g, float gw) {
        return 1.0f / ((a.tol * sqrtf(g / gw)) + 1e-6f);
    }
    __device__ static __forceinline__ float weight(float hn, float4) { return hn; }
    __device__ static __forceinline__ bool is_tap(float4, float4 cq) { return cq.w >= 0.0f; }
    __device__ static __forceinline__ float fourth(float, float, float, float v) { return v; }
    __device__ static __forceinline__ void display(const PassArgs&, size_t, float&, float&, float&) {}
};

// Albedo (rt_denoise_albedo_device, §4p): the Radiance filter on the illumination.  Pass 0 (kDivides) reads a
// pixel or tap q as c = g * g and divides it per channel by d_q, the first three words of q's albedo record;
// the last pass (kMultiplies) multiplies the centre's result by d_p before the display store; a one-pass filter
// does both.  The passes between are Radiance's own kernels, and each of the three is an instantiation of its
// own: one kernel doing both and choosing at run time, used for every pass, ran the whole 4-pass filter 5.8 %
// over the colour filter's instead of 2.6 %.  The albedo buffer is a kernel argument behind
// PassArgs' own, so the other filters' kernels keep their argument layout.
struct AlbedoPassArgs : PassArgs {
    const float4* albedo;     // (d.rgb, any) per pixel
};
template <bool kDivides, bool kMultiplies>
struct Albedo : Radiance {
    using Args = AlbedoPassArgs;
    __device__ static __forceinline__ float4 load(const Args& a, size_t q) {
        if constexpr (kDivides) {                  // pass 0: a.side is the radiance
            const float gr = a.side[3 * q + 0], gg = a.side[3 * q + 1], gb = a.side[3 * q + 2];
            const float4 d = a.albedo[q];
            const float r = (gr * gr) / d.x, g = (gg * gg) / d.y, b = (gb * gb) / d.z;
            return make_float4(r, g, b, lum_of(r, g, b));
        } else {
            return Radiance::load(a, q);
        }
    }
    __device__ static __forceinline__ float4 load_tap(const Args& a, size_t q, float4& q0, float4& q1) {
        q0 = a.hits[2 * q];
        q1 = a.hits[2 * q + 1];
        return load(a, q);
    }
    __device__ static __forceinline__ void display(const Args& a, size_t p, float& r, float& g, float& b) {
        if constexpr (kMultiplies) {
            const float4 d = a.albedo[p];
            r = r * d.x;
            g = g * d.y;
            b = b * d.z;
        }
    }
};

template <class F>
__device__ __forceinline__ void store_px(const typename F::Args& a, size_t p, float r, float g, float b, float w) {
    if (a.out_c) {
        a.out_c[p] = make_float4(r, g, b, F::fourth(r, g, b, w));
        return;
    }
    F::display(a, p, r, g, b);
    store_display(a.out_rgba, a.out_rad, p, r, g, b);
}

// One tap: hh = h[|dx|] * h[|dy|]; q0 / q1 the tap's hit record, cq its record, lq its luminance.
// A tap outside the frame or one that does not count leaves the sums as they are.
template <class F>
__device__ __forceinline__ void tap(Sums& s, const Guide& c, const PassArgs& a, float lum, float tol, float hh, float4 q0,
                                    float4 q1, float4 cq, float lq, bool inside) {
    float nd, x;
    guide_terms(c, a.npow, q0, q1, nd, x);
    const float y = __builtin_fabsf(lum - lq) * tol;
    const float w = F::weight(hh * nd, cq) / ((1.0f + x * x) * (1.0f + y * y));
    const bool take = inside && F::is_tap(q0, cq);
    s.sr = take ? s.sr + w * cq.x : s.sr;
    s.sg = take ? s.sg + w * cq.y : s.sg;
    s.sb = take ? s.sb + w * cq.z : s.sb;
    s.ws = take ? s.ws + w : s.ws;
    if constexpr (F::kFiltersW) s.vs = take ? s.vs + (w * w) * cq.w : s.vs;
}

template <class F>
__device__ __forceinline__ void finish(const typename F::Args& a, size_t p, const Sums& s, float4 cp) {
    const bool ok = s.ws > 0.0f;                   // NaN or zero: the pixel passes through
    float w = cp.w;
    if constexpr (F::kFiltersW) w = ok ? s.vs / (s.ws * s.ws) : cp.w;
    store_px<F>(a, p, ok ? s.sr / s.ws : cp.x, ok ? s.sg / s.ws : cp.y, ok ? s.sb / s.ws : cp.z, w);
}

// ---- plain: one lane per pixel, 64 x 4 pixels per workgroup, taps from global memory
template <class F>
__global__ __launch_bounds__(256, 4) void atrous_plain(typename F::Args a, int tiles_x) {
    const int bx = (int)(blockIdx.x % (unsigned)tiles_x), by = (int)(blockIdx.x / (unsigned)tiles_x);
    const int x = bx * 64 + (int)(threadIdx.x & 63u), y = by * 4 + (int)(threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * (size_t)a.W + (size_t)x;
    const auto h0 = [&] { return a.hits[2 * p]; };
    const auto h1 = [&] { return a.hits[2 * p + 1]; };
    Centre o;
    const bool t = F::test(a, p, [&] { return F::load(a, p); }, h0, h1, o);
    const float4 cp = o.c;
    if (F::kTestPasses ? t : !t) {
        store_px<F>(a, p, cp.x, cp.y, cp.z, cp.w);
        return;
    }
    // the 3x3 window, always at step 1: the records' fourth words, binomially weighted
    float g = 0.0f, gw = 0.0f;
    if constexpr (F::kWindow) {
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
    }
    const float tol = F::tolerance(a, cp, g, gw);
    const Guide c = F::guide(a, h0, h1, o);
    const float lum = F::lum(cp);
    Sums s;
    // a row of taps at a time: its 15 loads are in flight together, the next row's wait (registers)
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * a.step, qy = y + dy * a.step;
            const bool inside = qx >= 0 && qx < a.W && qy >= 0 && qy < a.H;
            const size_t q = inside ? (size_t)qy * (size_t)a.W + (size_t)qx : p;   // a safe address either way
            float4 q0, q1;
            const float4 cq = F::load_tap(a, q, q0, q1);
            tap<F>(s, c, a, lum, tol, b3(dx) * b3(dy), q0, q1, cq, F::lum(cq), inside);
        }
    }
    finish<F>(a, p, s, cp);
}

// ---- tiled: 32 x 8 pixels of one residue class per workgroup, the halo tile in LDS
constexpr int kTileX = 32, kTileY = 8, kHaloX = kTileX + 4, kHaloY = kTileY + 4;

template <class F>
__global__ __launch_bounds__(256, 4) void atrous_tiled(typename F::Args a, int tiles_x) {
    __shared__ float4 s_c[kHaloX * kHaloY], s_h0[kHaloX * kHaloY], s_h1[kHaloX * kHaloY];
    __shared__ float s_lum[F::kLumPlane ? kHaloX * kHaloY : 1];
    const int step = F::kTiledStep1 ? 1 : a.step;
    const unsigned s = (unsigned)step;
    unsigned id = blockIdx.x;                      // ((by * tiles_x + bx) * s + ry) * s + rx
    const int rx = (int)(id % s); id /= s;
    const int ry = (int)(id % s); id /= s;
    const int bx = (int)(id % (unsigned)tiles_x), by = (int)(id / (unsigned)tiles_x);
    // class coordinates (cx, cy) are pixel (rx + step * cx, ry + step * cy); 64-bit: step * cx may pass 2^31
    // (not at step 1)
    using coord = std::conditional_t<F::kTiledStep1, int, long long>;
    const coord W = a.W, H = a.H, st = step;
    // this class ends before the tile: the whole workgroup leaves, before any barrier (at step 1 there is one
    // class and the grid is exact: no such tile)
    if constexpr (!F::kTiledStep1)
        if (rx + st * (bx * kTileX) >= W || ry + st * (by * kTileY) >= H) return;
    for (int e = (int)threadIdx.x; e < kHaloX * kHaloY; e += 256) {
        const int i = e % kHaloX, j = e / kHaloX;
        const coord x = rx + st * (bx * kTileX - 2 + i), y = ry + st * (by * kTileY - 2 + j);
        float4 cq = make_float4(0.0f, 0.0f, 0.0f, F::kOutsideW), q0 = make_float4(0.0f, __int_as_float(-1), 0.0f, 0.0f),
               q1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // outside the frame: a tap without a hit, and no tap
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const size_t q = (size_t)y * (size_t)W + (size_t)x;
            cq = F::load(a, q);
            q0 = a.hits[2 * q];
            q1 = a.hits[2 * q + 1];
        }
        s_c[e] = cq;
        s_h0[e] = q0;
        s_h1[e] = q1;
        if constexpr (F::kLumPlane) s_lum[e] = F::lum(cq);
    }
    __syncthreads();                               // every lane of the workgroup arrives: no lane has left yet
    const int i = (int)(threadIdx.x & 31u), j = (int)(threadIdx.x >> 5);
    const coord x = rx + st * (bx * kTileX + i), y = ry + st * (by * kTileY + j);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    const int e0 = (j + 2) * kHaloX + (i + 2);
    const auto lum_at = [&](int e) { return F::kLumPlane ? s_lum[e] : F::lum(s_c[e]); };
    const auto h0 = [&] { return s_h0[e0]; };
    const auto h1 = [&] { return s_h1[e0]; };
    Centre o;
    const bool t = F::test(a, p, [&] { return s_c[e0]; }, h0, h1, o);
    const float4 cp = o.c;
    if (F::kTestPasses ? t : !t) {
        store_px<F>(a, p, cp.x, cp.y, cp.z, cp.w);
        return;
    }
    float g = 0.0f, gw = 0.0f;                     // the 3x3 window (at step 1 it lies inside the tile)
    if constexpr (F::kWindow) {
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const float vq = s_c[e0 + dy * kHaloX + dx].w;
                const bool take = vq >= 0.0f;      // (a record outside the frame holds kOutsideW)
                g = take ? g + (b2(dx) * b2(dy)) * vq : g;
                gw = take ? gw + b2(dx) * b2(dy) : gw;
            }
        }
    }
    const float tol = F::tolerance(a, cp, g, gw);
    const Guide c = F::guide(a, h0, h1, o);
    const float lum = lum_at(e0);
    Sums sm;
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int e = e0 + dy * kHaloX + dx;
            tap<F>(sm, c, a, lum, tol, b3(dx) * b3(dy), s_h0[e], s_h1[e], s_c[e], lum_at(e), true);
        }
    }
    finish<F>(a, p, sm, cp);
}

// ---- the Variance filter's first records
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

// One lane per pixel writes (c.rgb, v), v = the variance of the pixel's mean:
// the temporal one, max(0, m2 - m1^2) / max(n - 1, 1), where the history has
// min_history samples, else the larger of it and a 7x7 spatial estimate
// weighted by the guides.  Only the lanes with a short history walk the 49
// taps: a wave without one leaves after its own loads.
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

// The form each step size 2^i takes by default (option denoise_kernel 0), a row per filter.
//
// Radiance: the faster one of tools/denoise_bench.py's per-pass times on
// config 3 at 1920x1080 (profiles/denoise): tiled 0.075 / 0.079
// / 0.091 ms against plain 0.092 / 0.094 / 0.100 at steps 1 / 2 / 4, tiled
// 0.134 against plain 0.096 at step 8 (a residue class's tile rows lie 8 pixels
// apart, so its staging loads use 16 bytes of every 128 fetched).  Steps 16 and
// 32 keep the plain form; their times are in DESIGN.md §4g.
//
// History: from tools/adaptive_bench.py's per-pass times on config 3 at
// 1920x1080 (profiles/adaptive).  With one sample everywhere the
// passes cost what the Radiance filter's cost and the same forms win: tiled
// 0.070 / 0.076 / 0.088 ms against plain 0.089 / 0.094 / 0.100 at steps 1 / 2 /
// 4, plain 0.096 against tiled 0.134 at step 8.  After 8 frames only pass 0
// still filters every hit pixel.  The later passes mostly pass through, and
// there the plain form wins by far: a wave whose 64 pixels all pass through
// leaves after two loads and a store each, while a tile stages its halo
// whatever its pixels do.  Plain 0.019 against tiled 0.046 / 0.074 / 0.124 at
// steps 2 / 4 / 8 with a static camera, 0.035 / 0.034 / 0.032 against 0.053 /
// 0.081 / 0.134 orbiting 1 degree per frame.  The long history is the state a
// sequence spends its time in, so steps 2 and 4 take the plain form: the whole
// filter takes 0.03 ms more on a sequence's first frame and 0.06 to 0.08 ms
// less on every frame from the eighth on.
//
// Variance (tiled at step 1 alone): from tools/variance_bench.py's per-pass
// times on config 3 at 1920x1080 (profiles/variance).  Pass 0
// filters every live pixel whatever the history's length (floor(log2 n) <
// iterations up to n = 2^iterations - 1), so the tile's staging is never wasted
// there: tiled 0.0745 / 0.0760 / 0.0781 ms against plain 0.0972 / 0.0976 /
// 0.0981 after 1 frame / 8 static frames / 8 frames orbiting 1 degree per
// frame.
constexpr bool kTiledByStep[3][6] = {{true, true, true, false, false, false},
                                     {true, false, false, false, false, false},
                                     {true, false, false, false, false, false}};

using PassKernel = void (*)(PassArgs, int);
constexpr PassKernel kPlain[3] = {atrous_plain<Radiance>, atrous_plain<History>, atrous_plain<Variance>};
constexpr PassKernel kTiled[3] = {atrous_tiled<Radiance>, atrous_tiled<History>, atrous_tiled<Variance>};
// the albedo form's pass 0, last pass and only pass, [multiplies][divides] (neither: Radiance's kernels)
using AlbedoKernel = void (*)(AlbedoPassArgs, int);
constexpr AlbedoKernel kAlbedoPlain[2][2] = {{nullptr, atrous_plain<Albedo<true, false>>},
                                             {atrous_plain<Albedo<false, true>>, atrous_plain<Albedo<true, true>>}};
constexpr AlbedoKernel kAlbedoTiled[2][2] = {{nullptr, atrous_tiled<Albedo<true, false>>},
                                             {atrous_tiled<Albedo<false, true>>, atrous_tiled<Albedo<true, true>>}};

// ---- the first-hit albedo buffer (rt_albedo_device, §4p)
// a channel the filter may divide by: 2^-10 <= a <= 2^10, else 1 (a NaN fails both comparisons)
__device__ __forceinline__ float divisor_of(float a) { return (a >= 0x1p-10f && a <= 0x1p10f) ? a : 1.0f; }

// One lane per pixel: (d.rgb, type) of the triangle the pixel's hit record names, (1, 1, 1, -1) where it
// names none of the scene's n_flat.  Reads the record's tri alone.
__global__ __launch_bounds__(256) void first_hit_albedo(const int* hits, const float4* mats, unsigned n_flat, float4* out,
                                                        size_t px) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= px) return;
    const unsigned tri = (unsigned)hits[8 * p + 1];
    float4 r = make_float4(1.0f, 1.0f, 1.0f, -1.0f);
    if (tri < n_flat) {
        const float4 m = mats[(size_t)kShadeStride * tri];
        r = make_float4(divisor_of(m.x), divisor_of(m.y), divisor_of(m.z), m.w);
    }
    out[p] = r;
}

}  // namespace

hipError_t launch_albedo(const float4* hits, const float4* mats, unsigned n_flat, float4* out, size_t px,
                         hipStream_t stream) {
    hipLaunchKernelGGL(first_hit_albedo, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const int*>(hits), mats, n_flat, out, px);
    return hipGetLastError();
}

hipError_t launch_filter(const FilterArgs& d, hipStream_t stream) {
    const size_t px = (size_t)d.width * (size_t)d.height;
    float4* half[2] = {d.workspace, d.workspace + px};
    const size_t ptx = ((size_t)d.width + 63) / 64, pty = ((size_t)d.height + 3) / 4;
    const bool variance = d.kind == kFilterVariance;
    if (variance && d.only_pass < 0) {
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
    if (variance && d.stage == 0) return hipSuccess;   // option variance_stage 0: the estimate alone (timing)
    // pass i writes half i & 1, or, behind the estimate (which wrote half 0), the other one; it reads the half
    // the pass before it wrote
    const int first = variance ? 1 : 0;
    for (int i = 0; i < d.iterations; ++i) {
        if (d.only_pass >= 0 && i != d.only_pass) continue;
        PassArgs a;
        a.W = d.width; a.H = d.height; a.step = 1 << i;
        a.in = half[(i + first + 1) & 1];
        if (i == 0 && !variance) a.in = d.kind == kFilterHistory ? d.hist : nullptr;
        a.side = variance ? reinterpret_cast<const float*>(d.hist) : (i == 0 ? d.radiance : nullptr);
        a.hits = d.hits;
        const bool last = i == d.iterations - 1;
        a.out_c = last ? nullptr : half[(i + first) & 1];
        a.out_rgba = last ? d.out_rgba : nullptr;
        a.out_rad = last ? d.out_rad : nullptr;
        a.kd = d.sigma_depth;
        a.tol = variance ? d.tolerance : d.tolerance * (float)a.step;
        a.npow = d.normal_power_log2;
        a.left = d.iterations - i;
        // tiles of a residue class: ceil(ceil(W / step) / 32) x ceil(ceil(H / step) / 8), for step^2 classes
        const size_t cw = ((size_t)d.width + a.step - 1) / a.step, ch = ((size_t)d.height + a.step - 1) / a.step;
        const size_t ttx = (cw + kTileX - 1) / kTileX, tty = (ch + kTileY - 1) / kTileY;
        const size_t tiled_blocks = ttx * tty * (size_t)a.step * (size_t)a.step;
        bool tiled = d.form == 2 || (d.form == 0 && kTiledByStep[d.kind][i]);
        if (variance && i > 0) tiled = false;                        // its 3x3 window leaves a class's tile
        if (tiled_blocks > 0x7FFFFFFFull) tiled = false;             // past a 1-D grid: the plain form
        if (d.albedo && (i == 0 || last)) {                          // (kind Radiance: its table, its forms)
            AlbedoPassArgs b;
            static_cast<PassArgs&>(b) = a;
            b.albedo = d.albedo;
            if (tiled)
                hipLaunchKernelGGL(kAlbedoTiled[last][i == 0], dim3((unsigned)tiled_blocks), dim3(256), 0, stream, b,
                                   (int)ttx);
            else
                hipLaunchKernelGGL(kAlbedoPlain[last][i == 0], dim3((unsigned)(ptx * pty)), dim3(256), 0, stream, b,
                                   (int)ptx);
        } else if (tiled)
            hipLaunchKernelGGL(kTiled[d.kind], dim3((unsigned)tiled_blocks), dim3(256), 0, stream, a, (int)ttx);
        else
            hipLaunchKernelGGL(kPlain[d.kind], dim3((unsigned)(ptx * pty)), dim3(256), 0, stream, a, (int)ptx);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
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

void rt_variance_default_params(rt_variance_params* out) {
    if (!out) return;
    out->iterations = 4;
    out->normal_power_log2 = 7;
    out->sigma_depth = 0.005f;
    out->sigma_lum = 1.0f;
    out->min_history = 4;
    out->reserved[0] = out->reserved[1] = out->reserved[2] = 0;
}

size_t rt_denoise_workspace_bytes(int width, int height) {
    if (width < 1 || height < 1 || (int64_t)width * (int64_t)height > (int64_t)1 << 31) return 0;
    return (size_t)2 * (size_t)width * (size_t)height * 16;
}

}  // extern "C"
