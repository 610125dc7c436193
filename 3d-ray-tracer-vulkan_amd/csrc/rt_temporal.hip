// rt_temporal.hip — temporal accumulation reprojected through the first-hit
// buffer (rtamd.h "temporal").
//
// One kernel template.  A pixel with a hit projects its world position through
// the current and the previous camera, follows the difference to where the
// surface was in the previous frame, gathers the up to four history records
// around that point whose own first hits lie on the same plane with the same
// normal, and blends the new sample into their bilinear mean with weight 1 / n.
// A pixel without a hit, or one whose history is rejected, starts again from
// its own sample.  All arithmetic is IEEE binary32 in the order DESIGN.md §4h
// writes it (the library is built with -ffp-contract=off, `/` and sqrtf are
// correctly rounded, fminf drops a NaN operand), so tests/temporal_ref.py
// restates it bit for bit.
//
// With MOMENTS (rt_temporal_moments_device) a second history
// buffer travels beside the first: (m1, m2), the accumulated means of the
// samples' luminance and of its square, gathered through the same taps with the
// same weights.  The colour's operations are the same in the same order: the
// same history, radiance and RGBA8 bits.  A tap costs 8 B more, a pixel writes
// 8 B more.
//
// With MOTION (rt_temporal_motion_device) the triangles may have
// moved between the two frames: the pixel's triangle is read from the current
// and from the previous vertex records, the hit point is expressed in the
// barycentric coordinates of the one and evaluated on the other (binary64, in
// §4m's order), and that point and the previous normal stand in for the
// pixel's own on the previous-frame side: the projection through the previous
// camera and the taps' two tests.  A triangle whose nine coordinates are the
// same bits in both is the static contract exactly; a triangle index outside
// the records or a result that is not finite starts the pixel over.  The
// instantiations without MOTION do not read the extra kernel argument.
//
// A memory-bound gather: a pixel reads its own 12 + 32 B, each tap 48 B (the
// two 16-B halves of the previous hit record and one 16-B history record), and
// writes 16 + 12 + 4 B.  The four taps' twelve loads are issued together from
// clamped addresses and their contributions predicated, so no load waits for a
// branch.  Two lane mappings of the same 64 x 4-pixel workgroup:
//   rows  : a wave on 64 consecutive pixels of one row
//   tiles : a wave on a 16 x 4 tile (the render's wave tile on the accel tree)
// Which one ships was measured (kShippedForm below).
#include "rt_internal.h"
#include "rt_pixel.h"

namespace rtamd {
namespace {

// project(C, P) of DESIGN.md §4h: the viewport coordinates whose ray from C's origin passes through P
__device__ __forceinline__ bool project(const TemporalBasis& c, float px, float py, float pz, float& u, float& v) {
    const float wx = px - c.ox, wy = py - c.oy, wz = pz - c.oz;
    const float dn = dot3(wx, wy, wz, c.nx, c.ny, c.nz);
    u = dot3(wx, wy, wz, c.ax, c.ay, c.az) / dn;
    v = dot3(wx, wy, wz, c.bx, c.by, c.bz) / dn;
    return dn * c.det > 0.0f;
}

// §4m's dot and cross in binary64 (the library is built with -ffp-contract=off: one rounding per operation)
__device__ __forceinline__ double dot3d(double ax, double ay, double az, double bx, double by, double bz) {
    return (ax * bx + ay * by) + az * bz;
}

// The previous-frame side of a pixel across a geometry update (MOTION): its hit point q in the
// barycentric coordinates of its triangle as the current record c holds it, evaluated on the previous record
// v; the previous normal on the side the current one faces.  False when a component is not finite.
__device__ __forceinline__ bool previous_point(const float4 (&c)[3], const float4 (&v)[3], float qx, float qy, float qz,
                                               float nx, float ny, float nz, float (&P)[3], float (&N)[3]) {
    const float e1x = c[1].x - c[0].x, e1y = c[1].y - c[0].y, e1z = c[1].z - c[0].z;
    const float e2x = c[2].x - c[0].x, e2y = c[2].y - c[0].y, e2z = c[2].z - c[0].z;
    const float f1x = v[1].x - v[0].x, f1y = v[1].y - v[0].y, f1z = v[1].z - v[0].z;
    const float f2x = v[2].x - v[0].x, f2y = v[2].y - v[0].y, f2z = v[2].z - v[0].z;
    const double wx = (double)qx - (double)c[0].x, wy = (double)qy - (double)c[0].y, wz = (double)qz - (double)c[0].z;
    const double d11 = dot3d(e1x, e1y, e1z, e1x, e1y, e1z), d12 = dot3d(e1x, e1y, e1z, e2x, e2y, e2z),
                 d22 = dot3d(e2x, e2y, e2z, e2x, e2y, e2z);
    const double w1 = dot3d(wx, wy, wz, e1x, e1y, e1z), w2 = dot3d(wx, wy, wz, e2x, e2y, e2z);
    const double den = d11 * d22 - d12 * d12;
    const double b1 = (d22 * w1 - d12 * w2) / den, b2 = (d11 * w2 - d12 * w1) / den;
    P[0] = (float)(((double)v[0].x + b1 * (double)f1x) + b2 * (double)f2x);
    P[1] = (float)(((double)v[0].y + b1 * (double)f1y) + b2 * (double)f2y);
    P[2] = (float)(((double)v[0].z + b1 * (double)f1z) + b2 * (double)f2z);
    const double mx = (double)e1y * (double)e2z - (double)e1z * (double)e2y,
                 my = (double)e1z * (double)e2x - (double)e1x * (double)e2z,
                 mz = (double)e1x * (double)e2y - (double)e1y * (double)e2x;
    const double px = (double)f1y * (double)f2z - (double)f1z * (double)f2y,
                 py = (double)f1z * (double)f2x - (double)f1x * (double)f2z,
                 pz = (double)f1x * (double)f2y - (double)f1y * (double)f2x;
    const double s = dot3d(mx, my, mz, nx, ny, nz) < 0.0 ? -1.0 : 1.0;
    const double len = __builtin_sqrt(dot3d(px, py, pz, px, py, pz));
    N[0] = (float)((px / len) * s);
    N[1] = (float)((py / len) * s);
    N[2] = (float)((pz / len) * s);
    const auto finite = [](float f) { return __builtin_fabsf(f) < __builtin_inff(); };      // (a NaN fails)
    return finite(P[0]) && finite(P[1]) && finite(P[2]) && finite(N[0]) && finite(N[1]) && finite(N[2]);
}

template <bool TILES, bool MOMENTS, bool MOTION>
__global__ __launch_bounds__(256) void temporal_kernel(TemporalArgs a, int tiles_x, TemporalMotion mv) {
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
    const float l = lum_of(cr, cg, cb), l2 = l * l;              // (MOMENTS alone reads them)
    const bool hit = __float_as_int(p0.y) >= 0;
    // MOTION: the pixel's triangle in the current and the previous vertex records, from an index inside the
    // buffers either way; lanes on one triangle share the six loads
    float4 vc[3], vq[3];
    bool known = true;                                           // tri < n_tris
    if constexpr (MOTION) {
        known = (unsigned)__float_as_int(p0.y) < mv.n_tris;
        const size_t t3 = known ? 3 * (size_t)(unsigned)__float_as_int(p0.y) : 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            vc[k] = mv.verts_cur[t3 + k];
            vq[k] = mv.verts_prev[t3 + k];
        }
    }
    float orr = cr, og = cg, ob = cb, on = hit ? 1.0f : 0.0f;      // sky / invalid: passes through with n = 0
    float o1 = l, o2 = l2;
    if (hit && a.hist_prev) {
        float nx = p0.z, ny = p0.w, nz = p1.x, qx = p1.y, qy = p1.z, qz = p1.w;
        float uc, vc_, up, vp;
        const bool fc = project(a.cur, qx, qy, qz, uc, vc_);
        if constexpr (MOTION) {
            // an unmoved triangle (the nine floats bit for bit) is §4h exactly: P' and n' are selected, the
            // taps below are loaded by every lane alike
            bool moved = false;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                moved = moved || __float_as_int(vc[k].x) != __float_as_int(vq[k].x) ||
                        __float_as_int(vc[k].y) != __float_as_int(vq[k].y) ||
                        __float_as_int(vc[k].z) != __float_as_int(vq[k].z);
            if (moved) {
                float P[3], N[3];
                const bool fin = previous_point(vc, vq, qx, qy, qz, nx, ny, nz, P, N);
                known = known && fin;
                qx = P[0]; qy = P[1]; qz = P[2];
                nx = N[0]; ny = N[1]; nz = N[2];
            }
        }
        const bool fp = project(a.prev, qx, qy, qz, up, vp);
        const float fW = (float)W, fH = (float)H;
        const float fx = (float)x + (up - uc) * fW, fy = (float)y + (vc_ - vp) * fH;
        if (known && fc && fp && fx > -1.0f && fx < fW && fy > -1.0f && fy < fH) {      // (a NaN fails)
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
                if constexpr (MOMENTS) hm[k] = a.mom_prev[q];
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
                if constexpr (MOMENTS) {
                    s1 = take ? s1 + wt * hm[k].x : s1;
                    s2 = take ? s2 + wt * hm[k].y : s2;
                }
            }
            if (ws > 0.0f) {
                const float hr = sr / ws, hg = sg / ws, hb = sb / ws;
                const float nn = __builtin_fminf(nm + 1.0f, a.max_history), inv = 1.0f / nn;
                orr = hr + (cr - hr) * inv;
                og = hg + (cg - hg) * inv;
                ob = hb + (cb - hb) * inv;
                on = nn;
                if constexpr (MOMENTS) {
                    const float h1m = s1 / ws, h2m = s2 / ws;
                    o1 = h1m + (l - h1m) * inv;
                    o2 = h2m + (l2 - h2m) * inv;
                }
            }
        }
    }
    a.hist_out[p] = make_float4(orr, og, ob, on);
    if constexpr (MOMENTS) a.mom_out[p] = make_float2(o1, o2);
    // rt_pixel.h's store_display, written out: through the call the compiler no longer shares 3 * p between
    // the radiance loads above and these stores, and the kernel's registers and instructions change
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

// The lane mapping option temporal_tile 0 takes: the faster one of
// tools/temporal_bench.py's times on config 3 at 1920x1080 (profiles/temporal,
// DESIGN.md §4h): rows 0.0364 ms [0.0364, 0.0365] against tiles 0.0371
// [0.0370, 0.0372], with the camera orbiting 1 degree per frame.
constexpr int kShippedForm = 1;

}  // namespace

hipError_t launch_temporal(const TemporalArgs& t, hipStream_t stream, const TemporalMotion* motion) {
    const size_t tx = ((size_t)t.width + 63) / 64, ty = ((size_t)t.height + 3) / 4;   // <= 2^29 workgroups
    const bool tiles = (t.form ? t.form : kShippedForm) == 2;
    // MOTION only with vertex buffers (rt_temporal_motion_device): without them the kernels of §4h and §4j
    const auto kernel =
        motion ? (t.mom_out ? (tiles ? temporal_kernel<true, true, true> : temporal_kernel<false, true, true>)
                                 : (tiles ? temporal_kernel<true, false, true> : temporal_kernel<false, false, true>))
                    : (t.mom_out ? (tiles ? temporal_kernel<true, true, false> : temporal_kernel<false, true, false>)
                                 : (tiles ? temporal_kernel<true, false, false> : temporal_kernel<false, false, false>));
    hipLaunchKernelGGL(kernel, dim3((unsigned)(tx * ty)), dim3(256), 0, stream, t, (int)tx,
                       motion ? *motion : TemporalMotion{});
    return hipGetLastError();
}

}  // namespace rtamd

extern "C" {

void rt_temporal_default_params(rt_temporal_params* out) {
    if (!out) return;
    out->max_history = 32;
    out->plane_tol = 0.005f;
    out->normal_min = 0.9f;
    out->reserved = 0;
}

int rt_temporal_camera_basis(const rt_camera_ubo* cam, float out[13]) {
    if (!cam || !out) {
        rtamd::set_error("rt_temporal_camera_basis: null camera or output");
        return RT_ERR_INVALID_ARG;
    }
    const float* o = cam->origin;
    const float* h = cam->horizontal;
    const float* v = cam->vertical;
    const float a[3] = {cam->lower_left[0] - o[0], cam->lower_left[1] - o[1], cam->lower_left[2] - o[2]};
    const auto cross = [](const float* p, const float* q, float* r) {
        r[0] = p[1] * q[2] - p[2] * q[1];
        r[1] = p[2] * q[0] - p[0] * q[2];
        r[2] = p[0] * q[1] - p[1] * q[0];
    };
    out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
    cross(h, v, out + 3);       // N
    cross(v, a, out + 6);       // A
    cross(a, h, out + 9);       // B
    out[12] = (a[0] * out[3] + a[1] * out[4]) + a[2] * out[5];
    return RT_OK;
}

}  // extern "C"
