// rt_refit.hip — the device side of rt_update_geometry (rtamd.h "refit",
// DESIGN.md §4l): the scene's records recomputed in place from moved vertices.
//
// The host stages the raw vertex records (48 B per flattened triangle) and the
// node boxes (24 B per node); everything else is computed here, with the
// host's operations in the host's order.  The library is built with
// -ffp-contract=off and `/`, sqrtf and the double sqrt and division are
// correctly rounded, so the bits are the ones build_host_scene and the
// walk-record loop of scene_plan.cpp and accel_build write for the same buffers.
//
// Three stages on one stream, each a plain grid of independent lanes:
//   refit_reference : a lane per reference node (and per flattened triangle,
//                     for its shading normal): nodes / leafs / pairs / walk of
//                     a scene on the reference's tree, walk_ref beside accel
//                     records.  Links, pad bits and pad slots are never
//                     written.
//   refit_leaves    : a lane per kept primitive of the accel tree: its 64-B
//                     leaf into every layout, its box and force bit into the
//                     canonical array (2 float4 per tree node).
//   refit_level     : one launch per height of the accel tree, lowest first:
//                     a lane per node of that height reads both children from
//                     the canonical array, writes the union and the OR-ed
//                     force bit there and into the node's slot of every
//                     layout.
// No lane waits for another: a level's inputs were written by earlier
// launches of the same stream.  min and max are order-free, so the result
// does not depend on scheduling.  Bandwidth bound; no LDS, no atomics.
//
// rt_update_geometry_device fills the two staging arrays on
// the device instead, from input triangles in device memory: the refit_in_*
// kernels further down (a check that only reads, with an atomicMin per
// offender; the records; the leaf boxes in double; one launch per level of the
// reference's tree), in front of the same three stages.
#include "rt_internal.h"

#include "accel_build.h"

namespace rtamd {
namespace {

struct Tri { float v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z; };

// e1 = v1 - v0, e2 = v2 - v0 as hit_triangle computes them (compute_dynamic_ray.comp:106-107)
__device__ __forceinline__ Tri load_tri(const float4* st_verts, int tri) {
    const float4 a = st_verts[3 * (size_t)tri], b = st_verts[3 * (size_t)tri + 1], c = st_verts[3 * (size_t)tri + 2];
    return {a.x, a.y, a.z, b.x - a.x, b.y - a.y, b.z - a.z, c.x - a.x, c.y - a.y, c.z - a.z};
}

__device__ __forceinline__ unsigned bits(float f) { return __float_as_uint(f); }
__device__ __forceinline__ float from_bits(unsigned u) { return __uint_as_float(u); }

// accel_class(e1, e2) >= kAccelClassMin (accel_build.cpp), in double as there:
// floor(-log2 s) >= 7 exactly when s <= 2^-7, decided by comparison (a device
// log2 does not round as the host's does); a zero edge or parallel edges give
// s = NaN or 0: class 31.
__device__ __forceinline__ bool thin(const Tri& t) {
    const double a[3] = {t.e1x, t.e1y, t.e1z}, b[3] = {t.e2x, t.e2y, t.e2z};
    const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const double s = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) /
                     (sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) * sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]));
    return !(s > 0.0) || s <= 0.0078125;
}

__global__ __launch_bounds__(256) void refit_reference(RefitArgs r) {
    const int g = (int)(blockIdx.x * 256u + threadIdx.x);
    const RefitTables& t = r.t;
    if (g < t.n_tris) {
        // normalize(cross(e1, e2)) in build_host_scene's order
        const Tri q = load_tri(t.st_verts, g);
        const float cx = q.e1y * q.e2z - q.e1z * q.e2y;
        const float cy = q.e1z * q.e2x - q.e1x * q.e2z;
        const float cz = q.e1x * q.e2y - q.e1y * q.e2x;
        const float l = sqrtf((cx * cx + cy * cy) + cz * cz);
        r.scene.norms[kShadeStride * (size_t)g] = make_float4(cx / l, cy / l, cz / l, 0.f);
    }
    if (g >= t.n_ref) return;
    const float* bx = t.st_boxes + 6 * (size_t)g;
    const float lox = bx[0], loy = bx[1], loz = bx[2], hix = bx[3], hiy = bx[4], hiz = bx[5];
    const int info = t.ref_info[g];          // a leaf: its triangle; an internal node: -(right child + 1)
    const bool leaf = info >= 0;
    Tri q = {};
    if (leaf) q = load_tri(t.st_verts, info);
    float4* w = (r.scene.walk_ref ? r.scene.walk_ref : r.scene.walk) + 2 * (size_t)t.ref_slot[g];
    float4 A = w[0], B = w[1];
    A.x = lox; A.y = loy; A.z = loz;
    B.x = hix; B.y = hiy; B.z = hiz;
    if (leaf) B.w = q.v0x;
    w[0] = A;
    w[1] = B;
    if (leaf) {
        w[2] = make_float4(q.v0y, q.v0z, q.e1x, q.e1y);
        w[3] = make_float4(q.e1z, q.e2x, q.e2y, q.e2z);
    }
    if (r.scene.nodes) {
        float4* n = r.scene.nodes + 2 * (size_t)g;
        float4 N0 = n[0], N1 = n[1];
        N0.x = lox; N0.y = loy; N0.z = loz;
        N1.x = hix; N1.y = hiy; N1.z = hiz;
        n[0] = N0;
        n[1] = N1;
    }
    if (r.scene.leafs && leaf) {
        float4* l = r.scene.leafs + 3 * (size_t)g;
        l[0] = make_float4(q.v0x, q.v0y, q.v0z, l[0].w);
        l[1] = make_float4(q.e1x, q.e1y, q.e1z, 0.f);
        l[2] = make_float4(q.e2x, q.e2y, q.e2z, 0.f);
    }
    if (r.scene.pairs && !leaf) {
        const float* L = t.st_boxes + 6 * ((size_t)g + 1);
        const float* R = t.st_boxes + 6 * (size_t)(-(info + 1));
        float4* p = r.scene.pairs + 4 * (size_t)g;
        p[0] = make_float4(L[0], L[1], L[2], R[0]);
        p[1] = make_float4(L[3], L[4], L[5], R[1]);
        p[2] = make_float4(R[3], R[4], R[5], R[2]);
    }
}

__global__ __launch_bounds__(256) void refit_leaves(RefitArgs r) {
    const int p = (int)(blockIdx.x * 256u + threadIdx.x);
    const RefitTables& t = r.t;
    if (p >= t.n_prims) return;
    const int tri = t.prim[3 * (size_t)p], leaf = t.prim[3 * (size_t)p + 1], c = t.prim[3 * (size_t)p + 2];
    const Tri q = load_tri(t.st_verts, tri);
    const unsigned force = thin(q) ? kAccelForce : 0u;
    const float* bx = t.st_boxes + 6 * (size_t)leaf;
    const float lox = bx[0], loy = bx[1], loz = bx[2], hix = bx[3], hiy = bx[4], hiz = bx[5];
    t.canon[2 * (size_t)c] = make_float4(lox, loy, loz, from_bits(force));
    t.canon[2 * (size_t)c + 1] = make_float4(hix, hiy, hiz, 0.f);
    for (int o = 0; o < t.n_layouts; ++o) {
        float4* w = r.scene.walk + 2 * (size_t)t.slot[(size_t)o * t.n_canon + c];
        const unsigned w3 = (bits(w[0].w) & ~kAccelForce) | force;
        w[0] = make_float4(lox, loy, loz, from_bits(w3));
        w[1] = make_float4(hix, hiy, hiz, q.v0x);
        w[2] = make_float4(q.v0y, q.v0z, q.e1x, q.e1y);
        w[3] = make_float4(q.e1z, q.e2x, q.e2y, q.e2z);
    }
}

// std::min / std::max as accel_build's Builder applies them: the first operand on a tie
__device__ __forceinline__ float umin(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float umax(float a, float b) { return a < b ? b : a; }

__global__ __launch_bounds__(256) void refit_level(RefitArgs r, int first, int count) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    const RefitTables& t = r.t;
    if (i >= count) return;
    const int c = t.by_height[first + i];
    const int L = t.child[2 * (size_t)c], R = t.child[2 * (size_t)c + 1];
    const float4 la = t.canon[2 * (size_t)L], lb = t.canon[2 * (size_t)L + 1];
    const float4 ra = t.canon[2 * (size_t)R], rb = t.canon[2 * (size_t)R + 1];
    const unsigned force = (bits(la.w) | bits(ra.w)) & kAccelForce;
    const float lox = umin(la.x, ra.x), loy = umin(la.y, ra.y), loz = umin(la.z, ra.z);
    const float hix = umax(lb.x, rb.x), hiy = umax(lb.y, rb.y), hiz = umax(lb.z, rb.z);
    t.canon[2 * (size_t)c] = make_float4(lox, loy, loz, from_bits(force));
    t.canon[2 * (size_t)c + 1] = make_float4(hix, hiy, hiz, 0.f);
    for (int o = 0; o < t.n_layouts; ++o) {
        float4* w = r.scene.walk + 2 * (size_t)t.slot[(size_t)o * t.n_canon + c];
        float4 A = w[0], B = w[1];
        A.x = lox; A.y = loy; A.z = loz;
        A.w = from_bits((bits(A.w) & ~kAccelForce) | force);
        B.x = hix; B.y = hiy; B.z = hiz;      // word 7, L(first child) << 31, stays
        w[0] = A;
        w[1] = B;
    }
}

// ------------------------------------------------------------------------------------------------
// rt_update_geometry_device: rt_refit_scene (scene_build.cpp) restated here, operation
// for operation in double, so that st_verts and st_boxes hold the bytes the host path stages.
//   refit_in_check  : reads the input only.  A lane per flattened triangle: its source entry and the
//                     nine float casts; the first lanes also take a (dropped, kept) pair each.  The
//                     lowest offender of each kind goes into a status word (a vector-memory atomicMin).
//   refit_in_stage  : a lane per flattened triangle: its 48-B record.
//   refit_in_leaves : a lane per reference leaf: Triangle.calculateBoundingBox in double, cast once.
//   refit_in_level  : one launch per height: a lane per node, the union of its children's boxes.
// The union is taken of the children's float boxes: rounding to float is monotone, so the cast of the
// smaller double is the smaller (or an equal) float, and Math.min / Math.max pick -0.0 / +0.0 among
// zeros by sign alone, which the cast keeps (a double too small for a float becomes a zero of its sign).
// So min(cast a, cast b) has the bytes of cast(min(a, b)), and no double boxes are kept.

// java.lang.Math.min / max (scene_build.cpp jmin / jmax): NaN wins, -0.0 < +0.0
__device__ __forceinline__ double jmin(double a, double b) {
    if (a != a) return a;
    if (a == 0.0 && b == 0.0) return __double_as_longlong(a) < 0 ? a : b;
    return a <= b ? a : b;
}
__device__ __forceinline__ double jmax(double a, double b) {
    if (a != a) return a;
    if (a == 0.0 && b == 0.0) return __double_as_longlong(a) < 0 ? b : a;
    return a >= b ? a : b;
}
__device__ __forceinline__ float jminf(float a, float b) {
    if (a != a) return a;
    if (a == 0.f && b == 0.f) return (int)bits(a) < 0 ? a : b;
    return a <= b ? a : b;
}
__device__ __forceinline__ float jmaxf(float a, float b) {
    if (a != a) return a;
    if (a == 0.f && b == 0.f) return (int)bits(a) < 0 ? b : a;
    return a >= b ? a : b;
}

template <bool F32>
__device__ __forceinline__ void load_in(const RefitFront& f, size_t tri, double v[9]) {
    for (int k = 0; k < 9; ++k)
        v[k] = F32 ? (double)static_cast<const float*>(f.in)[9 * tri + k] : static_cast<const double*>(f.in)[9 * tri + k];
}

struct BoxF { float lo[3], hi[3]; };

// tri_box (scene_build.cpp) of 9 doubles, cast as write_node casts it
__device__ __forceinline__ BoxF tri_box(const double v[9]) {
    const double eps = 0.0001;                 // Triangle.java:65
    double mn[3], mx[3];
    for (int k = 0; k < 3; ++k) {
        mn[k] = jmin(v[k], jmin(v[3 + k], v[6 + k]));
        mx[k] = jmax(v[k], jmax(v[3 + k], v[6 + k]));
    }
    // each add touches all three components (x + 0.0 turns -0.0 into +0.0)
    for (int k = 0; k < 3; ++k)
        if (mx[k] - mn[k] < eps)
            for (int j = 0; j < 3; ++j) mx[j] = mx[j] + (j == k ? eps : 0.0);
    BoxF b;
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = (float)mn[k];
        b.hi[k] = (float)mx[k];
    }
    return b;
}

__device__ __forceinline__ bool finite_bits(float x) { return (bits(x) & 0x7F800000u) != 0x7F800000u; }

template <bool F32>
__global__ __launch_bounds__(256) void refit_in_check(RefitFront f) {
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (g < (unsigned)f.n_flat) {
        const size_t src = f.source ? f.source[g] : g;
        if (src >= f.n_in) {
            atomicMin(f.status + 0, g);
        } else {
            double v[9];
            load_in<F32>(f, src, v);
            bool ok = true;
            for (int k = 0; k < 9; ++k) ok = ok && finite_bits((float)v[k]);
            if (!ok) atomicMin(f.status + 1, g);
        }
    }
    if (g < (unsigned)f.n_dups) {
        const unsigned dropped = (unsigned)f.dups[4 * (size_t)g], kept = (unsigned)f.dups[4 * (size_t)g + 2];
        const size_t sa = f.source ? f.source[dropped] : dropped, sb = f.source ? f.source[kept] : kept;
        if (sa >= f.n_in || sb >= f.n_in) return;          // status[0] has it: both are flattened triangles
        double a[9], b[9];
        load_in<F32>(f, sa, a);
        load_in<F32>(f, sb, b);
        bool same = true;
        for (int k = 0; k < 9; ++k) same = same && bits((float)a[k]) == bits((float)b[k]);
        const BoxF ba = tri_box(a), bb = tri_box(b);
        for (int k = 0; k < 3; ++k) same = same && bits(ba.lo[k]) == bits(bb.lo[k]) && bits(ba.hi[k]) == bits(bb.hi[k]);
        if (!same) atomicMin(f.status + 2, dropped);
    }
}

template <bool F32>
__global__ __launch_bounds__(256) void refit_in_stage(RefitFront f) {
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (g >= (unsigned)f.n_flat) return;
    double v[9];
    load_in<F32>(f, f.source ? f.source[g] : g, v);
    float4* o = f.st_verts + 3 * (size_t)g;
    o[0] = make_float4((float)v[0], (float)v[1], (float)v[2], 0.0f);
    o[1] = make_float4((float)v[3], (float)v[4], (float)v[5], 0.0f);
    o[2] = make_float4((float)v[6], (float)v[7], (float)v[8], 0.0f);
}

template <bool F32>
__global__ __launch_bounds__(256) void refit_in_leaves(RefitFront f, int count) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= count) return;
    const int node = f.by_height[i];
    const unsigned tri = (unsigned)f.ref_info[node];       // a leaf: its flattened triangle
    double v[9];
    load_in<F32>(f, f.source ? f.source[tri] : tri, v);
    const BoxF b = tri_box(v);
    float* o = f.st_boxes + 6 * (size_t)node;
    for (int k = 0; k < 3; ++k) {
        o[k] = b.lo[k];
        o[3 + k] = b.hi[k];
    }
}

__global__ __launch_bounds__(256) void refit_in_level(RefitFront f, int first, int count) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= count) return;
    const int node = f.by_height[first + i];
    const float* L = f.st_boxes + 6 * ((size_t)node + 1);                      // AABB.surroundingBox(left, right)
    const float* R = f.st_boxes + 6 * (size_t)(-(f.ref_info[node] + 1));
    float* o = f.st_boxes + 6 * (size_t)node;
    for (int k = 0; k < 3; ++k) {
        o[k] = jminf(L[k], R[k]);
        o[3 + k] = jmaxf(L[3 + k], R[3 + k]);
    }
}

}  // namespace

hipError_t launch_refit_check(const RefitFront& f, hipStream_t stream) {
    const int n = f.n_flat > f.n_dups ? f.n_flat : f.n_dups;
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (f.f32) hipLaunchKernelGGL(refit_in_check<true>, grid, block, 0, stream, f);
    else hipLaunchKernelGGL(refit_in_check<false>, grid, block, 0, stream, f);
    return hipGetLastError();
}

hipError_t launch_refit_front(const RefitFront& f, const int* level_first, int n_levels, hipStream_t stream) {
    const dim3 block(256);
    if (f.n_flat > 0) {
        const dim3 grid((unsigned)((f.n_flat + 255) / 256));
        if (f.f32) hipLaunchKernelGGL(refit_in_stage<true>, grid, block, 0, stream, f);
        else hipLaunchKernelGGL(refit_in_stage<false>, grid, block, 0, stream, f);
    }
    for (int h = 0; h < n_levels; ++h) {
        const int first = level_first[h], count = level_first[h + 1] - first;
        if (count <= 0) continue;
        const dim3 grid((unsigned)((count + 255) / 256));
        if (h > 0) hipLaunchKernelGGL(refit_in_level, grid, block, 0, stream, f, first, count);
        else if (f.f32) hipLaunchKernelGGL(refit_in_leaves<true>, grid, block, 0, stream, f, count);
        else hipLaunchKernelGGL(refit_in_leaves<false>, grid, block, 0, stream, f, count);
    }
    return hipGetLastError();
}

hipError_t launch_refit(const RefitArgs& r, const int* level_first, int n_levels, hipStream_t stream) {
    const RefitTables& t = r.t;
    const int n = t.n_ref > t.n_tris ? t.n_ref : t.n_tris;
    if (n > 0) hipLaunchKernelGGL(refit_reference, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, r);
    if (t.n_prims > 0) {
        hipLaunchKernelGGL(refit_leaves, dim3((unsigned)((t.n_prims + 255) / 256)), dim3(256), 0, stream, r);
        for (int h = 0; h < n_levels; ++h) {
            const int first = level_first[h], count = level_first[h + 1] - first;
            if (count > 0)
                hipLaunchKernelGGL(refit_level, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, r, first,
                                   count);
        }
    }
    return hipGetLastError();
}

}  // namespace rtamd
