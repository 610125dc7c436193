/*
 * rt_accel_model.c — TEST INFRASTRUCTURE ONLY: a CPU model of option
 * "accel"'s walk, built as liboracle_accel.so.  The product
 * never loads it; tests/ and tools/accel_study.py use it as the checker of the
 * accel kernel's work counters and to study how far the accel walk's frames
 * lie from the reference-order oracle (liboracle.so).
 *
 * It is the oracle (rt_oracle.c) with the reference's stack DFS
 * (compute_dynamic_ray.comp:185-210) replaced, through ORC_WALK_HOOK, by the
 * walk the accel kernel runs over the records rt_accel_records returns
 * (3d-ray-tracer-vulkan_amd/csrc/accel_build.h): a ray walks the layout of its
 * direction's octant, slot by slot, next = leaf ? n+2 : (hit ? n+1 : skip),
 * with two rules in place of the reference's compares:
 *   box entered    iff t_exit > t_enter && t_exit > T_MIN &&
 *                  t_enter <= closest_t * (1 + 2^-10) + 2^-10
 *   triangle taken iff t > T_MIN && (t < closest_t || (t == closest_t &&
 *                  flattened index < the current hit's))
 * and one fallback: a segment whose hit lies before its own box's t_enter
 * (t < the leaf's t_enter: rounding on the box face) is walked again with the
 * reference's DFS, counting both walks.  Everything else (camera, scatter,
 * sky, the counters' definitions) is the oracle's own code.  Node visits are
 * box tests (slots walked), as in the reference's counts: 1 + 2 x the internal
 * nodes whose box is entered.
 *
 * orc_accel_format(1): the records are accel_build.h's format 1 (option
 * accel_half): 16-B slots, an internal node one slot with its box in IEEE half
 * precision (decoded exactly, as the kernel's v_cvt_f32_f16), a leaf four.
 *
 * Format 0's walk starts inside the root (round 6; orc_accel_root): the root's
 * box is not tested, the root counts as visited and its children are walked.
 *
 * Thin triangles (round 6, accel_build.h accel_class / kAccelForce): a record
 * whose bit 29 of word 3 is set (its subtree holds a triangle of shape class
 * >= 7) is entered whenever its slab test passes (R = infinity); format 1's
 * internal nodes take orc_accel_relax_half's one factor, and its thin leaves
 * (bit 29) R = infinity too.
 */
#define ORC_WALK_HOOK accel_walk
#include "rt_oracle.c"

static const uint32_t* g_rec = NULL;   /* 8 words per slot (format 1: 4) */
static int g_fmt = 0;
static int g_layouts = 1, g_slots = 0, g_root_leaf = 0;
static uint64_t g_fallbacks = 0;       /* segments re-walked in the reference's order */
static uint64_t g_leaf_visits = 0;     /* analysis: leaf slots walked (the rest are internal nodes) */
/* The walk's box margin: a box is entered when t_enter <= closest_t * RELAX +
 * RELAX_ABS (accel_build.h).  orc_accel_margin changes them for studies. */
static float g_relax = 1.0f + 1.0f / 1024.0f, g_relax_abs = 1.0f / 1024.0f;
static float g_relax_half = 1.0f + 1.0f / 1024.0f;
static int g_root_enter = 1;           /* format 0: the walk starts inside the root */
static int g_oct_mask = 7;             /* a study: rays walk layout (octant & mask) */

int orc_accel_octants(int mask) {
    g_oct_mask = mask & 7;
    return 0;
}

/* Format 0's root entry (1, what the kernel does: its slab test skipped; 0:
 * tested first, as the kernel did before round 6). */
int orc_accel_root(int on) {
    g_root_enter = on < 0 ? 0 : on;
    return 0;
}

int orc_accel_margin(float rel, float abs_) {
    g_relax = rel;
    g_relax_abs = abs_;
    return 0;
}

/* Format 1: the margin factor of every internal node (accel_relax of the
 * tree's largest shape class, AccelHost::relax_max). */
int orc_accel_relax_half(float r) {
    g_relax_half = r;
    return 0;
}

/* The margin factor of a record (word 3: aw). */
static float rec_factor(int leaf, uint32_t aw) {
    if (leaf || !g_fmt) return (aw & (1u << 29)) ? INFINITY : g_relax;
    return g_relax_half;
}

/* accel_build.cpp accel_class / accel_relax, restated (the audit's margin). */
static int shape_class(vec3 e1, vec3 e2) {
    const double a[3] = {e1.x, e1.y, e1.z}, b[3] = {e2.x, e2.y, e2.z};
    const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const double sn = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) /
                      (sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) * sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]));
    if (!(sn > 0.0)) return 31;
    const int k = (int)floor(-log2(sn));
    return k < 0 ? 0 : (k > 31 ? 31 : k);
}
static float class_relax(int cls) { return cls < 7 ? 1.0f + 1.0f / 1024.0f : 1.0f + ldexpf(1.0f, cls - 16); }

/* Segments re-walked in the reference's order since the last call (resets). */
uint64_t orc_accel_fallbacks(void) {
    const uint64_t f = g_fallbacks;
    g_fallbacks = 0;
    return f;
}

/* Leaf slots walked since the last call (resets); an analysis aid. */
uint64_t orc_accel_leaf_visits(void) {
    const uint64_t f = g_leaf_visits;
    g_leaf_visits = 0;
    return f;
}

/* The format of the records the following renders walk: 0, 1 or 2. */
int orc_accel_format(int fmt) {
    if (fmt < 0 || fmt > 2) return -2;
    g_fmt = fmt;
    return 0;
}

/* Format 2's per-lane stack (entries; accel_build.h kWideStack) and the
 * segments whose stack overflowed (walked again in the reference's order). */
static int g_stack_k = 12;
static uint64_t g_overflows = 0;
static int g_count_steps = 0;          /* analysis: node_visits counts record fetches */
int orc_accel_stack(int k) {
    if (k < 1 || k > 64) return -2;
    g_stack_k = k;
    return 0;
}
uint64_t orc_accel_overflows(void) {
    const uint64_t f = g_overflows;
    g_overflows = 0;
    return f;
}
int orc_accel_count_steps(int on) {
    g_count_steps = on;
    return 0;
}

/* An IEEE half (bits h) as float, exactly. */
static float half_to_float(uint32_t h) {
    const uint32_t e = (h >> 10) & 31u, m = h & 1023u;
    float v;
    if (e == 0) v = ldexpf((float)m, -24);
    else if (e == 31) v = m ? NAN : INFINITY;
    else v = ldexpf((float)(1024u + m), (int)e - 25);
    return (h & 0x8000u) ? -v : v;
}

/* Sets the records the following renders walk (the caller keeps them alive). */
int orc_accel_set(const uint32_t* rec, int n_layouts, int slots, int root_leaf) {
    if ((n_layouts != 1 && n_layouts != 8) || slots < 0 || (slots > 0 && !rec)) return -2;
    g_rec = rec;
    g_layouts = n_layouts;
    g_slots = slots;
    g_root_leaf = root_leaf;
    return 0;
}

static float rec_f(size_t slot, int w) {
    float f;
    memcpy(&f, &g_rec[(g_fmt ? 4 : 8) * slot + (size_t)w], 4);
    return f;
}

/* Analysis (orc_accel_quant): internal boxes widened to what a compressed
 * record could hold, to count the visits that would cost; leaves stay exact.
 * 1 = IEEE half precision of each coordinate, rounded outward. */
static int g_quant = 0;
int orc_accel_quant(int mode) { const int o = g_quant; g_quant = mode; return o; }
static float half_down(float x) {           /* the largest half-precision value <= x, as float */
    if (x == 0.0f || !isfinite(x)) return x;
    int E;
    (void)frexpf(x, &E);                     /* |x| in [2^(E-1), 2^E) */
    const int e = E - 1 < -14 ? -14 : E - 1;
    const float ulp = ldexpf(1.0f, e - 10);
    const float r = floorf(x / ulp) * ulp;
    return r > 65504.0f ? 65504.0f : (r < -65504.0f ? -INFINITY : r);
}
static float half_up(float x) { return -half_down(-x); }

/* Audit (orc_accel_audit; tools/accel_adversarial.py, tests/test_accel_model.py).
 * Before each segment's walk, an exhaustive walk of the same layout enters
 * every box the ray's line crosses in front (the slab test without the
 * closest_t compare) and tests every triangle in them: i* = the lowest
 * (t, flattened index), te* = the t_enter of i*'s own leaf box.  The accel
 * walk returns the reference's hit whenever te* <= t* (1 + 2^-10) + 2^-10
 * (i*'s leaf and all its ancestors are entered; a t* before
 * te* takes the fallback).  The audit records, per segment with a hit, the
 * share of that margin i* consumes, headroom = (te* - t*) / (t* 2^-10 +
 * 2^-10): <= 0 for a hit inside its box, in (0, 1] where only the margin
 * keeps the box entered, > 1 where the argument fails (unsafe). */
static int g_audit = 0;
static double g_audit_max = -INFINITY;   /* against the default margin, 2^-10 */
static double g_audit_max_c = -INFINITY; /* against i*'s class margin (what the walk applies) */
static uint64_t g_audit_hits = 0, g_audit_incons = 0, g_audit_half = 0, g_audit_unsafe = 0;
static uint64_t g_audit_sliver = 0;         /* hits on i* with |det| <= 1e-4 (the 1e-5 cut's decade, :110) */
static double g_audit_sliver_max = -INFINITY;
/* max headroom of the hits binned by floor(-log2 x) (bin 31: x <= 2^-31):
 * x = sin of the triangle's angle at v0, |e1 x e2| / (|e1| |e2|) (the shape
 * Moeller-Trumbore's arithmetic is anchored at), and x = |cos| of the ray to
 * the triangle's normal, |det| / (|e1 x e2| |d|) (grazing) */
static double g_audit_shape[32], g_audit_graze[32];
static uint64_t g_audit_shape_n[32], g_audit_graze_n[32];

static int audit_bin(double x) {
    if (!(x > 0.0)) return 31;
    const int b = (int)floor(-log2(x));
    return b < 0 ? 0 : (b > 31 ? 31 : b);
}

/* the per-bin maxima (32 doubles each; -inf: no hit in the bin) and counts */
int orc_accel_audit_bins(double shape[32], double graze[32], uint64_t shape_n[32], uint64_t graze_n[32]) {
    for (int k = 0; k < 32; ++k) {
        shape[k] = g_audit_shape[k];
        graze[k] = g_audit_graze[k];
        shape_n[k] = g_audit_shape_n[k];
        graze_n[k] = g_audit_graze_n[k];
    }
    return 0;
}

int orc_accel_audit(int on) {
    g_audit = on;
    g_audit_max = g_audit_max_c = -INFINITY;
    g_audit_hits = g_audit_incons = g_audit_half = g_audit_unsafe = g_audit_sliver = 0;
    g_audit_sliver_max = -INFINITY;
    for (int k = 0; k < 32; ++k) {
        g_audit_shape[k] = g_audit_graze[k] = -INFINITY;
        g_audit_shape_n[k] = g_audit_graze_n[k] = 0;
    }
    return 0;
}

/* {segments with a hit, of them t* < te*, headroom > 0.5, unsafe (the
 * class margin test fails), max headroom (default margin), hits with |det| <=
 * 1e-4, their max headroom, max headroom against the class margin} since
 * orc_accel_audit. */
int orc_accel_audit_get(double out[8]) {
    out[0] = (double)g_audit_hits;
    out[1] = (double)g_audit_incons;
    out[2] = (double)g_audit_half;
    out[3] = (double)g_audit_unsafe;
    out[4] = g_audit_max;
    out[5] = (double)g_audit_sliver;
    out[6] = g_audit_sliver_max;
    out[7] = g_audit_max_c;
    return 0;
}

static void audit_segment(const scene* s, ray r) {
    const int oct = g_layouts == 8 ? ((signbit(r.dir.x) ? 1 : 0) | (signbit(r.dir.y) ? 2 : 0) |
                                      (signbit(r.dir.z) ? 4 : 0)) : 0;
    size_t n = (size_t)oct * (size_t)g_slots;
    const size_t end = n + (size_t)g_slots;
    const size_t WS = g_fmt ? 4 : 8;
    int leaf = g_root_leaf;
    const vec3 inv = v3(rcp(r.dir.x), rcp(r.dir.y), rcp(r.dir.z));
    float best_t = INFINITY, best_te = 0.0f;
    int best = -1;
    while (n < end) {
        const uint32_t aw = g_rec[WS * n + 3], bw = g_fmt ? 0u : g_rec[8 * n + 7];
        vec3 blo, bhi;
        if (g_fmt && !leaf) {
            const uint32_t* w = &g_rec[4 * n];
            blo = v3(half_to_float(w[0] & 0xFFFFu), half_to_float(w[0] >> 16), half_to_float(w[1] & 0xFFFFu));
            bhi = v3(half_to_float(w[1] >> 16), half_to_float(w[2] & 0xFFFFu), half_to_float(w[2] >> 16));
        } else {
            blo = v3(rec_f(n, 0), rec_f(n, 1), rec_f(n, 2));
            bhi = v3(rec_f(n, 4), rec_f(n, 5), rec_f(n, 6));
        }
        const vec3 t0s = mul3(sub3(blo, r.origin), inv);
        const vec3 t1s = mul3(sub3(bhi, r.origin), inv);
        const float te = fmaxf(fmaxf(fminf(t0s.x, t1s.x), fminf(t0s.y, t1s.y)), fminf(t0s.z, t1s.z));
        const float tx = fminf(fminf(fmaxf(t0s.x, t1s.x), fmaxf(t0s.y, t1s.y)), fmaxf(t0s.z, t1s.z));
        const int hb = tx > te && tx > T_MIN;
        if (hb && leaf) {
            const int tri = (int)(aw & 0x1FFFFFFFu);
            vec3 nrm;
            float t = INFINITY;
            if ((size_t)tri < s->n_tris &&
                hit_triangle(r, vertex_pos(s, (size_t)tri * 3 + 0), vertex_pos(s, (size_t)tri * 3 + 1),
                             vertex_pos(s, (size_t)tri * 3 + 2), &t, &nrm) &&
                (t < best_t || (t == best_t && tri < best))) {
                best_t = t;
                best = tri;
                best_te = te;
            }
        }
        if (leaf) {
            n += g_fmt ? 4 : 2;
            leaf = (int)(aw >> 31);
        } else if (hb) {
            n += 1;
            leaf = g_fmt ? (int)((aw >> 30) & 1u) : (int)(bw >> 31);
        } else {
            n = aw & (g_fmt ? 0x3FFFFFFFu : 0x1FFFFFFFu);
            leaf = (int)(aw >> 31);
        }
    }
    if (best < 0) return;
    const double room = (double)best_t * (1.0 / 1024.0) + 1.0 / 1024.0;
    const double head = ((double)best_te - (double)best_t) / room;
    const vec3 v0 = vertex_pos(s, (size_t)best * 3 + 0);
    /* the walk enters i*'s leaf and ancestors with at least i*'s class factor */
    const float rc = class_relax(shape_class(sub3(vertex_pos(s, (size_t)best * 3 + 1), v0),
                                             sub3(vertex_pos(s, (size_t)best * 3 + 2), v0)));
    const int unsafe = !(best_te <= best_t * rc + g_relax_abs);
    const double head_c = ((double)best_te - (double)best_t) / ((double)best_t * ((double)rc - 1.0) + 1.0 / 1024.0);
    const float det = dot3(sub3(vertex_pos(s, (size_t)best * 3 + 1), v0), cross3(r.dir, sub3(vertex_pos(s,
                           (size_t)best * 3 + 2), v0)));
    const int sliver = det >= -1e-4f && det <= 1e-4f;
    const vec3 e1 = sub3(vertex_pos(s, (size_t)best * 3 + 1), v0), e2 = sub3(vertex_pos(s, (size_t)best * 3 + 2), v0);
    const double cx = (double)e1.y * e2.z - (double)e1.z * e2.y, cy = (double)e1.z * e2.x - (double)e1.x * e2.z,
                 cz = (double)e1.x * e2.y - (double)e1.y * e2.x;
    const double cn = sqrt(cx * cx + cy * cy + cz * cz);
    const double l1 = sqrt((double)e1.x * e1.x + (double)e1.y * e1.y + (double)e1.z * e1.z);
    const double l2 = sqrt((double)e2.x * e2.x + (double)e2.y * e2.y + (double)e2.z * e2.z);
    const double ld = sqrt((double)r.dir.x * r.dir.x + (double)r.dir.y * r.dir.y + (double)r.dir.z * r.dir.z);
    const int bs = audit_bin(cn / (l1 * l2));
    const int bg = audit_bin(fabs(((double)r.dir.x * cx + (double)r.dir.y * cy + (double)r.dir.z * cz) / (cn * ld)));
#ifdef _OPENMP
#pragma omp critical(orc_audit)
#endif
    {
        g_audit_hits++;
        g_audit_incons += best_t < best_te;
        g_audit_half += head > 0.5;
        g_audit_unsafe += (uint64_t)unsafe;
        if (head > g_audit_max) g_audit_max = head;
        if (head_c > g_audit_max_c) g_audit_max_c = head_c;
        g_audit_sliver += (uint64_t)sliver;
        if (sliver && head > g_audit_sliver_max) g_audit_sliver_max = head;
        g_audit_shape_n[bs]++;
        g_audit_graze_n[bg]++;
        if (head > g_audit_shape[bs]) g_audit_shape[bs] = head;
        if (head > g_audit_graze[bg]) g_audit_graze[bg] = head;
    }
}

/* Format 2 (accel_build.h): the 4-wide walk.  Each step fetches one 64-B
 * record.  A leaf: hit_triangle on its v0 / e1 / e2; only a hit the walk would
 * take (t < closest_t, or a tie with a lower index) reads the rest of the
 * leaf's exact box and runs its slab test (the reference's hit_aabb
 * arithmetic) with the leaf's rule, which decides.  A wide node: each child's
 * box decoded from the node's grid (origin + q 2^e in float) and slab-tested
 * with the child's rule; the entered children in (t_enter, slot) order, the
 * first next, the rest pushed farthest first on a stack of g_stack_k entries
 * (an overflow walks the segment again in the reference's order).  A stack
 * entry keeps its t_enter rounded down to bfloat16 (the kernel's 2-byte LDS
 * field); a popped default-margin entry whose rounded-down t_enter fails the
 * rule is dropped.  node_visits = 1 (the root) + box tests (children and leaf
 * boxes), tri_tests = leaf records read; g_count_steps: node_visits counts
 * record fetches instead (analysis). */
static float rec_f16(size_t idx, int w) {
    float f;
    memcpy(&f, &g_rec[16 * idx + (size_t)w], 4);
    return f;
}

static void slab3(vec3 lo, vec3 hi, ray r, vec3 inv, float* te, float* tx) {
    const vec3 t0s = mul3(sub3(lo, r.origin), inv);
    const vec3 t1s = mul3(sub3(hi, r.origin), inv);
    *te = fmaxf(fmaxf(fminf(t0s.x, t1s.x), fminf(t0s.y, t1s.y)), fminf(t0s.z, t1s.z));
    *tx = fminf(fminf(fmaxf(t0s.x, t1s.x), fmaxf(t0s.y, t1s.y)), fmaxf(t0s.z, t1s.z));
}

static float bf16_down(float x) {            /* truncated to bfloat16: down for x >= 0 */
    uint32_t u;
    memcpy(&u, &x, 4);
    u &= 0xFFFF0000u;
    memcpy(&x, &u, 4);
    return x;
}

#define WIDE_LEAF (1u << 31)
#define WIDE_THIN (1u << 30)
#define WIDE_WIDER (1u << 29)
#define WIDE_IDX 0x07FFFFFFu

static int wide_walk(const scene* s, ray r, float* closest_t, int* hit_index, vec3* hit_normal, orc_counts* cnt) {
    const vec3 inv = v3(rcp(r.dir.x), rcp(r.dir.y), rcp(r.dir.z));
    float c = *closest_t;
    float hit_te = 0.0f;
    int hit = -1;
    uint32_t st_link[64];
    float st_te[64];
    int sp = 0, overflow = 0;
    uint32_t cur = g_root_leaf ? WIDE_LEAF : 0u;
    if (!g_count_steps) cnt->node_visits++;      /* the root visit (the kernel counts it at segment start) */
    for (;;) {
        const size_t idx = cur & WIDE_IDX;
        if ((size_t)idx >= (size_t)g_slots) return -1;
        const uint32_t* w = &g_rec[16 * idx];
        if (g_count_steps) cnt->node_visits++;
        if (cur & WIDE_LEAF) {
            const int tri = (int)(w[0] & 0x1FFFFFFFu);
            cnt->tri_tests++;
            if ((size_t)tri >= s->n_tris || (size_t)tri >= s->n_mats) return -1;
            vec3 nrm;
            float t = INFINITY;
            if (hit_triangle(r, vertex_pos(s, (size_t)tri * 3 + 0), vertex_pos(s, (size_t)tri * 3 + 1),
                             vertex_pos(s, (size_t)tri * 3 + 2), &t, &nrm) &&
                (t < c || (t == c && tri < hit))) {
                if (!g_count_steps) cnt->node_visits++;
                float te, tx;
                slab3(v3(rec_f16(idx, 7), rec_f16(idx, 11), rec_f16(idx, 12)),
                      v3(rec_f16(idx, 13), rec_f16(idx, 14), rec_f16(idx, 15)), r, inv, &te, &tx);
                const float rf = (w[0] & (1u << 29)) ? INFINITY : g_relax;
                if (tx > te && tx > T_MIN && te <= c * rf + g_relax_abs) {
                    c = t;
                    hit = tri;
                    hit_te = te;
                    *hit_normal = nrm;
                }
            }
        } else {
            const int n = (int)((w[3] >> 24) & 7u);
            const vec3 org = v3(rec_f16(idx, 0), rec_f16(idx, 1), rec_f16(idx, 2));
            const int ex = (int8_t)(w[3] & 0xFFu), ey = (int8_t)((w[3] >> 8) & 0xFFu), ez = (int8_t)((w[3] >> 16) & 0xFFu);
            const float sx = ldexpf(1.0f, ex), sy = ldexpf(1.0f, ey), sz = ldexpf(1.0f, ez);
            const float nr = class_relax((int)(w[10] >> 27));
            const uint32_t base = w[10] & WIDE_IDX;
            float ce[4];
            uint32_t cl[4];
            int h = 0;
            for (int i = 0; i < n; ++i) {
                const int sh = 8 * i;
                const vec3 lo = v3(org.x + (float)((w[4] >> sh) & 0xFFu) * sx, org.y + (float)((w[5] >> sh) & 0xFFu) * sy,
                                   org.z + (float)((w[6] >> sh) & 0xFFu) * sz);
                const vec3 hi = v3(org.x + (float)((w[7] >> sh) & 0xFFu) * sx, org.y + (float)((w[8] >> sh) & 0xFFu) * sy,
                                   org.z + (float)((w[9] >> sh) & 0xFFu) * sz);
                if (!g_count_steps) cnt->node_visits++;
                float te, tx;
                slab3(lo, hi, r, inv, &te, &tx);
                const uint32_t f = (w[11] >> sh) & 0xFFu;
                const uint32_t link = (base + (uint32_t)i) | ((f & 1u) ? WIDE_LEAF : 0u) | ((f & 2u) ? WIDE_THIN : 0u) |
                                      ((f & 4u) ? WIDE_WIDER : 0u);
                const float rf = (f & 2u) ? INFINITY : ((f & 4u) ? nr : g_relax);
                if (tx > te && tx > T_MIN && te <= c * rf + g_relax_abs) {
                    /* insert in (t_enter, slot) order: a later slot goes after an equal te */
                    int k = h++;
                    while (k > 0 && ce[k - 1] > te) {
                        ce[k] = ce[k - 1];
                        cl[k] = cl[k - 1];
                        --k;
                    }
                    ce[k] = te;
                    cl[k] = link;
                }
            }
            if (h > 0) {
                if (sp + h - 1 > g_stack_k) {
                    overflow = 1;
                    break;
                }
                for (int k = h - 1; k >= 1; --k) {
                    st_link[sp] = cl[k];
                    st_te[sp] = bf16_down(ce[k]);
                    ++sp;
                }
                cur = cl[0];
                continue;
            }
        }
        int found = 0;
        while (sp > 0) {
            --sp;
            const uint32_t link = st_link[sp];
            if (!(link & (WIDE_THIN | WIDE_WIDER)) && !(st_te[sp] <= c * g_relax + g_relax_abs)) continue;
            cur = link;
            found = 1;
            break;
        }
        if (!found) break;
    }
    if (overflow || (hit >= 0 && c < hit_te)) {
#ifdef _OPENMP
#pragma omp atomic
#endif
        g_fallbacks++;
        if (overflow) {
#ifdef _OPENMP
#pragma omp atomic
#endif
            g_overflows++;
        }
        return reference_walk(s, r, closest_t, hit_index, hit_normal, cnt);
    }
    *closest_t = c;
    *hit_index = hit;
    return 0;
}

static int accel_walk(const scene* s, ray r, float* closest_t, int* hit_index, vec3* hit_normal,
                      orc_counts* cnt) {
    if (g_slots == 0) return 0;                 /* empty scene: every ray misses */
    if (g_fmt == 2) return wide_walk(s, r, closest_t, hit_index, hit_normal, cnt);
    if (g_audit) audit_segment(s, r);
    const int oct = g_layouts == 8 ? ((signbit(r.dir.x) ? 1 : 0) | (signbit(r.dir.y) ? 2 : 0) |
                                      (signbit(r.dir.z) ? 4 : 0)) & g_oct_mask : 0;
    size_t n = (size_t)oct * (size_t)g_slots;
    const size_t end = n + (size_t)g_slots;
    int leaf = g_root_leaf;
    const vec3 inv = v3(rcp(r.dir.x), rcp(r.dir.y), rcp(r.dir.z));
    float c = *closest_t;
    float hit_te = 0.0f;                      /* t_enter of the hit triangle's own box */
    int hit = -1;
    uint64_t leaf_visits = 0;
    const size_t WS = g_fmt ? 4 : 8;
    for (int k = 0; k < g_root_enter && !g_fmt && !leaf && g_slots > 1; ++k) {
        /* format 0: the walk starts inside the root (rt_trace.hip, DevScene::root_enter):
         * its box is not tested; it counts as visited and entered (a study:
         * g_root_enter > 1 enters the first child the same way, and so on) */
        cnt->node_visits++;
        leaf = (int)(g_rec[8 * n + 7] >> 31);
        n += 1;
    }
    while (n < end) {
        const uint32_t aw = g_rec[WS * n + 3], bw = g_fmt ? 0u : g_rec[8 * n + 7];
        cnt->node_visits++;
        trace_rec((int32_t)n);
        /* the slab test of hit_aabb (:88-103), t_enter <= closest_t */
        vec3 blo, bhi;
        if (g_fmt && !leaf) {
            const uint32_t* w = &g_rec[4 * n];
            blo = v3(half_to_float(w[0] & 0xFFFFu), half_to_float(w[0] >> 16), half_to_float(w[1] & 0xFFFFu));
            bhi = v3(half_to_float(w[1] >> 16), half_to_float(w[2] & 0xFFFFu), half_to_float(w[2] >> 16));
        } else {
            blo = v3(rec_f(n, 0), rec_f(n, 1), rec_f(n, 2));
            bhi = v3(rec_f(n, 4), rec_f(n, 5), rec_f(n, 6));
        }
        if (g_quant == 1 && !leaf) {
            blo = v3(half_down(blo.x), half_down(blo.y), half_down(blo.z));
            bhi = v3(half_up(bhi.x), half_up(bhi.y), half_up(bhi.z));
        }
        const vec3 t0s = mul3(sub3(blo, r.origin), inv);
        const vec3 t1s = mul3(sub3(bhi, r.origin), inv);
        const float te = fmaxf(fmaxf(fminf(t0s.x, t1s.x), fminf(t0s.y, t1s.y)), fminf(t0s.z, t1s.z));
        const float tx = fminf(fminf(fmaxf(t0s.x, t1s.x), fmaxf(t0s.y, t1s.y)), fmaxf(t0s.z, t1s.z));
        const int hb = tx > te && tx > T_MIN && te <= c * rec_factor(leaf, aw) + g_relax_abs;
        leaf_visits += (uint64_t)leaf;
        if (hb && leaf) {
            const int tri = (int)(aw & 0x1FFFFFFFu);
            cnt->tri_tests++;
            if ((size_t)tri >= s->n_tris || (size_t)tri >= s->n_mats) return -1;
            /* hit_triangle (:105-129) on the flattened triangle's own vertices */
            vec3 nrm;
            float t = INFINITY;
            if (hit_triangle(r, vertex_pos(s, (size_t)tri * 3 + 0), vertex_pos(s, (size_t)tri * 3 + 1),
                             vertex_pos(s, (size_t)tri * 3 + 2), &t, &nrm) &&
                (t < c || (t == c && tri < hit))) {
                c = t;
                hit = tri;
                hit_te = te;
                *hit_normal = nrm;
            }
        }
        size_t nxt;
        int nl;
        if (leaf) {
            nxt = n + (g_fmt ? 4 : 2);
            nl = (int)(aw >> 31);
        } else if (hb) {
            nxt = n + 1;
            nl = g_fmt ? (int)((aw >> 30) & 1u) : (int)(bw >> 31);
        } else {
            nxt = aw & (g_fmt ? 0x3FFFFFFFu : 0x1FFFFFFFu);
            nl = (int)(aw >> 31);
        }
        if (nxt <= n && !hb) return -1;         /* a link that does not move forward: bad records */
        n = nxt;
        leaf = nl;
    }
#ifdef _OPENMP
#pragma omp atomic
#endif
    g_leaf_visits += leaf_visits;
    if (hit >= 0 && c < hit_te) {
        /* The hit lies before its own box's t_enter (float rounding on the
         * box face): the one case where the reference's result depends on
         * its visit order.  Re-walk the segment in the reference's order. */
#ifdef _OPENMP
#pragma omp atomic
#endif
        g_fallbacks++;
        return reference_walk(s, r, closest_t, hit_index, hit_normal, cnt);
    }
    *closest_t = c;
    *hit_index = hit;
    return 0;
}
