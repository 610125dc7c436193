// scene_plan.cpp — the host side of a scene upload (scene_plan.h): the
// compact scene, the reference's walk records and option refit's tables.
#include "scene_plan.h"

#include "accel_build.h"
#include "refit_levels_host.h"
#include "../../include/rtamd.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>

namespace rtamd {

static inline float f32_at(const unsigned char* p, size_t off) {
    float f;
    std::memcpy(&f, p + off, 4);
    return f;
}
static inline int32_t i32_at(const unsigned char* p, size_t off) {
    int32_t v;
    std::memcpy(&v, p + off, 4);
    return v;
}
static inline uint32_t bits(float f) {
    uint32_t v;
    std::memcpy(&v, &f, 4);
    return v;
}
static inline float as_float(uint32_t v) {
    float f;
    std::memcpy(&f, &v, 4);
    return f;
}

int build_host_scene(const void* vertices, size_t vertex_bytes,
                     const void* materials, size_t material_bytes,
                     const void* bvh_nodes, size_t bvh_bytes,
                     HostScene* out, std::string* err) try {
    *out = HostScene{};
    const size_t n_nodes = bvh_bytes < RT_NODE_RECORD_BYTES ? 0 : bvh_bytes / RT_NODE_RECORD_BYTES;
    const size_t n_tris  = vertex_bytes < RT_VERTEX_RECORD_BYTES ? 0 : vertex_bytes / RT_VERTEX_RECORD_BYTES;
    const size_t n_mats  = material_bytes < RT_MATERIAL_RECORD_BYTES ? 0 : material_bytes / RT_MATERIAL_RECORD_BYTES;
    auto fail = [&](const std::string& m) {
        *err = m;
        *out = HostScene{};
        return RT_ERR_BAD_SCENE;
    };
    if (n_nodes && bvh_bytes % RT_NODE_RECORD_BYTES)
        return fail("bvh_bytes is not a multiple of 48");
    if (n_tris && vertex_bytes % RT_VERTEX_RECORD_BYTES)
        return fail("vertex_bytes is not a multiple of 48");
    if (n_mats && material_bytes % RT_MATERIAL_RECORD_BYTES)
        return fail("material_bytes is not a multiple of 16");
    if (n_nodes > (size_t)INT32_MAX / 2 || n_tris > (size_t)INT32_MAX / 3)
        return fail("scene too large for 32-bit node/triangle indices");
    if (n_nodes && (!bvh_nodes)) return fail("null bvh buffer");
    if (n_tris && (!vertices)) return fail("null vertex buffer");
    if (n_mats && (!materials)) return fail("null material buffer");

    out->n_nodes = (int)n_nodes;
    out->n_tris  = (int)n_tris;
    const unsigned char* nb = static_cast<const unsigned char*>(bvh_nodes);
    std::vector<int32_t> skip(n_nodes), depth(n_nodes, 0);

    // Pass 1 (reverse): leaf skip = i+1, internal skip = skip(right).  The
    // layout must be the reference flattener's preorder: left == i+1 and the
    // left subtree ends exactly where the right child starts.
    for (size_t k = n_nodes; k-- > 0;) {
        const unsigned char* r = nb + k * RT_NODE_RECORD_BYTES;
        const int32_t data = i32_at(r, 32), count = i32_at(r, 36);
        if (count < 0) {                                   // leaf (compute_dynamic_ray.comp:194-195)
            const int64_t tri = -((int64_t)data + 1);
            if (tri < 0 || (size_t)tri >= n_tris || (size_t)tri >= n_mats)
                return fail("leaf node " + std::to_string(k) + " references triangle " +
                            std::to_string(tri) + " outside the vertex/material buffers");
            skip[k] = (int32_t)(k + 1);
        } else {
            if ((size_t)data != k + 1 || count <= data || (size_t)count >= n_nodes)
                return fail("node " + std::to_string(k) +
                            " is not in the reference's preorder layout (left must be i+1, right > left)");
            if (skip[data] != count)
                return fail("node " + std::to_string(k) + ": left subtree does not end at the right child");
            skip[k] = skip[count];
        }
    }
    out->end = n_nodes ? skip[0] : 0;   // empty scene: every ray misses (reference: undefined read of node 0)
    std::vector<uint8_t> is_leaf(n_nodes + 1, 0);
    for (size_t k = 0; k < n_nodes; ++k) is_leaf[k] = i32_at(nb + k * RT_NODE_RECORD_BYTES, 36) < 0;
    out->root_leaf = is_leaf[0];
    // zero pages until written (LazyZero): the records nobody writes, and the padding, cost nothing
    out->nodes = HostScene::Array(2 * n_nodes + 2);
    out->leafs = HostScene::Array(3 * n_nodes + 1);
    out->pairs = HostScene::Array(4 * std::max<size_t>(n_nodes, 1));
    const unsigned char* vb = static_cast<const unsigned char*>(vertices);
    int max_depth = 0;
    for (size_t k = 0; k < (size_t)out->end; ++k) {
        const unsigned char* r = nb + k * RT_NODE_RECORD_BYTES;
        const int32_t data = i32_at(r, 32), count = i32_at(r, 36);
        if (count >= 0) {
            depth[data] = depth[k] + 1;
            depth[count] = depth[k] + 1;
        }
        if (depth[k] > max_depth) max_depth = depth[k];
        const uint32_t sk = (uint32_t)skip[k];
        const uint32_t aw = sk | ((sk < (uint32_t)out->end && is_leaf[sk]) ? 0x80000000u : 0u);
        const uint32_t bw = ((k + 1 < (size_t)out->end && is_leaf[k + 1]) ? 1u : 0u) | (is_leaf[k] ? 2u : 0u);
        const Vec4 A = {f32_at(r, 0), f32_at(r, 4), f32_at(r, 8), as_float(aw)};
        const Vec4 B = {f32_at(r, 16), f32_at(r, 20), f32_at(r, 24), as_float(bw)};
        out->nodes[2 * k] = A;
        out->nodes[2 * k + 1] = B;
        if (k == 0) {
            out->root_box[0] = A.x; out->root_box[1] = A.y; out->root_box[2] = A.z;
            out->root_box[3] = B.x; out->root_box[4] = B.y; out->root_box[5] = B.z;
        }
        if (count >= 0) {
            const unsigned char* l = nb + (size_t)data * RT_NODE_RECORD_BYTES;
            const unsigned char* rr = nb + (size_t)count * RT_NODE_RECORD_BYTES;
            const uint32_t rw = (uint32_t)count | (is_leaf[count] ? 0x80000000u : 0u);
            const uint32_t lw = is_leaf[data] ? 1u : 0u;
            out->pairs[4 * k + 0] = {f32_at(l, 0), f32_at(l, 4), f32_at(l, 8), f32_at(rr, 0)};
            out->pairs[4 * k + 1] = {f32_at(l, 16), f32_at(l, 20), f32_at(l, 24), f32_at(rr, 4)};
            out->pairs[4 * k + 2] = {f32_at(rr, 16), f32_at(rr, 20), f32_at(rr, 24), f32_at(rr, 8)};
            out->pairs[4 * k + 3] = {as_float(rw), as_float(lw), as_float(sk), 0.f};
        }
        if (count < 0) {
            // edge1 / edge2 exactly as hit_triangle computes them (compute_dynamic_ray.comp:106-107)
            const int32_t tri = -(data + 1);
            const unsigned char* v = vb + (size_t)tri * RT_VERTEX_RECORD_BYTES;
            const float v0x = f32_at(v, 0),  v0y = f32_at(v, 4),  v0z = f32_at(v, 8);
            const float v1x = f32_at(v, 16), v1y = f32_at(v, 20), v1z = f32_at(v, 24);
            const float v2x = f32_at(v, 32), v2y = f32_at(v, 36), v2z = f32_at(v, 40);
            out->leafs[3 * k + 0] = {v0x, v0y, v0z, as_float((uint32_t)tri)};
            out->leafs[3 * k + 1] = {v1x - v0x, v1y - v0y, v1z - v0z, 0.f};
            out->leafs[3 * k + 2] = {v2x - v0x, v2y - v0y, v2z - v0z, 0.f};
        }
    }
    out->max_depth = max_depth;

    out->shade = HostScene::Array(kShadeStride * std::max<size_t>(n_tris, 1));
    const unsigned char* mb = static_cast<const unsigned char*>(materials);
    for (size_t t = 0; t < n_tris; ++t) {
        const unsigned char* r = vb + t * RT_VERTEX_RECORD_BYTES;
        const float v0x = f32_at(r, 0),  v0y = f32_at(r, 4),  v0z = f32_at(r, 8);
        const float v1x = f32_at(r, 16), v1y = f32_at(r, 20), v1z = f32_at(r, 24);
        const float v2x = f32_at(r, 32), v2y = f32_at(r, 36), v2z = f32_at(r, 40);
        // normalize(cross(edge1, edge2)) exactly as hit_triangle computes it (:124)
        const float e1x = v1x - v0x, e1y = v1y - v0y, e1z = v1z - v0z;
        const float e2x = v2x - v0x, e2y = v2y - v0y, e2z = v2z - v0z;
        const float cx = e1y * e2z - e1z * e2y;
        const float cy = e1z * e2x - e1x * e2z;
        const float cz = e1x * e2y - e1y * e2x;
        const float l = std::sqrt((cx * cx + cy * cy) + cz * cz);
        out->shade[kShadeStride * t] = {cx / l, cy / l, cz / l, 0.f};
        if (t < n_mats) {
            const unsigned char* m = mb + t * RT_MATERIAL_RECORD_BYTES;
            out->shade[kShadeStride * t + 1] = {f32_at(m, 0), f32_at(m, 4), f32_at(m, 8), f32_at(m, 12)};
        } else {
            out->shade[kShadeStride * t + 1] = {0.f, 0.f, 0.f, -1.f};   // never referenced (validated above)
        }
    }
    return RT_OK;
} catch (const std::bad_alloc&) {
    *err = "out of host memory";
    *out = HostScene{};
    return RT_ERR_BAD_SCENE;
}

// walk 2's records (DevScene::walk; rt_internal.h): the reference's
// preorder with every leaf's triangle inlined after its box, so an
// internal node takes one 32-B slot and a leaf two.  slot(i) = i + the
// leaves before i; an internal node's left child is the next slot, a
// leaf's successor (its skip, i+1) the slot after its two, and only the
// internal skip is stored, as a slot.  The visit sequence is the
// reference's, node for node.
// Option leaf_align: a leaf that would start in the last slot of a 128-B
// line (and straddle two) starts one slot later; its predecessor's pad bit
// (a leaf's bit 29 of word [0].w, an internal node's bit 2 of word [1].w)
// tells the walk to step over the pad slot.
// Only the root's subtree, [0, end): nodes past the root's skip are
// never visited by the reference's DFS (compute_dynamic_ray.comp:185-210).
static int plan_walk(int leaf_align, ScenePlan* p, std::string* err) {
    const HostScene& hs = p->host;
    const size_t n2 = (size_t)hs.end;
    const auto is_leaf = [&hs](size_t i) { return (bits(hs.nodes[2 * i + 1].w) & 2u) != 0; };
    char msg[160];
    std::vector<int>& slot = p->node_slot;
    slot.assign(n2 + 1, 0);
    std::vector<uint8_t> padded(n2 + 1, 0);       // a pad slot precedes node i
    size_t n_leaves = 0;
    for (size_t i = 0; i < n2; ++i) n_leaves += is_leaf(i) ? 1 : 0;
    const bool align = leaf_align == 1 || (leaf_align == 2 && (n2 + n_leaves) * 32 > kWin32Bytes);
    size_t nslot = 0;
    for (size_t i = 0; i < n2; ++i) {
        if (align && is_leaf(i) && nslot % 4 == 3) {
            padded[i] = 1;
            ++nslot;
            p->padded = true;
        }
        slot[i] = (int)nslot;
        nslot += is_leaf(i) ? 2 : 1;
        if (nslot >= kMaxWalkSlots) {
            std::snprintf(msg, sizeof msg, "%zu nodes: at most %u walk slots (4 GB of walk records) supported", n2,
                          kMaxWalkSlots);
            *err = msg;
            return RT_ERR_BAD_SCENE;
        }
    }
    slot[n2] = (int)nslot;
    p->slots = (int)nslot;
    std::vector<Vec4>& walk = p->walk;
    walk.assign(2 * nslot + 4, Vec4{0.f, 0.f, 0.f, 0.f});   // + padding read at the end
    p->slot_node.assign(nslot + 1, -1);
    for (size_t i = 0; i < n2; ++i) {
        const size_t w = 2 * (size_t)slot[i];
        p->slot_node[slot[i]] = (int)i;
        walk[w] = hs.nodes[2 * i];
        walk[w + 1] = hs.nodes[2 * i + 1];
        const uint32_t link = bits(hs.nodes[2 * i].w);
        if (!is_leaf(i)) {                                  // internal: the skip as a slot (< 2^30: bit 30 clear)
            const uint32_t sk = link & 0x7FFFFFFFu;
            walk[w].w = as_float((uint32_t)slot[sk] | (link & 0x80000000u));
            if (padded[i + 1])                              // the left child (i+1) sits past a pad slot
                walk[w + 1].w = as_float(bits(walk[w + 1].w) | 4u);
            continue;
        }
        const uint32_t tri = bits(hs.leafs[3 * i].w);
        if ((link & 0x7FFFFFFFu) != i + 1 || tri >= (1u << 29)) {
            std::snprintf(msg, sizeof msg, "leaf %zu: skip %u is not i+1 or triangle index %u too large", i,
                          link & 0x7FFFFFFFu, tri);
            *err = msg;
            return RT_ERR_BAD_SCENE;
        }
        walk[w].w = as_float(tri | (padded[i + 1] ? 1u << 29 : 0u) | (1u << 30) | (link & 0x80000000u));
        const Vec4 P0 = hs.leafs[3 * i], P1 = hs.leafs[3 * i + 1], P2 = hs.leafs[3 * i + 2];
        walk[w + 1].w = P0.x;                                                // v0.x
        walk[w + 2] = {P0.y, P0.z, P1.x, P1.y};                              // v0.yz, e1.xy
        walk[w + 3] = {P1.z, P2.x, P2.y, P2.z};                              // e1.z, e2
    }
    return RT_OK;
}

// Option refit: what rt_update_geometry needs, laid out once as the bytes every device
// gets behind its staging buffers, and the context's side of it.  ah: the accel build, or null.
static void plan_refit(const void* bvh_nodes, const AccelHost* ah, bool refit_device, ScenePlan* p) {
    const HostScene& hs = p->host;
    const size_t n2 = (size_t)hs.end;
    std::vector<uint8_t>& tab = p->refit;      // the tables, sections 16-B aligned
    RefitLayout& rl = p->rl;
    const auto section = [&tab](size_t bytes) {
        const size_t at = tab.size();
        tab.resize(at + (bytes + 15) / 16 * 16, 0);
        return at;
    };
    rl.staging_boxes = (size_t)hs.n_tris * 48;
    rl.staging_bytes = (rl.staging_boxes + (size_t)hs.n_nodes * 24 + 15) / 16 * 16;
    rl.info = section(4 * n2);
    rl.slot = section(4 * n2);
    for (size_t i = 0; i < n2; ++i) {
        uint32_t v;
        if (bits(hs.nodes[2 * i + 1].w) & 2u) v = bits(hs.leafs[3 * i].w);                      // the triangle
        else v = (uint32_t)(-(int32_t)((bits(hs.pairs[4 * i + 3].x) & 0x7FFFFFFFu) + 1));      // the right child
        std::memcpy(&tab[rl.info + 4 * i], &v, 4);
        std::memcpy(&tab[rl.slot + 4 * i], &p->node_slot[i], 4);
    }
    p->refit_level_first.assign(1, 0);
    if (ah && ah->slots > 0) {
        const size_t m = ah->prim_tri.size(), nc = ah->node_height.size();
        rl.has_accel = true;
        rl.n_layouts = ah->n_layouts;
        rl.n_canon = (int)nc;
        rl.n_prims = (int)m;
        rl.prim = section(12 * m);
        for (size_t k = 0; k < m; ++k) {
            const int32_t rec[3] = {ah->prim_tri[k], ah->prim_leaf[k], ah->prim_node[k]};
            std::memcpy(&tab[rl.prim + 12 * k], rec, 12);
        }
        rl.child = section(8 * nc);
        std::memcpy(&tab[rl.child], ah->node_child.data(), 8 * nc);
        rl.layout_slot = section(4 * nc * (size_t)ah->n_layouts);
        std::memcpy(&tab[rl.layout_slot], ah->node_slot.data(), 4 * nc * (size_t)ah->n_layouts);
        // the internal nodes by height, lowest first (a counting sort), and where each height starts
        int top = 0;
        for (size_t c = 0; c < nc; ++c) top = std::max(top, ah->node_height[c]);
        std::vector<int> first(top + 2, 0);
        for (size_t c = 0; c < nc; ++c)
            if (ah->node_height[c] > 0) ++first[ah->node_height[c] + 1];
        for (int h = 1; h <= top + 1; ++h) first[h] += first[h - 1];
        rl.by_height = section(4 * (nc - m));
        std::vector<int> at(first.begin(), first.end());
        for (size_t c = 0; c < nc; ++c)
            if (ah->node_height[c] > 0) {
                const int32_t id = (int32_t)c;
                std::memcpy(&tab[rl.by_height + 4 * (size_t)at[ah->node_height[c]]++], &id, 4);
            }
        p->refit_level_first.assign(first.begin() + 1, first.end());         // heights 1 .. top, then the end
        rl.canon = section(32 * nc);
    }
    const unsigned char* nbytes = static_cast<const unsigned char*>(bvh_nodes);
    p->refit_links.resize(24 * (size_t)hs.n_nodes);
    for (size_t i = 0; i < (size_t)hs.n_nodes; ++i) {
        std::memcpy(&p->refit_links[24 * i], nbytes + 48 * i + 12, 4);
        std::memcpy(&p->refit_links[24 * i + 4], nbytes + 48 * i + 28, 20);
    }
    if (ah) p->refit_dups = ah->dup_pairs;
    // Option refit_device: the reference nodes by height, the dropped duplicates and
    // the check's status words behind the tables above, which stay where they are without it
    std::vector<int32_t> by_height;
    p->front = refit_device &&
               refit_levels(reinterpret_cast<const int32_t*>(tab.data() + rl.info), n2, &by_height, &p->refit_front_first);
    if (p->front) {
        rl.front_by_height = section(4 * n2);
        if (n2) std::memcpy(&tab[rl.front_by_height], by_height.data(), 4 * n2);
        rl.front_dups = section(4 * p->refit_dups.size());
        if (!p->refit_dups.empty()) std::memcpy(&tab[rl.front_dups], p->refit_dups.data(), 4 * p->refit_dups.size());
        rl.front_status = section(sizeof(unsigned) * kRefitStatusWords);
    }
}

int plan_scene(const void* vertices, size_t vertex_bytes, const void* materials, size_t material_bytes,
               const void* bvh_nodes, size_t bvh_bytes, const PlanOptions& opt, ScenePlan* out, std::string* err) {
    *out = ScenePlan{};
    int rc = build_host_scene(vertices, vertex_bytes, materials, material_bytes, bvh_nodes, bvh_bytes, &out->host, err);
    if (rc == RT_OK) rc = plan_walk(opt.leaf_align, out, err);
    if (rc != RT_OK) return rc;
    // Option accel: the binned-SAH records (accel_build.h), built once for
    // every device; the reference's walk records above stay beside them for
    // the fallback, and the node-indexed arrays (walk 0, the frontier walk of
    // heavy pixels) are not needed.
    // Past the slot cap 8 layouts become 1, and a scene too large for one
    // walks the reference's own tree (accel_used says which: 8, 1 or 0).
    AccelHost ah;
    if (opt.accel) {
        const int arc = accel_build_fit(vertices, vertex_bytes, materials, material_bytes, bvh_nodes,
                                        (size_t)out->host.end * RT_NODE_RECORD_BYTES, opt.accel, &ah, err,
                                        opt.accel_wide ? 2 : opt.accel_half ? 1 : 0, opt.accel_cap_slots,
                                        opt.refit != 0);
        if (arc != 0 && arc != kAccelTooBig) return RT_ERR_BAD_SCENE;
        out->has_accel = arc == 0;
    }
    // The half and wide record formats hold no refit tables.
    out->keep = opt.refit && !(out->has_accel && ah.format != 0);
    if (out->keep) plan_refit(bvh_nodes, out->has_accel ? &ah : nullptr, opt.refit_device != 0, out);
    if (out->has_accel) {
        out->n_layouts = ah.n_layouts;
        out->layout_slots = ah.slots;
        out->half = ah.format == 1 ? 1 : 0;
        out->wide = ah.format == 2 ? 1 : 0;
        out->relax_half = ah.relax_max;
        out->accel_root_leaf = ah.root_leaf;
        out->root_enter = ah.format == 0 && !ah.root_leaf && ah.slots > 1 ? 1 : 0;
        if (out->root_enter)
            for (int o = 0; o < ah.n_layouts; ++o)
                out->root_first_leaf |= (int)(ah.rec[8 * (size_t)o * (size_t)ah.slots + 7] >> 31) << o;
        out->accel_rec = std::move(ah.rec);
    }
    return RT_OK;
}

}  // namespace rtamd
