// scene_plan.h — what rt_upload_scene puts on a device, laid out on the host
// (pure host C++; no HIP types, so tools/scene_plan_check.cpp builds it with
// g++ and runs it under the sanitizers).
//
// plan_scene turns the caller's three buffers and the upload's options into a
// ScenePlan: every device array as the exact bytes the device receives, zero
// padding included, and the scalars DevScene and the context take.  The
// runtime only allocates and copies.  The arrays' formats are those of
// rt_internal.h (DevScene, RefitTables, RefitFront) and accel_build.h.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <new>
#include <string>
#include <utility>
#include <vector>

namespace rtamd {

struct Vec4 { float x, y, z, w; };       // a device float4's 16 bytes
static_assert(sizeof(Vec4) == 16, "Vec4 is a float4's bytes");

// norms and mats interleave in one array: kShadeStride Vec4 per flattened
// triangle, the normal, then albedo/type (DevScene::norms, rt_internal.h)
constexpr int kShadeStride = 2;
// coop_window 0: scenes whose walk records exceed the 8 XCDs' L2s together
// (8 x 4 MB) take 32-slot windows: config 5 (100 MB) fetched 22.4 instead of
// 28.5 GB per frame at the same frame time; config 3 (6.3 MB, L2-resident)
// is 1.2% faster with 64 (profiles/r04/r4f).  leaf_align 2 aligns past it too.
constexpr size_t kWin32Bytes = 32ull << 20;
// The walk's buffer loads address the records with 32-bit byte offsets
// (rt_trace.hip wbuf): at most 2^27 - 4 slots of 32 B (~45M triangles).
constexpr unsigned kMaxWalkSlots = (1u << 27) - 4;
constexpr int kRefitStatusWords = 4;     // RefitFront::status (rt_internal.h)

// An allocator whose vector(n) is calloc's memory left as it is: zero pages that
// cost nothing until written (half of leafs and pairs never is: config 5's
// upload spent 40 ms more writing those zeros out).  For types whose zero bytes
// are their value-initialised state.
template <class T> struct LazyZero {
    using value_type = T;
    LazyZero() = default;
    template <class U> LazyZero(const LazyZero<U>&) {}
    T* allocate(size_t n) {
        if (void* p = std::calloc(n, sizeof(T))) return static_cast<T*>(p);
        throw std::bad_alloc();
    }
    void deallocate(T* p, size_t) { std::free(p); }
    template <class U> void construct(U*) {}                       // value-initialisation: calloc's zeros
    template <class U, class A0, class... A> void construct(U* p, A0&& a0, A&&... a) {
        ::new (static_cast<void*>(p)) U(std::forward<A0>(a0), std::forward<A>(a)...);
    }
    bool operator==(const LazyZero&) const { return true; }
    bool operator!=(const LazyZero&) const { return false; }
};

// Host-side compact-scene build from the reference records; validates the
// buffers.  Returns RT_OK or RT_ERR_BAD_SCENE with a message in *err.
// nodes and leafs are padded by one zero record: walks read the record at
// index end (the node after the last) before they test for the end.
struct HostScene {
    using Array = std::vector<Vec4, LazyZero<Vec4>>;
    int n_nodes = 0, end = 0, n_tris = 0, max_depth = 0, root_leaf = 0;
    float root_box[6] = {0, 0, 0, 0, 0, 0};
    Array nodes;    // 2*n_nodes + 2
    Array leafs;    // 3*n_nodes + 1
    Array pairs;    // 4*max(n_nodes, 1)
    Array shade;    // kShadeStride*max(n_tris, 1): triangle t's normal, then its material
};
int build_host_scene(const void* vertices, size_t vertex_bytes,
                     const void* materials, size_t material_bytes,
                     const void* bvh_nodes, size_t bvh_bytes,
                     HostScene* out, std::string* err);

// The options an upload reads (rt_ctx's, rtamd.h) and the accel slot cap
// (0 = the hardware's; accel_build.h).
struct PlanOptions {
    int leaf_align = 2, accel = 8, accel_half = 0, accel_wide = 0, refit = 0, refit_device = 0;
    int64_t accel_cap_slots = 0;
};

// Option refit's tables: byte offsets of the 16-B aligned
// sections of ScenePlan::refit, which lies behind the staging arrays in the
// device's allocation.  The accel sections exist with has_accel, the last
// three with ScenePlan::front.
struct RefitLayout {
    size_t staging_boxes = 0;            // staging: the vertex records (48 B per triangle), then from here the
    size_t staging_bytes = 0;            //   boxes (24 B per node), staging_bytes in all; the tables follow
    size_t info = 0, slot = 0;           // RefitTables::ref_info, ref_slot
    bool   has_accel = false;
    int    n_layouts = 0, n_canon = 0, n_prims = 0;
    size_t prim = 0, child = 0, layout_slot = 0, by_height = 0, canon = 0;   // RefitTables::prim .. canon
    size_t front_by_height = 0, front_dups = 0, front_status = 0;            // RefitFront::by_height, dups, status
};

struct ScenePlan {
    HostScene host;                      // nodes, leafs, pairs (uploaded without accel) and shade (always)
    // The reference's walk records (DevScene::walk's comment, rt_internal.h),
    // + 64 B of zero padding read at the end: DevScene::walk without accel,
    // walk_ref beside the accel records with it.
    std::vector<Vec4> walk;
    std::vector<int>  slot_node;         // slots + 1: a slot's node, -1 on a pad slot and a leaf's second slot
    std::vector<int>  node_slot;         // end + 1: slot(i), then the slot count
    int  slots = 0;                      // the reference records' slots, pad slots included
    bool padded = false;                 // they hold pad slots (leaf_align)
    // Option accel (accel_build.h): the records every device gets and what
    // DevScene takes from the build; without it (option accel 0, or a scene
    // too large for one layout) has_accel is false and the rest unused.
    bool has_accel = false;
    std::vector<uint32_t> accel_rec;
    int   n_layouts = 0, layout_slots = 0, half = 0, wide = 0, root_enter = 0, root_first_leaf = 0;
    int   accel_root_leaf = 0;
    float relax_half = 0.0f;
    // Option refit: keep = the scene holds rt_update_geometry's tables, front =
    // rt_update_geometry_device's too; refit = the tables' bytes, and the
    // context's side (rt_ctx::refit_*).
    bool keep = false, front = false;
    RefitLayout rl;
    std::vector<uint8_t> refit;
    std::vector<uint8_t> refit_links;
    std::vector<int32_t> refit_dups;
    std::vector<int>     refit_level_first, refit_front_first;
};

// Returns RT_OK, or RT_ERR_BAD_SCENE with a message in *err.
int plan_scene(const void* vertices, size_t vertex_bytes, const void* materials, size_t material_bytes,
               const void* bvh_nodes, size_t bvh_bytes, const PlanOptions& opt, ScenePlan* out, std::string* err);

}  // namespace rtamd
