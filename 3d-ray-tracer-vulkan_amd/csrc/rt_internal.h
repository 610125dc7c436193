// rt_internal.h — shared declarations of the gfx950 path-trace backend.
//
// Device layout of a scene (laid out on the host once per rt_upload_scene, by
// plan_scene of scene_plan.cpp, from the reference's 48-B node / 48-B vertex /
// 16-B material records):
//
//   nodes : 2 x float4 per node (32 B), in the reference's preorder
//           [0] = (bbox_min.xyz, skip | L(skip) << 31)
//           [1] = (bbox_max.xyz, L(i+1) | L(i) << 1)
//           skip = first node after this subtree; L(j) = "node j is a leaf".
//           The left child of an internal node i is i+1 (BVHFlattener.java:51-75:
//           myIndex = currentNodeIndex++ and the left subtree is flattened
//           first), so the reference's stack DFS (compute_dynamic_ray.comp:185-210:
//           push right, push left) visits nodes in preorder, skipping the
//           subtree of every node whose box test fails.  "next = hit ? i+1 :
//           skip" replays exactly that visit sequence with no stack at all, and
//           the L bits tell a walker whether the node it moves to is a leaf, so
//           it fetches that leaf's triangle together with the node (one memory
//           round trip per visit).
//   leafs : 3 x float4 per NODE index (48 B; meaningful at leaves only)
//           [0] = (v0.xyz, triangle index) [1] = (e1.xyz, 0) [2] = (e2.xyz, 0)
//           e1 = v1-v0, e2 = v2-v0 are the values hit_triangle computes
//           (compute_dynamic_ray.comp:106-107), evaluated once on the host in
//           IEEE binary32: the same bits.
//   pairs : 4 x float4 per NODE index (64 B; meaningful at internal nodes only):
//           the boxes of both children of node i and where they are
//           [0] = (L.min.xyz, R.min.x) [1] = (L.max.xyz, R.min.y)
//           [2] = (R.max.xyz, R.min.z) [3] = (R | L(R) << 31, L(i+1), skip(i), 0)
//           with L = i+1 and R = the right child.  The frontier walk (heavy
//           pixels, option coop_walk 1) expands a hit internal node by
//           loading this one record and testing both children's boxes.
//   norms : 1 x float4 per flattened triangle: normalize(cross(e1,e2)) (:124),
//           likewise precomputed; read once per hit when shading.
//   mats  : 1 x float4 per flattened triangle (albedo.rgb, type)
#pragma once
#include <cstdint>
#include <cstddef>
#include <hip/hip_runtime.h>

#include "../../include/rtamd.h"
#include "rng_table_host.h"
#include "scene_plan.h"      // kShadeStride, kRefitStatusWords

namespace rtamd {

struct DevScene {
    int      n_nodes = 0;     // nodes in the compact array
    int      end     = 0;     // traversal ends when the node index reaches this (= skip of root)
    int      n_tris  = 0;
    int      root_leaf = 0;   // L(0)
    float    root_box[6] = {0, 0, 0, 0, 0, 0};   // node 0's min.xyz, max.xyz (kernel argument)
    float4*  nodes   = nullptr;
    float4*  leafs   = nullptr;
    float4*  pairs   = nullptr;
    // walk 2's records (the lockstep walk and the cooperative tail), 32-B
    // slots: the reference's preorder with every leaf's triangle inlined after
    // its box.  An internal node takes one slot, (min.xyz, skip slot |
    // L(skip) << 31), (max.xyz, L(i+1) | L(i) << 1); a leaf two, (min.xyz,
    // triangle index | 1 << 30 | L(i+1) << 31), (max.xyz, v0.x), then
    // (v0.yz, e1.xy), (e1.z, e2.xyz).  slot(i) = i + the leaves before i, so
    // an internal node's left child (i+1) is the next slot and a leaf's
    // successor (its skip, i+1) the slot after its two: only the internal
    // skip is stored.  A leaf visit reads its node and triangle from one
    // 64-B run (they were two arrays), sibling leaves sit side by side, and
    // the records take 32 B per node + 32 B per leaf instead of 64 B per node
    // (config 5: 100 MB instead of 134 MB).  Bit 30 of word [0].w is L(i) for
    // every node.  end2 = the slots; slot_node = the node index of a node's
    // first slot (the frontier tail's hand-off), -1 on a leaf's second slot.
    float4*  walk    = nullptr;
    int*     slot_node = nullptr;
    int*     node_slot = nullptr;   // slot(i) of node i (walk 0 hands its node index to the windows tail)
    int      end2    = 0;
    int      padded  = 0;   // 1: the walk records hold pad slots (leaf_align)
    // Option accel (accel_build.h): walk = the accel records,
    // n_layouts (1 or 8) layouts of layout_slots slots each (end2 = their
    // total, end = layout_slots), and the reference's walk records beside
    // them for the fallback (a segment whose hit lies before its own box's
    // t_enter is walked again in the reference's order): walk_ref, end2_ref
    // slots (pad slots as `ref_padded`).  n_layouts 0: no accel.
    int      n_layouts = 0;
    int      layout_slots = 0;
    int      wide = 0;          // accel format 2: the 4-wide tree, 64-B records (end2 = records)
    int      half = 0;          // accel format 1: 16-B slots, half-precision internal boxes (accel_build.h);
                                //   layout_slots and end2 then count 16-B slots
    float    relax_half = 0.0f;  // format 1: every internal node's margin factor (AccelHost::relax_max)
    int      root_enter = 0;     // format 0: the walk starts inside the root (its slab test skipped)
    int      root_first_leaf = 0;   // bit o: layout o's root's first child is a leaf
    int      oct_mask = 7;       // 8 layouts: a ray walks layout (its octant & oct_mask) (option accel_octants)
    float4*  walk_ref = nullptr;
    int      end2_ref = 0;
    int      ref_padded = 0;
    // norms and mats interleave in one allocation (kShadeStride float4 per
    // triangle: normal, then albedo/type), so shading a hit touches one 32-B
    // record; norms points at the allocation, mats one float4 in
    float4*  norms   = nullptr;
    float4*  mats    = nullptr;
    // extension kExtSpheres: 2 x float4 per sphere (centre.xyz, radius),
    // (albedo.rgb, type); n_spheres is 0 unless the extension is on
    const float4* spheres = nullptr;
    int      n_spheres = 0;
};

struct Counters {               // device-side work counters (see rt_stats)
    unsigned long long segments;
    unsigned long long node_visits;
    unsigned long long tri_tests;
    unsigned long long mat_reads;
};

struct CamF {                   // the four vec3 of the CameraUBO
    float ox, oy, oz;
    float lx, ly, lz;
    float hx, hy, hz;
    float vx, vy, vz;
};

// Non-reference extensions (option "extensions", off by
// default, kernel 0 only).  The reference has none of them (SURVEY.md §0 facts
// 3-4); oracle/rt_oracle.h ORC_EXT_* states the same semantics.
constexpr int kExtSkyToggle = 1;    // a miss is black when sky_enabled == 0
constexpr int kExtEmissive = 2;     // a type-3 hit ends the path with attenuation * albedo
constexpr int kExtAccumulate = 4;   // seed += frame_count*W*H; output sqrt(mean of linear colour)
constexpr int kExtSpheres = 8;      // spheres (rt_upload_spheres) after the BVH walk, in index order
constexpr int kExtNewSample = 16;   // seed += frame_count*W*H as kExtAccumulate moves it, and nothing else

constexpr int kMaxBatch = 16;  // frames per launch (rt_render_batch_device)

// A split launch's queue header (TraceArgs::q_hdr): a 128-B line per queue.
constexpr int kQHdrWords = 32;
constexpr int kQCount = 0;     // entries claimed (failed claims included)
constexpr int kQLimit = 1;     // ~(the lowest failed claim's base), 0 = no claim failed
constexpr int kQTicket = 2;    // kernel-2 waves of the queue that have read the header
constexpr int kMaxSplitQueues = 1024;   // option split_queues

struct TraceArgs {
    DevScene scene;
    CamF     cams[kMaxBatch] = {}; // frame f of the batch is seen through cams[f]
    int      n_frames = 0;      // frames in the launch (1..kMaxBatch): the same rows of each
    int      tiles_y = 0;       // wave-tile rows per frame (launcher-internal: ceil(th / tile height))
    int      width = 0, height = 0; // full frame
    int      max_bounces = 0;
    int      x0 = 0, y0 = 0, tw = 0, th = 0; // columns [x0, x0+tw); th local rows per frame
    // Local row ly is frame row y0 + ((ly / band_h) * band_stride + band_off) * band_h + ly % band_h:
    // a plain tile is band_h = th, band_stride = 1, band_off = 0; rank r of N
    // interleaved 16-row bands is band_h = 16, band_stride = N, band_off = r.
    // With band_list (device, nullable) it is band_list[ly / band_h] * band_h + ly % band_h; with
    // list_stride > 0 frame f reads its own list at band_list + f * list_stride, whose -1 entries
    // (trailing padding) and rows past the frame are not traced.
    int      band_h = 0, band_stride = 1, band_off = 0;
    const int* band_list = nullptr;
    // Outputs: n_frames x th x tw pixels, frame f's local row ly at row f * th + ly
    uchar4*  out_rgba = nullptr; // nullable
    float*   out_rad = nullptr; // 3 floats per pixel, nullable
    Counters* counters = nullptr; // nullable
    int      wave_tile = 0;     // wave tile (8<<s) x (8>>s), s in 0..3
    unsigned long long* diag = nullptr; // diagnostics: 8 words per wave, or null
    int      coop_lanes = 0;    // finish a wave's walks cooperatively once at most
                                //   this many lanes are still walking (0 = never)
    int      solo_lanes = 0;    // format-0 accel walk without the cooperative tail: once at most this many
                                //   lanes of a wave are still walking, their walks are finished one ray at a
                                //   time through the scalar cache (solo_walk, rt_trace.hip; 0 = never)
    int      ext = 0;           // non-reference extensions, kExt* bits (0 = the reference)
    int      sky_enabled = 1;   // CameraUBO.sky_enabled (@68), read only with kExtSkyToggle
    int      frame_count = 0;   // CameraUBO.frame_count (@64), read only with kExtAccumulate / kExtNewSample
    float*   accum = nullptr;   // kExtAccumulate: running linear-colour sums, 3 floats per pixel (tw*th)
    int      walk = 0;          // 0 = one node per step (nodes/leafs), 2 = the same software-pipelined
                                //   over the compact records (nodes2/leafs2; default)
    int      block_waves = 0;   // waves per workgroup, 4 (256 threads) or 1 (64 threads)
    const int* tile_order = nullptr; // block_waves 1: workgroup k traces wave tile tile_order[k] (or k)
    int      tiles_x = 0;       // with tile_order (1-D grid): wave tiles per tile row
    int      split_n = 0;       // with tile_order: the first split_n tiles of the order are traced
                                //   one pixel per wave (64 workgroups each; launcher-internal)
    int      heavy_tiles = 0;   // with tile_order: the first heavy_tiles tiles run in that split
                                //   mode as a concurrent launch on aux_stream (fork ev_fork, join ev_join)
    int      heavy_fused = 0;   // with heavy_tiles: 1 = the heavy tiles' one-pixel workgroups come
                                //   first in the same launch (option heavy_stream 2), no aux stream
    const int* heavy_px = nullptr; // fused, with tile_order: heavy pixels (tile * 64 + lane), traced one
    int      n_heavy_px = 0;    //   per wave by the first n_heavy_px workgroups of the launch
    const unsigned long long* tile_mask = nullptr; // per tile: the lanes (heavy pixels) its tile wave skips, or null
    unsigned* diag_lane = nullptr; // learning launch: each pixel's walk length (64 per wave), or null
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int      coop_walk = 0;     // cooperative tail: 0 = 64-node preorder windows (coop_walk),
                                //   1 = preorder frontier (frontier_walk)
    int      coop_win = 64;     // coop_walk's window: 64 or 32 slots (option coop_window)
    int      list_stride = 0;   // band_list per frame: frame f's at band_list + f * list_stride
                                //   (0 = one list for every frame of the launch)
    const int* row_off = nullptr;   // per frame: its first output row (null: f * th); device memory
    // Split launch (options split_bounce / split_pixels, accel walk; DESIGN.md
    // §4b): a kernel-1 wave with n paths still alive at bounce split_bounce
    // claims n entries (3 float4 each) of queue (its dispatch index mod
    // q_queues) with one atomic add on the queue's count and writes them in
    // lane order; a claim past q_cap leaves the paths with the wave and
    // records its base in the queue's limit.  Kernel 2, one wave per pack of
    // 64 entries, finishes the entries below min(count, limit, q_cap); the
    // last of a queue's q_packs waves to draw its ticket zeroes the header.
    // q_slots null: one kernel.
    int      split_bounce = 0;
    float4*  q_slots = nullptr;     // q_queues x q_cap entries
    unsigned* q_hdr = nullptr;      // kQHdrWords per queue (kQCount, kQLimit, kQTicket), zero between launches
    unsigned* q_overflow = nullptr; // waves whose claim did not fit (option split_overflow)
    int      q_queues = 0;
    int      q_cap = 0;             // entries per queue, a multiple of 64 (0: every claim fails)
    unsigned long long q_pixels = 0;    // the launch's pixels: an entry's pixel index is below it
    int      q_packs = 0;           // kernel 2's waves per queue: max(1, q_cap / 64)
    int      q_spare = 0;
    // Query launch (launch_query; rtamd.h rt_query_rays_device, rt_render_hits_device):
    // lane i % 64 of wave i / 64 walks ray i of ray_in (2 float4 per rt_ray: origin.xyz, t_max;
    // dir.xyz, reserved), or with ray_in null the primary ray of its pixel, once, and writes its
    // rt_hit (2 float4: t, tri, normal.xy; normal.z, pos.xyz) to hit_out.  Appended after every
    // field the render kernels read, so their argument offsets are the ones they always had.
    const float4* ray_in = nullptr;
    float4*  hit_out = nullptr;
    int      any_hit = 0;       // RT_QUERY_ANY: a lane's walk stops at its first consistent hit
    // Samples launch (rtamd.h rt_render_samples_device): a batch launch whose frames are
    // consecutive samples of one camera.  Both fields are read by the extension builds only (kFeatExt code),
    // and follow every field the other kernels read.
    int      sample_step = 0;   // frame f of the launch seeds with frame_count + f * sample_step (0: every
                                //   frame with frame_count, as always)
    float*   out_lin = nullptr; // when set, the end of a path stores its linear colour (finish_pixel's fin,
                                //   before the sqrt) as 3 floats where out_rad would put the pixel, and
                                //   neither out_rgba nor out_rad is written
    // The table of scatter draws (option rng_table; rng_table_host.h): rng_k planes of width x height
    // float4 entries, read by the kFeatRng kernels only, which a launch takes exactly when rng_k > 0.  Below
    // bounce rng_k such a path keeps its first seed y * width + x, which indexes every plane, where the other
    // kernels keep the running seed; the entry read at bounce rng_k - 1 hands over the running seed.
    // Behind every field the other kernels read, like the fields above.
    const float4* rng_table = nullptr;
    int      rng_k = 0;
};

// A learning launch's walk length of a pixel traced by a one-pixel heavy wave
// (its lockstep length is unknown there): above any real length, so it stays
// among the heavy pixels (rt_learn.hip).
constexpr unsigned kLearnHeavyMark = 0x3FFFFFFFu;

// Device-side heavy-first learning (rt_learn.hip): the order, heavy pixels and
// tile masks from a learning launch's diagnostic records, computed on the
// stream that ran it, with no host synchronisation.
struct LearnParams {
    int      n;              // tiles of the launch (records at rec_off + t, pixels at t * 64 + lane)
    int      rec_off;        // heavy-pixel waves ahead of the tile records (a fused launch in an order)
    int      learn_cost;     // 0 = lockstep steps + 2 x windows, 1 = wave duration
    int      order_split;    // percent (0 = every tile by cost)
    // heavy-pixel bar = heavy_pixel_factor / 100.0 x ((total steps x concurrent) / resident), evaluated
    // on the device in double in that order: learn_order's px_bar bit for bit
    int      heavy_pixel_factor;   // percent
    int      concurrent;     // launches of similar work in flight (>= 1)
    int      resident;       // resident trace waves of the device (>= 1)
    int      cap;            // at most this many heavy pixels
    // option xcd_order (> 0, n a multiple of 8): tile_order position k runs on
    // XCD k % 8 (workgroups are dealt round-robin); XCD c gets the c-th eighth
    // of the tiles in the order of (row class, row, frame, column), a row's
    // class being (row / xcd) % 8, still most expensive first within it.
    // Rows are the launch's own tile rows: on a band or list launch the rows
    // of its bands packed one after another, not the frame's.  A launch whose
    // tile count is no multiple of 8 keeps the plain order (learn_xcd_applies
    // says which; rt_learn_copy reports it), and an order learned on the host
    // is never grouped
    int      xcd = 0;
    int      tiles_x = 0, tiles_y = 0, frames = 0;
};
struct LearnScratch;         // device scratch (rt_learn.hip)
size_t learn_scratch_bytes(int n);
bool learn_xcd_applies(const LearnParams& lp);   // whether learn_on_device groups the order by XCD
// Enqueues on stream s: writes d_order (n tile indices, most expensive first),
// d_mask (n lane masks), d_hpix (<= cap heavy pixels, tile * 64 + lane, most
// expensive first) and *d_nhpix (their count).  scratch: learn_scratch_bytes(n).
hipError_t learn_on_device(const LearnParams& lp, const unsigned long long* rec, const unsigned* lane,
                           void* scratch, int* d_order, unsigned long long* d_mask, int* d_hpix, int* d_nhpix,
                           hipStream_t s);

// Kernel launcher (rt_trace.hip).  *kernels (nullable) = the kernels it
// enqueued (2 when the heavy tiles run as a launch of their own).
hipError_t launch_trace(const TraceArgs& a, hipStream_t stream, int* kernels = nullptr);

// The query launch (rt_trace.hip): a.scene is the accel format-0 scene or a
// reference-records scene (n_layouts 0); tw x th rays (th 1, wave_tile 3 for a
// ray batch) in a 1-D grid of one-wave workgroups.  One kernel, no learned
// order, no heavy pixels.
hipError_t launch_query(const TraceArgs& a, hipStream_t stream);

void set_error(const char* fmt, ...);

// rt_rngtable.hip: enqueues the kernel that fills the table of scatter draws (rng_table_host.h:
// rng_table_bytes(width, height, k) bytes at `table`) on `stream`.
hipError_t launch_rng_table(float4* table, int width, int height, int k, hipStream_t stream);

// rt_wire.hip: the RGB wire format of the multi-GPU exchange (n_px pixels;
// rgba 16-B aligned, rgb 4-B aligned).
hipError_t wire_pack(const void* rgba, void* rgb, size_t n_px, hipStream_t s);
hipError_t wire_unpack(const void* rgb, void* rgba, size_t n_px, hipStream_t s);

// rt_filter.hip: an a-trous filter's passes (rtamd.h rt_denoise_device,
// rt_denoise_albedo_device, rt_denoise_history_device and
// rt_denoise_variance_device), enqueued on `stream`; validated arguments, nothing allocated.
enum FilterKind { kFilterRadiance = 0, kFilterHistory = 1, kFilterVariance = 2 };
struct FilterArgs {
    FilterKind    kind;
    int           width, height;
    const float*  radiance;     // Radiance: the render's radiance, 3 floats per pixel (else null)
    const float4* hist;         // History, Variance: (c.rgb, n) per pixel (else null)
    const float2* mom;          // Variance: (m1, m2) per pixel (else null)
    const float4* hits;         // rt_hit records, 2 float4 per pixel
    float4*       workspace;    // 2 x width x height float4: a pass's records
    uchar4*       out_rgba;     // nullable
    float*        out_rad;      // nullable
    int           iterations, normal_power_log2;
    int           min_history;  // Variance
    float         sigma_depth;
    float         tolerance;    // Radiance, History: 1.0f / sigma_color, computed in float on the host;
                                //   Variance: sigma_lum
    int           form;         // option denoise_kernel: 0 = the measured choice per step, 1 = plain, 2 = tiled
                                //   (Variance: tiled at step 1 alone)
    int           only_pass;    // option denoise_pass: -1 = every pass (Variance: behind the estimate),
                                //   i = pass i alone (timing)
    int           stage;        // Variance, option variance_stage: -1 = everything, 0 = the estimate alone (timing)
    // Radiance on the illumination (rtamd.h rt_denoise_albedo_device): the albedo buffer,
    // (d.rgb, any) per pixel; null = the colour is filtered as it is
    const float4* albedo = nullptr;
};
hipError_t launch_filter(const FilterArgs& d, hipStream_t stream);
// The first-hit albedo buffer (rtamd.h rt_albedo_device): out[p] = (d.rgb, type) of the
// flattened triangle hits[p] names among the scene's n_flat material records `mats` (kShadeStride float4
// apart), (1, 1, 1, -1) where it names none; px pixels.
hipError_t launch_albedo(const float4* hits, const float4* mats, unsigned n_flat, float4* out, size_t px,
                         hipStream_t stream);

// rt_temporal.hip: the temporal accumulation's one kernel (rtamd.h
// rt_temporal_device and rt_temporal_moments_device),
// enqueued on `stream`; validated arguments, nothing allocated.
struct TemporalBasis {          // rt_temporal_camera_basis's 13 floats
    float ox, oy, oz;           // origin
    float nx, ny, nz;           // N = cross(horizontal, vertical)
    float ax, ay, az;           // A = cross(vertical, a), a = lower_left - origin
    float bx, by, bz;           // B = cross(a, horizontal)
    float det;                  // dot(a, N)
};
struct TemporalArgs {
    int           width, height;
    const float*  radiance;     // the render's radiance, 3 floats per pixel
    const float4* hits;         // rt_hit records, 2 float4 per pixel
    const float4* hist_prev;    // (c.rgb, n) per pixel, or null: no history
    const float4* hits_prev;    // the previous frame's rt_hit records (null with hist_prev)
    TemporalBasis cur, prev;
    float         plane_tol, normal_min, max_history;   // max_history as a float (1..1024: exact)
    float4*       hist_out;
    uchar4*       out_rgba;     // nullable
    float*        out_rad;      // nullable
    int           form;         // option temporal_tile: 0 = the shipped form, 1 = 64 x 1 waves, 2 = 16 x 4
    // the luminance moments (m1, m2) per pixel beside the history: mom_out null = none are kept;
    // mom_prev is null exactly when hist_prev is
    const float2* mom_prev;
    float2*       mom_out;
};
// rt_temporal_motion_device: the vertex records, 3 float4 per flattened triangle, as the
// frame's hit records saw them and as the previous frame's did.  A kernel argument of its own behind the
// others, so that the kernels without it keep their argument layout.
struct TemporalMotion {
    const float4* verts_cur = nullptr;
    const float4* verts_prev = nullptr;
    unsigned      n_tris = 0;       // 1..2^29: a hit record whose tri is not below it has no history
};
// motion null: the kernels of §4h and §4j
hipError_t launch_temporal(const TemporalArgs& t, hipStream_t stream, const TemporalMotion* motion = nullptr);

// rt_samples.hip: folds the linear-colour frames of one samples launch into
// the running sum, in frame order (rtamd.h rt_render_samples_device, DESIGN.md
// §4k), enqueued on `stream`; validated arguments, nothing allocated.
struct SamplesArgs {
    size_t        n_px;         // pixels of a frame
    const float*  slices;       // n_slices frames of 3 * n_px floats, one after another
    int           n_slices;     // 1..kMaxBatch
    int           load_sum;     // 1 = start from *sum, 0 = from slice 0 (sum is not read)
    float*        sum;          // 3 * n_px floats
    int           finish;       // 1 = the call's last chunk: also write the outputs
    float         divisor;      // finish: the samples in the sum, an exact float
    uchar4*       out_rgba;     // finish: nullable
    float*        out_rad;      // finish: nullable
    int           form;         // 0 = 16-byte accesses where every base and a frame's byte size allow them,
                                //   1 = the scalar form (one pixel per lane)
};
hipError_t launch_samples_resolve(const SamplesArgs& r, hipStream_t stream);

// rt_refit.hip: the scene's records recomputed in place from moved vertices
// (rtamd.h rt_update_geometry).  The tables are device arrays
// written at an upload with option refit 1; the two staging arrays are what a
// call copies in.
struct RefitTables {
    const float4* st_verts = nullptr;   // staging: the raw vertex records, 3 float4 per flattened triangle
    const float*  st_boxes = nullptr;   // staging: 6 floats per reference node (min.xyz, max.xyz)
    // the tables: sections of one byte blob laid out by scene_plan.cpp (RefitLayout names their offsets)
    int           n_ref = 0;            // reference nodes of the root's subtree (HostScene::end)
    int           n_tris = 0;           // flattened triangles
    const int*    ref_info = nullptr;   // per reference node: a leaf's triangle, or -(right child + 1)
    const int*    ref_slot = nullptr;   // per reference node: its slot in the reference's walk records
    // the accel tree (format 0): AccelHost's tables
    int           n_layouts = 0, n_canon = 0, n_prims = 0;
    const int*    prim = nullptr;       // 3 per kept primitive: triangle, reference leaf, canonical node
    const int*    child = nullptr;      // 2 per canonical node
    const uint32_t* slot = nullptr;     // n_layouts per canonical node: [o * n_canon + c]
    const int*    by_height = nullptr;  // the internal canonical nodes grouped by height, lowest first
    float4*       canon = nullptr;      // 2 per canonical node: (min.xyz, force bit), (max.xyz, 0)
};
struct RefitArgs {
    DevScene    scene;
    RefitTables t;
};
// Enqueues the three stages on `stream`; level_first: n_levels + 1 offsets into by_height (host memory).
hipError_t launch_refit(const RefitArgs& r, const int* level_first, int n_levels, hipStream_t stream);

// rt_update_geometry_device (option refit_device): rt_refit_scene restated on the device.
// The input triangles are read from device memory, checked, and staged into st_verts / st_boxes as the
// bytes rt_refit_scene writes; launch_refit then runs on the staged arrays as after a host update.
struct RefitFront {
    const void*     in = nullptr;        // n_in * 9 doubles (f32: floats): v0, v1, v2 of each input triangle
    const uint32_t* source = nullptr;    // flattened triangle f copies input triangle source[f]; null: f itself
    size_t          n_in = 0;
    int             f32 = 0;
    int             n_flat = 0;          // flattened triangles of the scene
    float4*         st_verts = nullptr;  // RefitTables' staging arrays
    float*          st_boxes = nullptr;
    const int*      ref_info = nullptr;  // RefitTables::ref_info
    const int*      by_height = nullptr; // the reference nodes of the root's subtree by height, leaves first
    const int*      dups = nullptr;      // 4 per dropped duplicate: its triangle and reference leaf, its keeper's
    int             n_dups = 0;
    unsigned*       status = nullptr;    // kRefitStatusWords words: the lowest offending flattened triangle per kind
};
// kRefitStatusWords (scene_plan.h) words: [0] a source entry >= n_in, [1] a cast that is not finite,
// [2] a dropped duplicate that no longer is one, [3] unused
// The check: reads the input only, and sets status (every word 0xFFFFFFFF where nothing offends).
hipError_t launch_refit_check(const RefitFront& f, hipStream_t stream);
// The stage kernel, the leaf boxes and one launch per level; level_first: n_levels + 1 offsets into by_height.
hipError_t launch_refit_front(const RefitFront& f, const int* level_first, int n_levels, hipStream_t stream);

}  // namespace rtamd
