// temporal_motion_host.h — the host-side decisions of the temporal history
// across a geometry update (rtamd.h rt_temporal_motion_device and option
// "temporal_motion"), free of HIP so that they also compile
// into a stand-alone host program: the vertex-buffer argument checks, and the
// bookkeeping of the copy of the previous vertex records.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rtamd {

constexpr size_t kMotionMaxTris = (size_t)1 << 29;

// Why rt_temporal_motion_device refuses its vertex arguments (a printf format taking the function's name),
// or null: both buffers null is the static call and never refused here.  Alignment and overlaps are
// check_buffers' business.
inline const char* temporal_motion_args_error(const void* verts_cur, const void* verts_prev, bool have_prev_frame,
                                              size_t n_tris) {
    if (!verts_cur && !verts_prev) return nullptr;
    if (!verts_cur || !verts_prev) return "%s: d_verts_cur and d_verts_prev must be both null or both given";
    if (!have_prev_frame) return "%s: vertex buffers without a previous frame";
    if (n_tris == 0 || n_tris > kMotionMaxTris) return "%s: n_tris must be in [1, 2^29]";
    return nullptr;
}

// What one device keeps between the calls.  staged: the refit staging array holds the scene's current vertex
// records (after an upload with the option on, and after every update).  pending: an update kept the
// history since the last temporal frame, and the copy holds the records as that frame's hit buffer saw them.
struct MotionBook {
    bool staged = false;
    bool pending = false;

    void on_upload(bool records_staged) { staged = records_staged; pending = false; }
    void on_history_dropped() { pending = false; }

    // An accepted rt_update_geometry, before it overwrites the staging array.  Returns whether the history
    // stays; *copy: the staging array must first be copied to the previous-records buffer (the first update
    // since the last temporal frame only, so that several updates between two frames keep that frame's state).
    bool on_update(bool option, size_t n_devices, bool history_valid, size_t n_tris, size_t n_nodes, bool* copy) {
        const bool keep = option && n_devices == 1 && history_valid && staged && n_tris != 0 && n_nodes != 0;
        *copy = keep && !pending;
        pending = keep;
        return keep;
    }
    void after_update(size_t n_tris) { staged = n_tris != 0; }

    // A temporal frame: false (and the mark cleared) when a kept history meets the option turned off, which
    // drops the history.  history_valid: after the frame's own drop rules.
    bool frame_keeps_history(bool option) const { return !(pending && !option); }
    // Whether the frame runs the MOTION kernel; clears the mark either way.
    bool take_frame(bool history_valid) {
        const bool motion = history_valid && pending;
        pending = false;
        return motion;
    }
};

}  // namespace rtamd
