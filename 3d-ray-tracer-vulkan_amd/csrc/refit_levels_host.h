// refit_levels_host.h — the level table of rt_update_geometry_device (rtamd.h
// option "refit_device"), free of HIP so that it also compiles
// into a stand-alone host program (tools/refit_levels_check.cpp).
//
// The reference's tree is in preorder: an internal node's left child is the
// next node and its right child a later one, so one reverse pass knows every
// node's height (a leaf's is 0) and a counting sort groups the nodes by it.
// A level's boxes are then the unions of boxes of lower levels only: one
// launch per level, lowest first, and no lane waits for another.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rtamd {

constexpr int kRefitMaxLevels = 1024;   // a taller tree (a hand-made chain) gets no tables: one launch per level

// ref_info: per node of the root's subtree [0, n_ref), a leaf's triangle (>= 0) or -(right child + 1)
// (RefitTables::ref_info).  by_height: the n_ref nodes, leaves first, then height 1, ...; level_first: where
// each height starts in it, n_levels + 1 entries.  False (both outputs empty) for a tree of more than
// kRefitMaxLevels levels or a right child that is not a later node of the subtree.
inline bool refit_levels(const int32_t* ref_info, size_t n_ref, std::vector<int32_t>* by_height,
                         std::vector<int>* level_first) {
    by_height->clear();
    level_first->assign(1, 0);
    if (n_ref == 0) return true;
    std::vector<int32_t> height(n_ref);
    int top = 0;
    for (size_t k = n_ref; k-- > 0;) {
        if (ref_info[k] >= 0) { height[k] = 0; continue; }
        const size_t right = (size_t)(-((int64_t)ref_info[k] + 1));
        if (k + 1 >= n_ref || right <= k + 1 || right >= n_ref) { level_first->assign(1, 0); return false; }
        const int h = 1 + (height[k + 1] > height[right] ? height[k + 1] : height[right]);
        if (h >= kRefitMaxLevels) { level_first->assign(1, 0); return false; }
        height[k] = h;
        if (h > top) top = h;
    }
    std::vector<int> first((size_t)top + 2, 0);
    for (size_t k = 0; k < n_ref; ++k) ++first[(size_t)height[k] + 1];
    for (int h = 1; h <= top + 1; ++h) first[h] += first[h - 1];
    by_height->resize(n_ref);
    std::vector<int> at(first.begin(), first.end() - 1);
    for (size_t k = 0; k < n_ref; ++k) (*by_height)[(size_t)at[height[k]]++] = (int32_t)k;
    *level_first = first;
    return true;
}

}  // namespace rtamd
