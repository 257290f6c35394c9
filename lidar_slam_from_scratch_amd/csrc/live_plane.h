// live_plane.h -- how the live count plane (live_counts.h) grows.  Host only: no HIP, so that
// tests/cpp/live_plane_check.cpp compiles it with the host compiler alone.
// The plane is a dense box of cells that has to hold the (2R + 3)^2 window around the sensor cell of every frame
// cast into it.  A frame whose window leaves the box makes the box grow; the old words are then moved by one device
// copy, so how often and by how much it grows decides what a drive pays in copies.  live_plane_grow keeps:
//     containment       the new box holds the old box and the window
//     one-sided growth  a side moves only if the window crossed it
//     geometric growth  a crossed side moves by at least half the box's extent on that axis, so a move that gets its
//                       slack multiplies the box's area by at least 3/2, and the cells copied by all such moves sum
//                       to at most 2x the final box.  Only the end of the cells a window can reach, +-kLiveCellMax,
//                       cuts a slack short; a move stopped there touches that limit.  The used frames' own box holds
//                       at most 2^31 - 1 cells (ray_plan), the plane's extents are less than three times its, and a
//                       box touching both limits of an axis would be 2^32 cells wide: at most one such move per axis,
//                       each copying at most the final box.  4x in all, over any drive ray_plan accepts.
//     no new refusals   nothing is refused here, and the slack is not held to ray_plan's 2^31 - 1 cells: the plane is
//                       indexed with 64-bit offsets and may pass them.  (Giving up the slack at that size instead
//                       cannot keep the bound above: a box with its slack to the north-east that is then crossed
//                       step by step on its west side would be copied whole at every step.)  What the slack costs is
//                       memory: at most 3/2 of the used frames' own extent on an axis the drive moves one way along,
//                       and less than 3x on one whose two sides it crosses in turn (a side's slack is at most half
//                       of the own extent plus the other side's slack).
#pragma once
#include <stdint.h>

#include <algorithm>

namespace icpmi {

// the farthest cell a window reaches: a sensor cell is at most 2^31 - 2 - R - 6 in magnitude, its window R + 1 more
constexpr int64_t kLiveCellMax = 2147483646LL - 6 + 1;

struct LiveBox {     // cells [x0, x0 + w) x [y0, y0 + h); w == 0: no box yet
    int64_t x0 = 0, y0 = 0, w = 0, h = 0;
};

// the window of a frame whose sensor cell is (sx, sy)
inline LiveBox live_window(int64_t sx, int64_t sy, int R) { return LiveBox{sx - R - 1, sy - R - 1, 2 * (int64_t)R + 3, 2 * (int64_t)R + 3}; }

inline bool live_box_holds(const LiveBox &b, const LiveBox &win)
{
    return b.w > 0 && win.x0 >= b.x0 && win.y0 >= b.y0 && win.x0 + win.w <= b.x0 + b.w && win.y0 + win.h <= b.y0 + b.h;
}

// One axis: the old extent [lo, hi) and the window's [wlo, whi) -> the new extent, with slack on the crossed sides.
inline void live_axis_grow(int64_t lo, int64_t hi, int64_t wlo, int64_t whi, int64_t &nlo, int64_t &nhi)
{
    const int64_t half = (hi - lo + 1) / 2;
    nlo = lo, nhi = hi;
    if (wlo < lo) nlo = std::max<int64_t>(std::min(wlo, lo - half), -kLiveCellMax);
    if (whi > hi) nhi = std::min<int64_t>(std::max(whi, hi + half), kLiveCellMax + 1);
}

// The box after a frame with window `win` (live_window(sx, sy, R)) is cast into a plane of box `old`.
inline LiveBox live_plane_grow(const LiveBox &old, const LiveBox &win)
{
    if (old.w == 0) return win;
    if (live_box_holds(old, win)) return old;
    int64_t x0, x1, y0, y1;
    live_axis_grow(old.x0, old.x0 + old.w, win.x0, win.x0 + win.w, x0, x1);
    live_axis_grow(old.y0, old.y0 + old.h, win.y0, win.y0 + win.h, y0, y1);
    return LiveBox{x0, y0, x1 - x0, y1 - y0};
}

} // namespace icpmi
