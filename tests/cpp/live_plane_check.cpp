// Host check of the live plane's growth arithmetic (csrc/live_plane.h), built with the host compiler by
// tests/test_live_plane_math.py.  Drives (straight, diagonal, outward spiral, random walk) at R = 0, 40, 200 and 4096,
// from sensor cells of both signs and next to +-(2^31 - 2 - R - 6), are fed window by window to live_plane_grow, and
// after every step the four conditions are checked:
//     containment       the new box holds the old box and the window
//     one-sided growth  a side the window did not cross has not moved
//     geometric growth  the cells moved so far (the old box's, at every step that changed the box) are at most 4 x
//                       the current box's
//     no new refusals   the box fits 32-bit extents and stays within the cells a window can reach
// for as long as ray_plan accepts the drive, that is while the exact union of the windows holds at most 2^31 - 1 cells
// with the raster's margin ((W + 10) (H + 10)); containment and one-sidedness also beyond.  Then two spans on one row at
// R = 0, one whose exact union just fits 2^31 - 1 cells and one whose union does not: the plane refuses neither (the
// second is ray_plan's to refuse) and gives both the same slack.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "live_plane.h"

using icpmi::LiveBox;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (failures++ < 20) {                        \
                std::printf("FAIL %s: ", #cond);          \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

// ray_plan's test on a box of w x h cells
static bool fits(int64_t w, int64_t h) { return (w + 10) <= 2147483647LL / (h + 10); }

static bool holds(const LiveBox &b, const LiveBox &in)
{
    return in.x0 >= b.x0 && in.y0 >= b.y0 && in.x0 + in.w <= b.x0 + b.w && in.y0 + in.h <= b.y0 + b.h;
}

struct Drive {
    const char *name;
    int R;
    int64_t limit;          // the largest sensor cell in magnitude
    LiveBox box, exact;     // the plane's box; the exact union of the windows
    long double moved = 0;  // cells copied so far
    int moves = 0, legal_moves = 0, steps = 0;

    Drive(const char *n, int r) : name(n), R(r), limit(2147483646LL - r - 6) {}

    void step(int64_t sx, int64_t sy)
    {
        sx = std::max(-limit, std::min(limit, sx));
        sy = std::max(-limit, std::min(limit, sy));
        const LiveBox win = icpmi::live_window(sx, sy, R), old = box;
        box = icpmi::live_plane_grow(old, win);
        ++steps;
        if (exact.w == 0) exact = win;
        else {
            const int64_t x0 = std::min(exact.x0, win.x0), y0 = std::min(exact.y0, win.y0);
            const int64_t x1 = std::max(exact.x0 + exact.w, win.x0 + win.w), y1 = std::max(exact.y0 + exact.h, win.y0 + win.h);
            exact = LiveBox{x0, y0, x1 - x0, y1 - y0};
        }
        CHECK(holds(box, win), "%s R=%d step %d: the window", name, R, steps);
        if (old.w == 0) {
            CHECK(box.x0 == win.x0 && box.y0 == win.y0 && box.w == win.w && box.h == win.h, "%s R=%d: the first box is the window", name, R);
            return;
        }
        CHECK(holds(box, old), "%s R=%d step %d: the old box", name, R, steps);
        if (win.x0 >= old.x0) CHECK(box.x0 == old.x0, "%s R=%d step %d: -x moved", name, R, steps);
        if (win.y0 >= old.y0) CHECK(box.y0 == old.y0, "%s R=%d step %d: -y moved", name, R, steps);
        if (win.x0 + win.w <= old.x0 + old.w) CHECK(box.x0 + box.w == old.x0 + old.w, "%s R=%d step %d: +x moved", name, R, steps);
        if (win.y0 + win.h <= old.y0 + old.h) CHECK(box.y0 + box.h == old.y0 + old.h, "%s R=%d step %d: +y moved", name, R, steps);
        if (box.x0 != old.x0 || box.y0 != old.y0 || box.w != old.w || box.h != old.h) {
            moved += (long double)old.w * (long double)old.h;
            ++moves;
        }
        if (!fits(exact.w, exact.h)) return;   // ray_plan refuses the drive from here on
        legal_moves = moves;
        CHECK(moved <= 4.0L * (long double)box.w * (long double)box.h, "%s R=%d step %d: %.0Lf cells moved, box %lld x %lld", name, R,
              steps, moved, (long long)box.w, (long long)box.h);
        CHECK(box.w <= INT32_MAX && box.h <= INT32_MAX, "%s R=%d step %d: extents", name, R, steps);
        CHECK(box.x0 >= -icpmi::kLiveCellMax && box.x0 + box.w - 1 <= icpmi::kLiveCellMax && box.y0 >= -icpmi::kLiveCellMax &&
                  box.y0 + box.h - 1 <= icpmi::kLiveCellMax,
              "%s R=%d step %d: cells out of reach", name, R, steps);
    }
};

static int run_drives(int R, int64_t ox, int64_t oy, int dirx, int diry, unsigned seed)
{
    // dirx, diry: the way the drives head (towards the limit when the origin is next to it)
    const int64_t s = R / 3 + 7;
    const int N = 400;
    int moves = 0;
    {
        Drive d("straight", R);
        for (int k = 0; k < N; ++k) d.step(ox + dirx * k * s, oy);
        moves += d.moves;
        CHECK(d.legal_moves >= 3 && d.legal_moves <= 20, "straight R=%d: %d moves", R, d.legal_moves);   // log_1.5 of the span
    }
    {
        Drive d("diagonal", R);
        for (int k = 0; k < N; ++k) d.step(ox + dirx * k * s, oy + diry * k * s);
        moves += d.moves;
        CHECK(d.legal_moves >= 3 && d.legal_moves <= 20, "diagonal R=%d: %d moves", R, d.legal_moves);
    }
    {
        Drive d("spiral", R); // square and outward: legs of 1, 1, 2, 2, 3, 3, ... steps, turning left
        int64_t x = ox, y = oy;
        int dx = dirx, dy = 0, k = 0;
        for (int leg = 1; k < N; ++leg)
            for (int turn = 0; turn < 2 && k < N; ++turn) {
                for (int i = 0; i < leg && k < N; ++i, ++k) d.step(x += dx * 2 * s, y += dy * 2 * s);
                const int t = dx;
                dx = -dy, dy = t;
            }
        moves += d.moves;
        CHECK(d.legal_moves >= 4 && d.legal_moves <= 40, "spiral R=%d: %d moves", R, d.legal_moves);
    }
    {
        Drive d("random walk", R);
        std::mt19937_64 rng(seed);
        std::uniform_int_distribution<int64_t> u(-3 * s, 3 * s);
        int64_t x = ox, y = oy;
        for (int k = 0; k < 4 * N; ++k) d.step(x += u(rng), y += u(rng));
        moves += d.moves;
    }
    return moves;
}

int main()
{
    int drives = 0, moves = 0;
    unsigned seed = 1;
    for (int R : {0, 40, 200, 4096}) {
        const int64_t limit = 2147483646LL - R - 6, s = R / 3 + 7;
        moves += run_drives(R, -150 * s, -150 * s, 1, 1, seed++);            // from negative cells into positive ones
        moves += run_drives(R, 150 * s, 90 * s, -1, -1, seed++);             // and back
        moves += run_drives(R, limit - 200 * s, limit - 200 * s, 1, 1, seed++);   // into the corner of the largest cells
        moves += run_drives(R, -limit + 200 * s, -limit + 200 * s, -1, -1, seed++);
        moves += run_drives(R, limit - 3, -limit + 5, -1, 1, seed++);         // starting next to the limits
        drives += 20;
    }
    // at 2^31 - 1 cells, R = 0 (3 x 3 windows on one row): (W + 10) * 13 <= 2^31 - 1 <=> W <= 165,191,039
    {
        CHECK(fits(165191039, 3) && !fits(165191040, 3), "the fit test");
        LiveBox b = icpmi::live_plane_grow(LiveBox{}, icpmi::live_window(0, 0, 0));
        b = icpmi::live_plane_grow(b, icpmi::live_window(149999998, 0, 0));          // the need is more than the slack
        CHECK(b.x0 == -1 && b.w == 150000001 && b.y0 == -1 && b.h == 3, "one long step: %lld + %lld", (long long)b.x0, (long long)b.w);
        // the exact union is 165,191,039 wide and just fits; the slack (half of 150,000,001, rounded up) goes past it
        const LiveBox just = icpmi::live_plane_grow(b, icpmi::live_window(165191036, 0, 0));
        CHECK(just.x0 == -1 && just.w == 150000001 + 75000001 && just.y0 == -1 && just.h == 3, "the union that just fits: %lld",
              (long long)just.w);
        // one cell more: ray_plan refuses these frames; the plane's rule does not, and does not change
        const LiveBox over = icpmi::live_plane_grow(b, icpmi::live_window(165191037, 0, 0));
        CHECK(over.x0 == just.x0 && over.w == just.w && over.h == 3, "the union that does not fit: %lld", (long long)over.w);
        const LiveBox left = icpmi::live_plane_grow(b, icpmi::live_window(-15191035, 0, 0));    // the same on the other side
        CHECK(left.x0 == -1 - 75000001 && left.x0 + left.w == 150000000 && left.h == 3, "left: %lld + %lld", (long long)left.x0,
              (long long)left.w);
        const LiveBox far = icpmi::live_plane_grow(b, icpmi::live_window(400000000, 0, 0));     // a need past the slack: exact
        CHECK(far.x0 == -1 && far.x0 + far.w == 400000002, "far: %lld", (long long)far.w);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok %d drives, %d moves\n", drives, moves);
    return 0;
}
