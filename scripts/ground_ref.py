"""The ground segmentation of csrc/ground.h (icpmi_ground_segment) restated in numpy: fp64, unfused, in the header's
order, so that labels, height, ground_z and the counts can be compared byte for byte.  The only step that is not
exact arithmetic is atan2, whose last ulp may differ between libraries; it matters only for a row whose
angle / sector_size lies within an ulp of an integer, so segment() also reports the smallest distance of any binned
row's quotient to an integer (the sector margin) and the tests keep their fixtures away from zero."""
import numpy as np

OBSTACLE, GROUND, IGNORED = 0, 1, 2
MAX_BINS = 20400

DEFAULTS = dict(n_rings=80, n_sectors=180, min_range=0.5, max_range=80.5, sensor_height=1.73, max_slope=0.15,
                step_tol=0.1, height_tol=0.2, clear_min=0.3, clear_max=2.0)


class GroundResult:
    def __init__(self, labels, height, ground_z, n_ground, n_obstacle, n_ignored, bins_accepted, sector_margin):
        self.labels, self.height, self.ground_z = labels, height, ground_z
        self.n_ground, self.n_obstacle, self.n_ignored = n_ground, n_obstacle, n_ignored
        self.bins_accepted, self.sector_margin = bins_accepted, sector_margin

    def counts(self):
        return (self.n_ground, self.n_obstacle, self.n_ignored, self.bins_accepted)


def check(cfg):
    """the cases icpmi_ground_segment refuses with ICPMI_ERR_ARG"""
    c = dict(DEFAULTS, **cfg)
    f = [c[k] for k in ("min_range", "max_range", "sensor_height", "max_slope", "step_tol", "height_tol", "clear_min",
                        "clear_max")]
    if not np.all(np.isfinite(f)):
        raise ValueError("a field is not finite")
    if c["n_rings"] < 1 or c["n_sectors"] < 1 or c["n_rings"] * c["n_sectors"] > MAX_BINS:
        raise ValueError("bad grid")
    if c["min_range"] < 0 or not c["max_range"] > c["min_range"]:
        raise ValueError("bad range")
    if c["max_slope"] < 0 or c["step_tol"] < 0 or c["height_tol"] < 0 or c["clear_max"] < c["clear_min"]:
        raise ValueError("bad tolerance")
    return c


def bins_of(xyz, c):
    """-> (bin per row, -1 where the row enters none; angle / sector_size per row)"""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    nr, ns = c["n_rings"], c["n_sectors"]
    ring_size = (np.float64(c["max_range"]) - np.float64(c["min_range"])) / np.float64(nr)
    sector_size = np.float64(2.0) * np.float64(3.14159265358979323846) / np.float64(ns)
    with np.errstate(all="ignore"):
        rng = np.sqrt(x * x + y * y)
        angle = np.arctan2(y, x) + np.float64(3.14159265358979323846)
        inside = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & ~(rng < c["min_range"]) & ~(rng > c["max_range"])
        qr = (rng - np.float64(c["min_range"])) / ring_size
        qs = angle / sector_size
    ok_r, ok_s = inside & (qr < nr), inside & (qs < ns)
    ring = np.where(ok_r, np.where(ok_r, qr, 0.0).astype(np.int64), nr - 1)      # (int) truncates; the clamp
    sector = np.where(ok_s, np.where(ok_s, qs, 0.0).astype(np.int64), ns - 1)
    ring, sector = np.maximum(ring, 0), np.maximum(sector, 0)
    return np.where(inside, ring * ns + sector, -1), qs


def segment(xyz, **cfg):
    c = check(cfg)
    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
    nr, ns = c["n_rings"], c["n_sectors"]
    ring_size = (np.float64(c["max_range"]) - np.float64(c["min_range"])) / np.float64(nr)
    b, qs = bins_of(xyz, c)
    binned = b >= 0
    z = xyz[:, 2]
    # the least z per bin on the order-preserving integer image of the double (sc_encode): -0.0 lies below +0.0
    bits = z[binned].view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    keys = np.where(bits >= top, ~bits, bits | top)
    kmin = np.full(nr * ns, ~np.uint64(0))
    np.minimum.at(kmin, b[binned], keys)
    filled = kmin != ~np.uint64(0)
    zmin = np.where(kmin >= top, kmin & ~top, ~kmin).view(np.float64)
    ground_z = np.empty(nr * ns)
    accepted = 0
    for s in range(ns):
        gz, gr = -np.float64(c["sensor_height"]), np.float64(0.0)
        for r in range(nr):
            e = r * ns + s
            if filled[e]:
                rc = np.float64(c["min_range"]) + (np.float64(r) + np.float64(0.5)) * ring_size
                lim = np.float64(c["step_tol"]) + np.float64(c["max_slope"]) * (rc - gr)
                if np.abs(zmin[e] - gz) <= lim:
                    gz, gr = zmin[e], rc
                    accepted += 1
            ground_z[e] = gz
    height = np.full(len(xyz), np.nan)
    height[binned] = z[binned] - ground_z[b[binned]]
    labels = np.full(len(xyz), IGNORED, dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        g = binned & (height <= c["height_tol"])
        o = binned & ~g & (c["clear_min"] <= height) & (height <= c["clear_max"])
    labels[g], labels[o] = GROUND, OBSTACLE
    margin = float(np.min(np.abs(qs[binned] - np.rint(qs[binned])))) if binned.any() else float("inf")
    return GroundResult(labels, height, ground_z, int(g.sum()), int(o.sum()), int(len(xyz) - g.sum() - o.sum()), accepted,
                        margin)
