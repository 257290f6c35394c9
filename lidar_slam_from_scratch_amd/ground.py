"""Ground segmentation of a scan in its sensor frame through the C ABI (icpmi_ground_segment, csrc/ground.h): a polar
grid of minimum heights, a walk outward along each sector that follows the ground while it stays within a slope, and a
label per row: OBSTACLE (within the clearance band over the ground), GROUND or IGNORED.  Not in the reference, which
names it as future work (README.md:304).  GlobalMap.set_ground feeds the occupancy products with the OBSTACLE rows;
scripts/ground_ref.py restates the labelling on the CPU."""
import ctypes as C

import numpy as np

from . import capi

OBSTACLE, GROUND, IGNORED = capi.GROUND_OBSTACLE, capi.GROUND_GROUND, capi.GROUND_IGNORED
MAX_BINS = capi.GROUND_MAX_BINS
_FIELDS = [name for name, _ in capi.GroundConfig._fields_]


class GroundConfig:
    """icpmi_ground_config; the defaults are icpmi_ground_config_default's"""

    def __init__(self, **kw):
        c = capi.GroundConfig()
        capi.load_library().icpmi_ground_config_default(C.byref(c))
        for name in _FIELDS:
            setattr(self, name, getattr(c, name))
        for name, v in kw.items():
            if name not in _FIELDS:
                raise TypeError("GroundConfig has no field %r" % name)
            setattr(self, name, v)

    def to_c(self):
        c = capi.GroundConfig()
        for name in _FIELDS:
            setattr(c, name, getattr(self, name))
        return c

    def as_dict(self):
        return {name: getattr(self, name) for name in _FIELDS}


class GroundSegmentation:
    """labels (uint8 per row), height (h per row, NaN for a row that entered no bin), ground_z (n_rings x n_sectors) and
    the counts of icpmi_ground_info"""

    def __init__(self, labels, height, ground_z, info):
        self.labels, self.height, self.ground_z = labels, height, ground_z
        self.n_ground, self.n_obstacle, self.n_ignored = info.n_ground, info.n_obstacle, info.n_ignored
        self.bins_accepted = info.bins_accepted

    def counts(self):
        return (self.n_ground, self.n_obstacle, self.n_ignored, self.bins_accepted)


def ground_segment(ctx, cloud, config=None, device_ptr=None, n_rows=None):
    """Label the rows of `cloud` (N x 3 fp64, host memory), or the n_rows rows at device_ptr.  config None: the
    defaults.  Returns a GroundSegmentation."""
    cfg = (config if config is not None else GroundConfig()).to_c()
    lib = capi.load_library()
    if device_ptr is None:
        pts = capi._f64(cloud) if len(cloud) else np.zeros((0, 3))
        n = pts.shape[0]
    else:
        n = int(n_rows)
    labels = np.empty(n, dtype=np.uint8)
    height = np.empty(n)
    ground_z = np.empty((max(cfg.n_rings, 0), max(cfg.n_sectors, 0)))
    info = capi.GroundInfo()
    args = (n, C.byref(cfg), labels.ctypes.data_as(C.POINTER(C.c_uint8)), capi._dp(height), capi._dp(ground_z), C.byref(info))
    if device_ptr is None:
        ctx._check(lib.icpmi_ground_segment(ctx._h, capi._dp(pts), *args))
    else:
        ctx._check(lib.icpmi_ground_segment_device(ctx._h, C.c_void_p(device_ptr), *args))
    return GroundSegmentation(labels, height, ground_z, info)
