"""Motion compensation (deskew) of a scan in its sensor frame through the C ABI (icpmi_deskew, csrc/deskew.h): a
spinning sensor measures row i at tau_i in [0, 1] of its sweep while it moves by the twist xi = (omega, v) per sweep, and
the row becomes Exp((tau_i - t_ref) xi) p_i -- the scan as a sensor standing at the pose of t_ref would have seen it.  Not
in the reference, which takes every scan as a snapshot.  The odometry drivers (odometry.run_odometry_device,
LocalMapOdometry, run_odometry_local_map, slam.run_slam) take `deskew=DeskewConfig(...)` and deskew each frame with
twist_from_delta(previous delta); scripts/deskew_ref.py restates all of it on the CPU."""
import ctypes as C

import numpy as np

from . import capi

TIMES, AZIMUTH = capi.DESKEW_TIMES, capi.DESKEW_AZIMUTH


class DeskewConfig:
    """icpmi_deskew_config; the defaults are icpmi_deskew_config_default's (a zero twist, t_ref 0.5, counter-clockwise from
    -pi), except that time_source None means: TIMES where times are given, AZIMUTH where not."""

    def __init__(self, twist=None, t_ref=None, time_source=None, direction=None, azimuth_start=None):
        c = capi.DeskewConfig()
        capi.load_library().icpmi_deskew_config_default(C.byref(c))
        self.twist = np.array(c.twist[:]) if twist is None else np.asarray(twist, dtype=np.float64).reshape(6).copy()
        self.t_ref = c.t_ref if t_ref is None else t_ref
        self.time_source = time_source
        self.direction = c.direction if direction is None else direction
        self.azimuth_start = c.azimuth_start if azimuth_start is None else azimuth_start

    def with_twist(self, twist):
        """a copy with another twist: what the drivers make per frame"""
        return DeskewConfig(twist, self.t_ref, self.time_source, self.direction, self.azimuth_start)

    def to_c(self, have_times=False):
        c = capi.DeskewConfig()
        for i, v in enumerate(np.asarray(self.twist, dtype=np.float64).reshape(6)):
            c.twist[i] = v
        c.t_ref, c.direction, c.azimuth_start = self.t_ref, int(self.direction), self.azimuth_start
        c.time_source = (TIMES if have_times else AZIMUTH) if self.time_source is None else int(self.time_source)
        return c


def twist_from_delta(delta):
    """icpmi_deskew_twist: the SE(3) log (omega, v) of a relative pose (4 x 4) -- the twist of the next sweep under constant
    velocity, from this frame's delta.  A pure host function: no context, no device."""
    T = np.ascontiguousarray(delta, dtype=np.float64)
    if T.shape != (4, 4):
        raise ValueError("expected a 4 x 4 transform")
    out = np.zeros(6)
    lib = capi.load_library()
    rc = lib.icpmi_deskew_twist(capi._dp(T), capi._dp(out))
    if rc != capi.OK:
        raise capi.IcpError(rc, lib.icpmi_last_error(None).decode())
    return out


def deskew(ctx, xyz, times=None, config=None):
    """The rows of xyz (N x 3 fp64, host memory) moved into the sensor frame at config.t_ref.  times: N doubles in [0, 1],
    or None for times from the rows' azimuths.  config None: the defaults (a zero twist: every row passes through)."""
    cfg = (config if config is not None else DeskewConfig()).to_c(times is not None)
    return ctx.deskew(xyz, times, cfg)


def split_frame(frame):
    """a driver's frame is `points` or `(points, times)` -> (points, times or None)"""
    if isinstance(frame, (tuple, list)) and len(frame) == 2 and np.ndim(frame[0]) == 2:
        return frame[0], frame[1]
    return frame, None


def frame_twist(delta_prev):
    """the drivers' rule: the twist of the previous frame's delta, zero for the first frames (None)"""
    return np.zeros(6) if delta_prev is None else twist_from_delta(delta_prev)


def deskew_frame(ctx, frame, config, delta_prev):
    """one frame of a driver on host memory -> (deskewed rows, the twist used)"""
    pts, times = split_frame(frame)
    twist = frame_twist(delta_prev)
    return deskew(ctx, pts, times, config.with_twist(twist)), twist

