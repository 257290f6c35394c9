"""A catalogue of calls on one context, for the call-order tests (tests/test_gpu_call_sequences.py) and for soaks.

The rule the catalogue holds the library to: what a call returns depends on its arguments and on the state
its documentation names, and on nothing else.  A call on a context that has done other things returns, byte for byte,
what it returns as the first call on a fresh context; the k-th step of a stateful object returns what it returns in the
object's undisturbed run.

  * An OPERATION (OPS) is a named call over fixed, seeded inputs: run(ctx, env) -> Out(digest, facts, raw).  `digest` is
    one hash of everything the call hands back (result fields, the error history, arrays, last_normal_matrix() right
    after a registration, debug_loop_rows, gate and robust info); `facts` is what must also agree ACROSS search engines
    (iteration counts, the convergence flag, matched indices); `raw` is what CHECKS holds to the CPU oracle and to the
    restatements in scripts/, so that the expected digests are not circular.  Nothing that is documented to accumulate
    is digested: get_profile, nn_reuse_passes, the stream's timing statistics.
  * A THREAD (THREADS) is a stateful object with its ordered steps: a generator over (ctx, env) that yields one digest
    per step and closes its object when it is closed.  `claims` names the context-wide state a thread owns while it
    runs: "stream" (the odometry stream's resident scans and settings: one per context) and "cells" (the context's
    occupancy set).  Two threads with a common claim cannot be interleaved on one context by the documentation itself,
    so shuffle_plan() runs them one after the other and interleaves everything else.

Sizes are the smallest that reach each form of a call (csrc/loop_plan.h, engine_for in capi.hip): see REGISTRATIONS.

As a program: a soak of shuffled sequences on one context, every digest against fresh contexts.
    python scripts/call_sequences.py --seeds 20 [--search auto|exact|mfma|pruned] [--profile 0|2]
"""
import argparse
import collections
import contextlib
import ctypes as C
import hashlib
import os
import re
import shutil
import sys
import tempfile
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from lidar_slam_from_scratch_amd import synth  # noqa: E402  (numpy only: the catalogue's inputs build without the library)

CSRC = os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc")
POSE_TOL_M, POSE_TOL_RAD, HIST_TOL = 1e-4, 1e-4, 1e-9     # tests/test_gpu_parity.py's check_against
DESKEW_LIB_TOL = 64.0 * 2.0 ** -52                        # tests/test_gpu_deskew.py's LIB_TOL (the device library's atan2)
HUBER, GEMAN_MCCLURE = 1, 2                               # capi.ROBUST_*

Out = collections.namedtuple("Out", "digest facts raw")


# ---------------------------------------------------------------------------------------------------------------- digests
def _bytes_of(p):
    if p is None:
        return b"\x00none"
    if isinstance(p, (bytes, bytearray)):
        return bytes(p)
    if isinstance(p, np.ndarray):
        a = np.ascontiguousarray(p)
        return ("%s%s" % (a.dtype.str, a.shape)).encode() + a.tobytes()
    if isinstance(p, C.Structure):
        return bytes(p)
    if isinstance(p, (bool, int, str)):
        return repr(p).encode()
    if isinstance(p, float):
        return np.float64(p).tobytes()
    if isinstance(p, (list, tuple)):
        return b"(" + b",".join(_bytes_of(e) for e in p) + b")"
    if isinstance(p, np.generic):
        return np.asarray(p).tobytes()
    raise TypeError("no digest of %r" % type(p))


def dig(*parts):
    h = hashlib.blake2b(digest_size=16)
    for p in parts:
        b = _bytes_of(p)
        h.update(len(b).to_bytes(8, "little"))
        h.update(b)
    return h.digest()


# ----------------------------------------------------------------------------------------------------------------- inputs
def _sweep_small(f):
    return synth.lidar_sweep(f, synth.accel_pose, beams=16, azimuths=600)


def build_inputs():
    """Every array the catalogue uses, from synth and default_rng alone: the same bytes at every call."""
    I = {}
    rng = np.random.default_rng(20251)
    # registrations (REGISTRATIONS): room corners for the exact and small-cloud paths, uniform boxes beyond
    s, t, _ = synth.c1_room_corner(1500)
    I["rc_s40"], I["rc_s1001"], I["rc_t1500"] = s[:40].copy(), s[:1001].copy(), t
    s, t, _ = synth.c1_room_corner(4500)
    I["rc_s3000"], I["rc_t4500"] = s[:3000].copy(), t
    s, t, _ = synth.c1_room_corner(300)
    I["rc_s300"], I["rc_t255"] = s, t[:255].copy()
    s, t, _ = synth.c3_uniform(16385, seed=14, perm_seed=15)
    I["u_s5000a"], I["u_t16385"] = s[:5000].copy(), t
    s, t, _ = synth.c3_uniform(24577, seed=16, perm_seed=17)
    I["u_s5000b"], I["u_t24577"] = s[:5000].copy(), t
    # primitives
    I["nn_t255"], I["nn_q513"] = rng.uniform(-50, 50, (255, 3)), rng.uniform(-50, 50, (513, 3))
    I["nn_t5000"], I["nn_q5000"] = rng.uniform(-50, 50, (5000, 3)), rng.uniform(-50, 50, (5000, 3))
    I["knn_12000"] = np.c_[rng.uniform(-30, 30, (12000, 2)), rng.uniform(-3, 5, 12000)]
    _, I["nrm_3000"], _ = synth.c1_room_corner(3000)
    I["p2p_s"] = rng.uniform(-20, 20, (4097, 3))
    I["p2p_t"] = I["p2p_s"] + rng.normal(0.0, 0.02, (4097, 3))
    nr = rng.normal(size=(4097, 3))
    I["p2p_n"] = nr / np.linalg.norm(nr, axis=1, keepdims=True)
    I["tf_T"] = synth.make_transform((0.3, -0.2, 0.7), (1.5, -2.5, 0.25))
    I["vox_shared"] = rng.uniform(-10, 10, (6000, 3))                       # voxel 2.0: 1,000 voxels of six rows
    g = np.stack(np.meshgrid(np.arange(20.0), np.arange(20.0), np.arange(15.0), indexing="ij"), axis=-1).reshape(-1, 3)
    I["vox_unique"] = (g + 0.25 + rng.uniform(-0.2, 0.2, g.shape))[rng.permutation(6000)]   # voxel 0.5: a voxel per row
    rec = np.zeros((4097, 4), dtype=np.float32)
    rec[:, :3] = rng.uniform(-80, 80, (4097, 3)).astype(np.float32)
    rec[:, 3] = rng.uniform(0, 1, 4097).astype(np.float32)
    I["f32_records"] = rec
    I["dk_xyz"], I["dk_tau"] = rng.uniform(-60, 60, (1025, 3)), rng.uniform(0.0, 1.0, 1025)
    w = rng.normal(size=3)
    I["dk_twist"] = np.r_[w * (0.05 / np.linalg.norm(w)), rng.normal(size=3) * 1.5]
    # 16 x 600 frames of the synthetic street: filtered (local map, global map, loop store, scan context) and raw
    for f in range(6):
        I["f16_%d" % f] = synth.lidar_frame(3 * f, beams=16, azimuths=600)
        I["p16_%d" % f] = synth.lidar_pose(3 * f)
        I["raw16_%d" % f] = synth.lidar_frame(f, voxel=0, beams=16, azimuths=600, **synth.DRIVE_200)
        I["world16_%d" % f] = synth.apply_transform(I["p16_%d" % f], I["f16_%d" % f])
    turn = synth.lidar_pose(0) @ synth.make_transform((0.0, 0.0, np.deg2rad(30.0)), (0.0, 0.0, 0.0))
    I["f16_revisit"] = synth.lidar_frame_at(turn, 77, beams=16, azimuths=600)      # frame 0's place, another heading
    I["ground_raw"] = synth.lidar_frame(2, voxel=0, beams=16, azimuths=600)
    for f in range(6):
        I["sweep16_%d" % f] = _sweep_small(f)[0]
    # stream A: 32 x 900 raw frames; stream B: 3,000 rows of each filtered frame (one cache key, eight contents)
    for f in range(8):
        raw = synth.lidar_frame(f, voxel=0, beams=32, azimuths=900, **synth.DRIVE_200)
        I["raw32_%d" % f] = raw
        filt = synth.voxel_centroids(raw, 0.5)
        if filt.shape[0] < 3000:
            raise RuntimeError("a filtered 32 x 900 frame has %d rows, stream B wants 3000" % filt.shape[0])
        I["b3000_%d" % f] = filt[np.sort(rng.choice(filt.shape[0], 3000, replace=False))].copy()
    I["b_tiny"] = I["b3000_3"][::6].copy()                                  # 500 rows: under min_points
    bad = I["b3000_4"].copy()
    bad[7, 1] = np.nan
    I["b_nan"] = bad
    # the pose graph: nine poses on a circle, noisy odometry, a closing edge and a chord
    ring = [synth.make_transform((0.0, 0.0, 2 * np.pi * k / 9), (10 * np.cos(2 * np.pi * k / 9), 10 * np.sin(2 * np.pi * k / 9), 0.1 * k))
            for k in range(9)]
    I["pg_ring"] = np.stack(ring)

    def noisy(rel):
        return rel @ synth.make_transform(rng.normal(0, 0.01, 3), rng.normal(0, 0.05, 3))
    I["pg_odom"] = np.stack([noisy(synth.invert_transform(ring[k]) @ ring[k + 1]) for k in range(8)])
    I["pg_close"] = noisy(synth.invert_transform(ring[8]) @ ring[0])
    I["pg_chord"] = noisy(synth.invert_transform(ring[4]) @ ring[0])
    I["pg_info"] = np.diag([4e4, 4e4, 4e4, 4e2, 4e2, 4e2]).astype(np.float64)
    for k in I:
        I[k] = np.ascontiguousarray(I[k])
        I[k].setflags(write=False)
    return I


def inputs_digest(I):
    return dig(*[(k, I[k]) for k in sorted(I)])


_INPUTS = None
_LOCK = threading.Lock()


def inputs():
    """built on the CPU once per process"""
    global _INPUTS
    with _LOCK:
        if _INPUTS is None:
            _INPUTS = build_inputs()
    return _INPUTS


class Env:
    """The inputs, their copies in device memory (torch, made on first use and never written) and the frame files."""

    def __init__(self):
        self.I = inputs()
        self._dev = {}
        self._lock = threading.Lock()
        self.tmp = tempfile.mkdtemp(prefix="call_sequences_")
        self.bin_paths = []
        for f in range(6):
            raw = self.I["raw16_%d" % f]
            rec = np.zeros((raw.shape[0], 4), dtype=np.float32)
            rec[:, :3] = raw
            path = os.path.join(self.tmp, "%06d.bin" % f)
            rec.tofile(path)
            self.bin_paths.append(path)

    def close(self):
        self._dev.clear()
        shutil.rmtree(self.tmp, ignore_errors=True)

    def dev(self, key):
        import torch
        with self._lock:
            if key not in self._dev:
                self._dev[key] = torch.from_numpy(np.array(self.I[key])).cuda()
                torch.cuda.synchronize()
            return self._dev[key]


def _sync():
    import torch
    torch.cuda.synchronize()


def _capi():
    from lidar_slam_from_scratch_amd import capi
    return capi


# ------------------------------------------------------------------------------------------------------------- operations
Op = collections.namedtuple("Op", "name rows kind run names claims reg")
OPS = collections.OrderedDict()
CHECKS = {}


def op(name, rows, kind, names, claims=(), reg=None):
    def deco(fn):
        OPS[name] = Op(name, rows, kind, fn, tuple(names), frozenset(claims), reg)
        return fn
    return deco


def check(name):
    def deco(fn):
        CHECKS[name] = fn
        return fn
    return deco


def _normal_matrix_parts(ctx, k=0):
    capi = _capi()
    try:
        nm = ctx.last_normal_matrix(k)
    except capi.IcpError as e:
        return [("no normal matrix", e.code)]
    return [nm.JtJ, nm.Jtb, nm.sum_sq, nm.weight, nm.pairs, nm.T]


def _reg_out(ctx, n_src, res, hist, extra, ruled=False):
    parts = [res, hist, extra] + _normal_matrix_parts(ctx)
    matches, valid = None, False
    if not ruled:       # (after a gated or weighted loop icpmi_debug_loop_rows refuses every row count: capi.hip, fill_result)
        idx, cur, perm, valid = ctx.debug_loop_rows(n_src)
        parts += [valid, perm, cur]
    if valid:
        parts.append(idx)
        matches = np.empty(n_src, dtype=np.int32)
        matches[perm] = idx                                   # row r of the loop is source row perm[r]
    facts = {"num_iterations": int(res.num_iterations), "converged": int(res.converged), "matches": matches}
    return Out(dig(*parts), facts, {"res": res, "hist": hist, "extra": extra})


# name -> (form, source, target, rule, iterations or None for a run to tolerance)
# Target sizes are split counts of 2,048 targets (kSplitTiles * kTile): 1 split, 3 splits with a ragged last, 9 splits
# (past the small-cloud kernel's 8: the all-pairs engine's general kernels), 13 splits (past kAutoCulledFrom = 12: AUTO
# takes the culled engine); 40 source rows are under kMfmaMinQueries = 64 and 255 targets under kMfmaMinTargets = 256,
# where AUTO takes the exact fp64 kernels.
GATE_RC, GATE_U_GENERAL, GATE_U_CULLED = 0.5, 0.5, 1.0      # each keeps some rows and drops some (the restatement's pairs)
HUBER_RULE = (HUBER, 0.05)
REGISTRATIONS = collections.OrderedDict([
    ("align_exact_40", ("align", "rc_s40", "rc_t1500", None, 3)),
    ("align_small_1001", ("align_device", "rc_s1001", "rc_t1500", None, 3)),
    ("align_small_3000", ("align", "rc_s3000", "rc_t4500", None, 3)),
    ("align_general_5000", ("align", "u_s5000a", "u_t16385", None, 3)),
    ("align_culled_5000", ("align_device", "u_s5000b", "u_t24577", None, 3)),
    ("align_tiny_target_300", ("align", "rc_s300", "rc_t255", None, 3)),
    ("align_exact_40_to_tolerance", ("align", "rc_s40", "rc_t1500", None, None)),
    ("align_small_1001_to_tolerance", ("align", "rc_s1001", "rc_t1500", None, None)),
    ("align_general_5000_to_tolerance", ("align_device", "u_s5000a", "u_t16385", None, None)),
    ("align_culled_5000_to_tolerance", ("align", "u_s5000b", "u_t24577", None, None)),
    ("gated_exact_40", ("align_gated", "rc_s40", "rc_t1500", GATE_RC, 3)),
    ("gated_small_3000", ("align_gated", "rc_s3000", "rc_t4500", GATE_RC, 3)),
    ("gated_general_5000", ("align_gated_device", "u_s5000a", "u_t16385", GATE_U_GENERAL, 3)),
    ("gated_culled_5000", ("align_gated", "u_s5000b", "u_t24577", GATE_U_CULLED, 3)),
    ("robust_exact_40", ("align_robust", "rc_s40", "rc_t1500", HUBER_RULE, 3)),
    ("robust_small_1001", ("align_robust", "rc_s1001", "rc_t1500", HUBER_RULE, 3)),
    ("robust_general_5000", ("align_robust_device", "u_s5000a", "u_t16385", HUBER_RULE, 3)),
    ("robust_culled_5000", ("align_robust", "u_s5000b", "u_t24577", HUBER_RULE, 3)),
])


def _cfg_kw(iters):
    return dict(max_iterations=50) if iters is None else dict(max_iterations=iters, tolerance=0.0, min_error=0.0)


def _make_registration(name, form, src, tgt, rule, iters):
    def run(ctx, env):
        capi = _capi()
        s, t = env.I[src], env.I[tgt]
        cfg = capi.Context.make_config(**_cfg_kw(iters))
        extra = []
        if form == "align":
            res, hist = ctx.align(s, t, cfg)
        elif form == "align_device":
            ds, dt = env.dev(src), env.dev(tgt)
            res, hist = ctx.align_device(ds.data_ptr(), ds.shape[0], dt.data_ptr(), dt.shape[0], cfg)
        elif form == "align_gated":
            res, hist, pairs = ctx.align_gated(s, t, cfg, rule)
            extra = [pairs]
        elif form == "align_gated_device":
            ds, dt = env.dev(src), env.dev(tgt)
            res, hist, pairs = ctx.align_gated_device(ds.data_ptr(), ds.shape[0], dt.data_ptr(), dt.shape[0], cfg, rule)
            extra = [pairs]
        elif form == "align_robust":
            res, hist, info = ctx.align_robust(s, t, cfg, rule)
            extra = [info]
        elif form == "align_robust_device":
            ds, dt = env.dev(src), env.dev(tgt)
            res, hist, info = ctx.align_robust_device(ds.data_ptr(), ds.shape[0], dt.data_ptr(), dt.shape[0], cfg, rule)
            extra = [info]
        else:
            raise ValueError(form)
        return _reg_out(ctx, s.shape[0], res, hist, extra, ruled=rule is not None)

    I = inputs()
    kind = "none" if rule is None else ("gate" if form.startswith("align_gated") else "robust")
    reg = {"n": I[src].shape[0], "m": I[tgt].shape[0], "rule": kind}
    names = (form, "last_normal_matrix") + (("debug_loop_rows",) if rule is None else ())
    op(name, max(reg["n"], reg["m"]), "registration", names, reg=reg)(run)

    @check(name)
    def _check(env, out, orc):
        s, t = env.I[src], env.I[tgt]
        kw = _cfg_kw(iters)
        kw.setdefault("tolerance", 1e-6)
        kw.setdefault("min_error", 1e-9)
        if kind == "none":
            ref = orc.icp_point_to_plane(s, t, nthreads=8, **kw)
        elif kind == "gate":
            import gated_icp_ref
            ref = gated_icp_ref.gated_icp(s, t, rule, orc=orc, **kw)
            assert out.raw["extra"][0] == ref.pairs, (name, out.raw["extra"][0], ref.pairs)
        else:
            import robust_icp_ref
            ref = robust_icp_ref.robust_icp(s, t, rule[0], rule[1], orc=orc, **kw)
        check_against(out.raw["res"], out.raw["hist"], ref.transformation, ref.converged, ref.num_iterations, ref.error_history)


def check_against(res, hist, ref_T, ref_conv, ref_iters, ref_hist):
    """tests/test_gpu_parity.py's, with its tolerances"""
    dt, dr = synth.pose_delta(np.array(res.transformation[:]).reshape(4, 4), ref_T)
    assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD, (dt, dr)
    assert bool(res.converged) == bool(ref_conv)
    assert res.num_iterations == int(ref_iters)
    assert len(hist) == len(ref_hist)
    np.testing.assert_allclose(hist, ref_hist, rtol=0, atol=HIST_TOL)
    assert res.final_error == hist[-1]


for _name, _spec in REGISTRATIONS.items():
    _make_registration(_name, *_spec)

BATCH = (("rc_s40", "rc_t1500"), ("rc_s1001", "rc_t1500"), ("rc_s3000", "rc_t4500"))


def _batch_out(ctx, runs):
    parts, iters = [], []
    for k, r in enumerate(runs):
        parts += [r[0], r[1], list(r[2:])] + _normal_matrix_parts(ctx, k)
        iters.append((int(r[0].num_iterations), int(r[0].converged)))
    return Out(dig(*parts), {"batch": iters}, {"runs": runs})


@op("align_batch_3", 4500, "registration", ("align_batch", "last_normal_matrix"))
def _align_batch(ctx, env):
    cfg = _capi().Context.make_config(**_cfg_kw(3))
    return _batch_out(ctx, ctx.align_batch([env.I[s] for s, _ in BATCH], [env.I[t] for _, t in BATCH], cfg))


@check("align_batch_3")
def _align_batch_check(env, out, orc):
    for (s, t), (res, hist) in zip(BATCH, out.raw["runs"]):
        ref = orc.icp_point_to_plane(env.I[s], env.I[t], nthreads=8, **_cfg_kw(3))
        check_against(res, hist, ref.transformation, ref.converged, ref.num_iterations, ref.error_history)


@op("gated_batch_2", 4500, "registration", ("align_gated_batch", "last_normal_matrix"))
def _gated_batch(ctx, env):
    cfg = _capi().Context.make_config(**_cfg_kw(3))
    return _batch_out(ctx, ctx.align_gated_batch([env.I[s] for s, _ in BATCH[1:]], [env.I[t] for _, t in BATCH[1:]], cfg, GATE_RC))


@op("robust_batch_2", 4500, "registration", ("align_robust_batch", "last_normal_matrix"))
def _robust_batch(ctx, env):
    cfg = _capi().Context.make_config(**_cfg_kw(3))
    rule = (GEMAN_MCCLURE, 0.1, GATE_RC)
    return _batch_out(ctx, ctx.align_robust_batch([env.I[s] for s, _ in BATCH[:2]], [env.I[t] for _, t in BATCH[:2]], cfg, rule))


# Plane-to-plane registrations (icp_gicp.h): the source's search structure and normals are built in front of the target's,
# in the buffers every other call's target uses -- what a used context could leak into, and out of.  (No `reg`: their
# plan is one form at every size, kRuleGicp, which tests/test_gicp_header.py holds; the paths' table above is the three
# older rules'.  The small form, ICPMI_GICP_FORM_SMALL, runs the small-cloud kernel's plane-to-plane expansion on the
# sorted normals and partial rows the gated small calls use: gicp_small_1001 and one problem of gicp_batch_2.)
GICP_RULE = (1e-3, GATE_RC)
GICP_RULE_SMALL = (1e-3, GATE_RC, True)


def _make_gicp(name, form, src, tgt, iters, rule=GICP_RULE):
    @op(name, max(inputs()[src].shape[0], inputs()[tgt].shape[0]), "registration", (form, "last_normal_matrix"))
    def run(ctx, env):
        s, t = env.I[src], env.I[tgt]
        cfg = _capi().Context.make_config(**_cfg_kw(iters))
        if form == "align_gicp":
            res, hist, info = ctx.align_gicp(s, t, cfg, rule)
        else:
            ds, dt = env.dev(src), env.dev(tgt)
            res, hist, info = ctx.align_gicp_device(ds.data_ptr(), ds.shape[0], dt.data_ptr(), dt.shape[0], cfg, rule)
        return _reg_out(ctx, s.shape[0], res, hist, [info], ruled=True)

    @check(name)
    def _check(env, out, orc):
        import gicp_ref
        kw = _cfg_kw(iters)
        ref = gicp_ref.gicp_icp(env.I[src], env.I[tgt], GICP_RULE[0], GICP_RULE[1], kw["max_iterations"], kw.get("tolerance", 1e-6),
                                kw.get("min_error", 1e-9), orc=orc)
        assert out.raw["extra"][0].pairs == ref.pairs, (name, out.raw["extra"][0].pairs, ref.pairs)
        check_against(out.raw["res"], out.raw["hist"], ref.transformation, ref.converged, ref.num_iterations, ref.error_history)


_make_gicp("gicp_1001", "align_gicp", "rc_s1001", "rc_t1500", 3)
_make_gicp("gicp_5000", "align_gicp_device", "u_s5000a", "u_t16385", 3)
_make_gicp("gicp_small_1001", "align_gicp", "rc_s1001", "rc_t1500", 3, GICP_RULE_SMALL)


@op("gicp_batch_2", 4500, "registration", ("align_gicp_batch", "last_normal_matrix"))
def _gicp_batch(ctx, env):
    cfg = _capi().Context.make_config(**_cfg_kw(3))
    rules = [GICP_RULE_SMALL, GICP_RULE]                 # (one problem in each form)
    return _batch_out(ctx, ctx.align_gicp_batch([env.I[s] for s, _ in BATCH[1:]], [env.I[t] for _, t in BATCH[1:]], cfg, rules))


@check("gicp_batch_2")
def _gicp_batch_check(env, out, orc):
    import gicp_ref
    kw = _cfg_kw(3)
    for (s, t), (res, hist, info) in zip(BATCH[1:], out.raw["runs"]):
        ref = gicp_ref.gicp_icp(env.I[s], env.I[t], GICP_RULE[0], GICP_RULE[1], kw["max_iterations"], kw.get("tolerance", 1e-6),
                                kw.get("min_error", 1e-9), orc=orc)
        assert info.pairs == ref.pairs, (s, info.pairs, ref.pairs)
        check_against(res, hist, ref.transformation, ref.converged, ref.num_iterations, ref.error_history)


# ---- primitives
def _nearest(name, tgt, qry):
    @op(name, max(inputs()[tgt].shape[0], inputs()[qry].shape[0]), "primitive", ("nearest_batch",))
    def run(ctx, env):
        idx, d2 = ctx.nearest_batch(env.I[tgt], env.I[qry])
        return Out(dig(idx, d2), {"idx": idx}, {"idx": idx, "d2": d2})

    @check(name)
    def _c(env, out, orc):
        oidx, od2 = orc.nearest_batch_brute(env.I[tgt], env.I[qry])
        assert (out.raw["idx"] == oidx).all() and (out.raw["d2"] == od2).all(), name


_nearest("nearest_513_255", "nn_t255", "nn_q513")
_nearest("nearest_5000_5000", "nn_t5000", "nn_q5000")


def _k_nearest(name, k):
    @op(name, 12000, "primitive", ("k_nearest",))
    def run(ctx, env):
        idx, d2 = ctx.k_nearest(env.I["knn_12000"], env.I["knn_12000"], k)
        return Out(dig(idx, d2), {"idx": idx}, {"idx": idx, "d2": d2})

    @check(name)
    def _c(env, out, orc):
        pts = env.I["knn_12000"]
        idx, d2 = out.raw["idx"], out.raw["d2"]
        for i in range(pts.shape[0]):
            want = orc.k_nearest_brute(pts, pts[i], k)
            assert (idx[i] == want).all(), (name, i)
        e = pts[idx] - pts[:, None, :]
        assert (((e[..., 0] ** 2 + e[..., 1] ** 2) + e[..., 2] ** 2) == d2).all(), name


_k_nearest("k_nearest_20", 20)
_k_nearest("k_nearest_40", 40)          # beyond 32 neighbours: the exact kernel


def _normals(name, key):
    @op(name, inputs()[key].shape[0], "primitive", ("estimate_normals",))
    def run(ctx, env):
        nrm = ctx.estimate_normals(env.I[key], 20)
        return Out(dig(nrm), None, {"nrm": nrm})

    @check(name)
    def _c(env, out, orc):
        assert (out.raw["nrm"] == orc.estimate_normals(env.I[key], None, 20, nthreads=8)).all(), name


_normals("normals_3000", "nrm_3000")
_normals("normals_24577", "u_t24577")


@op("normals_rows_middle", 16385, "primitive", ("estimate_normals_rows",))
def _normals_rows(ctx, env):
    nrm = ctx.estimate_normals_rows(env.I["u_t16385"], 20, 6001, 9000)
    return Out(dig(nrm), None, {"nrm": nrm})


@check("normals_rows_middle")
def _normals_rows_check(env, out, orc):
    assert (out.raw["nrm"] == orc.estimate_normals_rows(env.I["u_t16385"], 6001, 9000, None, 20, nthreads=8)).all()


@op("solve_point_to_plane", 4097, "primitive", ("solve_point_to_plane",))
def _solve(ctx, env):
    T = ctx.solve_point_to_plane(env.I["p2p_s"], env.I["p2p_t"], env.I["p2p_n"])
    return Out(dig(T), None, {"T": T})


@check("solve_point_to_plane")
def _solve_check(env, out, orc):
    want = orc.solve_point_to_plane(env.I["p2p_s"], env.I["p2p_t"], env.I["p2p_n"])
    np.testing.assert_allclose(out.raw["T"], want, rtol=0, atol=1e-12)       # (test_solve_point_to_plane's: the order of sums differs)


@op("transform_4097", 4097, "primitive", ("transform_points",))
def _transform(ctx, env):
    out = ctx.transform_points(env.I["tf_T"], env.I["p2p_s"])
    return Out(dig(out), None, {"out": out})


@check("transform_4097")
def _transform_check(env, out, orc):
    T, p = env.I["tf_T"], env.I["p2p_s"]
    for r in range(3):
        assert (out.raw["out"][:, r] == ((p[:, 0] * T[r, 0] + p[:, 1] * T[r, 1]) + p[:, 2] * T[r, 2]) + T[r, 3]).all()


def _voxel(name, key, voxel, shared):
    @op(name, 6000, "primitive", ("voxel_downsample",))
    def run(ctx, env):
        rows = ctx.voxel_downsample(env.I[key], voxel)
        return Out(dig(rows), None, {"rows": rows})

    @check(name)
    def _c(env, out, orc):
        rows = out.raw["rows"]
        assert (rows.shape[0] == 6000) == (not shared) and rows.shape[0] <= 6000, (name, rows.shape)
        want = orc.voxel_downsample(env.I[key], voxel)
        assert rows.shape == want.shape and (rows == want).all(), name


_voxel("voxel_many_per_voxel", "vox_shared", 2.0, True)
_voxel("voxel_one_per_voxel", "vox_unique", 0.5, False)


@op("voxel_device", 6000, "primitive", ("voxel_downsample_device",))
def _voxel_device(ctx, env):
    import torch
    d_in = env.dev("vox_shared")
    d_out = torch.full_like(d_in, 7.0)
    _sync()
    n = ctx.voxel_downsample_device(d_in.data_ptr(), d_in.shape[0], 1.0, d_out.data_ptr(), d_in.shape[0])
    _sync()
    rows = d_out[:n].cpu().numpy()
    return Out(dig(n, rows), None, {"rows": rows})


@check("voxel_device")
def _voxel_device_check(env, out, orc):
    want = orc.voxel_downsample(env.I["vox_shared"], 1.0)
    assert out.raw["rows"].shape == want.shape and (out.raw["rows"] == want).all()


@op("upload_points_f32", 4097, "primitive", ("upload_points_f32",))
def _upload(ctx, env):
    import torch
    rec = env.I["f32_records"]
    d_out = torch.full((rec.shape[0], 3), 7.0, dtype=torch.float64, device="cuda")
    _sync()
    ctx.upload_points_f32(rec, d_out.data_ptr())
    _sync()
    rows = d_out.cpu().numpy()
    return Out(dig(rows), None, {"rows": rows})


@check("upload_points_f32")
def _upload_check(env, out, orc):
    assert (out.raw["rows"] == env.I["f32_records"][:, :3].astype(np.float64)).all()


@op("load_cloud_device", 9600, "primitive", ("load_cloud_device_rows", "load_cloud_device"))
def _load(ctx, env):
    import torch
    n = ctx.load_cloud_device_rows(env.bin_paths[0])
    d_out = torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda")
    _sync()
    got = ctx.load_cloud_device(env.bin_paths[0], d_out.data_ptr(), n)
    _sync()
    rows = d_out.cpu().numpy()
    return Out(dig(n, got, rows), None, {"rows": rows})


@check("load_cloud_device")
def _load_check(env, out, orc):
    assert (out.raw["rows"] == env.I["raw16_0"].astype(np.float32).astype(np.float64)).all()


def _deskew_cfg(env, source, direction=1):
    from lidar_slam_from_scratch_amd import deskew
    return deskew.DeskewConfig(env.I["dk_twist"], time_source=source, direction=direction).to_c(True)


@op("deskew_times_1025", 1025, "primitive", ("deskew",))
def _deskew_times(ctx, env):
    out = ctx.deskew(env.I["dk_xyz"], env.I["dk_tau"], _deskew_cfg(env, _capi().DESKEW_TIMES))
    return Out(dig(out), None, {"out": out})


@check("deskew_times_1025")
def _deskew_times_check(env, out, orc):
    import deskew_ref
    want = deskew_ref.deskew(env.I["dk_xyz"], env.I["dk_twist"], env.I["dk_tau"])
    assert np.array_equal(out.raw["out"].view(np.uint64), want.xyz.view(np.uint64))


@op("deskew_azimuth_1025", 1025, "primitive", ("deskew",))
def _deskew_azimuth(ctx, env):
    out = ctx.deskew(env.I["dk_xyz"], None, _deskew_cfg(env, _capi().DESKEW_AZIMUTH))
    return Out(dig(out), None, {"out": out})


@check("deskew_azimuth_1025")
def _deskew_azimuth_check(env, out, orc):
    import deskew_ref
    xyz, twist = env.I["dk_xyz"], env.I["dk_twist"]
    want = deskew_ref.deskew(xyz, twist, None)
    scale = np.linalg.norm(xyz, axis=1) + np.linalg.norm(twist[3:])
    # (times from the device library's atan2: tests/test_gpu_deskew.py's bound for the library branches, per coordinate)
    assert (np.abs(out.raw["out"] - want.xyz).max(axis=1) <= DESKEW_LIB_TOL * scale).all()


@op("deskew_device_in_place", 1025, "primitive", ("deskew_device",))
def _deskew_device(ctx, env):
    d_xyz, d_tau = env.dev("dk_xyz").clone(), env.dev("dk_tau")
    _sync()
    ctx.deskew_device(d_xyz.data_ptr(), d_tau.data_ptr(), d_xyz.shape[0], _deskew_cfg(env, _capi().DESKEW_TIMES), d_xyz.data_ptr())
    _sync()
    out = d_xyz.cpu().numpy()
    return Out(dig(out), None, {"out": out})


CHECKS["deskew_device_in_place"] = _deskew_times_check


@op("scan_context_4", 3000, "primitive", ("scan_context", "scan_context_distances", "scan_context_distances_shift"))
def _scan_context(ctx, env):
    descs = [ctx.scan_context(env.I["f16_%d" % f]) for f in range(4)]
    query = ctx.scan_context(env.I["f16_revisit"])
    dist = ctx.scan_context_distances(query, np.stack(descs))
    dist2, shift = ctx.scan_context_distances_shift(query, np.stack(descs))
    return Out(dig(descs, query, dist, dist2, shift), None, {"descs": descs + [query], "dist": dist, "dist2": dist2})


@check("scan_context_4")
def _scan_context_check(env, out, orc):
    clouds = [env.I["f16_%d" % f] for f in range(4)] + [env.I["f16_revisit"]]
    for got, cloud in zip(out.raw["descs"], clouds):
        assert (got != orc.scan_context(cloud)).sum() <= 2        # (test_gpu_parity.py's: a point on a bin's edge)
    want = [orc.scan_context_distance(out.raw["descs"][4], h) for h in out.raw["descs"][:4]]
    assert (out.raw["dist"] == out.raw["dist2"]).all()
    np.testing.assert_allclose(out.raw["dist"], want, rtol=0, atol=1e-12)


@op("ground_16x600", 9600, "primitive", ("ground_segment",))
def _ground(ctx, env):
    from lidar_slam_from_scratch_amd import ground
    g = ground.ground_segment(ctx, env.I["ground_raw"])
    d = env.dev("ground_raw")
    gd = ground.ground_segment(ctx, None, device_ptr=d.data_ptr(), n_rows=d.shape[0])
    return Out(dig(g.labels, g.height, g.ground_z, list(g.counts()), gd.labels, gd.height, gd.ground_z, list(gd.counts())), None,
               {"labels": g.labels, "labels_device": gd.labels})


@check("ground_16x600")
def _ground_check(env, out, orc):
    import ground_ref
    from lidar_slam_from_scratch_amd import ground
    want = ground_ref.segment(env.I["ground_raw"], **ground.GroundConfig().as_dict())
    assert (out.raw["labels"] == want.labels).all() and (out.raw["labels_device"] == want.labels).all()


@op("occupancy_update_cells", 3000, "primitive", ("occupancy_clear", "occupancy_update", "occupancy_cells"), claims=("cells",))
def _occupancy(ctx, env):
    ctx.occupancy_clear()
    n = ctx.occupancy_update(env.I["world16_1"], env.I["p16_1"][:3, 3])
    cells = ctx.occupancy_cells()
    ctx.occupancy_clear()
    return Out(dig(n, cells), None, {"cells": cells})


@check("occupancy_update_cells")
def _occupancy_check(env, out, orc):
    want = orc.occupancy_update(set(), env.I["world16_1"], env.I["p16_1"][:3, 3])
    assert want and {tuple(c) for c in out.raw["cells"].tolist()} == want


# ---------------------------------------------------------------------------------------------------------------- threads
Thread = collections.namedtuple("Thread", "name run names claims")
THREADS = collections.OrderedDict()


def thread(name, names, claims=()):
    def deco(fn):
        THREADS[name] = Thread(name, fn, tuple(names), frozenset(claims))
        return fn
    return deco


def _stream_off(ctx):
    ctx.stream_reset()
    ctx.stream_set_robust(None)
    ctx.stream_set_deskew(None)


def _push_digest(ctx, res, hist, info, scan=True):
    capi = _capi()
    parts = [res, hist, info]
    if info.status == capi.STREAM_REGISTERED:
        parts += _normal_matrix_parts(ctx)
    if scan:
        parts.append(ctx.stream_current_scan())
    return dig(*parts)


@thread("stream_a", ("stream_reset", "stream_set_robust", "stream_set_deskew", "stream_push_host", "stream_current_scan",
                     "last_normal_matrix"), claims=("stream",))
def _stream_a(ctx, env):
    """eight 32 x 900 frames in host memory through the 0.5 m filter"""
    cfg = _capi().Context.make_config(max_iterations=20)
    _stream_off(ctx)
    try:
        for f in range(8):
            yield _push_digest(ctx, *ctx.stream_push_host(env.I["raw32_%d" % f], 0.5, 1000, cfg))
    finally:
        _stream_off(ctx)


@thread("stream_b", ("stream_reset", "stream_push_host", "stream_push", "stream_current_scan", "last_normal_matrix"),
        claims=("stream",))
def _stream_b(ctx, env):
    """unfiltered clouds of one size and different contents: the remembered target's (pointer, rows) key comes back every
    second push.  A frame under min_points, a push refused for a NaN row (through the filter, which is what looks at
    the rows) that leaves the stream where it was, and a reset in the middle."""
    capi = _capi()
    cfg = capi.Context.make_config(max_iterations=10)
    _stream_off(ctx)
    try:
        for f in range(3):
            yield _push_digest(ctx, *ctx.stream_push_host(env.I["b3000_%d" % f], 0.0, 1000, cfg))
        yield _push_digest(ctx, *ctx.stream_push_host(env.I["b_tiny"], 0.0, 1000, cfg))
        yield _push_digest(ctx, *ctx.stream_push_host(env.I["b3000_3"], 0.0, 1000, cfg))
        try:
            ctx.stream_push_host(env.I["b_nan"], 0.5, 1000, cfg)
            refused = 0
        except capi.IcpError as e:
            refused = e.code
        yield dig("refused", refused, ctx.stream_current_scan())
        yield _push_digest(ctx, *ctx.stream_push_host(env.I["b3000_4"], 0.0, 1000, cfg))
        ctx.stream_reset()
        for f in (5, 6, 7):
            d = env.dev("b3000_%d" % f)
            yield _push_digest(ctx, *ctx.stream_push(d.data_ptr(), d.shape[0], 0.0, 1000, cfg))
    finally:
        _stream_off(ctx)


@thread("stream_c", ("stream_reset", "stream_prefetch_file", "stream_push_file", "stream_map_update", "add_stream_frame",
                     "size", "world", "close"), claims=("stream",))
def _stream_c(ctx, env):
    """six .bin files, the next one's read and filter started before the current one is pushed; each filtered scan goes
    into world coordinates and into a global map, device to device"""
    from lidar_slam_from_scratch_amd.global_map import GlobalMap
    cfg = _capi().Context.make_config(max_iterations=20)
    _stream_off(ctx)
    gm = GlobalMap(ctx)
    try:
        pose = np.eye(4)
        poses = []
        for k, path in enumerate(env.bin_paths):
            if k + 1 < len(env.bin_paths):
                ctx.stream_prefetch_file(env.bin_paths[k + 1])
            res, hist, info = ctx.stream_push_file(path, 0.5, 500, cfg)
            pose = pose @ np.array(res.transformation[:]).reshape(4, 4)
            poses.append(pose)
            world, _cells = ctx.stream_map_update(pose, want_world=True, update_grid=False, n_rows=info.n_filtered)
            gm.add_stream_frame()
            yield dig(_push_digest(ctx, res, hist, info, scan=False), world, list(gm.size()))
        yield dig(gm.world(poses))
    finally:
        gm.close()
        _stream_off(ctx)


@thread("stream_settings", ("stream_reset", "stream_set_robust", "stream_set_deskew", "stream_push_host", "stream_last_robust",
                            "stream_current_scan"), claims=("stream",))
def _stream_settings(ctx, env):
    """the stream's robust rule and its deskew switched on and off between the pushes of raw sweeps"""
    from lidar_slam_from_scratch_amd import deskew
    capi = _capi()
    cfg = capi.Context.make_config(max_iterations=10)
    dk = deskew.DeskewConfig([0.0, 0.0, 0.004, 0.6, 0.0, 0.0], time_source=capi.DESKEW_AZIMUTH).to_c(False)
    settings = [(None, None), (HUBER_RULE, None), (HUBER_RULE, dk), (None, dk), (None, None), ((GEMAN_MCCLURE, 0.1, 2.0), dk)]
    _stream_off(ctx)
    try:
        for f, (rule, skew) in enumerate(settings):
            ctx.stream_set_robust(rule)
            ctx.stream_set_deskew(skew)
            res, hist, info = ctx.stream_push_host(env.I["sweep16_%d" % f], 0.5, 500, cfg)
            yield dig(_push_digest(ctx, res, hist, info), ctx.stream_last_robust())
    finally:
        _stream_off(ctx)


@thread("local_map", ("add", "register", "add_stream_frame", "register_robust", "register_device", "add_device",
                      "register_robust_device", "points", "size", "clear", "close", "stream_reset", "stream_push_host",
                      "last_normal_matrix"), claims=("stream",))
def _local_map(ctx, env):
    """six 16 x 600 frames three metres apart against a table of 10 m range: every add evicts"""
    from lidar_slam_from_scratch_amd.local_map import LocalMap, LocalMapConfig
    capi = _capi()
    lm = LocalMap(ctx, LocalMapConfig(voxel_size=0.5, max_range=10.0, capacity=1 << 15))

    def cfg(f):
        return capi.Context.make_config(max_iterations=8, initial_transform=env.I["p16_%d" % f])

    def table():
        pts, keys = lm.points()
        return [lm.size(), pts, keys]

    try:
        yield dig(lm.add(env.I["f16_0"], env.I["p16_0"]), table())
        res, hist = lm.register(env.I["f16_1"], cfg(1))
        yield dig(res, hist, _normal_matrix_parts(ctx))
        yield dig(lm.add(env.I["f16_1"], env.I["p16_1"]), table())
        ctx.stream_reset()
        _res, _hist, info = ctx.stream_push_host(env.I["f16_2"], 0.0, 0, cfg(2))
        yield dig(info, lm.add_stream_frame(env.I["p16_2"]), table())
        res, hist, rinfo = lm.register_robust(env.I["f16_3"], cfg(3), HUBER_RULE)
        yield dig(res, hist, rinfo, _normal_matrix_parts(ctx))
        yield dig(lm.add(env.I["f16_3"], env.I["p16_3"]), table())
        d = env.dev("f16_4")
        res, hist = lm.register_device(d.data_ptr(), d.shape[0], cfg(4))
        yield dig(res, hist, _normal_matrix_parts(ctx))
        yield dig(lm.add_device(d.data_ptr(), d.shape[0], env.I["p16_4"]), table())
        d = env.dev("f16_5")
        res, hist, rinfo = lm.register_robust_device(d.data_ptr(), d.shape[0], cfg(5), (GEMAN_MCCLURE, 0.1, 2.0))
        yield dig(res, hist, rinfo, _normal_matrix_parts(ctx))
        yield dig(lm.add(env.I["f16_5"], env.I["p16_5"]), table())
        lm.clear()
        yield dig(table())
    finally:
        lm.close()
        ctx.stream_reset()


def _raster_parts(r):
    return [r.min_x, r.min_y, r.width, r.height, r.resolution, r.n_occupied, r.n_free, r.data]


def _counts_parts(c):
    return [c.min_x, c.min_y, c.width, c.height, c.resolution, c.n_observed, c.n_hit_cells, c.max_hits, c.max_misses,
            c.frames_used, c.hits, c.misses, c.probability]


@thread("global_map", ("add_frame", "add_frame_device", "size", "world", "recent_clouds", "finish", "raycast", "raster",
                       "raycast_counts", "counts", "live_update", "live_counts", "live_clear", "set_ground", "ground_labels",
                       "close", "occupancy_cells", "world_static", "recent_clouds_static", "finish_static", "static_labels"),
        claims=("cells",))
def _global_map(ctx, env):
    from lidar_slam_from_scratch_amd import ground
    from lidar_slam_from_scratch_amd.global_map import GlobalMap
    gm = GlobalMap(ctx)
    poses = [env.I["p16_%d" % f] for f in range(5)]
    grid = ctx.make_grid_config()
    try:
        for f in range(4):
            gm.add_frame(env.I["f16_%d" % f])
            yield dig(list(gm.size()))
        d = env.dev("f16_4")
        gm.add_frame_device(d.data_ptr(), d.shape[0])
        yield dig(list(gm.size()))
        yield dig(gm.world(poses), gm.recent_clouds(poses, 2))
        cells, published = gm.finish(poses, grid, 1.0)
        yield dig(cells, published)
        yield dig(_raster_parts(gm.raycast(poses, grid)), _raster_parts(gm.raster()))
        yield dig(_counts_parts(gm.raycast_counts(poses, grid)), _counts_parts(gm.counts()))
        for k in (3, 5):
            info = gm.live_update(poses[:k], grid)
            counts, info2 = gm.live_counts()
            yield dig(info, info2, _counts_parts(counts))
        gm.set_ground(ground.GroundConfig())
        yield dig(gm.ground_labels(2), gm.ground_labels(4))
        info = gm.live_update(poses, grid)                                  # (a new ground config: a rebuild)
        yield dig(info, _counts_parts(gm.live_counts()[0]))
        cells, published = gm.finish(poses, grid, 1.0)
        yield dig(cells, published)
        gm.live_clear()
        gm.set_ground(None)
        info = gm.live_update(poses, grid)
        yield dig(info, _counts_parts(gm.live_counts()[0]))
        # the static map (appended: the digests above stay as they were)
        world, info = gm.world_static(poses, grid, (50, 2), 1)
        yield dig(world, info, gm.static_labels(0), gm.static_labels(4))
        yield dig(gm.recent_clouds_static(poses, grid, (50, 2), 2))
        published, info = gm.finish_static(poses[:4], grid, (50, 2), 1.0)         # (fewer poses: a rebuild of the live counts)
        yield dig(published, info, gm.static_labels(3))
    finally:
        gm.close()


def _closure_parts(r):
    return [r.query_frame, r.match_frame, r.transform, r.scan_context_distance, r.icp_fitness, r.sector_shift, r.pairs,
            r.weight_sum, r.information]


def loop_store_setup(ctx, env):
    """-> (an empty map, its detector, the clouds of the loop_store thread)"""
    from lidar_slam_from_scratch_amd import loop_closure as lc
    from lidar_slam_from_scratch_amd.global_map import GlobalMap
    gm = GlobalMap(ctx)
    cfg = lc.LoopClosureConfig(frame_gap=3, sc_distance_threshold=0.45, icp_fitness_threshold=0.5, max_candidates=3,
                               yaw_guess=True, max_correspondence_distance=2.0, robust_kind=HUBER, robust_scale=0.1,
                               information_sigma=0.05, information_floor=(0.01, 0.05))
    det = lc.StoreLoopClosureDetector(ctx, gm, cfg)
    return gm, det, [env.I["f16_%d" % f] for f in range(5)] + [env.I["f16_revisit"]]


@thread("loop_store", ("add_frame", "detect", "descriptor", "size", "set_gate", "set_robust", "set_gicp", "set_information",
                       "clear", "close"))
def _loop_store(ctx, env):
    """a detector over a map of its own, under a gate, a robust rule, the yaw guess and edge information, then with
    plane-to-plane verifications behind the gate; the last frame revisits the first one's place with another heading"""
    gm, det, clouds = loop_store_setup(ctx, env)
    try:
        for k, cloud in enumerate(clouds):
            gm.add_frame(cloud)
            det.add_frame(k, k)
            found = det.detect()
            yield dig(len(found), [_closure_parts(r) for r in found], det.descriptor(k), det.size())
        det.set_robust(0)
        det.set_gicp(1e-3)
        found = det.detect()
        yield dig(len(found), [_closure_parts(r) for r in found])
        det.set_gicp(0.0)
        det.set_gate(0.0)
        det.set_information(0.0)
        found = det.detect()
        yield dig(len(found), [_closure_parts(r) for r in found])
        det.clear()
        yield dig(det.size())
    finally:
        det.close()
        gm.close()


@thread("pose_graph", ("add_prior", "add_odometry_factor", "add_odometry_information", "add_loop_closure",
                       "add_loop_closure_information", "set_loop_loss", "loop_loss", "loop_weights", "optimize",
                       "joint_marginal_covariance", "marginal_covariance", "relative_covariance", "closure_distance",
                       "get_pose", "get_all_poses", "size", "loop_closure_count", "get_final_error", "get_iterations", "close"))
def _pose_graph(ctx, env):
    """a nine-pose ring: a Cauchy loss on its closing edge, an information matrix on one odometry edge and on a chord"""
    from lidar_slam_from_scratch_amd.pose_graph import PoseGraph
    capi = _capi()
    g = PoseGraph(ctx)
    I = env.I

    def stats():
        s = g.stats
        return [s.optimized, s.iterations, s.inner_trials, s.stop_reason, s.initial_error, s.final_error, s.final_lambda,
                [float(v) for v in s.history]]

    try:
        g.add_prior(0, I["pg_ring"][0])
        for k in range(8):
            if k == 3:
                g.add_odometry_information(k, k + 1, I["pg_odom"][k], I["pg_info"])
            else:
                g.add_odometry_factor(k, k + 1, I["pg_odom"][k], 0.05)
        g.set_loop_loss(capi.PG_LOSS_CAUCHY, 1.0)
        g.add_loop_closure(8, 0, I["pg_close"])
        g.add_loop_closure_information(4, 0, I["pg_chord"], I["pg_info"])
        yield dig(g.size(), g.loop_closure_count(), list(g.loop_loss()), np.stack(g.get_all_poses()))
        ok = g.optimize()
        yield dig(ok, stats(), np.stack(g.get_all_poses()), list(g.loop_weights()))
        yield dig(g.joint_marginal_covariance([0, 4, 8]))                   # (the first call after an optimize factors H)
        yield dig(g.marginal_covariance(3), g.relative_covariance(2, 7))
        yield dig(g.closure_distance(8, 0, I["pg_close"], np.linalg.inv(I["pg_info"])))
        ok = g.optimize()
        yield dig(ok, stats(), g.get_pose(5), g.get_final_error(), g.get_iterations())
        yield dig(g.joint_marginal_covariance([0, 4, 8]), g.relative_covariance(0, 8))
    finally:
        g.close()


@thread("occupancy", ("occupancy_clear", "occupancy_update", "occupancy_update_device", "occupancy_cells"), claims=("cells",))
def _occupancy_thread(ctx, env):
    """the context's cell set, grown by three scans"""
    ctx.occupancy_clear()
    try:
        for f in (0, 2):
            n = ctx.occupancy_update(env.I["world16_%d" % f], env.I["p16_%d" % f][:3, 3])
            yield dig(n, ctx.occupancy_cells())
        d = env.dev("world16_4")
        n = ctx.occupancy_update_device(d.data_ptr(), d.shape[0], env.I["p16_4"][:3, 3])
        yield dig(n, ctx.occupancy_cells())
        ctx.occupancy_clear()
        yield dig(ctx.occupancy_cells())
    finally:
        ctx.occupancy_clear()


# ------------------------------------------------------------------------------------------------------- plans and paths
def split_targets():
    """targets per split of the MFMA engines, from the headers (tests/test_gpu_exact_sums.py's)"""
    found = {}
    for header, name in (("nn_mfma.h", "kSplitTiles"), ("loop_plan.h", "kTile")):
        with open(os.path.join(CSRC, header)) as f:
            hit = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, f.read())
        assert hit, "%s: no `constexpr int %s = <number>;`" % (header, name)
        found[name] = int(hit.group(1))
    return found["kSplitTiles"] * found["kTile"]


def _constant(header, name):
    with open(os.path.join(CSRC, header)) as f:
        hit = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, f.read())
    assert hit, "%s: no `constexpr int %s = <number>;`" % (header, name)
    return int(hit.group(1))


def auto_facts(reg, cu=256):
    """engine_for (capi.hip) under SEARCH_AUTO, as loop_plan_print's facts, and the path's name"""
    per_split = split_targets()
    n, m = reg["n"], reg["m"]
    splits = (m + per_split - 1) // per_split
    mfma = m >= _constant("capi.hip", "kMfmaMinTargets") and n >= _constant("loop_plan.h", "kMfmaMinQueries")
    pruned = mfma and splits > _constant("capi.hip", "kAutoCulledFrom")
    facts = ["engine=%s" % ("mfma" if mfma else "exact"), "pruned=%d" % pruned, "splits=%d" % (splits if mfma else 0), "cu=%d" % cu,
             "rule=%s" % reg["rule"], "n=%d" % n]
    return facts, mfma, pruned


def planned(exe, reg, cu=256):
    """-> (path name, the plan's run of that call: loop_plan_print's tuple)"""
    import subprocess
    facts, mfma, pruned = auto_facts(reg, cu)
    r = subprocess.run([exe] + facts, capture_output=True, text=True, timeout=60, check=True)
    lines = r.stdout.strip().splitlines()
    assert lines[0].startswith("constants ") and len(lines) == 2 and not lines[1].endswith("refused"), r.stdout[:400]
    run = tuple(int(v) for v in lines[1].split())
    path = "exact" if not mfma else ("small" if run[6] else ("culled" if pruned else "general"))
    return path, run


def build_plan_printer(out_dir):
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        raise RuntimeError("no host C++ compiler")
    exe = os.path.join(str(out_dir), "loop_plan_print")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "loop_plan_print.cpp"),
                    "-o", exe], check=True)
    return exe


# -------------------------------------------------------------------------------------------------------------- harness
SEARCH = {"auto": 0, "exact": 1, "mfma": 2, "pruned": 3}


@contextlib.contextmanager
def fresh(search=0, profile=0):
    ctx = _capi().Context(device=0, search=search, profile=profile)
    try:
        yield ctx
    finally:
        ctx.close()


def run_thread(ctx, env, name):
    """a thread's undisturbed run -> its digests"""
    gen = THREADS[name].run(ctx, env)
    try:
        return list(gen)
    finally:
        gen.close()


def expected_ops(env, search=0, profile=0, names=None):
    """name -> Out of the call as the first call on a fresh context, closed afterwards"""
    out = collections.OrderedDict()
    for name in (names or OPS):
        with fresh(search, profile) as ctx:
            out[name] = OPS[name].run(ctx, env)
    return out


def expected_threads(env, search=0, profile=0, names=None):
    out = collections.OrderedDict()
    for name in (names or THREADS):
        with fresh(search, profile) as ctx:
            out[name] = run_thread(ctx, env, name)
    return out


class Tally:
    """the (operation, context-history) pairs a sequence asserted, and those that differed"""

    def __init__(self, tag=""):
        self.tag, self.count, self.bad = tag, 0, []

    def op(self, ctx, env, name, exp_ops, where):
        got = OPS[name].run(ctx, env)
        self.count += 1
        if got.digest != exp_ops[name].digest:
            self.bad.append((self.tag, where, name))
        return got

    def step(self, gen, tname, k, exp_threads, where):
        got = next(gen)
        self.count += 1
        if got != exp_threads[tname][k]:
            self.bad.append((self.tag, where, "%s[%d]" % (tname, k)))

    def merge(self, other):
        self.count += other.count
        self.bad += other.bad


def under_fire(ctx, env, tname, seed, exp_ops, exp_threads, tally):
    """one thread on a context of its own, one catalogue operation between every two steps (round-robin from a seeded
    offset; an operation with a claim of the thread's own is documented to disturb it and is passed over)"""
    th = THREADS[tname]
    names = [n for n in OPS if not (OPS[n].claims & th.claims)]
    at = int(np.random.default_rng(seed).integers(0, len(names)))
    gen = th.run(ctx, env)
    try:
        for k in range(len(exp_threads[tname])):
            tally.step(gen, tname, k, exp_threads, ("under fire", seed, k))
            tally.op(ctx, env, names[at % len(names)], exp_ops, ("under fire", seed, tname, k))
            at += 1
    finally:
        gen.close()


def lanes_of(threads=None):
    """threads that share a claim go into one lane, in catalogue order; every other thread is a lane of its own"""
    lanes, by_claim = [], {}
    for name in (threads or THREADS):
        claims = THREADS[name].claims
        lane = next((by_claim[c] for c in sorted(claims) if c in by_claim), None)
        if lane is None:
            lane = []
            lanes.append(lane)
        lane.append(name)
        for c in claims:
            by_claim[c] = lane
    return lanes


def shuffle_plan(seed, exp_threads, threads=None):
    """-> [(thread, step)]: every step of every thread, each thread's own order kept, dealt out by a seeded shuffle.
    The threads of one lane (lanes_of) follow each other, in a seeded order; the lanes interleave."""
    rng = np.random.default_rng(seed)
    queues = []
    for lane in lanes_of(threads):
        order = [lane[i] for i in rng.permutation(len(lane))]
        queues.append([(t, k) for t in order for k in range(len(exp_threads[t]))])
    deck = [i for i, q in enumerate(queues) for _ in q]
    rng.shuffle(deck)
    at = [0] * len(queues)
    plan = []
    for i in deck:
        plan.append(queues[i][at[i]])
        at[i] += 1
    return plan


def run_plan(ctx, env, plan, exp_threads, tally, tag):
    gens = {}
    try:
        for i, (tname, k) in enumerate(plan):
            if k == 0:
                gens[tname] = THREADS[tname].run(ctx, env)
            tally.step(gens[tname], tname, k, exp_threads, (tag, i))
            if k == len(exp_threads[tname]) - 1:
                gens.pop(tname).close()
    finally:
        for g in gens.values():
            g.close()


def size_orders(kinds=("registration", "primitive")):
    """the shrink-and-grow orders: descending row count, ascending, and the two interleaved (largest, smallest, ...)"""
    names = [n for n in OPS if OPS[n].kind in kinds]
    down = sorted(names, key=lambda n: -OPS[n].rows)
    up = down[::-1]
    mixed = [(down if i % 2 == 0 else up)[i // 2] for i in range(len(names))]
    return down, up, mixed


def refused_calls(ctx, env):
    """one refused call of each family, each refused by an argument check -> the error codes"""
    capi = _capi()
    I = env.I
    codes = []

    def refuse(fn):
        try:
            fn()
        except capi.IcpError as e:
            codes.append(e.code)
            return
        raise AssertionError("a call that must be refused was accepted")

    refuse(lambda: ctx.voxel_downsample(I["b_nan"], 0.5))
    refuse(lambda: ctx.align(I["rc_s1001"], I["rc_t1500"], capi.Context.make_config(max_iterations=-1)))
    cfg, res, hist = capi.Context.make_config(max_iterations=3), capi.Result(), np.zeros(4)
    s, t = I["rc_s1001"], I["rc_t1500"]
    refuse(lambda: ctx._check(ctx._lib.icpmi_align_gated(ctx._h, capi._dp(s), s.shape[0], capi._dp(t), t.shape[0], C.byref(cfg), None,
                                                         C.byref(res), None, capi._dp(hist), 4)))
    refuse(lambda: ctx.deskew(I["dk_xyz"], I["dk_tau"], _deskew_cfg(env, capi.DESKEW_TIMES, direction=0)))
    refuse(lambda: ctx.k_nearest(I["nn_t5000"], I["nn_q513"], 0))
    return codes


# ----------------------------------------------------------------------------------------------------------------- soak
def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seeds", type=int, default=10)
    ap.add_argument("--search", choices=sorted(SEARCH), default="auto")
    ap.add_argument("--profile", type=int, default=0)
    args = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime per process)
    from lidar_slam_from_scratch_amd import build
    build.build_library()
    env = Env()
    try:
        search = SEARCH[args.search]
        exp_ops, exp_threads = expected_ops(env, search, args.profile), expected_threads(env, search, args.profile)
        again = expected_ops(env, search, args.profile)
        unstable = [n for n in OPS if again[n].digest != exp_ops[n].digest]
        tally = Tally()
        with fresh(search, args.profile) as ctx:
            for seed in range(args.seeds):
                run_plan(ctx, env, shuffle_plan(seed, exp_threads), exp_threads, tally, ("soak", seed))
                for name in size_orders()[2]:
                    tally.op(ctx, env, name, exp_ops, ("soak", seed))
                for tname in THREADS:
                    under_fire(ctx, env, tname, seed, exp_ops, exp_threads, tally)
        print("call sequences: %d digests asserted over %d seeds, %d differ, %d operations unstable on fresh contexts"
              % (tally.count, args.seeds, len(tally.bad), len(unstable)))
        for b in tally.bad[:40]:
            print("   differs:", b)
        for n in unstable:
            print("   unstable:", n)
        return 1 if (tally.bad or unstable) else 0
    finally:
        env.close()


if __name__ == "__main__":
    sys.exit(main())
