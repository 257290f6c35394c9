"""Loop-closure detection: Scan Context candidates + ICP verification, the second caller of
the ICP hot path.  Host-side mirror of the reference's
    LoopClosureConfig / LoopClosureResult / LoopClosureDetector   (core/loop_closure.hpp)
    ScanContext                                                   (core/scan_context.hpp)
with the arithmetic behind a small backend object:
    backend.scan_context(cloud) -> (20, 60) descriptor            scan_context.hpp:44-82
    backend.distances(query_desc, hist_descs) -> array            scan_context.hpp:90-142
    backend.align(source, target, max_iterations, tolerance)      icp.hpp:157-258
`GpuBackend` goes through the C ABI; the parity tests plug the oracle in instead.

LoopClosureConfig(yaw_guess=True) (not in the reference) keeps the column shift that attained each
candidate's distance and starts its verification from Rz(shift * 6 deg) (icpmi_sc_shift_transform) instead of from the
identity, so a place revisited with another heading closes too.  The backend then also needs
    backend.distances_shift(query_desc, hist_descs) -> (distances, shifts)
and align / align_many that take keyword-only initial_transform / initial_transforms; with the option off neither is
touched, so a backend with the four-argument align keeps working.

LoopClosureConfig(max_correspondence_distance=d) with d > 0 (not in the reference) runs the verifications
behind a correspondence-distance gate (icpmi_align_gated): a pass sums only the rows whose nearest target is within d, so
a place revisited a lane aside -- scans that overlap only partly -- verifies, and icp_fitness is the RMS over the kept
rows.  align / align_many are then passed keyword-only max_distance, and their results carry `pairs`, the rows the last
pass kept.  0 (the default) passes nothing.  2 m suits 0.5 m voxel-filtered street scans; a tight gate (1 m) can make
the kept set alternate between passes, so that a verification runs out of iterations.

LoopClosureConfig(robust_kind=k, robust_scale=s) with k one of capi.ROBUST_* (not in the reference) runs the
verifications under robust row weights (icpmi_align_robust), with the gate above if that is set too.  align / align_many
are then passed keyword-only robust=(kind, scale), and their results carry `weight_sum`.  icp_fitness is then the WEIGHTED
RMS, which reads lower than the plain one against icp_fitness_threshold.  0 (the default) passes nothing.

LoopClosureConfig(information_sigma=s, information_floor=(sigma_R, sigma_t)) with s > 0 (not in the reference)
attaches to each result the 6 x 6 information matrix of its edge, icpmi_information_from_icp on that verification's own
normal matrix (icpmi_last_normal_matrix) and transform: what PoseGraph.add_loop_closure_information(match, query,
transform, information) takes.  align / align_many are then passed keyword-only information=(s, sigma_R, sigma_t), and their
results carry `information`.  0 (the default) passes nothing.

LoopClosureConfig(gicp_epsilon=e) with 0 < e <= 1 (not in the reference) runs the verifications as
plane-to-plane registrations (icpmi_align_gicp in its small form, capi.GICP_FORM_SMALL), behind the gate above if that is
set too.  align / align_many are then passed keyword-only gicp=(e,), and their results carry `pairs`, gate or not.  Not
together with robust_kind (ValueError; the store detector's setter refuses).  0 (the default) passes nothing.
"""
import ctypes as C
import weakref

import numpy as np

MAX_BATCH = 8   # ICPMI_MAX_BATCH (include/icp_mi355x.h): registrations one icpmi_align_batch call takes


class LoopClosureConfig:
    """loop_closure.hpp:14-19"""

    def __init__(self, frame_gap=50, sc_distance_threshold=0.25, icp_fitness_threshold=0.3, max_candidates=3,
                 yaw_guess=False, max_correspondence_distance=0.0, robust_kind=0, robust_scale=0.0,
                 information_sigma=0.0, information_floor=(0.0, 0.0), gicp_epsilon=0.0):
        self.gicp_epsilon = gicp_epsilon
        self.information_sigma = information_sigma
        self.information_floor = information_floor
        self.yaw_guess = yaw_guess
        self.robust_kind = robust_kind
        self.robust_scale = robust_scale
        self.max_correspondence_distance = max_correspondence_distance
        self.frame_gap = frame_gap
        self.sc_distance_threshold = sc_distance_threshold
        self.icp_fitness_threshold = icp_fitness_threshold
        self.max_candidates = max_candidates


class LoopClosureResult:
    """loop_closure.hpp:25-31; sector_shift: the column shift the verification started from (None: yaw_guess off);
    pairs: the rows the verification's last pass kept (None: neither a correspondence-distance gate nor gicp_epsilon); weight_sum: that pass's
    weight sum (None: no robust weights); information: the edge's 6 x 6 information matrix (None: information_sigma off)"""

    def __init__(self, query_frame, match_frame, transform, scan_context_distance, icp_fitness, sector_shift=None,
                 pairs=None, weight_sum=None, information=None):
        self.information = information
        self.sector_shift = sector_shift
        self.weight_sum = weight_sum
        self.pairs = pairs
        self.query_frame = query_frame
        self.match_frame = match_frame
        self.transform = transform
        self.scan_context_distance = scan_context_distance
        self.icp_fitness = icp_fitness


class GpuBackend:
    def __init__(self, ctx):
        self.ctx = ctx

    def scan_context(self, cloud):
        return self.ctx.scan_context(cloud)

    def distances(self, query_desc, hist_descs):
        return self.ctx.scan_context_distances(query_desc, hist_descs)

    def distances_shift(self, query_desc, hist_descs):
        """-> (distances, the smallest column shift attaining each), icpmi_scan_context_distances_shift"""
        return self.ctx.scan_context_distances_shift(query_desc, hist_descs)

    def align(self, source, target, max_iterations, tolerance, *, initial_transform=None, max_distance=None, robust=None,
              information=None, gicp=None):
        if initial_transform is None and max_distance is None and robust is None and information is None and gicp is None:
            from .odometry import gpu_align
            return gpu_align(self.ctx)(source, target, max_iterations, tolerance)
        return self.align_many(source, [target], max_iterations, tolerance,
                               initial_transforms=None if initial_transform is None else [initial_transform],
                               max_distance=max_distance, robust=robust, information=information, gicp=gicp)[0]

    def align_many(self, source, targets, max_iterations, tolerance, *, initial_transforms=None, max_distance=None,
                   robust=None, information=None, gicp=None):
        """The verifications of one detect() side by side on the GPU (icpmi_align_batch): same results as
        align() one after the other.  initial_transforms: one 4 x 4 per target (None: the identity for all).
        max_distance: the correspondence-distance gate (icpmi_align_gated_batch; None: none); the results then carry
        `pairs`.  robust: (kind, scale), the row weights (icpmi_align_robust_batch, behind max_distance if that is given
        too; None: none); the results then carry `weight_sum` as well.  information: (sigma, floor sigma_R, floor sigma_t);
        the results then carry `information`, capi.information_from_icp of problem k's normal matrix (None where its
        last pass kept no row: such a result has an infinite final_error and is never accepted).  gicp: (epsilon,), the
        plane-to-plane cost in its small form (icpmi_align_gicp_batch with capi.GICP_FORM_SMALL, behind max_distance if
        that is given too; None: point-to-plane; not with robust); the results then carry `pairs`, gate or not."""
        from . import capi
        if gicp is not None and robust is not None:
            raise ValueError("gicp= and robust= exclude each other: the plane-to-plane rows carry no robust weights")

        class _R:
            pass

        cfg = capi.Context.make_config(max_iterations=max_iterations, tolerance=tolerance)
        if initial_transforms is not None:
            cfg = [capi.Context.make_config(max_iterations=max_iterations, tolerance=tolerance, initial_transform=T)
                   for T in initial_transforms]
        out = []
        if gicp is not None:
            rule = capi.as_gicp((float(gicp[0]), 0.0 if max_distance is None else float(max_distance), True))
            runs = [(res, int(info.pairs), None) for res, _hist, info in
                    self.ctx.align_gicp_batch([source] * len(targets), targets, cfg, rule)]
        elif robust is not None:
            rule = capi.as_robust((robust[0], robust[1], 0.0 if max_distance is None else float(max_distance)))
            runs = [(res, int(info.pairs) if max_distance is not None else None, float(info.weight_sum)) for res, _hist, info in
                    self.ctx.align_robust_batch([source] * len(targets), targets, cfg, rule)]
        elif max_distance is None:
            runs = [(res, None, None) for res, _hist in self.ctx.align_batch([source] * len(targets), targets, cfg)]
        else:
            runs = [(res, pairs, None) for res, _hist, pairs in
                    self.ctx.align_gated_batch([source] * len(targets), targets, cfg, float(max_distance))]
        for k, (res, pairs, weight_sum) in enumerate(runs):
            r = _R()
            if information is not None:
                try:
                    nm = self.ctx.last_normal_matrix(k)
                    r.information = capi.information_from_icp(nm.JtJ, nm.T, *information)
                except capi.IcpError:
                    r.information = None
            r.transformation = np.array(res.transformation[:]).reshape(4, 4)
            r.converged, r.final_error, r.num_iterations = bool(res.converged), res.final_error, res.num_iterations
            r.pairs = pairs
            r.weight_sum = weight_sum
            out.append(r)
        return out


def sc_shift_transform(shift):
    """icpmi_sc_shift_transform (host only, no device): the 4 x 4 a verification starts from, Rz(shift * 2 pi / 60)"""
    from . import capi
    T = np.empty((4, 4))
    rc = capi.load_library().icpmi_sc_shift_transform(int(shift), capi._dp(T))
    if rc != capi.OK:
        raise capi.IcpError(rc, "shift %d outside 0..59" % int(shift))
    return T


class LoopClosureDetector:
    """loop_closure.hpp:41-148"""

    def __init__(self, backend, config=None):
        self.backend = backend
        self.config = config or LoopClosureConfig()
        self.clear()

    def add_frame(self, cloud, frame_idx):
        """loop_closure.hpp:54-60"""
        cloud = np.ascontiguousarray(cloud, dtype=np.float64)
        self._descriptors.append(np.asarray(self.backend.scan_context(cloud)).reshape(20, 60))
        self._clouds.append(cloud)
        self._frame_indices.append(int(frame_idx))
        self._latest = int(frame_idx)

    def size(self):
        return len(self._descriptors)

    def clear(self):
        self._descriptors, self._clouds, self._frame_indices, self._latest = [], [], [], -1

    def detect(self):
        """loop_closure.hpp:66-126: closures for the most recently added frame."""
        results = []
        if len(self._descriptors) < 2:
            return results
        q = len(self._descriptors) - 1
        hist = np.stack(self._descriptors[:-1])
        guess = bool(getattr(self.config, "yaw_guess", False))
        gate = float(getattr(self.config, "max_correspondence_distance", 0.0) or 0.0)
        gkw = {"max_distance": gate} if gate > 0.0 else {}   # (passed only when set, as the starts are)
        kind = int(getattr(self.config, "robust_kind", 0) or 0)
        robust = kind != 0
        gated = gate > 0.0
        if robust:
            gkw["robust"] = (kind, float(self.config.robust_scale))
        gicp = float(getattr(self.config, "gicp_epsilon", 0.0) or 0.0)
        if gicp != 0.0:
            if robust:
                raise ValueError("gicp_epsilon and robust_kind exclude each other")
            gkw["gicp"] = (gicp,)
            gated = True   # (the results carry the kept rows, gate or not)
        info_sigma = float(getattr(self.config, "information_sigma", 0.0) or 0.0)
        if info_sigma > 0.0:
            floor = getattr(self.config, "information_floor", (0.0, 0.0))
            gkw["information"] = (info_sigma, float(floor[0]), float(floor[1]))
        if guess:
            dist, shift = self.backend.distances_shift(self._descriptors[q], hist)
        else:
            dist = self.backend.distances(self._descriptors[q], hist)        # :86 for every i
        candidates = []
        for i in range(q):
            if self._frame_indices[q] - self._frame_indices[i] < self.config.frame_gap:   # :81-82
                continue
            if dist[i] < self.config.sc_distance_threshold:                   # :87-89
                candidates.append((float(dist[i]), i))
        candidates.sort()                                                     # :93 (the shift never enters the order)
        # The reference verifies the candidates one after the other until max_candidates are ACCEPTED (:96-123).
        # The registrations are independent, so the next (max_candidates - accepted) of them -- all of which the
        # sequential loop would reach -- run side by side when the backend can (icpmi_align_batch); the
        # outcomes are taken in the reference's order.
        verified, pos = 0, 0
        many = getattr(self.backend, "align_many", None)
        while pos < len(candidates) and verified < self.config.max_candidates:   # :97
            # (at most MAX_BATCH side by side: icpmi_align_batch's limit; a larger max_candidates takes more rounds)
            chunk = candidates[pos:pos + min(self.config.max_candidates - verified, MAX_BATCH)]
            pos += len(chunk)
            starts = [sc_shift_transform(int(shift[c])) for _, c in chunk] if guess else None
            if many is not None and len(chunk) > 1:
                kw = {"initial_transforms": starts} if guess else {}
                outs = many(self._clouds[q], [self._clouds[c] for _, c in chunk], 30, 1e-6, **kw, **gkw)
            elif guess:
                outs = [self.backend.align(self._clouds[q], self._clouds[c], 30, 1e-6, initial_transform=T, **gkw)
                        for (_, c), T in zip(chunk, starts)]
            else:
                outs = [self.backend.align(self._clouds[q], self._clouds[c], 30, 1e-6, **gkw) for _, c in chunk]   # :102-109
            for (sc_dist, cand), r in zip(chunk, outs):
                if r.converged and r.final_error < self.config.icp_fitness_threshold:   # :112
                    results.append(LoopClosureResult(self._frame_indices[q], self._frame_indices[cand],
                                                     np.asarray(r.transformation), sc_dist, r.final_error,
                                                     int(shift[cand]) if guess else None,
                                                     getattr(r, "pairs", None) if gated else None,
                                                     getattr(r, "weight_sum", None) if robust else None,
                                                     getattr(r, "information", None) if info_sigma > 0.0 else None))
                    verified += 1
        return results


class StoreLoopClosureDetector:
    """The same detector with its database on the device (icpmi_loop, csrc/loop_store.h): an index over the frames of a
    global_map.GlobalMap.  add_frame(store_frame, frame_idx) names a frame the store already holds; the detector keeps
    no clouds and no descriptors on the host, and detect() returns what LoopClosureDetector(GpuBackend(ctx)) returns
    over the same clouds, bit for bit."""

    def __init__(self, ctx, store, config=None):
        from . import capi
        self._lib = capi.load_library()
        self.ctx, self.store = ctx, store
        self.config = config or LoopClosureConfig()
        c = capi.LoopConfig()
        c.frame_gap, c.max_candidates = int(self.config.frame_gap), int(self.config.max_candidates)
        c.sc_distance_threshold = float(self.config.sc_distance_threshold)
        c.icp_fitness_threshold = float(self.config.icp_fitness_threshold)
        h = C.c_void_p()
        ctx._check(self._lib.icpmi_loop_create(store._h, C.byref(c), C.byref(h)))
        self._h = h
        try:
            self._configure(ctx, h)
        except Exception:
            self.close()               # (a setter refused: the handle goes now, not when the object is collected -- after its map)
            raise
        for owner in (ctx, store):     # Context.close() and store.close() destroy it before the map
            if not hasattr(owner, "_loops"):
                owner._loops = weakref.WeakSet()
            owner._loops.add(self)

    def _configure(self, ctx, h):
        if getattr(self.config, "yaw_guess", False):
            ctx._check(self._lib.icpmi_loop_set_yaw_guess(h, 1))
        self._gated = float(getattr(self.config, "max_correspondence_distance", 0.0) or 0.0) > 0.0
        if self._gated:
            ctx._check(self._lib.icpmi_loop_set_gate(h, float(self.config.max_correspondence_distance)))
        self._robust = int(getattr(self.config, "robust_kind", 0) or 0) != 0
        if self._robust:
            ctx._check(self._lib.icpmi_loop_set_robust(h, int(self.config.robust_kind), float(self.config.robust_scale)))
        self._gicp = float(getattr(self.config, "gicp_epsilon", 0.0) or 0.0) != 0.0
        if self._gicp:
            ctx._check(self._lib.icpmi_loop_set_gicp(h, float(self.config.gicp_epsilon)))
        self._information = float(getattr(self.config, "information_sigma", 0.0) or 0.0) > 0.0
        if self._information:
            floor = getattr(self.config, "information_floor", (0.0, 0.0))
            ctx._check(self._lib.icpmi_loop_set_information(h, float(self.config.information_sigma), float(floor[0]),
                                                            float(floor[1])))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.icpmi_loop_destroy(self._h)
            self._h = None

    __del__ = close

    def set_gate(self, max_distance):
        """icpmi_loop_set_gate: the verifications' correspondence-distance gate from the next detect on (0: off)"""
        self.ctx._check(self._lib.icpmi_loop_set_gate(self._h, float(max_distance)))
        self._gated = float(max_distance) > 0.0   # (the caller's config object, which it may share, is left alone)

    def set_robust(self, kind, scale=0.0):
        """icpmi_loop_set_robust: the verifications' row weights from the next detect on (kind 0: off)"""
        self.ctx._check(self._lib.icpmi_loop_set_robust(self._h, int(kind), float(scale)))
        self._robust = int(kind) != 0

    def set_gicp(self, epsilon):
        """icpmi_loop_set_gicp: plane-to-plane verifications (the small form) from the next detect on (0: off)"""
        self.ctx._check(self._lib.icpmi_loop_set_gicp(self._h, float(epsilon)))
        self._gicp = float(epsilon) != 0.0

    def set_information(self, sigma, floor_rotation_sigma=0.0, floor_translation_sigma=0.0):
        """icpmi_loop_set_information: each result's edge information from the next detect on (sigma 0: off)"""
        self.ctx._check(self._lib.icpmi_loop_set_information(self._h, float(sigma), float(floor_rotation_sigma),
                                                             float(floor_translation_sigma)))
        self._information = float(sigma) > 0.0

    def add_frame(self, store_frame, frame_idx):
        """loop_closure.hpp:54-60 for the cloud the store holds as frame `store_frame`"""
        self.ctx._check(self._lib.icpmi_loop_add_frame(self._h, int(store_frame), int(frame_idx)))

    def size(self):
        n = C.c_int64(0)
        self.ctx._check(self._lib.icpmi_loop_size(self._h, C.byref(n)))
        return n.value

    def clear(self):
        """drops every entry; the store is untouched"""
        self.ctx._check(self._lib.icpmi_loop_clear(self._h))

    def descriptor(self, entry):
        """entry's (20, 60) descriptor (icpmi_scan_context of its rows, bit for bit)"""
        from . import capi
        out = np.empty((20, 60))
        self.ctx._check(self._lib.icpmi_loop_descriptor(self._h, int(entry), capi._dp(out)))
        return out

    def detect(self):
        """loop_closure.hpp:66-126: closures for the most recently added entry"""
        from . import capi
        cap = max(int(self.config.max_candidates), 0)
        buf = (capi.LoopResult * max(cap, 1))()
        n = C.c_int64(0)
        self.ctx._check(self._lib.icpmi_loop_detect(self._h, buf, cap, C.byref(n)))
        shifts = [None] * n.value
        if getattr(self.config, "yaw_guess", False):
            sh = (C.c_int32 * max(n.value, 1))()
            m = C.c_int64(0)
            self.ctx._check(self._lib.icpmi_loop_last_shifts(self._h, sh, n.value, C.byref(m)))
            shifts = [int(v) for v in sh[:m.value]]
        pairs = [None] * n.value
        if self._gated or self._gicp:
            pr = (C.c_int64 * max(n.value, 1))()
            m = C.c_int64(0)
            self.ctx._check(self._lib.icpmi_loop_last_pairs(self._h, pr, n.value, C.byref(m)))
            pairs = [int(v) for v in pr[:m.value]]
        weights = [None] * n.value
        if self._robust:
            wt = (C.c_double * max(n.value, 1))()
            m = C.c_int64(0)
            self.ctx._check(self._lib.icpmi_loop_last_weights(self._h, wt, n.value, C.byref(m)))
            weights = [float(v) for v in wt[:m.value]]
        infos = [None] * n.value
        if self._information:
            mats = np.zeros((max(n.value, 1), 6, 6))
            m = C.c_int64(0)
            self.ctx._check(self._lib.icpmi_loop_last_information(self._h, capi._dp(mats), n.value, C.byref(m)))
            infos = [mats[i].copy() for i in range(m.value)]
        return [LoopClosureResult(r.query_frame, r.match_frame, np.array(r.transform[:]).reshape(4, 4),
                                  r.scan_context_distance, r.icp_fitness, s, p, w, a)
                for r, s, p, w, a in zip(buf[:n.value], shifts, pairs, weights, infos)]
