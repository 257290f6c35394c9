"""slam::PoseGraph (core/pose_graph.hpp:49-147, src/core/pose_graph.cpp) through the C ABI: the factors and estimates
live on the device (icpmi_pose_graph), Levenberg-Marquardt runs there (csrc/pose_graph.h).  Method names follow the
reference's, in Python spelling.  `stats` holds the last optimize()'s icpmi_pose_graph_info and error history."""
import ctypes as C
import weakref

import numpy as np

from . import capi


class PoseGraphConfig:
    """pose_graph.hpp:22-40"""

    def __init__(self, **kw):
        c = capi.PoseGraphConfig()
        capi.load_library().icpmi_pose_graph_config_default(C.byref(c))
        for name, _t in capi.PoseGraphConfig._fields_:
            if name != "reserved":
                setattr(self, name, getattr(c, name))
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError(k)
            setattr(self, k, v)

    def to_c(self):
        c = capi.PoseGraphConfig()
        for name, _t in capi.PoseGraphConfig._fields_:
            if name != "reserved":
                setattr(c, name, getattr(self, name))
        return c


class PoseGraphStats:
    def __init__(self, info, history):
        self.optimized = bool(info.optimized)
        self.iterations = info.iterations
        self.inner_trials = info.inner_iterations
        self.stop_reason = info.stop_reason
        self.initial_error = info.initial_error
        self.final_error = info.final_error
        self.final_lambda = info.final_lambda
        self.history = list(history[:info.history_len])


def _T(pose):
    T = np.ascontiguousarray(pose, dtype=np.float64)
    if T.shape != (4, 4):
        raise ValueError("expected a 4 x 4 transform")
    return T


class PoseGraph:
    def __init__(self, ctx, config=None):
        self._lib = capi.load_library()
        self.ctx = ctx
        self.config = config or PoseGraphConfig()
        h = C.c_void_p()
        cfg = self.config.to_c()
        ctx._check(self._lib.icpmi_pose_graph_create(ctx._h, C.byref(cfg), C.byref(h)))
        self._h = h
        self.stats = None
        if not hasattr(ctx, "_pose_graphs"):
            ctx._pose_graphs = weakref.WeakSet()
        ctx._pose_graphs.add(self)     # Context.close() destroys the graph first

    def close(self):
        if getattr(self, "_h", None):
            self._lib.icpmi_pose_graph_destroy(self._h)
            self._h = None

    __del__ = close

    def add_prior(self, index, pose):
        """pose_graph.cpp:58-79"""
        T = _T(pose)
        self.ctx._check(self._lib.icpmi_pose_graph_add_prior(self._h, int(index), capi._dp(T)))

    def add_odometry_factor(self, from_idx, to_idx, relative_transform, fitness_score=0.0):
        """pose_graph.cpp:81-116"""
        T = _T(relative_transform)
        self.ctx._check(self._lib.icpmi_pose_graph_add_odometry(self._h, int(from_idx), int(to_idx), capi._dp(T),
                                                                float(fitness_score)))

    def add_loop_closure(self, from_idx, to_idx, relative_transform):
        """pose_graph.cpp:118-141"""
        T = _T(relative_transform)
        self.ctx._check(self._lib.icpmi_pose_graph_add_loop_closure(self._h, int(from_idx), int(to_idx), capi._dp(T)))

    @staticmethod
    def _info(information):
        A = np.ascontiguousarray(information, dtype=np.float64)
        if A.shape != (6, 6):
            raise ValueError("expected a 6 x 6 information matrix")
        return A

    def add_odometry_information(self, from_idx, to_idx, relative_transform, information):
        """add_odometry_factor weighted by a full 6 x 6 information matrix in the factor's tangent order (omega, v)
        instead of the config's sigmas (icpmi_pose_graph_add_odometry_information; not in the reference).  A matrix
        that is not finite, symmetric and positive definite raises IcpError(ERR_ARG) and changes nothing."""
        T, A = _T(relative_transform), self._info(information)
        self.ctx._check(self._lib.icpmi_pose_graph_add_odometry_information(self._h, int(from_idx), int(to_idx),
                                                                            capi._dp(T), capi._dp(A)))

    def add_loop_closure_information(self, from_idx, to_idx, relative_transform, information):
        """add_loop_closure weighted by a full 6 x 6 information matrix (icpmi_pose_graph_add_loop_closure_information);
        the loop loss and loop_weights() see it as any loop closure, with d = ||R r||."""
        T, A = _T(relative_transform), self._info(information)
        self.ctx._check(self._lib.icpmi_pose_graph_add_loop_closure_information(self._h, int(from_idx), int(to_idx),
                                                                                capi._dp(T), capi._dp(A)))

    def set_loop_loss(self, kind, scale=0.0):
        """A robust loss on the loop-closure edges (icpmi_pose_graph_set_loop_loss; not in the reference): kind one of
        capi.PG_LOSS_*, scale in sigmas.  The graph's setting: every loop closure, past and future, at the next
        optimize().  A change clears the optimised state."""
        self.ctx._check(self._lib.icpmi_pose_graph_set_loop_loss(self._h, int(kind), float(scale)))

    def loop_loss(self):
        kind, scale = C.c_int32(0), C.c_double(0.0)
        self.ctx._check(self._lib.icpmi_pose_graph_loop_loss(self._h, C.byref(kind), C.byref(scale)))
        return kind.value, scale.value

    def loop_weights(self):
        """-> (weights, distances) of the loop closures at the optimised values, in add_loop_closure order; raises
        unless the optimised state of the last optimize() holds.  With the loss off the weights are 1."""
        n = C.c_int64(0)
        self.ctx._check(self._lib.icpmi_pose_graph_loop_weights(self._h, None, None, 0, C.byref(n)))
        w, d = np.zeros(n.value), np.zeros(n.value)
        if n.value:
            self.ctx._check(self._lib.icpmi_pose_graph_loop_weights(self._h, capi._dp(w), capi._dp(d), n.value,
                                                                    C.byref(n)))
        return w, d

    def joint_marginal_covariance(self, indices):
        """-> the (6q, 6q) joint marginal covariance of the q distinct poses `indices` at the optimised values
        (icpmi_pose_graph_marginals; GTSAM's Marginals::jointMarginalCovariance, not in the reference): block (a, b) is
        (H^-1)[indices[a], indices[b]] in the tangent order (omega, v).  Raises unless the optimised state of the last
        optimize() holds.  The first call after an optimize() factors H; later ones only solve."""
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        q = idx.shape[0]
        out = np.zeros((6 * q, 6 * q))
        self.ctx._check(self._lib.icpmi_pose_graph_marginals(self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)), q,
                                                             capi._dp(out)))
        return out

    def marginal_covariance(self, index):
        """-> the 6 x 6 marginal covariance of one pose (Marginals::marginalCovariance)"""
        return self.joint_marginal_covariance([int(index)])

    def relative_covariance(self, i, j):
        """-> the 6 x 6 first-order covariance of the tangent of X_i^-1 X_j (icpmi_pose_graph_relative_covariance)"""
        out = np.zeros((6, 6))
        self.ctx._check(self._lib.icpmi_pose_graph_relative_covariance(self._h, int(i), int(j), capi._dp(out)))
        return out

    def closure_distance(self, i, j, relative_transform, edge_covariance):
        """-> d^2 = e^T (Sigma_rel + edge_covariance)^-1 e with e = Log(rel^-1 X_i^-1 X_j): the squared Mahalanobis
        distance of a proposed edge i -> j against the graph (icpmi_pose_graph_closure_distance), chi-squared with 6
        degrees of freedom for a true closure."""
        T = _T(relative_transform)
        E = np.ascontiguousarray(edge_covariance, dtype=np.float64)
        if E.shape != (6, 6):
            raise ValueError("expected a 6 x 6 covariance matrix")
        d2 = C.c_double(0.0)
        self.ctx._check(self._lib.icpmi_pose_graph_closure_distance(self._h, int(i), int(j), capi._dp(T), capi._dp(E),
                                                                    C.byref(d2)))
        return d2.value

    def optimize(self):
        """pose_graph.cpp:147-171: False on an empty graph or where a factor names a pose with no estimate"""
        info = capi.PoseGraphInfo()
        hist = np.zeros(self.config.max_iterations + 1)
        rc = self._lib.icpmi_pose_graph_optimize(self._h, C.byref(info), capi._dp(hist), hist.shape[0])
        if rc == capi.ERR_ARG:
            self.stats = None
            return False
        self.ctx._check(rc)
        self.stats = PoseGraphStats(info, hist)
        return bool(info.optimized)

    def get_pose(self, index):
        """pose_graph.cpp:177-186"""
        out = np.zeros((4, 4))
        self.ctx._check(self._lib.icpmi_pose_graph_pose(self._h, int(index), capi._dp(out)))
        return out

    def get_all_poses(self):
        """pose_graph.cpp:188-200"""
        n = C.c_int64(0)
        self.ctx._check(self._lib.icpmi_pose_graph_poses(self._h, None, 0, C.byref(n), None))
        out = np.zeros((n.value, 4, 4))
        if n.value:
            self.ctx._check(self._lib.icpmi_pose_graph_poses(self._h, capi._dp(out), n.value, C.byref(n), None))
        return list(out)

    def _size(self):
        n, lc, info = C.c_int64(0), C.c_int64(0), capi.PoseGraphInfo()
        self.ctx._check(self._lib.icpmi_pose_graph_size(self._h, C.byref(n), C.byref(lc), C.byref(info)))
        return n.value, lc.value, info

    def size(self):
        return self._size()[0]

    def loop_closure_count(self):
        return self._size()[1]

    def get_final_error(self):
        return self._size()[2].final_error

    def get_iterations(self):
        return self._size()[2].iterations
