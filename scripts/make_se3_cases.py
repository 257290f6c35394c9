#!/usr/bin/env python3
"""tests/golden/se3_cases.npz: inputs and 60-digit results for the device SE(3) maps (csrc/se3.h), and the errors of the
fp64 CPU restatement (scripts/pose_graph_ref.py) against them.  numpy + mpmath, deterministic: running it again gives the
same bytes (tests/test_se3_cases.py).

    python scripts/make_se3_cases.py [out.npz]

The reference evaluates the closed forms that se3.h's comments state -- A = sin t / t ... F = (2t - 3 sin t + t cos t) /
(2 t^5), R = I + A W + B W^2, t = (I + B W + C W^2) v, the Shepperd quaternion with w >= 0 and omega = 2 atan2(|q|, w) q /
|q|, v = (I - W/2 + D W^2) t, Jr^-1 = [Jw^-1, 0; -Jw^-1 Q Jw^-1, Jw^-1] -- on the exact values of the fp64 inputs, with the
series limits only at t = 0.  Results are good to 60 digits: the arithmetic carries GUARD more, because F's numerator
cancels 50 digits at t = 1e-12.  They are then rounded to fp64.

Cases are twists (omega, v) = (theta * axis, v): every theta class below with six axes (two of +-x, +-y, +-z, so that
the fp64 seams at kSe3Tiny and kSe3Small are hit exactly; one of those tilted by 1e-3; one of (1,1,0), (1,0,1), (1,1,1);
two random) and all six kinds of v, plus the axes a class is there for (all six axis-aligned ones at the pi/2 Shepperd
seam, the tied and the (1,1,1) axes from theta = 2 up).  The pose of a case is the fp64-rounded 60-digit exp of its twist;
it is the input of log, and of inverse / compose / adjoint for every fourth case (compose with the pose of `partner`).

Errors are max-abs over a part of the output and over the cases of a theta class.  Rotation parts are absolute;
translation-carrying parts (v of exp and log, the coupling block of Jr^-1, t^ R of the adjoint, t of inverse and
compose) are divided by 1 + |v|_inf of the twist (both twists for compose); the coefficients are relative."""
import os
import sys
import zipfile

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_graph_ref as R  # noqa: E402

DIGITS, GUARD = 60, 100
PI = float(np.pi)
_dn = lambda x: float(np.nextafter(x, 0.0))        # noqa: E731
_up = lambda x: float(np.nextafter(x, np.inf))     # noqa: E731

THETAS = [
    ("0", 0.0), ("1e-12", 1e-12), ("1e-5", 1e-5),
    ("9.9e-9", 9.9e-9), ("tiny-", _dn(1e-8)), ("tiny", 1e-8), ("tiny+", _up(1e-8)), ("1.01e-8", 1.01e-8),
    ("1.9e-6", 1.9e-6), ("2.1e-6", 2.1e-6),
    ("0.0999999", 0.0999999), ("small-", _dn(0.1)), ("small", 0.1), ("small+", _up(0.1)), ("0.1000001", 0.1000001),
    ("0.5", 0.5), ("2", 2.0),
    ("pi/2-", PI / 2 - 1e-9), ("pi/2+", PI / 2 + 1e-9), ("2pi/3-", 2 * PI / 3 - 1e-9), ("2pi/3+", 2 * PI / 3 + 1e-9),
    ("3.0", 3.0), ("pi-1e-3", PI - 1e-3), ("pi-1e-6", PI - 1e-6), ("pi-1e-9", PI - 1e-9),
    ("3.5", 3.5), ("5.0", 5.0),
]
V_KINDS = ("zero", "ex", "ey", "ez", "sigma3", "1e3")
N_RANDOM = 12               # axes: 6 aligned, those 6 tilted, (1,1,0), (1,0,1), (1,1,1), then the random ones
AXIS_110, AXIS_101, AXIS_111 = 12, 13, 14
SUBSET_EVERY = 4            # inverse / compose / adjoint on every fourth case


def axes():
    e = np.eye(3)
    a = [e[0], e[1], e[2], -e[0], -e[1], -e[2]]
    a += [x + 1e-3 * np.roll(x, 1) for x in a[:6]]
    a += [np.array([1.0, 1.0, 0.0]), np.array([1.0, 0.0, 1.0]), np.array([1.0, 1.0, 1.0])]
    rng = np.random.default_rng(6355)
    a += list(rng.normal(size=(N_RANDOM, 3)))
    a = np.stack(a)
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def case_list():
    """(class, axis, v kind) of every case, class-major."""
    out = []
    for ti, (name, th) in enumerate(THETAS):
        ax = [ti % 6, (ti + 1) % 6, 6 + ti % 6, 12 + ti % 3, 15 + (2 * ti) % 12, 15 + (2 * ti + 1) % 12]
        if name.startswith("pi/2"):
            ax += [a for a in range(6) if a not in ax]
        if th >= 2.0:
            ax += [a for a in (AXIS_110, AXIS_101, AXIS_111) if a not in ax]
        out += [(ti, a, (k + ti) % 6) for k, a in enumerate(ax)]
    return out


def inputs():
    A = axes()
    cl = case_list()
    rng = np.random.default_rng(950)
    xi = np.zeros((len(cl), 6))
    for k, (ti, a, vk) in enumerate(cl):
        xi[k, :3] = THETAS[ti][1] * A[a] + 0.0          # + 0.0: no negative zeros
        if 1 <= vk <= 3:
            xi[k, 2 + vk] = 1.0
        elif vk == 4:
            xi[k, 3:] = rng.normal(0.0, 3.0, 3)
        elif vk == 5:
            xi[k, 3:] = rng.normal(0.0, 1e3, 3)
    n = len(cl)
    partner = (5 * np.arange(n) + 11) % n
    return A, np.array(cl, dtype=np.int32), xi, partner.astype(np.int32)


# ------------------------------------------------------------------------------------------- the reference (mpmath)

def _m(a):
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in np.asarray(a, dtype=np.float64).reshape(-1, 3)])


def _v(a):
    return mp.matrix([mp.mpf(float(x)) for x in a])


def _hat(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def mp_coefs(t):
    if t == 0:
        f = mp.mpf
        return f(1), f(1) / 2, f(1) / 6, f(1) / 12, f(1) / 24, f(1) / 120
    s, c = mp.sin(t), mp.cos(t)
    return (s / t, (1 - c) / t ** 2, (t - s) / t ** 3, 1 / t ** 2 - (1 + c) / (2 * t * s),
            (t ** 2 + 2 * c - 2) / (2 * t ** 4), (2 * t - 3 * s + t * c) / (2 * t ** 5))


def _norm(w):
    return mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)


def mp_exp(xi):
    w, v = _v(xi[:3]), _v(xi[3:])
    W = _hat(w)
    A, B, C = mp_coefs(_norm(w))[:3]
    I = mp.eye(3)
    return I + A * W + B * W * W, (I + B * W + C * W * W) * v


def shepperd_branch(Rm, tr):
    """0 w, 1 x, 2 y, 3 z: the largest quaternion component, se3.h's conditions."""
    if tr >= Rm[0, 0] and tr >= Rm[1, 1] and tr >= Rm[2, 2]:
        return 0
    if Rm[0, 0] >= Rm[1, 1] and Rm[0, 0] >= Rm[2, 2]:
        return 1
    return 2 if Rm[1, 1] >= Rm[2, 2] else 3


def mp_log(T12):
    Rm, t = _m(T12[:9]), _v(T12[9:])
    r = Rm
    br = shepperd_branch(r, r[0, 0] + r[1, 1] + r[2, 2])
    Rf = np.asarray(T12[:9], dtype=np.float64).reshape(3, 3)
    assert br == shepperd_branch(Rf, Rf[0, 0] + Rf[1, 1] + Rf[2, 2]), "branch depends on the rounding of the trace"
    if br == 0:
        w = mp.sqrt(1 + r[0, 0] + r[1, 1] + r[2, 2]) / 2
        x, y, z = (r[2, 1] - r[1, 2]) / (4 * w), (r[0, 2] - r[2, 0]) / (4 * w), (r[1, 0] - r[0, 1]) / (4 * w)
    elif br == 1:
        x = mp.sqrt(1 + r[0, 0] - r[1, 1] - r[2, 2]) / 2
        w, y, z = (r[2, 1] - r[1, 2]) / (4 * x), (r[0, 1] + r[1, 0]) / (4 * x), (r[0, 2] + r[2, 0]) / (4 * x)
    elif br == 2:
        y = mp.sqrt(1 - r[0, 0] + r[1, 1] - r[2, 2]) / 2
        w, x, z = (r[0, 2] - r[2, 0]) / (4 * y), (r[0, 1] + r[1, 0]) / (4 * y), (r[1, 2] + r[2, 1]) / (4 * y)
    else:
        z = mp.sqrt(1 - r[0, 0] - r[1, 1] + r[2, 2]) / 2
        w, x, y = (r[1, 0] - r[0, 1]) / (4 * z), (r[0, 2] + r[2, 0]) / (4 * z), (r[1, 2] + r[2, 1]) / (4 * z)
    if w < 0:
        w, x, y, z = -w, -x, -y, -z
    s = mp.sqrt(x * x + y * y + z * z)
    g = 2 * mp.atan2(s, w) / s if s != 0 else 2 / w
    om = mp.matrix([g * x, g * y, g * z])
    W = _hat(om)
    D = mp_coefs(_norm(om))[3]
    return om, (mp.eye(3) - W / 2 + D * W * W) * t


def mp_jr_inv(xi):
    w, v = _v(xi[:3]), _v(xi[3:])
    W, V = _hat(w), _hat(v)
    _, _, C, D, E, F = mp_coefs(_norm(w))
    Ji = mp.eye(3) + W / 2 + D * W * W
    Q = (-V / 2 + C * (W * V + V * W - W * V * W) - E * (W * W * V + V * W * W - 3 * W * V * W)
         + F * (W * V * W * W + W * W * V * W))
    return Ji, -(Ji * Q * Ji)


def _f(M):
    return np.array([float(x) for x in M], dtype=np.float64)      # mpf -> the nearest fp64


def reference(xi, partner):
    n = len(xi)
    pose = np.zeros((n, 12))
    for k in range(n):
        Rm, t = mp_exp(xi[k])
        pose[k, :9], pose[k, 9:] = _f(Rm), _f(t)
    log = np.zeros((n, 6))
    jr = np.zeros((n, 18))
    for k in range(n):
        om, v = mp_log(pose[k])
        log[k, :3], log[k, 3:] = _f(om), _f(v)
        Ji, Lo = mp_jr_inv(xi[k])
        jr[k, :9], jr[k, 9:] = _f(Ji), _f(Lo)
    sub = np.arange(0, n, SUBSET_EVERY)
    inv_t = np.zeros((len(sub), 3))
    mul = np.zeros((len(sub), 12))
    adj_tr = np.zeros((len(sub), 9))
    for q, k in enumerate(sub):
        Ra, ta = _m(pose[k, :9]), _v(pose[k, 9:])
        Rb, tb = _m(pose[partner[k], :9]), _v(pose[partner[k], 9:])
        inv_t[q] = _f(-(Ra.T * ta))
        mul[q, :9], mul[q, 9:] = _f(Ra * Rb), _f(Ra * tb + ta)
        adj_tr[q] = _f(_hat(ta) * Ra)
    coefs = np.array([[float(c) for c in mp_coefs(mp.mpf(th))] for _, th in THETAS])
    return dict(pose=pose, ref_log=log, ref_jr=jr, subset=sub.astype(np.int32), ref_inv_t=inv_t, ref_mul=mul,
                ref_adj_tr=adj_tr, ref_coefs=coefs)


# ---------------------------------------------------------------------------- errors of an fp64 evaluation of the maps

def to44(p):
    p = np.asarray(p, dtype=np.float64)
    T = np.zeros(p.shape[:-1] + (4, 4))
    T[..., :3, :3] = p[..., :9].reshape(p.shape[:-1] + (3, 3))
    T[..., :3, 3] = p[..., 9:]
    T[..., 3, 3] = 1.0
    return T


def to12(T):
    T = np.asarray(T, dtype=np.float64)
    return np.concatenate([T[..., :3, :3].reshape(T.shape[:-2] + (9,)), T[..., :3, 3]], -1)


def restatement(fx):
    """The maps by scripts/pose_graph_ref.py, in the layout of the check program's output (tests/test_gpu_se3.py)."""
    xi, pose, sub = fx["xi"], fx["pose"], fx["subset"]
    th = fx["theta"]
    J = R.se3_jr_inv(xi)
    Ta, Tb = to44(pose[sub]), to44(pose[fx["partner"][sub]])
    Ad = R.adjoint(Ta)
    return dict(coefs=np.stack(R._coefs(th), -1), exp=to12(R.se3_exp(xi)), log=R.se3_log(to44(pose)),
                jr=np.concatenate([J[:, :3, :3].reshape(-1, 9), J[:, 3:, :3].reshape(-1, 9)], 1),
                inv=to12(R.inverse(Ta)), mul=to12(Ta @ Tb), adj=Ad)


def pack(fx):
    """The check program's input (scripts/micro/se3_check.hip): n, m, theta, xi, pose, a, b as one float64 array."""
    sub = fx["subset"]
    return np.concatenate([[float(len(fx["xi"])), float(len(sub))], fx["theta"], fx["xi"].ravel(), fx["pose"].ravel(),
                           fx["pose"][sub].ravel(), fx["pose"][fx["partner"][sub]].ravel()]).astype(np.float64)


def unpack(fx, raw):
    """The check program's output as the dict restatement() returns."""
    n, m = len(fx["xi"]), len(fx["subset"])
    assert raw.shape == (60 * n + 60 * m,), raw.shape
    out, at = {}, 0
    for name, rows, shape in (("coefs", n, (6,)), ("exp", n, (12,)), ("log", n, (6,)), ("jr6", n, (6, 6)),
                              ("inv", m, (12,)), ("mul", m, (12,)), ("adj", m, (6, 6))):
        size = rows * int(np.prod(shape))
        out[name] = raw[at:at + size].reshape((rows,) + shape)
        at += size
    J = out["jr6"]
    out["jr"] = np.concatenate([J[:, :3, :3].reshape(-1, 9), J[:, 3:, :3].reshape(-1, 9)], 1)
    return out


PARTS = ("exp", "log", "relog", "jr", "inv", "mul", "adj")


def case_errors(fx, got):
    """Normalised errors of `got` (the dict restatement() returns, from any fp64 evaluation): coefs (classes, 6), every
    other map (cases, 2) = (rotation part, translation-carrying part)."""
    xi, pose, sub = fx["xi"], fx["pose"], fx["subset"]
    vs = 1.0 + np.abs(xi[:, 3:]).max(axis=1)
    vs2 = vs[sub] + vs[fx["partner"][sub]] - 1.0
    mx = lambda a: np.abs(a).max(axis=1)  # noqa: E731
    rc = fx["ref_coefs"][fx["cases"][:, 0]]
    out = {"coefs": np.abs(got["coefs"] - rc) / np.abs(rc)}
    out["exp"] = np.stack([mx(got["exp"][:, :9] - pose[:, :9]), mx(got["exp"][:, 9:] - pose[:, 9:]) / vs], 1)
    out["log"] = np.stack([mx(got["log"][:, :3] - fx["ref_log"][:, :3]),
                           mx(got["log"][:, 3:] - fx["ref_log"][:, 3:]) / vs], 1)
    re = to12(R.se3_exp(got["log"]))                      # the log put through the restatement's exp, against its input
    out["relog"] = np.stack([mx(re[:, :9] - pose[:, :9]), mx(re[:, 9:] - pose[:, 9:]) / vs], 1)
    out["jr"] = np.stack([mx(got["jr"][:, :9] - fx["ref_jr"][:, :9]), mx(got["jr"][:, 9:] - fx["ref_jr"][:, 9:]) / vs], 1)
    Rt = pose[sub, :9].reshape(-1, 3, 3).transpose(0, 2, 1).reshape(-1, 9)
    out["inv"] = np.stack([mx(got["inv"][:, :9] - Rt), mx(got["inv"][:, 9:] - fx["ref_inv_t"]) / vs[sub]], 1)
    out["mul"] = np.stack([mx(got["mul"][:, :9] - fx["ref_mul"][:, :9]),
                           mx(got["mul"][:, 9:] - fx["ref_mul"][:, 9:]) / vs2], 1)
    Ad = got["adj"]
    Rp = pose[sub, :9]
    rot = np.maximum(mx(Ad[:, :3, :3].reshape(-1, 9) - Rp), mx(Ad[:, 3:, 3:].reshape(-1, 9) - Rp))
    rot = np.maximum(rot, mx(Ad[:, :3, 3:].reshape(-1, 9)))
    out["adj"] = np.stack([rot, mx(Ad[:, 3:, :3].reshape(-1, 9) - fx["ref_adj_tr"]) / vs[sub]], 1)
    return out


def class_errors(fx, errs):
    """Per theta class: the largest case error (cases of the class; for inverse / compose / adjoint, of the subset)."""
    nc = len(fx["theta_values"])
    cls = fx["cases"][:, 0]
    out = {"coefs": np.zeros((nc, 6))}
    for c in range(nc):
        out["coefs"][c] = errs["coefs"][cls == c].max(axis=0)
    for m in PARTS:
        e = errs[m]
        k = cls if len(e) == len(cls) else cls[fx["subset"]]
        out[m] = np.zeros((nc, 2))
        for c in range(nc):
            if (k == c).any():
                out[m][c] = e[k == c].max(axis=0)
    return out


def make():
    mp.mp.dps = DIGITS + GUARD
    A, cases, xi, partner = inputs()
    fx = dict(class_names=np.array([n for n, _ in THETAS]), theta_values=np.array([t for _, t in THETAS]),
              v_kinds=np.array(V_KINDS), axes=A, cases=cases, xi=xi, partner=partner)
    fx["theta"] = fx["theta_values"][cases[:, 0]]
    fx.update(reference(xi, partner))
    ce = class_errors(fx, case_errors(fx, restatement(fx)))
    for m, e in ce.items():
        fx["err_" + m] = e
    del fx["theta"]
    return fx


def load(path):
    with np.load(path) as z:
        fx = {k: z[k] for k in z.files}
    fx["theta"] = fx["theta_values"][fx["cases"][:, 0]]
    return fx


def save(path, fx):
    """An .npz with nothing of the day in it: stored members in sorted order, one fixed timestamp."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for k in sorted(fx):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.ascontiguousarray(fx[k]), version=(1, 0), allow_pickle=False)


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(HERE), "tests", "golden", "se3_cases.npz")
    fx = make()
    save(out, fx)
    print("%s: %d cases, %d bytes" % (out, len(fx["xi"]), os.path.getsize(out)))
    for m in ("coefs",) + PARTS:
        print("  restatement %-6s max %s" % (m, np.array2string(fx["err_" + m].max(axis=0), precision=3)))
