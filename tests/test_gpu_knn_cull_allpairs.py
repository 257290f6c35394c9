"""The target's 20-NN pass on the all-pairs engine (SEARCH_MFMA_BF16) culls its coarse pass on targets of more than 12
splits, as the culled engine's does (launch_knn in capi.hip: k_knn_group_cull + k_nn_coarse_groups<true>); the ICP loop of
the engine stays all pairs.  Nothing may change in any bit: every case runs in child processes -- the all-pairs engine
with the cull (the default), the same with ICPMI_KNN_CULL=0 (the all-pairs coarse pass: the reference leg), and the culled
engine -- and normals, poses and error histories are compared byte for byte.  m = 26,001 is 13 splits, the smallest
target that takes the new branch, with a partial last split and a short last group (not a multiple of 64 or 2,048);
m = 24,576 is 12 splits, where the launches stay what they were.  ICPMI_SMALL=0 as in test_gpu_nn_reuse.py.
Marked gpu: runs on the MI355X box only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (26001, 24576)
CLOUDS = ("uniform", "lidar", "coincident_nan", "far_cluster")

# The child: argv[2] = output .npz, argv[3] = engine (2 or 3), argv[4] = "1" to run the registrations too.
_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import torch  # noqa: F401
from lidar_slam_from_scratch_amd import capi, dist as icpdist, synth

engine = int(sys.argv[3])

def clouds(m):
    yield "uniform", synth.c3_uniform(m, seed=31, perm_seed=32)[1]
    # a LiDAR-like scan: the raw returns of one sweep over the synthetic street, every few of them, m in all
    scan = synth.lidar_frame(0, voxel=0.0)
    assert scan.shape[0] >= m, scan.shape
    yield "lidar", scan[(np.arange(m, dtype=np.int64) * scan.shape[0]) // m]
    # 300 coincident points (their lists overflow) and three NaN rows (no list at all): k_knn_exact_rows answers
    t = synth.c3_uniform(m, seed=33, perm_seed=34)[1].copy()
    rng = np.random.default_rng(35)
    t[rng.choice(m, 300, replace=False)] = t[17]
    t[[5, m // 2, m - 1]] = np.nan
    yield "coincident_nan", t
    # 40 points scattered far outside the cloud: their neighbours are hundreds of metres away, so their groups' bounds
    # span the whole cloud and the box test has to keep the splits for them
    t = synth.c3_uniform(m, seed=36, perm_seed=37)[1].copy()
    rng = np.random.default_rng(38)
    t[rng.choice(m, 40, replace=False)] = np.array([600.0, -500.0, 200.0]) + rng.normal(0.0, 150.0, size=(40, 3))
    yield "far_cluster", t

out, info = {}, {}
for m in (26001, 24576):
    for name, tgt in clouds(m):
        assert tgt.shape == (m, 3)
        ctx = capi.Context(device=0, search=engine, profile=1)
        out["%s_%d" % (name, m)] = ctx.estimate_normals(tgt, 20)
        p = ctx.get_profile()
        info["%s_%d" % (name, m)] = {"knn_fallback_rows": int(p["knn_fallback_rows"]), "knn_culled_launches": int(p["knn_culled_launches"])}
        ctx.close()

if sys.argv[4] == "1":
    src, tgt, _ = synth.c3_uniform(26001, seed=41, perm_seed=42)
    cfg = lambda: capi.Context.make_config(max_iterations=12, tolerance=0.0, min_error=0.0)
    ctx = capi.Context(device=0, search=engine, profile=1)
    res, hist = ctx.align(src, tgt, cfg())
    p = ctx.get_profile()
    rows, blocks = ctx.nn_reuse_passes()
    out["align_T"] = np.array(res.transformation[:])
    out["align_hist"] = np.asarray(hist, dtype=np.float64)
    info["align"] = {"num_iterations": int(res.num_iterations), "converged": int(res.converged), "rows": [int(r) for r in rows],
                     "blocks": [int(b) for b in blocks], "nn_group_pairs": int(p["nn_group_pairs"]),
                     "bounded_launches": int(p["bounded_launches"]), "knn_culled_launches": int(p["knn_culled_launches"])}
    ctx.close()
    group = icpdist.LocalGroup(2)
    def body(rank):
        lo, hi = icpdist.shard_bounds(src.shape[0], 2, rank)
        c = capi.Context(device=0, search=engine, profile=1)
        group.attach(c, rank)
        res, hist = c.align(src[lo:hi], tgt, cfg())
        culled = int(c.get_profile()["knn_culled_launches"])
        c.comm_finalize(); c.close()
        return np.array(res.transformation[:]), np.asarray(hist, dtype=np.float64), int(res.num_iterations), culled
    for rank, (T, hist, its, culled) in enumerate(group.run(body)):
        out["rank%d_T" % rank], out["rank%d_hist" % rank] = T, hist
        info["rank%d" % rank] = {"num_iterations": its, "knn_culled_launches": culled}
np.savez(sys.argv[2], **out)
print(json.dumps(info))
"""


def _run(tmp, name, engine, cull, registrations):
    env = dict(os.environ, ICPMI_SMALL="0")
    env.pop("ICPMI_KNN_CULL", None)
    if not cull:
        env["ICPMI_KNN_CULL"] = "0"
    path = str(tmp / (name + ".npz"))
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path, str(engine), "1" if registrations else "0"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(path)), json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def legs(tmp_path_factory):
    """(arrays, counters) of the three legs, computed once: all-pairs engine with the cull, without it, culled engine"""
    tmp = tmp_path_factory.mktemp("knn_cull")
    return {"on": _run(tmp, "on", 2, True, True), "off": _run(tmp, "off", 2, False, True),
            "pruned": _run(tmp, "pruned", 3, True, False)}


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("cloud", CLOUDS)
def test_normals_byte_for_byte(legs, cloud, m):
    key = "%s_%d" % (cloud, m)
    on, off, pruned = (legs[k][0][key] for k in ("on", "off", "pruned"))
    fb = [legs[k][1][key]["knn_fallback_rows"] for k in ("on", "off", "pruned")]
    print(key, "knn_fallback_rows on / off / culled engine:", fb,
          "knn_culled_launches:", [legs[k][1][key]["knn_culled_launches"] for k in ("on", "off", "pruned")])
    assert on.shape == (m, 3)
    assert _same(on, off), key
    assert _same(on, pruned), key
    assert fb[0] == fb[1] == fb[2], fb
    if cloud == "coincident_nan":
        assert fb[0] >= 3, fb                    # (the NaN rows at least)
        assert np.isnan(on).any(axis=1).sum() >= 3
    else:
        assert np.isfinite(on).all(), key


@pytest.mark.parametrize("cloud", CLOUDS)
def test_the_cull_runs_from_13_splits_and_not_at_12(legs, cloud):
    """knn_culled_launches counts the k-NN coarse passes that ran over the surviving (group, split) pairs: one per
    estimate_normals call at 13 splits with the switch on, none with it off, none at 12 splits either way (the parent's
    launches); the culled engine culls at every size."""
    c = {(leg, m): legs[leg][1]["%s_%d" % (cloud, m)]["knn_culled_launches"] for leg in ("on", "off", "pruned") for m in SIZES}
    assert c[("on", 26001)] == 1 and c[("off", 26001)] == 0, c
    assert c[("on", 24576)] == 0 and c[("off", 24576)] == 0, c
    assert c[("pruned", 26001)] == 1 and c[("pruned", 24576)] == 1, c


def test_a_registration_keeps_every_bit(legs):
    """align of a 26,001 -> 26,001 pair, 12 iterations, tolerance 0, all-pairs engine: pose, history, iteration count and
    the rows and workgroup columns of every pass with the cull equal those without; the loop ran all pairs on both."""
    (a, ia), (b, ib) = legs["on"], legs["off"]
    assert _same(a["align_T"], b["align_T"]) and _same(a["align_hist"], b["align_hist"])
    assert a["align_hist"].shape == (13,) and np.isfinite(a["align_hist"]).all()
    ra, rb = ia["align"], ib["align"]
    assert ra["num_iterations"] == rb["num_iterations"] == 12 and ra["converged"] == rb["converged"]
    assert ra["rows"] == rb["rows"] and ra["blocks"] == rb["blocks"] and len(ra["rows"]) == 13
    assert ra["rows"][0] == ra["rows"][1] == 26001
    assert ra["bounded_launches"] == rb["bounded_launches"] == 13
    assert ra["nn_group_pairs"] == 0 and rb["nn_group_pairs"] == 0
    assert ra["knn_culled_launches"] == 1 and rb["knn_culled_launches"] == 0


def test_two_ranks_keep_every_bit(legs):
    """dist.LocalGroup(2) on the same pair: each rank computes the normals of its range of sorted rows (row0 a multiple of
    512) with the cull, and pose and history equal those of the run without it, bit for bit."""
    (a, ia), (b, ib) = legs["on"], legs["off"]
    for rank in (0, 1):
        assert _same(a["rank%d_T" % rank], b["rank%d_T" % rank]), rank
        assert _same(a["rank%d_hist" % rank], b["rank%d_hist" % rank]), rank
        assert ia["rank%d" % rank]["num_iterations"] == ib["rank%d" % rank]["num_iterations"] == 12
        assert ia["rank%d" % rank]["knn_culled_launches"] == 1 and ib["rank%d" % rank]["knn_culled_launches"] == 0
    assert _same(a["rank0_T"], a["rank1_T"]) and _same(a["rank0_hist"], a["rank1_hist"])
