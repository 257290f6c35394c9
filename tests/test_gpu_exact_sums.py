"""Every reduction tree of a pass's normal equations, and the 6 x 6 step, held to bits on exact fixtures.

tests/test_gpu_normal_matrix.py compares the sums with math.fsum on real geometry and needs a tolerance, because the
device adds rounded products in an order of its own.  Here the clouds of scripts/exact_lattice.py make every product and
every partial sum an exactly representable number (tests/test_exact_fixture.py holds the fixtures to that on the CPU),
so any order of additions gives the same bits and the device's sums must EQUAL an integer reference: one partial row
dropped, added twice or read past the end changes an integer.  The source sizes are not literals: tests/cpp/
loop_plan_print.cpp prints csrc/loop_plan.h's plan for each path, and the sizes are picked from it so that the partial
rows land on every edge of finish_sums (4, 8, 16 load slots, the second round), on the first sizes of the sum tree
(k_sum_groups: full groups, a short last group, more than 128 groups) and on partial last workgroups.

The small-cloud pass sums its partial rows in finish_sums itself, at 1,024 rows too, where the plan sets sum_tree: no
k_sum_groups runs there (queue_pass_small, capi.hip), so only the general kernels and the culled engine reach the sum
tree, and the tuples this test prints say for every path what ran, not what the plan's field says.

Paths (asserted from the profile counters against the plan, under a rule too): the exact fp64 engine, the small-cloud kernel (a target of 3 splits), the
all-pairs engine's general kernels and the culled engine (a target of 15 splits).

Equality.  `same` is equality of values with no NaN: for finite non-zero doubles equal bits; +0.0 and -0.0, which an
all-zero column may come out as, are one value.

The step.  With exact sums the solve's inputs are bit-equal to the oracle's, the library is built -ffp-contract=off and
both sides restate Eigen's LDLT operation by operation: the solution x, hence the translation column, must be
bit-equal.  The rotation block is R = (I + s K) + ((1 - c) K) K with K formed from bit-equal x on both sides; only s and c
differ: the device's sincos_step is within 2 ulp of the device library (test_wave_step_gives_the_one_lane_step_bits),
which is within 1 ulp of the true value, as is libm: |ds| <= 4 ulp(s) <= 2^-50, |dc| <= 4 ulp(c) <= 2^-50.  |K_ij| <= 1
and |(K K)_ij| <= 1, so the two terms move by at most 2^-50 each; and the twelve rounded operations that form an entry
(1 - c, s K_ij, its sum with I, three (1 - c) K_ik, three products, two additions, the last addition), each on a result
of magnitude at most 2, may round differently on the two sides by at most 2 * 2^-53 * 2 = 2^-51 each.
    ROT_BOUND = 2^-50 + 2^-50 + 12 * 2^-51 = 10 * 2^-50 = 8.9e-15 per entry
The tests print the worst observed ratio to that bound."""
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import torch  # noqa: F401  (first: one HIP runtime per process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import exact_lattice as xl  # noqa: E402
from lidar_slam_from_scratch_amd import capi  # noqa: E402

pytestmark = pytest.mark.gpu

ROT_BOUND = 10.0 * 2.0 ** -50
CSRC = os.path.join(ROOT, "lidar_slam_from_scratch_amd", "csrc")
# path -> (the gpu_ctx engine that runs it, patches of its target)
PATHS = {"exact": ("exact_f64", 3), "small": ("mfma_bf16", 3), "general": ("mfma_bf16", 18), "culled": ("mfma_pruned", 18)}
FIN_EDGES = (1, 127, 128, 129, 256, 257, 512, 513)
LARGEST_N = 140000


def same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))


_targets = {}


def target(patches):
    """the lattice target of that many patches, or the "cyclic" one: made once, shared, left unchanged"""
    if patches not in _targets:
        _targets[patches] = xl.target(3, cyclic=True) if patches == "cyclic" else xl.target(patches)
    return _targets[patches]


def split_targets():
    """targets per split of the MFMA engines, from the headers"""
    found = {}
    for header, name in (("nn_mfma.h", "kSplitTiles"), ("loop_plan.h", "kTile")):   # (nn_mfma.h is device code: not for the printer)
        with open(os.path.join(CSRC, header)) as f:
            hit = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, f.read())
        assert hit, "%s: no `constexpr int %s = <number>;` to read the targets per split from" % (header, name)
        found[name] = int(hit.group(1))
    return found["kSplitTiles"] * found["kTile"]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """-> plan(path, rule) = (constants, runs): loop_plan.h's plan of every source size up to LARGEST_N on that path, as
    runs (n_first, n_last, rblocks, sum_tree, rblocks2, fin_blocks, small, fused, pruned, resolve_waves)"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("plan") / "loop_plan_print")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "loop_plan_print.cpp"), "-o", exe], check=True)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    per_split = split_targets()
    seen = {}

    def plan(path, rule="none"):
        if (path, rule) not in seen:
            engine, patches = PATHS[path]
            m = len(target(patches).pts)
            facts = ["engine=%s" % ("exact" if engine == "exact_f64" else "mfma"), "pruned=%d" % (engine == "mfma_pruned"),
                     "splits=%d" % (0 if engine == "exact_f64" else (m + per_split - 1) // per_split), "cu=%d" % cu,
                     "rule=%s" % rule, "n=1:%d" % LARGEST_N]
            r = subprocess.run([exe] + facts, capture_output=True, text=True, timeout=60, check=True)
            lines = r.stdout.strip().splitlines()
            assert lines[0].startswith("constants ") and not any(ln.endswith("refused") for ln in lines[1:]), r.stdout[:400]
            seen[(path, rule)] = ([int(v) for v in lines[0].split()[1:]], [tuple(int(v) for v in ln.split()) for ln in lines[1:]])
        return seen[(path, rule)]

    return plan


def pick(run):
    """a size of the run with a partial last workgroup where the run has one: its first size (one row into the last
    workgroup), or for the run that starts at one row its last size but one"""
    first, last = run[0], run[1]
    return first if first > 1 else max(1, last - 1)


def sizes_for(path, planner, rule="none"):
    """-> sorted [(n, rblocks, fin_blocks, sum_tree, rblocks2)]: the sizes of this path that the plan puts on the edges.
    The small-cloud pass (queue_pass_small, capi.hip) hands its rblocks rows to the finish step itself and launches no
    k_sum_groups, whatever the plan's sum_tree says: its tuples say what runs -- fin_blocks = rblocks, no tree -- so its
    1,024-row sizes are two full rounds of finish_sums, not a sum tree."""
    (_min_q, small_max, group, tree_from), runs = planner(path, rule)
    is_small = path == "small"
    runs = [r for r in runs if bool(r[6]) == is_small]
    if is_small:
        assert runs and runs[-1][1] == small_max
    chosen = {}

    def take(run, n=None):
        n = pick(run) if n is None else n
        chosen[n] = (n, run[2], run[2], 0, 0) if is_small else (n, run[2], run[5], run[3], run[4])

    flat = [r for r in runs if not r[3]]
    for edge in FIN_EDGES:                                           # finish_sums' edges, without the tree in front
        hit = [r for r in flat if r[5] == edge]
        if hit:
            take(hit[0])
    tree = [r for r in runs if r[3]]
    wanted = [tree_from - 1, tree_from, tree_from + 1, (tree_from // group + 1) * group, (tree_from // group + 1) * group + group - 5]
    for rb in wanted:                                                # the tree's first sizes: full groups and a short last one
        hit = [r for r in runs if r[2] == rb]
        if hit:
            take(hit[0])
    cross = [r for r in tree if r[4] > FIN_EDGES[2]]                 # more group sums than finish_sums' four slots hold
    if cross:
        take(cross[0])
        before = [r for r in tree if r[4] == FIN_EDGES[2]]
        if before:
            take(before[-1], before[-1][1])                          # ... and the last size before, every workgroup full
    if is_small:
        take(runs[-1], small_max)                                    # the small-cloud kernel's largest source
    return [chosen[n] for n in sorted(chosen)]


def planned(planner, path, rule, n):
    """the plan's run that holds n source rows, on that path under that rule"""
    _constants, runs = planner(path, rule)
    return [r for r in runs if r[0] <= n <= r[1]][0]


def assert_path(ctx, run, tag):
    """The kernels that ran since reset_profile(), from the profile counters, against the plan's run of the call: the
    small-cloud kernel iff the plan says small, the culled engine's (row group, split) pairs iff it says pruned, a bounded
    resolve iff it says fused and not small (the switches are at their defaults).  Under a gate or weights the plan is
    never fused, hence never pruned: on the culled engine's context too such a call searches unfused over all pairs,
    and that is what is asserted of it."""
    small, fused, pruned = bool(run[6]), bool(run[7]), bool(run[8])
    prof = ctx.get_profile()
    seen = (prof["small_launches"], prof["nn_group_pairs"], prof["bounded_launches"])
    assert (seen[0] > 0) == small and (seen[1] > 0) == pruned and (seen[2] > 0) == (fused and not small), (tag, run, seen)


def assert_sums(nm, res, want, tag):
    assert nm.pairs == want.pairs, (tag, nm.pairs, want.pairs)
    assert nm.weight == want.weight, (tag, nm.weight, want.weight)
    bad = [(r, c, nm.JtJ[r, c], want.JtJ[r, c]) for r in range(6) for c in range(6) if not nm.JtJ[r, c] == want.JtJ[r, c]]
    assert not bad, (tag, bad)
    assert same(nm.Jtb, want.Jtb), (tag, nm.Jtb, want.Jtb)
    assert nm.sum_sq == want.sum_sq, (tag, nm.sum_sq, want.sum_sq)
    assert res.final_error == math.sqrt(want.sum_sq / want.weight), (tag, res.final_error)


def zero_iterations():
    return capi.Context.make_config(max_iterations=0)


def one_iteration():
    return capi.Context.make_config(max_iterations=1, tolerance=0.0, min_error=0.0)


def paths_of(ctx):
    return [p for p, (engine, _) in PATHS.items() if engine == ctx.engine]


def test_device_normals_are_axis_vectors(gpu_ctx):
    for patches in sorted({PATHS[p][1] for p in paths_of(gpu_ctx)}):
        t = target(patches)
        assert same(np.abs(gpu_ctx.estimate_normals(t.pts, 20)), xl.axis_normals(t.axis)), patches


def test_sums_on_every_edge_of_the_plan(gpu_ctx, planner):
    ran = []
    for path in paths_of(gpu_ctx):
        t = target(PATHS[path][1])
        sizes = sizes_for(path, planner)
        fins = {s[2] for s in sizes if not s[3]}
        # what each path can reach (loop_plan.h): the k_reduce family leaves at most one row per CU
        assert fins >= set(FIN_EDGES if path != "exact" else FIN_EDGES[:5]), (path, sorted(fins))
        assert (path in ("general", "culled")) == any(s[3] for s in sizes), path     # (who reaches k_sum_groups)
        for n, rblocks, fin, tree, rblocks2 in sizes:
            src, keep, w4, want = xl.variant("plain", t, n)
            tag = (path, n, rblocks, fin, tree, rblocks2)
            gpu_ctx.reset_profile()
            res, _hist = gpu_ctx.align(src.pts, t.pts, zero_iterations())
            assert_path(gpu_ctx, planned(planner, path, "none", n), tag)
            assert_sums(gpu_ctx.last_normal_matrix(), res, want, tag)
            ran.append(tag)
    print("exact sums: (path, n, rblocks, rows finish_sums adds, k_sum_groups ran, its group sums)")
    for tag in ran:
        print("   ", tag)


def test_auto_sends_tiny_sources_to_the_exact_kernels(planner):
    (min_queries, _small_max, _g, _t), _runs = planner("small")
    t = target(3)
    ctx = capi.Context(device=0, search=capi.SEARCH_AUTO, profile=1)
    try:
        for n, path in ((1, "exact"), (min_queries - 1, "exact"), (min_queries, "small")):
            src, keep, w4, want = xl.variant("plain", t, n)
            ctx.reset_profile()
            res, _hist = ctx.align(src.pts, t.pts, zero_iterations())
            assert_path(ctx, planned(planner, path, "none", n), ("auto", n))
            assert_sums(ctx.last_normal_matrix(), res, want, ("auto", n))
    finally:
        ctx.close()


def rule_sizes(path, planner, rule):
    """two sizes under a rule: the first that puts the partial rows on finish_sums' 128-row edge, and an odd one beyond"""
    _c, runs = planner(path, rule)
    runs = [r for r in runs if bool(r[6]) == (path == "small") and not r[3]]
    edge = [r for r in runs if r[5] == FIN_EDGES[2]][0]
    beyond = [r for r in runs if r[5] == FIN_EDGES[2] + 9][0]
    return [(pick(edge), edge[5]), (pick(beyond) + 6, beyond[5])]


def test_gate_and_weights_at_equality(gpu_ctx, planner):
    cfg = zero_iterations()
    for path in paths_of(gpu_ctx):
        t = target(PATHS[path][1])
        for n, fin in rule_sizes(path, planner, "gate"):
            src, keep, _w4, want = xl.variant("gate", t, n)
            tag = (path, "gate", n, fin)
            assert 0 < want.pairs < n and src.outside.any()
            gpu_ctx.reset_profile()
            res, _hist, pairs = gpu_ctx.align_gated(src.pts, t.pts, cfg, xl.GATE)
            assert_path(gpu_ctx, planned(planner, path, "gate", n), tag)
            assert pairs == want.pairs, (tag, pairs, want.pairs)     # d^2 == g^2: in; one representable number beyond: out
            assert_sums(gpu_ctx.last_normal_matrix(), res, want, tag)
        for kind, rule in (("huber", (capi.ROBUST_HUBER, xl.HUBER_K)), ("gm", (capi.ROBUST_GEMAN_MCCLURE, xl.GM_K))):
            for n, fin in rule_sizes(path, planner, "robust"):
                src, keep, w4, want = xl.variant(kind, t, n)
                tag = (path, kind, n, fin)
                assert want.weight < n and len(np.unique(w4)) == (3 if kind == "huber" else 2)
                gpu_ctx.reset_profile()
                res, _hist, info = gpu_ctx.align_robust(src.pts, t.pts, cfg, rule)
                assert_path(gpu_ctx, planned(planner, path, "robust", n), tag)
                assert info.pairs == n and info.weight_sum == want.weight, (tag, info.pairs, info.weight_sum, want.weight)
                assert_sums(gpu_ctx.last_normal_matrix(), res, want, tag)
        # the gate and the weights together: the rows at the gate are kept, and with k = 4/64 the largest |b| among them
        # equals k, which Huber's a <= k still weighs 1: the gate fixture's sums again
        n, fin = rule_sizes(path, planner, "robust")[1]
        src, keep, _w4, want = xl.variant("gate", t, n)
        assert np.abs(src.off[keep]).max() == 4.0 * xl.HUBER_K
        gpu_ctx.reset_profile()
        res, _hist, info = gpu_ctx.align_robust(src.pts, t.pts, cfg, (capi.ROBUST_HUBER, 4.0 * xl.HUBER_K, xl.GATE))
        assert_path(gpu_ctx, planned(planner, path, "robust", n), (path, "huber behind the gate", n))
        assert info.pairs == want.pairs and info.weight_sum == want.weight, (path, n, info.pairs, want.pairs)
        assert_sums(gpu_ctx.last_normal_matrix(), res, want, (path, "huber behind the gate", n, fin))


_oracle_normals = {}


def oracle_normals(oracle, patches):
    if patches not in _oracle_normals:
        _oracle_normals[patches] = oracle.estimate_normals(target(patches).pts, None, 20, nthreads=4)
    return _oracle_normals[patches]


def assert_step(T, T_oracle, tag):
    """translation column to the bit, rotation block within ROT_BOUND -> the worst rotation error / ROT_BOUND"""
    assert same(T[:3, 3], T_oracle[:3, 3]), (tag, T[:3, 3], T_oracle[:3, 3], T[:3, 3] - T_oracle[:3, 3])
    assert same(T[3], [0.0, 0.0, 0.0, 1.0]), (tag, T[3])
    worst = float(np.abs(T[:3, :3] - T_oracle[:3, :3]).max()) / ROT_BOUND
    assert worst <= 1.0, (tag, worst, T[:3, :3] - T_oracle[:3, :3])
    return worst


def test_one_step_through_every_finish_kernel(gpu_ctx, oracle, planner):
    """k_finish_step_transform (exact, general), k_finish_step_transform_cull (culled), k_finish_step behind the small-cloud
    kernel and, under a rule, behind k_reduce.  Where the target has three patches the cyclic fixture runs too: all
    three rotation diagonals and all three translation diagonals of its JtJ are tied."""
    cfg = one_iteration()
    worst = 0.0
    for path in paths_of(gpu_ctx):
        patches = PATHS[path][1]
        fixtures = [("step", target(patches), oracle_normals(oracle, patches), len(target(patches).pts) + 1237)]
        if patches == 3:
            fixtures.append(("cyclic_step", target("cyclic"), oracle_normals(oracle, "cyclic"), len(target("cyclic").pts)))
        for kind, t, nrm, n in fixtures:
            tag = (path, kind, n)
            src, _keep, _w4, want = xl.variant(kind, t, n)
            T_oracle = oracle.solve_point_to_plane(src.pts, t.pts[src.match], nrm[src.match])
            angle = math.acos(min(1.0, (np.trace(T_oracle[:3, :3]) - 1.0) / 2.0))
            assert 1e-4 < angle < math.pi / 4, (tag, angle)          # the solution rotates
            gpu_ctx.reset_profile()
            res, hist = gpu_ctx.align(src.pts, t.pts, cfg)
            assert_path(gpu_ctx, planned(planner, path, "none", n), tag)
            assert res.loop_iterations == 1 and hist[0] == math.sqrt(want.sum_sq / want.weight), (tag, hist)
            T = np.array(res.transformation[:]).reshape(4, 4)
            ratio = assert_step(T, T_oracle, tag)
            # the same step behind a gate that keeps every row and under weights that are all one
            gpu_ctx.reset_profile()
            res_g, hist_g, pairs = gpu_ctx.align_gated(src.pts, t.pts, cfg, 1.0)
            assert_path(gpu_ctx, planned(planner, path, "gate", n), tag + ("gate",))
            gpu_ctx.reset_profile()
            res_h, hist_h, info = gpu_ctx.align_robust(src.pts, t.pts, cfg, (capi.ROBUST_HUBER, 1.0))
            assert_path(gpu_ctx, planned(planner, path, "robust", n), tag + ("huber",))
            assert pairs == n and info.pairs == n and info.weight_sum == float(n)
            for r, h in ((res_g, hist_g), (res_h, hist_h)):
                # (the history's second entry is the post-loop pass over the moved rows: rounded sums, each path's own order)
                assert same(np.array(r.transformation[:]), np.array(res.transformation[:])) and h[0] == hist[0], tag
            print("one step:", tag, "angle", angle, "worst rotation error / bound", ratio)
            worst = max(worst, ratio)
    print("one step: worst rotation error / bound over the paths", worst)


def test_batch_of_three_is_each_call_alone(gpu_ctx):
    def bits(nm):
        return (nm.JtJ.tobytes(), nm.Jtb.tobytes(), nm.sum_sq, nm.weight, nm.pairs, nm.T.tobytes())

    t = target(PATHS[paths_of(gpu_ctx)[0]][1])
    srcs = [xl.variant("step", t, 3001)[0].pts, xl.variant("plain", t, len(t.pts) + 77)[0].pts, xl.variant("huber", t, 4097)[0].pts]
    cfgs = [one_iteration(), one_iteration(), zero_iterations()]
    alone = []
    for s, cfg in zip(srcs, cfgs):
        res, hist = gpu_ctx.align(s, t.pts, cfg)
        alone.append((bytes(res.transformation), res.final_error, hist.tobytes(), bits(gpu_ctx.last_normal_matrix())))
    out = gpu_ctx.align_batch(srcs, [t.pts] * 3, cfgs)
    for k, (res, hist) in enumerate(out):
        assert (bytes(res.transformation), res.final_error, hist.tobytes(), bits(gpu_ctx.last_normal_matrix(k))) == alone[k], k


def test_hand_made_systems(gpu_ctx, oracle):
    worst = 0.0
    for name, (src, tgt, nrm, expect) in xl.hand_made_systems().items():
        T = gpu_ctx.solve_point_to_plane(src, tgt, nrm)
        T_oracle = oracle.solve_point_to_plane(src, tgt, nrm)
        if expect == "identity":
            assert same(T, np.eye(4)), (name, T)
        elif expect == "nan":
            assert np.array_equal(np.isnan(T), np.isnan(T_oracle)) and np.isnan(T).any(), (name, T, T_oracle)
            assert same(T[~np.isnan(T)], T_oracle[~np.isnan(T_oracle)]), (name, T, T_oracle)
        else:
            ratio = assert_step(T, T_oracle, name)
            print("hand-made system:", name, "worst rotation error / bound", ratio)
            worst = max(worst, ratio)
    print("hand-made systems: worst rotation error / bound", worst)
