"""Call-order tests: every entry point's bits survive a used context.

What a call returns depends on its arguments and on the state its documentation names, and on nothing else: a call on
a context that has done other things returns, byte for byte, what it returns as the first call on a fresh context, and
the k-th step of a stateful object (the odometry stream, a local map, a global map with its live plane, a store loop
detector, a pose graph, the occupancy set) returns what it returns in the object's undisturbed run.  The operations,
the threads and the harness are scripts/call_sequences.py's; equality of digests is the assertion, with no tolerance
anywhere.  The expected digests come from one fresh AUTO, profile=0 context per operation or thread, and are held to
the CPU oracle and the restatements in scripts/ first (test_fresh_contexts_...), with the suite's existing tolerances.

Every test prints how many (operation, context-history) pairs it asserted.  Marked gpu: runs on the MI355X only."""
import os
import sys
import threading

import numpy as np
import pytest

import torch  # noqa: F401  (first: one HIP runtime per process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import call_sequences as cs  # noqa: E402
from lidar_slam_from_scratch_amd import capi  # noqa: E402
from lidar_slam_from_scratch_amd.global_map import GlobalMap  # noqa: E402
from lidar_slam_from_scratch_amd.local_map import LocalMap, LocalMapConfig  # noqa: E402

pytestmark = pytest.mark.gpu

SEEDS = (11, 12, 13)
# the contexts of test 5: (search, profile)
CONFIGS = {"exact_f64": (capi.SEARCH_EXACT_F64, 0), "mfma_bf16": (capi.SEARCH_MFMA_BF16, 0),
           "mfma_pruned": (capi.SEARCH_MFMA_PRUNED, 0), "auto_profile_2": (capi.SEARCH_AUTO, 2)}


@pytest.fixture(scope="module")
def env():
    """Fails loudly (no skip, no fallback) when the HIP library or the device is missing."""
    from lidar_slam_from_scratch_amd import build
    build.build_library()
    e = cs.Env()
    yield e
    e.close()


_expected = {}


def expected_for(env, search, profile):
    """(operations, threads) on fresh contexts made with these options: computed once, shared, left unchanged"""
    if (search, profile) not in _expected:
        _expected[(search, profile)] = (cs.expected_ops(env, search, profile), cs.expected_threads(env, search, profile))
    return _expected[(search, profile)]


@pytest.fixture(scope="module")
def exp(env):
    return expected_for(env, capi.SEARCH_AUTO, 0)


def done(tally, what):
    print("%s: %d (operation, context-history) pairs asserted, %d differ" % (what, tally.count, len(tally.bad)))
    assert not tally.bad, (what, tally.bad[:12])


# ------------------------------------------------------------------ before any used context is tried
def test_fresh_contexts_hold_to_the_oracle_and_agree_with_each_other(env, exp, oracle):
    exp_ops, exp_threads = exp
    missing = [n for n in cs.OPS if n not in cs.CHECKS and not n.endswith(("gated_batch_2", "robust_batch_2"))]
    assert not missing, missing                                  # (the two batches are held to their single calls below)
    for name, check in cs.CHECKS.items():
        check(env, exp_ops[name], oracle)
    # a batch is bit-identical to the single calls of its pairs (capi.align_*_batch), which are held to the restatements
    cfg = capi.Context.make_config(**cs._cfg_kw(3))
    with cs.fresh() as ctx:
        for (s, t), run in zip(cs.BATCH[1:], ctx.align_gated_batch([env.I[s] for s, _ in cs.BATCH[1:]], [env.I[t] for _, t in cs.BATCH[1:]],
                                                                    cfg, cs.GATE_RC)):
            res, hist, pairs = ctx.align_gated(env.I[s], env.I[t], cfg, cs.GATE_RC)
            assert bytes(res) == bytes(run[0]) and (hist == run[1]).all() and pairs == run[2], (s, t)
        rule = (cs.GEMAN_MCCLURE, 0.1, cs.GATE_RC)
        for (s, t), run in zip(cs.BATCH[:2], ctx.align_robust_batch([env.I[s] for s, _ in cs.BATCH[:2]], [env.I[t] for _, t in cs.BATCH[:2]],
                                                                    cfg, rule)):
            res, hist, info = ctx.align_robust(env.I[s], env.I[t], cfg, rule)
            assert bytes(res) == bytes(run[0]) and (hist == run[1]).all() and bytes(info) == bytes(run[2]), (s, t)
            import robust_icp_ref
            ref = robust_icp_ref.robust_icp(env.I[s], env.I[t], rule[0], rule[1], rule[2], orc=oracle, **cs._cfg_kw(3))
            cs.check_against(res, hist, ref.transformation, ref.converged, ref.num_iterations, ref.error_history)
            assert info.pairs == ref.pairs
    # the stream's refused push was refused, the local map did evict, the detector did verify and accept a closure
    with cs.fresh() as ctx:
        try:
            ctx.stream_push_host(env.I["b_nan"], 0.5, 1000, capi.Context.make_config(max_iterations=1))
            refused = False
        except capi.IcpError as e:
            refused = e.code == capi.ERR_ARG
        assert refused
        lm = LocalMap(ctx, LocalMapConfig(voxel_size=0.5, max_range=10.0, capacity=1 << 15))
        lm.add(env.I["f16_0"], env.I["p16_0"])
        assert lm.add(env.I["f16_2"], env.I["p16_2"]).evicted > 0
        lm.close()
        gm, det, clouds = cs.loop_store_setup(ctx, env)
        for k, cloud in enumerate(clouds):
            gm.add_frame(cloud)
            det.add_frame(k, k)
            found = det.detect()
        assert any(r.match_frame == 0 and r.sector_shift not in (None, 0) and 0 < r.pairs <= len(clouds[-1]) for r in found), \
            [(r.match_frame, r.sector_shift, r.pairs, r.icp_fitness) for r in found]
    # run to run: the same digests from a second fresh context
    again_ops, again_threads = cs.expected_ops(env), cs.expected_threads(env)
    unstable = [n for n in cs.OPS if again_ops[n].digest != exp_ops[n].digest]
    unstable += ["%s[%d]" % (t, k) for t in cs.THREADS for k, d in enumerate(exp_threads[t]) if again_threads[t][k] != d]
    assert all(len(again_threads[t]) == len(exp_threads[t]) for t in cs.THREADS)
    assert not unstable, unstable
    print("fresh contexts: %d operations and %d thread steps, each twice" % (len(cs.OPS), sum(len(v) for v in exp_threads.values())))


def test_every_registration_runs_on_the_path_its_name_claims(env, tmp_path):
    """from the profile counters against csrc/loop_plan.h's plan, as tests/test_gpu_exact_sums.py::assert_path does"""
    exe = cs.build_plan_printer(tmp_path)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    with cs.fresh(capi.SEARCH_AUTO, 1) as ctx:
        for name, op in cs.OPS.items():
            if op.reg is None:
                continue
            path, run = cs.planned(exe, op.reg, cu)
            assert "_%s_" % path in name or (path == "exact" and "tiny_target" in name), (name, path)
            small, fused, pruned = bool(run[6]), bool(run[7]), bool(run[8])
            ctx.reset_profile()
            op.run(ctx, env)
            prof = ctx.get_profile()
            seen = (prof["small_launches"], prof["nn_group_pairs"], prof["bounded_launches"])
            assert (seen[0] > 0) == small and (seen[1] > 0) == pruned and (seen[2] > 0) == (fused and not small), (name, run, seen)


# ------------------------------------------------------------------ 1. every ordered pair
@pytest.mark.parametrize("first", list(cs.OPS))
def test_every_ordered_pair(env, exp, first):
    """A, then every B of the catalogue, on one context: A's leftovers meet every B, and every B's meet A"""
    exp_ops, _ = exp
    tally = cs.Tally(first)
    with cs.fresh() as ctx:
        for second in cs.OPS:
            tally.op(ctx, env, first, exp_ops, ("before", second))
            tally.op(ctx, env, second, exp_ops, ("after", first))
        tally.op(ctx, env, first, exp_ops, "last")
    done(tally, "pairs from %s" % first)


# ------------------------------------------------------------------ 2. shrink and grow
def shrink_and_grow(ctx, env, exp_ops, tally):
    for order, tag in zip(cs.size_orders(), ("descending", "ascending", "interleaved")):
        for name in order:
            tally.op(ctx, env, name, exp_ops, tag)


def test_shrink_and_grow(env, exp):
    """the tail of every grow-only buffer holds a bigger call's data while a smaller call runs"""
    tally = cs.Tally("sizes")
    with cs.fresh() as ctx:
        shrink_and_grow(ctx, env, exp[0], tally)
    done(tally, "shrink and grow")


# ------------------------------------------------------------------ 3. threads under fire
@pytest.mark.parametrize("name", list(cs.THREADS))
def test_thread_under_fire(env, exp, name):
    tally = cs.Tally(name)
    with cs.fresh() as ctx:
        cs.under_fire(ctx, env, name, 5, exp[0], exp[1], tally)
    done(tally, "%s under fire" % name)


@pytest.mark.parametrize("seed", SEEDS)
def test_all_threads_on_one_context(env, exp, seed):
    tally = cs.Tally("seed %d" % seed)
    with cs.fresh() as ctx:
        cs.run_plan(ctx, env, cs.shuffle_plan(seed, exp[1]), exp[1], tally, ("shuffle", seed))
    done(tally, "all threads, seed %d" % seed)


def test_local_map_between_foreign_searches(env, exp):
    """The named sequence of the remembered target (prepare_nn's `prep_valid = false`): an add leaves the table prepared
    as the next registration's target; a search, a registration or a normal estimation in between takes the buffers
    that preparation filled, and the registration must prepare the table again."""
    tally = cs.Tally("local map")
    for foreign in ("nearest_5000_5000", "normals_3000", "align_culled_5000", "k_nearest_20"):
        with cs.fresh() as ctx:
            gen = cs.THREADS["local_map"].run(ctx, env)
            try:
                for k in range(len(exp[1]["local_map"])):
                    tally.step(gen, "local_map", k, exp[1], (foreign, k))
                    tally.op(ctx, env, foreign, exp[0], (foreign, k))
            finally:
                gen.close()
    done(tally, "local map between foreign searches")


# ------------------------------------------------------------------ 4. the same pointer, new rows
def _dev(a):
    t = torch.from_numpy(np.array(a)).cuda()
    torch.cuda.synchronize()
    return t


def _refill(t, a):
    t.copy_(torch.from_numpy(np.array(a)))
    torch.cuda.synchronize()


def _same_pointer(env, call, first, second):
    """call(ctx, tensors) -> digest.  A fresh context on fresh tensors of `second` gives the digest that a used context
    must give on the tensors of `first` once they have been overwritten with `second`."""
    with cs.fresh() as ctx:
        want = call(ctx, [_dev(a) for a in second])
    with cs.fresh() as ctx:
        tensors = [_dev(a) for a in first]
        addresses = [t.data_ptr() for t in tensors]
        call(ctx, tensors)
        for t, a in zip(tensors, second):
            _refill(t, a)
        assert [t.data_ptr() for t in tensors] == addresses
        got = call(ctx, tensors)
    return got == want


def test_the_same_pointer_with_new_rows(env):
    I = env.I
    cfg = capi.Context.make_config(max_iterations=3, tolerance=0.0, min_error=0.0)
    results = {}

    def align(ctx, t):
        res, hist = ctx.align_device(t[0].data_ptr(), t[0].shape[0], t[1].data_ptr(), t[1].shape[0], cfg)
        return cs._reg_out(ctx, t[0].shape[0], res, hist, []).digest
    results["align_device small"] = _same_pointer(env, align, (I["rc_s1001"], I["rc_t1500"]), (I["rc_s3000"][1000:2001], I["rc_t4500"][:1500]))
    results["align_device culled"] = _same_pointer(env, align, (I["u_s5000b"], I["u_t24577"]),
                                                   (I["u_s5000b"][::-1], I["u_t24577"][::-1] + np.array([0.25, -0.5, 0.125])))

    def voxel(ctx, t):
        out = torch.full_like(t[0], 7.0)
        torch.cuda.synchronize()
        n = ctx.voxel_downsample_device(t[0].data_ptr(), t[0].shape[0], 1.0, out.data_ptr(), t[0].shape[0])
        torch.cuda.synchronize()
        return cs.dig(n, out[:n].cpu().numpy())
    results["voxel_downsample_device"] = _same_pointer(env, voxel, (I["vox_shared"],), (I["vox_unique"],))

    def deskew(ctx, t):
        ctx.deskew_device(t[0].data_ptr(), t[1].data_ptr(), t[0].shape[0], cs._deskew_cfg(env, capi.DESKEW_TIMES), t[0].data_ptr())
        torch.cuda.synchronize()
        return cs.dig(t[0].cpu().numpy())
    results["deskew_device in place"] = _same_pointer(env, deskew, (I["dk_xyz"], I["dk_tau"]), (I["dk_xyz"][::-1], I["dk_tau"][::-1]))

    def occupancy(ctx, t):
        ctx.occupancy_clear()
        n = ctx.occupancy_update_device(t[0].data_ptr(), t[0].shape[0], I["p16_0"][:3, 3])
        return cs.dig(n, ctx.occupancy_cells())
    results["occupancy_update_device"] = _same_pointer(env, occupancy, (I["world16_0"][:2700],), (I["world16_1"][:2700],))

    maps = {}

    def local_map(ctx, t):
        if ctx not in maps:
            maps[ctx] = LocalMap(ctx, LocalMapConfig(voxel_size=0.5, max_range=10.0, capacity=1 << 15))
        lm = maps[ctx]
        lm.clear()
        info = lm.add_device(t[0].data_ptr(), t[0].shape[0], I["p16_1"])
        res, hist = lm.register_device(t[1].data_ptr(), t[1].shape[0], capi.Context.make_config(max_iterations=5, initial_transform=I["p16_1"]))
        pts, keys = lm.points()
        return cs.dig(info, res, hist, pts, keys, cs._normal_matrix_parts(ctx))
    results["LocalMap add_device / register_device"] = _same_pointer(
        env, local_map, (I["f16_1"][:2700], I["f16_2"][:2700]), (I["f16_1"][:2700] + np.array([0.0, 0.3, 0.0]), I["f16_2"][5:2705]))

    def global_map(ctx, t):
        gm = GlobalMap(ctx)
        try:
            gm.add_frame_device(t[0].data_ptr(), t[0].shape[0])
            return cs.dig(gm.world([I["p16_2"]]))
        finally:
            gm.close()
    results["GlobalMap add_frame_device"] = _same_pointer(env, global_map, (I["f16_2"][:2700],), (I["f16_3"][:2700],))

    print("the same pointer with new rows: %d (call, contents) pairs" % len(results))
    assert all(results.values()), results


def test_local_map_emptied_and_refilled(env):
    """An add that leaves the table empty prepares no target; the table that the next add builds at the same address
    registers as a new map's does (lmap_forget_target)."""
    I = env.I
    far = np.eye(4)
    far[0, 3] = 1000.0
    cfg = capi.Context.make_config(max_iterations=5, initial_transform=I["p16_3"])

    def tail(lm, ctx):
        info = lm.add(I["f16_3"], I["p16_3"])
        res, hist = lm.register(I["f16_4"], cfg)
        return cs.dig(info, res, hist, lm.points()[0], cs._normal_matrix_parts(ctx))

    with cs.fresh() as ctx:
        want = tail(LocalMap(ctx, LocalMapConfig(voxel_size=0.5, max_range=10.0, capacity=1 << 15)), ctx)
    with cs.fresh() as ctx:
        lm = LocalMap(ctx, LocalMapConfig(voxel_size=0.5, max_range=10.0, capacity=1 << 15))
        lm.add(I["f16_0"], I["p16_0"])
        lm.add(I["f16_1"], I["p16_1"])
        emptied = lm.add(I["f16_0"][:10] + 500.0, far)              # every resident out of range, every new row too
        assert emptied.rows == 0 and emptied.evicted > 0
        assert tail(lm, ctx) == want


# ------------------------------------------------------------------ 5. engines and profiling
def _cross_engine(name, facts, auto_facts):
    """what engines agree on: iteration counts, convergence, and the matched indices where both kept them"""
    if facts is None:
        return True
    for key, v in facts.items():
        w = auto_facts[key]
        if v is None or w is None:
            continue
        if not (np.array_equal(v, w) if isinstance(v, np.ndarray) else v == w):
            return False
    return True


@pytest.mark.parametrize("config", list(CONFIGS))
def test_engines_shuffled_threads(env, exp, config):
    search, profile = CONFIGS[config]
    _, exp_threads = expected_for(env, search, profile)
    assert {t: len(v) for t, v in exp_threads.items()} == {t: len(v) for t, v in exp[1].items()}
    tally = cs.Tally(config)
    with cs.fresh(search, profile) as ctx:
        cs.run_plan(ctx, env, cs.shuffle_plan(SEEDS[0], exp_threads), exp_threads, tally, (config, SEEDS[0]))
    done(tally, "all threads on %s, seed %d" % (config, SEEDS[0]))


@pytest.mark.parametrize("config", list(CONFIGS))
def test_engines_shrink_and_grow(env, exp, config):
    search, profile = CONFIGS[config]
    exp_ops, _ = expected_for(env, search, profile)
    differ = [n for n in cs.OPS if not _cross_engine(n, exp_ops[n].facts, exp[0][n].facts)]
    assert not differ, (config, differ)                          # against the AUTO context: iterations and matches
    tally = cs.Tally(config)
    with cs.fresh(search, profile) as ctx:
        shrink_and_grow(ctx, env, exp_ops, tally)
    done(tally, "shrink and grow on %s" % config)


# ------------------------------------------------------------------ 6. two contexts, two host threads
def test_two_contexts_two_host_threads(env, exp):
    exp_ops, exp_threads = exp
    tallies, errors = [cs.Tally("host thread 0"), cs.Tally("host thread 1")], []

    def body(i):
        try:
            with cs.fresh() as ctx:
                cs.run_plan(ctx, env, cs.shuffle_plan(SEEDS[1 + i], exp_threads), exp_threads, tallies[i], ("host thread", i))
                for name in cs.size_orders()[2]:
                    tallies[i].op(ctx, env, name, exp_ops, ("host thread", i))
        except BaseException as e:  # noqa: BLE001 -- reported by the test's own thread
            errors.append((i, repr(e)))

    workers = [threading.Thread(target=body, args=(i,)) for i in range(2)]
    for w in workers:
        w.start()
    for w in workers:
        w.join()
    assert not errors, errors
    tallies[0].merge(tallies[1])
    done(tallies[0], "two contexts, two host threads (seeds %d, %d)" % (SEEDS[1], SEEDS[2]))


# ------------------------------------------------------------------ 7. refused calls change nothing
@pytest.mark.parametrize("name", ["stream_a", "local_map"])
def test_refused_calls_change_nothing(env, exp, name):
    """between every two steps, one call of each family that an argument check refuses"""
    tally = cs.Tally(name)
    with cs.fresh() as ctx:
        gen = cs.THREADS[name].run(ctx, env)
        try:
            for k in range(len(exp[1][name])):
                tally.step(gen, name, k, exp[1], ("refused", k))
                codes = cs.refused_calls(ctx, env)
                assert len(codes) == 5 and all(c in (capi.ERR_ARG, capi.ERR_NULL) for c in codes), codes
        finally:
            gen.close()
    done(tally, "%s between refused calls" % name)
