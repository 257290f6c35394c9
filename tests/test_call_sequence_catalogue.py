"""The catalogue of scripts/call_sequences.py, checked without a GPU: its inputs are reproducible, its registration
shapes reach every form of a call that csrc/loop_plan.h distinguishes on a single GPU, and every entry point of the
Python binding is named by an operation or a thread -- a new entry point fails this test until it joins the catalogue,
which is the point of the test."""
import inspect
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import call_sequences as cs  # noqa: E402

# a context's methods the catalogue leaves to others: the communicator (tests/test_gpu_dist.py), the config makers, and
# what is documented to accumulate
LEFT_OUT = ("comm_", "make_", "reset_profile", "get_profile", "nn_")


def test_inputs_are_reproducible():
    a, b = cs.build_inputs(), cs.build_inputs()
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
    assert cs.inputs_digest(a) == cs.inputs_digest(b) == cs.inputs_digest(cs.inputs())


def test_registration_shapes_reach_every_plan(tmp_path):
    exe = cs.build_plan_printer(tmp_path)
    seen = {}
    for name, op in cs.OPS.items():
        if op.reg is None:
            continue
        path, run = cs.planned(exe, op.reg)
        seen.setdefault((path, op.reg["rule"]), []).append(name)
        # the plan's own fields agree with the path's name
        small, fused, pruned = bool(run[6]), bool(run[7]), bool(run[8])
        assert small == (path == "small") and pruned == (path == "culled" and op.reg["rule"] == "none"), (name, path, run)
        assert fused == (path != "exact" and op.reg["rule"] == "none"), (name, path, run)
    want = {(p, r) for p in ("exact", "small", "general", "culled") for r in ("none", "gate", "robust")}
    assert set(seen) == want, sorted(want - set(seen))
    # one split and three, the last one ragged, under the small-cloud kernel; a run to tolerance on every path
    per_split = cs.split_targets()
    splits = {-(-cs.OPS[n].reg["m"] // per_split) for n in seen[("small", "none")]}
    assert {1, 3} <= splits and any(cs.OPS[n].reg["m"] % per_split for n in seen[("small", "none")])
    for path in ("exact", "small", "general", "culled"):
        assert any(n.endswith("_to_tolerance") for n in seen[(path, "none")]), path


def _public(cls):
    return {n for n, f in inspect.getmembers(cls, predicate=inspect.isfunction) if not n.startswith("_")}


def test_every_entry_point_is_in_the_catalogue():
    from lidar_slam_from_scratch_amd import capi
    from lidar_slam_from_scratch_amd.global_map import GlobalMap
    from lidar_slam_from_scratch_amd.local_map import LocalMap
    from lidar_slam_from_scratch_amd.loop_closure import StoreLoopClosureDetector
    from lidar_slam_from_scratch_amd.pose_graph import PoseGraph
    named = set()
    helpers = "".join(inspect.getsource(f) for f in (cs._reg_out, cs._batch_out, cs._normal_matrix_parts, cs._push_digest, cs._stream_off))
    for entry in list(cs.OPS.values()) + list(cs.THREADS.values()):
        source = inspect.getsource(entry.run) + helpers
        for name in entry.names:
            assert "." + name + "(" in source or '"%s"' % name in source, (entry.name, name)   # it does call what it names
        named |= set(entry.names)
    context = {n for n in _public(capi.Context) if not n.startswith(LEFT_OUT)}
    context.discard("close")               # (every fresh context of the catalogue's harness is closed: call_sequences.fresh)
    assert "fresh" in dir(cs) and ".close()" in inspect.getsource(cs.fresh)
    assert not context - named, sorted(context - named)
    for cls in (LocalMap, GlobalMap, StoreLoopClosureDetector, PoseGraph):
        # (the thread of each object names its methods; what another class names by the same word does not count)
        thread = {LocalMap: "local_map", GlobalMap: "global_map", StoreLoopClosureDetector: "loop_store", PoseGraph: "pose_graph"}[cls]
        own = set(cs.THREADS[thread].names)
        if cls is GlobalMap:
            own |= set(cs.THREADS["stream_c"].names)      # (add_stream_frame needs the stream)
        assert not _public(cls) - own, (cls.__name__, sorted(_public(cls) - own))


def test_the_shuffle_keeps_each_thread_in_order_and_claims_apart():
    steps = {t: [None] * (3 + i) for i, t in enumerate(cs.THREADS)}
    for seed in range(5):
        plan = cs.shuffle_plan(seed, steps)
        assert sorted(plan) == sorted((t, k) for t in steps for k in range(len(steps[t])))
        for t in steps:
            assert [k for name, k in plan if name == t] == list(range(len(steps[t])))
        # two threads with a common claim never overlap
        live = set()
        for t, k in plan:
            if k == 0:
                assert not any(cs.THREADS[t].claims & cs.THREADS[o].claims for o in live), (seed, t, live)
                live.add(t)
            if k == len(steps[t]) - 1:
                live.discard(t)
    assert cs.shuffle_plan(1, steps) != cs.shuffle_plan(2, steps) and cs.shuffle_plan(3, steps) == cs.shuffle_plan(3, steps)
    down, up, mixed = cs.size_orders()
    assert sorted(down) == sorted(up) == sorted(mixed) and mixed[0] == down[0] and mixed[1] == up[0]
    assert all(cs.OPS[n].kind in ("registration", "primitive") for n in down)


if __name__ == "__main__":
    sys.exit(pytest.main([__file__, "-q"]))
