"""The pinned sensitive registrations of scripts/fuzz_stopping.py (PINNED_SENSITIVE) through AUTO, the all-pairs and the
culled engine with the caller's settings (50, 1e-6, 1e-9), each run judged by `classify` against the oracle's two legs
(sums in index order and in reversed row order).  No engine may be a MISMATCH; where a run is SENSITIVE it is so in the
way the table records for its seed.  At the five unsettled seeds the outcome is the oracle's (50, not converged, 51
history entries) and the caller's gate discards the result; at 320287, where the oracle's own two legs leave the loop
at 28 and at 50, the three engines take the same one.  tests/test_stopping_rule.py holds the generator and the oracle
side of these seeds on the CPU."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


@pytest.fixture(scope="module")
def engines():
    from lidar_slam_from_scratch_amd import build, capi
    build.build_library()
    ctxs = {"auto": capi.Context(device=0, search=capi.SEARCH_AUTO), "all pairs": capi.Context(device=0, search=capi.SEARCH_MFMA_BF16),
            "culled": capi.Context(device=0, search=capi.SEARCH_MFMA_PRUNED)}
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.mark.parametrize("seed", [320287, 411087, 321727, 321759, 91000, 320008])
def test_pinned_seed_through_every_engine(oracle, engines, seed):
    import fuzz_stopping as fs
    kind = fs.PINNED_SENSITIVE[seed]
    src, tgt, what = fs.make_case(seed)
    assert src.shape[0] <= 10500
    index, rev = fs.oracle_legs(src, tgt)
    print("seed %d (%s, %d -> %d rows, pinned as %s): index leg %s final_error %r, reversed leg %s final_error %r"
          % (seed, what, src.shape[0], tgt.shape[0], kind, fs.outcome(index), index.final_error, fs.outcome(rev), rev.final_error))
    runs, verdicts = {}, {}
    for name, ctx in engines.items():
        res, hist = ctx.align(src, tgt, fs.caller_config())
        runs[name] = fs.run_of_engine(res, hist)
        verdicts[name] = fs.classify(runs[name], index, rev)
        print("  engine %s: %s final_error %r -> %s: %s" % ((name, fs.outcome(runs[name]), runs[name].final_error) + verdicts[name]))
    for name, (verdict, reason) in verdicts.items():
        assert verdict != fs.MISMATCH, (name, reason)
        assert verdict == fs.OK or reason.startswith(kind), (name, verdict, reason)
        if kind == fs.UNSETTLED:
            assert fs.outcome(runs[name]) == fs.outcome(index) == (fs.MAX_IT, False, fs.MAX_IT + 1), (name, fs.outcome(runs[name]))
            assert fs.discarded(runs[name]) and fs.discarded(index)
        else:
            assert fs.outcome(runs[name]) in (fs.outcome(index), fs.outcome(rev)), (name, fs.outcome(runs[name]))
    if kind == fs.COUNT_MOVES:
        assert fs.outcome(index) != fs.outcome(rev)
        assert len({fs.outcome(r) for r in runs.values()}) == 1, {n: fs.outcome(r) for n, r in runs.items()}
