"""The decision rule of scripts/fuzz_stopping.py on the CPU: `classify` on hand-made results, the pins and caps through
`run_trials` (main's bookkeeping) with a stubbed trial, `check_case` on stubbed engines and oracle, and the pinned seeds'
generator and oracle side (description, row counts, the two legs' outcomes).  If the generator or the oracle drifts, the
pins of PINNED_SENSITIVE mean nothing; if the rule drifts, the GPU fuzz can be silenced by its own input again."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import fuzz_stopping as fs  # noqa: E402
from lidar_slam_from_scratch_amd import synth  # noqa: E402

OK, SENSITIVE, MISMATCH = fs.OK, fs.SENSITIVE, fs.MISMATCH


def pose(tx=0.0, rz=0.0):
    return synth.make_transform((0.0, 0.0, rz), (tx, 0.0, 0.0))


def run(n, converged, first, last, T=None, final_error=None):
    """a Run of n iterations: a history of n + 1 entries falling from `first` to `last`, final_error its last entry"""
    h = np.linspace(first, last, n + 1)
    return fs.Run(n, converged, h, pose() if T is None else T, float(h[-1]) if final_error is None else final_error)


def moved(r, tx=0.0, rz=0.0, history=0.0, final_error=0.0):
    """`r` with its pose moved by tx metres / rz radians, every history entry by `history`, final_error by `final_error`"""
    T = pose(tx, rz) @ r.pose
    return fs.Run(r.num_iterations, r.converged, r.history + history, T, r.final_error + final_error)


# seed 320287's shape: the index leg converges after 28 iterations and the caller accepts it (final_error <= 1), the
# reversed leg runs out of its 50 and is discarded, the two poses far apart
LEG_28 = run(28, True, 1.2, 0.85)
LEG_50 = run(50, False, 1.2, 2.04, T=pose(tx=6.6e3, rz=0.68))


def parent_rule(engine, leg_index, leg_reversed):
    """What the commit before this rule made of a run whose count differs from the index leg's above the margin floor
    (check_case's first branch and oracle_own_spread): excused as soon as the ORACLE's two counts differ, whatever the
    engine returned."""
    same = fs.outcome(engine) == fs.outcome(leg_index)
    assert not same
    own_count_moves = leg_index.num_iterations != leg_reversed.num_iterations
    return SENSITIVE if own_count_moves else MISMATCH


def test_engine_equal_to_the_index_leg_is_ok():
    assert fs.classify(LEG_28, LEG_28, None)[0] == OK
    assert fs.classify(LEG_28, LEG_28, LEG_50)[0] == OK
    assert fs.classify(moved(LEG_28, tx=5e-5, rz=5e-5, history=5e-10), LEG_28)[0] == OK
    unsettled = run(50, False, 1.2, 0.58)
    assert fs.classify(moved(unsettled, tx=5e-5, history=-5e-10), unsettled, None)[0] == OK      # inside the tolerances: no excuse needed


def test_engine_equal_to_the_reversed_leg_where_the_legs_differ_is_sensitive():
    verdict, reason = fs.classify(moved(LEG_50, tx=3.0, history=1e-3), LEG_28, LEG_50)      # both discarded: the pose is not compared
    assert verdict == SENSITIVE and reason.startswith(fs.COUNT_MOVES)
    # the other way round: the index leg unsettled, the reversed leg converged and accepted, the engine on the reversed leg
    verdict, reason = fs.classify(moved(LEG_28, tx=5e-5, final_error=5e-10), LEG_50, LEG_28)
    assert verdict == SENSITIVE and reason.startswith(fs.COUNT_MOVES)


@pytest.mark.parametrize("count,converged", [(37, True), (37, False), (3, True), (49, False), (50, True), (28, False)])
def test_a_count_that_is_neither_leg_is_a_mismatch(count, converged):
    """The regression this rule exists for: legs 28 | 50 (seed 320287) and an engine returning 37, or 3.  The parent
    commit's check_case reran the oracle reversed, saw ITS count move (oracle_own_spread -> inf), printed SENSITIVE and
    `continue`d without looking at the engine's count: `parent_rule` above restates that branch and excuses every case
    here.  (The parent's own check_case, given stub engines returning 37 and 3 at seed 320287 with the real oracle, printed
    "SENSITIVE seed 320287 (lidar f124+2 b16 az900 v0.3) engine thirty-seven: iterations 37 vs 28 -- the oracle's own count
    moves under reversed summation", the same for 3, and returned 0 mismatches; this one returns 2.)  Under the rule the
    outcome has to be one of the two legs' -- flag and history length included."""
    engine = run(count, converged, 1.2, 0.9)
    assert parent_rule(engine, LEG_28, LEG_50) == SENSITIVE
    verdict, reason = fs.classify(engine, LEG_28, LEG_50)
    assert verdict == MISMATCH, reason
    assert fs.classify(engine, LEG_50, LEG_28)[0] == MISMATCH


def test_a_differing_count_where_the_oracle_does_not_move_is_a_mismatch():
    assert fs.classify(LEG_50, LEG_28, moved(LEG_28, tx=1e-6))[0] == MISMATCH
    short = fs.Run(28, True, LEG_28.history[:-1], LEG_28.pose, LEG_28.final_error)      # equal count and flag, a history one entry short
    assert fs.classify(short, LEG_28, LEG_28)[0] == MISMATCH


def test_the_reversed_legs_outcome_with_another_caller_view_is_a_mismatch():
    """The engine leaves the loop where the reversed leg does and the caller ACCEPTS the result: then the pose the caller
    gets has to be that leg's."""
    assert fs.classify(moved(LEG_28, tx=1e-3), LEG_50, LEG_28)[0] == MISMATCH
    assert fs.classify(moved(LEG_28, rz=1e-3), LEG_50, LEG_28)[0] == MISMATCH
    assert fs.classify(moved(LEG_28, final_error=1e-8), LEG_50, LEG_28)[0] == MISMATCH
    # accepted on one side, discarded on the other: final_error 0.85 against 1.5 across the gate's 1.0
    assert not fs.discarded(LEG_28) and fs.discarded(moved(LEG_28, final_error=0.65))
    assert fs.classify(moved(LEG_28, final_error=0.65), LEG_50, LEG_28)[0] == MISMATCH
    assert fs.classify(LEG_28, LEG_50, moved(LEG_28, final_error=0.65))[0] == MISMATCH
    T, e = fs.caller_view(LEG_50)
    assert np.array_equal(T, np.eye(4)) and e == LEG_50.final_error
    assert np.array_equal(fs.caller_view(LEG_28)[0], LEG_28.pose)


def test_a_settled_loop_has_no_excuse():
    for other in (None, LEG_28, moved(LEG_28, tx=1.0, history=1e-3), LEG_50):
        assert fs.classify(moved(LEG_28, history=1e-8), LEG_28, other)[0] == MISMATCH
        assert fs.classify(moved(LEG_28, tx=2e-4), LEG_28, other)[0] == MISMATCH
        assert fs.classify(moved(LEG_28, rz=2e-4), LEG_28, other)[0] == MISMATCH
    h = LEG_28.history.copy()
    h[13] += 1e-8                                                                            # one entry in the middle
    assert fs.classify(fs.Run(28, True, h, LEG_28.pose, LEG_28.final_error), LEG_28)[0] == MISMATCH


UNSETTLED = run(50, False, 1.2, 1.58)
OWN = dict(tx=1e-3, rz=1e-3, history=1e-6, final_error=1e-6)       # what the oracle's own legs are apart in these cases


@pytest.mark.parametrize("part", ["tx", "rz", "history", "final_error", "all"])
def test_an_unsettled_loop_is_held_to_eight_times_the_oracles_own_spread(part):
    rev = moved(UNSETTLED, **OWN)
    seven = {k: 7 * v for k, v in OWN.items() if part in (k, "all")}
    nine = {k: 9 * v for k, v in OWN.items() if part in (k, "all")}
    verdict, reason = fs.classify(moved(UNSETTLED, **seven), UNSETTLED, rev)
    assert verdict == SENSITIVE and reason.startswith(fs.UNSETTLED), reason
    assert fs.classify(moved(UNSETTLED, **nine), UNSETTLED, rev)[0] == MISMATCH
    with pytest.raises(ValueError):
        fs.classify(moved(UNSETTLED, **seven), UNSETTLED, None)                               # it cannot be judged on one leg


def test_an_unsettled_loop_needs_the_same_outcome_on_both_legs_and_a_discarded_view():
    engine = moved(UNSETTLED, tx=2e-4)
    assert fs.classify(engine, UNSETTLED, moved(UNSETTLED, tx=1e-3))[0] == SENSITIVE
    assert fs.classify(engine, UNSETTLED, LEG_28)[0] == MISMATCH                              # the reversed leg left the loop elsewhere
    assert fs.classify(engine, UNSETTLED, moved(UNSETTLED, tx=1e-6))[0] == MISMATCH           # 200 times the own spread
    assert fs.classify(engine, UNSETTLED, UNSETTLED)[0] == MISMATCH                           # no spread at all: only the 1e-12 floor


def test_nan_is_a_mismatch():
    T = pose()
    T[0, 3] = np.nan
    R = pose()
    R[:3, :3] = np.nan
    h = LEG_28.history.copy()
    h[5] = np.nan
    for leg, rev in ((LEG_28, LEG_50), (UNSETTLED, moved(UNSETTLED, **OWN))):
        for bad in (fs.Run(leg.num_iterations, leg.converged, leg.history, T, leg.final_error),
                    fs.Run(leg.num_iterations, leg.converged, leg.history, R, leg.final_error),
                    fs.Run(leg.num_iterations, leg.converged, np.full_like(leg.history, np.nan), leg.pose, leg.final_error),
                    fs.Run(leg.num_iterations, leg.converged, leg.history, leg.pose, float("nan")) if not leg.converged else
                    fs.Run(28, True, h, leg.pose, leg.final_error)):
            verdict, reason = fs.classify(bad, leg, rev)
            assert verdict == MISMATCH, reason
    # accepted by the gate on the reversed leg's outcome, with a NaN pose
    assert fs.classify(fs.Run(28, True, LEG_28.history, T, LEG_28.final_error), LEG_50, LEG_28)[0] == MISMATCH


# ---------------------------------------------------------------------------------------------------------------------
# the pins and the caps, through main's bookkeeping


def stub_trial(sensitive=None, under=(), mismatching=()):
    """a check_case that runs nothing: the seeds of `sensitive` (seed -> kind) give one SENSITIVE engine run each"""
    sensitive = sensitive or {}

    def check(seed, ctxs, cfg, stats):
        stats["trials"] += 1
        if seed in under:
            stats["under"] += 1
        else:
            stats["decided"] += 1
        bad = 0
        for _ in ctxs:
            if seed in sensitive:
                bad += fs.record(stats, seed, SENSITIVE, sensitive[seed] + ": made up")[0]
            elif seed in mismatching:
                bad += fs.record(stats, seed, MISMATCH, "made up")[0]
            else:
                bad += fs.record(stats, seed, OK, "")[0]
        return bad
    return check


ENGINES = {"auto": None, "all pairs": None, "culled": None}


def test_one_sensitive_seed_in_forty_trials_fails(capsys):
    seeds = [411087] + list(range(9001, 9040))
    rc, bad, stats = fs.run_trials(seeds, ENGINES, None, stub_trial({411087: fs.UNSETTLED}))
    assert rc == 1 and bad == 0 and stats["sensitive"] == 3 and stats["sensitive_seeds"] == {411087} and not stats["unpinned"]
    assert "more than trials // 100 = 0" in capsys.readouterr().out
    assert fs.run_trials(range(9000, 9040), ENGINES, None, stub_trial())[0] == 0


def test_an_unpinned_sensitive_seed_fails_even_under_the_cap(capsys):
    seeds = list(range(320000, 320400))
    assert fs.run_trials(seeds, ENGINES, None, stub_trial({320287: fs.COUNT_MOVES, 320008: fs.UNSETTLED}))[0] == 0
    rc, bad, stats = fs.run_trials(seeds, ENGINES, None, stub_trial({320100: fs.UNSETTLED}))
    assert rc == 1 and bad == 0 and stats["unpinned"] == {320100}
    out = capsys.readouterr().out
    assert "320100" in out.splitlines()[-1] and "1 of them unpinned" in out.splitlines()[-1]     # the summary line carries the counts
    # pinned, but as the other kind: as unexamined as a new seed
    rc, _, stats = fs.run_trials(seeds, ENGINES, None, stub_trial({320287: fs.UNSETTLED}))
    assert rc == 1 and stats["unpinned"] == {320287}


def test_the_caps_and_mismatches_fail_the_run():
    pinned = dict(fs.PINNED_SENSITIVE)
    seeds = list(pinned) + list(range(1, 395))                                                    # 400 trials: the cap is 4
    assert len(seeds) == 400
    four = {s: pinned[s] for s in list(pinned)[:4]}
    five = {s: pinned[s] for s in list(pinned)[:5]}
    assert fs.run_trials(seeds, ENGINES, None, stub_trial(four))[0] == 0
    assert fs.run_trials(seeds, ENGINES, None, stub_trial(five))[0] == 1
    assert fs.run_trials(seeds, ENGINES, None, stub_trial(under={1, 2, 3, 4}))[0] == 0
    assert fs.run_trials(seeds, ENGINES, None, stub_trial(under={1, 2, 3, 4, 5}))[0] == 1
    rc, bad, _ = fs.run_trials(seeds, ENGINES, None, stub_trial(mismatching={7}))
    assert rc == 1 and bad == 3
    assert fs.run_trials(seeds[:399], ENGINES, None, stub_trial(four))[0] == 1                    # 399 // 100 = 3


def test_the_pin_table():
    assert fs.PINNED_SENSITIVE == {320287: fs.COUNT_MOVES, 411087: fs.UNSETTLED, 321727: fs.UNSETTLED, 321759: fs.UNSETTLED,
                                   91000: fs.UNSETTLED, 320008: fs.UNSETTLED}
    # fuzz_engines.py's exit code goes through the same function on its own stop_stats
    stats = fs.new_stats()
    stats["trials"] = 18
    assert fs.failures(stats) == []
    fs.record(stats, 20267, SENSITIVE, fs.COUNT_MOVES + ": made up")
    assert len(fs.failures(stats)) == 2                                                          # unpinned, and over the cap of 0
    src = open(os.path.join(ROOT, "scripts", "fuzz_engines.py")).read()
    assert "fuzz_stopping.new_stats()" in src and "fuzz_stopping.failures(stop_stats)" in src and "return 1 if bad or why else 0" in src


class FakeEngine:
    def __init__(self, r):
        self.r = r

    def align(self, src, tgt, cfg):
        res = types.SimpleNamespace(num_iterations=self.r.num_iterations, converged=int(self.r.converged),
                                    transformation=list(self.r.pose.reshape(16)), final_error=self.r.final_error)
        return res, self.r.history


def fake_oracle(monkeypatch, index, rev, calls):
    ref = types.SimpleNamespace(num_iterations=index.num_iterations, converged=index.converged, error_history=index.history,
                                transformation=index.pose, final_error=index.final_error)
    monkeypatch.setattr(fs, "make_case", lambda seed: (np.zeros((4, 3)), np.zeros((4, 3)), "made up"))
    monkeypatch.setattr(fs.orc, "icp_point_to_plane", lambda *a, **k: ref)

    def legs(src, tgt, which=("index", "reversed")):
        calls.append(which)
        return tuple({"index": index, "reversed": rev}[w] for w in which)
    monkeypatch.setattr(fs, "oracle_legs", legs)


def test_check_case_holds_every_engine_to_one_of_the_two_legs(monkeypatch, capsys):
    calls = []
    fake_oracle(monkeypatch, LEG_28, LEG_50, calls)
    ctxs = {"on the index leg": FakeEngine(LEG_28), "on the reversed leg": FakeEngine(moved(LEG_50, tx=2.0)),
            "neither": FakeEngine(run(37, True, 1.2, 0.9))}
    stats = fs.new_stats()
    assert fs.check_case(320287, ctxs, None, stats) == 1
    assert calls == [("reversed",)]                                                              # made once, and only when needed
    assert stats["sensitive"] == 1 and stats["sensitive_seeds"] == {320287} and not stats["unpinned"]
    out = capsys.readouterr().out
    assert "MISMATCH stopping seed 320287 (made up) engine neither" in out and "SENSITIVE seed 320287 (made up) engine on the reversed leg" in out
    # the same registration at a seed nobody has looked at
    stats = fs.new_stats()
    assert fs.check_case(5, {"on the reversed leg": FakeEngine(LEG_50)}, None, stats) == 0
    assert stats["unpinned"] == {5} and "UNPINNED SENSITIVE seed 5" in capsys.readouterr().out
    assert fs.failures(stats)
    # settled and equal: the reversed leg is never computed
    del calls[:]
    stats = fs.new_stats()
    assert fs.check_case(9000, {"a": FakeEngine(LEG_28), "b": FakeEngine(moved(LEG_28, tx=1e-6))}, None, stats) == 0
    assert calls == [] and stats["sensitive"] == 0 and stats["decided"] == 1 and not fs.failures(stats)


def test_check_case_counts_a_trial_under_the_margin_floor_and_does_not_hold_its_count(monkeypatch, capsys):
    h = LEG_28.history.copy()
    h[-2] = h[-3] - fs.TOL                   # the last stopping test the loop evaluated sits ON the tolerance: margin 0
    index = fs.Run(28, True, h, LEG_28.pose, LEG_28.final_error)
    fake_oracle(monkeypatch, index, index, [])
    stats = fs.new_stats()
    assert fs.check_case(1, {"a": FakeEngine(run(29, True, 1.2, 0.85)), "b": FakeEngine(moved(index, tx=1e-3))}, None, stats) == 1
    assert stats["under"] == 1 and stats["decided"] == 0                                         # the pose off by 1e-3 m IS held
    out = capsys.readouterr().out
    assert "UNDER MARGIN seed 1" in out and "NOT HELD seed 1 (made up) engine a" in out and "MISMATCH stopping seed 1 (made up) engine b" in out


# ---------------------------------------------------------------------------------------------------------------------
# the pinned seeds: the generator and the oracle side

# seed: (description, source rows, target rows, index leg's outcome, reversed leg's outcome,
#        the oracle's own spread between its legs (m, rad) as first recorded, or None where the counts differ)
PINNED = {
    320287: ("lidar f124+2 b16 az900 v0.3", 4755, 3358, (28, True, 29), (50, False, 51), None),
    411087: ("lidar f125+3 b16 az900 v0.5", 1863, 3174, (50, False, 51), (50, False, 51), (1.40e-4, 7.2e-5)),
    321727: ("lidar f124+1 b32 az1800 v0.3", 10467, 7233, (50, False, 51), (50, False, 51), (8.4e-11, 2.8e-12)),
    321759: ("lidar f124+1 b16 az450 v0.3", 3613, 2482, (50, False, 51), (50, False, 51), (1.2e-5, 4.4e-7)),
    91000: ("lidar f123+2 b16 az900 v0.8", 2061, 1536, (50, False, 51), (50, False, 51), (2.5e-13, 8e-15)),
    320008: ("lidar f122+3 b16 az900 v0.5", 3174, 2514, (50, False, 51), (50, False, 51), (1.8e11, 1.66)),
}


@pytest.mark.parametrize("seed", sorted(PINNED))
def test_pinned_seed_generator_and_oracle_legs(oracle, seed):
    what, n_src, n_tgt, want_index, want_reversed, own = PINNED[seed]
    src, tgt, desc = fs.make_case(seed)
    assert desc == what and (src.shape, tgt.shape) == ((n_src, 3), (n_tgt, 3))
    assert n_src <= 10500
    index, rev = fs.oracle_legs(src, tgt)
    ref = fs.run_of_oracle(oracle.icp_point_to_plane(src, tgt, fs.MAX_IT, fs.TOL, fs.MIN_ERR, nthreads=min(16, os.cpu_count() or 1)))
    print("seed %d (%s): index %s final_error %r, reversed %s final_error %r, legs %s apart"
          % (seed, what, fs.outcome(index), index.final_error, fs.outcome(rev), rev.final_error, fs.deltas(index, rev)[:2]))
    # check_case takes the oracle's own loop for the index leg: the restatement has to BE that loop
    assert fs.outcome(ref) == fs.outcome(index) and np.array_equal(ref.history, index.history) and ref.final_error == index.final_error
    assert fs.classify(ref, index, rev)[0] == OK
    assert fs.outcome(index) == want_index and fs.outcome(rev) == want_reversed
    assert fs.oracle_margin(types.SimpleNamespace(error_history=index.history)) > fs.MARGIN_FLOOR
    kind = fs.PINNED_SENSITIVE[seed]
    assert kind == (fs.COUNT_MOVES if want_index != want_reversed else fs.UNSETTLED)
    dt, dr = fs.deltas(index, rev)[:2]
    if kind == fs.COUNT_MOVES:
        # the caller's gate accepts the index leg and discards the reversed one: the two legs differ at the caller's level
        assert not fs.discarded(index) and fs.discarded(rev)
        assert index.final_error == pytest.approx(0.8499543419918527, abs=1e-9)
        assert rev.final_error == pytest.approx(2.0442451523365426, abs=1e-9)
        assert fs.classify(rev, index, rev)[0] == SENSITIVE
    else:
        assert fs.discarded(index) and fs.discarded(rev)
        assert own[0] / 2 <= dt <= own[0] * 2 and own[1] / 2 <= dr <= own[1] * 2, (dt, dr)
        assert fs.classify(rev, index, rev)[0] in (OK, SENSITIVE)                                # (OK where the legs are within 1e-4 / 1e-9)
    if seed == 320008:
        assert dt > 1.0
