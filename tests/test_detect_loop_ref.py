"""CPU tests of the loop-detection model (tests/detect_loop_ref.py): LoopClosing::detectLoop's consistency groups against tables
worked out by hand -- outcome, the groups with their counts, the enough list per call -- on the worlds of
tests/detect_loop_inputs.py, and the conditions that make the worlds mean what their names say."""
import numpy as np
import pytest

import detect_loop_inputs as di
import detect_loop_ref as dr


@pytest.fixture(scope="module")
def cases():
    return di.hand_cases()


def test_the_hand_cases_are_all_there(cases):
    assert sorted(cases) == sorted(di.HAND_CASES)


@pytest.mark.parametrize("name", di.HAND_CASES)
def test_hand_tables(cases, name):
    c = cases[name]
    m, got = di.run_model(c)
    want = [(o, [(sorted(g), n) for g, n in groups], list(enough)) for o, groups, enough in c["want"]]
    assert got == want


def test_the_gate_is_at_last_plus_10(cases):
    c = cases["gate_at_last_plus_9_and_10"]
    m = di.build_model(c["world"], c["D"], c["G"])
    assert m.detect_loop(12, 3) == dr.GATED and m.record["locked"] == 0 and m.groups_as_sets() == []
    assert m.detect_loop(13, 3) == dr.NOT_CONSISTENT and m.record["n_candidates"] == 1
    assert m.detect_loop(13, 4) == dr.GATED and m.groups_as_sets() == [(di.G123, 0)]      # (the groups are not touched)


def test_counts_run_0_1_2_and_the_fourth_call_detects(cases):
    m, got = di.run_model(cases["one_candidate_four_calls"])
    assert [g[1][0][1] for g in got] == [0, 1, 2, 3] and [g[0] for g in got] == [dr.NOT_CONSISTENT] * 3 + [dr.DETECTED]
    assert m.cull.locked[15] == 1 and [m.cull.locked[k] for k in (12, 13, 14)] == [0, 0, 0]   # (:59 stays on a detection only)


def test_the_neighbour_case_is_through_a_neighbour_only(cases):
    c = cases["consistent_through_a_neighbour_only"]
    m = di.build_model(c["world"], c["D"], c["G"])
    m.detect_loop(12, 0)
    prev = set(kf.id_ for kf in m.prevConsistentGroups_[0][0])
    m.detect_loop(13, 0)
    assert m.candidates == [4] and 4 not in prev and prev & set(di.G345) == {3}


def test_two_pushes_and_one_push(cases):
    m, got = di.run_model(cases["one_candidate_two_previous_groups"])
    assert m.candidates == [4] and len(got[1][1]) == 2 and m.record["groups_before"] == 2
    m, got = di.run_model(cases["two_candidates_one_previous_group"])
    assert m.candidates == [4, 8] and len(got[1][1]) == 1 and m.record["groups_before"] == 1


def test_a_flagged_group_still_counts_towards_enough(cases):
    m, got = di.run_model(cases["consistent_only_with_flagged_groups"])
    assert m.candidates == [2, 8] and got[-1] == (dr.DETECTED, [(di.G123, 3)], [2, 8])


def test_bad_and_erased_members_stay(cases):
    c = cases["bad_and_erased_members"]
    m = di.build_model(c["world"], c["D"], c["G"])
    for s in c["script"][:3]:
        di.model_step(m, s)
    assert m.cull.erased[3] == 1 and m.cull.store[1]["bad"] and m.groups_as_sets() == [(di.G123, 0)]    # the stored group keeps both
    di.model_step(m, c["script"][3])
    assert m.groups_as_sets() == [([1, 2], 1)]      # the bad key-frame 1 is a member of the new group; the erased one has left W


def test_a_bad_neighbour_raises_min_score_and_drops_a_candidate(cases):
    c = cases["conn_skips_a_bad_neighbour"]
    m = di.build_model(c["world"], c["D"], c["G"])
    assert m.cull.conn.ordered[12] == [11, 10]
    m.detect_loop(12, 0)
    first = m.result()
    di.model_step(m, ("bad", 10))
    m.detect_loop(12, 0)
    second = m.result()
    ms = lambda r: float(np.int32(r["min_score_bits"]).view(np.float32))
    assert (first["n_conn"], first["candidates"], ms(first)) == (2, [2, 4], 0.25)
    assert (second["n_conn"], second["candidates"]) == (1, [4]) and abs(ms(second) - 0.9) < 1e-6
    assert first["n_excl"] == second["n_excl"] == 3


def test_capacities_overflow_and_clear():
    w = di.overflow_world()
    m = di.build_model(w, 1, 8)
    assert m.detect_loop(12, 0) == dr.OVERFLOW and m.record["n_candidates"] == 2 and m.sticky == dr.STICKY_DETECT_CAPACITY
    assert m.groups_as_sets() == [] and m.cull.locked[12] == 0
    m = di.build_model(w, 2, 2)
    assert m.detect_loop(12, 0) == dr.NOT_CONSISTENT and len(m.prevConsistentGroups_) == 2
    assert m.detect_loop(13, 0) == dr.OVERFLOW and m.candidates == [4, 9] and m.groups_as_sets() == [] and m.sticky == dr.STICKY_DETECT_CAPACITY
    m = di.build_model(w, 2, 3)
    m.detect_loop(12, 0)
    assert m.detect_loop(13, 0) == dr.NOT_CONSISTENT and [n for _, n in m.groups_as_sets()] == [1, 1, 0]


def test_the_lock_rules():
    w = di.standard_world({k: "A" for k in di.CURRENTS})
    m = di.build_model(w, 4, 8)
    m.add_loop_edge(12, 5)
    assert m.detect_loop(12, 0) == dr.NOT_CONSISTENT and m.record["locked"] == 1      # a loop edge keeps the lock
    m.cull.pending[13] = 1
    assert m.detect_loop(13, 0) == dr.NOT_CONSISTENT and (m.record["locked"], m.record["pending"]) == (0, 1) and not m.cull.erased[13]
    m.cull.erase_keyframe(14)
    assert m.detect_loop(14, 0) == dr.NONE and m.sticky == dr.STICKY_INVALID and m.record["groups_after"] == 1
    # computeSim3's releases
    m.lock_candidates([2, 4, 5])
    m.cull.pending[4] = 1
    assert m.release_loop_locks(dr.UNDECIDED, [2, 4, 5], 15) == (0, [])
    assert m.release_loop_locks(dr.ACCEPTED, [2, 4, 5], 15, match=2) == (1, [4]) and [m.cull.locked[k] for k in (2, 4, 5)] == [1, 0, 1]
    m.cull.locked[15] = 1
    assert m.release_loop_locks(dr.NO_MATCH, [2, 4, 5], 15) == (2, []) and [m.cull.locked[k] for k in (2, 5, 15)] == [0, 1, 0]


def test_the_big_world_spans_three_words():
    w = di.big_world()
    m = di.build_model(w, 4, 8)
    assert m.detect_loop(100, 0) == dr.NOT_CONSISTENT and m.candidates == [64, 129]
    counts, members = m.groups(130)
    assert counts == [0, 0] and members.shape == (2, 130) and set(np.flatnonzero(members[0])) == {63, 64, 127, 128, 129}
    assert set(np.flatnonzero(members[1])) == {0, 64, 128, 129}
    outcomes = [m.detect_loop(k, 0) for k in (101, 102, 103)]
    assert outcomes == [dr.NOT_CONSISTENT] * 2 + [dr.DETECTED] and m.result()["enough"] == [64, 129]
    assert m.groups_as_sets() == [([63, 64, 127, 128, 129], 3)] * 2
