"""CPU tests of the loop-merge model tests/loop_merge_ref.py: against a pointer-object transcription of
src/loopClosing.cpp:439-455 with MapPoint::replaceMapPoint, addObservation, KeyFrame::addMapPoint and MapPoint::computeDescriptor
(src/mappoint.cpp:52-64, 118-190, 214-253; tests/test_fuse_ref.py's objects, which keep observedKFs_, mappoints_, badFlag_ and the
counters incrementally); hand tables; the two rules where the store deliberately differs from the pointer model; the conditions
on the inputs the device comparison (tests/test_gpu_loop_merge.py) relies on; and that the step matters to the chain.  The
model asserts the derivation of section 4s in every call, so every test below runs it."""
import numpy as np
import pytest

import fuse_inputs as fi
import loop_correct_inputs as ci
import loop_correct_ref as lr
import loop_merge_inputs as mi
import loop_merge_ref as mr
from test_fuse_ref import Pointers, _same_as_pointers


class MergePointers(Pointers):
    """test_fuse_ref.Pointers with the merge loop"""

    def mergeLoopMatches(self, keyframe_curr_, matchMapPoints_):              # loopClosing.cpp:439-455
        for i, mpLoop in enumerate(matchMapPoints_):
            if mpLoop is None:
                continue
            mpCurr = keyframe_curr_.mappoints_[i]
            if mpCurr is not None:
                mpCurr.replaceMapPoint(mpLoop)
            else:
                keyframe_curr_.mappoints_[i] = mpLoop                         # addMapPoint(mpLoop, i)
                mpLoop.addObservation(keyframe_curr_, i)
                mpLoop.computeDescriptor()


def _pad(per, n):
    return list(per) + [mr.NONE] * (n - len(per))


def _before(c):
    return mi.run_model(c["script"], **{k: c[k] for k in ("caps",) if k in c})


def _merged(c):
    m = _before(c)
    m.merge_loop_matches(c["curr"], c["match"])
    return m


def _took(m0, m, c):
    """a feature of curr that took its match holds the attributes the loop point had when the call began (its descriptor is
    computeDescriptor's: one of the rows of its holders)"""
    kf, n = m.store[c["curr"]], 0
    for i, b in enumerate(m.lm_branch):
        B = c["match"][i] if i < len(c["match"]) else -1
        if b in (mr.ADD, mr.REPLACE) and kf["ids"][i] == B and (kf["flags"][i] & 1) and m0.carriers(B):
            a = m0.attributes(B)
            got = (kf["points"][i], kf["normals"][i], kf["mind"][i], kf["maxd"][i], kf["ref"][i])
            want = (a["point"], a["normal"], a["mind"], a["maxd"], a["ref"])
            assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(got, want)), i
            n += 1
    return n


CASES = {name: (lambda name=name: mi.hand_case(name)) for name in mi.HAND_CASES}
CASES.update(no_step_alone=mi.no_step_alone_case, counters=mi.counters_case, erased_curr=mi.erased_curr_case)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_tables(name):
    c = CASES[name]()
    m = _merged(c)
    n = len(m.store[c["curr"]]["ids"])
    assert m.lm_record == c["rec"], (m.lm_record, c["rec"])
    assert list(m.loop_merge_result(c["NK"])["per_feature"][:n]) == _pad(c["per"], n)
    assert m.sticky == (mr.STICKY_INVALID if name == "erased_curr" else 0)
    _took(_before(c), m, c)


def test_carrier_limit_leaves_the_replace_undone():
    c = mi.capacity_carriers_case()
    m0, m = _before(c), _merged(c)
    assert m.lm_record == c["rec"] and m.sticky == mr.STICKY_FUSE and len(m.carriers(900)) == mr.CARRIERS_MAX + 1
    assert mr.store_bytes(m)[0] == mr.store_bytes(m0)[0]


POINTER_CASES = sorted(n for n in CASES if CASES[n]().get("pointers"))


@pytest.mark.parametrize("name", POINTER_CASES)
def test_merge_equals_the_pointer_model(name):
    """(the cases left out hold an id in two features of a key-frame at the start, meet a dead B, or add below or above a carrier of
    the same key-frame: the two rules below)"""
    c = CASES[name]()
    m = _before(c)
    p = MergePointers(m)
    rec = m.merge_loop_matches(c["curr"], c["match"])
    assert rec["n_dead"] == 0
    n = len(m.store[c["curr"]]["ids"])
    p.mergeLoopMatches(p.kfs[c["curr"]], [p.points.get(i) if i >= 0 else None for i in c["match"][:n]])
    _same_as_pointers(m, p, name)


def test_counters_are_added_when_both_are_listed():
    c = mi.counters_case()
    base = {e[0]: e[2:] for e in _before(c).recent_points()}
    m = _before(c)
    p = MergePointers(m)
    m.merge_loop_matches(c["curr"], c["match"])
    p.mergeLoopMatches(p.kfs[c["curr"]], [p.points.get(i) for i in c["match"]])
    got = {e[0]: e[2:] for e in m.recent_points()}
    assert got[900] == base[900] and base[900] != (0, 0)
    assert got[700] == (base[700][0] + base[900][0], base[700][1] + base[900][1]) == (p.points[700].found_cnt_, p.points[700].visible_cnt_)


def test_the_dead_b_rule():
    """the reference would hand a dead object's attributes to A's holders; the store skips the step and counts it"""
    c = mi.hand_case("b_is_the_a0_of_an_earlier_step")
    m = _merged(c)
    kf = m.store[c["curr"]]
    assert m.lm_record["n_dead"] == 1 and not m.carriers(900)
    assert kf["ids"][1] == 901 and (kf["flags"][1] & 1) and len(m.carriers(901)) == 2        # step 1 changed nothing
    m2 = _before(c)                                                                       # a dead id handed in by the caller
    before = mr.store_bytes(m2)
    m2.merge_loop_matches(c["curr"], [4242, -1])
    assert m2.lm_record["n_dead"] == 1 and m2.lm_record["steps"] == 1 and mr.store_bytes(m2) == before


@pytest.mark.parametrize("name,new,old", [("curr_holds_b_above", 0, 1), ("curr_holds_b_below", 1, 0)])
def test_the_add_beside_a_carrier_of_the_same_key_frame(name, new, old):
    """the reference does not test whether curr holds B already, and neither does the store: the id stands in two features, the
    observation is the lowest-numbered one (the pointer model would keep the one registered first: `old`)"""
    c = mi.hand_case(name)
    m = _merged(c)
    kf = m.store[c["curr"]]
    assert kf["ids"][new] == kf["ids"][old] == 700 and (kf["flags"][new] & 1) and (kf["flags"][old] & 1)
    assert m.observation(c["curr"], 700) == min(new, old) and len(m.carriers(700)) == 3 and len(m.observations(700)) == 2
    # computeDescriptor ran over the observations: curr's row is the lower feature's
    want = m.descriptor_set(700)
    assert any(np.asarray(w).tobytes() == np.asarray(kf["desc"][min(new, old)]).tobytes() for w in want)
    assert _took(_before(c), m, c) == 1


def test_a_step_that_shares_no_id_is_alone():
    for name, alone in (("every_step_alone", True), ("no_step_alone", False)):
        c = CASES[name]()
        m = _merged(c)
        kinds = [k for k in m.lm_kind if k]
        assert len(kinds) == c["rec"]["steps"] and all(k == (mr.ALONE if alone else mr.ORDERED) for k in kinds)
        assert m.lm_record["ordered"] == (0 if alone else c["rec"]["steps"])


# ---- the chains' scenes -------------------------------------------------------------------------------------------------------
def loop_scene(orc, name=ci.LOOP_SCENE):
    import loop_sim3_inputs as ls
    sc = mi.loop_scene(name)
    r = ls.run_model(orc, sc).result()
    return sc, r


def test_the_loop_scene_gives_curr_its_own_ids(orc):
    """the accepted scene's current key-frame carries its own copies of the shared points (ids NEW + p): the merge replaces
    them and adds to features without a point -- it is not a list of no-ops, so no variant of the scene is needed"""
    sc, r = loop_scene(orc)
    assert r["state"] == lr.ACCEPTED
    m = mi.scene_model(sc)
    p = MergePointers(m)
    cur = sc["current"]
    match = [int(x) for x in r["match_ids"]][:len(m.store[cur]["ids"])]
    L = m.propagate_loop(cur, lr.scw8_from13(r["Scw"]))
    assert L is not None
    rec = m.merge_loop_matches(cur, match)
    print("loop scene merge record:", rec)
    assert rec["n_dead"] == 0 and rec["adds"] >= 1 and rec["moved"] >= 1 and rec["replaces"] > 100 and rec["noops"] == 0
    assert rec["ordered"] == 0 and m.sticky == 0
    p.mergeLoopMatches(p.kfs[cur], [p.points.get(i) if i >= 0 else None for i in match])
    _same_as_pointers(m, p, "loop scene")


def test_the_merge_changes_the_loop_scene_chain(orc):
    sc, r = loop_scene(orc)
    cur, match_kf, ids = sc["current"], r["match_kf"], [int(x) for x in r["loop_point_ids"]]
    match = [int(x) for x in r["match_ids"]]
    out = []
    for merge in (True, False):
        m = mi.scene_model(sc)
        L, rows, w = mi.model_chain(m, cur, lr.scw8_from13(r["Scw"]), match[:len(m.store[cur]["ids"])], ids, match_kf, merge=merge)
        assert w is not None and m.sticky == 0
        out.append((rows, {k: np.asarray(v).tobytes() for k, v in w.items()}, mr.store_bytes(m)[0], m.loop_fuse_result()["totals"],
                    dict(m.conn.W[cur])))
    print("fusion totals with / without the merge:", out[0][3], out[1][3], "weights of curr:", out[0][4], out[1][4])
    # the merge takes compute_sim3's matches (searchByProjection, radius 10), the fusion re-finds most of them at radius 4: the map
    # and the covisibility weights between the two sides of the loop differ.  On THIS scene every weight is far above 100 either
    # way, so the rows and the window's edge list come out equal; the variant with 104 shared points and the seeded chain below
    # are where they differ
    assert out[0][2] != out[1][2], "the stores agree"
    assert out[0][4] != out[1][4] and all(out[0][4][k] > out[1][4][k] for k in out[1][4]), "the weights agree"
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]


def test_the_merge_decides_a_family_a_edge_on_the_loop_scene_variant(orc):
    """the same scene with 104 shared points is still ACCEPTED (the section 4n model), and there the window's edge list depends on the
    merge: curr - match has weight 104 with it (a family-A edge) and 97 without it (none)"""
    sc, r = loop_scene(orc, mi.LOOP_VARIANT)
    assert r["state"] == lr.ACCEPTED and r["match_kf"] == 1
    cur, match_kf, ids = sc["current"], r["match_kf"], [int(x) for x in r["loop_point_ids"]]
    match = [int(x) for x in r["match_ids"]]
    out = []
    for merge in (True, False):
        m = mi.scene_model(sc)
        L, rows, w = mi.model_chain(m, cur, lr.scw8_from13(r["Scw"]), match[:len(m.store[cur]["ids"])], ids, match_kf, merge=merge)
        assert w is not None and m.sticky == 0
        if merge:
            rec = m.lm_record
            assert rec["n_dead"] == 0 and rec["adds"] >= 1 and rec["moved"] >= 1 and rec["ordered"] == 0
        out.append((m.conn.W[cur][match_kf], m.pg_record["n_a"], m.pg_record["n_edges"], w["e_i"].tobytes() + w["e_j"].tobytes()))
    print("variant: (weight curr - match, n_a, n_edges) with / without the merge:", out[0][:3], out[1][:3])
    assert out[0][0] >= 100 > out[1][0] and out[0][1] == out[1][1] + 1 and out[0][2] == out[1][2] + 1 and out[0][3] != out[1][3]


def seeded_before_the_merge():
    mrun, m = mi.seeded_chain_model()
    for s in fi.seeded_chain():
        mrun.step(s)
        if s[0] == "neighbors":
            break
    for s in ci.seeded_old_keyframe(m):
        mrun.step(s)
    return mrun, m


def test_the_seeded_chain_has_adds_and_moving_replaces():
    mrun, m = seeded_before_the_merge()
    cur = ci.SEEDED_MATCH - 1
    match = mi.seeded_match_ids(m, cur)
    out = []
    for merge in (True, False):
        mrun, m = seeded_before_the_merge()
        L, rows, w = mi.model_chain(m, cur, ci.chain_scw(m, cur), match, ci.seeded_loop_ids(m, 0), ci.SEEDED_MATCH, merge=merge)
        assert w is not None and m.sticky == 0
        out.append((rows, {k: np.asarray(v).tobytes() for k, v in w.items()}))
        if merge:
            rec = m.lm_record
            print("seeded scene merge record:", rec)
            assert rec["n_dead"] == 0 and rec["adds"] == 60 and rec["replaces"] == 60 and rec["moved"] >= 1 and rec["ordered"] == 0
    assert out[0][0] != out[1][0] or out[0][1] != out[1][1], "the merge leaves the loop connections and the window as they were"
