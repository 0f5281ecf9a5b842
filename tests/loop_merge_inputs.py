"""Inputs of the loop-merge tests (test infrastructure): the models, the script step and its runner, the hand-made stores shared
by the model's CPU tests (tests/test_loop_merge_ref.py) and the device's GPU tests (tests/test_gpu_loop_merge.py), and the
chains' scenes.

A script is a list of the steps of tests/loop_fuse_inputs.py and one more:
  ("merge", curr, match_ids)      merge_loop_matches
The hand stores are tests/fuse_inputs.py's: seven key-frames at x = 0.3 k, y = 0.02 k looking down +z; the current key-frame is
key-frame 6.  A hand case states the branch of every feature of the current key-frame and the record, worked out by hand."""
import numpy as np

import fuse_inputs as fi
import loop_correct_inputs as ci
import loop_fuse_inputs as lfi
import loop_merge_ref as mr
from loop_fuse_ref import LoopFuseModel

CURR = fi.T_HAND
NONE, ADD, NOOP, REPLACE, DEAD, UNDONE = mr.NONE, mr.ADD, mr.NOOP, mr.REPLACE, mr.DEAD, mr.UNDONE


class HandModel(mr.LoopMergeModel, LoopFuseModel):
    """the merge on the loop fusion's store model, for the hand stores"""


class ChainModel(mr.LoopMergeModel, ci.ChainModel):
    """the merge, the loop correction, the loop fusion and the pose graph's window on one store, for the chains"""


class ModelRunner(lfi.ModelRunner):
    def __init__(self, *a, model=HandModel, **kw):
        super().__init__(*a, model=model, **kw)
        self.m.enable_loop_merge()

    def step(self, s):
        if s[0] == "merge":
            self.m.merge_loop_matches(s[1], s[2])
        else:
            super().step(s)


def run_model(script, caps=fi.CAPS, **kw):
    r = ModelRunner(caps, **kw)
    for s in script:
        r.step(s)
    return r.m


def _rec(**kw):
    return dict({k: 0 for k in mr.LM_RECORD}, curr=CURR, **kw)


def _finish(h, match, per, rec, NK=64, **extra):
    for k in range(7):          # every key-frame holds something (a pose, a record)
        h.see(k, h.point(600, 20 + 60 * k, T=k), d=1, pid=990 + k)
    return dict(extra, script=h.prepared(), curr=CURR, match=list(match), per=list(per), rec=rec, NK=NK)


def _add(h, u, v, B, d=5):
    """-> feature.  An empty feature of curr and a loop point B that key-frames 0 and 1 hold"""
    p = h.point(u, v)
    h.see(0, p, d=d, pid=B), h.see(1, p, d=d + 1, pid=B)
    return h.see(CURR, p, d=d + 2, flag=0, pid=-1)


def _replace(h, u, v, A, B, d=8):
    """-> feature.  A is held by curr, key-frame 2 and key-frame 3; B by key-frame 3 and key-frame 4: curr's and key-frame 2's
    features go over to B, key-frame 3's is cleared"""
    p = h.point(u, v)
    f = h.see(CURR, p, d=d, pid=A)
    h.see(2, p, d=d, pid=A), h.see(3, p, d=d, pid=A), h.see(3, p, d=d + 1, pid=B, stereo=True), h.see(4, p, d=d + 1, pid=B)
    return f


def _noop(h, u, v, B, d=3):
    p = h.point(u, v)
    f = h.see(CURR, p, d=d, pid=B)
    h.see(1, p, d=d, pid=B)
    return f


def hand_case(name):
    """-> dict(script, curr, match, per, rec, NK, pointers: the pointer transcription can run it and must agree)"""
    h = fi.Hand()
    if name == "add":
        _add(h, 100, 100, 700)
        return _finish(h, [700], [ADD], _rec(steps=1, adds=1), pointers=True)
    if name == "replace_moved_and_cleared":
        _replace(h, 200, 120, 900, 700)
        return _finish(h, [700], [REPLACE], _rec(steps=1, replaces=1, moved=1, cleared=1), pointers=True)
    if name == "a_equals_b":
        _noop(h, 100, 300, 700)
        return _finish(h, [700], [NOOP], _rec(steps=1, noops=1), pointers=True)
    if name == "every_step_alone":
        # an add, a replace, a no-op, a feature without a match, a second add and a second replace: no two steps share an id
        _add(h, 100, 100, 700), _replace(h, 200, 120, 900, 701), _noop(h, 100, 300, 702)
        h.see(CURR, h.point(50, 400), d=9, pid=950)
        _add(h, 400, 100, 703, d=20), _replace(h, 500, 220, 901, 704, d=30)
        return _finish(h, [700, 701, 702, -1, 703, 704], [ADD, REPLACE, NOOP, NONE, ADD, REPLACE],
                       _rec(steps=5, adds=2, noops=1, replaces=2, moved=2, cleared=2), pointers=True)
    if name == "a_in_two_features_both_matched":
        # two features of curr carry 900 (key-frame 1 holds it too): 900 -> 700 converts the lower one and key-frame 1's and clears
        # the other; the second step finds its feature empty and ADDS 701
        p, q = h.point(150, 350), h.point(500, 350)
        h.see(CURR, p, d=6, pid=900), h.see(CURR, q, d=7, pid=900), h.see(1, p, d=6, pid=900)
        h.see(0, p, d=8, pid=700), h.see(2, q, d=9, pid=701)
        return _finish(h, [700, 701], [REPLACE, ADD], _rec(steps=2, adds=1, replaces=1, moved=1, cleared=1, ordered=2), pointers=False)
    if name == "b_is_the_a0_of_an_earlier_step":
        # step 0 replaces 900 away; step 1 asks for 900: dead
        p, q = h.point(150, 150), h.point(450, 150)
        h.see(CURR, p, d=6, pid=900), h.see(1, p, d=6, pid=900), h.see(0, p, d=8, pid=700)
        h.see(CURR, q, d=7, pid=901), h.see(2, q, d=7, pid=901)
        return _finish(h, [700, 900], [REPLACE, DEAD], _rec(steps=2, replaces=1, moved=1, n_dead=1, ordered=2), pointers=False)
    if name == "b_is_the_a0_of_a_later_step":
        # step 0: 901 -> 900, which curr holds at feature 1: feature 0 is cleared, key-frame 2's goes over; step 1: 900 -> 700 takes
        # curr's feature 1, key-frame 1's and the one key-frame 2 has just been given
        p, q = h.point(150, 150), h.point(450, 150)
        h.see(CURR, q, d=7, pid=901), h.see(2, q, d=7, pid=901)
        h.see(CURR, p, d=6, pid=900), h.see(1, p, d=6, pid=900), h.see(0, p, d=8, pid=700)
        return _finish(h, [900, 700], [REPLACE, REPLACE], _rec(steps=2, replaces=2, moved=2, cleared=1, ordered=2), pointers=True)
    if name in ("curr_holds_b_above", "curr_holds_b_below"):
        # curr holds 700 at a feature without a match, and an empty feature is matched to 700: below it (the new feature becomes
        # curr's observation: the lowest-numbered) or above it (the old one stays)
        p = h.point(300, 200)
        h.see(0, p, d=5, pid=700)
        if name == "curr_holds_b_above":
            h.see(CURR, p, d=40, flag=0, pid=-1, shift=3.0), h.see(CURR, p, d=6, pid=700)
            match, per = [700, -1], [ADD, NONE]
        else:
            h.see(CURR, p, d=6, pid=700), h.see(CURR, p, d=40, flag=0, pid=-1, shift=3.0)
            match, per = [-1, 700], [NONE, ADD]
        return _finish(h, match, per, _rec(steps=1, adds=1), pointers=False)
    if name == "match_beyond_the_features":
        # the list is longer than curr has features (the filler of _finish makes two): the entries behind them are not steps
        _add(h, 100, 100, 700)
        p = h.point(300, 300)
        h.see(0, p, d=4, pid=701), h.see(1, p, d=4, pid=702)
        return _finish(h, [700, -1, 701, 702, 702], [ADD, NONE], _rec(steps=1, adds=1), pointers=True)
    if name == "negative_id_under_bit_0_clear":
        # an empty feature whose id word still holds an old id: bit 0 decides
        p = h.point(100, 100)
        h.see(0, p, d=5, pid=700), h.see(CURR, p, d=7, flag=0, pid=900), h.see(1, p, d=9, pid=900)
        return _finish(h, [700], [ADD], _rec(steps=1, adds=1), pointers=True)
    raise ValueError(name)


HAND_CASES = ("add", "replace_moved_and_cleared", "a_equals_b", "every_step_alone", "a_in_two_features_both_matched",
              "b_is_the_a0_of_an_earlier_step", "b_is_the_a0_of_a_later_step", "curr_holds_b_above", "curr_holds_b_below",
              "match_beyond_the_features", "negative_id_under_bit_0_clear")


def no_step_alone_case():
    """a_in_two_features_both_matched and b_is_the_a0_of_an_earlier_step on one store: four steps, every one shares an id"""
    h = fi.Hand()
    p, q = h.point(150, 350), h.point(500, 350)
    h.see(CURR, p, d=6, pid=900), h.see(CURR, q, d=7, pid=900), h.see(1, p, d=6, pid=900)
    h.see(0, p, d=8, pid=700), h.see(2, q, d=9, pid=701)
    r, s = h.point(150, 150), h.point(450, 150)
    h.see(CURR, r, d=6, pid=910), h.see(1, r, d=6, pid=910), h.see(0, r, d=8, pid=710)
    h.see(CURR, s, d=7, pid=911), h.see(2, s, d=7, pid=911)
    return _finish(h, [700, 701, 710, 910], [REPLACE, ADD, REPLACE, DEAD],
                   _rec(steps=4, adds=1, replaces=2, moved=2, cleared=1, n_dead=1, ordered=4), pointers=False)


def counters_case():
    """replace_moved_and_cleared with 900 and 700 in the recent list and counters that differ: 700 gets 900's on top"""
    c = hand_case("replace_moved_and_cleared")
    script = []
    for s in c["script"]:
        script.append(s)
        if s[0] == "xy":
            script.append(("process", s[1]))
    script.append(("stats", [900, 700], [3, 5], [2, 1]))
    return dict(c, script=script)


def erased_curr_case():
    c = hand_case("add")
    return dict(c, script=c["script"] + [("erase", CURR)], per=[NONE], rec=_rec(), pointers=False)


def capacity_carriers_case():
    """fuse_inputs.carriers_case: feature 0 of key-frame 0 carries a point with 1025 carriers; the replace is recorded and left undone"""
    c = fi.carriers_case()
    T, ids = c["fuse"]
    rec = dict({k: 0 for k in mr.LM_RECORD}, curr=T, steps=1, replaces=1, undone=1)
    return dict(script=c["script"], curr=T, match=[ids[0]], per=[UNDONE], rec=rec, NK=c["NK"], K=c["K"], caps=(16, 256, 1024), pointers=False)


# ---- the chains ---------------------------------------------------------------------------------------------------------------
def scene_model(sc, exp=None, log=None):
    """loop_correct_inputs.scene_model's store on the ChainModel with the merge in front"""
    import loop_sim3_inputs as ls
    m = ChainModel(ls.CAM6, ls.SF, 50000, ls.BA_CAPS, exp, log, ls.MAX_RECENT)
    m.enable_fuse(ls.BOUNDS, 1024)
    m.enable_loop_fuse(ci.LOOP_LC_CAPS[0], sc["caps"]["max_loop_points"])
    m.enable_loop_correct(*ci.LOOP_LC_CAPS)
    m.enable_loop_merge()
    for k, kf in enumerate(sc["store"]):
        m.insert(kf["ids"], kf["flags"], kf["bad"], kf["desc"], kf["angle"], kf["nodes"])
        m.set_keypoints(k, kf["octave"], kf["depth"], kf["uright"])
        m.set_xy(k, np.stack([kf["x"], kf["y"]], 1))
        if kf["pose"] is not None:
            m.set_pose(k, kf["pose"])
        m.set_map_side(k, kf["points"], kf["normals"], kf["min_dist"], kf["max_dist"])
        m.store[k]["pdesc"] = np.array(kf["point_desc"], np.uint8).reshape(-1, 32)
        m.set_point_refs(k, ci.scene_refs(kf, k))
    m.update_connections(list(range(len(sc["store"]))))
    return m


LOOP_VARIANT = "shared104"


def loop_scene(name):
    """loop_sim3_inputs.scene(name), or the variant below"""
    import loop_sim3_inputs as ls
    return loop_scene_variant() if name == LOOP_VARIANT else ls.scene(name)


def loop_scene_variant(n_shared=104, n_extra=20, n_own=6, seed=1):
    """loop_sim3_inputs' accepted scene (its default branch: the same world, cameras, drift and key-frames) with 104 shared points
    instead of 255: the merge gives curr - match a weight of 104, above the pose graph's family-A threshold of 100, where the
    fusion alone re-finds 97 of them -- the window's edge list depends on the merge (tests/test_loop_merge_ref.py)"""
    import loop_sim3_inputs as ls
    w = ls.World(seed)
    c_old, c_cur = np.array([0.0, 0.0, 0.0]), np.array([0.08, 0.03, -0.1])
    A, E = list(range(n_shared)), list(range(n_shared, n_shared + n_extra))
    own = list(range(n_shared + n_extra, n_shared + n_extra + n_own))
    B = list(range(n_shared + n_extra + n_own, n_shared + n_extra + n_own + 12))
    nb = (A + E)[:ls.NK - 8]
    w.keyframe(c_old + [-0.12, 0.0, 0.0], nb)                     # 0
    w.keyframe(c_old, A + B)                                      # 1: the candidate
    w.keyframe(c_old + [0.12, 0.02, 0.0], nb)                     # 2
    while len(w.store) < 6:                                       # fillers: old-pass key-frames elsewhere
        w.keyframe(c_old + [0.3, 0.1 * (len(w.store) % 2), 0.0], B)
    current = w.keyframe(c_cur, own + A + E, new=True, rot=(0.01, -0.02, 0.015), unmapped=E[::2])
    return dict(fix_scale=True, max_rounds=8, caps=dict(ls.LOOP_CAPS), store=w.store, current=current, cand=[1],
                rand=ls.rand_values(seed, 3 * 300), A=A, E=E)


def seeded_chain_model(exp=None, log=None):
    """-> (runner, model) of the seeded 12 x 256 scene (tests/test_loop_correct_ref.py's, on the ChainModel with the merge)"""
    r = ModelRunner(fi.SCENE_CAPS, exp=exp, log=log, max_recent=fi.SCENE_RECENT, max_candidates=fi.SCENE_CANDIDATES,
                    max_corrected=ci.CHAIN_LC_CAPS[0], max_loop_points=lfi.CHAIN_LOOP_POINTS, model=ChainModel)
    r.m.enable_loop_correct(*ci.CHAIN_LC_CAPS)
    return r, r.m


def seeded_match_ids(m, curr, seed=5, n_replace=60, n_add=60):
    """the seeded 12 x 256 scene's match list for key-frame curr: n_replace of its live features and n_add of its empty ones, each
    matched to a live point of the loop-side key-frame SEEDED_MATCH (distinct, none of them held by curr) -> match_ids"""
    rng = np.random.default_rng(seed)
    kf = m.store[curr]
    live = [f for f in range(len(kf["ids"])) if (kf["flags"][f] & 1) and kf["ids"][f] >= 0]
    free = [f for f in range(len(kf["ids"])) if not (kf["flags"][f] & 1)]
    give = [p for p in m.live_ids(ci.SEEDED_MATCH) if m.observation(curr, p) < 0]
    assert len(live) >= n_replace and len(free) >= n_add and len(give) >= n_replace + n_add, (len(live), len(free), len(give))
    feats = [int(f) for f in rng.choice(live, n_replace, replace=False)] + [int(f) for f in rng.choice(free, n_add, replace=False)]
    out = [-1] * len(kf["ids"])
    for f, p in zip(feats, give):
        out[f] = int(p)
    return out


def model_chain(m, curr, Scw, match_ids, ids, match, merge=True):
    """propagate_loop -> [merge_loop_matches] -> search_and_fuse -> loop_connections -> pg_window on model m
    -> (the propagate's lists, the rows, the window)"""
    L = m.propagate_loop(curr, Scw)
    assert L is not None, m.lc_record
    if merge:
        m.merge_loop_matches(curr, match_ids)
    m.search_and_fuse(L["corr_kf"], L["S_corr"], ids, ci.CHAIN_TH)
    rows = m.loop_connections()
    assert rows is not None, m.lc_record
    return L, rows, m.pg_window(curr, match, m.lc_inputs())
