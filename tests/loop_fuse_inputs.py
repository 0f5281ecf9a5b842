"""Inputs of the loop-fusion tests (test infrastructure): the script step, its runner on the model (tests/loop_fuse_ref.py), the
hand-made stores shared by the model's CPU tests and the device's GPU tests, and the seeded scene's chain.

A script is a list of the steps of tests/fuse_inputs.py and one more:
  ("loopfuse", corr_kf, S_corr, ids, threshold)      search_and_fuse
The hand stores are tests/fuse_inputs.py's: seven key-frames at x = 0.3 k, y = 0.02 k looking down +z.  sim3_of(k) is the Sim3
that gives key-frame k its own pose (scale 1), so that a pass under it sees what the key-frame sees."""
import numpy as np

import fuse_inputs as fi
import pose_graph_store_inputs as pi
import pose_graph_store_ref as pr
from loop_fuse_ref import LoopFuseModel

f32 = np.float32
MAX_CORRECTED, MAX_LOOP_POINTS = 8, 64
TH = 4.0


class ChainModel(LoopFuseModel, pr.PoseGraphModel):
    """the loop fusion and the pose graph's window (tests/pose_graph_store_ref.py) on one store, for the seeded chain"""


class ModelRunner(fi.ModelRunner):
    def __init__(self, caps=fi.CAPS, first_point_id=fi.FIRST_ID, exp=None, log=None, max_recent=fi.ui.MAX_RECENT,
                 max_candidates=fi.MAX_CANDIDATES, max_corrected=MAX_CORRECTED, max_loop_points=MAX_LOOP_POINTS, model=LoopFuseModel):
        self.m = model(fi.CAM6, fi.SF, first_point_id, caps, exp, log, max_recent)
        self.m.enable_fuse(fi.BOUNDS, max_candidates)
        self.m.enable_loop_fuse(max_corrected, max_loop_points)

    def step(self, s):
        if s[0] == "loopfuse":
            self.m.search_and_fuse(s[1], s[2], s[3], s[4])
        else:
            super().step(s)


def run_model(script, caps=fi.CAPS, **kw):
    r = ModelRunner(caps, **kw)
    for s in script:
        r.step(s)
    return r.m


def sim3_of(k, scale=1.0, spacing=None):
    """key-frame k's own pose as a Sim3 (identity rotation; the translation is the pose's, whatever the scale)"""
    t = (-0.3 * k, -0.02 * k, 0.0) if spacing is None else (-spacing * k, 0.0, 0.0)
    return [0.0, 0.0, 0.0, 1.0, t[0], t[1], t[2], scale]


def _finish(h, corr, ids, NK=64, th=TH, **extra):
    for k in range(7):          # every key-frame holds something (a pose, a record)
        h.see(k, h.point(600, 20 + 60 * k, T=k), d=1, pid=990 + k)
    return dict(extra, script=h.prepared(), corr_kf=[k for k, _ in corr], S_corr=[S for _, S in corr], ids=ids, th=th, NK=NK)


def hand_case(name):
    """-> dict(script, corr_kf, S_corr, ids, th, NK, per_pass = the model's result worked out by hand)"""
    h, T = fi.Hand(), fi.T_HAND
    empty = dict(flag=0, pid=-1)
    if name == "add":
        p = h.point(100, 100)
        h.see(0, p, d=5), h.see(1, p, d=6), h.see(T, p, d=5, **empty)
        return _finish(h, [(T, sim3_of(T))], [100 + p], per_pass=[(1, 1, 1, 0, 0, 0)])
    if name == "replace_three_holders":
        # 900 is held by the target, key-frame 2 and key-frame 3; key-frame 3 holds the loop point too: its feature is cleared
        p = h.point(200, 120)
        h.see(T, p, d=8, pid=900), h.see(2, p, d=8, pid=900), h.see(3, p, d=8, pid=900)
        h.see(3, p, d=9), h.see(4, p, d=9)
        return _finish(h, [(T, sim3_of(T))], [100 + p], per_pass=[(1, 1, 0, 1, 1, 1)])
    if name == "two_on_one_empty_feature":
        # 700 is added; 701 finds 700 there and replaces it: the target's feature and key-frame 0's go over to 701
        p = h.point(420, 150)
        h.see(T, p, d=10, **empty), h.see(0, p, d=10, pid=700), h.see(2, p, d=11, pid=701), h.see(3, p, d=11, pid=701)
        return _finish(h, [(T, sim3_of(T))], [700, 701], per_pass=[(2, 2, 1, 1, 1, 0)])
    if name == "same_org_one_feature":
        # both loop points hit the feature that carries 900: 900 -> 700 moves the target's and key-frame 1's features, 900 -> 701
        # finds 900 emptied and moves nothing
        p = h.point(300, 200)
        h.see(T, p, d=8, pid=900), h.see(1, p, d=8, pid=900), h.see(0, p, d=9, pid=700), h.see(2, p, d=9, pid=701)
        return _finish(h, [(T, sim3_of(T))], [700, 701], per_pass=[(2, 2, 0, 2, 1, 0)])
    if name == "same_org_two_features":
        # two features of the target carry 900: the first replace converts the lower one and clears the other
        p, q = h.point(150, 350), h.point(500, 350)
        h.see(T, p, d=6, pid=900), h.see(T, q, d=7, pid=900)
        h.see(0, p, d=6), h.see(1, p, d=6), h.see(0, q, d=7)
        return _finish(h, [(T, sim3_of(T))], [100 + p, 100 + q], per_pass=[(2, 2, 0, 2, 1, 1)])
    if name == "dies_in_pass_1":
        # pass 1 (key-frame 4): 700 is added and replaced by 701; pass 2 (key-frame 6) finds 700 bad
        p = h.point(420, 150, T=4)
        h.see(4, p, d=10, **empty), h.see(0, p, d=10, pid=700), h.see(2, p, d=11, pid=701), h.see(3, p, d=11, pid=701)
        return _finish(h, [(4, sim3_of(4)), (T, sim3_of(T))], [700, 701], per_pass=[(2, 2, 1, 1, 1, 0), (1, 0, 0, 0, 0, 0)])
    if name == "already_held":
        p, q = h.point(100, 300), h.point(400, 300)
        h.see(T, p, d=3), h.see(1, p, d=3)                      # held by the target already
        h.see(0, q, d=7), h.see(T, q, d=7, **empty)
        return _finish(h, [(T, sim3_of(T))], [100 + p, -1, 100 + q], per_pass=[(1, 1, 1, 0, 0, 0)])
    if name == "round_not_floor":
        # u = 255, radius <= 4.8: the floor range is column 25 alone; the feature at 256.5 is inside the radius, but its ROUNDED
        # column is 26
        p = h.point(255, 100)
        h.see(0, p, d=2), h.see(T, p, d=2, shift=1.5, **empty)
        return _finish(h, [(T, sim3_of(T))], [100 + p], per_pass=[(1, 0, 0, 0, 0, 0)])
    if name == "not_a_multiple_of_64":
        p = h.point(330, 260)
        h.filler(T, 66)
        h.see(0, p, d=9), h.see(2, p, d=9), h.see(T, p, d=9, **empty)      # feature 66 of the target
        q = h.point(50, 50)
        h.see(1, q, d=4), h.see(T, q, d=4, pid=900), h.see(T, q, d=30, pid=900, shift=40.0)
        return _finish(h, [(T, sim3_of(T))], [100 + p, 100 + q], NK=70, per_pass=[(2, 2, 1, 1, 1, 1)])
    if name == "scale_quirk":
        # scale 1.07 with the target's own translation: as it stands the pose is the target's and the feature AT the projection
        # wins; divided by the scale the camera moves 0.118 units and the projection 11.8 pixels, onto the second feature
        p = h.point(250, 200)
        h.see(0, p, d=5), h.see(T, p, d=5, **empty), h.see(T, p, d=5, shift=11.8, **empty)
        return _finish(h, [(T, sim3_of(T, 1.07))], [100 + p], per_pass=[(1, 1, 1, 0, 0, 0)])
    if name == "threshold":
        # the only feature sits 3.7 pixels from the projection: inside 4 * scale_factor, outside 3 * scale_factor at levels 0 and 1
        p = h.point(100, 100)
        h.see(0, p, d=5), h.see(T, p, d=5, shift=3.7, **empty)
        return _finish(h, [(T, sim3_of(T))], [100 + p], per_pass=[(1, 1, 1, 0, 0, 0)])
    if name == "targets_erased_or_without_a_pose":
        # the same point is added to key-frame 3 and to key-frame 6; key-frame 4 is erased and key-frame 5 has no pose in between
        p = h.point(300, 300, T=4)
        h.see(0, p, d=5)
        for k in (3, 4, 5, 6):
            h.see(k, p, d=5, **empty)
        c = _finish(h, [(k, sim3_of(k)) for k in (3, 4, 5, 6)], [100 + p], per_pass=[(1, 1, 1, 0, 0, 0), (0,) * 6, (0,) * 6, (1, 1, 1, 0, 0, 0)])
        c["script"] = [s for s in c["script"] if not (s[0] == "pose" and s[1] == 5)] + [("erase", 4)]
        return c
    raise ValueError(name)


HAND_CASES = ("add", "replace_three_holders", "two_on_one_empty_feature", "same_org_one_feature", "same_org_two_features", "dies_in_pass_1",
              "already_held", "round_not_floor", "not_a_multiple_of_64", "scale_quirk", "threshold", "targets_erased_or_without_a_pose")


def counters_case():
    """same_org_one_feature with 900, 700 and 701 in the recent list and counters that differ: both replaces add 900's"""
    c = hand_case("same_org_one_feature")
    script = []
    for s in c["script"]:
        script.append(s)
        if s[0] == "xy":
            script.append(("process", s[1]))
    script.append(("stats", [900, 700, 701], [3, 5, 7], [2, 1, 4]))
    return dict(c, script=script)


def z_case():
    """the camera of pass 1 stands a tenth of a millimetre in front of the loop point (z just above 0: not skipped there, the
    distance gate skips it); the camera of pass 2 stands a unit behind it (z < 0)"""
    h, T = fi.Hand(), fi.T_HAND
    p = h.point(320, 240, T=0)
    h.see(0, p, d=5), h.see(1, p, d=5)
    P = [float(x) for x in h.W[p]]                    # (key-frame 0's row is the world point itself)
    near = [0.0, 0.0, 0.0, 1.0, -P[0], -P[1], -P[2] + 1e-4, 1.0]
    behind = [0.0, 0.0, 0.0, 1.0, -P[0], -P[1], -P[2] - 1.0, 1.0]
    return _finish(h, [(5, near), (T, behind)], [100 + p], per_pass=[(0,) * 6, (0,) * 6])


def capacity_candidates_case():
    """three loop points pass the gates where a pass takes two; one of them would match"""
    c = fi.capacity_candidates_case()
    T, ids = c["fuse"]
    return dict(script=c["script"], corr_kf=[T], S_corr=[sim3_of(T)], ids=ids, th=TH, NK=c["NK"], max_candidates=2)


def capacity_matches_case():
    """point `a` of fuse_inputs.composed_case is added to key-frame 1 and to key-frame 2; the third match of the call does not
    fit the two nodes of the overlay: pass 3 and pass 4 are left undone"""
    script, current, a = fi.composed_case()
    corr = [1, 2, 3, 4]
    return dict(script=script, corr_kf=corr, S_corr=[sim3_of(k) for k in corr], ids=[a], th=TH, NK=64, max_candidates=2)


def capacity_carriers_case():
    """fuse_inputs.carriers_case: the feature of the target carries a point with 1025 carriers; the replace is recorded and left
    undone"""
    c = fi.carriers_case()
    T, ids = c["fuse"]
    S = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.5, 1.0]      # (key-frame 0 stands half a unit behind the others)
    return dict(script=c["script"], corr_kf=[T], S_corr=[S], ids=ids, th=TH, NK=c["NK"], K=c["K"], caps=(16, 256, 1024))


# ---- the seeded scene -------------------------------------------------------------------------------------------------------
CHAIN_CORRECTED = (4, 6, 7)
CHAIN_LOOP_POINTS = 40


def chain_inputs(m, seed=11):
    """the loop step of the seeded chain on the state of model m.  Key-frame 4 is corrected to its own pose (the Sim3 of the pose
    column, as the loop's anchor is), the key-frames 6 and 7 to Sim3s near theirs (pose_graph_store_inputs.sim3_near: a few
    centimetres and degrees off, so that their passes decide gates and match nothing); the loop points are the first 40 live
    points of the store that key-frame 4 does not hold"""
    corr = list(CHAIN_CORRECTED)
    S = [pr.from_pose(m.store[k]["pose"]) if k == corr[0] else pi.sim3_near(m.store[k]["pose"], seed + k) for k in corr]
    ids = []
    for k in range(len(m.store)):
        for p in m.live_ids(k):
            if p not in ids and m.observation(corr[0], p) < 0:
                ids.append(int(p))
    return corr, S, ids[:CHAIN_LOOP_POINTS]
