"""Inputs of the map-point fusion tests (test infrastructure): the script format, its runner on the model (tests/fuse_ref.py),
the hand-made stores shared by the model's CPU tests and the device's GPU tests, the target-list graphs and the seeded 12 x 256
scene with its chain.

A script is a list of the steps of tests/point_upkeep_inputs.py and three more:
  ("refresh", ids)            vo_kfstore_refresh_points (normals and min / max distance of hand-made points)
  ("fuse", T, ids)            fuse_map_points(T, ids, 3)
  ("neighbors", current)      search_in_neighbors
Hand-made key-frames stand at x = 0.3 k, y = 0.02 k and look down +z; the target of the hand cases is key-frame 6, whose pixel
(u, v) sees the world point at_pixel(u, v) at depth 5."""
import numpy as np

import local_ba_inputs as li
import new_points_inputs as ni
import point_upkeep_inputs as ui
from fuse_ref import FuseModel

f32 = np.float32
BOUNDS = (0.0, 640.0, 0.0, 480.0)
MAX_CANDIDATES = 256
CAPS, CAM6, SF, FIRST_ID = ui.CAPS, ui.CAM6, ui.SF, ui.FIRST_ID
T_HAND = 6


class ModelRunner(ui.ModelRunner):
    def __init__(self, caps=CAPS, first_point_id=FIRST_ID, exp=None, log=None, max_recent=ui.MAX_RECENT, max_candidates=MAX_CANDIDATES):
        self.m = FuseModel(CAM6, SF, first_point_id, caps, exp, log, max_recent)
        self.m.enable_fuse(BOUNDS, max_candidates)

    def step(self, s):
        m = self.m
        if s[0] == "refresh":
            m.refresh([int(p) for p in s[1]])
        elif s[0] == "fuse":
            m.fuse_map_points(s[1], s[2])
        elif s[0] == "neighbors":
            m.search_in_neighbors(s[1])
        else:
            super().step(s)


def run_model(script, caps=CAPS, **kw):
    r = ModelRunner(caps, **kw)
    for s in script:
        r.step(s)
    return r.m


def at_pixel(u, v, T=T_HAND, z=5.0):
    """the world point key-frame T sees at pixel (u, v) and depth z"""
    return np.array([(u - 320.0) / 500.0 * z + 0.3 * T, (v - 240.0) / 500.0 * z + 0.02 * T, z])


class Hand(ui.Hand):
    """point_upkeep_inputs.Hand over a world made point by point: point(u, v) -> the number of the world point key-frame 6
    sees at (u, v)"""

    big = True          # (the cases choose their own NK)

    def __init__(self, K=7, spacing=None):
        super().__init__(K, W=np.zeros((0, 3)))
        if spacing is not None:
            self.pose = [ni.pose12(np.eye(3), (spacing * k, 0.0, 0.0)) for k in range(K)]

    def filler(self, k, n):
        super().filler(k, n)
        self.desc[k] += [ui.bits(0)] * n

    def point(self, u, v, T=T_HAND):
        self.W = np.concatenate([self.W, at_pixel(u, v, T)[None]])
        return len(self.W) - 1

    def ids(self):
        return sorted({p for f in self.kf for p, fl in zip(f["ids"], f["flags"]) if p >= 0 and (fl & 1)})

    def prepared(self, updates=()):
        """the script with every point's normal, distances and descriptor computed (updates = None: and every key-frame's
        connections updated)"""
        ids = self.ids()
        return self.script(updates=updates) + [("refresh", ids), ("descriptors", ids)]


def hand_case(name):
    """-> dict(script, fuse = (T, ids), kinds = the model's fuse_log kinds worked out by hand, NK)"""
    h, T = Hand(), T_HAND
    empty = dict(flag=0, pid=-1)
    NK = 64
    if name == "add":
        p = h.point(100, 100)
        h.see(0, p, d=5), h.see(1, p, d=6), h.see(T, p, d=5, **empty)
        ids, kinds = [100 + p], [("add", -1)]
    elif name in ("obs_greater", "obs_equal", "obs_smaller"):
        p = h.point(200, 120)
        orgs, cands = {"obs_greater": ((0, 1, 2), (3,)), "obs_equal": ((0,), (3, 4)), "obs_smaller": ((), (3, 4))}[name]
        for k in orgs + (T,):
            h.see(k, p, d=8, pid=900)
        for k in cands:
            h.see(k, p, d=9)
        ids = [100 + p]
        kinds = [("kept_org" if name == "obs_greater" else "kept_candidate", 900)]
    elif name == "holder_overlap":
        p = h.point(300, 200)
        h.see(T, p, d=4, pid=900), h.see(3, p, d=4, pid=900)
        h.see(3, p, d=5), h.see(4, p, d=5), h.see(5, p, d=5, stereo=True)
        ids, kinds = [100 + p], [("kept_candidate", 900)]
    elif name == "held_and_repeated":
        p, q = h.point(100, 300), h.point(400, 300)
        h.see(T, p, d=3), h.see(1, p, d=3)                      # held by the target already
        h.see(0, q, d=7), h.see(T, q, d=7, **empty)
        ids, kinds = [100 + p, 100 + q, 100 + q, -1, 100 + p], [("add", -1)]
    elif name in ("two_on_one_feature", "two_on_one_feature_first_stays", "three_on_one_feature"):
        p = h.point(420, 150)
        h.see(T, p, d=10, **empty)
        if name == "two_on_one_feature":          # 700 is added (obs 2 with the target), 701 has 2: not greater, 700 goes
            h.see(0, p, d=10, pid=700), h.see(2, p, d=11, pid=701), h.see(3, p, d=11, pid=701)
            ids, kinds = [700, 701], [("add", -1), ("kept_candidate", 700)]
        elif name == "two_on_one_feature_first_stays":
            h.see(0, p, d=10, pid=700), h.see(1, p, d=10, pid=700), h.see(2, p, d=10, pid=700), h.see(4, p, d=11, pid=701)
            ids, kinds = [700, 701], [("add", -1), ("kept_org", 700)]
        else:
            h.see(0, p, d=10, pid=700), h.see(2, p, d=11, pid=701), h.see(3, p, d=11, pid=701), h.see(4, p, d=12, pid=702)
            ids, kinds = [700, 701, 702], [("add", -1), ("kept_candidate", 700), ("kept_org", 701)]
    elif name == "two_features_one_org":
        p, q = h.point(150, 350), h.point(500, 350)
        h.see(T, p, d=6, pid=900), h.see(T, q, d=7, pid=900)
        h.see(0, p, d=6), h.see(1, p, d=6), h.see(0, q, d=7)
        ids, kinds = [100 + p, 100 + q], [("kept_candidate", 900), ("add", -1)]
    elif name == "tie_by_cell_order":
        # octave 1 everywhere (level 1 or 2, radius >= 3.6): the floor range of u = 257 spans the cell columns 25 and 26;
        # feature 0 of the target sits at 258.5 (column 26), feature 1 at 254.5 (column 25), same descriptor: column 25 wins
        p = h.point(257, 240)
        h.see(0, p, d=20, octave=1, ref=0)
        h.see(T, p, d=21, octave=1, shift=1.5, **empty), h.see(T, p, d=21, octave=1, shift=-2.5, **empty)
        ids, kinds = [100 + p], [("add", -1)]
    elif name == "round_not_floor":
        # u = 255, radius <= 3.6: the floor range is column 25 alone; the feature at 256.5 is inside the radius, but its
        # ROUNDED column is 26
        p = h.point(255, 100)
        h.see(0, p, d=2), h.see(T, p, d=2, shift=1.5, **empty)
        ids, kinds = [100 + p], []
    elif name == "not_a_multiple_of_64":
        NK = 70
        p = h.point(330, 260)
        h.filler(T, 66)
        h.see(0, p, d=9), h.see(2, p, d=9), h.see(T, p, d=9, **empty)      # feature 66 of the target
        q = h.point(50, 50)
        h.see(1, q, d=4), h.see(T, q, d=4, pid=900), h.see(T, q, d=30, pid=900, shift=40.0)
        ids, kinds = [100 + p, 100 + q], [("add", -1), ("kept_candidate", 900)]
    else:
        raise ValueError(name)
    for k in range(7):          # every key-frame holds something (a pose, a record)
        h.see(k, h.point(600, 20 + 60 * k, T=k), d=1, pid=990 + k)
    return dict(script=h.prepared(), fuse=(T, ids), kinds=kinds, NK=NK)


HAND_CASES = ("add", "obs_greater", "obs_equal", "obs_smaller", "holder_overlap", "held_and_repeated", "two_on_one_feature",
              "two_on_one_feature_first_stays", "three_on_one_feature", "two_features_one_org", "tie_by_cell_order", "round_not_floor",
              "not_a_multiple_of_64")


def counters_case(both):
    """two_on_one_feature with the candidates in the recent list -- both (the counters merge) or 700 alone (they do not): every
    key-frame (or key-frame 0 alone) is processed as it comes in, then the counters are made to differ"""
    c = hand_case("two_on_one_feature")
    script = []
    for s in c["script"]:
        script.append(s)
        if s[0] == "xy" and (both or s[1] == 0):
            script.append(("process", s[1]))
    script.append(("stats", [700, 701], [3, 5], [2, 1]))
    return dict(c, script=script, listed=[700, 701] if both else [700])


def holders_case(n_holders, K=70, NK=4):
    """K key-frames a centimetre apart.  900 is held by the target 0 and the key-frames 1 .. n_holders - 1; the candidate 500 by
    the same key-frames in a second, stereo feature and by key-frame K - 1: obs(500) is the greater, 900 is replaced -- the
    target's feature takes 500, every other holder has 500 already and loses the feature -- and 500's descriptor is chosen
    among n_holders + 1 rows"""
    rng = np.random.default_rng(7)
    h = Hand(K, spacing=0.01)
    h.pose[0] = ni.pose12(np.eye(3), (0.0, 0.0, -0.5))      # (half a metre behind the others: the predicted level is decisive)
    p = h.point(300, 220, T=0)
    h.see(0, p, pid=900)
    for k in range(1, n_holders):
        h.see(k, p, pid=900), h.see(k, p, pid=500, stereo=True)
    h.see(K - 1, p, pid=500)
    for k in range(K):
        if not h.kf[k]["ids"]:
            h.see(k, p, pid=-1, flag=0)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    for k in range(K):
        h.desc[k] = [ni.flip_bits(rng, base, int(rng.integers(0, 6))) for _ in h.desc[k]]
    return dict(script=h.prepared(), fuse=(0, [500]), K=K, NK=NK, n_holders=n_holders)


def graph_case(bad_first=False, K=14, n_shared=30):
    """K key-frames that all share map points (more than 10 neighbours each), in different numbers so that the ordered lists
    differ; current = K - 1.  -> (script, current)"""
    h = Hand(K, spacing=0.02)
    pts = [h.point(40 + 18 * (i % 30), 40 + 30 * (i // 30), T=0) for i in range(n_shared + K)]
    for k in range(K):
        for i in range(n_shared + (k * 5) % K):
            h.see(k, pts[i], d=i % 7)
    script = h.prepared(updates=None)
    current = K - 1
    if bad_first:
        m = run_model(script)
        script = script + [("bad", m.conn.ordered[current][0])]
    return script, current


# ---- the seeded scene -------------------------------------------------------------------------------------------------------
K_SCENE, N_FEAT = ui.K_SCENE, ui.N_FEAT
SCENE_CAPS, SCENE_RECENT, SCENE_CANDIDATES = ui.SCENE_CAPS, ui.SCENE_RECENT, 4096
SEED = 3
# map points taken out of the seeded scene (their features come in without a map point), found on the CPU by running the
# model: the inserted candidates one of whose float gates decided with less than the margins tests/test_fuse_ref.py asks for
DROP = frozenset({159, 276, 369, 532})


# features (key-frame, feature) that come in with a random descriptor of their own, so that create_map_points matches nothing to them:
# the ends of the created map points one of whose float gates decided with less than three times the margins, found on the CPU
# the same way (their positions are the triangulation's, which the device computes in float: hence the factor)
# To make DROP and SCRAMBLE again (after a change to the triangulation or the solver moves the margins): run seeded_chain(drop=...,
# scramble=...) on a ModelRunner with m.margin, m.level_margin = 3e-4, 3e-3, the "ba" steps solved by oracle_lib.local_ba and
# applied with m.apply, "cullkf" by m.cull, keeping the rows of m.np_result["created"] after every create step; then read
# m.weak: an id below FIRST_ID goes into DROP; for a created id with row (neighbour, idx1, idx2, id) of create(current), add
# (current, idx1) and (neighbour, idx2) to SCRAMBLE; repeat until m.weak is empty (two or three rounds).
SCRAMBLE = frozenset({(6, 35), (7, 166), (8, 100), (8, 212), (8, 249), (9, 131), (9, 144), (10, 0), (10, 177), (10, 204)})
PLANT_IDS = (9001, 9002)


def _plant(inserts):
    """the last of the given key-frames gets two map points of its own, PLANT_IDS, both AT the place of a map point p that leaves the scene
    (its features come in empty): two candidates for one feature of the first target that sees the place -- a chain of two --
    and, the last key-frame holding both, a cleared feature.  They take p's position row and descriptor and sit in two
    features without a map point whose octave is p's.  -> p"""
    last = inserts[-1]
    ids, flags, octave, extra = last[1], last[2], last[3], last[6]
    for i, p in enumerate(ids):
        if not (flags[i] & 1) or p < 0 or p >= FIRST_ID or p in DROP or octave[i] > 3:
            continue
        if not all(p in s[1] for s in inserts[-4:-1]):
            continue
        free = [j for j in range(len(ids)) if ids[j] < 0 and octave[j] == octave[i]][:2]
        if len(free) < 2:
            continue
        for j, new in zip(free, PLANT_IDS):
            ids[j], flags[j] = new, 1
            extra["points"][j], extra["desc"][j], extra["refs"][j] = extra["points"][i], extra["desc"][i], -1
        return p
    raise ValueError("no place for the plant")


def _noise(k, i):
    """a descriptor of its own for feature i of key-frame k: nothing matches it"""
    return np.random.default_rng(1000 * k + i).integers(0, 256, 32, dtype=np.uint8)


def seeded_chain(seed=SEED, drop=None, scramble=None):
    """point_upkeep_inputs.seeded_chain with search_in_neighbors between create and ba for the last three key-frames, the plant
    of _plant, and DROP / SCRAMBLE"""
    drop, scramble = set(DROP if drop is None else drop), SCRAMBLE if scramble is None else scramble
    chain = []
    for s in ui.seeded_chain(seed):
        if s[0] == "insert":
            extra = dict(s[6])
            extra.update(points=np.array(extra["points"]), desc=np.array(extra["desc"]), refs=list(extra["refs"]))
            s = ("insert", list(s[1]), list(s[2]), list(s[3])) + s[4:6] + (extra,)
        chain.append(s)
    inserts = [s for s in chain if s[0] == "insert"]
    last = len(inserts) - 3          # the first key-frame with a fuse: no solver has moved the map yet, the rows are current
    drop.add(_plant(inserts[:last + 1]))
    out, k = [], -1
    for s in chain:
        if s[0] == "insert":
            k += 1
            for i, p in enumerate(s[1]):       # create_map_points has one BoW node in twelve to work on: few created points
                if p < 0 and s[6]["nodes"][i] % 12:
                    s[6]["desc"][i] = _noise(k, i)
            for kk, i in scramble:
                if kk == k:
                    s[6]["desc"][i] = _noise(k, i)
            for i, p in enumerate(s[1]):
                if p in drop:
                    s[1][i], s[2][i], s[6]["refs"][i] = -1, 0, -1
        out.append(s)
        if s[0] == "create":
            if s[1] == last:
                out += [("refresh", list(PLANT_IDS)), ("descriptors", list(PLANT_IDS))]
            out.append(("neighbors", s[1]))
    return out


def capacity_candidates_case():
    """three candidates pass the gates where a step takes two; one of them would match"""
    h, T = Hand(), T_HAND
    a, b, c = h.point(100, 100), h.point(300, 100), h.point(500, 100)
    h.see(0, a, d=5), h.see(T, a, d=5, flag=0, pid=-1)
    h.see(0, b, d=6), h.see(1, c, d=7)                      # the target has no feature there
    for k in range(7):
        h.see(k, h.point(600, 20 + 60 * k, T=k), d=1, pid=990 + k)
    return dict(script=h.prepared(), fuse=(T, [100 + a, 100 + b, 100 + c]), NK=64)


def composed_case():
    """seven key-frames that share 16 map points (everybody is in everybody's ordered list); point `a` is held by the current
    key-frame 6 and by key-frame 0, the key-frames 1 .. 5 see it in an empty feature: an add in the first step of each that matches (a
    later visit of the same key-frame finds the point held).  -> (script, current, id of a)"""
    h = Hand()
    link = [h.point(60 + 30 * i, 400) for i in range(16)]
    a = h.point(250, 150)
    for k in range(7):
        for p in link:
            h.see(k, p, d=3)
    h.see(6, a, d=12), h.see(0, a, d=12)
    for k in (1, 2, 3, 4, 5):
        h.see(k, a, d=12, flag=0, pid=-1)
    return h.prepared(updates=None), 6, 100 + a


def carriers_case(n=1025, NK=2):
    """n key-frames a millimetre apart.  900 is carried by every one of them, the target 0 included (n carriers, one more than a
    replace collects); the candidate 500 by the key-frames 1 and 2 in their second feature: the match is counted, the replace
    is left undone"""
    h = Hand(n, spacing=0.001)
    h.pose[0] = ni.pose12(np.eye(3), (0.0, 0.0, -0.5))
    p = h.point(300, 220, T=0)
    for k in range(n):
        h.see(k, p, pid=900)
    h.see(1, p, pid=500), h.see(2, p, pid=500)
    return dict(script=h.script(updates=()) + [("refresh", [500, 900])], fuse=(0, [500]), K=n, NK=NK, n=n)
