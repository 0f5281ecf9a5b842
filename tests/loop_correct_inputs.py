"""Inputs of the loop-correction tests (test infrastructure): the models, the script runner, and the hand-made stores shared by
the model's CPU tests (tests/test_loop_correct_ref.py) and the device's GPU tests (tests/test_gpu_loop_correct.py).

A script is a list of the steps of tests/pose_graph_store_inputs.py and one more, which stands for what a fusion does to a
key-frame between propagate_loop and loop_connections:
  ("setids", k, ids, flags)      the ids and flags of key-frame k replaced
The hand stores are pose_graph_store_inputs.Scene's, at most 8 key-frames of NK_HAND features on HAND_POSES (the last three turn
by about 175 degrees about x, y and z: the stored pose's quaternion comes through each of Eigen's three off-branches)."""
import math

import numpy as np

import loop_correct_ref as lr
import loop_fuse_inputs as lfi
import pose_graph_store_inputs as pi
import pose_graph_store_ref as pr

NK_HAND = pi.NK_HAND
LC_CAPS = (8, 256, 64)


class Model(lr.LoopCorrectModel, pr.PoseGraphModel):
    """the loop correction on the pose graph's store model"""


class ChainModel(lr.LoopCorrectModel, lfi.ChainModel):
    """the loop correction, the loop fusion and the pose graph's window on one store, for the chains"""


class ModelRunner(pi.ModelRunner):
    def __init__(self, caps=pi.CAPS, max_edges=pi.MAX_EDGES, exp=None, log=None, lc_caps=LC_CAPS):
        self.m = Model(pi.CAM6, pi.SF, pi.FIRST_ID, caps, exp, log, max_edges)
        self.m.enable_loop_correct(*lc_caps)

    def step(self, s):
        if s[0] == "setids":
            self.m.update_points(s[1], s[2], s[3])
        else:
            super().step(s)


def run_model(script, **kw):
    r = ModelRunner(**kw)
    for s in script:
        r.step(s)
    return r.m


def loop_sim3(T12, scale=1.0, angle=math.radians(6.0), shift=(0.25, -0.1, 0.15), stretch=1.0001):
    """a loop Sim3 for a key-frame whose pose is T12: its pose turned by `angle` and moved by `shift` (0.3 m), the translation
    multiplied by the scale as a Sim3 holds it, the quaternion deliberately not of unit length"""
    R = pi.rot((0.3, 1.0, -0.2), angle) @ np.asarray(T12[:9]).reshape(3, 3)
    S = pr.from_pose(pi.pose12(R, np.asarray(T12[9:]) + np.asarray(shift)))
    return [stretch * c for c in S[:4]] + [scale * c for c in S[4:7]] + [scale]


# ---- the propagation's hand store -------------------------------------------------------------------------------------------
G = list(range(1000, 1016))       # 16 points the key-frames 2, 3, 5, 6, 7 share: every one of them is in every other's list
G_OUT = [p for p in G if p % 4 == 2]   # ... of which key-frame 1 (outside the set) holds four, as their reference key-frame
H5 = list(range(1100, 1106))      # held by 5, 7 and key-frame 0 (outside): corrected through 5, at position 2
DUP = 1200                        # in two features of key-frame 3, and in key-frame 4 (outside)
OWN = {k: list(range(1300 + 10 * k, 1300 + 10 * k + 3)) for k in range(8)}
CURR = 6
CORR = [2, 3, 5, 6, 7]


def _g_ref(p):
    return (2, 5, 1, -1)[p % 4]   # the correcting key-frame itself, one above it, one outside the set, unknown


def propagate_scene(bad=(), poses=None, dup_shift=0.01):
    """-> script.  Key-frame 6 is current; its ordered list is 2, 3, 5, 7 in some order.  The second feature of key-frame 3 that
    carries DUP stores a row `dup_shift` off the first, so that WHICH row is read shows"""
    s = pi.Scene(pi.HAND_POSES)
    for k in range(8):
        s.see(k, OWN[k], k)
    for k in CORR:
        s.see(k, G, _g_ref)
    s.see(1, G_OUT, _g_ref)
    s.see(5, H5, lambda p: 7 if p % 2 else 0), s.see(7, H5, lambda p: 7 if p % 2 else 0), s.see(0, H5, lambda p: 7 if p % 2 else 0)
    s.see(3, [DUP], 4), s.see(4, [DUP], 4), s.see(3, [DUP], 4)
    script = s.script(poses=poses)
    for st in script:
        if st[0] == "insert" and st[1].count(DUP) == 2:
            f = len(st[1]) - 1 - st[1][::-1].index(DUP)
            st[6]["points"][f] = st[6]["points"][f] + dup_shift
    return script + [("bad", k) for k in bad]


def lonely_scene():
    """two key-frames that share nothing: the current one's ordered list is empty"""
    s = pi.Scene(pi.HAND_POSES[:2])
    s.see(0, range(1000, 1010), 0), s.see(1, range(1100, 1110), 1)
    return s.script()


# ---- the loop connections' hand store ---------------------------------------------------------------------------------------
C_G = list(range(2000, 2016))     # 16 points the key-frames 4, 5, 6, 7 share
C_57 = [2020, 2021]               # 5 and 7 only: 5 comes first in 7's list (18 against 16, 16)
C_O15 = list(range(2100, 2115))   # 6 and 2: key-frame 2, outside the set, is in 6's list before the loop
C_X3 = [2200, 2201, 2202]         # 6 and 1: weight 3, in 6's map and not in its list -- until the list becomes the whole map
C_40 = [2300, 2301]               # 4 and 0: weight 2
C_F100 = list(range(2400, 2500))  # key-frame 0's own: what the fusion gives key-frame 7 (weight 100: a family-A edge of the pose graph)
C_T3 = [2550, 2551, 2552]         # key-frame 3's own: what the fusion gives key-frame 7 below the threshold
C_OWN7 = list(range(2600, 2703))  # key-frame 7's own features, which the fusion rewrites
C_OWN5 = [2800]                   # a feature of key-frame 5 that the fusion gives a point of 6 and 2
C_CURR = 7
C_LIST = [5, 6, 4, 7]
C_ROWS = {4: [0], 5: [2], 6: [], 7: [0, 3]}   # worked out by hand (tests/test_loop_correct_ref.py walks through it)


def connections_scene():
    s = pi.Scene(pi.HAND_POSES)
    for k in (4, 5, 6, 7):
        s.see(k, C_G, 4)
    s.see(5, C_57, 5), s.see(7, C_57, 5)
    s.see(6, C_O15, 2), s.see(2, C_O15, 2)
    s.see(6, C_X3, 1), s.see(1, C_X3, 1)
    s.see(4, C_40, 0), s.see(0, C_40, 0)
    s.see(0, C_F100, 0), s.see(3, C_T3, 3)
    s.see(7, C_OWN7, 7), s.see(5, C_OWN5, 5)
    return s


def fusion_steps(s):
    """what stands for searchAndFuse: 7 takes a hundred points of key-frame 0 and three of key-frame 3; 5 takes a point 6 and 2 share
    (which CHANGES the weight 5 - 6); 4 loses everything (its update finds no connection)"""
    ids7 = [p for p in s.kf[7]["ids"] if p not in C_OWN7] + C_F100 + C_T3
    ids5 = [C_O15[0] if p in C_OWN5 else p for p in s.kf[5]["ids"]]
    n4 = len(s.kf[4]["ids"])
    return [("setids", 7, ids7, [1] * len(ids7)), ("setids", 5, ids5, [1] * len(ids5)), ("setids", 4, list(s.kf[4]["ids"]), [0] * n4)]


# ---- the seeded 12 x 256 scene of the loop fusion's chain -------------------------------------------------------------------
CHAIN_LC_CAPS = (12, 2048, 64)
CHAIN_TH = lfi.TH


def chain_scw(m, curr):
    """the loop Sim3 of the seeded chain: the current key-frame's pose moved by a few centimetres and half a degree, so that the
    fusion behind it still finds its matches"""
    return loop_sim3(m.store[curr]["pose"], 1.0, math.radians(0.5), (0.03, -0.01, 0.02))


# the float64 model's worst error against the numpy.longdouble matrix formulation over the Sim3s, poses and moved points of the
# hand stores, measured and checked by tests/test_loop_correct_ref.py; the device gets ten times that
MODEL_LONGDOUBLE_WORST = 1.5e-14   # measured 1.48e-14


# ---- the chains: the same steps on the model for the CPU checks and beside the device ------------------------------------------
LOOP_SCENE = "n255"               # loop_sim3_inputs' accepted scene with 255 shared points: the fusion lifts curr - match above 100
LOOP_LC_CAPS = (8, 1024, 64)
SEEDED_MATCH = 10                 # the key-frame seeded_old_keyframe appends behind the scene's first ten
SEEDED_OLD_IDS = list(range(2000, 2120))   # (the scene's ids are below 575, created ones start at fuse_inputs.FIRST_ID)


def scene_model(sc, exp=None, log=None):
    """loop_sim3_inputs' scene as a ChainModel, every layer enabled as tests/test_gpu_loop_correct.py enables it on the device"""
    import loop_sim3_inputs as ls
    m = ChainModel(ls.CAM6, ls.SF, 50000, ls.BA_CAPS, exp, log, ls.MAX_RECENT)
    m.enable_fuse(ls.BOUNDS, 1024)
    m.enable_loop_fuse(LOOP_LC_CAPS[0], sc["caps"]["max_loop_points"])
    m.enable_loop_correct(*LOOP_LC_CAPS)
    for k, kf in enumerate(sc["store"]):
        m.insert(kf["ids"], kf["flags"], kf["bad"], kf["desc"], kf["angle"], kf["nodes"])
        m.set_keypoints(k, kf["octave"], kf["depth"], kf["uright"])
        m.set_xy(k, np.stack([kf["x"], kf["y"]], 1))
        if kf["pose"] is not None:
            m.set_pose(k, kf["pose"])
        m.set_map_side(k, kf["points"], kf["normals"], kf["min_dist"], kf["max_dist"])
        m.store[k]["pdesc"] = np.array(kf["point_desc"], np.uint8).reshape(-1, 32)
        m.set_point_refs(k, scene_refs(kf, k))
    m.update_connections(list(range(len(sc["store"]))))
    return m


def scene_refs(kf, k):
    """the reference key-frame of a scene's feature: its own key-frame where it holds a point, else unknown"""
    live = np.asarray(kf["flags"]) & 1
    return np.full(len(kf["ids"]), k, np.int32) * live - (1 - live)


def seeded_old_keyframe(m):
    """-> steps.  The loop side of the seeded chain: one more key-frame, number SEEDED_MATCH, with 120 map points of its own and
    no connection (it is never updated), so that it lies outside the current key-frame's currConnect"""
    assert len(m.store) == SEEDED_MATCH and not any(p in SEEDED_OLD_IDS for kf in m.store for p in kf["ids"])
    n = len(SEEDED_OLD_IDS)
    rng = np.random.default_rng(77)
    pts = np.stack([rng.uniform(-3, 7, n), rng.uniform(-2, 2, n), rng.uniform(4, 9, n)], 1)
    xy = np.stack([np.float32(20.0) + np.float32(5.0) * np.arange(n, dtype=np.float32), np.full(n, np.float32(200.0))], 1).astype(np.float32)
    T = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, -2.0, 0.1, 0.3]
    return [("insert", list(SEEDED_OLD_IDS), [1] * n, [0] * n, [-1.0] * n, [-1.0] * n,
             dict(desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), angle=[0.0] * n, nodes=[0] * n, points=pts, refs=[SEEDED_MATCH] * n)),
            ("pose", SEEDED_MATCH, T), ("xy", SEEDED_MATCH, xy)]


def seeded_block(m, curr, n=110):
    """the fused block of the seeded chain: ("setids", curr, ids, flags) that gives `curr`, in features without a map point, n live
    points of key-frame SEEDED_MATCH that curr does not hold -- a connection of weight >= 100 to a key-frame outside currConnect"""
    kf = m.store[curr]
    ids, flags = list(kf["ids"]), list(kf["flags"])
    free = [f for f in range(len(ids)) if not (flags[f] & 1)]
    give = [p for p in m.live_ids(SEEDED_MATCH) if m.observation(curr, p) < 0][:n]
    assert len(free) >= n and len(give) == n, (len(free), len(give))
    for f, p in zip(free, give):
        ids[f], flags[f] = int(p), flags[f] | 1
    return ("setids", curr, ids, flags)


def seeded_loop_ids(m, corr0, n=lfi.CHAIN_LOOP_POINTS):
    """the first n live points of the store that key-frame corr0 does not hold"""
    ids = []
    for k in range(len(m.store)):
        for p in m.live_ids(k):
            if p not in ids and m.observation(corr0, p) < 0:
                ids.append(int(p))
    return ids[:n]


def model_chain(m, curr, Scw, ids, match, block=None):
    """propagate_loop -> search_and_fuse -> [the fused block] -> loop_connections -> pg_window on model m
    -> (the propagate's lists, the rows, the window)"""
    L = m.propagate_loop(curr, Scw)
    assert L is not None, m.lc_record
    m.search_and_fuse(L["corr_kf"], L["S_corr"], ids, CHAIN_TH)
    if block is not None:
        blk = block(m) if callable(block) else block
        m.update_points(blk[1], blk[2], blk[3])
    rows = m.loop_connections()
    assert rows is not None, m.lc_record
    return L, rows, m.pg_window(curr, match, m.lc_inputs())
