"""Inputs of the map-point upkeep tests (test infrastructure): the script format, its runner on the model
(tests/point_upkeep_ref.py), the hand-made scripts shared by the model's CPU tests and the device's GPU tests, and the seeded
12 x 256 scene with its chain.

A script is a list of the steps of tests/local_ba_inputs.py and four more:
  ("process", k)                     process_new_keyframe
  ("descriptors", ids)               compute_descriptors
  ("stats", ids, visible, found)     add_point_stats
  ("cullmp", current)                cull_map_points
Descriptors of the hand-made stores are bits(n): the first n bits set, so that the Hamming distance of bits(a) and bits(b) is
|a - b| and a median can be worked out by hand."""
import numpy as np

import local_ba_inputs as li
import new_points_inputs as ni
from point_upkeep_ref import UpkeepModel

f32 = np.float32
NK_HAND = 16
CAPS = li.CAPS
CAM6, SF, FIRST_ID = ni.CAM6, ni.SF, ni.FIRST_ID
MAX_RECENT = 32


class ModelRunner(li.ModelRunner):
    def __init__(self, caps=CAPS, first_point_id=FIRST_ID, exp=None, log=None, max_recent=MAX_RECENT):
        self.m = UpkeepModel(CAM6, SF, first_point_id, caps, exp, log, max_recent)

    def step(self, s):
        m = self.m
        if s[0] == "process":
            m.process_new_keyframe(s[1])
        elif s[0] == "descriptors":
            m.compute_descriptors(s[1])
        elif s[0] == "stats":
            m.add_point_stats(s[1], s[2], s[3])
        elif s[0] == "cullmp":
            m.cull_map_points(s[1])
        else:
            super().step(s)


def run_model(script, caps=CAPS, **kw):
    r = ModelRunner(caps, **kw)
    for s in script:
        r.step(s)
    return r.m


def bits(n):
    d = np.zeros(256, np.uint8)
    d[:n] = 1
    return np.packbits(d)


class Hand(li.Hand):
    """local_ba_inputs.Hand with a descriptor per feature: see(..., d=n) gives the feature bits(n)"""

    def __init__(self, K, W=None):
        super().__init__(K, W)
        self.desc = [[] for _ in range(K)]

    def see(self, k, p, d=0, **kw):
        i = super().see(k, p, **kw)
        self.desc[k].append(bits(d))
        assert len(self.kf[k]["ids"]) <= NK_HAND or self.big
        return i

    def script(self, poses=None, updates=()):
        out = []
        for s in super().script(poses, updates):
            if s[0] == "insert":
                k = sum(1 for x in out if x[0] == "insert")
                s = s[:6] + (dict(s[6], desc=np.array(self.desc[k], np.uint8).reshape(-1, 32)),)
            out.append(s)
        return out


# ---- computeDescriptor ------------------------------------------------------------------------------------------------------
# id = 100 + world point.  `want`: the id's winning (key-frame, feature) worked out by hand, None: unchanged
def descriptor_case():
    h = Hand(6)
    want = {}
    h.see(0, 0, d=7), want.update({100: (0, 0)})                                   # N = 1
    h.see(0, 1, d=10), h.see(2, 1, d=30), want.update({101: (0, 1)})               # N = 2: entry 0 of both rows is 0, the first wins
    # N = 3, rows 0 / 10 / 30: medians (entry 1) 10, 10, 20 -- two equal medians, the first wins
    h.see(0, 2, d=0), h.see(2, 2, d=10), h.see(3, 2, d=30), want.update({102: (0, 2)})
    # N = 4 (the even case takes sorted entry 1), rows 0 / 40 / 50 / 60: medians 40, 10, 10, 10 -- key-frame 2's row
    h.see(0, 3, d=0), h.see(3, 3, d=50), h.see(4, 3, d=60), want.update({103: (2, h.see(2, 3, d=40))})
    # a bad holder (key-frame 1) is left out: rows 100 (bad) / 0 / 90 / 95 have medians 5, 90, 5, 5 and would elect the bad one's
    # own row; without it rows 0 / 90 / 95 have medians 90, 5, 5: key-frame 3's
    h.see(1, 4, d=100), h.see(2, 4, d=0), h.see(4, 4, d=95), want.update({104: (3, h.see(3, 4, d=90))})
    h.see(1, 5, d=50), want.update({105: None})                                    # every holder bad: unchanged
    want.update({777: None})                                                       # an id nobody holds
    # an id in two features of key-frame 2, the lower one (bits 20) its observation; N = 2 with key-frame 4: the first wins, and
    # both features of key-frame 2 carry the result
    i = h.see(2, 6, d=20)
    h.see(2, 6, d=200), h.see(4, 6, d=60), want.update({106: (2, i)})
    return dict(script=h.script() + [("bad", 1)], want=want, ids=[100, 101, 102, 103, 104, 105, 777, 106, 103, 100, 103])


def holders_case(K, counts, NK=4, seed=3):
    """K key-frames without poses; point 100 + j is held by the key-frames 0 .. counts[j] - 1, random descriptors (no key-frame
    needs a pose: compute_descriptors reads none)"""
    rng = np.random.default_rng(seed)
    script = []
    for k in range(K):
        ids = [100 + j for j, c in enumerate(counts) if k < c]
        n = len(ids)
        script.append(("insert", ids, [1] * n, [0] * n, [-1.0] * n, [-1.0] * n,
                       dict(desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), angle=[0.0] * n, nodes=[0] * n)))
    return dict(script=script, ids=[100 + j for j in range(len(counts))], NK=NK, K=K)


# ---- processNewKeyFrame -----------------------------------------------------------------------------------------------------
def process_base(bad=None, erase=None, poses=None):
    """six key-frames, current = 5.  Points 0 .. 3: key-frames 3, 4 and 5 (tracked); 4: key-frames 1 and 5 (tracked through one
    other holder); 5: key-frames 2 and 5; 6 .. 8: key-frame 5 alone (created with it), 7 in two features; 9: key-frame 5 with bit 0
    clear although key-frame 3 holds it; 10: key-frame 4 alone.  `erase` happens before key-frame 5 comes in"""
    h = Hand(6)
    for k in (3, 4):
        for p in range(4):
            h.see(k, p, d=10 * p + k, stereo=(p + k) % 2 == 0, octave=p % 3, ref=3)
    h.see(1, 4, d=3, ref=1), h.see(2, 5, d=9, stereo=True, ref=2), h.see(3, 9, d=1), h.see(4, 10, d=2)
    for p in range(4):
        h.see(5, p, d=10 * p + 4, octave=1)
    h.see(5, 4, d=60), h.see(5, 5, d=70, stereo=True)
    h.see(5, 6, d=80, stereo=True), h.see(5, 7, d=81, stereo=True), h.see(5, 8, d=82), h.see(5, 7, d=83)
    h.see(5, 9, d=90, flag=0), h.see(5, 2, d=99, octave=2)      # and tracked point 2 in a second feature
    s, out = h.script(poses), []
    for x in s:
        if x[0] == "insert" and len(x[1]) == len(h.kf[5]["ids"]) and sum(1 for y in out if y[0] == "insert") == 5:
            out += ([("bad", bad)] if bad is not None else []) + ([("erase", erase)] if erase is not None else [])
        out.append(x)
        if x[0] == "xy" and x[1] < 5:
            out.append(("process", x[1]))      # every earlier key-frame has been processed as it came in
    return out


PROCESS_BEFORE = 8  # listed before key-frame 5 comes in: points 4, 5, 0 .. 3, 9, 10 with the key-frames 1, 2, 3, 3, 4
PROCESS_ALONE = 3   # points 6, 7, 8


def process_cases():
    c = {}
    c["tracked_and_created_with"] = process_base() + [("process", 5)]
    c["other_holder_bad"] = process_base(bad=1) + [("process", 5)]           # point 4: still tracked; key-frame 1's row is left out
    c["other_holder_erased"] = process_base(erase=2) + [("process", 5)]      # point 5: created with key-frame 5
    c["current_without_a_pose"] = process_base(poses=[0, 1, 2, 3, 4]) + [("process", 5)]
    c["current_erased"] = process_base() + [("erase", 5), ("process", 5)]
    c["twice"] = process_base() + [("process", 5), ("process", 5)]
    return c


# ---- cullingMapPoints -------------------------------------------------------------------------------------------------------
def cull_script():
    """seven key-frames, every one processed as it comes in.  first_kf = 0: points 0 .. 7, = 1: points 8 .. 12, = 2: point 13.
      0  obs 4 (0 stereo, 1 mono, 3 mono)    1  obs 3 (0 stereo, 1 mono)      2  ratio 1/4       3  ratio 1/5
      4  obs 5, twice in key-frame 3          5  ratio 1/5, twice in key-frame 1
      6, 7 obs 5                              8  obs 3 (1 stereo, 2 mono)      9  obs 4 (1 stereo, 2 mono, 3 mono)
      10 obs 5                               13  key-frame 2 alone, which is then erased: a dead entry
    key-frame 2 holds 13 and, like the others, the link points 20 .. 22 (so that the erase kills nothing else)"""
    h = Hand(7)
    link = lambda k: [h.see(k, p, d=p, stereo=True) for p in (20, 21, 22)]
    h.see(0, 0, stereo=True), h.see(0, 1, stereo=True)
    for p in (2, 3, 5):
        h.see(0, p, stereo=True)
    h.see(0, 4, stereo=True), h.see(0, 6, stereo=True), h.see(0, 7, stereo=True), link(0)
    h.see(1, 0), h.see(1, 1), h.see(1, 5), h.see(1, 5, d=9), h.see(1, 4, stereo=True), h.see(1, 6, stereo=True), h.see(1, 7, stereo=True)
    h.see(1, 8, stereo=True), h.see(1, 9, stereo=True), h.see(1, 10, stereo=True), link(1)
    h.see(2, 8), h.see(2, 9), h.see(2, 10, stereo=True), h.see(2, 13), link(2)
    h.see(3, 0), h.see(3, 9), h.see(3, 4), h.see(3, 4, d=5), h.see(3, 6), h.see(3, 7), h.see(3, 10), link(3)
    for k in (4, 5, 6):
        link(k)
    s, out = h.script(), []
    for x in s:
        out.append(x)
        if x[0] == "xy":
            out.append(("process", x[1]))
    return out + [("stats", [102, 103, 105, -1, 999, 103], [3, 2, 4, 7, 7, 2], [0, 0, 0, 7, 7, 0])]


CULL_FIRST = {100: 0, 101: 0, 102: 0, 103: 0, 104: 0, 105: 0, 106: 0, 107: 0, 108: 1, 109: 1, 110: 1, 113: 2}


def cull_want(current, dead):
    """the branch of every entry worked out by hand (DEAD .. KEPT = 1 .. 5)"""
    obs = {100: 4, 101: 3, 102: 2, 103: 2, 104: 5, 105: 3, 106: 5, 107: 5, 108: 3, 109: 4, 110: 5, 113: 1}
    if dead:   # key-frame 2 erased: 113 and 108 (obs 2 without it) have died, 109 and 110 have lost an observation
        obs.update({109: 3, 110: 3})
    out = {}
    for p, first in CULL_FIRST.items():
        if p in (108, 113) and dead:
            out[p] = 1
        elif p in (103, 105):
            out[p] = 2
        elif current > first + 2 and obs[p] <= 3:
            out[p] = 3
        elif current > first + 3:
            out[p] = 4
        else:
            out[p] = 5
    return out


# ---- the seeded scene -------------------------------------------------------------------------------------------------------
K_SCENE, N_FEAT = 12, 256
SCENE_CAPS = li.SCENE_CAPS
SCENE_RECENT = 1024
SEED = 3   # chosen on the CPU (tests/test_point_upkeep_ref.py checks it): every create gate decisive, every cull branch taken


def seeded_chain(seed=SEED, K=K_SCENE, n_feat=N_FEAT, n_world=575, n_nodes=48):
    """local_ba_inputs.seeded_scene's geometry, every key-frame followed by process -> stats -> cullmp and, for the last three,
    create -> ba -> cullkf.  One mapped point in four is FLAKY: a key-frame that sees it carries its map point one time in
    three (few observations: branch 3).  The counters: one listed id in six is seen five times more and found never (branch 2),
    the others are seen and found twice; ids nobody lists and negative ones are mixed in"""
    rng = np.random.default_rng(seed)
    W = np.stack([np.sort(rng.uniform(-3, 7, n_world)), rng.uniform(-2, 2, n_world), rng.uniform(4, 9, n_world)], 1)
    Wn = W + rng.normal(0, 0.01, W.shape)
    mapped = rng.random(n_world) < 0.4
    flaky = rng.random(n_world) < 0.25
    base_d = rng.integers(0, 256, (n_world, 32), dtype=np.uint8)
    node = rng.integers(0, n_nodes, n_world)
    level = rng.integers(0, 4, n_world)
    rot0 = rng.uniform(0, 360, n_world)
    first = {}
    script, c = [], np.zeros(3)
    for k in range(K):
        c = c + (np.array([0.0, 0.02, 0.15]) if k % 3 == 2 else np.array([rng.uniform(0.25, 0.45), rng.uniform(-0.05, 0.05), 0.0]))
        T = ni.se3(rng.normal(0, 0.02, 3), c)
        seen = 25 * k + np.sort(rng.choice(300, n_feat, replace=False))
        seen = seen[rng.permutation(n_feat)]
        ids, flags, octave, depth, ur, desc, angle, nodes, xy, pts, refs = [], [], [], [], [], [], [], [], [], [], []
        for p in seen:
            pc = [T[3 * r] * W[p][0] + T[3 * r + 1] * W[p][1] + T[3 * r + 2] * W[p][2] + T[9 + r] for r in range(3)]
            has = bool(mapped[p]) and (not flaky[p] or rng.random() < 1 / 3)
            off = rng.normal(0, 0.5, 2) + (np.array([8.0, -6.0]) if has and rng.random() < 0.04 else 0.0)
            u, v, z = f32(500.0 * pc[0] / pc[2] + 320.0 + off[0]), f32(500.0 * pc[1] / pc[2] + 240.0 + off[1]), f32(pc[2])
            stereo = rng.random() < 0.33
            d = z * (f32(1.5) if rng.random() < 1 / 12 else f32(1.0))
            ids.append(int(p) if has else -1), flags.append(int(rng.choice([1, 3])) if has else 0)
            octave.append(int(level[p] + (4 if rng.random() < 0.05 else 0)))
            depth.append(float(d) if stereo else -1.0), ur.append(float(u - f32(40.0) / d) if stereo else -1.0)
            desc.append(ni.flip_bits(rng, base_d[p], int(rng.integers(0, 6))))
            angle.append(float(f32((rot0[p] + 20.0 * k + rng.uniform(-2, 2)) % 360.0)) if rng.random() < 0.9 else float(f32(rng.uniform(0, 360))))
            nodes.append(int(node[p])), xy.append((u, v))
            pts.append(Wn[p] if has else np.zeros(3))
            if has:
                first.setdefault(int(p), k)
            refs.append((first[int(p)] if p % 5 else -1) if has else -1)
        script.append(("insert", ids, flags, octave, depth, ur, dict(desc=np.array(desc, np.uint8), angle=angle, nodes=nodes,
                                                                      points=np.array(pts), refs=refs)))
        script.append(("pose", k, T))
        script.append(("xy", k, np.array(xy, f32)))
        script.append(("process", k))
        n_s = 96
        sid = np.concatenate([rng.integers(0, n_world, n_s - 16), rng.integers(FIRST_ID, FIRST_ID + 400, 12), [-1, -1, 9999, 9998]]).astype(np.int32)
        low = (sid % 6) == 0
        script.append(("stats", [int(x) for x in sid], [5 if b else 2 for b in low], [0 if b else 2 for b in low]))
        script.append(("cullmp", k))
        if k >= K - 3:
            script += [("create", k, 10), ("ba", k), ("cullkf", k, 40.0)]
    return script
