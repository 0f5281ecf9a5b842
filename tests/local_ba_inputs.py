"""Inputs of the store's local-BA tests (test infrastructure): the script format, its runner on the model
(tests/local_ba_store_ref.py), the hand-made stores shared by the model's CPU tests and the device's GPU tests, and the
seeded scene.

A script is a list of the steps of tests/new_points_inputs.py; the dict of an insert step may also carry `points` [n][3] (the
rows of the store's position column) and `refs` [n] (MapPoint::keyFrame_ref_ per feature as a key-frame number):
  ("insert", ids, flags, octave, depth, u_right, dict(desc, angle, nodes[, points, refs]))
  ("pose", k, Tcw12)  ("xy", k, xy)  ("update", [k])  ("bad", k)  ("erase", k)  ("create", current, max_neighbors)
A hand case is dict(name, script, current, caps, want): `want` = the fields of the window's record worked out by hand, and
where the case is about the write-back, `erase` = a function of the model's window giving the edges to erase with `after` =
{id: flags-bit-0 survives?} worked out by hand."""
import numpy as np

import new_points_inputs as ni
from local_ba_store_ref import EMPTY, OK, OVERFLOW, LocalBaModel

f32 = np.float32
NK_HAND = 64
CAPS = (16, 256, 1024)
CAM6, SF, FIRST_ID = ni.CAM6, ni.SF, ni.FIRST_ID


class ModelRunner:
    def __init__(self, caps=CAPS, first_point_id=FIRST_ID, exp=None, log=None):
        self.m = LocalBaModel(CAM6, SF, first_point_id, caps, exp, log)

    def step(self, s):
        m = self.m
        if s[0] == "insert":
            k = m.insert(s[1], s[2], desc=s[6]["desc"], angle=s[6]["angle"], nodes=s[6]["nodes"])
            m.set_keypoints(k, s[3], s[4], s[5])
            if "points" in s[6]:
                m.set_map_side(k, points=s[6]["points"])
            if "refs" in s[6]:
                m.set_point_refs(k, s[6]["refs"])
        elif s[0] == "update":
            m.update_connections(s[1])
        elif s[0] == "bad":
            m.set_bad(s[1])
        elif s[0] == "erase":
            m.erase_keyframe(s[1])
        elif s[0] == "pose":
            m.set_pose(s[1], s[2])
        elif s[0] == "xy":
            m.set_xy(s[1], s[2])
        elif s[0] == "create":
            m.create(s[1], s[2])
        else:
            raise ValueError(s[0])


def run_model(script, caps=CAPS, **kw):
    r = ModelRunner(caps, **kw)
    for s in script:
        r.step(s)
    return r.m


def insert_arrays(s):
    """the arrays KeyFrameStore.insert takes for an insert step"""
    a = ni.insert_arrays(s)
    if "points" in s[6]:
        a["points"] = np.ascontiguousarray(s[6]["points"], np.float64).reshape(-1, 3)
    return a


# ---- hand-made stores ---------------------------------------------------------------------------------------------------------
def world(n=48, seed=5):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-1.5, 2.5, n), rng.uniform(-1.2, 1.2, n), rng.uniform(4, 8, n)], 1)


class Hand:
    """key-frames at x = 0.3 k looking down +z; see(k, p, ...) appends the exact projection of world point p as the next
    feature of k, its map point id 100 + p, the store row P + 1e-3 k (so that WHICH holder's row a window takes shows)"""

    def __init__(self, K, W=None):
        self.W = world() if W is None else W
        self.pose = [ni.pose12(np.eye(3), (0.3 * k, 0.02 * k, 0.0)) for k in range(K)]
        self.kf = [dict(ids=[], flags=[], octave=[], depth=[], ur=[], xy=[], points=[], refs=[]) for _ in range(K)]

    def see(self, k, p, stereo=False, octave=0, flag=1, ref=-1, pid=None, shift=0.0):
        T, P, f = self.pose[k], self.W[p], self.kf[k]
        pc = [T[3 * r] * P[0] + T[3 * r + 1] * P[1] + T[3 * r + 2] * P[2] + T[9 + r] for r in range(3)]
        u, v, z = f32(500.0 * pc[0] / pc[2] + 320.0 + shift), f32(500.0 * pc[1] / pc[2] + 240.0), f32(pc[2])
        f["ids"].append(100 + p if pid is None else pid), f["flags"].append(flag), f["octave"].append(octave)
        f["depth"].append(float(z) if stereo else -1.0), f["ur"].append(float(u - f32(40.0) / z) if stereo else -1.0)
        f["xy"].append((u, v)), f["points"].append(P + 1e-3 * k), f["refs"].append(ref)
        assert len(f["ids"]) <= NK_HAND or self.big
        return len(f["ids"]) - 1

    big = False

    def filler(self, k, n):
        """n features without a map point"""
        f = self.kf[k]
        for i in range(n):
            f["ids"].append(-1), f["flags"].append(0), f["octave"].append(0), f["depth"].append(-1.0), f["ur"].append(-1.0)
            f["xy"].append((f32(10 + i % 600), f32(10 + i // 600))), f["points"].append(np.zeros(3)), f["refs"].append(-1)

    def script(self, poses=None, updates=None):
        out = []
        for k, f in enumerate(self.kf):
            n = len(f["ids"])
            out.append(("insert", list(f["ids"]), list(f["flags"]), list(f["octave"]), list(f["depth"]), list(f["ur"]),
                        dict(desc=np.zeros((n, 32), np.uint8), angle=[0.0] * n, nodes=[0] * n, points=np.array(f["points"]).reshape(n, 3),
                             refs=list(f["refs"]))))
            if poses is None or k in poses:
                out.append(("pose", k, list(self.pose[k])))
            out.append(("xy", k, np.array(f["xy"], f32).reshape(n, 2)))
        return out + [("update", [k]) for k in (range(len(self.kf)) if updates is None else updates)]


A = list(range(18))          # the points key-frames 1 .. 5 share: weight 18 >= 15, every one in every other's ordered list
B = [18, 19, 20, 21]         # key-frame 4 and key-frame 0 only
C = [22, 23, 24]             # the current key-frame alone
E4, E3, E2, E3S = 25, 26, 27, 28   # obs 4 (5, 4, 3, 2 mono), 3 (5, 4, 3), 2 (5, 4), 3 (5 stereo, 4 mono)


def base(kf0_sees=6, dup=False):
    """six key-frames, current = 5.  Key-frame 0 sees the first kf0_sees points of A (weight < 15: outside every list) and B.
    Key-frame 5's features: A with feature 0 = point 0, then C, then the E points"""
    h = Hand(6)
    for k in range(1, 6):
        for p in A:
            h.see(k, p, stereo=(p + k) % 3 == 0, octave=(p + k) % 4, ref=1 if p % 2 else -1)
    for p in A[:kf0_sees] + B:
        h.see(0, p, stereo=p % 2 == 0, ref=0)
    for p in B:
        h.see(4, p, ref=0)
    for p in C:
        h.see(5, p, stereo=p == 23, ref=5)
    for p, ks in ((E4, (5, 4, 3, 2)), (E3, (5, 4, 3)), (E2, (5, 4))):
        for k in ks:
            h.see(k, p, ref=ks[-1])
    h.see(5, E3S, stereo=True, ref=4), h.see(4, E3S, ref=4)
    if dup:   # an id in two features of one key-frame: in the current one and in key-frame 2
        h.see(5, 4, octave=2), h.see(2, 3, stereo=True)
    return h


def _edges(w, kf=None, pid=None, feature=None):
    """indices of the window's edges on key-frame kf / map point id pid / feature index"""
    sel = np.ones(len(w["e_cam"]), bool)
    if kf is not None:
        sel &= w["cam_keyframe"][w["e_cam"]] == kf
    if pid is not None:
        sel &= w["point_id"][w["e_pt"]] == pid
    if feature is not None:
        sel &= w["e_feature"] == feature
    return [int(e) for e in np.nonzero(sel)[0]]


def hand_cases():
    cases = []

    def case(name, script, want, current=5, caps=CAPS, **extra):
        cases.append(dict(name=name, script=script, current=current, caps=caps, want=want, **extra))

    nA, nB, nC = len(A), len(B), len(C)
    # points: A + C + 4 E from the current key-frame, B through key-frame 4.  Edges: A: 5 holders each + key-frame 0 on six of
    # them; B: 2 each; C: 1 each; E: 4 + 3 + 2 + 2
    n_pts = nA + nC + 4 + nB
    n_edges = 5 * nA + 6 + 2 * nB + nC + 11
    ok = dict(n_cams=6, n_local=5, n_fixed=1, n_points=n_pts, n_edges=n_edges, n_dropped=0, status=OK)
    s = base().script()
    # a fixed camera shared by many points, which is key-frame 0; points held only by `current`; first occurrences in the
    # current key-frame although key-frames 0 .. 4 hold the ids too; ref_kf = -1 on every other point of A.
    # The erases: feature 0 of the current key-frame (Q-B3's case), the reference key-frame 1 of point 1, and the E points down
    # to obs 3 (lives), 2, 1 and -- through the stereo observation -- 1 (die)
    case("a_base_fixed_kf0_and_erases", s, ok,
         erase=lambda w: _edges(w, 5, 100, 0) + _edges(w, 1, 101) + _edges(w, 2, 100 + E4) + _edges(w, 3, 100 + E3) + _edges(w, 4, 100 + E2)
         + _edges(w, 5, 100 + E3S),
         after={100: True, 101: True, 100 + E4: True, 100 + E3: False, 100 + E2: False, 100 + E3S: False}, n_feature0=1, n_dead=3)
    # two erases on one point in either order, and the erase of a point only `current` holds
    case("b_two_erases_on_one_point", s, ok,
         erase=lambda w: _edges(w, 2, 100 + E4) + _edges(w, 4, 100 + E4) + _edges(w, 5, 100 + C[0]),
         after={100 + E4: False, 100 + C[0]: False, 100 + C[1]: True}, n_feature0=0, n_dead=2)
    # key-frame 3 is bad INSIDE the ordered list: marked local, no camera, its 18 + 2 observations dropped
    case("c_bad_inside_the_list", s + [("bad", 3)], dict(ok, n_cams=5, n_local=4, n_edges=n_edges - nA - 2, n_dropped=nA + 2))
    # key-frame 0 is a bad holder OUTSIDE the list: no fixed camera
    case("d_bad_holder_outside_the_list", s + [("bad", 0)], dict(ok, n_cams=5, n_fixed=0, n_edges=n_edges - 6 - nB, n_dropped=6 + nB))
    # key-frame 0 sees all of A: it is in the list, a local camera, and constant because of its number
    case("e_kf0_in_the_list", base(kf0_sees=nA).script(), dict(ok, n_local=6, n_fixed=0, n_edges=n_edges - 6 + nA), kf0_local=True)
    # an id in two features of one key-frame: one point, one edge per key-frame, at the lower feature
    case("f_id_in_two_features", base(dup=True).script(), ok,
         erase=lambda w: _edges(w, 2, 103) + _edges(w, 5, 104), after={103: True, 104: True}, n_feature0=0, n_dead=0, dup=True)
    # a camera without a pose: local (2) or fixed (0)
    empty = dict(n_cams=0, n_local=0, n_fixed=0, n_points=0, n_edges=0, n_dropped=0, status=EMPTY)
    case("g_local_camera_without_a_pose", base().script(poses=[0, 1, 3, 4, 5]), empty, sticky=1)
    case("h_fixed_camera_without_a_pose", base().script(poses=[1, 2, 3, 4, 5]), empty, sticky=1)
    case("i_current_without_a_pose", base().script(poses=[0, 1, 2, 3, 4]), empty, sticky=1)
    case("j_current_erased", s + [("erase", 5)], empty, sticky=1)
    # each capacity exceeded by one: the true counts, nothing else
    over = dict(ok, status=OVERFLOW)
    case("k_one_camera_too_many", s, over, caps=(5, CAPS[1], CAPS[2]), sticky=4)
    case("l_one_point_too_many", s, over, caps=(CAPS[0], n_pts - 1, CAPS[2]), sticky=4)
    case("m_one_edge_too_many", s, over, caps=(CAPS[0], CAPS[1], n_edges - 1), sticky=4)
    case("n_capacities_met_exactly", s, ok, caps=(6, n_pts, n_edges))
    return cases


def big_case(NK=1100):
    """three key-frames of NK features (more than a workgroup has threads): 300 shared points spread over the whole feature
    range, the rest without a map point"""
    W = world(300, seed=9)
    h = Hand(3, W)
    h.big = True
    rng = np.random.default_rng(3)
    for k in range(3):
        slots = set(int(x) for x in rng.choice(NK, 300, replace=False))
        order = [int(x) for x in rng.permutation(300)]
        for i in range(NK):
            if i in slots:
                p = order.pop()
                h.see(k, p, stereo=(p + k) % 4 == 0, octave=p % 3, ref=k if p % 5 else -1)
            else:
                h.filler(k, 1)
    return dict(name="o_more_features_than_a_workgroup", script=h.script(), current=2, caps=(4, 512, 2048),
                want=dict(n_cams=3, n_local=3, n_fixed=0, n_points=300, n_edges=900, n_dropped=0, status=OK), NK=NK)


def perturbation(w, seed=1):
    """a solver's result made by hand: poses moved by about a centimetre and half a degree, points by a centimetre"""
    rng = np.random.default_rng(seed)
    return w["poses"] + rng.normal(0, 0.01, w["poses"].shape), w["points"] + rng.normal(0, 0.01, w["points"].shape)


def mask(w, edges):
    m = np.zeros(len(w["e_cam"]), np.uint8)
    m[list(edges)] = 1
    return m


# ---- the seeded scene ---------------------------------------------------------------------------------------------------------
def seeded_scene(seed, K=12, n_feat=256, n_world=575, n_nodes=48):
    """new_points_inputs.random_scene with a map side: the points that have map points already carry their world position
    (a centimetre of noise, the same in every holder) and a reference key-frame (the lowest holder, -1 for one in five); a
    pixel of noise on every key-point, the points ordered along x and seen through a window of 300 that moves by 25 per key-frame
    (so that the first key-frames fall out of the last one's ordered list and become fixed cameras), and one observation in twenty-five 8 px off (what the chi2 gates erase).  create runs
    for the last three key-frames in turn with an update between them, as there"""
    rng = np.random.default_rng(seed)
    W = np.stack([np.sort(rng.uniform(-3, 7, n_world)), rng.uniform(-2, 2, n_world), rng.uniform(4, 9, n_world)], 1)
    Wn = W + rng.normal(0, 0.01, W.shape)
    mapped = rng.random(n_world) < 0.4
    base_d = rng.integers(0, 256, (n_world, 32), dtype=np.uint8)
    node = rng.integers(0, n_nodes, n_world)
    level = rng.integers(0, 4, n_world)
    rot0 = rng.uniform(0, 360, n_world)
    first = {}
    script, c = [], np.zeros(3)
    for k in range(K):
        c = c + (np.array([0.0, 0.02, 0.15]) if k % 3 == 2 else np.array([rng.uniform(0.25, 0.45), rng.uniform(-0.05, 0.05), 0.0]))
        T = ni.se3(rng.normal(0, 0.02, 3), c)
        seen = 25 * k + np.sort(rng.choice(300, n_feat, replace=False))   # a window that moves with the camera
        seen = seen[rng.permutation(n_feat)]
        ids, flags, octave, depth, ur, desc, angle, nodes, xy, pts, refs = [], [], [], [], [], [], [], [], [], [], []
        for p in seen:
            pc = [T[3 * r] * W[p][0] + T[3 * r + 1] * W[p][1] + T[3 * r + 2] * W[p][2] + T[9 + r] for r in range(3)]
            off = rng.normal(0, 0.5, 2) + (np.array([8.0, -6.0]) if mapped[p] and rng.random() < 0.04 else 0.0)
            u, v, z = f32(500.0 * pc[0] / pc[2] + 320.0 + off[0]), f32(500.0 * pc[1] / pc[2] + 240.0 + off[1]), f32(pc[2])
            stereo = rng.random() < 0.33
            d = z * (f32(1.5) if rng.random() < 1 / 12 else f32(1.0))
            ids.append(int(p) if mapped[p] else -1), flags.append(int(rng.choice([1, 3])) if mapped[p] else 0)
            octave.append(int(level[p] + (4 if rng.random() < 0.05 else 0)))
            depth.append(float(d) if stereo else -1.0), ur.append(float(u - f32(40.0) / d) if stereo else -1.0)
            desc.append(ni.flip_bits(rng, base_d[p], int(rng.integers(0, 6))))
            angle.append(float(f32((rot0[p] + 20.0 * k + rng.uniform(-2, 2)) % 360.0)) if rng.random() < 0.9 else float(f32(rng.uniform(0, 360))))
            nodes.append(int(node[p])), xy.append((u, v))
            pts.append(Wn[p] if mapped[p] else np.zeros(3))
            first.setdefault(int(p), k)
            refs.append((first[int(p)] if p % 5 else -1) if mapped[p] else -1)
        script.append(("insert", ids, flags, octave, depth, ur, dict(desc=np.array(desc, np.uint8), angle=angle, nodes=nodes,
                                                                      points=np.array(pts), refs=refs)))
        script.append(("pose", k, T))
        script.append(("xy", k, np.array(xy, f32)))
        script.append(("update", [k]))
    for k in (K - 3, K - 2, K - 1):
        script += [("create", k, 10), ("update", [k])]
    return script


SEED = 1   # chosen on the CPU (tests/test_local_ba_store_ref.py checks it): every chi2 decisive, no point at obs 2 by a margin edge
SCENE_CAPS = (16, 2048, 16384)
SCENE_CURRENT = 11
# the oracle's own se3_log against tests/se3_ref.py on the poses of these stores (measured 3.53e-16 by
# tests/test_local_ba_store_ref.py, which checks the figure); the device's poses6 get ten times that
POSES6_ORACLE_WORST = 3.6e-16


def all_poses():
    """every pose the windows of these tests take a logarithm of, as Tcw12"""
    return [np.array(s[2], np.float64) for s in seeded_scene(SEED) if s[0] == "pose"] + [np.array(p, np.float64) for p in Hand(6).pose]
