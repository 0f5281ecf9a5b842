"""Inputs of the store's loop-pose-graph tests (test infrastructure): the script runner on the model
(tests/pose_graph_store_ref.py), the hand-made stores shared by the model's CPU tests and the device's GPU tests, the wide
store and the drifted loop.

A script is a list of the steps of tests/local_ba_inputs.py and two more: ("loop_edge", a, b) and ("refs", k, ref_kf [n]).  A case is
dict(name, script, curr, match, inp, want[, NK, max_edges, dev]): inp = pose_graph_store_ref.make_inputs(...), want = fields of
the window's record worked out by hand.

Unlike local_ba_inputs.Hand, every carrier of a map point stores the SAME position and the same reference key-frame: the
write-back moves a feature row through its own reference, and equal rows must stay equal."""
import math

import numpy as np

import local_ba_inputs as li
import pose_graph_store_ref as pr

f32 = np.float32
NK_HAND = 128
MAX_EDGES = 512
CAPS = (16, 1024, 8192)
CAM6, SF, FIRST_ID = li.CAM6, li.SF, li.FIRST_ID


class ModelRunner(li.ModelRunner):
    def __init__(self, caps=CAPS, max_edges=MAX_EDGES, exp=None, log=None):
        self.m = pr.PoseGraphModel(CAM6, SF, FIRST_ID, caps, exp, log, max_edges)

    def step(self, s):
        if s[0] == "loop_edge":
            self.m.add_loop_edge(s[1], s[2])
        elif s[0] == "refs":
            self.m.set_point_refs(s[1], s[2])
        else:
            super().step(s)


def run_model(script, max_edges=MAX_EDGES, **kw):
    r = ModelRunner(max_edges=max_edges, **kw)
    for s in script:
        r.step(s)
    return r.m


def rot(axis, angle):
    """Rodrigues, row-major 9 floats"""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def pose12(R, t):
    return [float(x) for x in np.asarray(R).reshape(-1)] + [float(x) for x in t]


def sim3_near(T12, seed, scale=1.0):
    """a Sim3 a few centimetres and degrees off the pose, its quaternion deliberately not of unit length"""
    rng = np.random.default_rng(seed)
    R = rot(rng.normal(size=3), rng.uniform(0.01, 0.05)) @ np.asarray(T12[:9]).reshape(3, 3)
    S = pr.from_pose(pose12(R, np.asarray(T12[9:]) + rng.normal(0, 0.05, 3)))
    return [1.0001 * c for c in S[:4]] + [scale * c for c in S[4:7]] + [scale]


class Scene:
    """see(k, pid, ref): map point pid in the next feature of key-frame k; its position is a function of pid alone"""

    def __init__(self, poses):
        self.pose = [list(p) for p in poses]
        self.kf = [dict(ids=[], refs=[]) for _ in poses]

    @staticmethod
    def position(pid):
        rng = np.random.default_rng(pid)
        return np.array([rng.uniform(-2, 3), rng.uniform(-1.5, 1.5), rng.uniform(3, 9)])

    def see(self, k, pids, ref):
        for p in pids:
            self.kf[k]["ids"].append(int(p)), self.kf[k]["refs"].append(ref(p) if callable(ref) else ref)

    def script(self, update=True, after=None, poses=None):
        out, after = [], after or {}
        for k, f in enumerate(self.kf):
            n = len(f["ids"])
            pts = np.array([self.position(p) for p in f["ids"]]).reshape(n, 3)
            xy = np.stack([f32(20.0) + f32(4.0) * np.arange(n, dtype=f32), np.full(n, f32(100.0 + k))], 1).astype(f32)
            out.append(("insert", list(f["ids"]), [1] * n, [0] * n, [-1.0] * n, [-1.0] * n,
                        dict(desc=np.zeros((n, 32), np.uint8), angle=[0.0] * n, nodes=[0] * n, points=pts)))
            if poses is None or k in poses:
                out.append(("pose", k, list(self.pose[k])))
            out.append(("xy", k, xy))
            if update:
                out.append(("update", [k]))
            out += after.get(k, [])
        # (the reference key-frames go in once every key-frame is there: the setter takes numbers below the store's size)
        return out + [("refs", k, list(f["refs"])) for k, f in enumerate(self.kf)]


# key-frame poses of the hand cases: small rotations, and turns of about 175 degrees about x, y and z, so that the pose
# column's quaternion comes through each of Eigen's four branches
HAND_POSES = [pose12(rot((0.2, 1, 0.1), 0.02 * k), (0.3 * k, 0.02 * k, 0.01 * k)) for k in range(5)] + \
    [pose12(rot((1, 0.02, 0.01), 3.05), (1.5, 0.1, 0.2)), pose12(rot((0.01, 1, 0.03), 3.06), (1.8, 0.1, 0.0)), pose12(rot((0.02, 0.01, 1), 3.04), (2.1, 0.0, 0.1))]
H = list(range(1000, 1104))      # 104 points every key-frame 1 .. 7 sees: every pair of them has weight >= 104
L0 = list(range(2000, 2020))     # key-frames 0, 1, 7: weight 20
E36, E46, E56 = [2100, 2101], [2110, 2111, 2112, 2113], [2120, 2121, 2122]
OWN0 = list(range(2200, 2210))
CP_POINT = H[8]                  # in cp_id with cp_ref 6, its stored ref_kf is 1
REF_ERASED, REF_UNKNOWN = H[0:4], H[4:8]   # ref_kf = 4 (erased below), ref_kf = -1


def _h_ref(p):
    return 4 if p in REF_ERASED else -1 if p in REF_UNKNOWN else 1


def main_scene():
    """eight key-frames inserted and connected one after the other, so that parent[k] < k: 1 -> 0, 2 -> 1, 3 -> 2, 4 -> 3, 5 -> 4
    (ties go to the higher number), 6 -> 4 (108 against 107).  Erasing 4 once 6 is in re-parents 6 -> 3 (106 against 5's 104)
    and then 5 -> 6 (107 against 104): a child with a LOWER number than its parent.  Then 7 -> 1 (124 with the points of L0)."""
    s = Scene(HAND_POSES)
    s.see(0, L0 + OWN0, 0)
    for k in range(1, 8):
        s.see(k, H, _h_ref)
    s.see(1, L0, 0), s.see(7, L0, 0)
    s.see(3, E36, 3), s.see(6, E36, 3), s.see(4, E46, 4), s.see(6, E46, 4), s.see(5, E56, 5), s.see(6, E56, 5)
    return s.script(after={6: [("erase", 4)]})


def main_inputs(scales=(1.05, 0.97, 1.02)):
    P = HAND_POSES
    corr = {k: (sim3_near(P[k], 10 + k, sc), sim3_near(P[k], 20 + k)) for k, sc in zip((5, 6, 7), scales)}
    return pr.make_inputs(corr, {6: [0, 1, 2], 7: [0]}, {CP_POINT: 6})


def clique_scene(K, shared):
    s = Scene(HAND_POSES[:K])
    for k in range(K):
        s.see(k, range(1000, 1000 + shared), 0)
    return s


def hand_cases():
    cases = []

    def case(name, script, curr, match, inp, want, **extra):
        cases.append(dict(name=name, script=script, curr=curr, match=match, inp=inp, want=want, **extra))

    none = pr.make_inputs()
    # the spanning tree alone: three key-frames of weight 20
    case("b_tree_alone", clique_scene(3, 20).script(), 2, 0, none, dict(n_nodes=3, n_edges=2, n_a=0, n_b=2, n_c=0, n_d=0, status=pr.OK))
    # earlier loop edges alone: no connection was ever computed; 0 - 1 is below curr on both sides, 1 - 2 only from 2
    case("c_loop_edges_alone", clique_scene(3, 20).script(update=False) + [("loop_edge", 0, 1), ("loop_edge", 2, 1)], 2, 0, none,
         dict(n_nodes=3, n_edges=3, n_a=0, n_b=0, n_c=3, n_d=0, status=pr.OK), dev=True)
    # weight 104 everywhere: the tree 1 -> 0, 2 -> 1 and the one covisibility edge 2 -> 0 (A and D need weights, and weights a tree)
    case("d_covisibility_beside_the_tree", clique_scene(3, 104).script(), 2, 0, none,
         dict(n_nodes=3, n_edges=3, n_a=0, n_b=2, n_c=0, n_d=1, status=pr.OK))
    # the same with the corrected pair as a loop connection: A takes 2 -> 0 and D loses it to `inserted`
    case("e_loop_connection_replaces_it", clique_scene(3, 104).script(), 2, 0,
         pr.make_inputs({2: (sim3_near(HAND_POSES[2], 1, 1.1), sim3_near(HAND_POSES[2], 2))}, {2: [0]}),
         dict(n_nodes=3, n_edges=3, n_a=1, n_b=2, n_c=0, n_d=0, status=pr.OK), dev=True)
    # everything together (main_scene): key-frame 4 erased in the middle, 1 bad and not erased, the loop edges 5 - 2 (below curr on
    # both sides) and 7 - 3 (7 is above curr = 6).  A: 6 -> 1, 6 -> 2 (6 -> 0 has weight 0, 7 -> 0 weight 20: dropped).
    # B: 1, 2, 3, 5, 6, 7.  C: 5 -> 2, 2 -> 5, 7 -> 3.  D: worked out by the pointer model (tests/test_pose_graph_store_ref.py)
    tail = [("bad", 1), ("loop_edge", 5, 2), ("loop_edge", 7, 3)]
    case("f_all_together", main_scene() + tail, 6, 2, main_inputs(), dict(n_nodes=7, n_a=2, n_b=6, n_c=3, status=pr.OK), main=True)
    case("g_all_together_device_form", main_scene() + tail, 6, 2, main_inputs((1.0, 1.0, 1.0)), dict(n_nodes=7, n_a=2, n_b=6, n_c=3, status=pr.OK),
         main=True, dev=True)
    # EMPTY: match erased; a node without a pose.  OVERFLOW: one edge too many
    empty = dict(n_nodes=0, n_edges=0, n_a=0, n_b=0, n_c=0, n_d=0, status=pr.EMPTY)
    case("h_match_erased", main_scene() + tail, 6, 4, main_inputs(), empty, sticky=1)
    case("i_node_without_a_pose", clique_scene(3, 20).script(poses=[0, 2]), 2, 0, none, empty, sticky=1)
    case("j_one_edge_too_many", clique_scene(3, 104).script(), 2, 0, none,
         dict(n_nodes=3, n_edges=3, n_a=0, n_b=2, n_c=0, n_d=1, status=pr.OVERFLOW), max_edges=2, sticky=pr.STICKY_PG_CAPACITY)
    return cases


def wide_case(K=130, NK=16):
    """130 key-frames of 16 features in a chain (each shares 8 points with the one before: below 15, so the strongest is the
    only connection and the parent), and eleven earlier loop edges: 129 tree edges and 22 loop edges, 130 nodes -- the counts,
    the scan and the emit cross 64 and 128 on both"""
    rng = np.random.default_rng(4)
    poses = [pose12(rot(rng.normal(size=3), rng.uniform(0, 0.3)), (0.2 * k, rng.uniform(-0.1, 0.1), 0.0)) for k in range(K)]
    s = Scene(poses)
    for k in range(K):
        s.see(k, range(3000 + 8 * k, 3000 + 8 * k + 16), lambda p: min((p - 3000) // 8, K - 1))   # a holder, the same in both
    loops = [("loop_edge", 10 * i + 45, 10 * i) for i in range(8)] + [("loop_edge", 128, 3), ("loop_edge", 127, 3), ("loop_edge", 126, 3)]
    corr = {129: (sim3_near(poses[129], 7), sim3_near(poses[129], 8)), 128: (sim3_near(poses[128], 9), sim3_near(poses[128], 10))}
    return dict(name="k_wide", script=s.script() + loops, curr=129, match=3, inp=pr.make_inputs(corr, {129: [3]}, {}), NK=NK,
                want=dict(n_nodes=130, n_edges=151, n_a=0, n_b=129, n_c=22, n_d=0, status=pr.OK))


def drifted_loop(N=12):
    """a ring of N key-frames whose estimates drift: neighbours share 20 points (a chain of tree edges and nothing else), the
    last and the first share 104 (the loop connection) and the last two 110, so that the last one's parent is its predecessor;
    256 features per key-frame.  S_corr of the last is what the loop measurement makes of the first's
    pose; the graph is ONE cycle of N equally weighted edges"""
    true, est = [], []
    rng = np.random.default_rng(11)
    for k in range(N):
        a = 2 * math.pi * k / N
        Rwc = rot((0, 1, 0), a)
        c = np.array([3 * math.sin(a), 0.0, 3 - 3 * math.cos(a)])
        true.append(pose12(Rwc.T, -Rwc.T @ c))
        d = 0.01 * k
        Rd = Rwc.T   # the drift is in the positions alone: a rotation error would trade against translation residuals by lever arm
        est.append(pose12(Rd, -Rd @ (c + np.array([d, 0.3 * d, -0.5 * d]))))
    s = Scene(est)
    group = lambda k: range(4000 + 200 * k, 4000 + 200 * k + (110 if k == N - 2 else 20))   # shared by k and k + 1
    for k in range(N):
        s.see(k, group(k), k)
        if k:
            s.see(k, group(k - 1), k - 1)
    s.see(0, range(5000, 5104), 0), s.see(N - 1, range(5000, 5104), 0)
    # the loop measurement: the true relative pose last <- first; the corrected pose of the last follows from the first's estimate
    T = lambda p: np.vstack([np.hstack([np.asarray(p[:9]).reshape(3, 3), np.asarray(p[9:]).reshape(3, 1)]), [0, 0, 0, 1]])
    Tcm = T(true[N - 1]) @ np.linalg.inv(T(true[0]))
    Tcw = Tcm @ T(est[0])
    S_corr = pr.from_pose(pose12(Tcw[:3, :3], Tcw[:3, 3]))
    return dict(name="l_drifted_loop", script=s.script(), curr=N - 1, match=0, N=N, Tcm=Tcm, NK=256,
                inp=pr.make_inputs({N - 1: (S_corr, pr.from_pose(est[N - 1]))}, {N - 1: [0]}, {}),
                want=dict(n_nodes=N, n_edges=N, n_a=1, n_b=N - 1, n_c=0, n_d=0, status=pr.OK))


# the float64 model's worst error against the numpy.longdouble matrix formulation over the edges and moved points of these
# cases, measured and checked by tests/test_pose_graph_store_ref.py; the device gets ten times that
MODEL_LONGDOUBLE_WORST = 6.6e-15   # measured 6.53e-15
