"""Model of the store's loop pose graph (test infrastructure): the pose collection and the four edge families of
Optimizer::solvePoseGraphLoop (src/optimizer_ceres.cpp:1062-1236) and its write-back (:1264-1301), restated in plain Python on
top of tests/local_ba_store_ref.py's LocalBaModel (the store, the connections, the erase, the refresh), as the contract block
of include/vo_hip.h states them.

A Sim3 is a list of 8 Python floats: quaternion x y z w, translation, scale.  A Python float is the reference's double, every
operation rounded on its own; the functions below follow the operation order of csrc/sim3_compose.h line by line, so that
every quaternion, translation and point agrees with the device bit for bit."""
import math

import numpy as np

from local_ba_store_ref import EMPTY, OK, OVERFLOW, STICKY_INVALID, LocalBaModel

STICKY_PG_CAPACITY = 128
MAX_LOOP_EDGES = 8
MAX_NODES = 683
MIN_WEIGHT = 100
PG_RECORD = ("n_nodes", "n_edges", "n_a", "n_b", "n_c", "n_d", "status", "curr", "match", "fixed_node", "n_points_moved", "n_unanchored")
D_RULES = ("parent", "child", "loop", "bad", "not_lower", "inserted")


# ---- csrc/sim3_compose.h, line by line ----------------------------------------------------------------------------------------
def dot3(a, b, c, d, e, f):
    return (a * b + c * d) + e * f


def normalize(q):
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [c / n for c in q]


def quat_from_matrix(m):
    q = [0.0] * 4
    t = (m[0] + m[4]) + m[8]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (m[7] - m[5]) * t, (m[2] - m[6]) * t, (m[3] - m[1]) * t
        return q
    i = 0
    if m[4] > m[0]:
        i = 1
    if m[8] > m[4 * i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = math.sqrt(((m[4 * i] - m[4 * j]) - m[4 * k]) + 1.0)
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3] = (m[3 * k + j] - m[3 * j + k]) * t
    q[j] = (m[3 * j + i] + m[3 * i + j]) * t
    q[k] = (m[3 * k + i] + m[3 * i + k]) * t
    return q


def matrix(q):
    tx, ty, tz = q[0] + q[0], q[1] + q[1], q[2] + q[2]
    twx, twy, twz, txx, txy, txz = tx * q[3], ty * q[3], tz * q[3], tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return [1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)]


def rotate(R, p):
    return [dot3(R[3 * r], p[0], R[3 * r + 1], p[1], R[3 * r + 2], p[2]) for r in range(3)]


def act(S, p):
    r = rotate(matrix(S), p)
    return [S[7] * r[c] + S[4 + c] for c in range(3)]


def mul(A, B):
    q = [((A[3] * B[0] + A[0] * B[3]) + A[1] * B[2]) - A[2] * B[1],
         ((A[3] * B[1] + A[1] * B[3]) + A[2] * B[0]) - A[0] * B[2],
         ((A[3] * B[2] + A[2] * B[3]) + A[0] * B[1]) - A[1] * B[0],
         ((A[3] * B[3] - A[0] * B[0]) - A[1] * B[1]) - A[2] * B[2]]
    return normalize(q) + act(A, B[4:7]) + [A[7] * B[7]]


def inv(S):
    q = [-S[0], -S[1], -S[2], S[3]]
    s = 1.0 / S[7]
    r = rotate(matrix(q), S[4:7])
    return q + [-(s * r[c]) for c in range(3)] + [s]


def load(src):
    S = [float(x) for x in src]
    return normalize(S[:4]) + S[4:]


def from_pose(T):
    T = [float(x) for x in T]
    return normalize(quat_from_matrix(T)) + [T[9], T[10], T[11], 1.0]


# ---- the model ----------------------------------------------------------------------------------------------------------------
class CapacityError(Exception):
    pass


def make_inputs(corr=None, loop_connections=None, corrected_points=None):
    """correctLoop's outputs as the entry points take them.  corr: {key-frame: (S_corr, S_uncorr)}; loop_connections:
    {key-frame of corr: iterable of key-frames}; corrected_points: {id: correctReference_}"""
    corr, lc, cp = corr or {}, loop_connections or {}, corrected_points or {}
    keys = sorted(corr)
    assert set(lc) <= set(keys)
    start, flat = [0], []
    for k in keys:
        flat += sorted(lc.get(k, ()))
        start.append(len(flat))
    ids = sorted(cp)
    return dict(corr_kf=np.array(keys, np.int32), S_corr=np.array([corr[k][0] for k in keys], np.float64).reshape(-1, 8),
                S_uncorr=np.array([corr[k][1] for k in keys], np.float64).reshape(-1, 8), lc_start=np.array(start, np.int32),
                lc_kf=np.array(flat, np.int32), cp_id=np.array(ids, np.int32), cp_ref=np.array([cp[i] for i in ids], np.int32))


class PoseGraphModel(LocalBaModel):
    def __init__(self, cam6=None, scale_factors=None, first_point_id=0, caps=(64, 8192, 65536), exp=None, log=None, max_edges=4096):
        super().__init__(cam6, scale_factors, first_point_id, caps, exp, log)
        self.max_edges = int(max_edges)
        self.loop_edges = []
        self.pg_win, self.pg_inp, self.pg_nodes = None, None, None
        self.pg_record = {k: 0 for k in PG_RECORD}
        self.pg_record.update(status=EMPTY, fixed_node=-1)
        self.pg_families, self.pg_skips = [], []   # per edge its family; per skipped D entry (k, w, the rules that apply)

    def insert(self, ids, flags, bad=False, desc=None, angle=None, nodes=None):
        k = super().insert(ids, flags, bad, desc, angle, nodes)
        self.loop_edges.append(set())
        return k

    def add_loop_edge(self, a, b):
        """KeyFrame::addLoopEdge both ways (src/keyframe.cpp:528-533)"""
        assert a != b
        for x, y in ((a, b), (b, a)):
            if y not in self.loop_edges[x] and len(self.loop_edges[x]) >= MAX_LOOP_EDGES:
                raise CapacityError((a, b))
        self.loop_edges[a].add(b), self.loop_edges[b].add(a)
        self.locked[a] = self.locked[b] = 1

    def weight(self, a, b):
        return self.conn.W[a].get(b, 0)

    # ---- the window (:1062-1236) ---------------------------------------------------------------------------------------
    def pg_window(self, curr, match, inp):
        rec = {k: 0 for k in PG_RECORD}
        rec.update(curr=curr, match=match, fixed_node=-1)
        self.pg_record, self.pg_win, self.pg_inp, self.pg_nodes = rec, None, inp, None
        self.pg_families, self.pg_skips = [], []
        size = len(self.store)

        def empty():
            self.sticky |= STICKY_INVALID
            rec["status"] = EMPTY
            return None

        if self.erased[curr] or self.erased[match]:
            return empty()
        nodes = [k for k in range(size) if not self.erased[k]]
        if any(self.store[k]["pose"] is None for k in nodes):
            return empty()
        node_of = {k: i for i, k in enumerate(nodes)}
        rec.update(n_nodes=len(nodes), fixed_node=node_of[match])
        corr = [int(k) for k in inp["corr_kf"]]
        row_of = {k: r for r, k in enumerate(corr)}
        S = {k: load(inp["S_corr"][row_of[k]]) if k in row_of else from_pose(self.store[k]["pose"]) for k in nodes}
        unc = lambda x: load(inp["S_uncorr"][row_of[x]]) if x in row_of else S[x]
        edges, inserted = [], set()
        for r, k in enumerate(corr):                                  # A: loop connections on corrected poses (:1094-1125)
            if k not in node_of:
                continue
            for j in (int(x) for x in inp["lc_kf"][inp["lc_start"][r]:inp["lc_start"][r + 1]]):
                if j != k and j in node_of and self.weight(k, j) >= MIN_WEIGHT:   # Q-B5: only the weight gate acts
                    edges.append((0, k, j))
                    inserted.add((min(k, j), max(k, j)))
        for k in nodes:                                               # (:1128-1236)
            parent = self.conn.parent[k]
            if parent != k and parent in node_of:
                edges.append((1, k, parent))
            loops = sorted(self.loop_edges[k])
            for l in loops:
                if l < curr and l != k and l in node_of:
                    edges.append((2, k, l))
            for w in self.conn.ordered[k]:
                if w == k:
                    continue
                if self.weight(k, w) < MIN_WEIGHT:
                    break
                why = [name for name, hit in zip(D_RULES, (w == parent, w in self.conn.children[k], w in self.loop_edges[k], self.store[w]["bad"],
                                                          w >= k, (min(k, w), max(k, w)) in inserted)) if hit]
                if why or w not in node_of:
                    self.pg_skips.append((k, w, why))
                    continue
                edges.append((3, k, w))
        rec.update(n_edges=len(edges), **{"n_" + "abcd"[f]: sum(1 for e in edges if e[0] == f) for f in range(4)})
        if len(nodes) > MAX_NODES or len(edges) > self.max_edges:
            self.sticky |= STICKY_PG_CAPACITY
            rec["status"] = OVERFLOW
            return None
        q_meas, t_meas, s_meas = [], [], []
        for f, k, j in edges:
            Sji = mul(S[j], inv(S[k])) if f == 0 else mul(unc(j), inv(unc(k)))
            q_meas.append(Sji[:4]), t_meas.append(Sji[4:7]), s_meas.append(Sji[7])
        self.pg_families, self.pg_nodes = [e[0] for e in edges], nodes
        self.pg_win = dict(node_kf=np.array(nodes, np.int32), quats=np.array([S[k][:4] for k in nodes], np.float64).reshape(-1, 4),
                           trans=np.array([S[k][4:7] for k in nodes], np.float64).reshape(-1, 3), scales=np.array([S[k][7] for k in nodes], np.float64),
                           e_i=np.array([node_of[e[1]] for e in edges], np.int32), e_j=np.array([node_of[e[2]] for e in edges], np.int32),
                           q_meas=np.array(q_meas, np.float64).reshape(-1, 4), t_meas=np.array(t_meas, np.float64).reshape(-1, 3),
                           s_meas=np.array(s_meas, np.float64))
        return self.pg_win

    # ---- the write-back (:1264-1301) -----------------------------------------------------------------------------------
    def pg_apply(self, quats, trans):
        w, inp, nodes = self.pg_win, self.pg_inp, self.pg_nodes
        assert w is not None
        quats, trans = np.asarray(quats, np.float64).reshape(-1, 4), np.asarray(trans, np.float64).reshape(-1, 3)
        node_of = {k: i for i, k in enumerate(nodes)}
        Srw = [[float(x) for x in w["quats"][i]] + [float(x) for x in w["trans"][i]] + [float(w["scales"][i])] for i in range(len(nodes))]
        Swr = []
        for i, k in enumerate(nodes):                                 # a. poses
            Siw = normalize([float(x) for x in quats[i]]) + [float(x) for x in trans[i]] + [Srw[i][7]]
            self.store[k]["pose"] = matrix(Siw) + [Siw[4 + c] / Siw[7] for c in range(3)]
            Swr.append(inv(Siw))
        cp = {int(i): int(r) for i, r in zip(inp["cp_id"], inp["cp_ref"])}
        moved = unanchored = 0
        live = set()
        for k in nodes:                                               # b. re-anchoring, a feature row at a time
            kf = self.store[k]
            for f in range(len(kf["ids"])):
                if not (kf["flags"][f] & 1):
                    continue
                p = kf["ids"][f]
                if p >= 0:
                    live.add(p)
                idm = cp[p] if p in cp else kf["ref"][f]
                if idm in node_of:
                    i = node_of[idm]
                    kf["points"][f] = act(Swr[i], act(Srw[i], [float(x) for x in kf["points"][f]]))
                    moved += 1
                else:
                    unanchored += 1
        self.refresh(sorted(live))                                    # c. updateNormalAndDepth of every live point
        self.pg_record.update(n_points_moved=moved, n_unanchored=unanchored)
        self.pg_win = None
        return Srw, Swr
