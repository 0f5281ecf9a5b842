"""CPU tests of the model of the store's loop pose graph (tests/pose_graph_store_ref.py): its edge list against an independent
restatement of src/optimizer_ceres.cpp:1094-1236 over Python objects, sets and dicts (the pointer model); its Sim3 algebra
against 4 x 4 matrices in numpy.longdouble, whose distance from the float64 model is the yardstick of the device's bounds; the
hand cases' records; and that every case is about what its name says."""
import numpy as np
import pytest

import pose_graph_store_inputs as pi
import pose_graph_store_ref as pr

LD = np.longdouble


# ---- the pointer model: KeyFrame objects as the reference holds them ----------------------------------------------------------
class KF:
    def __init__(self, id_):
        self.id, self.parent, self.children, self.loop_edges, self.weights, self.ordered, self.bad = id_, None, set(), set(), {}, [], False

    def covisibles_by_weight(self, w):   # src/keyframe.cpp:341-356
        wts = [self.weights[k] for k in self.ordered]
        if not wts:
            return []
        n = 0
        while n < len(wts) and wts[n] >= w:   # upper_bound on a descending list
            n += 1
        return self.ordered[:n]


def pointer_edges(m, curr, match, inp):
    """(family, id1, id2) in the reference's order, from objects built off the model's state"""
    alive = [k for k in range(len(m.store)) if not m.erased[k]]
    kfs = {k: KF(k) for k in alive}
    for k, kf in kfs.items():
        p = m.conn.parent[k]
        kf.parent = kfs.get(p) if p >= 0 else None
        kf.children = {kfs[c] for c in m.conn.children[k] if c in kfs}
        kf.loop_edges = {kfs[l] for l in m.loop_edges[k] if l in kfs}
        kf.weights = {kfs[j]: w for j, w in m.conn.W[k].items() if j in kfs}
        kf.ordered = [kfs[j] for j in m.conn.ordered[k] if j in kfs]
        kf.bad = bool(m.store[k]["bad"])
    keys = [int(k) for k in inp["corr_kf"]]
    loop_connections = {kfs[k]: {kfs[int(j)] for j in inp["lc_kf"][inp["lc_start"][r]:inp["lc_start"][r + 1]] if int(j) in kfs}
                        for r, k in enumerate(keys) if k in kfs}
    out, inserted = [], set()
    by_id = lambda s: sorted(s, key=lambda kf: kf.id)
    for kf in by_id(loop_connections):
        for kc in by_id(loop_connections[kf]):
            if kc is kf:
                continue
            if (kc.id != curr or kc.id != match) and kf.weights.get(kc, 0) < 100:
                continue
            out.append((0, kf.id, kc.id))
            inserted.add((min(kf.id, kc.id), max(kf.id, kc.id)))
    for kf in by_id(kfs.values()):
        if kf.parent is not None:
            out.append((1, kf.id, kf.parent.id))
        for kfl in by_id(kf.loop_edges):
            if kfl.id < curr:
                out.append((2, kf.id, kfl.id))
        for kfw in kf.covisibles_by_weight(100):
            if kfw is kf.parent or kfw in kf.children or kfw in kf.loop_edges:
                continue
            if kfw.bad or not (kfw.id < kf.id):
                continue
            if (kfw.id, kf.id) in inserted:
                continue
            out.append((3, kf.id, kfw.id))
    return out


def model_edges(m, w):
    return [(f, int(w["node_kf"][i]), int(w["node_kf"][j])) for f, i, j in zip(m.pg_families, w["e_i"], w["e_j"])]


ALL = pi.hand_cases() + [pi.wide_case(), pi.drifted_loop()]


@pytest.fixture(scope="module")
def windows():
    out = {}
    for c in ALL:
        m = pi.run_model(c["script"], c.get("max_edges", pi.MAX_EDGES))
        out[c["name"]] = (c, m, m.pg_window(c["curr"], c["match"], c["inp"]))
    return out


@pytest.mark.parametrize("name", [c["name"] for c in ALL])
def test_records_and_edges_against_the_pointer_model(windows, name):
    c, m, w = windows[name]
    assert {k: m.pg_record[k] for k in c["want"]} == c["want"]
    assert m.sticky == c.get("sticky", 0)
    if w is None:
        return
    assert model_edges(m, w) == pointer_edges(m, c["curr"], c["match"], c["inp"])
    assert m.pg_record["fixed_node"] == list(w["node_kf"]).index(c["match"])
    assert np.abs(np.linalg.norm(w["quats"], axis=1) - 1).max() < 1e-15 and np.abs(np.linalg.norm(w["q_meas"], axis=1) - 1).max() < 1e-15


def test_the_main_case_is_about_what_it_says(windows):
    c, m, w = windows["f_all_together"]
    # the tree after the erase: a child below its parent
    assert [m.conn.parent[k] for k in (1, 2, 3, 5, 6, 7)] == [0, 1, 2, 6, 3, 1] and m.erased[4] and list(w["node_kf"]) == [0, 1, 2, 3, 5, 6, 7]
    # every rule of family D excludes an entry on its own
    alone = {why[0] for k, w_, why in m.pg_skips if len(why) == 1}
    assert alone == set(pr.D_RULES), alone
    assert m.pg_record["n_d"] > 0
    edges = model_edges(m, w)
    assert (0, 6, 1) in edges and (0, 6, 2) in edges and not any(e[0] == 0 and e[2] == 0 for e in edges)   # weights 0 and 20 dropped
    assert (2, 7, 3) in edges and (2, 3, 7) not in edges and (2, 5, 2) in edges and (2, 2, 5) in edges      # l > curr, l < curr
    assert m.locked[5] and m.locked[2] and m.locked[7] and m.locked[3]
    # the pose column reaches the quaternion through each of Eigen's branches
    traces = [p[0] + p[4] + p[8] for p in pi.HAND_POSES]
    assert sum(t > 0 for t in traces) >= 1 and {int(np.argmax([p[0], p[4], p[8]])) for p, t in zip(pi.HAND_POSES, traces) if t <= 0} == {0, 1, 2}


# ---- the algebra against 4 x 4 matrices in longdouble ---------------------------------------------------------------------------
def M(S):
    q = np.array(S[:4], LD)
    q = q / np.sqrt((q * q).sum())
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], LD)
    T = np.eye(4, dtype=LD)
    T[:3, :3], T[:3, 3] = LD(S[7]) * R, np.array(S[4:7], LD)
    return T


def inv4(T):
    s2 = (T[0, :3] * T[0, :3]).sum()
    out = np.eye(4, dtype=LD)
    out[:3, :3] = T[:3, :3].T / s2
    out[:3, 3] = -(out[:3, :3] @ T[:3, 3])
    return out


def err(S, T):
    return float(np.abs(M(S) - T).max())


def longdouble_errors(m, c, w):
    """the float64 model against the matrix formulation: every node Sim3 read from the pose column, every measurement, and (after
    an apply with the window's own poses nudged) every moved point"""
    worst = 0.0
    row = {int(k): r for r, k in enumerate(c["inp"]["corr_kf"])}
    S = {int(k): [*w["quats"][i], *w["trans"][i], w["scales"][i]] for i, k in enumerate(w["node_kf"])}
    for k in S:
        if k not in row:
            T = np.eye(4, dtype=LD)
            T[:3, :3], T[:3, 3] = np.array(m.store[k]["pose"][:9], LD).reshape(3, 3), np.array(m.store[k]["pose"][9:], LD)
            worst = max(worst, err(S[k], T))
    unc = lambda x: pr.load(c["inp"]["S_uncorr"][row[x]]) if x in row else S[x]
    for e, (f, k, j) in enumerate(model_edges(m, w)):
        T = M(S[j]) @ inv4(M(S[k])) if f == 0 else M(unc(j)) @ inv4(M(unc(k)))
        worst = max(worst, err([*w["q_meas"][e], *w["t_meas"][e], w["s_meas"][e]], T))
    return worst


def nudged(w, seed=3):
    rng = np.random.default_rng(seed)
    return w["quats"] + rng.normal(0, 0.01, w["quats"].shape), w["trans"] + rng.normal(0, 0.02, w["trans"].shape)


def apply_errors(m, w):
    """p_new against Swr * (Srw * p_old) in longdouble matrices, for every feature row of the store"""
    before = [np.array(kf["points"], np.float64).copy() for kf in m.store]
    refs = [list(kf["ref"]) for kf in m.store]
    inp, nodes = m.pg_inp, list(m.pg_nodes)
    Srw, Swr = m.pg_apply(*nudged(w))
    cp = {int(i): int(r) for i, r in zip(inp["cp_id"], inp["cp_ref"])}
    worst, moved = 0.0, 0
    for k in nodes:
        kf = m.store[k]
        for f in range(len(kf["ids"])):
            if not (kf["flags"][f] & 1):
                continue
            idm = cp.get(kf["ids"][f], refs[k][f])
            if idm in nodes:
                i = nodes.index(idm)
                want = (M(Swr[i]) @ (M(Srw[i]) @ np.array([*before[k][f], 1.0], LD)))[:3]
                worst = max(worst, float(np.abs(np.array(kf["points"][f], LD) - want).max()))
                moved += 1
            else:
                assert np.array_equal(kf["points"][f], before[k][f])
    return worst, moved


def test_algebra_against_longdouble_matrices_and_the_recorded_yardstick(windows):
    worst = 0.0
    for name, (c, m, w) in windows.items():
        if w is None:
            continue
        worst = max(worst, longdouble_errors(m, c, w))
        if c.get("main"):
            e, moved = apply_errors(m, w)
            assert moved == m.pg_record["n_points_moved"] > 0 and m.pg_record["n_unanchored"] > 0
            worst = max(worst, e)
    print("float64 model against longdouble matrices:", worst)
    assert 0 < worst <= pi.MODEL_LONGDOUBLE_WORST < 1e-13, worst


def test_apply_keeps_equal_rows_equal_and_counts_the_unanchored():
    c = [x for x in pi.hand_cases() if x["name"] == "f_all_together"][0]
    m = pi.run_model(c["script"])
    w = m.pg_window(c["curr"], c["match"], c["inp"])
    old = {p: m.store[j]["points"][i].copy() for p in pi.H for j, i in m.carriers(p)[:1]}
    m.pg_apply(*nudged(w))
    for p in pi.H + pi.L0:
        rows = [m.store[j]["points"][i].tobytes() for j, i in m.carriers(p)]
        assert len(set(rows)) == 1 and len(rows) >= 3, p
    # ref_kf 4 is erased and -1 is unknown: 8 points x 6 live carriers keep their bytes; the refresh then resolves their reference
    assert m.pg_record["n_unanchored"] == 8 * 6
    for p in pi.REF_ERASED + pi.REF_UNKNOWN:
        j, i = m.carriers(p)[0]
        assert np.array_equal(m.store[j]["points"][i], old[p]) and m.store[j]["ref"][i] == 1
    # every other live feature row moved
    total = sum(len(m.carriers(p)) for p in set(x for s in m.store for x in s["ids"]))
    assert m.pg_record["n_points_moved"] == total - 8 * 6


def test_loop_edge_capacity_and_repeats():
    m = pi.run_model(pi.Scene([pi.HAND_POSES[0]] * 11).script(update=False))   # eleven key-frames without features
    for b in range(1, 9):
        m.add_loop_edge(0, b)
    m.add_loop_edge(0, 3)   # a repeat changes nothing
    assert sorted(m.loop_edges[0]) == list(range(1, 9))
    with pytest.raises(pr.CapacityError):
        m.add_loop_edge(9, 0)
    assert m.loop_edges[9] == set() and not m.locked[9]
