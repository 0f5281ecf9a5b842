"""The model of the store's loop correction (tests/loop_correct_ref.py) against (a) a pointer-object transcription of
src/loopClosing.cpp:364-437 and :461-479 that really runs in the reference's order -- std::map walked in ascending key-frame
number, setPose after the key-frame's points, updateNormalAndDepth in place on whatever poses stand, updateConnections from
tests/connections_ref.py -- and (b) a matrix formulation in numpy.longdouble (4 x 4 similarity matrices, no quaternions).  It
also holds the conditions the hand stores of tests/loop_correct_inputs.py rely on.  No GPU."""
import copy
import math

import numpy as np
import pytest

import loop_correct_inputs as ci
import loop_correct_ref as lr
import pose_graph_store_inputs as pi
import pose_graph_store_ref as pr
import test_pose_graph_store_ref as tr
from connections_ref import holder_index
from new_points_ref import _center, _dot3

f32 = np.float32
LD = tr.LD


# ---- the pointer-object transcription -----------------------------------------------------------------------------------------
class MP:
    def __init__(self, id_):
        self.id, self.pos, self.ref, self.obs, self.corrected_by, self.correct_ref, self.bad = id_, None, -1, {}, -1, -1, False
        self.normal, self.mind, self.maxd = None, None, None


class KF:
    def __init__(self, id_, pose, n):
        self.id, self.pose, self.mappoints = id_, pose, [None] * n


def objects(m):
    """KeyFrame and MapPoint objects off the model's store: a point's position and reference key-frame are those of its first live
    carrier; observations_ is keyed by key-frame, at the lowest feature"""
    kfs = [KF(k, kf["pose"], len(kf["ids"])) for k, kf in enumerate(m.store)]
    mps = {}
    for k, kf in enumerate(m.store):
        if m.erased[k]:
            continue
        for f in range(len(kf["ids"])):
            p = kf["ids"][f]
            if not (kf["flags"][f] & 1) or p < 0:
                continue
            mp = mps.get(p)
            if mp is None:
                mp = mps[p] = MP(p)
                mp.pos, mp.ref = [float(x) for x in kf["points"][f]], kf["ref"][f]
            kfs[k].mappoints[f] = mp
            mp.obs.setdefault(k, f)
    return kfs, mps


def update_normal_and_depth(m, kfs, mp):
    """src/mappoint.cpp:66-116 on the poses that stand in the objects NOW"""
    if not mp.obs:
        return
    normal, n = [0.0, 0.0, 0.0], 0
    for k in sorted(mp.obs):
        Ow = _center(kfs[k].pose)
        d = [mp.pos[c] + -Ow[c] for c in range(3)]
        ln = math.sqrt(_dot3(d[0], d[0], d[1], d[1], d[2], d[2]))
        normal = [normal[c] + d[c] / ln for c in range(3)]
        n += 1
    ref = mp.ref if mp.ref in mp.obs else min(mp.obs)
    mp.ref = ref
    Ow = _center(kfs[ref].pose)
    d = [mp.pos[c] + -Ow[c] for c in range(3)]
    dist = math.sqrt(_dot3(d[0], d[0], d[1], d[1], d[2], d[2]))
    level = min(max(m.store[ref]["octave"][mp.obs[ref]], 0), 15)
    mp.maxd = f32(dist) * f32(m.sf[level])
    mp.mind = mp.maxd / f32(m.sf[len(m.sf) - 1])
    mp.normal = [normal[c] / float(n) for c in range(3)]


def pointer_propagate(m, curr, Scw):
    """-> (kfs, mps, conn, currConnect, correctSim3, uncorrectSim3) after :364-437, sequentially"""
    kfs, mps = objects(m)
    conn = copy.deepcopy(m.conn)
    vis = m._visible()
    index = holder_index(vis)
    conn.update(vis, curr, index)                                          # :364
    curr_connect = [kfs[k] for k in conn.ordered[curr]] + [kfs[curr]]      # :367-368
    Scw = pr.load(Scw)
    correct, uncorrect = {curr: Scw}, {}
    Swc = pr.inv(pr.from_pose(kfs[curr].pose))                             # :378 (as Sim3 algebra at scale 1)
    for kf in curr_connect:                                                # :384-398
        Siw = pr.from_pose(kf.pose)
        if kf is not kfs[curr]:
            correct[kf.id] = pr.mul(pr.mul(Siw, Swc), Scw)
        uncorrect[kf.id] = Siw
    for k in sorted(correct):                                              # :401 std::map<KeyFrame*, ...>
        kf, Siw, Swi, Sun = kfs[k], correct[k], pr.inv(correct[k]), uncorrect[k]
        for mp in kf.mappoints:                                            # :409
            if mp is None or mp.bad or mp.corrected_by == curr:
                continue
            mp.pos = pr.act(Swi, pr.act(Sun, mp.pos))                      # :421-423
            mp.corrected_by, mp.correct_ref = curr, k
            update_normal_and_depth(m, kfs, mp)                            # :426, in place
        kf.pose = pr.matrix(Siw) + [Siw[4 + c] / Siw[7] for c in range(3)]   # :430-435, AFTER the points
        conn.update(vis, k, index)                                         # :436
    return kfs, mps, conn, [kf.id for kf in curr_connect], correct, uncorrect


def pointer_loop_connections(m, curr_connect):
    """:461-479 on the model's store as it stands -> ({kf: set}, conn)"""
    conn = copy.deepcopy(m.conn)
    vis = m._visible()
    index = holder_index(vis)
    out = {}
    for kf in curr_connect:
        neighbors = list(conn.ordered[kf])
        conn.update(vis, kf, index)
        lc = set(conn.W[kf])                                               # getConnectKFs: the whole map
        for n in neighbors:
            lc.discard(n)
        for c in curr_connect:
            lc.discard(c)
        out[kf] = lc
    return out, conn


def _same_conn(a, b, size):
    for k in range(size):
        assert a.state(k, size) == b.state(k, size), k


def _check_propagate(script, curr, Scw):
    m0 = ci.run_model(script)
    kfs, mps, conn, lst, correct, uncorrect = pointer_propagate(m0, curr, Scw)
    m = ci.run_model(script)
    L = m.propagate_loop(curr, Scw)
    assert L is not None and m.lc_record["status"] == lr.OK
    assert L["list"] == lst and L["corr_kf"] == sorted(correct)
    for j, k in enumerate(L["corr_kf"]):
        assert L["S_corr"][j] == correct[k] and L["S_uncorr"][j] == uncorrect[k]
    assert dict(zip(L["cp_id"], L["cp_ref"])) == {p: mp.correct_ref for p, mp in mps.items() if mp.corrected_by == curr}
    rows = 0
    for k, kf in enumerate(m.store):
        assert kf["pose"] == kfs[k].pose, k
        for f in range(len(kf["ids"])):
            mp = kfs[k].mappoints[f]
            if mp is None or mp.corrected_by != curr:
                continue
            rows += 1
            assert [float(x) for x in kf["points"][f]] == mp.pos, (k, f)
            assert [float(x) for x in kf["normals"][f]] == mp.normal and kf["ref"][f] == mp.ref, (k, f)
            assert f32(kf["maxd"][f]) == mp.maxd and f32(kf["mind"][f]) == mp.mind, (k, f)
    assert rows == m.lc_record["n_rows_moved"] and rows > 0
    _same_conn(m.conn, conn, len(m.store))
    return m0, m, L


SCW = lambda T, scale=1.1: ci.loop_sim3(T, scale)


def test_propagate_against_the_pointer_transcription():
    script = ci.propagate_scene(bad=(3,))
    m0, m, L = _check_propagate(script, ci.CURR, SCW(pi.HAND_POSES[ci.CURR]))
    assert L["corr_kf"] == ci.CORR and sorted(L["list"][:-1]) == [2, 3, 5, 7] and L["list"][-1] == ci.CURR and m.store[3]["bad"]
    cp = dict(zip(L["cp_id"], L["cp_ref"]))
    # a point held by five corrected key-frames moves once, through the lowest; one held by 5, 7 and 0 through 5; the id in two
    # features of key-frame 3 through 3, its carrier in key-frame 4 (outside the set) written too
    assert all(cp[p] == 2 for p in ci.G) and all(cp[p] == 5 for p in ci.H5) and cp[ci.DUP] == 3
    f1, f2 = [f for f, p in enumerate(m.store[3]["ids"]) if p == ci.DUP]
    f4 = m.store[4]["ids"].index(ci.DUP)
    want = pr.act(pr.inv(L["S_corr"][1]), pr.act(L["S_uncorr"][1], [float(x) for x in m0.store[3]["points"][f1]]))
    other = pr.act(pr.inv(L["S_corr"][1]), pr.act(L["S_uncorr"][1], [float(x) for x in m0.store[3]["points"][f2]]))
    assert [list(m.store[k]["points"][f]) for k, f in ((3, f1), (3, f2), (4, f4))] == [want] * 3 and max(abs(a - b) for a, b in zip(want, other)) > 5e-3
    # the naive form (every corrected holder moves the point) ends elsewhere
    p = ci.G[0]
    f = m.store[2]["ids"].index(p)
    twice = pr.act(pr.inv(L["S_corr"][1]), pr.act(L["S_uncorr"][1], [float(x) for x in m.store[2]["points"][f]]))
    assert max(abs(a - b) for a, b in zip(twice, m.store[2]["points"][f])) > 0.05
    # the holders: at the correcting key-frame's position, above it, outside the set; NEVER below it (the model asserts it per
    # point): the lowest corrected holder corrects, and the reference key-frame is a holder
    kinds = set()
    for p, k, j, holders in m.lc_log:
        kinds |= {"at" if q == j else "above" if q > j else "outside" for _, q in holders}
        assert all(q < 0 or q >= j for _, q in holders)
    assert kinds == {"at", "above", "outside"}
    refs = {m.store[k]["ref"][f] for k in ci.CORR for f, p in enumerate(m.store[k]["ids"]) if p in ci.G + ci.H5}
    assert refs >= {2, 5, 1, 7, 0}                      # the correcting key-frame, one above it, ones outside the set
    # the pose translation is t / s: with t the pose differs by more than rounding
    j = L["corr_kf"].index(ci.CURR)
    S = L["S_corr"][j]
    assert S[7] == 1.1 and m.store[ci.CURR]["pose"][9:] == [S[4 + c] / 1.1 for c in range(3)]
    assert max(abs(S[4 + c] - m.store[ci.CURR]["pose"][9 + c]) for c in range(3)) > 0.01
    # each of s3_quat_from_matrix's three off-branches in a stored pose of a corrected key-frame
    branch = []
    for k in ci.CORR:
        T = m0.store[k]["pose"]
        if (T[0] + T[4]) + T[8] <= 0:
            branch.append(int(np.argmax([T[0], T[4], T[8]])))
    assert sorted(branch) == [0, 1, 2]


def test_the_drift_is_large_enough_to_show_a_wrong_pose_state():
    """the correction is at least 0.2 m and 5 degrees, and a normal refreshed on the corrected poses instead of the stored ones
    (what the reference's order rules out) differs by more than 1e-3"""
    script = ci.propagate_scene()
    m0 = ci.run_model(script)
    m = ci.run_model(script)
    L = m.propagate_loop(ci.CURR, SCW(pi.HAND_POSES[ci.CURR]))
    worst_t, worst_a = 1e9, 1e9
    for j, k in enumerate(L["corr_kf"]):
        A, B = tr.M(pr.from_pose(m0.store[k]["pose"])), tr.M(pr.from_pose(m.store[k]["pose"]))
        D = B @ tr.inv4(A)
        worst_t = min(worst_t, float(np.linalg.norm(np.asarray(D[:3, 3], np.float64))))
        worst_a = min(worst_a, math.degrees(math.acos(min(1.0, (float(np.trace(D[:3, :3])) - 1) / 2))))
    assert worst_t >= 0.2 and worst_a >= 5.0, (worst_t, worst_a)
    other = ci.run_model(script)
    other.propagate_loop(ci.CURR, SCW(pi.HAND_POSES[ci.CURR]))
    diffs = []
    for p, k, j, holders in m.lc_log:
        other._refresh_with(p, lambda h: other.store[h]["pose"])          # every pose as step 6 left it
        kk, f = other.carriers(p)[0]
        diffs.append(float(np.abs(np.asarray(other.store[kk]["normals"][f]) - np.asarray(m.store[kk]["normals"][f])).max()))
    assert min(diffs) > 1e-3, min(diffs)


def test_propagate_with_an_empty_list():
    m0, m, L = _check_propagate(ci.lonely_scene(), 1, SCW(pi.HAND_POSES[1], 1.0))
    assert L["corr_kf"] == [1] and L["list"] == [1] and m.lc_record["n_cp"] == 10 and L["S_corr"][0] == pr.load(SCW(pi.HAND_POSES[1], 1.0))


def _snapshot(m):
    size = len(m.store)
    return ([{k: np.asarray(v).tobytes() for k, v in m.state(j).items()} for j in range(size)], [m.conn.state(j, size) for j in range(size)])


def test_refusals_leave_the_store_beyond_step_1():
    Scw = SCW(pi.HAND_POSES[ci.CURR])
    ok = ci.run_model(ci.propagate_scene())
    n_cp = len(ok.propagate_loop(ci.CURR, Scw)["cp_id"])
    for kw, script, status, sticky, n_corr in ((dict(lc_caps=(4, 256, 64)), ci.propagate_scene(), lr.OVERFLOW, lr.STICKY_LC_CAPACITY, 5),
                                                (dict(lc_caps=(8, n_cp - 1, 64)), ci.propagate_scene(), lr.OVERFLOW, lr.STICKY_LC_CAPACITY, 5),
                                                (dict(), ci.propagate_scene(poses=[0, 1, 2, 4, 5, 6, 7]), lr.EMPTY, lr.STICKY_INVALID, 5)):
        m = ci.run_model(script, **kw)
        ref = ci.run_model(script, **kw)
        ref.update_connections([ci.CURR])
        assert m.propagate_loop(ci.CURR, Scw) is None
        assert (m.lc_record["status"], m.sticky, m.lc_record["n_corr"]) == (status, sticky, n_corr)
        assert _snapshot(m) == _snapshot(ref)
        assert m.loop_connections() is None and m.sticky & lr.STICKY_INVALID
    m = ci.run_model(ci.propagate_scene(), lc_caps=(5, n_cp, 64))          # both capacities met exactly
    assert m.propagate_loop(ci.CURR, Scw) is not None and m.sticky == 0
    m = ci.run_model(ci.propagate_scene())
    before = _snapshot(m)
    assert m.propagate_loop(ci.CURR, Scw, state=2) is None and m.sticky == lr.STICKY_INVALID and _snapshot(m) == before


# ---- the loop connections -----------------------------------------------------------------------------------------------------
def _connections_model(**kw):
    s = ci.connections_scene()
    m = ci.run_model(s.script(), **kw)
    L = m.propagate_loop(ci.C_CURR, SCW(pi.HAND_POSES[ci.C_CURR], 1.0))
    assert L["list"] == ci.C_LIST and all(m.conn.ordered[k] and min(m.conn.weights[k]) >= 15 for k in ci.C_LIST)   # thresholded lists
    for st in ci.fusion_steps(s):
        m.update_points(st[1], st[2], st[3])
    return m


def test_loop_connections_against_the_pointer_transcription_and_by_hand():
    m = _connections_model()
    snapshot = {k: set(m.conn.ordered[k]) for k in ci.C_LIST}               # taken BEFORE the loop: the wrong `old`
    w61, w56 = m.conn.W[6][1], m.conn.W[6][5]
    want, conn = pointer_loop_connections(m, ci.C_LIST)
    twin = copy.deepcopy(m)
    rows = m.loop_connections()
    assert rows == {k: sorted(v) for k, v in want.items()} == ci.C_ROWS and m.lc_record["n_lc"] == 4 and m.sticky == 0
    _same_conn(m.conn, conn, len(m.store))
    twin.update_connections(ci.C_LIST)                                      # the graph afterwards
    _same_conn(m.conn, twin.conn, len(m.store))
    # what the rows are about: a connection the fusion created, one of them below 15; a member of the old list (2 in 6's) and the
    # members of currConnect removed; the mode switch (x = 1 with weight 3 is NOT in 6's row; the snapshot puts it there); an
    # update that finds no connection keeps the old map, whose entry below 15 (key-frame 0) then shows
    assert m.conn.W[7][0] == 100 and m.conn.W[7][3] == 3 and m.conn.W[5][2] == 1
    assert w61 == 3 and 1 not in snapshot[6] and 2 in snapshot[6] and w56 == 16 and m.conn.W[6][5] == 17
    naive6 = {j for j, w in m.conn.W[6].items() if w} - snapshot[6] - set(ci.C_LIST)
    assert naive6 == {1} and rows[6] == []
    assert not any(m.store[4]["flags"]) and m.conn.W[4] == {0: 2, 5: 16, 6: 16, 7: 16} and rows[4] == [0]
    inp = m.lc_inputs()
    assert list(inp["corr_kf"]) == [4, 5, 6, 7] and list(inp["lc_start"]) == [0, 1, 2, 2, 4] and list(inp["lc_kf"]) == [0, 2, 0, 3]


def test_loop_connections_capacity_and_no_propagate():
    m = _connections_model(lc_caps=(8, 256, 3))
    twin = copy.deepcopy(m)
    assert m.loop_connections() is None and m.lc_record["n_lc"] == 4 and m.lc_record["connections_status"] == lr.OVERFLOW
    assert m.sticky == lr.STICKY_LC_CAPACITY
    twin.update_connections(ci.C_LIST)
    _same_conn(m.conn, twin.conn, len(m.store))
    m = ci.run_model(ci.connections_scene().script())
    before = _snapshot(m)
    assert m.loop_connections() is None and m.sticky == lr.STICKY_INVALID and _snapshot(m) == before


# ---- the matrix formulation in longdouble -------------------------------------------------------------------------------------
def _T4(T):
    out = np.eye(4, dtype=LD)
    out[:3, :3], out[:3, 3] = np.array(T[:9], LD).reshape(3, 3), np.array(T[9:], LD)
    return out


def longdouble_errors(m0, m, L, Scw, curr):
    """S_uncorr, S_corr, the pose columns and every moved row against 4 x 4 matrices: S_corr[k] = T_k T_curr^-1 Scw,
    p' = S_corr^-1 T_k p, the pose [R | t / s]"""
    worst = 0.0
    Mscw, Tc = tr.M(Scw), _T4(m0.store[curr]["pose"])
    Mk = {}
    for j, k in enumerate(L["corr_kf"]):
        Tk = _T4(m0.store[k]["pose"])
        Mk[k] = (Tk, Mscw if k == curr else Tk @ tr.inv4(Tc) @ Mscw)
        worst = max(worst, tr.err(L["S_uncorr"][j], Tk), tr.err(L["S_corr"][j], Mk[k][1]))
        s = LD(L["S_corr"][j][7])
        P = Mk[k][1].copy()
        P[:3, :3], P[:3, 3] = P[:3, :3] / s, P[:3, 3] / s
        worst = max(worst, float(np.abs(_T4(m.store[k]["pose"]) - P).max()))
    for p, k in zip(L["cp_id"], L["cp_ref"]):
        kk, f = m0.carriers(p)[0] if m0.carriers(p)[0][0] == k else [c for c in m0.carriers(p) if c[0] == k][0]
        old = np.array([*m0.store[kk]["points"][f], 1.0], LD)
        new = tr.inv4(Mk[k][1]) @ (Mk[k][0] @ old)
        for jj, i in m.carriers(p):
            worst = max(worst, float(np.abs(np.array(m.store[jj]["points"][i], LD) - new[:3]).max()))
    return worst


def test_model_against_longdouble_matrices():
    worst = 0.0
    for script, curr, scale in ((ci.propagate_scene(bad=(3,)), ci.CURR, 1.1), (ci.lonely_scene(), 1, 1.0),
                                (ci.connections_scene().script(), ci.C_CURR, 1.0)):
        Scw = SCW(pi.HAND_POSES[curr], scale)
        m0, m = ci.run_model(script), ci.run_model(script)
        L = m.propagate_loop(curr, Scw)
        worst = max(worst, longdouble_errors(m0, m, L, Scw, curr))
    print("model against longdouble matrices:", worst)
    assert worst <= ci.MODEL_LONGDOUBLE_WORST and worst >= 0.2 * ci.MODEL_LONGDOUBLE_WORST   # (the recorded figure is the measured one)


# ---- the chains' scenes: the model alone shows a family-A edge and moved points -----------------------------------------------
def seeded_chain_model(exp=None, log=None):
    """-> (runner, model) of the seeded 12 x 256 scene at its first fuse, with the loop-side key-frame behind it"""
    import fuse_inputs as fi
    import loop_fuse_inputs as lfi
    mr = lfi.ModelRunner(fi.SCENE_CAPS, exp=exp, log=log, max_recent=fi.SCENE_RECENT, max_candidates=fi.SCENE_CANDIDATES,
                         max_corrected=ci.CHAIN_LC_CAPS[0], max_loop_points=lfi.CHAIN_LOOP_POINTS, model=ci.ChainModel)
    mr.m.enable_loop_correct(*ci.CHAIN_LC_CAPS)
    return mr, mr.m


def test_the_seeded_chain_shows_a_family_a_edge_and_moved_points():
    import fuse_inputs as fi
    mr, m = seeded_chain_model()
    for s in fi.seeded_chain():
        mr.step(s)
        if s[0] == "neighbors":
            break
    for s in ci.seeded_old_keyframe(m):
        mr.step(s)
    cur = ci.SEEDED_MATCH - 1
    L, rows, w = ci.model_chain(m, cur, ci.chain_scw(m, cur), ci.seeded_loop_ids(m, 0), ci.SEEDED_MATCH, block=lambda mm: ci.seeded_block(mm, cur))
    assert w is not None and m.pg_record["n_a"] >= 1 and m.lc_record["n_rows_moved"] >= 1 and m.lc_record["n_cp"] > 100
    assert ci.SEEDED_MATCH not in L["corr_kf"] and rows[cur] == [ci.SEEDED_MATCH] and m.conn.W[cur][ci.SEEDED_MATCH] >= 100
    assert m.loop_fuse_result()["totals"][0] > 20 and m.sticky == 0


def test_the_loop_scene_chain_shows_a_family_a_edge_and_moved_points(orc):
    """compute_sim3's model (tests/loop_sim3_ref.py) accepts the scene; the chain behind it on the store model"""
    import loop_sim3_inputs as ls
    sc = ls.scene(ci.LOOP_SCENE)
    r = ls.run_model(orc, sc).result()
    assert r["state"] == lr.ACCEPTED and len(r["loop_point_ids"]) > 100
    m = ci.scene_model(sc)
    L, rows, w = ci.model_chain(m, sc["current"], lr.scw8_from13(r["Scw"]), [int(x) for x in r["loop_point_ids"]], r["match_kf"])
    assert w is not None and m.pg_record["n_a"] >= 1 and m.lc_record["n_rows_moved"] >= 1
    assert r["match_kf"] in rows[sc["current"]] and m.conn.W[sc["current"]][r["match_kf"]] >= 100
    assert m.loop_fuse_result()["totals"][3] > 100 and m.sticky == 0
