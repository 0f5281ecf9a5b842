"""The store's loop pose graph on the device against the model tests/pose_graph_store_ref.py, through
the binding: vo_kfstore_pose_graph_window in both forms (index arrays and the record exact; quats, trans, scales and the
measurements byte for byte, and within ten times the model's own longdouble error of the matrix formulation),
vo_kfstore_pose_graph_apply and vo_kfstore_pose_graph against Optimizer.solvePoseGraphLoop on the window's own bytes followed
by the model's write-back (every byte of the store identical) and against the oracle within test_gpu_ba.py's pose-graph
bounds, the invariant of the re-anchoring, a drifted loop, the chain behind compute_sim3, and the misuse of every entry point."""
import numpy as np
import pytest

import loop_sim3_inputs as ls
import pose_graph_store_inputs as pi
import pose_graph_store_ref as pr
import test_gpu_local_ba_store as lb
import test_pose_graph_store_ref as tr

pytestmark = pytest.mark.gpu

BOUND = 10 * pi.MODEL_LONGDOUBLE_WORST
MAX_CORR, MAX_CP = 16, 64


class Dev(lb.Dev):
    def __init__(self, vo, K, NK, caps=pi.CAPS, max_edges=pi.MAX_EDGES, dev=False, pose_graph=True):
        super().__init__(vo, K, NK, caps, dev)
        if pose_graph:
            self.s.enable_pose_graph(max_edges, MAX_CORR, MAX_CP)

    def step(self, s):
        if s[0] == "loop_edge":
            self.s.add_loop_edge(s[1], s[2])
        elif s[0] == "refs":
            self.s.set_point_refs(s[1], np.asarray(s[2], np.int32))
        else:
            super().step(s)


def _build(vo, case, dev=False):
    K = sum(1 for s in case["script"] if s[0] == "insert")
    d = Dev(vo, K, case.get("NK", pi.NK_HAND), max_edges=case.get("max_edges", pi.MAX_EDGES), dev=dev)
    mr = pi.ModelRunner(max_edges=case.get("max_edges", pi.MAX_EDGES), exp=lb._exp(vo), log=lb._log(vo))
    for s in case["script"]:
        d.step(s), mr.step(s)
    return d, mr.m


def _window(d, case, dev):
    inp, keep = case["inp"], None
    if dev:
        import torch
        keep = inp = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in case["inp"].items()}
    d.s.pose_graph_window(case["curr"], case["match"], inp)
    got = d.s.pose_graph_window_result()
    return got, keep


def _same_window(got, m, want):
    rec = got["record"]
    assert {k: rec[k] for k in pr.PG_RECORD} == m.pg_record
    if want is None:
        assert all(len(v) == 0 for k, v in got.items() if k not in ("record", "fixed"))
        return
    for key, w in want.items():
        assert got[key].dtype == w.dtype and got[key].shape == w.shape and got[key].tobytes() == w.tobytes(), key


CASES = pi.hand_cases() + [pi.wide_case(), pi.drifted_loop()]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_window_equals_the_model(vo, case):
    dev = bool(case.get("dev"))
    d, m = _build(vo, case, dev)
    want = m.pg_window(case["curr"], case["match"], case["inp"])
    got, keep = _window(d, case, dev)
    assert {k: got["record"][k] for k in case["want"]} == case["want"]
    _same_window(got, m, want)
    assert d.s.connections_status() == m.sticky == case.get("sticky", 0)
    if want is not None:   # and against the matrix formulation in longdouble, with the DEVICE's arrays
        worst = tr.longdouble_errors(m, case, got)
        print(case["name"], "device against longdouble matrices:", worst)
        assert worst <= BOUND
        for k in range(len(m.store)):
            assert d.s.loop_edges(k) == sorted(m.loop_edges[k])
            assert d.s.cull_state(k)["locked"] == m.locked[k]


def test_both_forms_give_the_same_bytes(vo):
    case = [c for c in CASES if c["name"] == "f_all_together"][0]
    out = []
    for dev in (False, True):
        d, m = _build(vo, case, dev)
        got, keep = _window(d, case, dev)
        out.append(got)
    for k in out[0]:
        if k not in ("record", "fixed"):
            assert out[0][k].tobytes() == out[1][k].tobytes(), k
    assert out[0]["record"] == out[1]["record"] and out[0]["record"]["n_edges"] > 10


def _all_states_equal(d, m, where):
    lb._same_store(d, m, where)


def test_apply_equals_the_model_and_keeps_equal_rows_equal(vo):
    case = [c for c in CASES if c["name"] == "f_all_together"][0]
    d, m = _build(vo, case)
    want = m.pg_window(case["curr"], case["match"], case["inp"])
    got, _ = _window(d, case, False)
    q, t = tr.nudged(want)
    d.s.pose_graph_apply(q, t)
    m.pg_apply(q, t)
    _all_states_equal(d, m, "apply")
    rec = d.s.pose_graph_window_result()["record"]
    assert {k: rec[k] for k in pr.PG_RECORD} == m.pg_record and rec["n_unanchored"] == 48 and rec["n_points_moved"] > 600
    assert d.s.connections_status() == m.sticky == 0
    for p in pi.H + pi.L0:   # every live feature that carries a point ends with the same bytes
        rows = {d.state(j)["points"][i].tobytes() for j, i in m.carriers(p)}
        assert len(rows) == 1, p
    with pytest.raises(vo.VoError, match="status -1"):   # one window, one apply
        d.s.pose_graph_apply(q, t)


def _graph(w):
    return dict(quats=w["quats"], trans=w["trans"], scales=w["scales"], e_i=w["e_i"], e_j=w["e_j"], q_meas=w["q_meas"], t_meas=w["t_meas"],
                s_meas=w["s_meas"], fixed=w["fixed"])


@pytest.mark.parametrize("name", ["g_all_together_device_form", "k_wide", "l_drifted_loop"])
def test_composed_call_against_the_plain_solver_and_the_oracle(vo, orc, name):
    case = [c for c in CASES if c["name"] == name][0]
    d, m = _build(vo, case)
    want = m.pg_window(case["curr"], case["match"], case["inp"])
    got, _ = _window(d, case, False)
    _same_window(got, m, want)
    before = [d.state(k) for k in range(len(m.store))]
    # the same solver on the same bytes, then the model's write-back
    q, t, s = vo.Optimizer.solvePoseGraphLoop(_graph(got))
    s2 = d.s.pose_graph(case["curr"], case["match"], case["inp"])
    assert (s2.iterations, s2.accepted, s2.termination) == (s.iterations, s.accepted, s.termination) and s.iterations >= 1
    Srw, Swr = m.pg_apply(q, t)
    _all_states_equal(d, m, name)
    # against the oracle on the same window: test_gpu_ba.py::test_pose_graph_matches_oracle's bounds
    oq, ot, os_ = orc.pose_graph_solve(_graph(got))
    assert (s.iterations, s.accepted, s.termination) == (os_.iterations, os_.accepted, os_.termination)
    assert abs(s.final_cost - os_.final_cost) <= 1e-10 * os_.final_cost
    assert np.abs(q - oq).max() < 1e-9 and np.abs(t - ot).max() < 1e-8
    # the invariant no model enters: a moved point keeps its coordinates in its anchor key-frame, Srw_old * p_old == Siw_new * p_new
    nodes = [int(k) for k in got["node_kf"]]
    cp = {int(i): int(r) for i, r in zip(case["inp"]["cp_id"], case["inp"]["cp_ref"])}
    worst, moved = 0.0, 0
    for k in nodes:
        after = d.state(k)
        for f in np.nonzero(before[k]["flags"] & 1)[0]:
            idm = cp.get(int(before[k]["ids"][f]), int(before[k]["ref"][f]))
            if idm not in nodes:
                assert after["points"][f].tobytes() == before[k]["points"][f].tobytes()
                continue
            i = nodes.index(idm)
            qn = q[i] / np.linalg.norm(q[i])
            old = tr.M([*got["quats"][i], *got["trans"][i], got["scales"][i]]) @ np.array([*before[k]["points"][f], 1.0], tr.LD)
            new = tr.M([*qn, *t[i], got["scales"][i]]) @ np.array([*after["points"][f], 1.0], tr.LD)
            worst, moved = max(worst, float(np.abs(old - new).max())), moved + 1
    print(name, "anchor coordinates before against after:", worst, "over", moved)
    assert moved >= 100 and worst <= BOUND
    if name == "l_drifted_loop":
        # ONE cycle of N equally weighted edges: the least-squares optimum spreads the inconsistency evenly, so the loop edge keeps
        # 1 / N of the gap the drifted estimates leave (twice that: the solver's residual is not this matrix distance)
        N, Tcm = case["N"], case["Tcm"]
        T4 = lambda T: np.vstack([np.hstack([T[:9].reshape(3, 3), T[9:].reshape(3, 1)]), [0, 0, 0, 1]])
        gap = lambda Tc, Tm: float(np.abs(Tc @ np.linalg.inv(Tm) - Tcm).max())
        g0 = gap(T4(before[N - 1]["pose"]), T4(before[0]["pose"]))
        g1 = gap(T4(d.state(N - 1)["pose"]), T4(d.state(0)["pose"]))
        print("loop gap before", g0, "after", g1)
        assert g0 > 0.05 and g1 <= 2 * g0 / N
        assert d.state(0)["pose"].tobytes() != b"" and np.abs(d.state(0)["pose"] - before[0]["pose"]).max() < 1e-15   # the fixed node


def test_solver_refusal_leaves_every_byte(vo):
    """what vo_pose_graph_solve itself refuses -- free scales, an edge i == j, more than 6 (nodes - 1) <= 4096 unknowns -- a window
    never hands it: scales are fixed, j != k is part of every family and the node limit overflows the window first.  So the two
    refusals in front of the solver stand for it: an overflowed window (status -4) and an empty one (status -1)"""
    case = [c for c in CASES if c["name"] == "j_one_edge_too_many"][0]
    d, m = _build(vo, case)
    before = [d.state(k) for k in range(len(m.store))]
    with pytest.raises(vo.VoError, match="status -4"):
        d.s.pose_graph(case["curr"], case["match"], case["inp"])
    case = [c for c in CASES if c["name"] == "i_node_without_a_pose"][0]
    d2, m2 = _build(vo, case)
    with pytest.raises(vo.VoError, match="status -1"):
        d2.s.pose_graph(case["curr"], case["match"], case["inp"])
    for k, b in enumerate(before):
        a = d.state(k)
        for key in b:
            assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (k, key)


def test_misuse(vo):
    case = [c for c in CASES if c["name"] == "f_all_together"][0]
    # a store without the block refuses every entry point
    d0 = Dev(vo, 8, pi.NK_HAND, pose_graph=False)
    for s in case["script"]:
        if s[0] != "loop_edge":
            d0.step(s)   # (the reference key-frames are local BA's)
    for call in (lambda: d0.s.add_loop_edge(0, 1), lambda: d0.s.loop_edges(0), lambda: d0.s.pose_graph_window(6, 2, case["inp"]),
                 lambda: d0.s.pose_graph_window_result(), lambda: d0.s.pose_graph_apply(np.zeros((7, 4)), np.zeros((7, 3))),
                 lambda: d0.s.pose_graph(6, 2, case["inp"])):
        with pytest.raises(vo.VoError, match="status -1"):
            call()
    with pytest.raises(vo.VoError, match="status -1"):   # not on a store that holds key-frames
        d0.s.enable_pose_graph(8, 8, 8)
    s1 = vo.KeyFrameStore(4, 16)
    with pytest.raises(vo.VoError, match="status -1"):   # not without local BA
        s1.enable_pose_graph(8, 8, 8)
    d, m = _build(vo, case)
    with pytest.raises(vo.VoError, match="status -1"):   # capacities below 1 (and a second enable on a filled store)
        Dev(vo, 2, 16, pose_graph=False).s.enable_pose_graph(0, 1, 1)
    with pytest.raises(vo.VoError, match="status -1"):   # no window yet
        d.s.pose_graph_apply(np.zeros((7, 4)), np.zeros((7, 3)))
    before = [d.state(k) for k in range(8)]
    inp = case["inp"]
    swap = lambda a: np.concatenate([a[1:2], a[0:1], a[2:]])
    bad_inputs = [dict(inp, corr_kf=swap(inp["corr_kf"])), dict(inp, corr_kf=np.array([5, 6, 8], np.int32)), dict(inp, lc_kf=swap(inp["lc_kf"])),
                  dict(inp, lc_kf=np.array([0, 1, 9, 0], np.int32)), dict(inp, cp_id=np.array([-1], np.int32)), dict(inp, cp_ref=np.array([8], np.int32)),
                  dict(inp, lc_start=np.array([0, 0, 4, 3], np.int32)),
                  dict(inp, cp_id=np.array([7, 7], np.int32), cp_ref=np.array([1, 1], np.int32))]
    for b in bad_inputs:
        with pytest.raises(vo.VoError, match="status -1"):
            d.s.pose_graph_window(6, 2, b)
    for cur, mat in ((8, 2), (6, -1)):
        with pytest.raises(vo.VoError, match="status -1"):
            d.s.pose_graph_window(cur, mat, inp)
    many = pr.make_inputs({}, {}, {i: 0 for i in range(MAX_CP + 1)})
    with pytest.raises(vo.VoError, match="status -4"):   # more corrected points than the block holds
        d.s.pose_graph_window(6, 2, many)
    # the device form sees the same faults on the device: EMPTY and the sticky bit
    import torch
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in bad_inputs[0].items()}
    d.s.pose_graph_window(6, 2, t)
    rec = d.s.pose_graph_window_result()["record"]
    assert rec["status"] == pr.EMPTY and d.s.connections_status() == 1
    # apply after a write: the generation word has moved
    d.s.pose_graph_window(6, 2, inp)
    w = d.s.pose_graph_window_result()
    d.s.set_erase_lock(0, False)
    with pytest.raises(vo.VoError, match="status -1"):
        d.s.pose_graph_apply(w["quats"], w["trans"])
    # loop-edge capacity, a == b, numbers outside the store; nothing written
    for a, b in ((0, 0), (0, 8), (-1, 0)):
        with pytest.raises(vo.VoError, match="status -1"):
            d.s.add_loop_edge(a, b)
    for k in range(8):
        after = d.state(k)
        for key in before[k]:
            assert np.asarray(after[key]).tobytes() == np.asarray(before[k][key]).tobytes(), (k, key)
    d9 = Dev(vo, 11, 16)
    for s in pi.Scene([pi.HAND_POSES[0]] * 11).script(update=False):
        d9.step(s)
    for b in range(1, 9):
        d9.s.add_loop_edge(0, b)
    d9.s.add_loop_edge(3, 0)   # a repeat changes nothing
    with pytest.raises(vo.VoError, match="status -4"):
        d9.s.add_loop_edge(9, 0)
    assert d9.s.loop_edges(0) == list(range(1, 9)) and d9.s.loop_edges(9) == [] and d9.s.cull_state(9)["locked"] == 0
    assert d9.s.loop_edges(3) == [0] and d9.s.cull_state(3)["locked"] == 1


def _loop_store(vo, sc):
    """loop_sim3_inputs.build_device with the pose-graph block"""
    store = sc["store"]
    s = vo.KeyFrameStore(len(store), ls.NK)
    s.enable_connections()
    s.enable_culling()
    s.enable_mapping(ls.CAM6, ls.SF, 50000)
    s.enable_local_ba(*ls.BA_CAPS)
    s.enable_pose_graph(256, MAX_CORR, MAX_CP)
    s.enable_point_upkeep(ls.MAX_RECENT)
    s.enable_fuse(ls.BOUNDS, ls.FUSE_CANDIDATES)
    s.enable_loop(**sc["caps"])
    for k, kf in enumerate(store):
        s.insert(dict(angle=kf["angle"], desc=kf["desc"], flags=kf["flags"], points=kf["points"], ids=kf["ids"], point_desc=kf["point_desc"],
                      min_dist=kf["min_dist"], max_dist=kf["max_dist"], nodes=kf["nodes"], bad=kf["bad"]))
        s.set_keypoints(k, kf["octave"], kf["depth"], kf["uright"])
        s.set_keypoint_xy(k, np.stack([kf["x"], kf["y"]], 1))
        if kf["pose"] is not None:
            s.set_pose(k, kf["pose"])
        s.set_normals(k, kf["normals"])
        s.set_point_refs(k, np.full(len(kf["ids"]), k, np.int32) * (np.asarray(kf["flags"]) & 1) - (1 - (np.asarray(kf["flags"]) & 1)))
    s.update_connections(list(range(len(store))))
    return s


def test_chain_behind_compute_sim3(vo):
    """compute_sim3 -> correctLoop's arrays made on the host -> pose_graph -> add_loop_edge -> update_connections; a second
    closure then sees the first as a family-C edge, both ways"""
    sc = ls.scene("accepted")
    s = _loop_store(vo, sc)
    cur = sc["current"]
    s.compute_sim3(cur, sc["cand"], sc["rand"], ls.RAND_MAX, sc["fix_scale"], sc["max_rounds"])
    r = s.loop_result()
    assert r["state"] == s.LOOP_ACCEPTED
    match = r["match_kf"]
    T, _ = s.pose(cur)
    Scw = r["Scw"]
    S_corr = pr.from_pose(list(Scw[:12]))
    S_corr = S_corr[:7] + [float(Scw[12])]
    inp = pr.make_inputs({cur: (S_corr, pr.from_pose(list(T)))}, {cur: [match]}, {})
    summary = s.pose_graph(cur, match, inp)
    rec = s.pose_graph_window_result()["record"]
    assert rec["status"] == pr.OK and rec["n_c"] == 0 and rec["n_points_moved"] > 0 and summary.iterations >= 1
    s.add_loop_edge(cur, match)
    s.update_connections([cur])
    assert s.loop_edges(cur) == [match] and s.loop_edges(match) == [cur] and s.connections_status() == 0
    # a second closure, from a key-frame number above both: the first closure is now an earlier loop edge
    T2, _ = s.pose(cur)
    s.pose_graph_window(cur, 0, pr.make_inputs({cur: (pr.from_pose(list(T2)), pr.from_pose(list(T2)))}, {}, {}))
    w = s.pose_graph_window_result()
    kf = [int(k) for k in w["node_kf"]]
    pairs = {(kf[i], kf[j]) for i, j in zip(w["e_i"], w["e_j"])}
    assert w["record"]["n_c"] == 1 and (cur, match) in pairs   # (match -> cur needs cur < curr: it is curr itself)
    s.close()


ctx = lb.ctx   # (test_gpu_local_map's module fixture: relocalised frames whose slot ids the chain's store is keyed by)


def test_chain_ends_in_the_local_map(vo, ctx):
    """pose_graph -> add_loop_edge -> update_connections -> vo_tracker_build_local_map.  Store A (the hand case with everything
    in it, its ids mapped one to one into the id space of relocalised frames) goes through the chain on the device; store B is
    a plain store holding what A holds afterwards, its graph set from A's connections.  The local map built from either is
    byte-identical, and it lists positions the write-back wrote"""
    lm = lb.lm
    case = [c for c in CASES if c["name"] == "f_all_together"][0]
    rng = np.random.default_rng(5)
    max_local = 4000
    trk_a, _, slots, _ = lm._relocalized(vo, ctx, max_local)
    trk_b, _, _, _ = lm._relocalized(vo, ctx, max_local)
    live = rng.permutation(np.unique(slots[slots >= 0]))
    mine = sorted({p for s in case["script"] if s[0] == "insert" for p in s[1]})
    assert len(live) >= len(mine)
    to = {p: int(live[i]) for i, p in enumerate(mine)}
    script = [(s[0], [to[p] for p in s[1]]) + tuple(s[2:]) if s[0] == "insert" else s for s in case["script"]]
    cp = sorted((to[int(i)], int(r)) for i, r in zip(case["inp"]["cp_id"], case["inp"]["cp_ref"]))
    inp = dict(case["inp"], cp_id=np.array([i for i, _ in cp], np.int32), cp_ref=np.array([r for _, r in cp], np.int32))
    a = Dev(vo, 8, pi.NK_HAND)
    for s in script:
        a.step(s)
    before = [a.state(k) for k in range(8)]
    a.s.pose_graph(case["curr"], case["match"], inp)
    a.s.add_loop_edge(case["curr"], case["match"])
    a.s.update_connections([case["curr"]])
    assert a.s.connections_status() == 0
    held = [a.state(k) for k in range(8)]
    moved = np.concatenate([h["ids"][(h["flags"] & 1).astype(bool) & (h["points"] != b["points"]).any(1)] for h, b in zip(held, before)])
    assert len(moved) >= 600
    b = vo.KeyFrameStore(8, pi.NK_HAND)
    erased = [a.s.cull_state(k)["erased"] for k in range(8)]
    for k, s in enumerate(s for s in script if s[0] == "insert"):
        arr = lb.li.insert_arrays(s)
        b.insert(dict(arr, flags=held[k]["flags"] * (1 - erased[k]), ids=held[k]["ids"], points=held[k]["points"], point_desc=held[k]["point_desc"],
                      min_dist=held[k]["min_dist"], max_dist=held[k]["max_dist"], bad=held[k]["bad"]))
        b.set_normals(k, held[k]["normals"])
    conn = [a.s.connections(k) for k in range(8)]
    b.set_graph_batch(0, [[] if erased[k] else g["ordered"][:10] for k, g in enumerate(conn)], [g["children"] for g in conn], [g["parent"] for g in conn])
    keys = lm.ARRAYS + ("LOCAL_KEYFRAMES", "LOCAL_N_KEYFRAMES", "LOCAL_N_POINTS", "LOCAL_REF_KF")
    got = []
    for trk, store in ((trk_a, a.s), (trk_b, b)):
        trk.build_local_map(store)
        trk.results()
        got.append({key: trk.get(getattr(trk, key)) for key in keys})
    for key in keys:
        assert got[0][key].tobytes() == got[1][key].tobytes(), key
    assert got[0]["LOCAL_N_KEYFRAMES"].sum() > 0 and np.isin(got[0]["LOCAL_POINT_IDS"], moved).sum() >= 50
    trk_a.close()
    trk_b.close()
