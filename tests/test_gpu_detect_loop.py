"""Loop detection on the device against the model tests/detect_loop_ref.py, through the binding:
vo_kfstore_detect_loop with its result calls, compute_sim3_detected, release_loop_locks and the composed loop_closing_step.
Nothing has a tolerance: the record, the candidates, the enough list, the groups (counts and member bytes), the erased / locked /
pending columns, the sticky word and the database's neighbour rows are compared as integers or bytes after EVERY step of a
case's script, because the groups carry over from call to call.  tests/test_detect_loop_ref.py (CPU) holds the hand tables."""
import ctypes as C

import numpy as np
import pytest

import connections_inputs as cin
import detect_loop_inputs as di
import detect_loop_ref as dr
import loop_correct_inputs as ci
import loop_merge_inputs as mi
import loop_sim3_inputs as ls

pytestmark = pytest.mark.gpu

LOOP_CAPS = dict(max_candidates=4, max_loop_points=64, max_rand=64)


class Dev:
    """a world on the device: the store with every layer detect_loop needs, and the database"""

    def __init__(self, vo, world, D=4, G=8, detect=True, db_size=None):
        K = world.K
        self.s = s = vo.KeyFrameStore(K, di.NK)
        s.enable_connections(), s.enable_culling(), s.enable_mapping(ls.CAM6, ls.SF, 50000), s.enable_local_ba(*ls.BA_CAPS)
        s.enable_pose_graph(64, 8, 64), s.enable_point_upkeep(ls.MAX_RECENT), s.enable_fuse(ls.BOUNDS, 64), s.enable_loop(**LOOP_CAPS)
        if detect:
            s.enable_detect_loop(D, G)
        self.db = vo.KeyFrameDatabase(di.N_WORDS, K, 16, 1)
        for k in range(K):
            s.insert(cin.device_arrays(world.store[k]))
        for k in range(K if db_size is None else db_size):
            self.db.insert(*world.vector(k))
        s.update_connections(world.update_order)

    def step(self, st):
        s = self.s
        if st[0] == "detect":
            s.detect_loop(self.db, st[1], st[2])
        elif st[0] == "bad":
            s.set_bad(st[1])
        elif st[0] == "erase":
            s.erase_keyframe(st[1])
        elif st[0] == "lock":
            s.set_erase_lock(st[1], st[2])
        elif st[0] == "edge":
            s.add_loop_edge(st[1], st[2])
        else:
            raise ValueError(st)


def _same(s, db, m, where):
    """everything the layer writes, device against model; the sticky word is read and cleared on both sides"""
    K = len(m.kfs)
    got, want = s.detect_loop_result(), m.result()
    for key in dr.DL_RECORD + ("candidates", "enough"):
        assert got[key] == want[key], (where, key, got, want)
    assert got["min_score"].tobytes() == np.int32(want["min_score_bits"]).tobytes()
    counts, members = s.detect_loop_groups()
    wc, wm = m.groups(K)
    assert counts == wc and members.tobytes() == wm.tobytes(), (where, counts, wc, m.groups_as_sets())
    state = [s.cull_state(k) for k in range(K)]
    assert [(c["erased"], c["locked"], c["pending"]) for c in state] == list(zip(m.cull.erased, m.cull.locked, m.cull.pending)), (where, state)
    assert [db.neighbors(k) for k in range(K)] == [[n.index for n in m.db.kfs[k].neighbors] for k in range(K)], where
    assert s.connections_status() == m.sticky, where
    m.sticky = 0


def _run(vo, world, script, D=4, G=8):
    d, m = Dev(vo, world, D, G), di.build_model(world, D, G)
    out = []
    for st in script:
        d.step(st), di.model_step(m, st)
        _same(d.s, d.db, m, st)
        if st[0] == "detect":
            out.append((m.record["outcome"], m.groups_as_sets(), m.result()["enough"]))
    return d, m, out


# ---- the hand tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", di.HAND_CASES)
def test_hand_cases(vo, name):
    c = di.hand_cases()[name]
    d, m, got = _run(vo, c["world"], c["script"], c["D"], c["G"])
    assert got == [(o, [(sorted(g), n) for g, n in groups], list(enough)) for o, groups, enough in c["want"]]


def test_three_bitset_words_with_a_ragged_tail(vo):
    w = di.big_world()
    assert w.K == 130
    d, m = Dev(vo, w), di.build_model(w, 4, 8)
    for i, cur in enumerate((100, 101, 102, 103)):
        st = ("detect", cur, 0)
        d.step(st), di.model_step(m, st)
        _same(d.s, d.db, m, st)
        if i == 0:
            counts, members = d.s.detect_loop_groups()
            assert set(np.flatnonzero(members[0])) == {63, 64, 127, 128, 129} and set(np.flatnonzero(members[1])) == {0, 64, 128, 129}
    res = d.s.detect_loop_result()
    assert res["outcome"] == dr.DETECTED and res["candidates"] == [64, 129] == res["enough"]


# ---- capacities, locks, refusals ---------------------------------------------------------------------------------------------------
def test_overflow_of_candidates_and_of_groups(vo):
    w = di.overflow_world()
    S = vo.KeyFrameStore
    d, m, got = _run(vo, w, [("detect", 12, 0)], D=1, G=8)
    assert got == [(dr.OVERFLOW, [], [])] and d.s.detect_loop_result()["n_candidates"] == 2
    d, m, got = _run(vo, w, [("detect", 12, 0), ("detect", 13, 0), ("detect", 12, 0)], D=2, G=2)
    assert [g[0] for g in got] == [dr.NOT_CONSISTENT, dr.OVERFLOW, dr.NOT_CONSISTENT] and got[1][1] == [] and len(got[2][1]) == 2
    # (_same has compared the sticky word on every step: VO_KFSTORE_DETECT_CAPACITY behind the overflows, on both sides)
    d2 = Dev(vo, w, 1, 8)
    d2.s.detect_loop(d2.db, 12, 0)
    assert d2.s.connections_status() == S.CONNECTIONS_DETECT_CAPACITY == 512 and d2.s.connections_status() == 0
    d, m, got = _run(vo, w, [("detect", 12, 0), ("detect", 13, 0)], D=2, G=3)
    assert got[1][0] == dr.NOT_CONSISTENT and [n for _, n in got[1][1]] == [1, 1, 0]


def test_a_loop_edge_keeps_the_lock_on_every_outcome(vo):
    w = di.standard_world({12: "A", 13: ""})
    script = [("edge", 12, 5), ("edge", 13, 7), ("detect", 12, 0), ("detect", 13, 0), ("detect", 12, 5)]
    d, m, got = _run(vo, w, script)
    assert [g[0] for g in got] == [dr.NOT_CONSISTENT, dr.NO_CANDIDATES, dr.GATED]
    assert d.s.cull_state(12)["locked"] == 1 and d.s.cull_state(13)["locked"] == 1
    d, m, got = _run(vo, di.overflow_world(), [("edge", 12, 5), ("detect", 12, 0)], D=1)
    assert got[0][0] == dr.OVERFLOW and d.s.detect_loop_result()["locked"] == 1
    one = di.standard_world({k: "A" for k in di.CURRENTS})
    d, m, got = _run(vo, one, [("detect", k, 0) for k in di.CURRENTS])
    assert got[-1][0] == dr.DETECTED and [d.s.cull_state(k)["locked"] for k in di.CURRENTS] == [0, 0, 0, 1]


def test_pending_is_reported_and_nothing_is_erased(vo):
    w = di.standard_world({k: "A" for k in di.CURRENTS})
    d, m, got = _run(vo, w, [("lock", 13, True), ("erase", 13), ("detect", 13, 0)])
    res = d.s.detect_loop_result()
    assert (res["outcome"], res["locked"], res["pending"]) == (dr.NOT_CONSISTENT, 0, 1)
    assert d.s.cull_state(13) == dict(erased=0, locked=0, pending=1)


def test_an_erased_current(vo):
    w = di.standard_world({k: "A" for k in di.CURRENTS})
    d, m, got = _run(vo, w, [("detect", 12, 0), ("erase", 14), ("detect", 14, 0), ("detect", 13, 0)])
    assert [g[0] for g in got] == [dr.NOT_CONSISTENT, dr.NONE, dr.NOT_CONSISTENT] and got[1][1] == got[0][1] and got[2][1] == [(di.G123, 1)]
    assert d.s.cull_state(14) == dict(erased=1, locked=0, pending=0)


def test_the_refresh_overwrites_set_neighbors(vo):
    w = di.standard_world({k: "A" for k in di.CURRENTS})
    d, m = Dev(vo, w), di.build_model(w, 4, 8)
    d.db.set_neighbors(2, [5, 6]), m.db.set_neighbors(2, [5, 6])
    assert d.db.neighbors(2) == [5, 6]
    st = ("detect", 12, 3)                                    # GATED: returns before the refresh
    d.step(st), di.model_step(m, st)
    _same(d.s, d.db, m, st)
    assert d.db.neighbors(2) == [5, 6]
    st = ("detect", 12, 0)
    d.step(st), di.model_step(m, st)
    _same(d.s, d.db, m, st)
    assert sorted(d.db.neighbors(2)) != [5, 6] and d.db.neighbors(2) == d.s.connections(2)["ordered"][:10]


def test_refusals_and_return_codes(vo):
    L = vo.lib()
    w = di.standard_world({k: "A" for k in di.CURRENTS})
    rand = np.arange(6, dtype=np.int32)
    plain = Dev(vo, w, detect=False)                                           # no enable_detect_loop
    h, dbh = plain.s._h, plain.db._h
    k32 = C.c_int32(0)
    for rc in (L.vo_kfstore_detect_loop(h, dbh, 12, 0), L.vo_kfstore_detect_loop_result(h, None, None, None),
               L.vo_kfstore_detect_loop_groups(h, C.byref(k32), None, None),
               L.vo_kfstore_compute_sim3_detected(h, 1, 6, vo._p(rand), ls.RAND_MAX, 1),
               L.vo_kfstore_compute_sim3_detected_dev(h, 1, 0, None, ls.RAND_MAX, 1), L.vo_kfstore_release_loop_locks(h),
               L.vo_kfstore_loop_locks_result(h, None, None, None), L.vo_kfstore_set_last_loop_keyframe(h, 3),
               L.vo_kfstore_get_last_loop_keyframe(h, C.byref(k32)),
               L.vo_kfstore_loop_closing_step(h, dbh, 12, 1, 6, vo._p(rand), ls.RAND_MAX, 1, C.c_float(4.0), 20, None, None),
               L.vo_kfstore_enable_detect_loop(h, 4, 8)):                      # (the last: the store holds key-frames)
        assert rc == -1
    assert L.vo_kfstore_enable_detect_loop(None, 4, 8) == -1
    e = vo.KeyFrameStore(4, di.NK)
    e.enable_connections(), e.enable_culling(), e.enable_mapping(ls.CAM6, ls.SF, 50000), e.enable_local_ba(*ls.BA_CAPS)
    e.enable_point_upkeep(ls.MAX_RECENT), e.enable_fuse(ls.BOUNDS, 64), e.enable_loop(**LOOP_CAPS)
    assert L.vo_kfstore_enable_detect_loop(e._h, 4, 8) == -1                   # no enable_pose_graph
    e.enable_pose_graph(64, 8, 64)
    for D, G in ((0, 8), (4, 3), (4, 1025)):
        assert L.vo_kfstore_enable_detect_loop(e._h, D, G) == -1
    assert L.vo_kfstore_enable_detect_loop(e._h, 4, 8) == 0 and L.vo_kfstore_enable_detect_loop(e._h, 4, 8) == 0
    d = Dev(vo, w)
    h, dbh = d.s._h, d.db._h
    assert L.vo_kfstore_compute_sim3_detected(h, 1, 6, vo._p(rand), ls.RAND_MAX, 1) == -1     # no detect_loop yet
    for rc in (L.vo_kfstore_detect_loop(h, dbh, 16, 0), L.vo_kfstore_detect_loop(h, dbh, -1, 0), L.vo_kfstore_detect_loop(h, dbh, 12, -1),
               L.vo_kfstore_detect_loop(h, None, 12, 0), L.vo_kfstore_set_last_loop_keyframe(h, -1)):
        assert rc == -1
    short = Dev(vo, w, db_size=15)                                             # the database one key-frame behind the store
    assert L.vo_kfstore_detect_loop(short.s._h, short.db._h, 12, 0) == -1
    m = di.build_model(w, 4, 8)
    _same(d.s, d.db, m, "nothing was enqueued by a refused call")
    d.s.detect_loop(d.db, 12, 0)
    assert L.vo_kfstore_compute_sim3_detected(h, 1, 65, vo._p(np.zeros(65, np.int32)), ls.RAND_MAX, 1) == -4   # more than max_rand
    assert L.vo_kfstore_compute_sim3_detected(h, 1, 6, None, ls.RAND_MAX, 1) == -1
    d.s.last_loop_keyframe = 7
    assert d.s.last_loop_keyframe == 7


def test_a_store_with_the_layer_unused_behaves_as_one_without(vo):
    w = di.min_score_world()
    out = []
    for detect in (True, False):
        d = Dev(vo, w, detect=detect)
        for st in (("bad", 10), ("lock", 4, True), ("erase", 4), ("erase", 3), ("edge", 12, 2)):
            d.step(st)
        d.s.update_connections([12, 2])
        out.append(([d.s.connections(k) for k in range(w.K)], [d.s.cull_state(k) for k in range(w.K)], [d.s.flags(k) for k in range(w.K)],
                    [d.s.loop_edges(k) for k in range(w.K)], [d.db.neighbors(k) for k in range(w.K)], d.s.connections_status()))
    assert out[0] == out[1] and out[0][1][3]["erased"] == 1 and out[0][1][4]["pending"] == 1


def test_the_host_query_on_host_lists_finds_the_same_candidates(vo):
    c = di.hand_cases()["conn_skips_a_bad_neighbour"]
    d, m, got = _run(vo, c["world"], c["script"])
    for cur, world in ((12, c["world"]), (12, di.overflow_world())):
        if world is not c["world"]:
            d, m, got = _run(vo, world, [("detect", cur, 0)])
        res, con = d.s.detect_loop_result(), d.s.connections(cur)
        excl = sorted(set(j for j, wt in enumerate(con["weights"]) if wt != 0) | {cur})
        conn = [k for k in con["ordered"] if not d.s.flags(k)[1]]
        assert (len(excl), len(conn)) == (res["n_excl"], res["n_conn"])
        host = d.db.query_loop([world.vector(cur)], [excl], connected=[conn], max_out=4)
        assert [int(x) for x in host[0]] == res["candidates"] and len(res["candidates"]) >= 1


# ---- behind a detection: compute_sim3_detected, release_loop_locks ---------------------------------------------------------------
def _loop_store(vo, sc, detect=True):
    """the scene's store with every layer of the loop thread, as tests/test_gpu_loop_merge.py enables them, and its database"""
    store = sc["store"]
    s = vo.KeyFrameStore(len(store), ls.NK)
    s.enable_connections(), s.enable_culling(), s.enable_mapping(ls.CAM6, ls.SF, 50000), s.enable_local_ba(*ls.BA_CAPS)
    s.enable_pose_graph(256, ci.LOOP_LC_CAPS[0], ci.LOOP_LC_CAPS[1])
    s.enable_point_upkeep(ls.MAX_RECENT), s.enable_fuse(ls.BOUNDS, 1024), s.enable_loop(**sc["caps"])
    s.enable_loop_fuse(ci.LOOP_LC_CAPS[0], sc["caps"]["max_loop_points"])
    s.enable_loop_correct(*ci.LOOP_LC_CAPS)
    s.enable_loop_merge()
    if detect:
        s.enable_detect_loop(4, 8)
    db = vo.KeyFrameDatabase(di.N_WORDS, len(store), 16, 1)
    for k, kf in enumerate(store):
        s.insert(dict(angle=kf["angle"], desc=kf["desc"], flags=kf["flags"], points=kf["points"], ids=kf["ids"], point_desc=kf["point_desc"],
                      min_dist=kf["min_dist"], max_dist=kf["max_dist"], nodes=kf["nodes"], bad=kf["bad"]))
        s.set_keypoints(k, kf["octave"], kf["depth"], kf["uright"])
        s.set_keypoint_xy(k, np.stack([kf["x"], kf["y"]], 1))
        if kf["pose"] is not None:
            s.set_pose(k, kf["pose"])
        s.set_normals(k, kf["normals"])
        s.set_point_refs(k, ci.scene_refs(kf, k))
        db.insert(*sc["world"].vector(k))
    s.update_connections(list(range(len(store))))
    return s, db


def _loop_bytes(s):
    r = s.loop_result()
    out = {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in r.items()}
    out["solver"] = [{k: v.tobytes() for k, v in s.loop_solver_inputs(c).items()} for c in range(4)]
    return out


def _detected(vo, sc, calls=4):
    s, db = _loop_store(vo, sc)
    m = di.build_model(sc["world"], 4, 8)
    for _ in range(calls):
        s.detect_loop(db, sc["current"], 0), m.detect_loop(sc["current"], 0)
    _same(s, db, m, "the scene behind %d calls" % calls)
    return s, db, m


@pytest.mark.parametrize("name,state", [("accepted", dr.ACCEPTED), ("rejected", dr.REJECTED), ("filtered_below_20", dr.NO_MATCH)])
def test_compute_sim3_detected_equals_compute_sim3_on_a_twin_and_the_locks_are_released(vo, name, state):
    sc = di.padded_scene(ls.scene(name))
    cur, K = sc["current"], len(sc["store"])
    a, db, m = _detected(vo, sc)
    res = a.detect_loop_result()
    assert res["outcome"] == dr.DETECTED and res["enough"] == sc["cand"]
    a.compute_sim3_detected(sc["rand"], ls.RAND_MAX, sc["fix_scale"], sc["max_rounds"])
    b, _ = _loop_store(vo, sc, detect=False)                        # the twin: the same list by hand, the locks by hand
    for k in sc["cand"] + [cur]:
        b.set_erase_lock(k, True)
    b.compute_sim3(cur, sc["cand"], sc["rand"], ls.RAND_MAX, sc["fix_scale"], sc["max_rounds"])
    ra, rb = _loop_bytes(a), _loop_bytes(b)
    assert ra == rb and ra["state"] == state
    assert [a.cull_state(k) for k in range(K)] == [b.cull_state(k) for k in range(K)]
    assert a.connections_status() == b.connections_status() == 0
    # the device form on a third store gives the same bytes
    import torch
    c, dbc, _ = _detected(vo, sc)
    keep = torch.from_numpy(np.ascontiguousarray(sc["rand"], np.int32)).cuda()
    c.compute_sim3_detected(keep, ls.RAND_MAX, sc["fix_scale"], sc["max_rounds"])
    assert _loop_bytes(c) == ra
    # computeSim3's releases against the model's lock table
    m.lock_candidates(sc["cand"])
    a.release_loop_locks()
    want = m.release_loop_locks(state, sc["cand"], cur, ra["match_kf"])
    assert a.loop_locks_result() == want
    assert [a.cull_state(k)["locked"] for k in range(K)] == m.cull.locked
    assert want[0] == (0 if state == dr.ACCEPTED else 2) and a.cull_state(cur)["locked"] == (1 if state == dr.ACCEPTED else 0)


def test_compute_sim3_detected_behind_a_call_that_detected_nothing(vo):
    sc = di.padded_scene(ls.scene("accepted"))
    s, db, m = _detected(vo, sc, calls=1)
    assert s.detect_loop_result()["outcome"] == dr.NOT_CONSISTENT
    s.compute_sim3_detected(sc["rand"], ls.RAND_MAX, sc["fix_scale"], sc["max_rounds"])
    r = s.loop_result()
    assert (r["state"], r["rounds"], r["rand_used"], r["match_kf"]) == (dr.NO_MATCH, 0, 0, -1)
    assert all(p == dict.fromkeys(p, 0) for p in r["per_candidate"])
    assert s.connections_status() == vo.KeyFrameStore.CONNECTIONS_INVALID
    s.release_loop_locks()                                           # NO MATCH with zero candidates: `current`, unlocked already
    assert s.loop_locks_result() == (0, []) and s.cull_state(sc["current"])["locked"] == 0
    assert [s.cull_state(k)["locked"] for k in range(len(sc["store"]))] == [0] * len(sc["store"])


def test_more_enough_candidates_than_the_loop_layer_holds(vo):
    w = di.standard_world({12: "A", 13: "A", 14: "A", 15: "AD"})
    one = vo.KeyFrameStore(w.K, di.NK)
    one.enable_connections(), one.enable_culling(), one.enable_mapping(ls.CAM6, ls.SF, 50000), one.enable_local_ba(*ls.BA_CAPS)
    one.enable_pose_graph(64, 8, 64), one.enable_point_upkeep(ls.MAX_RECENT), one.enable_fuse(ls.BOUNDS, 64)
    one.enable_loop(max_candidates=1, max_loop_points=64, max_rand=64), one.enable_detect_loop(4, 8)
    db = vo.KeyFrameDatabase(di.N_WORDS, w.K, 16, 1)
    for k in range(w.K):
        one.insert(cin.device_arrays(w.store[k])), db.insert(*w.vector(k))
    one.update_connections(w.update_order)
    for k in di.CURRENTS:
        one.detect_loop(db, k, 0)
    assert one.detect_loop_result()["enough"] == [2, 8]
    one.compute_sim3_detected(np.arange(6, dtype=np.int32), ls.RAND_MAX)
    r = one.loop_result()
    # (the hand worlds set no pose: k_loop_begin raises CONNECTIONS_INVALID for `current` beside the capacity bit)
    S = vo.KeyFrameStore
    assert (r["state"], r["rounds"]) == (dr.NO_MATCH, 0) and one.connections_status() == S.CONNECTIONS_LOOP_CAPACITY | S.CONNECTIONS_INVALID
    assert [one.cull_state(k)["locked"] for k in (2, 8)] == [0, 0]


# ---- the composed step -------------------------------------------------------------------------------------------------------------
def test_loop_closing_step_equals_the_step_wise_sequence(vo):
    import test_gpu_loop_merge as glm
    S = vo.KeyFrameStore
    sc = di.padded_scene(mi.loop_scene(ci.LOOP_SCENE), tail=9)
    cur, K = sc["current"], len(sc["store"])
    n = [len(kf["ids"]) for kf in sc["store"]]
    (a, dba), (b, dbb) = _loop_store(vo, sc), _loop_store(vo, sc)
    args = (sc["rand"], ls.RAND_MAX, sc["fix_scale"], sc["max_rounds"], ci.CHAIN_TH, 20)

    def same(where):
        ea, eb = glm._everything(a, n), glm._everything(b, n)
        assert ea == eb, where
        assert a.detect_loop_result() == b.detect_loop_result() and a.last_loop_keyframe == b.last_loop_keyframe, where
        ga, gb = a.detect_loop_groups(), b.detect_loop_groups()
        assert ga[0] == gb[0] and ga[1].tobytes() == gb[1].tobytes(), where
        assert [dba.neighbors(k) for k in range(K)] == [dbb.neighbors(k) for k in range(K)], where

    # once ending GATED
    a.last_loop_keyframe = b.last_loop_keyframe = cur - 5
    _, rec = a.loop_closing_step(dba, cur, *args)
    b.detect_loop(dbb, cur, cur - 5)
    assert rec == dict(outcome=S.DETECT_GATED, state=-1, correct_loop=1, stopped_at=0, n_enough=0, match=-1, continue_passes=0,
                       last_loop_keyframe=cur - 5)
    same("gated")
    a.last_loop_keyframe = b.last_loop_keyframe = 0
    # three times NOT_CONSISTENT
    for i in range(3):
        _, rec = a.loop_closing_step(dba, cur, *args)
        b.detect_loop(dbb, cur, 0)
        assert (rec["outcome"], rec["state"], rec["stopped_at"], rec["last_loop_keyframe"]) == (S.DETECT_NOT_CONSISTENT, -1, 0, 0)
        same(("not consistent", i))
    # once through correct_loop
    summary, rec = a.loop_closing_step(dba, cur, *args)
    b.detect_loop(dbb, cur, 0)
    assert b.detect_loop_result()["outcome"] == S.DETECT_DETECTED
    b.compute_sim3_detected(sc["rand"], ls.RAND_MAX, sc["fix_scale"], sc["max_rounds"])
    assert b.loop_result()["state"] == S.LOOP_ACCEPTED
    b.release_loop_locks()
    b.correct_loop(ci.CHAIN_TH, 20)
    b.last_loop_keyframe = cur
    match = sc["cand"][0]
    assert rec == dict(outcome=S.DETECT_DETECTED, state=S.LOOP_ACCEPTED, correct_loop=0, stopped_at=0, n_enough=1, match=match,
                       continue_passes=0, last_loop_keyframe=cur)
    same("through correct_loop")
    assert a.loop_edges(cur) == [match] and a.last_loop_keyframe == cur
    assert _loop_bytes(a) == _loop_bytes(b) and a.loop_locks_result() == b.loop_locks_result()
    # nine key-frames later: GATED by the word the step has just set
    _, rec = a.loop_closing_step(dba, cur + 9, *args)
    b.detect_loop(dbb, cur + 9, cur)
    assert (rec["outcome"], rec["last_loop_keyframe"]) == (S.DETECT_GATED, cur)
    same("nine key-frames later")
    assert a.cull_state(cur + 9)["locked"] == 0
