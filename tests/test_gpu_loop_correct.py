"""The loop correction on the device against the model tests/loop_correct_ref.py, through the binding:
vo_kfstore_propagate_loop in its three forms, vo_kfstore_loop_connections, vo_kfstore_loop_correct_result and
vo_kfstore_loop_correct_arrays.  Everything is compared byte for byte, with no tolerance: flags, ids, points, normals, min / max,
ref_kf, the pose column, the connection state, the record, the sticky word and every result array; S_corr, the poses and the moved
rows also against the longdouble matrix formulation within ten times the model's own error of it.  What a case is about is
asserted on the model by tests/test_loop_correct_ref.py (CPU), which also holds the model against the reference's sequence.

One case the contract names cannot be built: a corrected point with a holder, or its reference key-frame, at a position of
corr_kf BELOW the key-frame it is corrected through.  That key-frame is the lowest corrected holder, and the reference key-frame
is a holder (section 4k), so there is none; the model asserts it for every point it corrects.  What remains of the mixed state
-- stored poses although the same call overwrites them -- is what test_propagate_equals_the_model pins: it fails when a pose is
taken corrected (tests/test_loop_correct_ref.py measures the difference: more than 1e-3 in every normal)."""
import ctypes as C

import numpy as np
import pytest

import fuse_inputs as fi
import loop_correct_inputs as ci
import loop_correct_ref as lr
import loop_fuse_inputs as lfi
import loop_sim3_inputs as ls
import pose_graph_store_inputs as pi
import pose_graph_store_ref as pr
import test_gpu_local_ba_store as lb
import test_gpu_loop_fuse as glf
import test_gpu_pose_graph_store as pg
import test_loop_correct_ref as tr

pytestmark = pytest.mark.gpu

BOUND = 10 * ci.MODEL_LONGDOUBLE_WORST
ARRAYS = ("list", "corr_kf", "S_corr", "S_uncorr", "cp_id", "cp_ref")


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Dev(pg.Dev):
    """test_gpu_pose_graph_store.Dev with the opt-in and the step that stands for a fusion"""

    def __init__(self, vo, K, NK=ci.NK_HAND, lc_caps=ci.LC_CAPS, **kw):
        super().__init__(vo, K, NK, pose_graph=False, **kw)
        self.s.enable_pose_graph(pi.MAX_EDGES, 16, 512)          # (corrected points: more than that file's 64)
        if lc_caps is not None:
            self.s.enable_loop_correct(*lc_caps)

    def step(self, s):
        if s[0] == "setids":
            p = self.s.points(s[1], self.n[s[1]])
            self.s.update_points(s[1], np.asarray(s[3], np.uint8), p["points"], np.asarray(s[2], np.int32), p["point_desc"], p["min_dist"], p["max_dist"])
        else:
            super().step(s)


def _build(vo, script, lc_caps=ci.LC_CAPS):
    K = sum(1 for s in script if s[0] == "insert")
    d = Dev(vo, K, lc_caps=lc_caps)
    mr = ci.ModelRunner(exp=lb._exp(vo), log=lb._log(vo), lc_caps=lc_caps)
    for s in script:
        d.step(s), mr.step(s)
    return d, mr.m


def _model_arrays(m):
    L = m.lc
    if L is None:
        return {k: np.zeros(0) for k in ARRAYS}
    return dict(list=np.array(L["list"], np.int32), corr_kf=np.array(L["corr_kf"], np.int32), S_corr=np.array(L["S_corr"], np.float64).reshape(-1, 8),
                S_uncorr=np.array(L["S_uncorr"], np.float64).reshape(-1, 8), cp_id=np.array(L["cp_id"], np.int32), cp_ref=np.array(L["cp_ref"], np.int32))


def _same(d, m, where):
    """store, connections, record, arrays and the sticky word (read and cleared on both sides)"""
    lb._same_store(d, m, where)
    K = len(m.store)
    assert [d.s.connections(k) for k in range(K)] == [m.connections(k) for k in range(K)], where
    got = d.s.loop_correct_result()
    assert got["record"] == m.lc_record, (where, got["record"], m.lc_record)
    for key, w in _model_arrays(m).items():
        assert got[key].tobytes() == w.tobytes(), (where, key)
    if m.lc_rows is not None:
        inp = m.lc_inputs()
        assert got["lc_start"].tobytes() == inp["lc_start"].tobytes() and got["lc_kf"].tobytes() == inp["lc_kf"].tobytes(), where
    else:
        assert len(got["lc_start"]) == 0 and len(got["lc_kf"]) == 0, where
    assert d.s.connections_status() == m.sticky, where
    m.sticky = 0
    return got


def _scw(curr, scale=1.1):
    return ci.loop_sim3(pi.HAND_POSES[curr], scale)


# ---- propagate_loop -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "dev"])
def test_propagate_equals_the_model(vo, form):
    """the hand store with everything in it: points held by two and more corrected key-frames (moved once, through the lowest),
    holders at the correcting key-frame's position, above it and outside the set with the reference key-frame among each, scale 1.1
    (the pose translation is t / s), an id in two features of one key-frame, a carrier outside the set, a bad key-frame in the list,
    stored poses through each of the quaternion's three off-branches"""
    script = ci.propagate_scene(bad=(3,))
    d, m = _build(vo, script)
    m0 = ci.run_model(script, exp=lb._exp(vo), log=lb._log(vo))
    Scw = _scw(ci.CURR)
    keep = _cuda(np.array(Scw)) if form == "dev" else None
    d.s.propagate_loop(ci.CURR, keep if form == "dev" else Scw)
    L = m.propagate_loop(ci.CURR, Scw)
    got = _same(d, m, form)
    assert got["record"]["status"] == lr.OK and list(got["corr_kf"]) == ci.CORR and got["record"]["n_rows_moved"] > 100
    # the device's own arrays and store against the longdouble matrix formulation
    dm = ci.run_model(script, exp=lb._exp(vo), log=lb._log(vo))
    for k in range(len(dm.store)):
        st = d.state(k)
        dm.store[k]["points"], dm.store[k]["pose"] = st["points"], [float(x) for x in st["pose"]]
    dL = dict(L, S_corr=[list(r) for r in got["S_corr"]], S_uncorr=[list(r) for r in got["S_uncorr"]])
    worst = tr.longdouble_errors(m0, dm, dL, Scw, ci.CURR)
    print("device against longdouble matrices:", worst)
    assert worst <= BOUND


def test_empty_list(vo):
    d, m = _build(vo, ci.lonely_scene())
    d.s.propagate_loop(1, _scw(1, 1.0)), m.propagate_loop(1, _scw(1, 1.0))
    got = _same(d, m, "lonely")
    assert got["record"]["n_corr"] == 1 and got["record"]["n_cp"] == 10 and list(got["list"]) == [1]


def test_refusals_on_the_device_leave_the_store_beyond_step_1(vo):
    """more corrected key-frames or points than the layer was enabled for, and a listed key-frame without a pose: the status,
    the counts and the sticky words are the model's, the store's bytes those of update_connections([curr]) alone"""
    Scw = _scw(ci.CURR)
    n_cp = len(ci.run_model(ci.propagate_scene()).propagate_loop(ci.CURR, Scw)["cp_id"])
    for caps, script, status in (((4, 256, 64), ci.propagate_scene(), lr.OVERFLOW), ((8, n_cp - 1, 64), ci.propagate_scene(), lr.OVERFLOW),
                                 (ci.LC_CAPS, ci.propagate_scene(poses=[0, 1, 2, 4, 5, 6, 7]), lr.EMPTY)):
        d, m = _build(vo, script, caps)
        d2, m2 = _build(vo, script, caps)
        d2.s.update_connections([ci.CURR])
        d.s.propagate_loop(ci.CURR, Scw)
        assert m.propagate_loop(ci.CURR, Scw) is None and m.lc_record["status"] == status and m.sticky != 0
        _same(d, m, (caps, status))
        for k in range(len(m.store)):
            a, b = d.state(k), d2.state(k)
            assert all(np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes() for key in a), k
            assert d.s.connections(k) == d2.s.connections(k)
        d.s.loop_connections(), m.loop_connections()              # no lists were left
        _same(d, m, "loop_connections behind a refused propagate")
    d, m = _build(vo, ci.propagate_scene())                       # a scale of 0: step 6 would divide by it
    zero = Scw[:7] + [0.0]
    d.s.propagate_loop(ci.CURR, zero), m.propagate_loop(ci.CURR, zero)
    assert _same(d, m, "scale 0")["record"]["status"] == lr.EMPTY
    d, m = _build(vo, ci.propagate_scene(), (5, n_cp, 64))        # both capacities met exactly
    d.s.propagate_loop(ci.CURR, Scw), m.propagate_loop(ci.CURR, Scw)
    assert _same(d, m, "met exactly")["record"]["status"] == lr.OK


def test_opt_in_and_refusals(vo):
    L = vo.lib()
    Scw = np.array(_scw(ci.CURR))
    plain = Dev(vo, 8, lc_caps=None)                              # a store without the layer refuses every entry point
    for s in ci.propagate_scene():
        plain.step(s)
    before = [plain.state(k) for k in range(8)]
    h = plain.s._h
    ptr = C.c_void_p()
    for rc in (L.vo_kfstore_propagate_loop(h, ci.CURR, vo._p(Scw)), L.vo_kfstore_propagate_loop_dev(h, ci.CURR, vo._p(Scw)),
               L.vo_kfstore_propagate_loop_sim3(h), L.vo_kfstore_loop_connections(h),
               L.vo_kfstore_loop_correct_result(h, None, None, None, None, None, None, None, None, None),
               L.vo_kfstore_loop_correct_arrays(h, C.byref(ptr), None, None, None, None, None, None),
               L.vo_kfstore_enable_loop_correct(h, 8, 8, 8)):    # (the last: the store holds key-frames)
        assert rc == -1
    for k in range(8):
        after = plain.state(k)
        assert all(np.asarray(after[key]).tobytes() == np.asarray(before[k][key]).tobytes() for key in after), k
    no_pg = pg.Dev(vo, 4, 16, pose_graph=False)
    assert L.vo_kfstore_enable_loop_correct(no_pg.s._h, 8, 8, 8) == -1        # no enable_pose_graph
    e = pg.Dev(vo, 4, 16)
    for caps in ((0, 8, 8), (8, 0, 8), (8, 8, 0)):
        assert L.vo_kfstore_enable_loop_correct(e.s._h, *caps) == -1
    assert L.vo_kfstore_enable_loop_correct(None, 8, 8, 8) == -1
    assert L.vo_kfstore_enable_loop_correct(e.s._h, 8, 8, 8) == 0 and L.vo_kfstore_enable_loop_correct(e.s._h, 8, 8, 8) == 0
    assert L.vo_kfstore_loop_connections(e.s._h) == -1                        # an empty store
    d, m = _build(vo, ci.propagate_scene())
    h = d.s._h
    for rc in (L.vo_kfstore_propagate_loop(h, 8, vo._p(Scw)), L.vo_kfstore_propagate_loop(h, -1, vo._p(Scw)), L.vo_kfstore_propagate_loop(h, ci.CURR, None),
               L.vo_kfstore_propagate_loop_dev(h, 8, vo._p(Scw)), L.vo_kfstore_propagate_loop_dev(h, ci.CURR, None),
               L.vo_kfstore_propagate_loop_sim3(h)):             # (the last: no enable_loop)
        assert rc == -1
    d.s.loop_connections(), m.loop_connections()                  # no propagate before it: decided on the device
    got = _same(d, m, "no propagate")
    assert got["record"]["connections_status"] == lr.EMPTY
    d.s.erase_keyframe(ci.CURR), m.erase_keyframe(ci.CURR)        # curr erased: decided on the device
    d.s.propagate_loop(ci.CURR, Scw), m.propagate_loop(ci.CURR, list(Scw))
    _same(d, m, "curr erased")
    assert d.s.loop_correct_result()["record"]["status"] == lr.EMPTY
    assert L.vo_kfstore_loop_correct_result(h, None, None, None, None, None, None, None, None, None) == 0


def test_a_store_with_the_layer_unused_returns_the_same_bytes(vo):
    """the pose graph's main case with the layer enabled and without it"""
    case = [c for c in pg.CASES if c["name"] == "f_all_together"][0]
    out = []
    for caps in (ci.LC_CAPS, None):
        d = Dev(vo, 8, lc_caps=caps)
        for s in case["script"]:
            d.step(s)
        d.s.pose_graph_window(case["curr"], case["match"], case["inp"])
        w = d.s.pose_graph_window_result()
        out.append(([{k: np.asarray(v).tobytes() for k, v in d.state(j).items()} for j in range(8)], [d.s.connections(j) for j in range(8)],
                    {k: np.asarray(v).tobytes() for k, v in w.items() if k not in ("record", "fixed")}, w["record"]))
    assert out[0] == out[1] and out[0][3]["n_edges"] > 10


# ---- loop_connections ---------------------------------------------------------------------------------------------------------
def _connections_run(vo, lc_caps=ci.LC_CAPS):
    s = ci.connections_scene()
    d, m = _build(vo, s.script(), lc_caps)
    Scw = _scw(ci.C_CURR, 1.0)
    d.s.propagate_loop(ci.C_CURR, Scw), m.propagate_loop(ci.C_CURR, Scw)
    _same(d, m, "propagate")
    for st in ci.fusion_steps(s):
        d.step(st), m.update_points(st[1], st[2], st[3])
    return d, m


def test_loop_connections_equal_the_model_and_the_hand_rows(vo):
    """a connection the fusion created (one of weight 100, ones of weight 3 and 1), a member of the old list and the members of
    currConnect removed, the mode switch (key-frame 1 is NOT in 6's row), an entry whose update finds no connection; the graph
    afterwards is update_connections' on the same list"""
    d, m = _connections_run(vo)
    twin, mt = _connections_run(vo)
    d.s.loop_connections(), m.loop_connections()
    got = _same(d, m, "loop_connections")
    rows = {int(k): [int(x) for x in got["lc_kf"][got["lc_start"][r]:got["lc_start"][r + 1]]] for r, k in enumerate(got["corr_kf"])}
    assert rows == ci.C_ROWS and got["record"]["n_lc"] == 4 and got["record"]["connections_status"] == lr.OK
    twin.s.update_connections(ci.C_LIST)
    assert [d.s.connections(k) for k in range(8)] == [twin.s.connections(k) for k in range(8)]
    # and into the pose graph: the device arrays straight in, the downloaded ones through the host form, the model's
    A, rec = d.s.loop_correct_arrays(), got["record"]
    want = m.pg_window(ci.C_CURR, 0, m.lc_inputs())
    vo.check(vo.lib().vo_kfstore_pose_graph_window_dev(d.s._h, ci.C_CURR, 0, rec["n_corr"], vo._p(A["corr_kf"]), vo._p(A["S_corr"]), vo._p(A["S_uncorr"]),
                                                       vo._p(A["lc_start"]), rec["n_lc"], vo._p(A["lc_kf"]), rec["n_cp"], vo._p(A["cp_id"]),
                                                       vo._p(A["cp_ref"])), "vo_kfstore_pose_graph_window_dev")
    w_dev = d.s.pose_graph_window_result()
    d.s.pose_graph_window(ci.C_CURR, 0, {k: got[k] for k in ("corr_kf", "S_corr", "S_uncorr", "lc_start", "lc_kf", "cp_id", "cp_ref")})
    w_host = d.s.pose_graph_window_result()
    assert w_dev["record"] == w_host["record"] and {k: w_dev["record"][k] for k in pr.PG_RECORD} == m.pg_record
    assert w_dev["record"]["status"] == pr.OK and w_dev["record"]["n_a"] >= 1
    for key, w in want.items():
        assert w_dev[key].tobytes() == w_host[key].tobytes() == w.tobytes(), key
    assert d.s.connections_status() == m.sticky == 0


def test_loop_connections_capacity(vo):
    d, m = _connections_run(vo, (8, 256, 3))
    twin, mt = _connections_run(vo, (8, 256, 3))
    d.s.loop_connections(), m.loop_connections()
    got = _same(d, m, "capacity")
    assert got["record"]["n_lc"] == 4 and got["record"]["connections_status"] == lr.OVERFLOW and len(got["lc_kf"]) == 0
    twin.s.update_connections(ci.C_LIST)
    assert [d.s.connections(k) for k in range(8)] == [twin.s.connections(k) for k in range(8)]


# ---- behind compute_sim3 ------------------------------------------------------------------------------------------------------
LOOP_LC_CAPS = ci.LOOP_LC_CAPS


def _loop_store(vo, sc):
    """loop_sim3_inputs.build_device with the pose graph, the loop fusion and the loop correction"""
    store = sc["store"]
    s = vo.KeyFrameStore(len(store), ls.NK)
    s.enable_connections(), s.enable_culling(), s.enable_mapping(ls.CAM6, ls.SF, 50000), s.enable_local_ba(*ls.BA_CAPS)
    s.enable_pose_graph(256, LOOP_LC_CAPS[0], LOOP_LC_CAPS[1])
    s.enable_point_upkeep(ls.MAX_RECENT), s.enable_fuse(ls.BOUNDS, 1024), s.enable_loop(**sc["caps"])
    s.enable_loop_fuse(LOOP_LC_CAPS[0], sc["caps"]["max_loop_points"])
    s.enable_loop_correct(*LOOP_LC_CAPS)
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


def _loop_devices(vo, name, n):
    sc = ls.scene(name)
    out = []
    for _ in range(n):
        s = _loop_store(vo, sc)
        s.compute_sim3(sc["current"], sc["cand"], sc["rand"], ls.RAND_MAX, sc["fix_scale"], sc["max_rounds"])
        out.append(s)
    return sc, out


def _all_bytes(s, n):
    return (glf._states(s, n), [s.pose(k)[0].tobytes() for k in range(len(n))], [s.connections(k) for k in range(len(n))],
            {k: (v if k == "record" else v.tobytes()) for k, v in s.loop_correct_result().items()})


def test_the_three_forms_give_the_same_bytes_behind_an_accepted_compute_sim3(vo):
    sc, (a, b, c) = _loop_devices(vo, "accepted", 3)
    res = a.loop_result()
    assert res["state"] == vo.KeyFrameStore.LOOP_ACCEPTED
    n = [len(kf["ids"]) for kf in sc["store"]]
    before = _all_bytes(a, n)
    Scw8 = lr.scw8_from13(res["Scw"])
    keep = _cuda(np.array(Scw8))
    a.propagate_loop()                                            # the _loop form: curr and Scw read in place
    b.propagate_loop(sc["current"], Scw8)                         # the host form
    c.propagate_loop(sc["current"], keep)                         # the device form
    ra = _all_bytes(a, n)
    assert ra == _all_bytes(b, n), "the _loop form and the host form differ"
    assert ra == _all_bytes(c, n), "the _loop form and the device form differ"
    rec = ra[3]["record"]
    assert rec["status"] == lr.OK and rec["curr"] == sc["current"] and rec["n_corr"] >= 1 and rec["n_cp"] > 20 and rec["n_rows_moved"] >= rec["n_cp"]
    assert ra[0] != before[0] and ra[1] != before[1]
    assert a.connections_status() == b.connections_status() == c.connections_status() == 0


def test_loop_form_behind_a_rejected_compute_sim3(vo):
    sc, (a,) = _loop_devices(vo, "rejected", 1)
    assert a.loop_result()["state"] == vo.KeyFrameStore.LOOP_REJECTED
    n = [len(kf["ids"]) for kf in sc["store"]]
    a.connections_status()
    before = _all_bytes(a, n)
    a.propagate_loop()
    after = _all_bytes(a, n)
    assert after[:3] == before[:3] and after[3]["record"]["status"] == lr.EMPTY and after[3]["record"]["n_corr"] == 0
    assert a.connections_status() == vo.KeyFrameStore.CONNECTIONS_INVALID
    a.loop_connections()
    assert _all_bytes(a, n)[:3] == before[:3] and a.connections_status() == vo.KeyFrameStore.CONNECTIONS_INVALID


def _setids(s, n, step):
    """the ("setids", k, ids, flags) step on a store: everything else of the key-frame's map side stays"""
    k = step[1]
    p = s.points(k, n[k])
    s.update_points(k, np.asarray(step[3], np.uint8), p["points"], np.asarray(step[2], np.int32), p["point_desc"], p["min_dist"], p["max_dist"])


def _state(s, k, nk):
    p = s.points(k, nk)
    T, on = s.pose(k)
    return dict(flags=p["flags"], ids=p["ids"], points=p["points"], ref=s.point_refs(k, nk), normals=p["normals"], min_dist=p["min_dist"],
                max_dist=p["max_dist"], pose=T if on else np.zeros(12), bad=s.flags(k, nk)[1], point_desc=p["point_desc"])


def _same_as_model(s, n, m, where):
    """store, connections, the layer's record and arrays, the sticky word"""
    for k in range(len(m.store)):
        got = _state(s, k, n[k])
        for key, w in m.state(k).items():
            assert np.asarray(got[key]).tobytes() == np.asarray(w).tobytes(), (where, k, key)
    assert [s.connections(k) for k in range(len(n))] == [m.connections(k) for k in range(len(n))], where
    got = s.loop_correct_result()
    assert got["record"] == m.lc_record, (where, got["record"], m.lc_record)
    for key, w in _model_arrays(m).items():
        assert got[key].tobytes() == w.tobytes(), (where, key)
    assert s.connections_status() == m.sticky, where
    m.sticky = 0
    return got


def _chain_on_the_device(vo, s, curr, match, ids_tensor=None, block=None):
    """propagate has run: search_and_fuse (_loop form, or the device form on ids_tensor) -> [block()] -> loop_connections ->
    pose_graph_window_dev, every array by its device address; then the host-form window on the downloaded arrays"""
    L = vo.lib()
    A = s.loop_correct_arrays()
    rec = s.loop_correct_result()["record"]
    assert rec["status"] == lr.OK
    th = C.c_float(ci.CHAIN_TH)
    if ids_tensor is None:
        vo.check(L.vo_kfstore_search_and_fuse_loop(s._h, rec["n_corr"], vo._p(A["corr_kf"]), vo._p(A["S_corr"]), th), "vo_kfstore_search_and_fuse_loop")
    else:
        vo.check(L.vo_kfstore_search_and_fuse_dev(s._h, rec["n_corr"], vo._p(A["corr_kf"]), vo._p(A["S_corr"]), int(ids_tensor.numel()),
                                                  vo._p(ids_tensor), th), "vo_kfstore_search_and_fuse_dev")
    if block is not None:
        block()
    s.loop_connections()
    got = s.loop_correct_result()
    rec = got["record"]
    assert rec["connections_status"] == lr.OK
    vo.check(L.vo_kfstore_pose_graph_window_dev(s._h, curr, match, rec["n_corr"], vo._p(A["corr_kf"]), vo._p(A["S_corr"]), vo._p(A["S_uncorr"]),
                                                vo._p(A["lc_start"]), rec["n_lc"], vo._p(A["lc_kf"]), rec["n_cp"], vo._p(A["cp_id"]), vo._p(A["cp_ref"])),
             "vo_kfstore_pose_graph_window_dev")
    w_dev = s.pose_graph_window_result()
    s.pose_graph_window(curr, match, {k: got[k] for k in ("corr_kf", "S_corr", "S_uncorr", "lc_start", "lc_kf", "cp_id", "cp_ref")})
    w_host = s.pose_graph_window_result()
    assert w_dev["record"] == w_host["record"] and w_dev["record"]["status"] == pr.OK
    for key in w_dev:
        if key not in ("record", "fixed"):
            assert w_dev[key].tobytes() == w_host[key].tobytes(), key
    return got, w_dev


def _same_chain_end(s, n, m, got, w, want, where):
    """after the chain: the store, the rows, the fusion's record and the window against the model's"""
    _same_as_model(s, n, m, where)
    inp = m.lc_inputs()
    assert got["record"] == m.lc_record and s.loop_fuse_result() == m.loop_fuse_result(), where
    assert got["lc_start"].tobytes() == inp["lc_start"].tobytes() and got["lc_kf"].tobytes() == inp["lc_kf"].tobytes(), where
    assert {k: w["record"][k] for k in pr.PG_RECORD} == m.pg_record and want is not None, where
    for key, x in want.items():
        assert w[key].tobytes() == x.tobytes(), (where, key)
    assert w["record"]["n_a"] >= 1 and got["record"]["n_rows_moved"] >= 1, (where, w["record"], got["record"])


def test_chain_behind_compute_sim3(vo):
    """compute_sim3 -> propagate_loop (_sim3 form) -> search_and_fuse_loop -> loop_connections -> pose_graph_window_dev on the
    accepted loop scene with 255 shared points, no array through the host: equal to the model's chain after the propagation and
    at the end, the window also to the host form's on the downloaded arrays; a family-A edge (the fusion lifts curr - match above
    100) and moved points, which tests/test_loop_correct_ref.py shows on the model alone"""
    sc, (a,) = _loop_devices(vo, ci.LOOP_SCENE, 1)
    res = a.loop_result()
    assert res["state"] == vo.KeyFrameStore.LOOP_ACCEPTED
    n = [len(kf["ids"]) for kf in sc["store"]]
    m = ci.scene_model(sc, lb._exp(vo), lb._log(vo))
    _same_as_model(a, n, m, "the scene")
    cur, match, ids = sc["current"], res["match_kf"], [int(x) for x in res["loop_point_ids"]]
    a.propagate_loop()
    assert m.propagate_loop(cur, lr.scw8_from13(res["Scw"])) is not None
    _same_as_model(a, n, m, "propagate_loop")
    L = m.lc
    m.search_and_fuse(L["corr_kf"], L["S_corr"], ids, ci.CHAIN_TH)
    got, w = _chain_on_the_device(vo, a, cur, match)
    assert m.loop_connections() is not None
    want = m.pg_window(cur, match, m.lc_inputs())
    _same_chain_end(a, n, m, got, w, want, "the chain")
    print("loop scene: record", got["record"], "fusion", a.loop_fuse_result()["totals"], "window", w["record"])


def test_seeded_chain(vo):
    """the seeded 12 x 256 scene at its first fuse with a loop-side key-frame behind it: propagate_loop_dev -> search_and_fuse_dev ->
    the fused block -> loop_connections -> pose_graph_window_dev fed with the layer's device arrays, equal to the model's chain"""
    d = glf.LDev(vo, fi.K_SCENE, fi.N_FEAT, fi.SCENE_CAPS, True, fi.SCENE_RECENT, fi.SCENE_CANDIDATES, max_corrected=ci.CHAIN_LC_CAPS[0],
                 max_loop_points=lfi.CHAIN_LOOP_POINTS, form="dev")
    d.s.enable_pose_graph(4096, ci.CHAIN_LC_CAPS[0], ci.CHAIN_LC_CAPS[1])
    d.s.enable_loop_correct(*ci.CHAIN_LC_CAPS)
    mr, m = tr.seeded_chain_model(lb._exp(vo), lb._log(vo))
    where = glf._seeded_until_first_fuse(d, mr)
    for s in ci.seeded_old_keyframe(m):
        d.step(s), mr.step(s)
    glf._same(d, m, where)
    cur = ci.SEEDED_MATCH - 1
    Scw = ci.chain_scw(m, cur)
    keep = _cuda(np.array(Scw))
    d.s.propagate_loop(cur, keep)
    L = m.propagate_loop(cur, Scw)
    assert L is not None and len(L["corr_kf"]) >= 3 and m.lc_record["n_rows_moved"] > len(L["cp_id"]) > 100
    _same_as_model(d.s, d.n, m, "propagate_loop")
    ids = ci.seeded_loop_ids(m, 0)
    tensor = _cuda(np.array(ids, np.int32))
    m.search_and_fuse(L["corr_kf"], L["S_corr"], ids, ci.CHAIN_TH)
    block = ci.seeded_block(m, cur)
    m.update_points(block[1], block[2], block[3])
    got, w = _chain_on_the_device(vo, d.s, cur, ci.SEEDED_MATCH, tensor, block=lambda: _setids(d.s, d.n, block))
    assert m.loop_connections() is not None
    want = m.pg_window(cur, ci.SEEDED_MATCH, m.lc_inputs())
    _same_chain_end(d.s, d.n, m, got, w, want, "the chain")
    assert d.s.recent_points() == m.recent_points()
    print("seeded scene: record", got["record"], "fusion", m.loop_fuse_result()["totals"], "window", w["record"])
