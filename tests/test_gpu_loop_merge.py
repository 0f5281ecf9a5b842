"""The merge of the loop matches on the device against the model tests/loop_merge_ref.py, through the
binding: vo_kfstore_merge_loop_matches in its three forms, vo_kfstore_loop_merge_result and the composed vo_kfstore_correct_loop.
Everything is compared byte for byte, with no tolerance: flags, ids, points, point_desc, normals, min / max, ref_kf, the recent
list, the record, per_feature and the sticky word; the chains also the connection state, the layer arrays and the pose graph's
window.  What a case is about is asserted through the record; tests/test_loop_merge_ref.py (CPU) holds the hand tables, the model
against the reference's sequence and the conditions on the scenes."""
import ctypes as C

import numpy as np
import pytest

import fuse_inputs as fi
import loop_correct_inputs as ci
import loop_correct_ref as lr
import loop_fuse_inputs as lfi
import loop_merge_inputs as mi
import loop_merge_ref as mr
import loop_sim3_inputs as ls
import pose_graph_store_ref as pr
import test_gpu_local_ba_store as lb
import test_gpu_loop_correct as glc
import test_gpu_loop_fuse as glf

pytestmark = pytest.mark.gpu


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class MDev(glf.LDev):
    """test_gpu_loop_fuse.LDev with the opt-in and the merge step; form: "host" or "dev" (the list as a device tensor)"""

    def __init__(self, vo, K, NK, merge=True, **kw):
        super().__init__(vo, K, NK, **kw)
        if merge:
            self.s.enable_loop_merge()

    def merge(self, curr, match):
        a = np.asarray(match, np.int32)
        if self.form == "dev":
            a = _cuda(a)
            self.keep.append(a)
        self.s.merge_loop_matches(curr, a)

    def step(self, s):
        if s[0] == "merge":
            self.merge(s[1], s[2])
        else:
            super().step(s)


def _model(vo, **kw):
    return mi.ModelRunner(exp=lb._exp(vo), log=lb._log(vo), **kw)


def _same_merge(s, m, where):
    got, want = s.loop_merge_result(), m.loop_merge_result(s.max_features)
    assert got["record"] == want["record"], (where, got["record"], want["record"])
    assert got["per_feature"].tobytes() == want["per_feature"].tobytes(), (where, got["per_feature"], want["per_feature"])


def _same_call(d, m, where):
    glf._same(d, m, where, result=False)
    _same_merge(d.s, m, where)


def _run(vo, c, form="host", **kw):
    K = sum(1 for s in c["script"] if s[0] == "insert")
    caps = {k: c[k] for k in ("caps",) if k in c}
    d, mrun = MDev(vo, K, c["NK"], form=form, **caps, **kw), _model(vo, **caps)
    step = ("merge", c["curr"], c["match"])
    for s in c["script"] + [step]:
        d.step(s), mrun.step(s)
    _same_call(d, mrun.m, step[:2])
    return d, mrun.m, step


CASES = {name: (lambda name=name: mi.hand_case(name)) for name in mi.HAND_CASES}
CASES.update(no_step_alone=mi.no_step_alone_case, counters=mi.counters_case, erased_curr=mi.erased_curr_case)
DEV_FORM = ("add", "every_step_alone", "no_step_alone", "b_is_the_a0_of_a_later_step")


# ---- the hand-made stores: one call each, then the same call again ------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_cases(vo, name):
    c = CASES[name]()
    d, m, step = _run(vo, c, form="dev" if name in DEV_FORM else "host")
    got = d.s.loop_merge_result()
    n = len(c["per"])
    assert got["record"] == c["rec"] and list(got["per_feature"][:n]) == c["per"] and not got["per_feature"][n:].any()
    if name == "erased_curr":
        assert m.sticky == 0 and got["record"]["steps"] == 0          # (_same_call has compared and cleared CONNECTIONS_INVALID)
    # the same call again finds what the first left (every replace has become a no-op or an add), and the model agrees
    d.step(step), m.merge_loop_matches(*step[1:])
    _same_call(d, m, "second call")


def test_every_step_alone_and_no_step_alone(vo):
    for c, ordered in ((mi.hand_case("every_step_alone"), 0), (mi.no_step_alone_case(), 4)):
        d, m, _ = _run(vo, c)
        rec = d.s.loop_merge_result()["record"]
        assert rec["ordered"] == ordered and rec["steps"] == c["rec"]["steps"] and (ordered == 0 or ordered == rec["steps"])


def test_counters_are_added_when_both_are_listed(vo):
    c = mi.counters_case()
    before = {e[0]: e[2:] for e in mi.run_model(c["script"]).recent_points()}
    d, m, _ = _run(vo, c)
    got = {e[0]: e[2:] for e in d.s.recent_points()}
    assert got[700] == (before[700][0] + before[900][0], before[700][1] + before[900][1]) and got[900] == before[900]


def test_carrier_capacity(vo):
    c = mi.capacity_carriers_case()
    d, m, _ = _run(vo, c)
    assert len(m.carriers(900)) == vo.KeyFrameStore.FUSE_MAX_CARRIERS + 1 and d.s.loop_merge_result()["record"] == c["rec"]
    # (_same_call has compared the sticky word: VO_KFSTORE_FUSE_CAPACITY on both sides)


def test_the_record_of_the_last_search_and_fuse_survives(vo):
    c = lfi.hand_case("replace_three_holders")
    K = sum(1 for s in c["script"] if s[0] == "insert")
    d, mrun = MDev(vo, K, c["NK"]), _model(vo)
    for s in c["script"] + [("loopfuse", c["corr_kf"], c["S_corr"], c["ids"], c["th"])]:
        d.step(s), mrun.step(s)
    fused = d.s.loop_fuse_result()
    assert fused["totals"][3] == 1
    step = ("merge", fi.T_HAND, [c["ids"][0]])
    d.step(step), mrun.step(step)
    _same_call(d, mrun.m, "merge behind a fusion")
    assert d.s.loop_fuse_result() == fused == mrun.m.loop_fuse_result()


# ---- refusals, opt-in ---------------------------------------------------------------------------------------------------------
def test_opt_in_and_refusals(vo):
    L = vo.lib()
    ids = np.array([700], np.int32)
    c = mi.hand_case("add")
    plain = MDev(vo, 7, 64, merge=False)                                       # no enable_loop_merge
    for s in c["script"]:
        plain.step(s)
    h = plain.s._h
    for rc in (L.vo_kfstore_merge_loop_matches(h, mi.CURR, 1, vo._p(ids)), L.vo_kfstore_merge_loop_matches_dev(h, mi.CURR, 1, vo._p(ids)),
               L.vo_kfstore_merge_loop_matches_loop(h), L.vo_kfstore_loop_merge_result(h, None, None),
               L.vo_kfstore_correct_loop(h, C.c_float(4.0), 20, None, None),
               L.vo_kfstore_enable_loop_merge(h)):                             # (the last: the store holds key-frames)
        assert rc == -1
    no_lf = glf.LDev(vo, 4, 16, max_corrected=None)
    assert L.vo_kfstore_enable_loop_merge(no_lf.s._h) == -1                    # no enable_loop_fuse
    assert L.vo_kfstore_enable_loop_merge(None) == -1
    e = glf.LDev(vo, 4, 16)
    assert L.vo_kfstore_enable_loop_merge(e.s._h) == 0 and L.vo_kfstore_enable_loop_merge(e.s._h) == 0
    d, m, _ = _run(vo, c)
    h = d.s._h
    before = [d.state(k) for k in range(7)]
    big = np.full(65, -1, np.int32)
    assert L.vo_kfstore_merge_loop_matches(h, mi.CURR, 65, vo._p(big)) == -4   # n > max_features
    assert L.vo_kfstore_merge_loop_matches_dev(h, mi.CURR, 65, vo._p(big)) == -4
    for rc in (L.vo_kfstore_merge_loop_matches(h, mi.CURR, -1, vo._p(ids)), L.vo_kfstore_merge_loop_matches(h, mi.CURR, 1, None),
               L.vo_kfstore_merge_loop_matches_dev(h, mi.CURR, 1, None), L.vo_kfstore_merge_loop_matches_loop(h),   # (no enable_loop)
               L.vo_kfstore_correct_loop(h, C.c_float(4.0), 20, None, None)):
        assert rc == -1
    assert L.vo_kfstore_merge_loop_matches(h, mi.CURR, 0, None) == 0           # an empty list is a call with no steps
    m.merge_loop_matches(mi.CURR, [])
    _same_call(d, m, "empty list")
    for curr in (7, -1):                                                       # curr outside the store: decided on the device
        d.s.merge_loop_matches(curr, ids), m.merge_loop_matches(curr, [700])
        assert m.sticky == mr.STICKY_INVALID
        _same_call(d, m, ("curr", curr))
        assert d.s.loop_merge_result()["record"]["steps"] == 0
    for k in range(7):
        after = d.state(k)
        assert all(np.asarray(after[key]).tobytes() == np.asarray(before[k][key]).tobytes() for key in after), k
    assert L.vo_kfstore_loop_merge_result(h, None, None) == 0


def test_a_store_with_the_layer_unused_returns_the_same_bytes(vo):
    """the loop fusion's main hand case with the layer enabled and without it"""
    c = lfi.hand_case("replace_three_holders")
    K = sum(1 for s in c["script"] if s[0] == "insert")
    out = []
    for merge in (True, False):
        d = MDev(vo, K, c["NK"], merge=merge)
        for s in c["script"] + [("loopfuse", c["corr_kf"], c["S_corr"], c["ids"], c["th"])]:
            d.step(s)
        out.append(([{k: np.asarray(v).tobytes() for k, v in d.state(j).items()} for j in range(K)], [d.s.connections(j) for j in range(K)],
                    d.s.recent_points(), d.s.loop_fuse_result(), d.s.connections_status()))
    assert out[0] == out[1] and out[0][3]["totals"][3] == 1


# ---- behind compute_sim3 ------------------------------------------------------------------------------------------------------
LOOP_LC_CAPS = ci.LOOP_LC_CAPS


def _loop_store(vo, sc, lc_caps=LOOP_LC_CAPS, max_edges=256):
    """test_gpu_loop_correct._loop_store with the merge layer"""
    store = sc["store"]
    s = vo.KeyFrameStore(len(store), ls.NK)
    s.enable_connections(), s.enable_culling(), s.enable_mapping(ls.CAM6, ls.SF, 50000), s.enable_local_ba(*ls.BA_CAPS)
    s.enable_pose_graph(max_edges, LOOP_LC_CAPS[0], LOOP_LC_CAPS[1])
    s.enable_point_upkeep(ls.MAX_RECENT), s.enable_fuse(ls.BOUNDS, 1024), s.enable_loop(**sc["caps"])
    s.enable_loop_fuse(LOOP_LC_CAPS[0], sc["caps"]["max_loop_points"])
    s.enable_loop_correct(*lc_caps)
    s.enable_loop_merge()
    for k, kf in enumerate(store):
        s.insert(dict(angle=kf["angle"], desc=kf["desc"], flags=kf["flags"], points=kf["points"], ids=kf["ids"], point_desc=kf["point_desc"],
                      min_dist=kf["min_dist"], max_dist=kf["max_dist"], nodes=kf["nodes"], bad=kf["bad"]))
        s.set_keypoints(k, kf["octave"], kf["depth"], kf["uright"])
        s.set_keypoint_xy(k, np.stack([kf["x"], kf["y"]], 1))
        if kf["pose"] is not None:
            s.set_pose(k, kf["pose"])
        s.set_normals(k, kf["normals"])
        s.set_point_refs(k, ci.scene_refs(kf, k))
    s.update_connections(list(range(len(store))))
    return s


def _loop_devices(vo, name, n, **kw):
    sc = mi.loop_scene(name)
    out = []
    for _ in range(n):
        s = _loop_store(vo, sc, **kw)
        s.compute_sim3(sc["current"], sc["cand"], sc["rand"], ls.RAND_MAX, sc["fix_scale"], sc["max_rounds"])
        out.append(s)
    return sc, out


def _all_bytes(s, n):
    K = len(n)
    m = s.loop_merge_result()
    return (glf._states(s, n), [s.pose(k)[0].tobytes() for k in range(K)], [s.connections(k) for k in range(K)],
            {k: (v if k == "record" else v.tobytes()) for k, v in s.loop_correct_result().items()}, m["record"], m["per_feature"].tobytes(),
            s.recent_points())


def test_the_three_forms_give_the_same_bytes_behind_an_accepted_compute_sim3(vo):
    sc, (a, b, c) = _loop_devices(vo, "accepted", 3)
    res = a.loop_result()
    assert res["state"] == vo.KeyFrameStore.LOOP_ACCEPTED
    n = [len(kf["ids"]) for kf in sc["store"]]
    cur = sc["current"]
    for s in (a, b, c):
        s.propagate_loop()
    before = _all_bytes(a, n)
    match = np.ascontiguousarray(res["match_ids"][:n[cur]], np.int32)
    keep = _cuda(match)
    a.merge_loop_matches()                                        # the _loop form: curr and the list read in place
    b.merge_loop_matches(cur, match)                              # the host form
    c.merge_loop_matches(cur, keep)                               # the device form
    ra = _all_bytes(a, n)
    assert ra == _all_bytes(b, n), "the _loop form and the host form differ"
    assert ra == _all_bytes(c, n), "the _loop form and the device form differ"
    rec = ra[4]
    assert rec["curr"] == cur and rec["steps"] == int((match >= 0).sum()) > 20 and rec["replaces"] >= 1 and rec["moved"] >= 1
    assert ra[0] != before[0]
    assert a.connections_status() == b.connections_status() == c.connections_status() == 0


def test_loop_form_behind_a_rejected_compute_sim3(vo):
    sc, (a,) = _loop_devices(vo, "rejected", 1)
    assert a.loop_result()["state"] == vo.KeyFrameStore.LOOP_REJECTED
    n = [len(kf["ids"]) for kf in sc["store"]]
    a.connections_status()
    before = _all_bytes(a, n)
    a.merge_loop_matches()
    after = _all_bytes(a, n)
    assert after[:4] == before[:4] and after[6] == before[6] and after[4]["steps"] == 0 and not np.frombuffer(after[5], np.int32).any()
    assert a.connections_status() == vo.KeyFrameStore.CONNECTIONS_INVALID


@pytest.mark.parametrize("name", [ci.LOOP_SCENE, mi.LOOP_VARIANT])
def test_chain_behind_compute_sim3(vo, name):
    """compute_sim3 -> propagate_loop -> merge_loop_matches (_loop forms) -> search_and_fuse_loop -> loop_connections ->
    pose_graph_window_dev on the accepted loop scene with 255 shared points and on its variant with 104 (where the merge decides a
    family-A edge of the window), no array through the host: equal to the model's chain after the merge and at the end"""
    sc, (a,) = _loop_devices(vo, name, 1)
    res = a.loop_result()
    assert res["state"] == vo.KeyFrameStore.LOOP_ACCEPTED
    n = [len(kf["ids"]) for kf in sc["store"]]
    m = mi.scene_model(sc, lb._exp(vo), lb._log(vo))
    cur, match, ids = sc["current"], res["match_kf"], [int(x) for x in res["loop_point_ids"]]
    a.propagate_loop()
    assert m.propagate_loop(cur, lr.scw8_from13(res["Scw"])) is not None
    a.merge_loop_matches()
    m.merge_loop_matches(cur, [int(x) for x in res["match_ids"][:n[cur]]])
    glc._same_as_model(a, n, m, "merge_loop_matches")
    _same_merge(a, m, "merge_loop_matches")
    rec = a.loop_merge_result()["record"]
    assert rec["adds"] >= 1 and rec["replaces"] >= 1 and rec["moved"] >= 1 and rec["n_dead"] == 0 and rec["ordered"] == 0
    L = m.lc
    m.search_and_fuse(L["corr_kf"], L["S_corr"], ids, ci.CHAIN_TH)
    got, w = glc._chain_on_the_device(vo, a, cur, match)
    assert m.loop_connections() is not None
    want = m.pg_window(cur, match, m.lc_inputs())
    glc._same_chain_end(a, n, m, got, w, want, "the chain")
    _same_merge(a, m, "the chain")
    print("loop scene", name, ": merge", rec, "fusion", a.loop_fuse_result()["totals"], "window", w["record"])


def test_seeded_chain(vo):
    """the seeded 12 x 256 scene with a loop-side key-frame behind it and a seeded match list (60 replaces, 60 adds): the merge is
    what gives the current key-frame its connection of weight >= 100 to the loop side, a family-A edge of the window"""
    d = MDev(vo, fi.K_SCENE, fi.N_FEAT, merge=False, caps=fi.SCENE_CAPS, dev=True, max_recent=fi.SCENE_RECENT, max_candidates=fi.SCENE_CANDIDATES,
             max_corrected=ci.CHAIN_LC_CAPS[0], max_loop_points=lfi.CHAIN_LOOP_POINTS, form="dev")
    d.s.enable_pose_graph(4096, ci.CHAIN_LC_CAPS[0], ci.CHAIN_LC_CAPS[1])
    d.s.enable_loop_correct(*ci.CHAIN_LC_CAPS)
    d.s.enable_loop_merge()
    mrun, m = mi.seeded_chain_model(lb._exp(vo), lb._log(vo))
    where = glf._seeded_until_first_fuse(d, mrun)
    for s in ci.seeded_old_keyframe(m):
        d.step(s), mrun.step(s)
    glf._same(d, m, where)
    cur = ci.SEEDED_MATCH - 1
    Scw = ci.chain_scw(m, cur)
    keep = _cuda(np.array(Scw))
    d.s.propagate_loop(cur, keep)
    L = m.propagate_loop(cur, Scw)
    assert L is not None
    match = mi.seeded_match_ids(m, cur)
    d.merge(cur, match), m.merge_loop_matches(cur, match)
    glc._same_as_model(d.s, d.n, m, "merge_loop_matches")
    _same_merge(d.s, m, "merge_loop_matches")
    rec = d.s.loop_merge_result()["record"]
    assert rec["adds"] == 60 and rec["replaces"] == 60 and rec["moved"] >= 1 and rec["n_dead"] == 0
    ids = ci.seeded_loop_ids(m, 0)
    tensor = _cuda(np.array(ids, np.int32))
    m.search_and_fuse(L["corr_kf"], L["S_corr"], ids, ci.CHAIN_TH)
    got, w = glc._chain_on_the_device(vo, d.s, cur, ci.SEEDED_MATCH, tensor)
    assert m.loop_connections() is not None
    want = m.pg_window(cur, ci.SEEDED_MATCH, m.lc_inputs())
    glc._same_chain_end(d.s, d.n, m, got, w, want, "the chain")
    assert d.s.recent_points() == m.recent_points()
    print("seeded scene: merge", rec, "fusion", m.loop_fuse_result()["totals"], "window", w["record"])


# ---- correct_loop -------------------------------------------------------------------------------------------------------------
def _everything(s, n):
    K = len(n)
    return _all_bytes(s, n) + ([s.loop_edges(k) for k in range(K)], [s.cull_state(k) for k in range(K)], s.loop_fuse_result(),
                               s.pose_graph_window_result()["record"], s.connections_status())


def _steps_1_to_6(vo, s, th):
    """the step-wise sequence through the binding up to the loop connections -> (match, the layer's record, its arrays)"""
    res = s.loop_result()
    s.propagate_loop()
    s.merge_loop_matches()
    rec = s.loop_correct_result()["record"]
    A = s.loop_correct_arrays()
    vo.check(vo.lib().vo_kfstore_search_and_fuse_loop(s._h, rec["n_corr"], vo._p(A["corr_kf"]), vo._p(A["S_corr"]), C.c_float(th)),
             "vo_kfstore_search_and_fuse_loop")
    s.loop_connections()
    return res["match_kf"], s.loop_correct_result()["record"], A


def test_correct_loop_equals_the_step_wise_sequence(vo):
    sc, (a, b) = _loop_devices(vo, ci.LOOP_SCENE, 2)
    n = [len(kf["ids"]) for kf in sc["store"]]
    cur = sc["current"]
    assert _everything(a, n) == _everything(b, n)
    summary, record = a.correct_loop(ci.CHAIN_TH, 20)
    match, rec, A = _steps_1_to_6(vo, b, ci.CHAIN_TH)
    vo.check(vo.lib().vo_kfstore_pose_graph_window_dev(b._h, cur, match, rec["n_corr"], vo._p(A["corr_kf"]), vo._p(A["S_corr"]), vo._p(A["S_uncorr"]),
                                                       vo._p(A["lc_start"]), rec["n_lc"], vo._p(A["lc_kf"]), rec["n_cp"], vo._p(A["cp_id"]),
                                                       vo._p(A["cp_ref"])), "vo_kfstore_pose_graph_window_dev")
    w = b.pose_graph_window_result()
    assert w["record"]["status"] == pr.OK
    q, t, _ = vo.Optimizer.solvePoseGraphLoop(w, 20)
    b.pose_graph_apply(q, t)
    b.add_loop_edge(cur, match)
    ea, eb = _everything(a, n), _everything(b, n)
    for i, (x, y) in enumerate(zip(ea, eb)):
        assert x == y, ("the composed call and the step-wise sequence differ", i)
    mrec, frec, wrec = a.loop_merge_result()["record"], a.loop_fuse_result()["totals"], a.pose_graph_window_result()["record"]
    assert record == dict(curr=cur, match=match, n_corr=rec["n_corr"], n_cp=rec["n_cp"], n_lc=rec["n_lc"], merge_adds=mrec["adds"],
                          merge_replaces=mrec["replaces"], fuse_adds=frec[2], fuse_replaces=frec[3], n_nodes=wrec["n_nodes"],
                          n_edges=wrec["n_edges"], n_points_moved=wrec["n_points_moved"], stopped_at=0), record
    assert record["merge_adds"] >= 1 and record["merge_replaces"] >= 1 and record["n_points_moved"] >= 1 and record["n_edges"] >= 1
    assert a.loop_edges(cur) == [match] and a.loop_edges(match) == [cur]
    assert a.cull_state(cur)["locked"] == 1 and a.cull_state(match)["locked"] == 1
    print("correct_loop record:", record)


def _refused(vo, s, status):
    with pytest.raises(vo.VoError) as e:
        s.correct_loop(ci.CHAIN_TH, 20)
    assert ("status %d" % status) in str(e.value), str(e.value)
    return s.correct_loop_record


def test_correct_loop_not_accepted(vo):
    sc, (a,) = _loop_devices(vo, "rejected", 1)
    n = [len(kf["ids"]) for kf in sc["store"]]
    a.connections_status()
    before = _everything(a, n)
    rec = _refused(vo, a, -1)
    assert rec["stopped_at"] == 1 and rec["n_corr"] == 0
    after = _everything(a, n)
    assert after[:3] == before[:3] and after[6:10] == before[6:10] and after[-1] == vo.KeyFrameStore.CONNECTIONS_INVALID


def test_correct_loop_overflowed_propagation(vo):
    """the propagation overflows (on every compute_sim3 scene the current key-frame has no neighbour, so n_corr is 1 and
    max_corrected >= 1 cannot be exceeded: the corrected points are what overflows): VO_ERR_CAPACITY, the store as steps 1 - 2 leave it"""
    sc, (a, b) = _loop_devices(vo, ci.LOOP_SCENE, 2, lc_caps=(LOOP_LC_CAPS[0], 16, LOOP_LC_CAPS[2]))
    n = [len(kf["ids"]) for kf in sc["store"]]
    rec = _refused(vo, a, -4)
    assert rec["stopped_at"] == 1 and rec["n_cp"] > 16
    b.propagate_loop(), b.merge_loop_matches()
    assert _everything(a, n) == _everything(b, n)


def test_correct_loop_overflowed_window(vo):
    """more loop connections than the pose graph was enabled for: VO_ERR_CAPACITY at step 7, the store as steps 1 - 6 leave it"""
    sc, (a, b) = _loop_devices(vo, ci.LOOP_SCENE, 2, max_edges=2)
    n = [len(kf["ids"]) for kf in sc["store"]]
    rec = _refused(vo, a, -4)
    assert rec["stopped_at"] == 7 and rec["n_lc"] > 2
    _steps_1_to_6(vo, b, ci.CHAIN_TH)
    ea, eb = _everything(a, n), _everything(b, n)
    assert ea[:10] == eb[:10] and ea[-1] == eb[-1] and ea[7] == [[] for _ in n]


def test_correct_loop_solver_refusal_writes_nothing_back(vo):
    """compute_sim3 with free scales is accepted, vo_pose_graph_solve refuses free scales: its status is returned, nothing is
    written back by step 7 or 8, the store is as steps 1 - 6 leave it"""
    sc, (a, b) = _loop_devices(vo, "free_scale", 2)
    assert a.loop_result()["state"] == vo.KeyFrameStore.LOOP_ACCEPTED
    n = [len(kf["ids"]) for kf in sc["store"]]
    rec = _refused(vo, a, -1)
    assert rec["stopped_at"] == 7 and rec["n_nodes"] >= 2 and rec["n_edges"] >= 1
    _steps_1_to_6(vo, b, ci.CHAIN_TH)
    ea, eb = _everything(a, n), _everything(b, n)
    assert ea[:10] == eb[:10] and ea[-1] == eb[-1] and ea[7] == [[] for _ in n]
