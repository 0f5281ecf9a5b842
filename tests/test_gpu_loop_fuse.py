"""The loop fusion on the device against the model tests/loop_fuse_ref.py, through the binding:
vo_kfstore_search_and_fuse, its _dev and _loop forms and vo_kfstore_loop_fuse_result.  Everything is compared byte for byte:
flags, ids, points, normals, min / max, ref_kf, point_desc, the recent list, the record and per_pass, the connection state and
the sticky word; the generation word and the stale index through the calls that depend on them.  No tolerance: the call copies
attributes and decides gates; tests/test_loop_fuse_ref.py holds the conditions on the inputs (every float gate decides with a
margin).  What a case is about is asserted to have occurred, through per_pass or the model's log."""
import ctypes as C

import numpy as np
import pytest

import fuse_inputs as fi
import loop_fuse_inputs as lfi
import loop_sim3_inputs as lsi
import point_upkeep_inputs as ui
import pose_graph_store_ref as pr
from fuse_ref import LEVEL_MARGIN, MARGIN

from test_gpu_fuse import FDev, _same
from test_gpu_local_ba_store import _exp, _log

pytestmark = pytest.mark.gpu


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class LDev(FDev):
    """test_gpu_fuse.FDev with the opt-in and the loop step; form: "host" or "dev" (the step's arrays as device tensors)"""

    def __init__(self, vo, K, NK, caps=fi.CAPS, dev=False, max_recent=ui.MAX_RECENT, max_candidates=fi.MAX_CANDIDATES,
                 max_corrected=lfi.MAX_CORRECTED, max_loop_points=lfi.MAX_LOOP_POINTS, form="host", stream=None, **kw):
        super().__init__(vo, K, NK, caps, dev, max_recent, max_candidates, **kw)
        self.form = form
        if stream is not None:
            assert vo.lib().vo_kfstore_set_stream(self.s._h, vo._p(stream)) == 0
        if max_corrected is not None:
            self.s.enable_loop_fuse(max_corrected, max_loop_points)

    def loopfuse(self, corr_kf, S_corr, ids, th):
        ck, sc, a = np.asarray(corr_kf, np.int32), np.asarray(S_corr, np.float64).reshape(-1, 8), np.asarray(ids, np.int32)
        if self.form == "dev":
            ck, sc, a = _cuda(ck), _cuda(sc), _cuda(a)
            self.keep += [ck, sc, a]
        self.s.search_and_fuse(ck, sc, a, th)

    def step(self, s):
        if s[0] == "loopfuse":
            self.loopfuse(*s[1:5])
        else:
            super().step(s)


def _model(vo, **kw):
    return lfi.ModelRunner(exp=_exp(vo), log=_log(vo), **kw)


def _same_call(d, m, where):
    _same(d, m, where, result=False)
    got = d.s.loop_fuse_result()
    assert got == m.loop_fuse_result(), (where, got, m.loop_fuse_result())


def _run(vo, c, form="host", th=None, **kw):
    K = sum(1 for s in c["script"] if s[0] == "insert")
    caps = {k: c[k] for k in ("max_candidates", "caps") if k in c}
    d, mr = LDev(vo, K, c["NK"], form=form, **caps, **kw), _model(vo, **caps, **kw)
    step = ("loopfuse", c["corr_kf"], c["S_corr"], c["ids"], c["th"] if th is None else th)
    for s in c["script"] + [step]:
        d.step(s), mr.step(s)
    _same_call(d, mr.m, step[:2])
    return d, mr.m, step


# ---- the hand-made stores: one call each, then the same call again ----------------------------------------------------------
@pytest.mark.parametrize("name", lfi.HAND_CASES)
def test_hand_cases(vo, name):
    c = lfi.hand_case(name)
    d, m, step = _run(vo, c, form="dev" if name in ("add", "same_org_two_features", "dies_in_pass_1") else "host")
    assert m.loop_fuse_result()["per_pass"] == c["per_pass"]
    if name == "two_on_one_empty_feature":
        assert [e[4:] for e in m.lf_log] == [("add", -1), ("replace", 700)]           # the second replaces the first
    if name == "replace_three_holders":
        assert m.lf_moved[0][3] == 2 and m.loop_fuse_result()["totals"][5] == 1       # two features go over, key-frame 3's is cleared
    if name in ("same_org_one_feature", "same_org_two_features"):
        assert [x[3] > 0 for x in m.lf_moved] == [True, False]                        # the second replace moves nothing
    if name == "dies_in_pass_1":
        assert (1, 0, 700, "bad") in m.lf_gates
    if name == "already_held":
        assert (0, 0, c["ids"][0], "held") in m.lf_gates
    if name == "targets_erased_or_without_a_pose":
        assert m.erased[4] and m.store[5]["pose"] is None
    # the same call again finds what the first left, and the model agrees
    d.step(step), m.search_and_fuse(*step[1:])
    _same_call(d, m, "second call")


def test_counters_are_added_twice_when_both_are_listed(vo):
    c = lfi.counters_case()
    before = {e[0]: e[2:] for e in lfi.run_model(c["script"]).recent_points()}
    d, m, _ = _run(vo, c)
    got = {e[0]: e[2:] for e in d.s.recent_points()}
    for b in (700, 701):
        assert got[b] == (before[b][0] + before[900][0], before[b][1] + before[900][1])
    assert got[900] == before[900] and [x[3] for x in m.lf_moved] == [2, 0]


def test_z_just_above_zero_and_behind_the_camera(vo):
    d, m, _ = _run(vo, lfi.z_case())
    assert [g[3] for g in m.lf_gates] == ["gates", "gates"] and m.loop_fuse_result()["totals"] == (0,) * 6


def test_the_unscaled_translation_decides_which_feature_wins(vo):
    """quirk 1 (matcher.cpp:1144): the device's add is where the model with t as it stands puts it, not where t / s would"""
    c = lfi.hand_case("scale_quirk")
    d, m, _ = _run(vo, c)
    other = lfi.run_model(c["script"])
    other.divide_t = True
    other.search_and_fuse(c["corr_kf"], c["S_corr"], c["ids"], c["th"])
    T, f, g = c["corr_kf"][0], m.lf_log[0][3], other.lf_log[0][3]
    ids = d.state(T)["ids"]
    assert f != g and ids[f] == c["ids"][0] and ids[g] != c["ids"][0]


def test_threshold_4_against_3(vo):
    c = lfi.hand_case("threshold")
    _, m4, _ = _run(vo, c, th=4.0)
    _, m3, _ = _run(vo, c, th=3.0)
    assert m4.loop_fuse_result()["totals"][1:3] == (1, 1) and m3.loop_fuse_result()["totals"][:3] == (1, 0, 0)


# ---- the three limits, each hit once ------------------------------------------------------------------------------------------
def test_candidate_capacity(vo):
    d, m, _ = _run(vo, lfi.capacity_candidates_case())
    assert m.loop_fuse_result()["per_pass"] == [(3, 1, 0, 0, 0, 0)] and m.undone[-1][1] == "candidates"


def test_match_capacity(vo):
    d, m, _ = _run(vo, lfi.capacity_matches_case())
    assert [r[2] for r in m.loop_fuse_result()["per_pass"]] == [1, 1, 0, 0] and [u[1] for u in m.undone] == ["matches", "matches"]


def test_carrier_capacity(vo):
    c = lfi.capacity_carriers_case()
    d, mr = LDev(vo, c["K"], c["NK"], caps=c["caps"]), _model(vo, caps=c["caps"])
    for s in c["script"] + [("loopfuse", c["corr_kf"], c["S_corr"], c["ids"], c["th"])]:
        d.step(s), mr.step(s)
    m = mr.m
    assert len(m.carriers(900)) == vo.KeyFrameStore.FUSE_MAX_CARRIERS + 1 and m.loop_fuse_result()["per_pass"] == [(1, 1, 0, 1, 0, 0)]
    assert m.sticky == vo.KeyFrameStore.CONNECTIONS_FUSE_CAPACITY
    _same_call(d, m, "carriers")


# ---- refusals, opt-in ---------------------------------------------------------------------------------------------------------
def test_opt_in_and_refusals(vo):
    L = vo.lib()
    th = C.c_float(4.0)
    c = lfi.hand_case("add")
    ck, sc, ids = np.array(c["corr_kf"], np.int32), np.array(c["S_corr"], np.float64), np.array(c["ids"], np.int32)
    plain = FDev(vo, 4, 16)                                                    # no enable_loop_fuse
    for rc in (L.vo_kfstore_search_and_fuse(plain.s._h, 1, vo._p(ck), vo._p(sc), 1, vo._p(ids), th),
               L.vo_kfstore_search_and_fuse_dev(plain.s._h, 1, vo._p(ck), vo._p(sc), 1, vo._p(ids), th),
               L.vo_kfstore_search_and_fuse_loop(plain.s._h, 1, vo._p(ck), vo._p(sc), th), L.vo_kfstore_loop_fuse_result(plain.s._h, None, None)):
        assert rc == -1
    no_fuse = FDev(vo, 4, 16, max_candidates=None)
    assert L.vo_kfstore_enable_loop_fuse(no_fuse.s._h, 4, 16) == -1            # no enable_fuse
    assert L.vo_kfstore_enable_loop_fuse(plain.s._h, 0, 16) == -1 and L.vo_kfstore_enable_loop_fuse(plain.s._h, 4, 0) == -1
    plain.s.enable_loop_fuse(4, 16)                                            # (through the binding, which sizes per_pass by it)
    assert L.vo_kfstore_enable_loop_fuse(plain.s._h, 4, 16) == 0               # a second time: nothing to do
    assert plain.s.loop_fuse_result() == dict(passes=0, per_pass=[], totals=(0,) * 6)
    K = sum(1 for s in c["script"] if s[0] == "insert")
    d, mr = LDev(vo, K, c["NK"], max_corrected=2, max_loop_points=4), _model(vo, max_corrected=2, max_loop_points=4)
    for s in c["script"]:
        d.step(s), mr.step(s)
    h = d.s._h
    assert L.vo_kfstore_enable_loop_fuse(h, 2, 4) == -1                        # the store holds key-frames
    two, s2 = np.array([6, 5], np.int32), np.array(c["S_corr"] * 2, np.float64)
    three, s3, five = np.array([3, 5, 6], np.int32), np.array(c["S_corr"] * 3, np.float64), np.zeros(5, np.int32)
    for rc, want in ((L.vo_kfstore_search_and_fuse(h, 2, vo._p(two), vo._p(s2), 1, vo._p(ids), th), -1),           # not ascending
                     (L.vo_kfstore_search_and_fuse(h, 2, vo._p(np.array([6, 6], np.int32)), vo._p(s2), 1, vo._p(ids), th), -1),
                     (L.vo_kfstore_search_and_fuse(h, 1, vo._p(ck), vo._p(sc), 1, vo._p(ids), C.c_float(0.0)), -1),
                     (L.vo_kfstore_search_and_fuse(h, 1, vo._p(ck), vo._p(sc), 1, vo._p(ids), C.c_float(-1.0)), -1),
                     (L.vo_kfstore_search_and_fuse(h, 1, None, vo._p(sc), 1, vo._p(ids), th), -1),
                     (L.vo_kfstore_search_and_fuse(h, 1, vo._p(ck), None, 1, vo._p(ids), th), -1),
                     (L.vo_kfstore_search_and_fuse(h, 1, vo._p(ck), vo._p(sc), 1, None, th), -1),
                     (L.vo_kfstore_search_and_fuse(h, -1, vo._p(ck), vo._p(sc), 1, vo._p(ids), th), -1),
                     (L.vo_kfstore_search_and_fuse(h, 1, vo._p(ck), vo._p(sc), -1, vo._p(ids), th), -1),
                     (L.vo_kfstore_search_and_fuse_dev(h, 1, None, None, 1, None, th), -1),
                     (L.vo_kfstore_search_and_fuse_dev(h, 1, vo._p(ck), vo._p(sc), 1, vo._p(ids), C.c_float(0.0)), -1),
                     (L.vo_kfstore_search_and_fuse_loop(h, 1, vo._p(ck), vo._p(sc), th), -1),                       # no enable_loop
                     (L.vo_kfstore_search_and_fuse(h, 3, vo._p(three), vo._p(s3), 1, vo._p(ids), th), -4),          # n_corr > max_corrected
                     (L.vo_kfstore_search_and_fuse(h, 1, vo._p(ck), vo._p(sc), 5, vo._p(five), th), -4),            # n_points > max_loop_points
                     (L.vo_kfstore_search_and_fuse_dev(h, 3, vo._p(three), vo._p(s3), 1, vo._p(ids), th), -4)):
        assert rc == want
    assert d.s.loop_fuse_result() == dict(passes=0, per_pass=[], totals=(0,) * 6)
    _same(d, mr.m, "after the refused calls", result=False)                    # nothing changed
    assert L.vo_kfstore_search_and_fuse(h, 0, None, None, 0, None, th) == 0 and d.s.loop_fuse_result()["passes"] == 0
    d.loopfuse(c["corr_kf"], c["S_corr"], c["ids"], c["th"]), mr.m.search_and_fuse(c["corr_kf"], c["S_corr"], c["ids"], c["th"])
    _same_call(d, mr.m, "a good call after them")


def test_a_key_frame_number_outside_the_store_is_decided_on_the_device(vo):
    """the device form validates nothing but counts on the host: pass 2 names key-frame 99"""
    c = lfi.hand_case("add")
    c = dict(c, corr_kf=[c["corr_kf"][0], 99], S_corr=c["S_corr"] * 2, per_pass=c["per_pass"] + [(0,) * 6])
    d, m, _ = _run(vo, c, form="dev")
    assert m.loop_fuse_result()["per_pass"] == c["per_pass"]


def test_the_generation_advances_and_the_index_is_stale(vo):
    """a local-BA window taken before the call is no longer the store's; the connection update behind the call sees the added
    observations (the index has been rebuilt)"""
    c = lfi.hand_case("add")
    K = sum(1 for s in c["script"] if s[0] == "insert")
    d, mr = LDev(vo, K, c["NK"]), _model(vo)
    for s in c["script"] + [("update", list(range(K)))]:
        d.step(s), mr.step(s)
    T = c["corr_kf"][0]
    before = d.s.connections(T)
    d.s.local_ba_window(T), mr.m.window(T)
    step = ("loopfuse", c["corr_kf"], c["S_corr"], c["ids"], c["th"])
    d.step(step), mr.step(step)
    with pytest.raises(vo.VoError, match="changed since"):
        d.s.local_ba_apply(np.zeros((1, 6)), np.zeros((1, 3)), np.zeros(1, np.uint8))
    _same_call(d, mr.m, "not updated by the call")                           # (connections included: unchanged so far)
    assert d.s.connections(T) == before
    d.step(("update", [T])), mr.step(("update", [T]))
    _same_call(d, mr.m, "updated")


# ---- the forms ----------------------------------------------------------------------------------------------------------------
def _states(s, n):
    out = []
    for k, nk in enumerate(n):
        p = s.points(k, nk)
        out.append(tuple(np.asarray(p[key]).tobytes() for key in ("flags", "ids", "points", "normals", "min_dist", "max_dist", "point_desc"))
                   + (np.asarray(s.point_refs(k, nk)).tobytes(),))
    return out


def test_host_and_device_forms_give_the_same_bytes(vo):
    c = lfi.hand_case("not_a_multiple_of_64")
    (dh, mh, _), (dd, md, _) = _run(vo, c, form="host"), _run(vo, c, form="dev")
    assert _states(dh.s, dh.n) == _states(dd.s, dd.n) and dh.s.loop_fuse_result() == dd.s.loop_fuse_result()
    assert dh.s.loop_fuse_result()["totals"][1] == 2


def test_the_device_form_behind_its_inputs_producer(vo):
    """the call is made while the producer of its inputs is still enqueued on the store's stream: it returns with the stream
    busy, and the result is the model's"""
    import torch
    c = lfi.hand_case("two_on_one_empty_feature")
    K = sum(1 for s in c["script"] if s[0] == "insert")
    st = torch.cuda.Stream()
    d, mr = LDev(vo, K, c["NK"], stream=st.cuda_stream), _model(vo)
    for s in c["script"]:
        d.step(s), mr.step(s)
    host = [torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for a in
            (np.array(c["corr_kf"], np.int32), np.array(c["S_corr"], np.float64), np.array(c["ids"], np.int32))]
    with torch.cuda.stream(st):
        torch.cuda._sleep(200_000_000)                     # a tenth of a second of device time in front of the inputs
        ck, sc, ids = (t.to("cuda", non_blocking=True) for t in host)
        d.s.search_and_fuse(ck, sc, ids, c["th"])
        busy = not st.query()
    mr.m.search_and_fuse(c["corr_kf"], c["S_corr"], c["ids"], c["th"])
    _same_call(d, mr.m, "producer")
    assert busy and mr.m.loop_fuse_result()["totals"][1] == 2


def _loop_store(vo, sc):
    """loop_sim3_inputs.build_device with the loop fusion enabled too (every opt-in comes before the first key-frame)"""
    store = sc["store"]
    s = vo.KeyFrameStore(len(store), lsi.NK)
    s.enable_connections(), s.enable_culling(), s.enable_mapping(lsi.CAM6, lsi.SF, 50000), s.enable_local_ba(*lsi.BA_CAPS)
    s.enable_point_upkeep(lsi.MAX_RECENT), s.enable_fuse(lsi.BOUNDS, 1024), s.enable_loop(**sc["caps"])
    s.enable_loop_fuse(4, sc["caps"]["max_loop_points"])
    for k, kf in enumerate(store):
        s.insert(dict(angle=kf["angle"], desc=kf["desc"], flags=kf["flags"], points=kf["points"], ids=kf["ids"], point_desc=kf["point_desc"],
                      min_dist=kf["min_dist"], max_dist=kf["max_dist"], nodes=kf["nodes"], bad=kf["bad"]))
        s.set_keypoints(k, kf["octave"], kf["depth"], kf["uright"])
        s.set_keypoint_xy(k, np.stack([kf["x"], kf["y"]], 1))
        if kf["pose"] is not None:
            s.set_pose(k, kf["pose"])
        s.set_normals(k, kf["normals"])
    s.update_connections(list(range(len(store))))
    return s


def _loop_devices(vo, name, n):
    sc = lsi.scene(name)
    out = []
    for _ in range(n):
        s = _loop_store(vo, sc)
        s.compute_sim3(sc["current"], sc["cand"], sc["rand"], lsi.RAND_MAX, sc["fix_scale"], sc["max_rounds"])
        out.append(s)
    return sc, out


def test_loop_form_behind_an_accepted_compute_sim3(vo):
    """the list compute_sim3 left on the device, read in place, against the host and device forms given the same ids on stores
    built the same way: the same bytes.  The current key-frame is corrected to the loop's Scw (it gains the loop points it
    sees), the match's neighbour 0 to its own pose"""
    sc, (a, b, c) = _loop_devices(vo, "accepted", 3)
    res = a.loop_result()
    assert res["state"] == vo.KeyFrameStore.LOOP_ACCEPTED and len(res["loop_point_ids"]) > 20
    Scw = res["Scw"]
    Rq = pr.normalize(pr.quat_from_matrix([float(x) for x in Scw[:9]]))
    cur = sc["current"]
    corr = np.array([0, cur], np.int32)
    S = np.array([pr.from_pose([float(x) for x in sc["store"][0]["pose"]]), Rq + [float(x) for x in Scw[9:12]] + [float(Scw[12])]])
    n = [len(kf["ids"]) for kf in sc["store"]]
    before = _states(a, n)
    keep = (_cuda(corr), _cuda(S), _cuda(res["loop_point_ids"].astype(np.int32)))
    a.search_and_fuse(keep[0], keep[1])                                     # the _loop form
    b.search_and_fuse(corr, S, res["loop_point_ids"], 4.0)                  # the host form
    c.search_and_fuse(*keep, 4.0)                                           # the device form
    ra = a.loop_fuse_result()
    assert ra == b.loop_fuse_result() == c.loop_fuse_result() and ra["passes"] == 2
    assert ra["totals"][0] > 20 and ra["totals"][1] > 0, ra
    assert a.connections_status() == b.connections_status() == c.connections_status() == 0
    sa = _states(a, n)
    assert sa == _states(b, n), "the _loop form and the host form differ"
    assert sa == _states(c, n), "the _loop form and the device form differ"
    assert sa != before and ra["totals"][2] + ra["totals"][4] > 0, ra       # something was added or moved


def test_loop_form_behind_a_rejected_compute_sim3(vo):
    sc, (a,) = _loop_devices(vo, "rejected", 1)
    res = a.loop_result()
    assert res["state"] == vo.KeyFrameStore.LOOP_REJECTED
    n = [len(kf["ids"]) for kf in sc["store"]]
    before = _states(a, n)
    a.connections_status()
    corr, S = np.array([0], np.int32), np.array([pr.from_pose([float(x) for x in sc["store"][0]["pose"]])])
    keep = (_cuda(corr), _cuda(S))
    a.search_and_fuse(keep[0], keep[1])
    assert a.loop_fuse_result() == dict(passes=0, per_pass=[], totals=(0,) * 6)
    assert _states(a, n) == before and a.connections_status() == vo.KeyFrameStore.CONNECTIONS_INVALID


# ---- the seeded scene ---------------------------------------------------------------------------------------------------------
def _seeded_until_first_fuse(d, mr):
    for i, s in enumerate(fi.seeded_chain()):
        d.step(s), mr.step(s)
        if s[0] == "create":
            for k in range(len(mr.m.store)):
                got = d.state(k)
                mr.m.set_map_side(k, got["points"], got["normals"], got["min_dist"], got["max_dist"])
        if s[0] == "neighbors":
            return (i, s[:2])


def test_a_store_without_the_layer_returns_the_same_bytes(vo):
    """search_in_neighbors on the seeded scene, with the layer enabled but unused and without it"""
    out = []
    for layer in (lfi.MAX_CORRECTED, None):
        d = LDev(vo, fi.K_SCENE, fi.N_FEAT, fi.SCENE_CAPS, True, fi.SCENE_RECENT, fi.SCENE_CANDIDATES, max_corrected=layer)
        mr = fi.ModelRunner(fi.SCENE_CAPS, exp=_exp(vo), log=_log(vo), max_recent=fi.SCENE_RECENT, max_candidates=fi.SCENE_CANDIDATES)
        where = _seeded_until_first_fuse(d, mr)
        _same(d, mr.m, where)
        out.append((_states(d.s, d.n), d.s.fuse_result(), d.s.recent_points(), [d.s.connections(k) for k in range(len(d.n))]))
    assert out[0] == out[1] and out[0][1]["totals"][1] > 20


def test_seeded_chain(vo):
    """insert ... search_in_neighbors -> search_and_fuse (3 corrected key-frames) -> update_connections -> pose_graph_window on the
    seeded 12 x 256 scene, equal to the model's chain at every step"""
    d = LDev(vo, fi.K_SCENE, fi.N_FEAT, fi.SCENE_CAPS, True, fi.SCENE_RECENT, fi.SCENE_CANDIDATES, max_loop_points=lfi.CHAIN_LOOP_POINTS, form="dev")
    d.s.enable_pose_graph(4096, 8, 8)
    mr = lfi.ModelRunner(fi.SCENE_CAPS, exp=_exp(vo), log=_log(vo), max_recent=fi.SCENE_RECENT, max_candidates=fi.SCENE_CANDIDATES,
                         max_loop_points=lfi.CHAIN_LOOP_POINTS, model=lfi.ChainModel)
    where = _seeded_until_first_fuse(d, mr)
    m = mr.m
    _same(d, m, where)
    corr, S, ids = lfi.chain_inputs(m)
    n0 = len(m.margins)
    step = ("loopfuse", corr, S, ids, lfi.TH)
    d.step(step), mr.step(step)
    _same_call(d, m, "search_and_fuse")
    res = m.loop_fuse_result()
    assert res["passes"] == 3 and res["totals"][0] > 20 and res["totals"][2] >= 2
    assert not m.weak and min(x for _, x in m.margins[n0:]) >= MARGIN and min(m.level_fracs) >= LEVEL_MARGIN, sorted(m.weak)
    d.step(("update", corr)), mr.step(("update", corr))
    _same_call(d, m, "update_connections")
    cur = len(m.store) - 1
    inp = pr.make_inputs({k: (s, pr.from_pose(m.store[k]["pose"])) for k, s in zip(corr, S)}, {}, {})
    want = m.pg_window(cur, corr[0], inp)
    d.s.pose_graph_window(cur, corr[0], inp)
    got = d.s.pose_graph_window_result()
    assert {k: got["record"][k] for k in pr.PG_RECORD} == m.pg_record and want is not None and got["record"]["n_edges"] > 0
    for key, w in want.items():
        assert got[key].tobytes() == w.tobytes(), key
    assert d.s.connections_status() == m.sticky
