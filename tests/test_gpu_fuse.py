"""Map-point fusion on the device against the model tests/fuse_ref.py, through the binding:
vo_kfstore_fuse_map_points and vo_kfstore_search_in_neighbors.  Everything is compared byte for byte: flags, ids, points,
normals, min / max, ref_kf, point_desc, the recent list, the result arrays, the connection state and the sticky word.  No
tolerance: a fuse copies attributes, and the only floating-point results written are section 4k's refresh, which is exact
against its model.  tests/test_fuse_ref.py holds the conditions on the inputs (every float gate decides with a margin)."""
import numpy as np
import pytest

import fuse_inputs as fi
import point_upkeep_inputs as ui
from collections import Counter

from fuse_ref import LEVEL_MARGIN, MARGIN, STEP

from test_gpu_local_ba_store import _exp, _log
from test_gpu_point_upkeep import UDev

pytestmark = pytest.mark.gpu


class FDev(UDev):
    """test_gpu_point_upkeep.UDev with the opt-in and the three new steps"""

    def __init__(self, vo, K, NK, caps=fi.CAPS, dev=False, max_recent=ui.MAX_RECENT, max_candidates=fi.MAX_CANDIDATES, **kw):
        super().__init__(vo, K, NK, caps, dev, max_recent, **kw)
        if max_candidates is not None:
            self.s.enable_fuse(fi.BOUNDS, max_candidates)

    def step(self, s):
        if s[0] == "refresh":
            self.s.refresh_points(s[1])
        elif s[0] == "fuse":
            self.s.fuse_map_points(s[1], self._list(s[2]))
        elif s[0] == "neighbors":
            self.s.search_in_neighbors(s[1])
        else:
            super().step(s)


def _model(vo, caps=fi.CAPS, max_recent=ui.MAX_RECENT, max_candidates=fi.MAX_CANDIDATES):
    return fi.ModelRunner(caps, exp=_exp(vo), log=_log(vo), max_recent=max_recent, max_candidates=max_candidates)


def _same(d, m, where, result=True):
    K = len(m.store)
    for k in range(K):
        got, want = d.state(k), m.state(k)
        for key, w in want.items():
            assert np.asarray(got[key]).tobytes() == np.asarray(w).tobytes(), (where, k, key)
    assert [d.s.connections(k) for k in range(K)] == [m.connections(k) for k in range(K)], where
    assert d.s.recent_points() == m.recent_points(), where
    if result:
        got = d.s.fuse_result()
        assert got == m.fuse_result(), (where, got, m.fuse_result())
    assert d.s.connections_status() == m.sticky, where
    m.sticky = 0


def _run(vo, script, K, NK, dev=False, check=("fuse", "neighbors"), **kw):
    d, mr = FDev(vo, K, NK, dev=dev, **kw), _model(vo, **{k: v for k, v in kw.items() if k in ("caps", "max_recent", "max_candidates")})
    for i, s in enumerate(script):
        d.step(s), mr.step(s)
        if s[0] in check:
            _same(d, mr.m, (i, s[:2]))
    return d, mr.m


# ---- one fuse call on hand-made stores --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fi.HAND_CASES)
def test_hand_cases(vo, name):
    c = fi.hand_case(name)
    d, m = _run(vo, c["script"] + [("fuse",) + c["fuse"]], 7, c["NK"], dev=name in ("add", "three_on_one_feature"))
    assert [(k, o) for _, _, _, k, o in m.fuse_log] == c["kinds"]
    if name == "tie_by_cell_order":
        assert m.fuse_log[0][2] == 1          # the second feature of the target: the lower cell column
    # a second call finds nothing left to do but what the first left, and the model agrees
    d.step(("fuse",) + c["fuse"]), m.fuse_map_points(*c["fuse"])
    _same(d, m, "second call")


@pytest.mark.parametrize("both", [True, False], ids=["both_listed", "one_listed"])
def test_counters_merge_only_when_both_are_listed(vo, both):
    c = fi.counters_case(both)
    d, m = _run(vo, c["script"] + [("fuse",) + c["fuse"]], 7, c["NK"])
    got = {e[0]: e[2:] for e in d.s.recent_points()}
    assert set(c["listed"]) <= set(got)
    assert got[700] == (3, 4)                 # the one that goes keeps its entry and its counters
    if both:
        assert got[701] == (2 + 3, 6 + 4)


@pytest.mark.parametrize("how", ["bad", "erased", "no_pose"])
def test_target_bad_erased_or_without_a_pose(vo, how):
    c = fi.hand_case("add")
    script = list(c["script"])
    if how == "no_pose":
        script = [s for s in script if not (s[0] == "pose" and s[1] == fi.T_HAND)]
    else:
        script.append(("bad" if how == "bad" else "erase", fi.T_HAND))
    d, m = _run(vo, script + [("fuse",) + c["fuse"]], 7, c["NK"])
    assert m.fuse_result()["totals"][2] == (1 if how == "bad" else 0)     # fuseMapPoints does not ask whether its key-frame is bad
    d.step(("fuse", fi.T_HAND, [])), m.fuse_map_points(fi.T_HAND, [])    # an empty list raises the same sticky word
    assert m.sticky == (0 if how == "bad" else 1)
    _same(d, m, "empty list")


@pytest.mark.parametrize("n", [64, 65])
def test_a_point_with_64_or_65_holders_is_replaced(vo, n):
    c = fi.holders_case(n)
    d, m = _run(vo, c["script"] + [("fuse",) + c["fuse"]], c["K"], c["NK"], caps=(80, 256, 1024))
    res = m.fuse_result()
    assert res["totals"] == (1, 1, 0, 0, 1, n - 1) and len(m.observations(500)) == n + 1 and not m.carriers(900)


# ---- the composed call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad_first", [False, True], ids=["", "first_neighbour_bad"])
def test_target_list(vo, bad_first):
    script, current = fi.graph_case(bad_first)
    d, m = _run(vo, script + [("neighbors", current)], 14, 64, caps=(16, 512, 8192))
    t = m.fuse_result()["targets"]
    first = [k for k in m.conn.ordered[current][:10] if not m.store[k]["bad"]]
    assert len(m.conn.ordered[current]) > 10 and t[-1] == current and current not in t[:-1]
    assert len(set(t[:-1])) < len(t[:-1]) and all(k in t for k in first)          # a key-frame reached twice
    assert any(current in m.conn.ordered[k][:5] for k in first)                    # current as a second neighbour, left out
    if bad_first:
        assert m.conn.ordered[current][0] not in t and m.store[m.conn.ordered[current][0]]["bad"]


def test_current_erased(vo):
    script, current = fi.graph_case()
    d, m = _run(vo, script + [("erase", current), ("neighbors", current)], 14, 64, caps=(16, 512, 8192))
    assert m.fuse_result()["targets"] == []


def test_composed_call_adds_through_the_overlay(vo):
    """point `a` of the current key-frame is added to the targets that see it in an empty feature, once each: a later visit of
    the same key-frame finds it held, through the entries the call has added"""
    script, current, a = fi.composed_case()
    d, m = _run(vo, script + [("neighbors", current)], 7, 64)
    res = m.fuse_result()
    assert res["totals"][2] >= 3 and len(set(res["targets"])) < len(res["targets"]) and len(m.observations(a)) == 2 + res["totals"][2]


# ---- the three limits, each hit once: the step is left undone, the bit is raised ---------------------------------------------
def test_candidate_capacity(vo):
    """three candidates pass the gates where a step takes two (one of them would have matched)"""
    c = fi.capacity_candidates_case()
    d, m = _run(vo, c["script"] + [("fuse",) + c["fuse"]], 7, c["NK"], max_candidates=2)
    assert m.fuse_result()["per_target"] == [(3, 1, 0, 0, 0, 0)] and m.undone == [(fi.T_HAND, "candidates")]
    L, h = vo.lib(), d.s._h
    big = np.zeros(60 * c["NK"] + 1, np.int32)
    import ctypes as C
    assert L.vo_kfstore_fuse_map_points(h, 0, len(big), vo._p(big), C.c_float(3.0)) == -4      # a list the block cannot take


def test_match_capacity(vo):
    """the matches of a call (each reserves its node of the overlay) exceed max_candidates in its third matching step: two adds
    are made, that step and every later one are left undone"""
    script, current, a = fi.composed_case()
    d, m = _run(vo, script + [("neighbors", current)], 7, 64, max_candidates=2)
    res = m.fuse_result()
    assert res["totals"][2] == 2 and res["totals"][1] > 2 and all(x[0] <= 2 for x in res["per_target"])
    assert {kind for _, kind in m.undone} == {"matches"}


def test_carrier_capacity(vo):
    """a replace between points of which one has 1025 carriers: counted as a match, left undone"""
    c = fi.carriers_case()
    d = FDev(vo, c["K"], c["NK"], caps=(16, 256, 1024))
    mr = _model(vo, caps=(16, 256, 1024))
    for s in c["script"] + [("fuse",) + c["fuse"]]:
        d.step(s), mr.step(s)
    m = mr.m
    assert len(m.carriers(900)) == vo.KeyFrameStore.FUSE_MAX_CARRIERS + 1 and m.fuse_result()["per_target"] == [(1, 1, 0, 0, 0, 0)]
    assert m.sticky == vo.KeyFrameStore.CONNECTIONS_FUSE_CAPACITY
    _same(d, m, "carriers")


def test_seeded_chain(vo):
    """insert -> process -> stats -> cull -> create -> search_in_neighbors -> local BA -> cull key-frames on the seeded
    12 x 256 scene, compared after every fuse"""
    import local_ba_inputs as li
    d = FDev(vo, fi.K_SCENE, fi.N_FEAT, fi.SCENE_CAPS, True, fi.SCENE_RECENT, fi.SCENE_CANDIDATES)
    mr = _model(vo, fi.SCENE_CAPS, fi.SCENE_RECENT, fi.SCENE_CANDIDATES)
    m, ba, totals = mr.m, None, np.zeros(len(STEP), int)
    for i, s in enumerate(fi.seeded_chain()):
        where = (i, s[:2])
        if s[0] == "ba":
            d.s.local_ba_window(s[1])
            want, w = m.window(s[1]), d.s.local_ba_window_result()
            assert want is not None and w["record"]["status"] == 0 and w["point_id"].tobytes() == want["point_id"].tobytes(), where
            pr = dict({k: w[k] for k in ("poses", "fixed", "points", "e_cam", "e_pt", "e_obs", "e_inv_sigma")}, cam=np.array([float(c) for c in li.CAM6[:5]]))
            ba = vo.BundleAdjuster(pr) if ba is None else (ba.reset(pr), ba)[1]
            erase, _, rc = ba.local_ba()
            poses, pts = ba.state()
            _, rc2 = d.s.local_ba(ba, s[1])
            assert rc == 0 and rc2 == 0, where
            m.apply(poses, pts, erase)
            _same(d, m, where, result=False)
        elif s[0] == "cullkf":
            d.s.cull_keyframes(s[1], s[2]), m.cull(s[1], s[2])
            assert d.s.cull_result() == m.result, where
            _same(d, m, where, result=False)
        else:
            d.step(s), mr.step(s)
            if s[0] == "create":
                for k in range(len(m.store)):
                    got = d.state(k)
                    m.set_map_side(k, got["points"], got["normals"], got["min_dist"], got["max_dist"])
            elif s[0] == "neighbors":
                _same(d, m, where)
                totals += np.array(m.fuse_result()["totals"])
    ba.close()
    assert (totals > 0).all()                  # candidates, matches, adds, replaces in both directions, cleared features
    chains = Counter((call, e[2]) for call, e in zip(m.fuse_log_call, m.fuse_log))
    assert max(chains.values()) >= 2           # a chain of two matches inside one fuse call
    # the conditions on the inputs, on the state THIS run compared (created points at the device's positions, the solver's
    # result applied): every float gate decided with the margins of tests/test_fuse_ref.py
    assert not m.weak and min(x for _, x in m.margins) >= MARGIN and min(m.level_fracs) >= LEVEL_MARGIN, sorted(m.weak)


# ---- opt-in and misuse ------------------------------------------------------------------------------------------------------
def test_opt_in_and_misuse(vo):
    import ctypes as C
    L = vo.lib()
    zi, b = np.zeros(8, np.int32), np.array(fi.BOUNDS, np.float32)
    th = C.c_float(3.0)
    plain = UDev(vo, 4, 16, ui.CAPS)                                           # no enable_fuse
    for rc in (L.vo_kfstore_fuse_map_points(plain.s._h, 0, 1, vo._p(zi), th), L.vo_kfstore_fuse_map_points_dev(plain.s._h, 0, 1, vo._p(zi), th),
               L.vo_kfstore_search_in_neighbors(plain.s._h, 0), L.vo_kfstore_fuse_result(plain.s._h, None, None, None)):
        assert rc == -1
    no_up = UDev(vo, 4, 16, ui.CAPS, max_recent=None)
    assert L.vo_kfstore_enable_fuse(no_up.s._h, vo._p(b), 8) == -1             # no enable_point_upkeep
    bad = np.array([0, 0, 0, 480], np.float32)
    assert L.vo_kfstore_enable_fuse(plain.s._h, vo._p(bad), 8) == -1 and L.vo_kfstore_enable_fuse(plain.s._h, vo._p(b), 0) == -1
    assert L.vo_kfstore_enable_fuse(plain.s._h, None, 8) == -1
    assert L.vo_kfstore_enable_fuse(plain.s._h, vo._p(b), 8) == 0 and L.vo_kfstore_enable_fuse(plain.s._h, vo._p(b), 8) == 0
    assert plain.s.fuse_result() == dict(targets=[], per_target=[], totals=(0,) * 6)
    c = fi.hand_case("add")
    d, m = _run(vo, c["script"], 7, c["NK"])
    h = d.s._h
    for rc in (L.vo_kfstore_fuse_map_points(h, 7, 1, vo._p(zi), th), L.vo_kfstore_fuse_map_points(h, -1, 1, vo._p(zi), th),
               L.vo_kfstore_fuse_map_points(h, 0, -1, vo._p(zi), th), L.vo_kfstore_fuse_map_points(h, 0, 1, None, th),
               L.vo_kfstore_fuse_map_points(h, 0, 1, vo._p(zi), C.c_float(0.0)), L.vo_kfstore_fuse_map_points_dev(h, 0, 1, None, th),
               L.vo_kfstore_search_in_neighbors(h, 7), L.vo_kfstore_search_in_neighbors(h, -1), L.vo_kfstore_enable_fuse(h, vo._p(b), 8)):
        assert rc == -1
    assert L.vo_kfstore_fuse_map_points(h, 0, 0, None, th) == 0
    _same(d, m, "after the refused calls", result=False)
