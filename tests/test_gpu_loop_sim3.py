"""vo_kfstore_compute_sim3 (LoopClosing::computeSim3 on the device) against the model
tests/loop_sim3_ref.py, through the binding.  Exact: the state, the matched key-frame, rounds, verifications, rand_used, every
per-candidate row, the inlier counts, match_ids, loop_point_ids and the sticky word.  Scm and Scw within 1e-8 as (R, t) distance
and scale -- the bound tests/test_gpu_loop_rotated.py holds for the same refinement against the oracle; it applies unchanged,
because equal discrete results mean equal solver inputs.  The gathered camera-frame points byte for byte (the operation order
is fixed, as in new_points_geom.h) and so within the 1e-12 the contract states.  The store's other state byte for byte against a
snapshot.  tests/test_loop_sim3_ref.py holds the conditions on the inputs (every float gate decides with a margin)."""
import numpy as np
import pytest

import loop_sim3_inputs as li
import oracle_lib as orc
from loop_sim3_ref import ACCEPTED, NO_MATCH, REJECTED, STICKY_CAPACITY, STICKY_RAND_SHORT, UNDECIDED

pytestmark = pytest.mark.gpu

SIM_TOL = 1e-8
DISCRETE = ("state", "match_pos", "match_kf", "rounds", "verifications", "rand_used", "refine_inliers", "match_cnt", "n_loop_points")


def _snapshot(s, sc):
    out = []
    for k, kf in enumerate(sc["store"]):
        n = len(kf["ids"])
        p = s.points(k, n)
        T, on = s.pose(k)
        out.append([np.asarray(p[key]).tobytes() for key in ("flags", "ids", "points", "normals", "min_dist", "max_dist", "point_desc")] +
                   [np.asarray(T).tobytes(), on, s.flags(k, n)[1], s.point_refs(k, n).tobytes(), repr(s.connections(k)), repr(s.cull_state(k))])
    return out, s.recent_points()


def _sim_distance(a, b):
    return max(float(np.abs(a[:12] - b[:12]).max()), abs(float(a[12] - b[12])))


def _compare(s, m, sc, where=""):
    n_cur = len(sc["store"][sc["current"]]["ids"])
    got, want = s.loop_result(n_cur), m.result()
    assert {k: got[k] for k in DISCRETE} == {k: want[k] for k in DISCRETE}, (where, got, want)
    nc = len(sc["cand"])
    assert got["per_candidate"][:nc] == want["per_candidate"][:nc], (where, got["per_candidate"][:nc], want["per_candidate"][:nc])
    assert np.array_equal(got["match_ids"], want["match_ids"]), (where, np.nonzero(got["match_ids"] != want["match_ids"])[0])
    assert np.array_equal(got["loop_point_ids"], want["loop_point_ids"]), where
    assert _sim_distance(got["Scm"], want["Scm"]) <= SIM_TOL and _sim_distance(got["Scw"], want["Scw"]) <= SIM_TOL, \
        (where, _sim_distance(got["Scm"], want["Scm"]), _sim_distance(got["Scw"], want["Scw"]))
    for i in range(nc):
        if want["per_candidate"][i]["n"] > 0:
            d, sol = s.loop_solver_inputs(i), m.solvers[i]
            assert d["pc1"].tobytes() == sol["pc1"].tobytes() and d["pc2"].tobytes() == sol["pc2"].tobytes(), (where, i)
            assert np.abs(d["pc1"] - sol["pc1"]).max() <= 1e-12 and np.abs(d["pc2"] - sol["pc2"]).max() <= 1e-12
            assert np.abs(d["px1"] - sol["px1"]).max() <= 1e-9 and np.abs(d["px2"] - sol["px2"]).max() <= 1e-9
            assert np.array_equal(d["me1"], sol["me1"]) and np.array_equal(d["me2"], sol["me2"]) and np.array_equal(d["index"], sol["index"])
    assert s.connections_status() == m.sticky, where
    m.sticky = 0
    return got


def _run(vo, name, dev=False, rand=None, max_rounds=None, **caps):
    import torch
    sc = li.scene(name)
    s = li.build_device(vo, sc, **caps)
    before = _snapshot(s, sc)
    m = li.run_model(orc, sc, rand=rand, max_rounds=max_rounds, **caps)
    r = sc["rand"] if rand is None else rand
    rounds = sc["max_rounds"] if max_rounds is None else max_rounds
    if dev:
        keep = (torch.tensor(sc["cand"], dtype=torch.int32).cuda(), torch.from_numpy(np.ascontiguousarray(r, np.int32)).cuda())
        s.compute_sim3(sc["current"], keep[0], keep[1], li.RAND_MAX, sc["fix_scale"], rounds)
    else:
        s.compute_sim3(sc["current"], sc["cand"], r, li.RAND_MAX, sc["fix_scale"], rounds)
    got = _compare(s, m, sc, name)
    assert _snapshot(s, sc) == before, "the call changed the store"
    return s, m, sc, got


# (a) .. (h), (m): every scenario of tests/loop_sim3_inputs.py; (l): the device form on two of them
@pytest.mark.parametrize("name", li.SCENARIOS)
def test_scenario_equals_the_model(vo, name):
    s, m, sc, got = _run(vo, name)
    want = dict(accepted=ACCEPTED, three_candidates=ACCEPTED, filtered_below_20=NO_MATCH, outliers_only=ACCEPTED, fails_then_wins=ACCEPTED,
                rejected=REJECTED, free_scale=ACCEPTED).get(name, ACCEPTED)
    assert got["state"] == want


@pytest.mark.parametrize("name", ["accepted", "fails_then_wins"])
def test_the_device_form_agrees_with_the_host_form(vo, name):
    _, _, _, host = _run(vo, name)
    _, _, _, dev = _run(vo, name, dev=True)
    for k in DISCRETE:
        assert host[k] == dev[k]
    assert host["Scw"].tobytes() == dev["Scw"].tobytes() and np.array_equal(host["match_ids"], dev["match_ids"])


# (i) rounds split across calls
def test_one_round_per_call_equals_one_call(vo):
    s1, m, sc, whole = _run(vo, "fails_then_wins")
    s = li.build_device(vo, sc)
    s.compute_sim3(sc["current"], sc["cand"], sc["rand"], li.RAND_MAX, sc["fix_scale"], 1)
    first = s.loop_result(len(sc["store"][sc["current"]]["ids"]))
    assert first["state"] == UNDECIDED and first["rounds"] == 1 and first["verifications"] == 1 and s.connections_status() == 0
    for _ in range(3):
        s.compute_sim3_continue(1)
    m2 = li.run_model(orc, sc)
    got = _compare(s, m2, sc, "split")
    assert got["Scw"].tobytes() == whole["Scw"].tobytes() and got["rounds"] == whole["rounds"] == 2
    # and the model split the same way
    m3 = li.run_model(orc, sc, max_rounds=1)
    assert m3.result()["state"] == UNDECIDED and m3.sticky == 0
    m3.continue_(1)
    assert m3.result()["state"] == ACCEPTED


def test_too_few_rounds_is_undecided_without_a_sticky_bit(vo):
    s, m, sc, got = _run(vo, "fails_then_wins", max_rounds=1)
    assert got["state"] == UNDECIDED and got["verifications"] == 1
    s2, m2, sc2, got2 = _run(vo, "accepted", max_rounds=0)
    assert got2["state"] == UNDECIDED and got2["rounds"] == 0


# (j) rand_values one short of the need
def test_rand_values_one_short(vo):
    sc = li.scene("outliers_only")
    need = li.run_model(orc, sc).result()["rand_used"]
    s, m, sc, got = _run(vo, "outliers_only", rand=sc["rand"][:need - 1])
    assert got["state"] == UNDECIDED and m.log[-1] == ("rand_short",)
    s.compute_sim3_continue(2)                     # undecided for good
    assert s.loop_result()["state"] == UNDECIDED
    s2, m2, _, got2 = _run(vo, "outliers_only", rand=sc["rand"][:need])
    assert got2["state"] == ACCEPTED and got2["rand_used"] == need


# (k) max_loop_points one short
def test_loop_points_one_short(vo):
    n = li.run_model(orc, li.scene("accepted")).result()["n_loop_points"]
    s, m, sc, got = _run(vo, "accepted", max_loop_points=n - 1)
    assert got["state"] == UNDECIDED and got["n_loop_points"] == n and ("capacity",) in m.log
    s2, m2, _, got2 = _run(vo, "accepted", max_loop_points=n)
    assert got2["state"] == ACCEPTED


@pytest.mark.parametrize("how", ["erased", "no_pose"])
def test_current_erased_or_without_a_pose(vo, how):
    sc = li.scene("accepted")
    if how == "no_pose":
        sc["store"][sc["current"]]["pose"] = None
    s = li.build_device(vo, sc)
    if how == "erased":
        s.erase_keyframe(sc["current"])
    s.compute_sim3(sc["current"], sc["cand"], sc["rand"], li.RAND_MAX, True, 4)
    got = s.loop_result(0)
    assert got["state"] == UNDECIDED and got["rounds"] == 0 and got["rand_used"] == 0 and got["per_candidate"][0]["kf"] == sc["cand"][0]
    assert s.connections_status() == 1
    if how == "no_pose":
        m = li.run_model(orc, sc)
        assert m.sticky == 1 and m.result()["state"] == UNDECIDED and m.log == [("invalid",)]


# (n) misuse
def test_a_store_without_the_block_refuses(vo):
    import ctypes as C
    sc = li.scene("accepted")
    s = li.build_device(vo, sc, loop=False)
    before = _snapshot(s, sc)
    L, h = vo.lib(), s._h
    cand, rnd = np.array(sc["cand"], np.int32), np.ascontiguousarray(sc["rand"], np.int32)
    rec = np.zeros(16, np.int32)
    n = C.c_int32(0)
    for rc in (L.vo_kfstore_compute_sim3(h, sc["current"], 1, vo._p(cand), 1, len(rnd), vo._p(rnd), li.RAND_MAX, 4),
               L.vo_kfstore_compute_sim3_dev(h, sc["current"], 1, vo._p(cand), 1, len(rnd), vo._p(rnd), li.RAND_MAX, 4),
               L.vo_kfstore_compute_sim3_continue(h, 1), L.vo_kfstore_loop_result(h, vo._p(rec), None, None, None, None, None, None),
               L.vo_kfstore_loop_solver_inputs(h, 0, C.byref(n), None, None, None, None, None, None, None),
               L.vo_kfstore_enable_loop(h, 4, 64, 64)):                         # (the last: not empty)
        assert rc == -1
    assert _snapshot(s, sc) == before and s.connections_status() == 0
    e = vo.KeyFrameStore(4, 64)
    assert L.vo_kfstore_enable_loop(e._h, 4, 64, 64) == -1                      # no enable_fuse
    s3 = li.build_device(vo, sc)
    h3 = s3._h
    assert L.vo_kfstore_compute_sim3(h3, len(sc["store"]), 1, vo._p(cand), 1, len(rnd), vo._p(rnd), li.RAND_MAX, 4) == -1
    bad = np.array([99], np.int32)
    assert L.vo_kfstore_compute_sim3(h3, sc["current"], 1, vo._p(bad), 1, len(rnd), vo._p(rnd), li.RAND_MAX, 4) == -1
    many = np.zeros(5, np.int32)
    assert L.vo_kfstore_compute_sim3(h3, sc["current"], 5, vo._p(many), 1, len(rnd), vo._p(rnd), li.RAND_MAX, 4) != 0
    assert L.vo_kfstore_compute_sim3_continue(h3, 1) == -1                     # nothing enqueued yet
