"""CPU tests of the loop-fusion model tests/loop_fuse_ref.py: against a pointer-object transcription of
Matcher::fuseByPose (src/matcher.cpp:1135-1238), LoopClosing::searchAndFuse (src/loopClosing.cpp:496-516) and
MapPoint::replaceMapPoint (src/mappoint.cpp:214-253) that keeps observedKFs_, mappoints_, badFlag_ and the counters
incrementally (tests/test_fuse_ref.py's objects); the gates decided a second time by a direct numpy transcription of
matcher.cpp:1164-1191; hand tables; and the conditions on the inputs the device comparison (tests/test_gpu_loop_fuse.py)
relies on."""
import copy

import numpy as np
import pytest

import fuse_inputs as fi
import loop_fuse_inputs as lfi
from fuse_ref import LEVEL_MARGIN, MARGIN, STICKY_FUSE, STICKY_INVALID
from loop_fuse_ref import pose_from_sim3
from test_fuse_ref import Pointers, _same_as_pointers

f32 = np.float32


def gates_transcribed(m, S, a):
    """matcher.cpp:1144-1145 and :1164-1191 with keyframe.cpp:64-67 and mappoint.cpp:198-212, 391-401, written out with numpy's
    own matrix product, norm and a rotation matrix of its own (not the model's operation order; the margins of the scenes cover
    the difference) -> (u, v, level) or None"""
    q = np.array(S[:4], np.float64)
    x, y, z, w = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    t = np.array(S[4:7], np.float64)                  # Scw.translation(): not divided by the scale
    Ow = -R.T @ t
    fx, fy, cx, cy = (f32(c) for c in m.cam[:4])
    p_world = np.array(a["point"], np.float64)
    p_cam = R @ p_world + t
    zc = f32(p_cam[2])
    if zc < 0:
        return None
    with np.errstate(all="ignore"):
        invz = f32(1.0) / zc
        u, v = fx * (f32(p_cam[0]) * invz) + cx, fy * (f32(p_cam[1]) * invz) + cy
    xMin, xMax, yMin, yMax = m.bounds
    if not (u >= xMin and v >= yMin and u < xMax and v < yMax):
        return None
    pline = p_world - Ow
    distance = f32(np.linalg.norm(pline))
    if distance < f32(0.8) * a["mind"] or distance > f32(1.2) * a["maxd"]:
        return None
    if float(pline @ np.array(a["normal"], np.float64)) < 0.5 * float(distance):
        return None
    scale = int(np.ceil(f32(np.log(a["maxd"] / distance)) / f32(np.log(m.sf[1]))))
    return u, v, min(max(scale, 0), len(m.sf) - 1)


class LoopPointers(Pointers):
    """test_fuse_ref.Pointers with fuseByPose and searchAndFuse"""

    def fuseByPose(self, kf, S, loopMapPoints, replaceMapPoints, th):     # matcher.cpp:1135-1238
        calc = self.calc
        stored, calc.store[kf.id_]["pose"] = calc.store[kf.id_]["pose"], pose_from_sim3(S)
        alreadyFound = {mp for mp in kf.mappoints_ if mp is not None and not mp.isBad()}
        fused = 0
        for i, mp in enumerate(loopMapPoints):
            if mp is None or mp.isBad() or mp in alreadyFound:
                continue
            q = calc.project(kf.id_, mp.id_, th, attrs=mp.a)
            g = gates_transcribed(calc, S, mp.a)                          # the gates, decided independently of the model
            assert (q is None) == (g is None), (kf.id_, mp.id_)
            if q is None:
                continue
            assert (q["level"], abs(float(q["u"] - g[0])) < 1e-3, abs(float(q["v"] - g[1])) < 1e-3) == (g[2], True, True)
            self.n_gates += 1
            bestIdx = calc.search_by_pose(kf.id_, q)
            if bestIdx < 0:
                continue
            mpKF = kf.mappoints_[bestIdx]
            if mpKF is not None:
                if not mpKF.isBad():
                    replaceMapPoints[i] = mpKF
            else:
                mp.addObservation(kf, bestIdx)
                kf.mappoints_[bestIdx] = mp
            fused += 1
        calc.store[kf.id_]["pose"] = stored
        return fused

    def searchAndFuse(self, correctPose, loopConnectKFMapPoints_, th=4):  # loopClosing.cpp:496-516
        fused = []
        for kid in sorted(correctPose):
            kf, Scw = self.kfs[kid], correctPose[kid]
            replaceMapPoints = [None] * len(loopConnectKFMapPoints_)
            fused.append(self.fuseByPose(kf, Scw, loopConnectKFMapPoints_, replaceMapPoints, th))
            for i, mp in enumerate(replaceMapPoints):
                if mp is not None:
                    mp.replaceMapPoint(loopConnectKFMapPoints_[i])
        return fused


def _run(c, **kw):
    m = lfi.run_model(c["script"], **{k: c[k] for k in ("max_candidates", "caps") if k in c}, **kw)
    return m


def _fuse(m, c, th=None):
    m.search_and_fuse(c["corr_kf"], c["S_corr"], c["ids"], c["th"] if th is None else th)
    return m.loop_fuse_result()


SINGLE = [n for n in lfi.HAND_CASES if n not in ("same_org_two_features", "not_a_multiple_of_64", "targets_erased_or_without_a_pose")]


@pytest.mark.parametrize("name", lfi.HAND_CASES)
def test_hand_tables(name):
    c = lfi.hand_case(name)
    m = _run(c)
    assert _fuse(m, c)["per_pass"] == c["per_pass"]


@pytest.mark.parametrize("name", SINGLE)
def test_search_and_fuse_equals_the_pointer_model(name):
    """(the cases left out hold an id in two features of a key-frame, or a key-frame the pointer model has no state for)"""
    c = lfi.hand_case(name)
    m = _run(c)
    p = LoopPointers(m)
    res = _fuse(m, c)
    fused = p.searchAndFuse(dict(zip(c["corr_kf"], c["S_corr"])), [p.points.get(i) for i in c["ids"]], c["th"])
    assert fused == [row[1] for row in res["per_pass"]]
    _same_as_pointers(m, p, name)


def test_counters_are_added_twice_when_both_are_listed():
    c = lfi.counters_case()
    m = _run(c)
    p = LoopPointers(m)
    _fuse(m, c)
    p.searchAndFuse(dict(zip(c["corr_kf"], c["S_corr"])), [p.points.get(i) for i in c["ids"]], c["th"])
    got = {e[0]: e[2:] for e in m.recent_points()}
    base = {e[0]: e[2:] for e in _run(c).recent_points()}
    assert got[900] == base[900]                                         # the one that goes keeps its entry and its counters
    for b in (700, 701):
        assert got[b] == (base[b][0] + base[900][0], base[b][1] + base[900][1]) == (p.points[b].found_cnt_, p.points[b].visible_cnt_)
    assert [x[3] for x in m.lf_moved] == [2, 0]                          # the second replace moved nothing


def test_what_each_hand_case_is_about():
    m = {}
    for name in lfi.HAND_CASES:
        c = lfi.hand_case(name)
        m[name] = _run(c)
        _fuse(m[name], c)
    assert [e[4] for e in m["two_on_one_empty_feature"].lf_log] == ["add", "replace"] and m["two_on_one_empty_feature"].lf_log[1][5] == 700
    assert m["replace_three_holders"].lf_moved == [(0, 900, m["replace_three_holders"].lf_log[0][2], 2)]
    assert [x[3] for x in m["same_org_two_features"].lf_moved] == [1, 0] and [x[3] for x in m["same_org_one_feature"].lf_moved] == [2, 0]
    assert (1, 0, 700, "bad") in m["dies_in_pass_1"].lf_gates and (1, 1, 701, "passed") in m["dies_in_pass_1"].lf_gates
    assert [g[3] for g in m["already_held"].lf_gates] == ["held", "negative", "passed"]
    assert m["targets_erased_or_without_a_pose"].erased[4] and m["targets_erased_or_without_a_pose"].store[5]["pose"] is None
    # the window rules: the feature inside the radius is not in the list / the second feature of the target wins the add
    assert not m["round_not_floor"].lf_log and m["not_a_multiple_of_64"].lf_log[0][3] == 66


def test_the_unscaled_translation_decides_which_feature_wins():
    """quirk 1: with t / s the projection lands on the other feature"""
    c = lfi.hand_case("scale_quirk")
    a, b = _run(c), _run(c)
    b.divide_t = True
    _fuse(a, c), _fuse(b, c)
    fa, fb = [e[3] for e in a.lf_log], [e[3] for e in b.lf_log]
    assert len(fa) == len(fb) == 1 and fa != fb
    T = c["corr_kf"][0]
    assert abs(float(a.store[T]["xy"][fb[0], 0] - a.store[T]["xy"][fa[0], 0])) > 2 * 4.8


def test_threshold_4_against_3():
    c = lfi.hand_case("threshold")
    a, b = _run(c), _run(c)
    assert _fuse(a, c, 4.0)["per_pass"] == [(1, 1, 1, 0, 0, 0)] and _fuse(b, c, 3.0)["per_pass"] == [(1, 0, 0, 0, 0, 0)]


def test_z_just_above_zero_is_not_skipped():
    c = lfi.z_case()
    m = _run(c)
    n0 = len(m.margins)
    assert _fuse(m, c)["per_pass"] == c["per_pass"]
    assert [g[3] for g in m.lf_gates] == ["gates", "gates"]
    # pass 1 went on to isInImg and the distance gate (both passes are decided twice: derivation 1's dry run); pass 2 stopped at z
    assert [g for g, _ in m.margins[n0:]] == ["img"] * 4 + ["dist"] * 2 + ["img"] * 4 + ["dist"] * 2
    for S, want in zip(c["S_corr"], (True, False)):
        T = pose_from_sim3(S)
        P = m.attributes(c["ids"][0])["point"]
        z = f32(T[6] * P[0] + T[7] * P[1] + T[8] * P[2] + T[11])
        assert (z >= 0) == want and abs(float(z)) >= 5e-5


def test_the_three_capacity_limits():
    c = lfi.capacity_candidates_case()
    m = _run(c)
    assert _fuse(m, c)["per_pass"] == [(3, 1, 0, 0, 0, 0)] and m.undone == [(c["corr_kf"][0], "candidates")] and m.sticky & STICKY_FUSE
    c = lfi.capacity_matches_case()
    m = _run(c)
    assert _fuse(m, c)["per_pass"] == [(1, 1, 1, 0, 0, 0), (1, 1, 1, 0, 0, 0), (1, 1, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0)]
    assert m.undone == [(3, "matches"), (4, "matches")] and m.sticky & STICKY_FUSE
    c = lfi.capacity_carriers_case()
    m = _run(c)
    assert _fuse(m, c)["per_pass"] == [(1, 1, 0, 1, 0, 0)] and [e[4] for e in m.lf_log] == ["capacity"] and m.sticky & STICKY_FUSE
    assert len(m.carriers(900)) == 1025


def test_targets_erased_or_without_a_pose_raise_the_sticky_word():
    c = lfi.hand_case("targets_erased_or_without_a_pose")
    m = _run(c)
    m.sticky = 0
    _fuse(m, c)
    assert m.sticky == STICKY_INVALID
    m.sticky = 0
    m.search_and_fuse(c["corr_kf"], c["S_corr"], c["ids"], c["th"], state=2)     # a compute_sim3 that ended REJECTED
    assert m.sticky == STICKY_INVALID and m.loop_fuse_result() == dict(passes=0, per_pass=[], totals=(0,) * 6)


# ---- the seeded scene -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded():
    """the seeded chain of tests/fuse_inputs.py on the model up to (and with) its first search_in_neighbors, then the loop step
    with the pointer model run beside it"""
    r = lfi.ModelRunner(fi.SCENE_CAPS, max_recent=fi.SCENE_RECENT, max_candidates=fi.SCENE_CANDIDATES, model=lfi.ChainModel)
    for s in fi.seeded_chain():
        r.step(s)
        if s[0] == "neighbors":
            break
    m = r.m
    corr, S, ids = lfi.chain_inputs(m)
    p = LoopPointers(m)
    n0 = len(m.margins)
    m.search_and_fuse(corr, S, ids, lfi.TH)
    fused = p.searchAndFuse(dict(zip(corr, S)), [p.points.get(i) for i in ids], lfi.TH)
    return m, p, fused, n0


def test_search_and_fuse_equals_the_pointer_model_on_the_seeded_scene(seeded):
    m, p, fused, _ = seeded
    res = m.loop_fuse_result()
    assert fused == [row[1] for row in res["per_pass"]] and res["passes"] == len(lfi.CHAIN_CORRECTED)
    _same_as_pointers(m, p, "seeded")
    assert res["totals"][0] > 20 and res["totals"][2] >= 2 and p.n_gates == res["totals"][0]


def _scenes():
    for name in lfi.HAND_CASES:
        c = lfi.hand_case(name)
        m = _run(c)
        _fuse(m, c)
        if name == "threshold":
            _fuse(m, c, 3.0)
        yield name, m
    for name, c in (("counters", lfi.counters_case()), ("candidates", lfi.capacity_candidates_case()),
                    ("matches", lfi.capacity_matches_case()), ("carriers", lfi.capacity_carriers_case())):
        m = _run(c)
        _fuse(m, c)
        yield name, m


def test_every_float_gate_decides_with_a_margin(seeded):
    """the conditions on the inputs the device comparison relies on, in every scene: relative margin >= 1e-4 at the image bounds,
    the distance range, the normal and the radius tests; log(ratio) / log(sf[1]) at least 1e-3 from an integer.  (z_case is
    about the sign of z alone: its first pass stands 1e-4 in front of the point, asserted above.)"""
    for name, m in _scenes():
        assert m.margins and min(x for _, x in m.margins) >= MARGIN, name
        assert not m.level_fracs or min(m.level_fracs) >= LEVEL_MARGIN, name
        assert not m.weak, name
    m, _, _, n0 = seeded
    assert not m.weak and min(x for _, x in m.margins[n0:]) >= MARGIN and min(m.level_fracs) >= LEVEL_MARGIN, sorted(m.weak)


def test_the_chain_goes_on_to_the_pose_graph_window(seeded):
    """update_connections and pose_graph_window behind the loop step, on the model (the device's chain: tests/test_gpu_loop_fuse.py)"""
    import pose_graph_store_ref as pr
    m = copy.deepcopy(seeded[0])
    corr, S, _ = lfi.chain_inputs(seeded[0])
    m.update_connections(corr)
    inp = pr.make_inputs({k: (s, pr.from_pose(m.store[k]["pose"])) for k, s in zip(corr, S)}, {}, {})
    assert m.pg_window(len(m.store) - 1, corr[0], inp) is not None and m.pg_record["n_edges"] > 0
