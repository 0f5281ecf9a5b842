"""CPU tests of the fusion model tests/fuse_ref.py: against a pointer-object transcription of
LocalMapping::searchInNeighbors (src/localMapping.cpp:363-432), Matcher::fuseMapPoints (src/matcher.cpp:1012-1133) and
MapPoint::replaceMapPoint (src/mappoint.cpp:214-253) that keeps observedKFs_, observe_cnt_, mappoints_ and the counters
incrementally; against the oracle's fuse matching for the search step; hand tables where the restatement's choices differ; and
the conditions on the inputs the device comparison (tests/test_gpu_fuse.py) relies on."""
import copy
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import fuse_inputs as fi
from fuse_ref import LEVEL_MARGIN, MARGIN, TH_LOW
from test_point_upkeep_ref import literal_choice

f32 = np.float32


# ---- the pointer model --------------------------------------------------------------------------------------------------------
class MapPoint:
    def __init__(self, pid, attrs, found, visible):
        self.id_, self.a, self.observedKFs_, self.observe_cnt_, self.badFlag_ = pid, attrs, {}, 0, False
        self.found_cnt_, self.visible_cnt_, self.fuseForKF_, self.replaced = found, visible, 0, None

    def isBad(self):
        return self.badFlag_

    def beObserved(self, kf):
        return kf in self.observedKFs_

    def addObservation(self, kf, idx):                    # mappoint.cpp:52-64
        if kf in self.observedKFs_:
            return
        self.observedKFs_[kf] = idx
        self.observe_cnt_ += 2 if kf.uRight_[idx] >= 0 else 1

    def computeDescriptor(self):                          # mappoint.cpp:118-179
        if self.badFlag_ or not self.observedKFs_:
            return
        desp = [kf.desc[idx] for kf, idx in sorted(self.observedKFs_.items(), key=lambda t: t[0].id_) if not kf.bad]
        if desp:
            self.a = dict(self.a, pdesc=desp[literal_choice(desp)].copy())

    def replaceMapPoint(self, mp):                        # mappoint.cpp:214-253
        if mp.id_ == self.id_:
            return
        obs, self.observedKFs_, self.badFlag_ = self.observedKFs_, {}, True
        visible, found, self.replaced = self.visible_cnt_, self.found_cnt_, mp
        for kf, idx in obs.items():
            if not mp.beObserved(kf):
                kf.mappoints_[idx] = mp
                mp.addObservation(kf, idx)
            else:
                kf.mappoints_[idx] = None
        mp.found_cnt_ += found
        mp.visible_cnt_ += visible
        mp.computeDescriptor()


class KeyFrame:
    def __init__(self, kid, kf, ordered):
        self.id_, self.uRight_, self.desc, self.bad = kid, kf["u_right"], kf["desc"], kf["bad"]
        self.mappoints_, self.ordered, self.fuseKFId_ = [None] * len(kf["ids"]), ordered, 0


def gates_transcribed(m, T, a, threshold):
    """matcher.cpp:1032-1063 with keyframe.cpp:64-67 and mappoint.cpp:198-212, 391-401 written out with numpy's own matrix
    product and norm (not the model's operation order; the margins of the scenes cover the difference) -> (u, v, ur, level) or
    None"""
    pose = np.array(m.store[T]["pose"], np.float64)
    R, t = pose[:9].reshape(3, 3), pose[9:]
    fx, fy, cx, cy, bf = (f32(c) for c in m.cam[:5])
    p_world = np.array(a["point"], np.float64)
    pcam = R @ p_world + t
    z = f32(pcam[2])
    if z < f32(0.0):
        return None
    invz = f32(1.0) / z
    x, y = f32(pcam[0]) * invz, f32(pcam[1]) * invz
    u, v = fx * x + cx, fy * y + cy
    xMin, xMax, yMin, yMax = m.bounds
    if not (u >= xMin and v >= yMin and u < xMax and v < yMax):
        return None
    ur = u - bf * invz
    Ow = -R.T @ t
    line = p_world - Ow
    dist = f32(np.linalg.norm(line))
    if dist < f32(0.8) * a["mind"] or dist > f32(1.2) * a["maxd"]:
        return None
    if float(line @ np.array(a["normal"], np.float64)) < 0.5 * float(dist):
        return None
    ratio = a["maxd"] / dist
    scale = int(np.ceil(f32(np.log(ratio)) / f32(np.log(m.sf[1]))))
    return u, v, ur, min(max(scale, 0), len(m.sf) - 1)


class Pointers:
    """the map of a model as objects (the model's state must have no id in two features of a key-frame).  The gates of a
    candidate are decided by gates_transcribed and must agree with the model's; the window search, which reads no mutable state
    but the candidate's own descriptor, is the model's, held against the oracle below"""

    def __init__(self, m):
        self.calc, self.n_gates = copy.deepcopy(m), 0
        self.kfs = [KeyFrame(k, kf, None) for k, kf in enumerate(m.store)]
        for k, kf in enumerate(self.kfs):
            kf.ordered = [self.kfs[j] for j in m.conn.ordered[k]]
        self.points = {}
        for k, kf in enumerate(m.store):
            if m.erased[k]:
                continue
            for i, (p, fl) in enumerate(zip(kf["ids"], kf["flags"])):
                if (fl & 1) and p >= 0:
                    if p not in self.points:
                        first, found, visible = m.recent.get(p, [0, 1, 1])
                        self.points[p] = MapPoint(p, m.attributes(p), found, visible)
                    assert not self.points[p].beObserved(self.kfs[k]), "an id in two features of a key-frame"
                    self.points[p].addObservation(self.kfs[k], i)
                    self.kfs[k].mappoints_[i] = self.points[p]

    def fuseMapPoints(self, kf, mappoints, threshold):    # matcher.cpp:1012-1133
        cnt = 0
        for mp in mappoints:
            if mp is None or mp.isBad() or mp.beObserved(kf):
                continue
            q = self.calc.project(kf.id_, mp.id_, threshold, attrs=mp.a)
            g = gates_transcribed(self.calc, kf.id_, mp.a, threshold)        # the gates, decided independently of the model
            assert (q is None) == (g is None)
            if q is None:
                continue
            assert (q["level"], abs(float(q["u"] - g[0])) < 1e-3, abs(float(q["v"] - g[1])) < 1e-3, abs(float(q["ur"] - g[2])) < 1e-3) == (g[3], True, True, True)
            self.n_gates += 1
            bestIdx = self.calc.search(kf.id_, q)
            if bestIdx < 0:
                continue
            mpOrg = kf.mappoints_[bestIdx]
            if mpOrg is not None:
                if not mpOrg.isBad():
                    if mpOrg.observe_cnt_ > mp.observe_cnt_:
                        mp.replaceMapPoint(mpOrg)
                    else:
                        mpOrg.replaceMapPoint(mp)
            else:
                mp.addObservation(kf, bestIdx)
                kf.mappoints_[bestIdx] = mp
            cnt += 1
        return cnt

    def searchInNeighbors(self, cur):                     # localMapping.cpp:363-432
        expand = []
        for kfn in cur.ordered[:10]:
            if kfn.bad or kfn.fuseKFId_ == cur.id_:
                continue
            expand.append(kfn)
            kfn.fuseKFId_ = cur.id_
            for kfs in kfn.ordered[:5]:
                if kfs.bad or kfs.fuseKFId_ == cur.id_ or kfs.id_ == cur.id_:
                    continue
                expand.append(kfs)
        mappoints_curr = list(cur.mappoints_)
        for kf in expand:
            self.fuseMapPoints(kf, mappoints_curr, 3.0)
        cand = []
        for kfg in expand:
            for mp in kfg.mappoints_:
                if mp is None or mp.isBad() or mp.fuseForKF_ == cur.id_:
                    continue
                mp.fuseForKF_ = cur.id_
                cand.append(mp)
        self.fuseMapPoints(cur, cand, 3.0)
        for mp in cur.mappoints_:
            if mp is not None and not mp.isBad():
                mp.computeDescriptor()
        return [kf.id_ for kf in expand]


def _same_as_pointers(m, p, where):
    for k, kf in enumerate(p.kfs):
        if m.erased[k]:
            continue
        live = [int(mp is not None and not mp.isBad()) for mp in kf.mappoints_]
        assert [f & 1 for f in m.store[k]["flags"]] == live, (where, k)
        for i, mp in enumerate(kf.mappoints_):
            if live[i]:
                assert m.store[k]["ids"][i] == mp.id_, (where, k, i)
                assert m.store[k]["pdesc"][i].tobytes() == mp.a["pdesc"].tobytes(), (where, k, i)
                assert m.obs(mp.id_) == mp.observe_cnt_ and dict(m.observations(mp.id_)) == {kf2.id_: ix for kf2, ix in mp.observedKFs_.items()}
    for pid, e in m.recent.items():
        if pid in p.points and not p.points[pid].isBad():
            assert (e[1], e[2]) == (p.points[pid].found_cnt_, p.points[pid].visible_cnt_), (where, pid)


SINGLE = [n for n in fi.HAND_CASES if n not in ("two_features_one_org", "not_a_multiple_of_64")]     # (those hold an id twice)


@pytest.mark.parametrize("name", SINGLE)
def test_fuse_equals_the_pointer_model(name):
    c = fi.hand_case(name)
    m = fi.run_model(c["script"])
    p = Pointers(m)
    T, ids = c["fuse"]
    m.fuse_map_points(T, ids)
    cnt = p.fuseMapPoints(p.kfs[T], [p.points.get(i) for i in ids], 3.0)
    assert cnt == m.fuse_result()["totals"][1] == len(c["kinds"])
    assert [(k, o) for _, _, _, k, o in m.fuse_log] == c["kinds"]
    _same_as_pointers(m, p, name)


@pytest.mark.parametrize("both", [True, False])
def test_counters_against_the_pointer_model(both):
    """both listed: the pointer model's sums; one listed: the store has no counters for the other, nothing is added"""
    c = fi.counters_case(both)
    m = fi.run_model(c["script"])
    p = Pointers(m)
    m.fuse_map_points(*c["fuse"])
    p.fuseMapPoints(p.kfs[c["fuse"][0]], [p.points.get(i) for i in c["fuse"][1]], 3.0)
    got = {e[0]: e[2:] for e in m.recent_points()}
    assert got[700] == (3, 4)
    if both:
        assert got[701] == (5, 10) == (p.points[701].found_cnt_, p.points[701].visible_cnt_)
    else:
        assert 701 not in got


def test_the_restatement_clears_what_the_pointer_model_leaves_dangling():
    """two features of the target carry org: the pointer model replaces the observation and leaves the second feature pointing
    at the bad org (so a later candidate there is counted and nothing happens); the store clears it, and the candidate is added"""
    c = fi.hand_case("two_features_one_org")
    m = fi.run_model(c["script"])
    T, ids = c["fuse"]
    second = [i for i, p in enumerate(m.store[T]["ids"]) if p == 900][1]
    m.fuse_map_points(T, ids)
    assert m.fuse_result()["per_target"] == [(2, 2, 1, 0, 1, 1)]
    assert m.store[T]["ids"][second] == ids[1] and m.store[T]["flags"][second] & 1 and not m.carriers(900)


def _seeded_model_before_the_first_fuse():
    r = fi.ModelRunner(fi.SCENE_CAPS, max_recent=fi.SCENE_RECENT, max_candidates=fi.SCENE_CANDIDATES)
    rest = []
    chain = fi.seeded_chain()
    for i, s in enumerate(chain):
        if s[0] == "neighbors":
            rest = chain[i:]
            break
        r.step(s)
    return r, rest


@pytest.fixture(scope="module")
def seeded(orc):
    """the seeded chain on the model, the local BA solved by the oracle, with the pointer model run beside it through the first
    search_in_neighbors"""
    r, rest = _seeded_model_before_the_first_fuse()
    m = r.m
    p = Pointers(m)
    targets = p.searchInNeighbors(p.kfs[rest[0][1]])
    r.step(rest[0])
    first = dict(targets=targets, result=m.fuse_result(), same=lambda: _same_as_pointers(m, p, "seeded"))
    first["same"]()
    first["gates"] = p.n_gates
    cleared = m.fuse_result()["totals"][5]
    for s in rest[1:]:
        if s[0] == "ba":
            w = m.window(s[1])
            poses, pts, erase, _, rc = orc.local_ba(dict(w, cam=np.array([float(c) for c in m.cam[:5]])))
            assert rc == 0
            m.apply(poses, pts, erase)
            continue
        if s[0] == "cullkf":
            m.cull(s[1], s[2])
            continue
        r.step(s)
        if s[0] == "neighbors":
            cleared += m.fuse_result()["totals"][5]
    first["cleared"] = cleared
    return m, first


def test_search_in_neighbors_equals_the_pointer_model_on_the_seeded_scene(seeded):
    m, first = seeded
    assert first["result"]["targets"][:-1] == first["targets"] and len(first["targets"]) > 10
    assert first["result"]["totals"][1] > 20 and first["gates"] > 500


def test_the_seeded_scene_is_not_vacuous(seeded):
    """an add, a replace in each direction, a cleared feature, a chain of two matches inside one fuse call and a repeated target,
    all in the seeded chain's own log (the last two through fuse_inputs._plant)"""
    m, first = seeded
    kinds = Counter(k for *_, k, _ in m.fuse_log)
    assert kinds["add"] > 0 and kinds["kept_org"] > 0 and kinds["kept_candidate"] > 0
    assert first["cleared"] > 0
    chains = Counter((call, e[2]) for call, e in zip(m.fuse_log_call, m.fuse_log))
    assert max(chains.values()) >= 2
    assert any(e[1] in fi.PLANT_IDS for e in m.fuse_log)
    t = m.fuse_result()["targets"][:-1]
    assert len(set(t)) < len(t)                                            # a repeated target


def _scenes():
    for name in fi.HAND_CASES:
        c = fi.hand_case(name)
        m = fi.run_model(c["script"])
        m.fuse_map_points(*c["fuse"])
        yield name, m
    for both in (True, False):
        c = fi.counters_case(both)
        m = fi.run_model(c["script"])
        m.fuse_map_points(*c["fuse"])
        yield "counters", m
    for n in (64, 65):
        c = fi.holders_case(n)
        m = fi.run_model(c["script"], caps=(80, 256, 1024))
        m.fuse_map_points(*c["fuse"])
        assert m.fuse_result()["totals"] == (1, 1, 0, 0, 1, n - 1)
        yield "holders", m
    c = fi.capacity_candidates_case()
    m = fi.run_model(c["script"], max_candidates=2)
    m.fuse_map_points(*c["fuse"])
    yield "candidates", m
    script, current, _ = fi.composed_case()
    m = fi.run_model(script)
    m.search_in_neighbors(current)
    yield "composed", m
    c = fi.carriers_case()
    m = fi.run_model(c["script"], caps=(16, 256, 1024))
    m.fuse_map_points(*c["fuse"])
    yield "carriers", m
    for bad in (False, True):
        script, current = fi.graph_case(bad)
        m = fi.run_model(script, caps=(16, 512, 8192))
        m.search_in_neighbors(current)
        yield "graph", m


def test_every_float_gate_decides_with_a_margin(seeded):
    """the conditions on the inputs the device comparison relies on, in every scene: relative margin >= 1e-4 at the image bounds,
    the distance range, the normal, both chi-square gates and the radius tests; log(ratio) / log(sf[1]) at least 1e-3 from an
    integer.  (The seeded chain on the device takes the device's created points and a solver's result; tests/test_gpu_fuse.py
    asserts the same conditions on the state it compares.)"""
    for name, m in _scenes():
        assert m.margins and min(x for _, x in m.margins) >= MARGIN, name
        assert min(m.level_fracs) >= LEVEL_MARGIN, name
        assert not m.weak, name
    m, _ = seeded
    assert not m.weak and min(x for _, x in m.margins) >= MARGIN and min(m.level_fracs) >= LEVEL_MARGIN
    assert {g for g, _ in m.margins} == {"img", "dist", "normal", "radius", "chi2"}


def test_the_search_equals_the_oracle(orc, seeded):
    """orc_match_fuse (oracle/match_oracle.c) on the queries of every scene: the same feature or none"""
    sf = np.array([float(s) for s in fi.SF] + [float(fi.SF[-1])] * 8, np.float32)
    n_q = n_hit = 0
    for name, m in list(_scenes()) + [("seeded", seeded[0])]:
        frames = {}
        for T, q in m.queries[:4000]:
            if T not in frames:
                kf = m.store[T]
                frames[T] = orc.FrameData(kf["xy"][:, 0], kf["xy"][:, 1], kf["octave"], kf["angle"], np.array(kf["u_right"], f32), kf["desc"])
            best = np.full(1, -1, np.int32)
            orc.lib().orc_match_fuse(C.byref(frames[T].c), 1, np.ones(1, np.uint8), np.array([q["u"]], f32), np.array([q["v"]], f32),
                                     np.array([q["ur"]], f32), np.array([q["level"]], np.int32), np.ascontiguousarray(q["pdesc"]), 3.0, sf, best)
            m2 = m.search(T, q)
            assert int(best[0]) == m2, (name, T, q["p"])
            n_q, n_hit = n_q + 1, n_hit + (m2 >= 0)
    assert n_q > 1000 and n_hit > 50
