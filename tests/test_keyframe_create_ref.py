"""CPU tests of the key-frame creation model (tests/keyframe_create_ref.py): the model against a line-by-line pointer-object
transcription of VisualOdometry::initVisualOdometry (src/visualOdometry.cpp:170-198), createNewKeyFrame (:463-517),
cullingTempMapPoints' slot loop (:844-853) and the MapPoint(KeyFrame*) constructor with addObservation / updateNormalAndDepth
(src/mappoint.cpp:36-116), on random frames and on the tables that hit every rule of the depth walk; the hand-worked counts of
those tables; and the model's stated operation order against a plain inv(T) @ p in float64."""
import numpy as np
import pytest

import keyframe_create_inputs as ki
import point_upkeep_inputs as ui
from keyframe_create_ref import KeyframeCreateModel, camera2world, pixel2camera

f32 = np.float32


# ---- the pointer transcription ----------------------------------------------------------------------------------------------
class _KeyFrame:
    def __init__(self, number, T, u_right, octave, erased=False):
        self.number, self.T, self.uRight_, self.octave, self.erased = number, np.asarray(T, np.float64), u_right, octave, erased
        self.mappoints_ = {}

    def getCamCenter(self):
        R, t = self.T[:9].reshape(3, 3), self.T[9:]
        return -R.T @ t


class _MapPoint:
    factory_id_ = 0

    def __init__(self, pos, keyframe, idx, ident=None):          # (mappoint.cpp:36-50)
        self.pos_, self.keyFrame_ref_, self.idx_ = np.asarray(pos, np.float64), keyframe, idx
        self.observedKFs_, self.observe_cnt_ = {}, 0
        self.minDistance_ = self.maxDistance_ = f32(0.0)
        self.normalVector_ = None
        if ident is None:
            ident = _MapPoint.factory_id_
            _MapPoint.factory_id_ += 1
        self.id_ = ident

    def addObservation(self, keyframe, idx):                     # (:52-64)
        if keyframe in self.observedKFs_:
            return
        self.observedKFs_[keyframe] = idx
        self.observe_cnt_ += 2 if keyframe.uRight_[idx] >= 0 else 1

    def getObsCnt(self):
        return self.observe_cnt_

    def updateNormalAndDepth(self, sf):                          # (:66-116)
        if not self.keyFrame_ref_ or not self.observedKFs_:
            return
        normal, n = np.zeros(3), 0
        with np.errstate(all="ignore"):
            for kf in sorted(self.observedKFs_, key=lambda k: k.number):
                ni_ = self.pos_ - kf.getCamCenter()
                normal = normal + ni_ / np.linalg.norm(ni_)
                n += 1
            ref = self.keyFrame_ref_
            dist = f32(np.linalg.norm(self.pos_ - ref.getCamCenter()))
            level = ref.octave[self.observedKFs_[ref]]
            self.maxDistance_ = dist * f32(sf[level])
            self.minDistance_ = self.maxDistance_ / f32(sf[len(sf) - 1])
            self.normalVector_ = normal / n


def _pixel2world(cam, u, v, z, T):                               # (camera.cpp:82-94) with a plain inverse
    fx, fy, cx, cy = (f32(c) for c in cam[:4])
    with np.errstate(all="ignore"):
        x, y = (f32(u) - cx) * f32(z) / fx, (f32(v) - cy) * f32(z) / fy
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = np.asarray(T[:9]).reshape(3, 3), T[9:]
        return (np.linalg.inv(M) @ np.array([float(x), float(y), float(z), 1.0]))[:3]


def _pointer_world(m):
    """the model's store as pointer objects: a MapPoint per id with the observations of its non-erased holders"""
    kfs = [_KeyFrame(k, np.zeros(12) if kf["pose"] is None else kf["pose"], kf["u_right"], kf["octave"], bool(m.erased[k]))
           for k, kf in enumerate(m.store)]
    points = {}
    for k, kf in enumerate(m.store):
        for i, p in enumerate(kf["ids"]):
            if p >= 0:
                mp = points.setdefault(p, _MapPoint(kf["points"][i], kfs[k], i, ident=p))
                if (kf["flags"][i] & 1) and not m.erased[k]:
                    mp.addObservation(kfs[k], i)
    return kfs, points


def _pointer_create(m, f, th_depth, initial):
    """-> (the new _KeyFrame, frame_curr_->mappoints_ afterwards) by the reference's statements"""
    kfs, points = _pointer_world(m)
    n = len(f["depth"])
    _MapPoint.factory_id_ = m.next_id
    # frame_curr_->mappoints_: an id nobody has ever carried is a temporary point of updateLastFrame (no observations)
    mappoints = [None] * n
    if not initial:
        for i, p in enumerate(f["slot_ids"]):
            if p >= 0:
                mappoints[i] = points.get(int(p)) or _MapPoint(np.zeros(3), None, 0, ident=int(p))
        for i in range(n):                                       # cullingTempMapPoints (:844-853)
            mp = mappoints[i]
            if mp and mp.getObsCnt() < 1:
                mappoints[i] = None
    kf = _KeyFrame(len(kfs), f["Tcw12"], f["u_right"], f["octave"])
    kf.mappoints_ = dict(enumerate(mappoints))
    created = []

    def new_point(idx, d):
        p_world = _pixel2world(m.cam, f["x"][idx], f["y"][idx], d, kf.T)
        point = _MapPoint(p_world, kf, idx)
        kf.mappoints_[idx] = point
        mappoints[idx] = point
        point.addObservation(kf, idx)
        point.updateNormalAndDepth(m.sf)
        created.append(idx)

    if initial:                                                  # (:179-198)
        for i in range(n):
            d = f32(f["depth"][i])
            if d < 0:
                continue
            new_point(i, d)
    else:                                                        # (:469-513)
        depthPairs = []
        for i in range(n):
            d = f32(f["depth"][i])
            if d > 0:
                depthPairs.append((d, i))
        if depthPairs:
            depthPairs.sort()
            threshold, point_cnt = f32(th_depth), 0
            for j in range(len(depthPairs)):
                idx, d = depthPairs[j][1], depthPairs[j][0]
                mp = mappoints[idx]
                if not mp or (mp and mp.getObsCnt() < 1):
                    new_point(idx, d)
                    point_cnt += 1
                if d > threshold and point_cnt > 100:
                    break
    return kf, mappoints, created


def _close(a, b, rel=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~fin & ~np.isnan(a)], b[~fin & ~np.isnan(b)])
    scale = max(1.0, float(np.abs(b[fin]).max())) if fin.any() else 1.0
    assert np.all(np.abs(a[fin] - b[fin]) <= rel * scale)


def _holder_model():
    m = KeyframeCreateModel(ki.CAM6, ki.SF, ki.FIRST_ID, ki.CAPS, max_recent=ki.MAX_RECENT)
    r = ui.ModelRunner.__new__(ui.ModelRunner)
    r.m = m
    for s in ki.holder_store():
        r.step(s)
    return m


def _check_against_pointers(f, th, initial):
    m = _holder_model()
    kf, mappoints, created = _pointer_create(m, f, th, initial)
    k = m.create_keyframe(f, th, initial)
    st, rec = m.state(k), m.keyframe_result()
    assert [i for i, _ in rec["created"]] == created                                  # the walk order
    assert [p for _, p in rec["created"]] == [mappoints[i].id_ for i in created]      # factory_id_++ in that order
    assert rec["next_id"] == _MapPoint.factory_id_ and rec["n_created"] == len(created)
    for i, mp in enumerate(mappoints):
        if mp is None:
            assert st["flags"][i] == 0 and st["ids"][i] == -1 and st["ref"][i] == -1 and not st["points"][i].any()
            continue
        assert st["flags"][i] == 3 and st["ids"][i] == mp.id_
        if i in created:
            assert st["ref"][i] == k and st["point_desc"][i].tobytes() == np.asarray(f["desc"][i], np.uint8).tobytes()
            _close(st["points"][i], mp.pos_)
            if np.all(np.isfinite(mp.pos_)) and np.linalg.norm(mp.pos_ - kf.getCamCenter()) > 1e-6:
                _close(st["normals"][i], mp.normalVector_, 1e-9)
                assert abs(float(st["max_dist"][i]) - float(mp.maxDistance_)) <= 2e-6 * float(mp.maxDistance_)
                assert abs(float(st["min_dist"][i]) - float(mp.minDistance_)) <= 2e-6 * float(mp.minDistance_)
        else:   # tracked: the attributes of the map point, as its lowest holder carries them
            j, g = m.first_observation(mp.id_)
            assert st["points"][i].tobytes() == np.asarray(m.store[j]["points"][g], np.float64).tobytes() and st["ref"][i] == m.store[j]["ref"][g]
    return m, rec


TABLES = ki.tables()


@pytest.mark.parametrize("name", list(TABLES))
def test_tables_against_the_pointer_transcription(name):
    f, want = TABLES[name]
    m, rec = _check_against_pointers(f, ki.TH, False)
    assert rec["n_created"] == want, (name, rec)        # the count worked out by hand (keyframe_create_inputs.tables)
    assert rec["first_id"] == ki.FIRST_ID and rec["next_id"] == ki.FIRST_ID + want


def test_tables_hit_their_rules():
    rec = {name: _check_against_pointers(f, ki.TH, False)[1] for name, (f, _) in TABLES.items()}
    assert rec["all_below"]["ended_early"] == 0 and rec["all_below"]["n_walked"] == rec["all_below"]["n_pairs"] == 150
    for k in (100, 101, 102):
        r = rec[f"near_{k}_then_far"]
        assert r["ended_early"] == 1 and r["n_walked"] == k + 1 and r["n_pairs"] == k + 20
    assert rec["fewer_than_101_near"]["n_walked"] == 101 and rec["fewer_than_101_near"]["ended_early"] == 1
    r = rec["far_tracked_ends"]
    assert r["n_walked"] == 102 and r["n_created"] == 101 and r["n_tracked"] == 1     # the tracked pair ends it, uncreated
    r = rec["depth_equals_th"]
    assert r["n_walked"] == 104 and r["n_pairs"] == 105                               # neither d == th pair ends the walk
    f = TABLES["equal_depths"][0]
    made = [i for i, _ in rec["equal_depths"]["created"]]
    assert made[:40] == sorted(made[:40]) and made[40:] == sorted(made[40:])          # equal depths: ids follow the feature index
    assert all(f["depth"][i] == f32(1.25) for i in made[:40])
    r = rec["special_depths"]
    assert r["n_pairs"] == 8 and r["n_tracked"] == 3 and r["ended_early"] == 0        # -1, -0, 0 and NaN are no pairs; +inf is
    r = rec["holder_rules"]
    assert r["n_tracked"] == 9 and r["n_created"] == 5


def test_an_id_in_two_slots_and_the_first_observation():
    f, _ = TABLES["holder_rules"]
    m = _holder_model()
    k = m.create_keyframe(f, ki.TH, False)
    ids = m.store[k]["ids"]
    assert ids.count(ki.HELD[6]) == 2 and ids.count(ki.TWICE) == 2 and ids.count(ki.ERASED_AND_3) == 2
    assert m.first_observation(ki.ERASED_AND_3) == (3, 12) and m.first_observation(ki.BAD_ONLY)[0] == 4
    assert m.first_observation(ki.TWICE) == (0, 12) and m.first_observation(ki.SECOND) == (0, 15)
    assert m.first_observation(ki.ERASED_ONLY) is None and m.first_observation(ki.UNFLAGGED) is None
    i = list(f["slot_ids"]).index(ki.SECOND)
    assert m.store[k]["points"][i].tobytes() == np.asarray(m.store[0]["points"][15]).tobytes()


def test_initial_key_frame_against_the_pointer_transcription():
    f, want = ki.initial_table()
    m = KeyframeCreateModel(ki.CAM6, ki.SF, ki.FIRST_ID, ki.CAPS, max_recent=ki.MAX_RECENT)
    kf, mappoints, created = _pointer_create(m, f, ki.TH, True)
    k = m.create_keyframe(f, ki.TH, True)
    rec = m.keyframe_result()
    assert k == 0 and rec["n_created"] == want == len(created) and [i for i, _ in rec["created"]] == created == sorted(created)
    d = np.asarray(f["depth"])
    zero, nan = np.flatnonzero(d == 0), np.flatnonzero(np.isnan(d))
    assert len(zero) == 2 and len(nan) == 1 and all(i in created for i in list(zero) + list(nan))     # quirk Q-V1
    assert all(m.store[0]["flags"][i] == 0 for i in np.flatnonzero(d < 0))
    for i in created:
        if np.isfinite(d[i]) and d[i] > 0:
            _close(m.store[0]["points"][i], mappoints[i].pos_)


@pytest.mark.parametrize("seed", range(6))
def test_random_frames_against_the_pointer_transcription(seed):
    ids = ki.HELD + [ki.ERASED_ONLY, ki.ERASED_AND_3, ki.BAD_ONLY, ki.UNFLAGGED, ki.TWICE, ki.SECOND, ki.NOBODY]
    f = ki.random_frame(100 + seed, 200 + 9 * seed, ids, p_null=0.5)
    m, rec = _check_against_pointers(f, f32(2.0 + seed), False)
    assert rec["n_created"] > 50 and rec["n_tracked"] > 20


def test_the_operation_order_agrees_with_a_plain_inverse():
    rng = np.random.default_rng(11)
    for _ in range(200):
        f = ki.frame(rng, rng.uniform(0.3, 40.0, 4), [-1] * 4)
        for i in range(4):
            p = camera2world(f["Tcw12"], pixel2camera(ki.CAM6, f["x"][i], f["y"][i], f["depth"][i]))
            want = _pixel2world(ki.CAM6, f["x"][i], f["y"][i], f["depth"][i], f["Tcw12"])
            assert np.all(np.abs(np.array(p) - want) <= 1e-12 * max(1.0, float(np.abs(want).max())))


def test_need_stats_on_the_holder_store():
    m = _holder_model()
    f, _ = TABLES["holder_rules"]
    near = [i for i, d in enumerate(f["depth"]) if 0 < d < ki.TH]
    held = [i for i in near if m.first_observation(int(f["slot_ids"][i]))]
    assert m.need_stats(0, 2, f["depth"], f["slot_ids"], ki.TH)[1:] == (len(held), len(near)) == (7, 12)
    t3, t99 = m.need_stats(0, 3, f["depth"], f["slot_ids"], ki.TH)[0], m.need_stats(0, 99, f["depth"], f["slot_ids"], ki.TH)[0]
    assert t3 >= len(ki.HELD) and t99 == 0                        # ids 0 .. 11 have four holders
    assert m.need_stats(2, 2, f["depth"], f["slot_ids"], ki.TH) == (0, 0, 0) and m.sticky & 1      # an erased reference
    m.sticky = 0
    assert m.need_stats(9, 2, f["depth"], f["slot_ids"], ki.TH) == (0, 0, 0) and m.sticky & 1


def test_the_chain_inputs_are_decisive():
    """the seed of the chain (tests/test_gpu_keyframe_create.py) is chosen here: every triangulation gate of its
    create_map_points is decisive, and the chain creates, tracks and triangulates"""
    m, log = ki.model_chain()
    assert all(e[4]["decisive"] for e in m.evals) and len(m.evals) > 10
    assert sum(1 for e in m.evals if e[4]["accepted"]) > 5
    assert all(r["n_created"] > 20 for r in log["records"]) and all(r["n_tracked"] > 50 for r in log["records"][1:])
    assert log["window"]["status"] == 0 and log["window"]["n_points"] > 100
