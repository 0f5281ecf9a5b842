"""The culling model (tests/cull_ref.py) against an independent formulation -- a small object model with MapPoint.observedKFs_
and observe_cnt_ maintained incrementally by addObservation / eraseObservedKF and KeyFrame.connectedKFWts_ as dicts,
transcribed from the reference's control flow --, against the hand-made cases of tests/cull_inputs.py, and the C-ABI of the
new entry points (no GPU needed: the calls below fail before they reach the device)."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import cull_inputs as qi
from cull_ref import CullModel

ROOT = pathlib.Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["vo_kfstore_enable_culling", "vo_kfstore_set_keypoints", "vo_kfstore_set_keypoints_dev", "vo_kfstore_set_erase_lock",
               "vo_kfstore_cull_keyframes", "vo_kfstore_erase_keyframe", "vo_kfstore_cull_result", "vo_kfstore_cull_state",
               "vo_kfstore_get_flags"]


# ---- the object model: pointers are objects, pointer-keyed containers are walked in ascending key-frame id --------------------
class MapPoint:
    def __init__(self, pid):
        self.id, self.observedKFs_, self.observe_cnt_, self.bad = pid, {}, 0, False

    def addObservation(self, kf, idx):          # mappoint.cpp:52-64
        if kf in self.observedKFs_:
            return
        self.observedKFs_[kf] = idx
        self.observe_cnt_ += 2 if kf.uRight_[idx] >= 0 else 1

    def eraseObservedKF(self, kf):              # mappoint.cpp:333-360
        erase = False
        if kf in self.observedKFs_:
            idx = self.observedKFs_[kf]
            self.observe_cnt_ -= 2 if kf.uRight_[idx] >= 0 else 1
            del self.observedKFs_[kf]
            if self.observe_cnt_ <= 2:
                erase = True
        if erase:
            self.eraseMapPoint()

    def eraseMapPoint(self):                    # mappoint.cpp:362-381
        self.bad = True
        observed, self.observedKFs_ = self.observedKFs_, {}
        for kf, idx in observed.items():
            kf.mappoints_[idx] = None           # setMapPointNull


class KeyFrame:
    def __init__(self, kid, octave, depth, u_right):
        self.id_, self.octave, self.depth_, self.uRight_ = kid, octave, depth, u_right
        self.mappoints_ = [None] * len(octave)
        self.connectedKFWts_, self.orderedConnectKFs_ = {}, []
        self.firstConnect_, self.parent_, self.children_ = True, None, set()
        self.badFlag_, self.notErase, self.toBeErase = False, False, False

    def updateBestCovisibles(self):             # keyframe.cpp:176-198
        pairs = sorted(((w, kf.id_, kf) for kf, w in self.connectedKFWts_.items()), key=lambda t: t[:2])
        self.orderedConnectKFs_ = [t[2] for t in reversed(pairs)]

    def addConnection(self, kf, w):             # keyframe.cpp:157-171
        if self.connectedKFWts_.get(kf) == w:
            return
        self.connectedKFWts_[kf] = w
        self.updateBestCovisibles()

    def updateConnections(self):                # keyframe.cpp:69-152
        counter = {}
        for mp in self.mappoints_:
            if mp is None or mp.bad:
                continue
            for kf in mp.observedKFs_:
                if kf.id_ != self.id_:
                    counter[kf] = counter.get(kf, 0) + 1
        if not counter:
            return
        nmax, kfmax, pairs = 0, None, []
        for kf in sorted(counter, key=lambda k: k.id_):
            if counter[kf] > nmax:
                nmax, kfmax = counter[kf], kf
            if counter[kf] >= 15:
                pairs.append((counter[kf], kf.id_, kf))
                kf.addConnection(self, counter[kf])
        if not pairs:
            pairs.append((nmax, kfmax.id_, kfmax))
            kfmax.addConnection(self, nmax)
        pairs.sort(key=lambda t: t[:2])
        self.connectedKFWts_ = dict(counter)
        self.orderedConnectKFs_ = [t[2] for t in reversed(pairs)]
        if self.firstConnect_ and self.id_ != 0:
            self.parent_ = self.orderedConnectKFs_[0]
            self.parent_.children_.add(self)
            self.firstConnect_ = False

    def eraseConnection(self, kf):              # keyframe.cpp:512-526
        if kf in self.connectedKFWts_:
            del self.connectedKFWts_[kf]
            self.updateBestCovisibles()

    def eraseKeyFrame(self):                    # keyframe.cpp:400-491
        if self.id_ == 0:
            return
        if self.notErase:
            self.toBeErase = True
            return
        for kf in sorted(self.connectedKFWts_, key=lambda k: k.id_):
            kf.eraseConnection(self)
        for mp in list(self.mappoints_):
            if mp is not None:
                mp.eraseObservedKF(self)
        self.connectedKFWts_, self.orderedConnectKFs_ = {}, []
        cands = [self.parent_] if self.parent_ is not None else []   # (the reference inserts a null pointer here)
        while self.children_:
            go, wmax, parent, child = False, -1, None, None
            for kf in sorted(self.children_, key=lambda k: k.id_):
                if kf.badFlag_:
                    continue
                for c in kf.orderedConnectKFs_:
                    for p in cands:
                        if c.id_ == p.id_:
                            w = kf.connectedKFWts_[c]
                            if w > wmax:
                                wmax, parent, child, go = w, c, kf, True
            if not go:
                break
            child.parent_ = parent
            parent.children_.add(child)
            cands.append(child)
            self.children_.discard(child)
        for kf in self.children_:
            kf.parent_ = self.parent_
            if self.parent_ is not None:
                self.parent_.children_.add(kf)
        self.children_ = set()
        if self.parent_ is not None:
            self.parent_.children_.discard(self)
        self.badFlag_ = True
        self.erased_ = True                     # (bookkeeping of the test: the store never updates an erased key-frame)


def cullingKeyFrames(cur, th_depth):            # localMapping.cpp:434-494
    out = []
    th = np.float32(th_depth)
    for kf in list(cur.orderedConnectKFs_):
        mp_cnt = re_obs = 0
        if kf.badFlag_ or kf.id_ == 0:
            out.append((kf.id_, 0, 0, 3))
            continue
        mappoints = list(kf.mappoints_)
        for i, mp in enumerate(mappoints):
            if mp is None or mp.bad:
                continue
            if kf.depth_[i] < 0 or kf.depth_[i] > th:
                continue
            mp_cnt += 1
            if mp.observe_cnt_ > 3:
                level, obskf = kf.octave[i], 0
                for kfm in sorted(mp.observedKFs_, key=lambda k: k.id_):
                    if kfm.badFlag_ or kfm is kf:
                        continue
                    if kfm.octave[mp.observedKFs_[kfm]] <= level + 1:
                        obskf += 1
                        if obskf >= 3:
                            break
                if obskf >= 3:
                    re_obs += 1
        decided = re_obs > 0.9 * mp_cnt
        if decided:
            kf.eraseKeyFrame()
        out.append((kf.id_, mp_cnt, re_obs, (2 if kf.notErase else 1) if decided else 0))
    return out


class ObjectRunner:
    """a script of tests/cull_inputs.py on the object model (no "points" steps: a key-frame's map points change through
    the erases alone)"""

    def __init__(self):
        self.kfs, self.points, self.result = [], {}, []

    def step(self, s):
        if s[0] == "insert":
            kf = KeyFrame(len(self.kfs), list(s[3]), [np.float32(x) for x in s[4]], [np.float32(x) for x in s[5]])
            self.kfs.append(kf)
            for i, (p, f) in enumerate(zip(s[1], s[2])):
                if f & 1:
                    mp = self.points.get(p)
                    if mp is None or mp.bad:   # (an id that died names a new point when a later key-frame flags it)
                        mp = self.points[p] = MapPoint(p)
                    kf.mappoints_[i] = mp
                    mp.addObservation(kf, i)
        elif s[0] == "update":
            for k in s[1]:
                if not getattr(self.kfs[k], "erased_", False):
                    self.kfs[k].updateConnections()
        elif s[0] == "bad":
            self.kfs[s[1]].badFlag_ = True
        elif s[0] == "lock":
            self.kfs[s[1]].notErase = bool(s[2])
        elif s[0] == "cull":
            self.result = cullingKeyFrames(self.kfs[s[1]], s[2])
        elif s[0] == "erase":
            self.kfs[s[1]].eraseKeyFrame()
        else:
            raise ValueError(s[0])
        return s[0] in ("cull", "erase")

    def compare(self, model):
        """everything the two formulations both define"""
        m = model
        assert self.result == m.result
        for k, kf in enumerate(self.kfs):
            assert {x.id_: w for x, w in kf.connectedKFWts_.items()} == m.conn.W[k], k
            assert [x.id_ for x in kf.orderedConnectKFs_] == m.conn.ordered[k], k
            assert (kf.parent_.id_ if kf.parent_ is not None else -1) == m.conn.parent[k], k
            assert {x.id_ for x in kf.children_} == m.conn.children[k], k
            assert kf.badFlag_ == m.store[k]["bad"] and kf.toBeErase == bool(m.pending[k]), k
            if not m.erased[k]:   # (an erased key-frame's flags bytes are frozen in the restatement and read by nobody)
                assert [int(mp is not None and not mp.bad) for mp in kf.mappoints_] == [f & 1 for f in m.store[k]["flags"]], k
        for p, mp in self.points.items():   # obs(p) IS the incrementally maintained count, the holders ARE observedKFs_
            if not mp.bad:
                assert mp.observe_cnt_ == m.obs(p), p
                assert sorted((kf.id_, i) for kf, i in mp.observedKFs_.items()) == m.observations(p), p


def _both(script):
    o, r = ObjectRunner(), qi.ModelRunner()
    checked = 0
    for s in script:
        after = o.step(s)
        r.step(s)
        if after:
            o.compare(r.m)
            checked += 1
    return r.m, checked


@pytest.mark.parametrize("seed", [3, 4, 5, 6])
def test_model_equals_the_object_model_on_random_sequences(seed):
    script = [s for s in qi.random_script(seed) if s[0] != "points"]
    m, checked = _both(script)
    assert checked >= 9


def test_the_gpu_tests_seed_exercises_every_path():
    m, _ = _both(qi.random_script(qi.SEED))
    qi.assert_not_vacuous(m)


@pytest.mark.parametrize("case", [c for c in qi.hand_cases() if not any(s[0] == "points" for s in c["script"])], ids=lambda c: c["name"])
def test_hand_made_case_on_the_object_model(case):
    _both(case["script"])


@pytest.mark.parametrize("case", qi.hand_cases(), ids=lambda c: c["name"])
def test_hand_made_case_on_the_model(case):
    _, snaps = qi.run_model(case["script"])
    assert case["check"](snaps)


def test_nine_tenths_in_double_is_the_integer_test():
    """`re_obs > 0.9 * mp_cnt` in double decides like 10 re_obs > 9 mp_cnt for every count a store can hold"""
    mp = np.arange(0, 65535, dtype=np.int64)
    first = 9 * mp // 10 + 1                        # the smallest re_obs with 10 re_obs > 9 mp_cnt
    prod = 0.9 * mp.astype(np.float64)
    assert (first.astype(np.float64) > prod).all() and not ((first - 1).astype(np.float64) > prod).any()


def test_columns_never_set_mean_never_culled():
    m = CullModel()
    for k in range(5):
        m.insert(list(range(100, 120)), [1] * 20)
        m.update_connections([k])
    assert m.cull(4, qi.TH) == [(3, 0, 0, 0), (2, 0, 0, 0), (1, 0, 0, 0), (0, 0, 0, 3)] and not any(m.erased)


# ---- the ABI of the new entry points (fails on the parent commit) ------------------------------------------------------------
def test_header_declares_and_binding_lists_the_new_symbols(vo):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "vo_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(vo_[a-z0-9_]+)\s*\(", text))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(vo.SYMBOLS)
    assert all(hasattr(vo.lib(), s) for s in NEW_SYMBOLS)
    for name, value in (("KEPT", 0), ("ERASED", 1), ("PENDING", 2), ("SKIPPED", 3)):
        assert re.search(rf"#define\s+VO_KFSTORE_CULL_{name}\s+{value}\b", text)
        assert getattr(vo.KeyFrameStore, "CULL_" + name) == value
    for method in ("enable_culling", "set_keypoints", "set_erase_lock", "cull_keyframes", "erase_keyframe", "cull_result", "cull_state"):
        assert callable(getattr(vo.KeyFrameStore, method))


def test_null_handles_are_rejected(vo):
    L = vo.lib()
    w = C.c_int32(0)
    assert L.vo_kfstore_enable_culling(None) == -1
    assert L.vo_kfstore_set_keypoints(None, 0, None, None, None) == -1
    assert L.vo_kfstore_set_keypoints_dev(None, 0, None, None, None) == -1
    assert L.vo_kfstore_set_erase_lock(None, 0, 1) == -1
    assert L.vo_kfstore_cull_keyframes(None, 0, C.c_float(5.0)) == -1
    assert L.vo_kfstore_erase_keyframe(None, 0) == -1
    assert L.vo_kfstore_cull_result(None, C.byref(w), None, None, None, None) == -1
    assert L.vo_kfstore_cull_state(None, 0, None, None, None) == -1
    assert L.vo_kfstore_get_flags(None, 0, None, None) == -1
