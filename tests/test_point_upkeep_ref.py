"""The upkeep model (tests/point_upkeep_ref.py) against independent formulations: its descriptor choice against the oracle's
median_descriptor and a literal transcription of mappoint.cpp:145-173; processNewKeyFrame / cullingMapPoints against a small
pointer-object model that maintains observedKFs_, observe_cnt_, found_cnt_ / visible_cnt_ and addedMapPoints_ incrementally
(as tests/test_cull_ref.py does for obs); the hand-made tables of tests/point_upkeep_inputs.py; and the conditions on the seeded
chain that keep the GPU comparison from passing vacuously."""
import numpy as np
import pytest

import point_upkeep_inputs as ui
from new_points_ref import hamming
from point_upkeep_ref import CREATED, CULL, DEAD, FEW_OBS, KEPT, MATURED, PROCESS, RATIO, found_ratio_low

f32 = np.float32


# ---- mappoint.cpp:145-173, line by line ---------------------------------------------------------------------------------------
def literal_choice(desp):
    N = len(desp)
    distances = [[f32(0)] * N for _ in range(N)]
    for i in range(N):
        distances[i][i] = f32(0)
        for j in range(i + 1, N):
            distij = hamming(desp[i], desp[j])
            distances[i][j] = f32(distij)
            distances[j][i] = f32(distij)
    bestMid, bestIdx = 256, 0
    for i in range(N):
        dist = sorted(int(x) for x in distances[i])
        mid = dist[int(0.5 * (N - 1))]
        if mid < bestMid:
            bestMid, bestIdx = mid, i
    return bestIdx


# ---- the pointer model --------------------------------------------------------------------------------------------------------
class MapPoint:
    def __init__(self, pid, kf, idx):           # mappoint.cpp:36-50
        self.id, self.observedKFs_, self.observe_cnt_, self.bad = pid, {}, 0, False
        self.found_cnt_, self.visible_cnt_, self.firstAddedIdxofKF_ = 1, 1, kf.id_
        self.descriptor_, self.computed = kf.desc[idx].copy(), False

    def beObserved(self, kf):
        return kf in self.observedKFs_

    def addObservation(self, kf, idx):          # mappoint.cpp:52-64
        if kf in self.observedKFs_:
            return
        self.observedKFs_[kf] = idx
        self.observe_cnt_ += 2 if kf.uRight_[idx] >= 0 else 1

    def computeDescriptor(self):                # mappoint.cpp:118-179
        if self.bad or not self.observedKFs_:
            return
        desp = [kf.desc[idx] for kf, idx in sorted(self.observedKFs_.items(), key=lambda t: t[0].id_) if not kf.bad]
        if not desp:
            return
        self.descriptor_, self.computed = desp[literal_choice(desp)].copy(), True

    def eraseMapPoint(self):                    # mappoint.cpp:362-381
        self.bad = True
        observed, self.observedKFs_ = self.observedKFs_, {}
        for kf, idx in observed.items():
            kf.mappoints_[idx] = None


class KeyFrame:
    def __init__(self, kid, u_right, desc):
        self.id_, self.uRight_, self.desc, self.bad = kid, u_right, desc, False
        self.mappoints_ = [None] * len(u_right)


class Pointers:
    """insert / process / stats / cullmp / bad of a script.  An id whose map point has been erased comes back as a NEW map point
    (what a caller of the reference would have created).  processNewKeyFrame visits a map point at the key-frame's first
    feature that holds it: the store's "handled once" """

    def __init__(self):
        self.kfs, self.points, self.added = [], {}, []

    def step(self, s):
        if s[0] == "insert":
            kf = KeyFrame(len(self.kfs), [f32(x) for x in s[5]], np.asarray(s[6]["desc"], np.uint8).reshape(-1, 32))
            self.kfs.append(kf)
            for i, (p, fl) in enumerate(zip(s[1], s[2])):
                if not (fl & 1) or p < 0:
                    continue
                mp = self.points.get(p)
                if mp is None or mp.bad:                                   # createNewKeyFrame: constructor + addObservation
                    mp = self.points[p] = MapPoint(p, kf, i)
                    mp.addObservation(kf, i)
                kf.mappoints_[i] = mp                                      # else: attached by the local-map search
        elif s[0] == "process":                                            # localMapping.cpp:110-125
            kf, seen = self.kfs[s[1]], set()
            for i, mp in enumerate(kf.mappoints_):
                if mp is not None and not mp.bad and mp not in seen:
                    seen.add(mp)
                    if not mp.beObserved(kf):
                        mp.addObservation(kf, i)
                        mp.computeDescriptor()
                    elif mp not in self.added:
                        self.added.append(mp)
        elif s[0] == "stats":
            for p, v, f in zip(s[1], s[2], s[3]):
                mp = self.points.get(p)
                if mp is not None and mp in self.added:
                    mp.visible_cnt_ += v
                    mp.found_cnt_ += f
        elif s[0] == "cullmp":                                             # localMapping.cpp:496-524
            cur, keep = s[1], []
            for mp in self.added:
                if mp.bad:
                    continue
                if found_ratio_low(mp.found_cnt_, mp.visible_cnt_):
                    mp.eraseMapPoint()
                elif cur > mp.firstAddedIdxofKF_ + 2 and mp.observe_cnt_ <= 3:
                    mp.eraseMapPoint()
                elif cur > mp.firstAddedIdxofKF_ + 3:
                    pass
                else:
                    keep.append(mp)
            self.added = keep
        elif s[0] == "bad":
            self.kfs[s[1]].bad = True
        elif s[0] not in ("pose", "xy", "update"):
            raise ValueError(s[0])


def _same_as_pointers(script, **kw):
    r, p = ui.ModelRunner(**kw), Pointers()
    n_desc = 0
    for s in script:
        r.step(s), p.step(s)
        if s[0] not in ("process", "cullmp", "stats"):
            continue
        m = r.m
        assert m.recent_points() == sorted((mp.id, mp.firstAddedIdxofKF_, mp.found_cnt_, mp.visible_cnt_) for mp in p.added), s[:2]
        for k, kf in enumerate(p.kfs):
            live = [int(mp is not None and not mp.bad) for mp in kf.mappoints_]
            assert [f & 1 for f in m.store[k]["flags"]] == live, (s[:2], k)
            for i, mp in enumerate(kf.mappoints_):
                if live[i] and mp.computed:
                    n_desc += 1
                    assert m.store[k]["pdesc"][i].tobytes() == mp.descriptor_.tobytes(), (s[:2], k, i)
    return r.m, n_desc


# ---- descriptors --------------------------------------------------------------------------------------------------------------
def _descriptor_sets():
    """every desp the scripts' stores hold: (name, id, list of rows)"""
    out = []
    scripts = {"descriptors": ui.descriptor_case()["script"], "wave_boundary": ui.holders_case(70, (64, 65))["script"],
               "cull": ui.cull_script()}
    scripts.update({"process_" + k: v for k, v in ui.process_cases().items()})
    for name, script in scripts.items():
        m = ui.run_model(script)
        for p in sorted({p for kf in m.store for p in kf["ids"] if p >= 0}):
            out.append((name, p, m.descriptor_set(p)))
    return out


def test_descriptor_choice_equals_the_oracle_and_the_literal_transcription(orc):
    from new_points_ref import median_descriptor
    sets = [s for s in _descriptor_sets() if s[2]]
    assert len(sets) >= 40 and {len(s[2]) for s in sets} >= {1, 2, 3, 4, 64, 65}
    for name, p, desp in sets:
        want = literal_choice(desp)
        assert median_descriptor(desp) == want, (name, p)
        assert orc.lib().orc_median_descriptor(np.ascontiguousarray(np.array(desp, np.uint8).reshape(-1)), len(desp)) == want, (name, p)


def test_descriptor_case_by_hand():
    c = ui.descriptor_case()
    m = ui.run_model(c["script"])
    before = [kf["pdesc"].copy() for kf in m.store]
    m.compute_descriptors(c["ids"])
    for p, win in c["want"].items():
        carriers = m.carriers(p)
        if win is None:
            assert all(m.store[j]["pdesc"][i].tobytes() == before[j][i].tobytes() for j, i in carriers), p
        else:
            assert carriers and all(m.store[j]["pdesc"][i].tobytes() == m.store[win[0]]["desc"][win[1]].tobytes() for j, i in carriers), p
    assert len(m.carriers(106)) == 3 and m.sticky == 0


def test_more_holders_than_the_kernel_stages_keep_the_descriptor():
    c = ui.holders_case(1025, (1024, 1025), NK=2)
    m = ui.run_model(c["script"])
    m.compute_descriptors(c["ids"])
    assert m.sticky == 8
    assert len(m.carriers(100)) == 1024 and len(m.carriers(101)) == 1025
    # the vectorised restatement tests/test_gpu_point_upkeep.py uses at this size elects the model's row
    desp = np.stack(m.descriptor_set(100))
    pop = np.array([bin(x).count("1") for x in range(256)], np.uint8)
    med = np.sort(pop[desp[:, None, :] ^ desp[None, :, :]].sum(2, dtype=np.int32), 1)[:, int(0.5 * (1024 - 1))]
    assert m.store[0]["pdesc"][0].tobytes() == desp[int(np.argmin(med))].tobytes()
    assert all(m.store[j]["pdesc"][i].any() for j, i in m.carriers(100)) and not any(m.store[j]["pdesc"][i].any() for j, i in m.carriers(101))


# ---- process / cull -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in ui.process_cases() if "erased" not in k])
def test_process_equals_the_pointer_model(name):
    m, n_desc = _same_as_pointers(ui.process_cases()[name])
    assert n_desc >= 10 and m.up_record["kind"] == PROCESS


def test_process_cases_by_hand():
    c = ui.process_cases()
    rec = lambda name, **kw: ui.run_model(c[name], **kw)
    m = rec("tracked_and_created_with")
    assert m.split(5) == ([100, 101, 102, 103, 104, 105], [106, 107, 108])
    assert [e for e in m.recent_points() if e[1] == 5] == [(106, 5, 1, 1), (107, 5, 1, 1), (108, 5, 1, 1)]
    assert len(m.recent) == ui.PROCESS_BEFORE + ui.PROCESS_ALONE
    assert m.up_record == dict(m.up_record, n_tracked=6, n_new=3, n_appended=3, n_recent=11) and m.sticky == 0
    # a bad other holder: tracked all the same, its row left out of the descriptor (the current key-frame's own row is the only
    # one), its direction in the normal (two holders)
    m = rec("other_holder_bad")
    assert 104 in m.split(5)[0] and len(m.descriptor_set(104)) == 1 and len(m.observations(104)) == 2
    i = m.store[5]["ids"].index(104)
    assert m.store[5]["pdesc"][i].tobytes() == m.store[5]["desc"][i].tobytes()
    # the only other holder erased: the restatement's choice -- created with the key-frame
    m = rec("other_holder_erased")
    assert 105 in m.split(5)[1] and 105 in m.recent
    m = rec("current_without_a_pose")
    assert m.sticky & 1 and m.up_record["n_tracked"] == 6
    m = rec("current_erased")
    assert m.sticky & 1 and m.up_record == dict(m.up_record, n_tracked=0, n_new=0, n_appended=0) and len(m.recent) == ui.PROCESS_BEFORE
    a, b = rec("tracked_and_created_with"), rec("twice")
    assert a.recent_points() == b.recent_points() and b.up_record["n_new"] == 0
    assert all(np.asarray(a.state(k)[key]).tobytes() == np.asarray(b.state(k)[key]).tobytes() for k in range(6) for key in a.state(k))
    # the capacity met exactly and exceeded by one
    m = rec("tracked_and_created_with", max_recent=ui.PROCESS_BEFORE + ui.PROCESS_ALONE)
    assert len(m.recent) == 11 and m.sticky == 0
    m = rec("tracked_and_created_with", max_recent=ui.PROCESS_BEFORE + ui.PROCESS_ALONE - 1)
    assert len(m.recent) == 8 and m.sticky == 8 and m.up_record == dict(m.up_record, n_new=3, n_appended=0, n_tracked=6, n_recent=8)


@pytest.mark.parametrize("current", [2, 3, 4, 5, 6])
@pytest.mark.parametrize("dead", [False, True])
def test_cull_branches_by_hand_and_against_the_pointer_model(current, dead):
    script = ui.cull_script()
    if dead:
        m = ui.run_model(script + [("erase", 2), ("cullmp", current)])
    else:
        m, _ = _same_as_pointers(script + [("cullmp", current)])
    want = ui.cull_want(current, dead)
    assert {p: m.outcomes[p] for p in want} == want
    assert m.up_erased == sorted(p for p, b in m.outcomes.items() if b in (RATIO, FEW_OBS))
    assert m.up_record["kind"] == CULL and m.up_record["n_erased"] == len(m.up_erased)
    for p in m.up_erased:
        assert not m.carriers(p)
    # the exact quarter is kept, a fifth is not
    assert want[102] != RATIO and want[103] == RATIO and m.recent_points() == sorted(m.recent_points())


def test_all_branches_occur_in_the_hand_script():
    seen = set()
    for current in (2, 3, 4, 5, 6):
        for dead in (False, True):
            seen |= set(ui.cull_want(current, dead).values())
    assert seen == {DEAD, RATIO, FEW_OBS, MATURED, KEPT}


# ---- the seeded chain ---------------------------------------------------------------------------------------------------------
def run_chain_on_the_model(orc, seed=ui.SEED):
    r = ui.ModelRunner(ui.SCENE_CAPS, max_recent=ui.SCENE_RECENT)
    m = r.m
    log = dict(outcomes=[], split=[], created=[], ba=[])
    for s in ui.seeded_chain(seed):
        if s[0] == "ba":
            w = m.window(s[1])
            assert w is not None
            pr = dict(w, cam=np.array([float(c) for c in m.cam[:5]]))
            poses, pts, erase, _, rc = orc.local_ba(pr)
            assert rc == 0
            m.apply(poses, pts, erase)
            log["ba"].append(dict(m.record))
        elif s[0] == "cullkf":
            m.cull(s[1], s[2])
        else:
            if s[0] == "process":
                log["split"].append(tuple(len(x) for x in m.split(s[1])))
            r.step(s)
            if s[0] == "cullmp":
                log["outcomes"].append(dict(m.outcomes))
            if s[0] == "create":
                log["created"].append(m.up_record["n_appended"])
    return m, log


def test_the_seeded_chain_is_not_vacuous(orc):
    m, log = run_chain_on_the_model(orc)
    seen = {b for o in log["outcomes"] for b in o.values()}
    print("branches:", {b: sum(1 for o in log["outcomes"] for x in o.values() if x == b) for b in sorted(seen)}, "split:", log["split"],
          "created:", log["created"], "dead by BA:", [r["n_dead"] for r in log["ba"]])
    assert seen == {DEAD, RATIO, FEW_OBS, MATURED, KEPT}
    assert all(t >= 1 and a >= 1 for t, a in log["split"][1:]) and log["split"][0][1] >= 1      # (key-frame 0 has nothing to track)
    assert all(n >= 1 for n in log["created"]) and m.up_record["kind"] in (CULL, CREATED) and m.sticky == 0
    assert all(e["decisive"] for *_, e in m.evals)      # no create gate could fall the other way on the device
