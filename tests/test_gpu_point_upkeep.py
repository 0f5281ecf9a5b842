"""Map-point upkeep on the device against the model tests/point_upkeep_ref.py, through the binding:
vo_kfstore_compute_descriptors, process_new_keyframe, add_point_stats, cull_map_points and the append behind
create_map_points.  Everything is compared byte for byte: flags, ids, point_desc, normals, min / max, ref_kf, the recent list,
the record, the erased ids, the connection state and the sticky word.  No tolerance: the only floating-point path is section
4k's refresh, which is exact against its model."""
import numpy as np
import pytest

import local_ba_inputs as li
import point_upkeep_inputs as ui
from point_upkeep_ref import CREATED, DEAD, FEW_OBS, KEPT, MATURED, RATIO, RECORD

from test_gpu_local_ba_store import Dev, _exp, _log

pytestmark = pytest.mark.gpu


class UDev(Dev):
    """test_gpu_local_ba_store.Dev with the opt-in and the four new steps; dev: lists go in as device tensors"""

    def __init__(self, vo, K, NK, caps, dev=False, max_recent=ui.MAX_RECENT, **kw):
        super().__init__(vo, K, NK, caps, dev, **kw)
        if max_recent is not None:
            self.s.enable_point_upkeep(max_recent)

    def _list(self, a):
        a = np.ascontiguousarray(a, np.int32)
        if not self.dev:
            return a
        import torch
        self.keep.append(torch.from_numpy(a).cuda())
        return self.keep[-1]

    def step(self, s):
        if s[0] == "process":
            self.s.process_new_keyframe(s[1])
        elif s[0] == "descriptors":
            self.s.compute_descriptors(self._list(s[1]))
        elif s[0] == "stats":
            self.s.add_point_stats(*(self._list(x) for x in s[1:4]))
        elif s[0] == "cullmp":
            self.s.cull_map_points(s[1])
        else:
            super().step(s)


def _model(vo, caps=ui.CAPS, max_recent=ui.MAX_RECENT):
    return ui.ModelRunner(caps, exp=_exp(vo), log=_log(vo), max_recent=max_recent)


def _same(d, m, where, store=True):
    """the device store against the model, byte for byte; the sticky words are read (and cleared) on both sides"""
    K = len(m.store)
    if store:
        for k in range(K):
            got, want = d.state(k), m.state(k)
            for key, w in want.items():
                assert np.asarray(got[key]).tobytes() == np.asarray(w).tobytes(), (where, k, key)
        assert [d.s.connections(k) for k in range(K)] == [m.connections(k) for k in range(K)], where
    assert d.s.recent_points() == m.recent_points(), where
    got = d.s.upkeep_result()
    assert got == m.upkeep_result() and set(RECORD) <= set(got), (where, got, m.upkeep_result())
    assert d.s.connections_status() == m.sticky, where
    m.sticky = 0


def _run(vo, script, K, NK=ui.NK_HAND, dev=False, max_recent=ui.MAX_RECENT, caps=ui.CAPS, check=("process", "descriptors", "stats", "cullmp")):
    d, mr = UDev(vo, K, NK, caps, dev, max_recent), _model(vo, caps, max_recent)
    for i, s in enumerate(script):
        d.step(s), mr.step(s)
        if s[0] in check:
            _same(d, mr.m, (i, s[:2]))
    return d, mr.m


# ---- computeDescriptor ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True], ids=["host_form", "dev_form"])
def test_descriptors_hand_case(vo, dev):
    c = ui.descriptor_case()
    ids = c["ids"] + ([-1] if dev else [])        # (the device form skips a negative entry)
    d, m = _run(vo, c["script"] + [("descriptors", ids)], 6, dev=dev)
    zero = bytes(32)
    for p, win in c["want"].items():
        for j, i in m.carriers(p):
            got = d.state(j)["point_desc"][i].tobytes()
            assert got == (zero if win is None else m.store[win[0]]["desc"][win[1]].tobytes()), (p, j, i)
    assert len(m.carriers(106)) == 3 and m.descriptor_set(105) == [] and len(m.observations(105)) == 1


def test_descriptors_at_the_wave_boundary(vo):
    """70 key-frames: a point of exactly 64 holders (the wavefront kernel) and one of 65 (the overflow list)"""
    c = ui.holders_case(70, (64, 65))
    d, m = _run(vo, c["script"] + [("descriptors", c["ids"])], 70, NK=4)
    assert [len(m.descriptor_set(p)) for p in c["ids"]] == [64, 65]
    assert all(d.state(j)["point_desc"][i].any() for p in c["ids"] for j, i in m.carriers(p))


def test_descriptors_at_the_holder_capacity(vo):
    """1025 key-frames: 1024 holders are computed, 1025 keep their descriptor and raise the sticky bit.  The expected row comes
    from a vectorised restatement of the selection (the model's pair-by-pair one takes seconds at this size;
    tests/test_point_upkeep_ref.py holds the two equal on the sets the model is run on)"""
    c = ui.holders_case(1025, (1024, 1025), NK=2)
    d = UDev(vo, 1025, 2, ui.CAPS)
    for s in c["script"]:
        d.step(s)
    d.step(("descriptors", c["ids"]))
    assert d.s.connections_status() == vo.KeyFrameStore.CONNECTIONS_UPKEEP_CAPACITY
    desp = np.stack([s[6]["desc"][0] for s in c["script"][:1024]])
    pop = np.array([bin(x).count("1") for x in range(256)], np.uint8)
    dist = pop[desp[:, None, :] ^ desp[None, :, :]].sum(2, dtype=np.int32)
    med = np.sort(dist, 1)[:, int(0.5 * (1024 - 1))]
    win = desp[int(np.argmin(med))].tobytes()          # (argmin: the first of equal medians)
    got = [d.s.points(k, len(c["script"][k][1]))["point_desc"] for k in range(1025)]
    assert all(got[k][0].tobytes() == win for k in range(1024))
    assert not any(got[k][1].any() for k in range(1024)) and not got[1024][0].any()


# ---- processNewKeyFrame -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ui.process_cases()))
def test_process_cases(vo, name):
    d, m = _run(vo, ui.process_cases()[name], 6)
    assert m.up_record["current"] == 5
    if name == "other_holder_bad":       # tracked through a bad holder: its row left out, its direction in the normal
        i = m.store[5]["ids"].index(104)
        st = d.state(5)
        assert st["point_desc"][i].tobytes() == m.store[5]["desc"][i].tobytes() and st["normals"][i].any()
    if name == "other_holder_erased":
        assert (105, 2, 1, 1) in d.s.recent_points() or (105, 5, 1, 1) in d.s.recent_points()
    if name == "current_erased":
        assert d.s.upkeep_result()["n_tracked"] == 0


@pytest.mark.parametrize("spare", [0, -1], ids=["met_exactly", "exceeded_by_one"])
def test_process_at_the_list_capacity(vo, spare):
    R = ui.PROCESS_BEFORE + ui.PROCESS_ALONE + spare
    d, m = _run(vo, ui.process_cases()["tracked_and_created_with"], 6, max_recent=R)
    rec = d.s.upkeep_result()
    assert (rec["n_new"], rec["n_appended"], rec["n_tracked"]) == (3, 3 if spare == 0 else 0, 6)
    assert len(d.s.recent_points()) == (R if spare == 0 else ui.PROCESS_BEFORE)


# ---- the counters and cullingMapPoints --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True], ids=["host_form", "dev_form"])
def test_stats_forms(vo, dev):
    """absent ids, negative ids and repeats (the script's stats step), then a second step on top"""
    script = ui.cull_script() + [("stats", [103, 103, 100, 555, -1], [1, 2, 3, 4, 5], [1, 0, 3, 4, 5])]
    d, m = _run(vo, script, 7, dev=dev, check=("stats",))
    got = {e[0]: e[2:] for e in d.s.recent_points()}
    assert got[102] == (1, 4) and got[103] == (2, 8) and got[105] == (1, 5) and got[100] == (4, 4) and got[101] == (1, 1)


@pytest.mark.parametrize("current", [2, 3, 4, 5, 6])
@pytest.mark.parametrize("dead", [False, True], ids=["", "kf2_erased"])
def test_cull_branches(vo, current, dead):
    script = ui.cull_script() + ([("erase", 2)] if dead else []) + [("cullmp", current)]
    d, m = _run(vo, script, 7, check=("cullmp",))
    want = ui.cull_want(current, dead)
    assert {p: m.outcomes[p] for p in want} == want
    rec = d.s.upkeep_result()
    assert rec["erased"] == sorted(p for p, b in m.outcomes.items() if b in (RATIO, FEW_OBS)) and 103 in rec["erased"] and 105 in rec["erased"]
    assert [rec[k] for k in ("n_dead", "n_ratio", "n_few_obs", "n_matured", "n_kept")] == [sum(1 for b in m.outcomes.values() if b == x)
                                                                                            for x in (DEAD, RATIO, FEW_OBS, MATURED, KEPT)]
    # point 5 sits in two features of key-frame 1: both have lost bit 0
    f1 = d.state(1)
    assert [int(f) & 1 for f, p in zip(f1["flags"], f1["ids"]) if p == 105] == [0, 0]
    # behind the erases the index is rebuilt: a second call finds the survivors only
    d.step(("cullmp", current)), m.cull_map_points(current)
    _same(d, m, "second cull")


# ---- the chain --------------------------------------------------------------------------------------------------------------
def test_seeded_chain(vo):
    """insert_dev -> process_new_keyframe -> add_point_stats -> cull_map_points for every key-frame of the seeded scene, and
    create_map_points -> local_ba -> cull_keyframes behind the last three; compared after every step.  Behind a create step
    flags, ids and reference key-frames are compared and the model takes the device's map side (its positions are the float
    SVD's, section 4j's tolerance)"""
    d, mr = UDev(vo, ui.K_SCENE, ui.N_FEAT, ui.SCENE_CAPS, True, ui.SCENE_RECENT), _model(vo, ui.SCENE_CAPS, ui.SCENE_RECENT)
    m, ba, seen, created = mr.m, None, set(), []
    for i, s in enumerate(ui.seeded_chain()):
        where = (i, s[:2])
        if s[0] == "ba":
            d.s.local_ba_window(s[1])
            want, w = m.window(s[1]), d.s.local_ba_window_result()
            assert want is not None and w["record"]["status"] == 0 and w["point_id"].tobytes() == want["point_id"].tobytes(), where
            pr = dict({k: w[k] for k in ("poses", "fixed", "points", "e_cam", "e_pt", "e_obs", "e_inv_sigma")}, cam=np.array([float(c) for c in li.CAM6[:5]]))
            if ba is None:
                ba = vo.BundleAdjuster(pr)
            else:
                ba.reset(pr)
            erase, _, rc = ba.local_ba()
            poses, pts = ba.state()
            _, rc2 = d.s.local_ba(ba, s[1])
            assert rc == 0 and rc2 == 0, where
            m.apply(poses, pts, erase)
            _same(d, m, where)
        elif s[0] == "cullkf":
            d.s.cull_keyframes(s[1], s[2]), m.cull(s[1], s[2])
            assert d.s.cull_result() == m.result, where
            _same(d, m, where)
        else:
            d.step(s), mr.step(s)
            if s[0] == "create":
                for k in range(len(m.store)):
                    got, want = d.state(k), m.state(k)
                    for key in ("flags", "ids", "ref"):
                        assert got[key].tobytes() == want[key].tobytes(), (where, k, key)
                    m.set_map_side(k, got["points"], got["normals"], got["min_dist"], got["max_dist"])
                assert m.up_record["kind"] == CREATED
                created.append(m.up_record["n_appended"])
                _same(d, m, where)
            elif s[0] in ("process", "stats", "cullmp"):
                _same(d, m, where, store=s[0] != "stats")
                if s[0] == "cullmp":
                    seen |= set(m.outcomes.values())
    ba.close()
    assert seen == {DEAD, RATIO, FEW_OBS, MATURED, KEPT} and all(n >= 1 for n in created) and len(created) == 3


# ---- opt-in and misuse ------------------------------------------------------------------------------------------------------
def test_a_store_without_the_opt_in_creates_the_same_points_and_refuses_the_calls(vo):
    script = [s for s in ui.seeded_chain() if s[0] in ("insert", "pose", "xy", "create")]
    script = [x for s in script for x in ([s, ("update", [s[1]])] if s[0] == "xy" else [s])]
    a, b = UDev(vo, ui.K_SCENE, ui.N_FEAT, ui.SCENE_CAPS, max_recent=ui.SCENE_RECENT), UDev(vo, ui.K_SCENE, ui.N_FEAT, ui.SCENE_CAPS, max_recent=None)
    n_created = 0
    for s in script:
        a.step(s), b.step(s)
        if s[0] == "create":
            ra = a.s.new_points_result()
            assert ra == b.s.new_points_result() and a.s.next_point_id() == b.s.next_point_id()
            n_created += len(ra["created"])
            assert a.s.upkeep_result()["n_appended"] == len(ra["created"])
    assert n_created > 0 and sorted(e[0] for e in a.s.recent_points()) == list(range(li.FIRST_ID, li.FIRST_ID + n_created))
    for k in range(ui.K_SCENE):
        sa, sb = a.state(k), b.state(k)
        for key in sa:
            assert np.asarray(sa[key]).tobytes() == np.asarray(sb[key]).tobytes(), (k, key)
    L, h, zi = vo.lib(), b.s._h, np.zeros(8, np.int32)
    for rc in (L.vo_kfstore_compute_descriptors(h, 1, vo._p(zi)), L.vo_kfstore_compute_descriptors_dev(h, 1, vo._p(zi)),
               L.vo_kfstore_process_new_keyframe(h, 0), L.vo_kfstore_add_point_stats(h, 1, vo._p(zi), vo._p(zi), vo._p(zi)),
               L.vo_kfstore_add_point_stats_dev(h, 1, vo._p(zi), vo._p(zi), vo._p(zi)), L.vo_kfstore_cull_map_points(h, 0),
               L.vo_kfstore_recent_points(h, None, None, None, None, None), L.vo_kfstore_upkeep_result(h, vo._p(zi), None),
               L.vo_kfstore_enable_point_upkeep(h, 8)):                       # (the last: not empty)
        assert rc == -1
    assert b.s.connections_status() == 0


def test_misuse(vo):
    L = vo.lib()
    zi, neg = np.zeros(64, np.int32), np.full(4, -1, np.int32)
    no_ba = Dev(vo, 4, 16, li.CAPS, local_ba=False)
    assert L.vo_kfstore_enable_point_upkeep(no_ba.s._h, 8) == -1            # no enable_local_ba
    e = Dev(vo, 4, 16, li.CAPS)
    assert L.vo_kfstore_enable_point_upkeep(e.s._h, 0) == -1 and L.vo_kfstore_enable_point_upkeep(None, 8) == -1
    assert L.vo_kfstore_enable_point_upkeep(e.s._h, 8) == 0 and L.vo_kfstore_enable_point_upkeep(e.s._h, 8) == 0
    d, m = _run(vo, ui.process_cases()["tracked_and_created_with"], 6, max_recent=16)
    h, cap = d.s._h, 16 + ui.NK_HAND
    before = [d.state(k) for k in range(6)], d.s.recent_points()
    big = np.zeros(cap + 1, np.int32)
    assert L.vo_kfstore_compute_descriptors(h, cap + 1, vo._p(big)) == -4 and L.vo_kfstore_compute_descriptors_dev(h, cap + 1, vo._p(big)) == -4
    assert L.vo_kfstore_add_point_stats(h, cap + 1, vo._p(big), vo._p(big), vo._p(big)) == -4
    for rc in (L.vo_kfstore_compute_descriptors(h, 4, vo._p(neg)), L.vo_kfstore_compute_descriptors(h, -1, vo._p(zi)),
               L.vo_kfstore_compute_descriptors(h, 1, None), L.vo_kfstore_compute_descriptors_dev(h, 1, None),
               L.vo_kfstore_process_new_keyframe(h, 6), L.vo_kfstore_process_new_keyframe(h, -1),
               L.vo_kfstore_add_point_stats(h, 4, vo._p(zi), vo._p(neg), vo._p(zi)), L.vo_kfstore_add_point_stats(h, 4, vo._p(zi), vo._p(zi), vo._p(neg)),
               L.vo_kfstore_add_point_stats(h, 1, vo._p(zi), None, vo._p(zi)), L.vo_kfstore_add_point_stats_dev(h, 1, None, None, None),
               L.vo_kfstore_cull_map_points(h, 6), L.vo_kfstore_cull_map_points(h, -1), L.vo_kfstore_enable_point_upkeep(h, 16)):
        assert rc == -1
    assert L.vo_kfstore_compute_descriptors(h, 0, None) == 0 and L.vo_kfstore_add_point_stats(h, 0, None, None, None) == 0
    assert L.vo_kfstore_recent_points(h, None, None, None, None, None) == 0 and L.vo_kfstore_upkeep_result(h, None, None) == 0
    after = [d.state(k) for k in range(6)], d.s.recent_points()
    assert before[1] == after[1] and all(np.asarray(b[key]).tobytes() == np.asarray(a[key]).tobytes() for b, a in zip(before[0], after[0]) for key in b)
    with pytest.raises(vo.VoError, match="differ in length"):
        d.s.add_point_stats([1, 2], [1], [1])
