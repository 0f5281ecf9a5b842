"""The store's local bundle adjustment on the device against the model tests/local_ba_store_ref.py,
through the binding: vo_kfstore_local_ba_window (every array exact; poses6 against tests/se3_ref.py within ten times the
oracle's own error), vo_kfstore_local_ba_apply and vo_kfstore_refresh_points (flags, ids, points, ref_kf, normals, min / max,
the pose column, the record and the sticky word byte for byte), vo_kfstore_local_ba against BundleAdjuster on the same bytes
followed by the model's write-back (identical) and against the oracle within test_gpu_ba.py's bounds, the chain
create_map_points -> local_ba -> update_connections -> cull_keyframes -> build_local_map, and the misuse of every entry point."""
import ctypes as C

import numpy as np
import pytest

import local_ba_inputs as li
import se3_ref
from local_ba_store_ref import EMPTY, OK, OVERFLOW, RECORD

import test_gpu_local_map as lm

pytestmark = pytest.mark.gpu

ctx = lm.ctx   # (its module fixture: the relocalisation inputs of the chain's last step)


def _exp(vo):
    def f(xi):
        R, t = vo.se3_exp(xi)
        return list(R.reshape(-1)) + list(t)
    return f


def _log(vo):
    return lambda T: vo.se3_log(np.asarray(T, np.float64)[:9], np.asarray(T, np.float64)[9:])


class Dev:
    """a script of tests/local_ba_inputs.py on a store.  dev: every other key-frame goes in through insert_dev, and the
    columns, poses, key-point positions and reference key-frames through the device forms of their setters"""

    def __init__(self, vo, K, NK, caps, dev=False, local_ba=True, first_point_id=li.FIRST_ID):
        self.s = vo.KeyFrameStore(K, NK)
        self.s.enable_connections()
        self.s.enable_culling()
        self.s.enable_mapping(li.CAM6, li.SF, first_point_id)
        if local_ba:
            self.s.enable_local_ba(*caps)
        self.dev, self.local_ba, self.keep, self.n = dev, local_ba, [], []

    def step(self, s):
        import torch
        st = self.s
        cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        if s[0] == "insert":
            k = len(st)
            a = li.insert_arrays(s)
            cols = (np.asarray(s[3], np.int32), np.asarray(s[4], np.float32), np.asarray(s[5], np.float32))
            refs = np.asarray(s[6].get("refs", [-1] * len(s[1])), np.int32)
            if self.dev and k % 2:
                a = {key: cuda(v) for key, v in a.items()}
                self.keep.append(a)
                st.insert_dev(a)
            else:
                st.insert(a)
            if self.dev:
                cols, refs = tuple(cuda(c) for c in cols), cuda(refs)
                self.keep += [cols, refs]
            st.set_keypoints(k, *cols)
            if self.local_ba and "refs" in s[6]:
                st.set_point_refs(k, refs)
            self.n.append(len(s[1]))
        elif s[0] == "update":
            st.update_connections(s[1])
        elif s[0] == "bad":
            st.set_bad(s[1])
        elif s[0] == "erase":
            st.erase_keyframe(s[1])
        elif s[0] == "pose":
            T = np.asarray(s[2], np.float64)
            if self.dev:
                self.keep.append(cuda(T))
                T = self.keep[-1]
            st.set_pose(s[1], T)
        elif s[0] == "xy":
            xy = np.asarray(s[2], np.float32)
            if self.dev:
                self.keep.append(cuda(xy))
                xy = self.keep[-1]
            st.set_keypoint_xy(s[1], xy)
        elif s[0] == "create":
            st.create_map_points(s[1], s[2])
        else:
            raise ValueError(s[0])

    def state(self, k):
        p = self.s.points(k, self.n[k])
        T, on = self.s.pose(k)
        return dict(flags=p["flags"], ids=p["ids"], points=p["points"], ref=self.s.point_refs(k, self.n[k]) if self.local_ba else None,
                    normals=p["normals"], min_dist=p["min_dist"], max_dist=p["max_dist"], pose=T if on else np.zeros(12),
                    bad=self.s.flags(k, self.n[k])[1], point_desc=p["point_desc"])


def _same_store(d, m, where, skip=()):
    for k in range(len(m.store)):
        got, want = d.state(k), m.state(k)
        for key, w in want.items():
            if key not in skip:
                assert np.asarray(got[key]).tobytes() == np.asarray(w).tobytes(), (where, k, key)


def _build(vo, case, dev=False):
    NK = case.get("NK", li.NK_HAND)
    K = sum(1 for s in case["script"] if s[0] == "insert")
    d = Dev(vo, K, NK, case["caps"], dev)
    mr = li.ModelRunner(case["caps"], exp=_exp(vo), log=_log(vo))
    for s in case["script"]:
        d.step(s), mr.step(s)
    return d, mr.m


def _poses6_error(d, w):
    worst = 0.0
    for c, k in enumerate(w["cam_keyframe"]):
        T, _ = d.s.pose(int(k))
        worst = max(worst, se3_ref.err(w["poses"][c], se3_ref.log(T[:9].reshape(3, 3), T[9:])))
    return worst


def _same_window(d, got, m, want):
    """-> the worst poses6 error against tests/se3_ref.py"""
    rec = got["record"]
    assert {k: rec[k] for k in RECORD} == m.record
    if want is None:
        assert all(len(v) == 0 for k, v in got.items() if k != "record")
        return 0.0
    for key, w in want.items():
        if key != "poses":
            assert got[key].dtype == w.dtype and got[key].tobytes() == w.tobytes(), key
    worst = _poses6_error(d, got)
    assert got["poses"].shape == want["poses"].shape and worst <= 10 * li.POSES6_ORACLE_WORST, worst
    return worst


CASES = li.hand_cases() + [li.big_case()]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_hand_case_window_apply_and_refresh(vo, case):
    d, m = _build(vo, case)
    d.s.local_ba_window(case["current"])
    want = m.window(case["current"])
    got = d.s.local_ba_window_result()
    assert {k: got["record"][k] for k in case["want"]} == case["want"]
    worst = _same_window(d, got, m, want)
    assert d.s.connections_status() == m.sticky == case.get("sticky", 0)
    m.sticky = 0
    before = [d.state(k) for k in range(len(m.store))]
    if want is None:   # empty or overflowed: an apply is refused and not a byte changes
        z = np.zeros(8)
        with pytest.raises(vo.VoError, match="status -1"):
            d.s.local_ba_apply(z[:6], z[:3], z[:1].astype(np.uint8))
        _same_store(d, m, "refused")
        return
    print(f"{case['name']}: worst poses6 error {worst:.3g} (bound {10 * li.POSES6_ORACLE_WORST:.3g})")
    # refresh_points alone, on a second store with the same contents: every id of the window and one nobody holds
    d2, m2 = _build(vo, case)
    ids = ([99999] + [int(p) for p in want["point_id"]])[:case["caps"][1]]   # (the list's capacity is max_points)
    d2.s.refresh_points(ids), m2.refresh(ids)
    _same_store(d2, m2, "refresh")
    assert any(b["normals"].tobytes() != a["normals"].tobytes() for b, a in zip(before, (d2.state(k) for k in range(len(m.store)))))
    assert d2.s.connections_status() == m2.sticky
    # the write-back of a hand-made result: the case's erases (or a pattern), poses and points moved
    erase = case["erase"](want) if "erase" in case else [e for e in range(len(want["e_cam"])) if (5 * e + 1) % 7 == 0]
    poses, pts = li.perturbation(want)
    msk = li.mask(want, erase)
    d.s.local_ba_apply(poses, pts, msk), m.apply(poses, pts, msk)
    _same_store(d, m, "apply")
    rec = d.s.local_ba_window_result()["record"]
    assert {k: rec[k] for k in RECORD} == m.record and rec["n_erased"] == len(erase)
    if "n_dead" in case:
        assert (rec["n_feature0"], rec["n_dead"]) == (case["n_feature0"], case["n_dead"])
    assert d.s.connections_status() == m.sticky == 0
    free = [int(k) for c, k in enumerate(want["cam_keyframe"]) if not want["fixed"][c]]
    assert free and all(d.state(k)["pose"].tobytes() != before[k]["pose"].tobytes() for k in free)
    assert all(d.state(int(k))["pose"].tobytes() == before[int(k)]["pose"].tobytes() for c, k in enumerate(want["cam_keyframe"]) if want["fixed"][c])
    with pytest.raises(vo.VoError, match="status -1"):   # one window, one apply
        d.s.local_ba_apply(poses, pts, msk)
    # behind the write-back the index is rebuilt: the next window is the model's next window
    d.s.local_ba_window(case["current"])
    _same_window(d, d.s.local_ba_window_result(), m, m.window(case["current"]))


def _run_scene(vo, dev):
    """the seeded scene on a device store and on the model; behind every create step flags and ids are compared and the model
    takes the device's map side (its positions are the float SVD's, equal to the model's within section 4j's tolerance only,
    and everything below is compared exactly)"""
    script = li.seeded_scene(li.SEED)
    d = Dev(vo, 12, 256, li.SCENE_CAPS, dev)
    mr = li.ModelRunner(li.SCENE_CAPS, exp=_exp(vo), log=_log(vo))
    for s in script:
        d.step(s), mr.step(s)
        if s[0] == "create":
            for k in range(len(mr.m.store)):
                got, want = d.state(k), mr.m.state(k)
                for key in ("flags", "ids", "ref"):
                    assert got[key].tobytes() == want[key].tobytes(), (s, k, key)
                mr.m.set_map_side(k, got["points"], got["normals"], got["min_dist"], got["max_dist"])
    return d, mr.m


@pytest.mark.parametrize("dev", [False, True], ids=["host_forms", "dev_forms"])
def test_seeded_scene_composed_call(vo, orc, dev):
    d, m = _run_scene(vo, dev)
    assert sum(1 for kf in m.store for r in kf["ref"] if r >= 9) >= 100        # the create steps wrote reference key-frames
    cur = li.SCENE_CURRENT
    # the window on its own first (enqueue only), against the model
    d.s.local_ba_window(cur)
    want = m.window(cur)
    w = d.s.local_ba_window_result()
    worst = _same_window(d, w, m, want)
    print(f"seeded scene: {w['record']}; worst poses6 error {worst:.3g} (bound {10 * li.POSES6_ORACLE_WORST:.3g})")
    assert w["record"]["n_fixed"] >= 1 and w["record"]["n_points"] >= 300
    pr = {k: w[k] for k in ("poses", "fixed", "points", "e_cam", "e_pt", "e_obs", "e_inv_sigma")}
    pr["cam"] = np.array([float(c) for c in li.CAM6[:5]])
    # the same solver on the same bytes
    ba = vo.BundleAdjuster(pr)
    erase, sums, rc = ba.local_ba()
    poses, pts = ba.state()
    assert rc == 0 and 10 <= int(erase.sum())
    # the composed call on a handle that held another problem
    sums2, rc2 = d.s.local_ba(ba, cur)
    assert rc2 == 0 and [sums2[i].iterations for i in range(2)] == [sums[i].iterations for i in range(2)]
    m.apply(poses, pts, erase)
    _same_store(d, m, "composed")
    rec = d.s.local_ba_window_result()["record"]
    assert {k: rec[k] for k in RECORD} == m.record and rec["n_dead"] >= 1 and d.s.connections_status() == m.sticky == 0
    # against the oracle on the same window: test_gpu_ba.py's bounds
    oposes, opts, oerase, _, orc_rc = orc.local_ba(pr)
    assert orc_rc == 0 and np.array_equal(erase, oerase)
    assert np.abs(poses - oposes).max() < 1e-7
    scale = np.maximum(np.linalg.norm(opts, axis=1), 1.0)[:, None]
    assert (np.abs(pts - opts) <= 1e-8 * scale).all(), float((np.abs(pts - opts) / scale).max())
    ba.close()
    # the chain goes on: update_connections -> cull_keyframes, against the models chained the same way
    d.s.update_connections([cur]), m.update_connections([cur])
    d.s.cull_keyframes(cur, 40.0), m.cull(cur, 40.0)
    assert d.s.cull_result() == m.result
    assert [d.s.connections(k) for k in range(12)] == [m.connections(k) for k in range(12)]
    _same_store(d, m, "culled")


def test_chain_ends_in_the_local_map(vo, ctx):
    """create_map_points -> local_ba -> update_connections -> cull_keyframes -> vo_tracker_build_local_map.  Store A goes
    through the chain on the device, its old ids mapped into the id space of relocalised frames; store B is a plain store
    holding what A holds afterwards (read back; an erased key-frame holds nothing), its graph set from A's connections.  The
    local map built from either is byte-identical, and it lists positions the write-back wrote"""
    from vo_slam_test_amd import synth
    c = ctx
    rng = np.random.default_rng(21)
    max_local, first, cur = 4000, 2_000_000, li.SCENE_CURRENT
    trk_a, _, slots, _ = lm._relocalized(vo, c, max_local)
    trk_b, _, _, _ = lm._relocalized(vo, c, max_local)
    live = rng.permutation(np.unique(slots[slots >= 0]))
    script = [(s[0], [int(live[p % len(live)]) if p >= 0 else -1 for p in s[1]]) + tuple(s[2:]) if s[0] == "insert" else s
              for s in li.seeded_scene(li.SEED)]
    a = Dev(vo, 12, 256, li.SCENE_CAPS, first_point_id=first)
    for s in script:
        a.step(s)
    before = [a.state(k) for k in range(12)]
    ba = vo.BundleAdjuster(synth.make_lba_problem(3, n_kf=4, n_pts=50, n_fixed=1))
    _, rc = a.s.local_ba(ba, cur)
    ba.close()
    assert rc == 0 and a.s.connections_status() == 0
    a.s.update_connections([cur])
    a.s.cull_keyframes(cur, 40.0)
    held = [a.state(k) for k in range(12)]
    moved = np.concatenate([h["ids"][(h["flags"] & 1).astype(bool) & (h["points"] != b["points"]).any(1)] for h, b in zip(held, before)])
    assert len(moved) >= 100
    b = vo.KeyFrameStore(12, 256)
    erased = [a.s.cull_state(k)["erased"] for k in range(12)]
    for k, s in enumerate(s for s in script if s[0] == "insert"):
        arr = li.insert_arrays(s)
        b.insert(dict(arr, flags=held[k]["flags"] * (1 - erased[k]), ids=held[k]["ids"], points=held[k]["points"], point_desc=held[k]["point_desc"],
                      min_dist=held[k]["min_dist"], max_dist=held[k]["max_dist"], bad=held[k]["bad"]))
        b.set_normals(k, held[k]["normals"])
    conn = [a.s.connections(k) for k in range(12)]
    b.set_graph_batch(0, [[] if erased[k] else g["ordered"][:10] for k, g in enumerate(conn)], [g["children"] for g in conn], [g["parent"] for g in conn])
    keys = lm.ARRAYS + ("LOCAL_KEYFRAMES", "LOCAL_N_KEYFRAMES", "LOCAL_N_POINTS", "LOCAL_REF_KF")
    got = []
    for trk, store in ((trk_a, a.s), (trk_b, b)):
        trk.build_local_map(store)
        trk.results()
        got.append({key: trk.get(getattr(trk, key)) for key in keys})
    for key in keys:
        assert got[0][key].tobytes() == got[1][key].tobytes(), key
    assert got[0]["LOCAL_N_KEYFRAMES"].sum() > 0 and np.isin(got[0]["LOCAL_POINT_IDS"], moved).sum() >= 50
    trk_a.close()
    trk_b.close()


def test_stop_flag_writes_nothing_back(vo):
    d, m = _build(vo, CASES[0])
    w0 = m.window(5)
    pr = dict({k: w0[k] for k in ("poses", "fixed", "points", "e_cam", "e_pt", "e_obs", "e_inv_sigma")}, cam=np.array([float(c) for c in li.CAM6[:5]]))
    ba = vo.BundleAdjuster(pr)
    before = [d.state(k) for k in range(6)]
    flag = C.c_ubyte(1)
    _, rc = d.s.local_ba(ba, 5, stop=flag)
    assert rc == -5
    after = [d.state(k) for k in range(6)]
    assert all(np.asarray(b[key]).tobytes() == np.asarray(a[key]).tobytes() for b, a in zip(before, after) for key in b)
    flag.value = 0
    _, rc = d.s.local_ba(ba, 5, stop=flag)   # and the same call with the flag down goes through
    assert rc == 0 and any(np.asarray(b["pose"]).tobytes() != np.asarray(a["pose"]).tobytes() for b, a in zip(before, (d.state(k) for k in range(6))))
    ba.close()


def test_composed_call_reports_empty_and_overflowed_windows(vo):
    by_name = {c["name"][0]: c for c in CASES}
    pr = None
    for key, status, rc_want in (("g", EMPTY, -1), ("k", OVERFLOW, -4), ("l", OVERFLOW, -4), ("m", OVERFLOW, -4)):
        case = by_name[key]
        d, m = _build(vo, case)
        if pr is None:
            from vo_slam_test_amd import synth
            pr = synth.make_lba_problem(3, n_kf=4, n_pts=50, n_fixed=1)
            ba = vo.BundleAdjuster(pr)
        before = [d.state(k) for k in range(6)]
        rc = vo.lib().vo_kfstore_local_ba(d.s._h, ba._h, case["current"], None, None)
        assert rc == rc_want, key
        rec = d.s.local_ba_window_result()["record"]
        assert rec["status"] == status and {k: rec[k] for k in case["want"]} == case["want"]      # the true counts
        after = [d.state(k) for k in range(6)]
        assert all(np.asarray(b[k2]).tobytes() == np.asarray(a[k2]).tobytes() for b, a in zip(before, after) for k2 in b)
    ba.close()


def test_misuse(vo):
    L = vo.lib()
    z, zi, zb = np.zeros(64), np.zeros(64, np.int32), np.zeros(64, np.uint8)
    plain = Dev(vo, 4, 64, li.CAPS, local_ba=False)
    h = plain.s._h
    from vo_slam_test_amd import synth
    ba = vo.BundleAdjuster(synth.make_lba_problem(3, n_kf=4, n_pts=50, n_fixed=1))
    for rc in (L.vo_kfstore_set_point_refs(h, 0, vo._p(zi)), L.vo_kfstore_set_point_refs_dev(h, 0, vo._p(zi)),
               L.vo_kfstore_get_point_refs(h, 0, vo._p(zi)), L.vo_kfstore_local_ba_window(h, 0),
               L.vo_kfstore_local_ba_window_result(h, vo._p(zi), *([None] * 10)), L.vo_kfstore_local_ba_apply(h, vo._p(z), vo._p(z), vo._p(zb)),
               L.vo_kfstore_refresh_points(h, 1, vo._p(zi)), L.vo_kfstore_local_ba(h, ba._h, 0, None, None)):
        assert rc == -1                                                       # no enable_local_ba
    for call in (plain.s.local_ba_window_result, lambda: plain.s.local_ba_window(0), lambda: plain.s.refresh_points([1])):
        with pytest.raises(vo.VoError, match="status -1"):                   # and through the binding
            call()
    for bad in ((0, 8, 8), (8, 0, 8), (8, 8, 0)):
        assert L.vo_kfstore_enable_local_ba(h, *bad) == -1
    no_map = vo.KeyFrameStore(4, 64)
    no_map.enable_connections(), no_map.enable_culling()
    assert L.vo_kfstore_enable_local_ba(no_map._h, 8, 8, 8) == -1            # no enable_mapping
    case = CASES[0]
    d, m = _build(vo, case)
    assert L.vo_kfstore_enable_local_ba(d.s._h, 8, 8, 8) == -1                # not empty
    for call in (lambda: d.s.local_ba_window(6), lambda: d.s.local_ba_window(-1), lambda: d.s.set_point_refs(6, zi[:4]),
                 lambda: d.s.set_point_refs(0, np.full(d.n[0], 6, np.int32)), lambda: d.s.set_point_refs(0, np.full(d.n[0], -2, np.int32)),
                 lambda: d.s.refresh_points([-1]), lambda: d.s.local_ba_apply(z[:6], z[:3], zb[:1])):           # (no window yet)
        with pytest.raises(vo.VoError, match="status -1"):
            call()
    with pytest.raises(vo.VoError, match="status -4"):
        d.s.refresh_points(np.arange(li.CAPS[1] + 1))
    assert L.vo_kfstore_local_ba(d.s._h, None, 5, None, None) == -1
    # an apply after a mutation: any call that writes the store in between
    for mutate in (lambda: d.s.set_bad(1, False), lambda: d.s.set_pose(1, np.asarray(case["script"][1][2])), lambda: d.s.refresh_points([100]),
                   lambda: d.s.update_connections([5]), lambda: d.s.set_erase_lock(2, False)):
        d.s.local_ba_window(5)
        w = d.s.local_ba_window_result()
        mutate()
        with pytest.raises(vo.VoError, match="status -1"):
            d.s.local_ba_apply(w["poses"], w["points"], np.zeros(len(w["e_cam"]), np.uint8))
    d.s.local_ba_window(5)                                                    # reads in between do not count
    w = d.s.local_ba_window_result()
    d.state(3), d.s.connections(2), d.s.connections_status()
    d.s.local_ba_apply(w["poses"], w["points"], np.zeros(len(w["e_cam"]), np.uint8))
    ba.close()


def test_a_store_without_the_opt_in_creates_the_same_points(vo):
    """create_map_points on the seeded scene with and without enable_local_ba: every byte get_points returns, the result
    record and the id counter are the same (the ref_kf column exists on one side only)"""
    script = li.seeded_scene(li.SEED)
    a, b = Dev(vo, 12, 256, li.SCENE_CAPS), Dev(vo, 12, 256, li.SCENE_CAPS, local_ba=False)
    for s in script:
        a.step(s), b.step(s)
        if s[0] == "create":
            assert a.s.new_points_result() == b.s.new_points_result() and a.s.next_point_id() == b.s.next_point_id()
    assert len(a.s.new_points_result()["created"]) > 0
    for k in range(12):
        sa, sb = a.state(k), b.state(k)
        for key in sa:
            if key != "ref":
                assert np.asarray(sa[key]).tobytes() == np.asarray(sb[key]).tobytes(), (k, key)
    assert [a.s.connections(k) for k in range(12)] == [b.s.connections(k) for k in range(12)]
