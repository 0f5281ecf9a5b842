"""The motion route from the key-frame store on the device against the model tests/motion_store_ref.py,
through the binding: vo_tracker_build_local_map after vo_tracker_track_first, vo_tracker_point_stats,
vo_tracker_record_ref_pose / vo_tracker_refresh_last_pose.  The model is applied to the tracker's state as read before each call.
Every discrete output is compared exactly; the poses are compared bit for bit with the model evaluated on the device's own
FRAME_POSE and on the store's poses read back with vo_kfstore_get_pose.  No tolerance is introduced."""
import ctypes as C

import numpy as np
import pytest

import handover_inputs as hi
import motion_store_inputs as mi
import test_gpu_handover as th
from handover_ref import HandoverModel, compose
from motion_store_ref import RefPoseModel, build, link, slot_ids, stats
from test_gpu_local_map import ARRAYS, _device_store

pytestmark = pytest.mark.gpu
f32 = np.float32
MAX_LOCAL = 2048
LM_KEYS = ("LOCAL_KEYFRAMES", "LOCAL_N_KEYFRAMES", "LOCAL_N_POINTS", "LOCAL_REF_KF")
STAT_KEYS = ("STAT_IDS", "STAT_VISIBLE", "STAT_FOUND")
_CACHE = {}


def _world(vo):
    """the streams, the maps of frame 0 with the streams' id offsets, the synthetic store's key-frames and their model"""
    if "w" not in _CACHE:
        imgs, raw, maps, cap, _ = th._inputs(vo, "synth")
        maps = mi.stream_maps(maps)
        kfs = mi.store(maps)
        _CACHE["w"] = (imgs, raw, maps, cap, kfs, mi.model_store(kfs))
    return _CACHE["w"]


def _tracker(vo, max_local=MAX_LOCAL, ids="all", stream=None, relabel=None, beyond=0):
    """a tracker whose last-frame list is the maps' (no local map).  ids: "all", "held" (entries whose id no key-frame holds carry
    none: no slot is nulled) or None; relabel: a function applied to the ids handed in; beyond > 0: max_last = max_features +
    beyond and the list handed in back to front over all max_last entries, so that every stream's first entries lie at indices
    >= max_features"""
    imgs, raw, maps, cap, kfs, _ = _world(vo)
    n_last = cap + beyond if beyond else max(len(m[1]["flags"]) for m in maps)
    trk = vo.Tracker(hi.B, hi.CAM5, None, hi.W, hi.H, max_last=cap + beyond, max_local=max_local, inv_depth_scale=float(hi.INV), stream=stream,
                     single_stream=stream is not None)
    T = np.stack([m[0] for m in maps])
    turn = (lambda a: np.ascontiguousarray(a[:, ::-1])) if beyond else (lambda a: a)
    la = {k: turn(th._stack([m[1][k] for m in maps], n_last)) for k in ("points", "flags", "octave", "angle", "desc")}
    trk.set_last_frame(T, la["points"], la["flags"], la["octave"], la["angle"], la["desc"])
    if ids is not None:
        lid = turn(th._stack([m[1]["ids"] for m in maps], n_last, -1))
        if ids == "held":
            held = np.unique(np.concatenate([k["ids"][(k["flags"] & 1) != 0] for k in kfs]))
            lid = np.where(np.isin(lid, held), lid, -1).astype(np.int32)
        trk.set_last_frame_ids(lid if relabel is None else relabel(lid))
    trk.set_last_pose(T, np.ones(hi.B, np.uint8))
    return trk


def _first_state(trk):
    """what the model takes of the tracker behind vo_tracker_track_first"""
    return dict(n=[trk.download_frame(f)["n"] for f in range(trk.B)], has=trk.get(trk.FEATURE_HAS_POINT), a0=trk.get(trk.ASSIGNED_LAST),
                last_ids=trk.get(trk.LAST_IDS), last_flags=trk.get(trk.LAST_FLAGS))


def _model_build(vo, s, max_local, f):
    _, _, _, cap, kfs, mstore = _world(vo)
    w, first, has = build(s["n"][f], s["has"][f], s["a0"][f], s["last_ids"][f], mstore, max_local)
    loc = mi.local_map(w, kfs, max_local)
    loc["link"] = link(s["last_flags"][f], s["last_ids"][f], loc["ids"])
    return w, first, has, loc


def _compare_build(vo, trk, s, max_local, expect_capacity=False):
    """every output of the build on the motion route against the model -> per frame (build_local_map's dict, local map)"""
    want = [_model_build(vo, s, max_local, f) for f in range(trk.B)]
    assert any(w[0]["capacity"] for w in want) == expect_capacity
    if expect_capacity:
        with pytest.raises(vo.VoError, match="status -4"):
            trk.results()
    trk.results()                                             # (sticky: reported once)
    lk, nk, npts, best = (trk.get(getattr(trk, key)) for key in LM_KEYS)
    got = {key: trk.get(getattr(trk, key)) for key in ARRAYS}
    first, has = trk.get(trk.FIRST_SLOT_IDS), trk.get(trk.FEATURE_HAS_POINT)
    for f, (w, wfirst, whas, loc) in enumerate(want):
        assert list(lk[f]) == w["keyframes"] + [-1] * (84 - len(w["keyframes"])), f
        assert (nk[f], npts[f], best[f]) == (w["n_keyframes"], w["n_points"], w["best"]), f
        n = len(loc["ids"])
        for key, col in (("LOCAL_POINTS", "points"), ("LOCAL_NORMALS", "normals"), ("LOCAL_MIN_DISTANCE", "min_dist"), ("LOCAL_MAX_DISTANCE", "max_dist"),
                         ("LOCAL_DESC", "desc"), ("LOCAL_MAP_FLAGS", "valid"), ("LOCAL_POINT_IDS", "ids"), ("LOCAL_LINK", "link")):
            assert got[key][f, :n].dtype == loc[col].dtype and got[key][f, :n].tobytes() == loc[col].tobytes(), (f, key)
        assert not got["LOCAL_MAP_FLAGS"][f, n:max_local].any() and (got["LOCAL_POINT_IDS"][f, n:max_local] == -1).all()
        assert (got["LOCAL_LINK"][f, n:max_local] == -1).all()
        assert np.array_equal(first[f], wfirst) and np.array_equal(has[f], whas), f
    return want


def test_build_after_the_motion_route(vo):
    """frame 0 (every stream tracks; most slot ids are held by no key-frame and are nulled, temporary points are not) and frame 1
    (stream 2 is lost: an empty map, best key-frame -1)"""
    imgs, raw, _, _, kfs, _ = _world(vo)
    store = _device_store(vo, kfs, mi.NK)
    trk = _tracker(vo)
    counts = None
    for k in range(2):
        trk.track_first(imgs[k], raw[k])
        trk.results()
        s = _first_state(trk)
        before = np.stack([slot_ids(s["n"][f], s["has"][f], s["a0"][f], s["last_ids"][f]) for f in range(trk.B)])
        trk.build_local_map(store)
        want = _compare_build(vo, trk, s, MAX_LOCAL)
        first = np.stack([w[1] for w in want])
        if k == 0:
            counts = [w[0]["n_points"] for w in want]
            assert ((before >= 0) & (first < 0)).sum() >= 1 and all(c > 0 for c in counts)
            assert all(mi.KF_PER_STREAM * f + 3 in w[0]["keyframes"] for f, w in enumerate(want))       # the expansion acted
            assert all((w[3]["link"] >= 0).any() and (w[3]["link"] < 0).any() for w in want)
        else:
            temp = (s["has"] != 0) & (before < 0)                                                          # temporary points of begin_frame:
            assert temp.any() and(trk.get(trk.FEATURE_HAS_POINT) != 0)[temp].all()              # no id, no vote, not nulled
            assert want[hi.LOST][0]["keyframes"] == [] and want[hi.LOST][0]["best"] == -1 and all(w[0]["best"] >= 0 for w in want[:2])
        trk.track_local_map()
        trk.end_frame(2.0), trk.begin_frame(2.0)
    trk.close()
    # max_local one below the largest frame's count: sticky VO_ERR_CAPACITY, the other frames stay valid
    small = max(counts) - 1
    assert sorted(counts)[-2] < small
    trk = _tracker(vo, max_local=small)
    trk.track_first(imgs[0], raw[0])
    trk.results()
    s = _first_state(trk)
    trk.build_local_map(store)
    want = _compare_build(vo, trk, s, small, expect_capacity=True)
    assert max(w[0]["n_points"] for w in want) == small + 1 and max(len(w[3]["ids"]) for w in want) == small
    trk.close(), store.close()


def test_link_reaches_last_entries_beyond_max_features(vo):
    """max_last = max_features + 512 and a host-set list whose first 512 entries per stream lie at indices >= max_features: their
    ids vote, their points enter the local map WITH their link, and the local search skips them (no point is claimed a second time)"""
    imgs, raw, _, cap, kfs, _ = _world(vo)
    store = _device_store(vo, kfs, mi.NK)
    trk = _tracker(vo, beyond=512)
    assert trk.max_last == cap + 512
    trk.track_first(imgs[0], raw[0])
    trk.results()
    s = _first_state(trk)
    assert s["last_flags"].shape[1] == cap + 512 and all((s["a0"][f] >= cap).sum() >= 20 for f in range(trk.B))
    trk.build_local_map(store)
    want = _compare_build(vo, trk, s, MAX_LOCAL)
    matched = np.zeros(s["last_flags"].shape, bool)
    for f in range(trk.B):
        matched[f, s["a0"][f][s["a0"][f] >= 0]] = True
    skipped = [(w[3]["link"] >= cap) & matched[f][np.clip(w[3]["link"], 0, None)] for f, w in enumerate(want)]
    print("links to matched entries beyond max_features:", [int(sk.sum()) for sk in skipped])
    assert all(sk.sum() >= 1 for sk in skipped) and sum(int(sk.sum()) for sk in skipped) >= 10
    trk.track_local_map()
    a1 = trk.get(trk.ASSIGNED_LOCAL)
    for f, sk in enumerate(skipped):
        assert not np.isin(a1[f][a1[f] >= 0], np.nonzero(sk)[0]).any(), f
    trk.close(), store.close()


def _snapshot(trk):
    out = dict(trk.results())
    out["ASSIGNED_LOCAL"] = trk.get(trk.ASSIGNED_LOCAL)
    return out


def _set_local(trk, locs, max_local, relabel=None):
    """the model's local maps through vo_tracker_set_local_map / _ids with their link"""
    B = len(locs)
    z = lambda shape, dt, fill=0: np.full((B, max_local) + shape, fill, dt)
    arr = dict(points=z((3,), np.float64), normals=z((3,), np.float64), min_dist=z((), f32), max_dist=z((), f32), valid=z((), np.uint8),
               desc=z((32,), np.uint8), link=z((), np.int32, -1), ids=z((), np.int32, -1))
    for f, loc in enumerate(locs):
        for key in arr:
            arr[key][f, :len(loc[key])] = loc[key]
    trk.set_local_map(arr["points"], arr["normals"], arr["min_dist"], arr["max_dist"], arr["valid"], arr["desc"], link=arr["link"])
    trk.set_local_map_ids(arr["ids"] if relabel is None else relabel(arr["ids"]))


def _empty_local(trk):
    """a local map of eight absent points, without ids"""
    z = lambda shape, dt: np.zeros((trk.B, 8) + shape, dt)
    trk.set_local_map(z((3,), np.float64), z((3,), np.float64), z((), f32), z((), f32), z((), np.uint8), z((32,), np.uint8))


def _stats_want(trk, first_ids):
    """the model's three arrays on the tracker's state behind vo_tracker_track_local_map"""
    n = [trk.download_frame(f)["n"] for f in range(trk.B)]
    a1, out, lid, lfl = trk.get(trk.ASSIGNED_LOCAL), trk.get(trk.FEATURE_OUTLIER), trk.get(trk.LOCAL_POINT_IDS), trk.get(trk.LOCAL_FLAGS)
    rows = [stats(n[f], first_ids[f], a1[f], out[f], lid[f], lfl[f], max_local=trk.max_local) for f in range(trk.B)]
    return {key: np.stack([r[i] for r in rows]) for i, key in enumerate(STAT_KEYS)}


RELABEL = lambda a: np.where(a >= 0, 100 + a % 6, -1).astype(np.int32)      # onto the recent points of point_upkeep_inputs.cull_script()


def test_second_stage_and_point_stats_on_a_built_and_on_a_host_set_map(vo):
    """vo_tracker_track_local_map on the built map equals the stage on the model's map set from the host with the same link; the
    counters of both against the model; frame 0's row into vo_kfstore_add_point_stats_dev straight from the device"""
    import point_upkeep_inputs as ui
    import torch
    from test_gpu_point_upkeep import UDev
    imgs, raw, _, _, kfs, _ = _world(vo)
    store = _device_store(vo, kfs, mi.NK)
    snaps = []
    # ---- built
    a = _tracker(vo, ids="held")
    a.track_first(imgs[0], raw[0])
    a.results()
    s = _first_state(a)
    a.build_local_map(store)
    want = _compare_build(vo, a, s, MAX_LOCAL)
    assert all(np.array_equal(w[2], s["has"][f]) for f, w in enumerate(want))       # no orphan: the host form cannot null slots
    a.track_local_map()
    snaps.append(_snapshot(a))
    first = a.get(a.FIRST_SLOT_IDS)
    w_stats = _stats_want(a, first)
    a.point_stats()
    got = {key: a.get(getattr(a, key)) for key in STAT_KEYS}
    for key in STAT_KEYS:
        assert got[key].dtype == np.int32 and got[key].tobytes() == w_stats[key].tobytes(), key
    cap = a.cap
    assert got["STAT_FOUND"][:, :cap].sum() > 100 and got["STAT_FOUND"][:, cap:].sum() > 100 and (got["STAT_VISIBLE"] > got["STAT_FOUND"]).any()
    # ---- set from the host, under other labels
    b = _tracker(vo, ids="held", relabel=RELABEL)
    b.track_first(imgs[0], raw[0])
    b.results()
    _set_local(b, [w[3] for w in want], MAX_LOCAL, relabel=RELABEL)
    b.track_local_map()
    snaps.append(_snapshot(b))
    for key in snaps[0]:
        assert snaps[0][key].tobytes() == snaps[1][key].tobytes(), key
    assert (snaps[0]["n_matches_local"][:2] > 0).all()
    sb = _first_state(b)                                                               # (the state as it stands now: the same gather)
    first_b = np.stack([slot_ids(sb["n"][f], sb["has"][f], sb["a0"][f], sb["last_ids"][f]) for f in range(b.B)])
    w_stats = _stats_want(b, first_b)
    b.point_stats()
    got = {key: b.get(getattr(b, key)) for key in STAT_KEYS}
    for key in STAT_KEYS:
        assert got[key].tobytes() == w_stats[key].tobytes(), key
    assert set(np.unique(got["STAT_IDS"])) == {-1, 100, 101, 102, 103, 104, 105}
    # ---- frame 0's row into the store's counters: the device pointers against the downloaded row through the host form
    p_ids, p_vis, p_fnd, row = b.point_stats_arrays()
    assert row == cap + MAX_LOCAL and b.point_stats_arrays() == (p_ids, p_vis, p_fnd, row)
    stores = [UDev(vo, 7, ui.NK_HAND, ui.CAPS, max_recent=row) for _ in range(2)]     # (max_recent >= max_local: the call's bound)
    for d in stores:
        for step in ui.cull_script():
            d.step(step)
    before = stores[0].s.recent_points()
    vo.check(vo.lib().vo_kfstore_add_point_stats_dev(stores[0].s._h, row, C.c_void_p(p_ids), C.c_void_p(p_vis), C.c_void_p(p_fnd)),
             "vo_kfstore_add_point_stats_dev")
    stores[1].s.add_point_stats(got["STAT_IDS"][0], got["STAT_VISIBLE"][0], got["STAT_FOUND"][0])
    after = stores[0].s.recent_points()
    assert after == stores[1].s.recent_points() and after != before and [e[0] for e in after] == [e[0] for e in before]
    torch.cuda.synchronize()
    a.close(), b.close(), store.close()


def _pose_store(vo, kfs, unset=()):
    """the key-frames in a store with the mapping layer; key-frame k's pose is a small motion of its own, `unset` have none"""
    from vo_slam_test_amd import synth
    import point_upkeep_inputs as ui
    s = vo.KeyFrameStore(len(kfs), mi.NK)
    s.enable_connections(), s.enable_culling(), s.enable_mapping(ui.CAM6, ui.SF, 0)
    for k in kfs:
        n = len(k["ids"])
        s.insert(dict(angle=np.zeros(n, f32), desc=np.zeros((n, 32), np.uint8), nodes=np.zeros(n, np.int32), flags=k["flags"], points=k["points"],
                      ids=k["ids"], point_desc=k["point_desc"], min_dist=k["min_dist"], max_dist=k["max_dist"], bad=k["bad"]))
    for k in range(len(kfs)):
        if k not in unset:
            R, t = synth.se3_exp(np.array([0.01 * k, -0.02, 0.005 * k, 0.01, 0.002 * k, -0.01]))
            s.set_pose(k, np.concatenate([R.reshape(-1), t]))
    return s


def _poses(store, K):
    out = []
    for k in range(K):
        T, on = store.pose(k)
        out.append(np.array(T, np.float64) if on else None)
    return out


def test_ref_pose_recorded_and_refreshed(vo):
    """two frames.  REF_TCR / REF_KF against the model; dev_ref_kf entries of -1, out of range and without a pose keep the
    remembered key-frame; the lost stream's invalid last pose keeps its pair; a key-frame pose moved between the two calls moves
    the start pose and the temporary points of the next vo_tracker_begin_frame exactly as the model says"""
    import torch
    from vo_slam_test_amd import synth
    imgs, raw, _, _, kfs, _ = _world(vo)
    K, UNSET = len(kfs), 5
    store, poses_store = _device_store(vo, kfs, mi.NK), _pose_store(vo, kfs, unset=(UNSET,))
    trk = _tracker(vo)
    thd = th._median_depth(vo, "synth")
    hm, rp = HandoverModel(trk.B, trk.cap, trk.max_last, hi.CAM5[:4]), RefPoseModel(trk.B)
    hm.set_last_pose(trk.get(trk.TCW_START), np.ones(trk.B, np.uint8))
    for k in range(2):
        trk.track_first(imgs[k], raw[k])
        trk.build_local_map(store)
        trk.track_local_map()
        state, frame, res = th._state(trk, True)
        best = trk.get(trk.LOCAL_REF_KF)
        trk.end_frame(thd)
        e = th._read(trk, ("frame_pose", "velocity"))
        want_e = hm.end_frame(state, e["frame_pose"])
        assert e["velocity"].tobytes() == want_e["velocity"].tobytes()
        poses = _poses(poses_store, K)
        assert poses[UNSET] is None and all(p is not None for i, p in enumerate(poses) if i != UNSET)
        trk.record_ref_pose(poses_store)
        rp.record(e["frame_pose"], hm.last_valid, best, poses)
        assert trk.get(trk.REF_TCR).tobytes() == rp.tcr.tobytes() and trk.get(trk.REF_KF).tobytes() == rp.kf.tobytes(), k
        if k == 0:
            assert (rp.kf >= 0).all() and np.array_equal(rp.kf, best)
            kept = rp.kf.copy()
            trk.record_ref_pose(poses_store, torch.tensor([-1, K + 3, UNSET], dtype=torch.int32).cuda())    # all three keep the remembered one
            rp.record(e["frame_pose"], hm.last_valid, [-1, K + 3, UNSET], poses)
            assert np.array_equal(rp.kf, kept) and trk.get(trk.REF_KF).tobytes() == kept.tobytes() and trk.get(trk.REF_TCR).tobytes() == rp.tcr.tobytes()
            other = (int(kept[0]) + 1) % mi.KF_PER_STREAM                                                     # an explicit key-frame for frame 0
            trk.record_ref_pose(poses_store, torch.tensor([other, -1, -1], dtype=torch.int32).cuda())
            rp.record(e["frame_pose"], hm.last_valid, [other, -1, -1], poses)
            assert rp.kf[0] == other and trk.get(trk.REF_KF).tobytes() == rp.kf.tobytes() and trk.get(trk.REF_TCR).tobytes() == rp.tcr.tobytes()
        else:
            assert not hm.last_valid[hi.LOST] and best[hi.LOST] == -1 and rp.kf[hi.LOST] >= 0              # the lost stream keeps its pair
        # local BA moves the remembered key-frames between the two calls
        for kf in sorted(set(int(x) for x in rp.kf)):
            R, t = synth.se3_exp(np.array([0.004, -0.003, 0.002, 0.02, -0.01, 0.015]) * (kf + 1))
            poses_store.set_pose(kf, compose(np.concatenate([R.reshape(-1), t]), poses[kf]))
        poses = _poses(poses_store, K)
        last_before = hm.last_pose.copy()
        trk.refresh_last_pose(poses_store)
        hm.last_pose = rp.refresh(hm.last_pose, poses)
        assert np.abs(hm.last_pose - last_before).max() > 1e-3
        trk.begin_frame(thd)                                                                               # still accepted
        got_b = th._read(trk, th.LAST_KEYS + ("temp_count", "Tcw"))
        want_b = hm.begin_frame(frame, thd, None, state["local"]["ids"])
        th._same(got_b, want_b, th.LAST_KEYS + ("temp_count", "Tcw"), ("refresh", k))
        assert (want_b["temp_count"][:2] >= 1).all()
        with pytest.raises(vo.VoError, match="status -1"):
            trk.refresh_last_pose(poses_store)                                                             # behind begin_frame: refused
    trk.close(), store.close(), poses_store.close()


CHAIN_KEYS = th.LAST_KEYS + ("slot_ids", "velocity", "frame_pose", "temp_count", "Tcw", "pose_start", "link")


def _chain(vo, read):
    """four frames: begin_frame -> track_first_dev -> build_local_map -> track_local_map -> point_stats -> end_frame ->
    record_ref_pose -> refresh_last_pose.  read: every array is read after every call (synchronising), else frames 1 .. 3 are
    nothing but enqueues behind a device sleep"""
    import torch
    st = torch.cuda.Stream()
    imgs, raw, _, _, kfs, _ = _world(vo)
    store, poses_store = _device_store(vo, kfs, mi.NK), _pose_store(vo, kfs)
    trk = _tracker(vo, stream=st.cuda_stream)
    thd = th._median_depth(vo, "synth")
    t_img, t_raw = torch.from_numpy(imgs).cuda(), torch.from_numpy(raw.view(np.int16)).cuda()
    torch.cuda.synchronize()
    peek = lambda: (trk.results(), th._read(trk, CHAIN_KEYS), [trk.get(getattr(trk, key)) for key in STAT_KEYS + ("REF_TCR", "REF_KF", "FIRST_SLOT_IDS")])
    busy, built = None, False
    with torch.cuda.stream(st):
        for k in range(hi.N_STEPS):
            if k == 1 and not read:
                st.synchronize()
                torch.cuda._sleep(200_000_000)                                     # a tenth of a second of device time in front of the chain
            for name, call in (("begin", lambda: trk.begin_frame(thd)), ("first", lambda: trk.track_first_dev(t_img[k], t_raw[k])),
                               ("build", lambda: trk.build_local_map(store)), ("local", trk.track_local_map), ("stats", trk.point_stats),
                               ("end", lambda: trk.end_frame(thd)), ("record", lambda: trk.record_ref_pose(poses_store)),
                               ("refresh", lambda: trk.refresh_last_pose(poses_store))):
                if name == "begin" and k == 0:
                    continue
                call()
                built = built or name == "build"
                if read and built:
                    peek()                                                         # (every getter synchronises)
        busy = not st.query()
    st.synchronize()
    out = peek()
    trk.close(), store.close(), poses_store.close()
    return out + (busy,)


def test_chain_of_four_frames_enqueued_equals_the_chain_read_step_by_step(vo):
    res_a, last_a, more_a, _ = _chain(vo, read=True)
    res_b, last_b, more_b, busy = _chain(vo, read=False)
    assert busy                                                # frames 1 .. 3 were enqueued while the stream was still sleeping
    for k in res_a:
        assert res_a[k].tobytes() == res_b[k].tobytes(), k
    th._same(last_b, last_a, list(last_a), "chain")
    for x, y in zip(more_a, more_b):
        assert x.tobytes() == y.tobytes()
    assert not res_a["status"][:2].any() and (res_a["n_tracked"][:2] >= 30).all() and res_a["status"][hi.LOST] != 0
    assert more_a[2].sum() > 0 and (more_a[4][:2] >= 0).all()


def test_refusals_enqueue_and_change_nothing(vo):
    import torch
    st = torch.cuda.Stream()
    imgs, raw, _, _, kfs, _ = _world(vo)
    store, poses_store = _device_store(vo, kfs, mi.NK), _pose_store(vo, kfs)
    trk = _tracker(vo, ids=None, stream=st.cuda_stream)
    keys = ("LOCAL_POINT_IDS", "LOCAL_LINK", "LOCAL_MAP_FLAGS", "FEATURE_HAS_POINT", "LAST_FLAGS", "LAST_IDS", "TCW_START")
    block = STAT_KEYS + ("FIRST_SLOT_IDS", "REF_TCR", "REF_KF")

    def refused(call, with_block=False):
        st.synchronize()
        ks = keys + (block if with_block else ())
        before = {key: trk.get(getattr(trk, key)) for key in ks}
        with pytest.raises(vo.VoError, match="status -1"):
            call()
        assert st.query()                                      # nothing was enqueued
        for key in ks:
            assert trk.get(getattr(trk, key)).tobytes() == before[key].tobytes(), key
    trk.set_last_pose(trk.get(trk.TCW_START), np.ones(hi.B, np.uint8))                 # (the hand-over block: LAST_IDS reads)
    refused(lambda: trk.build_local_map(store))                                         # before any track
    trk.track_first(imgs[0], raw[0])
    refused(lambda: trk.build_local_map(store))                                         # no ids on the last list
    refused(trk.point_stats)
    _, _, maps, _, _, _ = _world(vo)
    n_last = max(len(m[1]["flags"]) for m in maps)
    trk.set_last_frame_ids(th._stack([m[1]["ids"] for m in maps], n_last, -1))
    _empty_local(trk)
    trk.track(imgs[0], raw[0])
    refused(lambda: trk.build_local_map(store))                                         # both stages in one call
    trk.track_first(imgs[0], raw[0])
    trk.results()
    s = _first_state(trk)
    trk.build_local_map(store)                                                          # the valid call gives the plain result
    want = _compare_build(vo, trk, s, MAX_LOCAL)
    refused(trk.point_stats, True)                                                      # before a local stage
    refused(lambda: trk.record_ref_pose(poses_store), True)                             # before end_frame
    refused(lambda: trk.refresh_last_pose(poses_store), True)
    trk.track_local_map()
    first = trk.get(trk.FIRST_SLOT_IDS)
    w_stats = _stats_want(trk, first)
    trk.point_stats()
    for key in STAT_KEYS:
        assert trk.get(getattr(trk, key)).tobytes() == w_stats[key].tobytes(), key
    trk.end_frame(2.0)
    refused(lambda: trk.record_ref_pose(store), True)                                   # a store without the mapping layer
    refused(lambda: trk.refresh_last_pose(store), True)
    trk.record_ref_pose(poses_store), trk.refresh_last_pose(poses_store), trk.begin_frame(2.0)      # the valid calls are accepted
    refused(lambda: trk.refresh_last_pose(poses_store), True)                           # behind begin_frame
    assert (trk.get(trk.REF_KF) >= 0).all()
    # point_stats behind a local stage of the split motion route, the local map without ids: the ids test refuses
    _empty_local(trk)
    trk.track_first(imgs[1], raw[1])
    trk.track_local_map()
    refused(trk.point_stats, True)
    # and with ids on both sides behind another route (both stages in one call)
    trk.set_local_map_ids(np.full((hi.B, 8), -1, np.int32))
    trk.track(imgs[1], raw[1])
    refused(trk.point_stats, True)
    _set_local(trk, [w[3] for w in want], MAX_LOCAL)                                    # the valid sequence is accepted afterwards
    trk.track_first(imgs[1], raw[1])
    trk.track_local_map()
    sb = _first_state(trk)
    w_stats = _stats_want(trk, np.stack([slot_ids(sb["n"][f], sb["has"][f], sb["a0"][f], sb["last_ids"][f]) for f in range(hi.B)]))
    trk.point_stats()
    for key in STAT_KEYS:
        assert trk.get(getattr(trk, key)).tobytes() == w_stats[key].tobytes(), key
    trk.close(), store.close(), poses_store.close()


def test_point_stats_needs_ids_and_the_split_motion_route(vo):
    imgs, raw, _, _, kfs, _ = _world(vo)
    store = _device_store(vo, kfs, mi.NK)
    trk = _tracker(vo)
    trk.track_first(imgs[0], raw[0])
    trk.results()
    s = _first_state(trk)
    locs = [_model_build(vo, s, MAX_LOCAL, f)[3] for f in range(trk.B)]
    B = trk.B
    _empty_local(trk)
    trk.track_local_map()
    with pytest.raises(vo.VoError, match="status -1"):
        trk.point_stats()                                                               # a local map without ids
    trk.track(imgs[0], raw[0])
    with pytest.raises(vo.VoError, match="status -1"):
        trk.point_stats()                                                               # both stages in one call: another route
    # and the valid sequence afterwards gives the model's rows
    trk.track_first(imgs[0], raw[0])
    _set_local(trk, locs, MAX_LOCAL)
    trk.track_local_map()
    sb = _first_state(trk)
    first = np.stack([slot_ids(sb["n"][f], sb["has"][f], sb["a0"][f], sb["last_ids"][f]) for f in range(B)])
    w_stats = _stats_want(trk, first)
    trk.point_stats()
    for key in STAT_KEYS:
        assert trk.get(getattr(trk, key)).tobytes() == w_stats[key].tobytes(), key
    trk.close(), store.close()
