"""vo_tracker_track_local_map behind a relocalisation (visualOdometry.cpp:61, :74, :82-83 -> :726-774, :287-310) against the
CPU model tests/reloc_local_ref.py, on three frames of the relocalisation fixture: one that relocalises, one whose only
candidate is unrelated (RELOC_FAILED) and one without candidates."""
import numpy as np
import pytest

import reloc_db_inputs
import reloc_inputs
import reloc_ref
from reloc_local_ref import local_map_after_reloc, make_local_map

pytestmark = pytest.mark.gpu

FRAMES = (1, 4, 5)   # of the fixture: success through the first top-up; every candidate fails; no candidates
W, H = reloc_inputs.W, reloc_inputs.H
ALL = lambda ids: np.ones(len(ids), bool)
HALF = lambda ids: np.asarray(ids) % 2 == 0
MAX_LOCAL = 1400


class _Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(vo, orc):
    fx = reloc_inputs.build(orc)
    c = _Ctx()
    c.fx = fx
    c.sub = sub_inputs(fx)
    c.imgs = np.ascontiguousarray(fx["imgs"][list(FRAMES)])
    c.raw = np.ascontiguousarray(fx["raw"][list(FRAMES)]).view(np.uint16)
    vd = fx["vocab"]
    c.voc = vo.Vocabulary(vd["L"], vd["child_start"], vd["children"], vd["node_desc"], vd["node_weight"], vd["word_id"])
    c.cache = {}
    yield c
    c.voc.close()


def _tracker(vo, c, mc=reloc_inputs.MAX_CAND):
    return vo.Tracker(len(FRAMES), c.fx["cam5"], None, W, H, max_last=8, max_local=MAX_LOCAL, inv_depth_scale=float(c.fx["inv"]),
                      max_reloc_candidates=mc, max_reloc_features=c.fx["nk"])


def _with_observed(k, observed):
    """bit 1 of the flags (observe_cnt_ > 0) as a function of the map point's id"""
    fl = np.asarray(k["flags"], np.uint8) & 1
    return dict(k, flags=(fl | (2 * (fl & np.asarray(observed(np.asarray(k["ids"], np.int64)), np.uint8)))).astype(np.uint8))


def _snapshot(trk):
    out = dict(trk.results())
    for key in ("ASSIGNED_LOCAL", "FEATURE_HAS_POINT", "FEATURE_OUTLIER", "RELOC_POINT_IDS", "RELOC_WINNER", "LOCAL_FLAGS", "LOCAL_U"):
        out[key] = trk.get(getattr(trk, key))
    pts = trk.get(trk.FEATURE_POINTS)
    out["FEATURE_POINTS"] = np.where(out["FEATURE_HAS_POINT"][..., None] != 0, pts, 0.0)
    return out


def _set_local(trk, local, with_ids=True):
    B, n = len(FRAMES), len(local["valid"])
    z = lambda a: np.concatenate([np.asarray(a)[None], np.zeros((B - 1,) + np.asarray(a).shape, np.asarray(a).dtype)])
    trk.set_local_map(z(local["points"]), z(local["normals"]), z(local["min_dist"]), z(local["max_dist"]), z(local["valid"]), z(local["desc"]))
    if with_ids:
        trk.set_local_map_ids(z(local["ids"]))
    return n


def _relocalize(vo, orc, c, trk, route, observed):
    """runs the relocalisation route on the batch -> the candidates of frame 0 as the device walked them (the model's input)"""
    import torch
    nk = c.fx["nk"]
    if route == "host":
        cl = [[_with_observed(k, observed) for k in reloc_db_inputs.dense_ids(cands)[0]] for cands in c.sub["candidates"]]
        trk.set_reloc_candidates(c.voc, cl)
        trk.relocalize(c.imgs, c.raw)
        return cl[0], None
    if route == "store":
        kfs, lists = reloc_db_inputs.keyframes(c.sub)
    else:
        kfs, lists = reloc_db_inputs.db_keyframes(orc, c.sub)
    kfs = [_with_observed(dict(k, ids=np.asarray(k["ids"], np.int64) + nk), observed) for k in kfs]   # (global ids away from 0)
    store = vo.KeyFrameStore(len(kfs), nk)
    for k in kfs:
        store.insert(k)
    if route == "store":
        stride = max(len(ls) for ls in lists)
        cand = np.full((len(lists), stride), -1, np.int32)
        for f, ls in enumerate(lists):
            cand[f, :len(ls)] = ls
        trk.relocalize_store(store, c.voc, torch.tensor([len(ls) for ls in lists], dtype=torch.int32).cuda(), torch.from_numpy(cand).cuda(),
                             c.imgs, c.raw)
        return [kfs[g] for g in lists[0]], store
    dbi = reloc_db_inputs.database(orc, c.sub, kfs, lists)
    words = [c.voc.transform(k["desc"])[:2] for k in kfs]
    db = vo.KeyFrameDatabase(dbi["n_words"], len(kfs), nk, len(FRAMES))
    for w, v in vo.bow_vector([w for w, _ in words], [v for _, v in words]):
        db.insert(w, v)
    db.set_neighbors_batch(0, dbi["neighbors"])
    trk.relocalize_db(db, store, c.voc, c.imgs, c.raw)
    trk.sync()
    walked = trk.get(trk.RELOC_CANDIDATES)[0]
    return [kfs[g] for g in walked[walked >= 0]], (store, db)


def _case(vo, orc, c, route, observed, mc=reloc_inputs.MAX_CAND):
    key = (route, observed is ALL)
    if key in c.cache:
        return c.cache[key]
    trk = _tracker(vo, c, mc)
    cands, keep = _relocalize(vo, orc, c, trk, route, observed)
    before = _snapshot(trk)
    fr = c.sub["frames"][0]
    end = reloc_ref.relocalize(orc, fr[0], fr[1], fr[2], fr[3], fr[4], c.sub["fnodes"][0], cands, c.fx["cam5"], c.fx["sf"])
    n = len(fr[0])
    assert end["winner"] >= 0 and before["RELOC_WINNER"][0] == end["winner"] and np.array_equal(before["RELOC_POINT_IDS"][0, :n], end["ids"])
    local = make_local_map(fr, end, c.fx["cam5"])
    obs_of = {}
    for k in cands:
        for i, fl in zip(np.asarray(k["ids"], np.int64), np.asarray(k["flags"])):
            if fl & 1:
                obs_of[int(i)] = bool(fl & 2)
    want = local_map_after_reloc(orc, fr, end, lambda ids: np.array([obs_of[int(i)] for i in ids], bool), local, c.fx["cam5"], c.fx["sf"])
    _set_local(trk, local)
    trk.track_local_map(th_radius=5.0)
    got = _snapshot(trk)
    trk.close()
    c.cache[key] = (got, want, before, local, n)
    return c.cache[key]


def _check(got, want, before, n):
    """frame 0 against the model; frames 1 and 2 (RELOC_FAILED) untouched"""
    assert np.array_equal(got["ASSIGNED_LOCAL"][0, :n], want["assigned_local"])
    assert got["n_matches_local"][0] == want["n_local"] and got["n_inliers"][0] == want["inliers"] and got["n_tracked"][0] == want["n_tracked"]
    assert np.abs(got["pose"][0] - want["pose"]).max() < 1e-9
    assert np.array_equal(got["FEATURE_OUTLIER"][0, :n], want["outlier"]) and np.array_equal(got["FEATURE_HAS_POINT"][0, :n] != 0, want["has"])
    assert np.array_equal(got["RELOC_POINT_IDS"][0, :n], want["ids"])
    assert got["status"][0] == 0 and got["n_matches_last"][0] == before["n_matches_last"][0]
    assert (before["status"][1:] & 4).all()
    for key in got:
        assert np.array_equal(got[key][1:], before[key][1:]), key
    assert (got["n_matches_local"][1:] == 0).all()


def test_device_against_the_model_after_relocalize_store(vo, orc, ctx):
    got, want, before, local, n = _case(vo, orc, ctx, "store", ALL)
    assert want["n_skipped"] >= 20 and want["n_searched"] >= 20   # the skip and the search both act
    assert want["n_local"] > 0 and want["n_tracked"] <= want["inliers"]
    _check(got, want, before, n)


@pytest.mark.parametrize("route", ["host", "db"])
def test_the_same_after_relocalize_and_relocalize_db(vo, orc, ctx, route):
    got, want, before, local, n = _case(vo, orc, ctx, route, ALL, mc=reloc_inputs.MAX_CAND if route == "host" else 4)
    assert want["n_skipped"] >= 20 and want["n_searched"] >= 20
    _check(got, want, before, n)


def test_occupied_uses_bit_1(vo, orc, ctx):
    """bit 1 cleared on half of the winner's features: slots whose point has no observations can be claimed"""
    got, want, before, local, n = _case(vo, orc, ctx, "store", HALF)
    _check(got, want, before, n)
    full = _case(vo, orc, ctx, "store", ALL)[0]
    assert not np.array_equal(got["ASSIGNED_LOCAL"][0], full["ASSIGNED_LOCAL"][0])   # else the case shows nothing


def test_argument_errors_then_a_valid_sequence(vo, orc, ctx):
    c = ctx
    want_got, want, before, local, n = _case(vo, orc, c, "store", ALL)
    trk = _tracker(vo, c)
    cands, keep = _relocalize(vo, orc, c, trk, "store", ALL)
    with pytest.raises(vo.VoError, match="status -1"):
        trk.track_local_map(th_radius=5.0)          # no local map set
    _set_local(trk, local, with_ids=False)
    with pytest.raises(vo.VoError, match="status -1"):
        trk.set_local_map_ids(np.zeros((len(FRAMES), len(local["valid"]) - 1), np.int32))   # another n than the local map's
    _set_local(trk, local)
    trk.track_local_map(th_radius=5.0)
    got = _snapshot(trk)
    for key in got:
        assert np.array_equal(got[key], want_got[key]), key
    trk.close()


# ---------------------------------------------------------------------------------------------------------------------
# Relocalise from the store, then vo_tracker_track_local_map, after a rigid change of the world frame (tests/gauge.py): the
# key-frames' points and the local map go to G P / R_G n.  The fixture's true pose is the identity, so the PnP pose that the
# route turns into its se3 on the device (se3_log_from_R in reloc.hip) and every pose after it sit next to G^-1.  The PnP
# step reads the points as float32, whose rounding is not carried along by G: the gauges agree to that rounding at the PnP
# pose, and to the solver's round-off only once the pose-only solve has converged on the double points.
GAUGE_POSE_TOL = 2.05e-7


def sub_inputs(fx):
    return dict(fx, frames=[fx["frames"][f] for f in FRAMES], fnodes=[fx["fnodes"][f] for f in FRAMES],
                candidates=[fx["candidates"][1], fx["candidates"][4][:1], []])


def gauged_model(orc, fx, sub, G, end0=None):
    """the store's key-frames in the gauge G and the CPU model of frame 0 on them -> (kfs, lists, end, local, want); the local
    map is the one make_local_map builds around the identity-gauge result (end0; this call's own where None), moved by G"""
    import gauge
    nk = fx["nk"]
    kfs, lists = reloc_db_inputs.keyframes(sub)
    kfs = [_with_observed(dict(k, ids=np.asarray(k["ids"], np.int64) + nk, points=gauge.points(G, k["points"])), ALL) for k in kfs]
    cands = [kfs[g] for g in lists[0]]
    fr = sub["frames"][0]
    end = reloc_ref.relocalize(orc, fr[0], fr[1], fr[2], fr[3], fr[4], sub["fnodes"][0], cands, fx["cam5"], fx["sf"])
    local = make_local_map(fr, end if end0 is None else end0, fx["cam5"])
    local = dict(local, points=gauge.points(G, local["points"]), normals=gauge.directions(G, local["normals"]))
    obs_of = {}
    for k in cands:
        for i, fl in zip(np.asarray(k["ids"], np.int64), np.asarray(k["flags"])):
            if fl & 1:
                obs_of[int(i)] = bool(fl & 2)
    want = local_map_after_reloc(orc, fr, end, lambda ids: np.array([obs_of[int(i)] for i in ids], bool), local, fx["cam5"], fx["sf"])
    return kfs, lists, end, local, want


MODEL_SAME = ("assigned_local", "n_local", "inliers", "n_tracked", "outlier", "ids", "has")


@pytest.mark.parametrize("name", ["skew_2.6_w_negative", "skew_2.4_w_positive", "y_pi_minus_0.02"])
def test_relocalize_store_and_local_map_in_a_rotated_world_frame(vo, orc, ctx, name):
    """1. Device against the model in the new gauge as test_device_against_the_model_after_relocalize_store: the winner, the
    ids after the walk, the local-map assignments, counts and outlier flags equal, the pose within 1e-9 (as (R, t)).  The
    model takes its se3 of the PnP pose from synth.se3_log (scipy), the device from se3_log_from_R; a start pose whose
    translation part is off changes the iterates of the solves that follow far beyond 1e-9.
    2. Against the identity gauge: the same winner, ids, assignments, counts and flags; poses mapped back through G within
    GAUGE_POSE_TOL = 2.05e-7, ten times the worst deviation of the corrected model between the gauges on this frame,
    2.05e-8, measured on the CPU.  It is that large because PnP reads float32 points and the solves
    behind it stop at Ceres' relative function tolerance of 1e-6, a few 1e-8 short of the common minimum."""
    import torch
    import gauge
    from vo_slam_test_amd import synth
    c = ctx
    G = gauge.GAUGES[name]
    got0, want0, before0, local0, n = _case(vo, orc, c, "store", ALL)
    if "gauge_end0" not in c.cache:
        c.cache["gauge_end0"] = gauged_model(orc, c.fx, c.sub, gauge.IDENTITY)[2]
    end0 = c.cache["gauge_end0"]
    kfs, lists, end, local, want = gauged_model(orc, c.fx, c.sub, G, end0)
    trk = _tracker(vo, c)
    store = vo.KeyFrameStore(len(kfs), c.fx["nk"])
    for k in kfs:
        store.insert(k)
    stride = max(len(ls) for ls in lists)
    cand = np.full((len(lists), stride), -1, np.int32)
    for f, ls in enumerate(lists):
        cand[f, :len(ls)] = ls
    trk.relocalize_store(store, c.voc, torch.tensor([len(ls) for ls in lists], dtype=torch.int32).cuda(), torch.from_numpy(cand).cuda(), c.imgs, c.raw)
    before = _snapshot(trk)
    assert end["winner"] >= 0 and before["RELOC_WINNER"][0] == end["winner"] and np.array_equal(before["RELOC_POINT_IDS"][0, :n], end["ids"])
    assert gauge.pose_distance(synth.se3_exp(before["pose"][0]), synth.se3_exp(end["pose"])) < 1e-9
    assert gauge.quat_w_sign(synth.se3_exp(end["pose"])[0]) == (1 if "positive" in name else -1)
    _set_local(trk, local)
    trk.track_local_map(th_radius=5.0)
    got = _snapshot(trk)
    trk.close(), store.close()
    # 1. device against the model, this gauge
    assert np.array_equal(got["ASSIGNED_LOCAL"][0, :n], want["assigned_local"])
    assert got["n_matches_local"][0] == want["n_local"] and got["n_inliers"][0] == want["inliers"] and got["n_tracked"][0] == want["n_tracked"]
    assert gauge.pose_distance(synth.se3_exp(got["pose"][0]), synth.se3_exp(want["pose"])) < 1e-9
    assert np.array_equal(got["FEATURE_OUTLIER"][0, :n], want["outlier"]) and np.array_equal(got["FEATURE_HAS_POINT"][0, :n] != 0, want["has"])
    assert np.array_equal(got["RELOC_POINT_IDS"][0, :n], want["ids"])
    assert got["status"][0] == 0 and (before["status"][1:] & 4).all()
    # 2. against the identity gauge
    assert end["winner"] == end0["winner"] and np.array_equal(end["ids"], end0["ids"]) and np.array_equal(end["outlier"], end0["outlier"])
    for key in MODEL_SAME:
        assert np.array_equal(want[key], want0[key]), key
    for key in ("ASSIGNED_LOCAL", "FEATURE_HAS_POINT", "FEATURE_OUTLIER", "RELOC_POINT_IDS", "RELOC_WINNER", "n_tracked", "n_inliers",
                "n_matches_last", "n_matches_local", "status"):
        assert np.array_equal(got[key], got0[key]), key
    for label, a, b in (("after the walk", before, before0), ("after the local map", got, got0)):
        d = gauge.pose_distance(gauge.pose6_back(G, a["pose"][0]), synth.se3_exp(b["pose"][0]))
        print(f"{name} {label}: rotated gauge mapped back - identity gauge {d:.3g}")
        assert d < GAUGE_POSE_TOL, (label, d)


# ---------------------------------------------------------------------------------------------------------------------
# The se3 that the route takes from the PnP pose on the device (se3_log_from_R in reloc.hip), read directly: a candidate
# that PnP rejects with fewer than ten inliers leaves that se3 in the frame's pose (visualOdometry.cpp:808-825 write the
# pose back before the count is tested), nothing runs behind it, and vo_tracker_results hands it out.
def bow_matches(orc, fr, fnode, kf):
    """searchByBoW(key-frame, frame) of the route on the oracle -> per frame feature the key-frame feature, or -1"""
    import ctypes as C
    k, d, ux, uy, ur = fr[:5]
    n, nk = len(k), len(kf["flags"])
    of = orc.FrameData(ux, uy, k["octave"], k["angle"], ur, d)
    okf = orc.FrameData(np.zeros(nk, np.float32), np.zeros(nk, np.float32), np.zeros(nk, np.int32), np.ascontiguousarray(kf["angle"], np.float32),
                        np.full(nk, -1, np.float32), np.ascontiguousarray(kf["desc"]))
    ba, bb = orc.BowData(kf["nodes"]), orc.BowData(fnode)
    m = np.full(n, -1, np.int32)
    orc.lib().orc_match_bow(C.byref(okf.c), (np.asarray(kf["flags"]) & 1).astype(np.uint8), C.byref(ba.c), C.byref(of.c), np.ones(n, np.uint8),
                            C.byref(bb.c), 0, 0.75, 1, m)
    return m


def rejected_by_pnp(orc, fx, sub, seed=2, n_good=9, n_junk=10):
    """frame 0's winning key-frame cut down to n_good features that PnP keeps and n_junk whose points are moved by 0.3 .. 1 m:
    enough BoW matches for PnP to run (>= 15), fewer than ten PnP inliers"""
    fr, kf = sub["frames"][0], sub["candidates"][0][1]
    full = reloc_ref.relocalize(orc, fr[0], fr[1], fr[2], fr[3], fr[4], sub["fnodes"][0], [kf], fx["cam5"], fx["sf"])
    src, mask = full["pnp_problems"][0]
    m = bow_matches(orc, fr, sub["fnodes"][0], kf)
    rng = np.random.default_rng(seed)
    good = rng.choice(m[src[mask]], n_good, replace=False)
    junk = np.setdiff1d(rng.choice(m[src], n_junk, replace=False), good)
    fl = np.zeros_like(kf["flags"])
    fl[good], fl[junk] = np.asarray(kf["flags"])[good], np.asarray(kf["flags"])[junk]
    pts = np.asarray(kf["points"], np.float64).copy()
    pts[junk] += rng.uniform(0.3, 1.0, (len(junk), 3)) * rng.choice([-1, 1], (len(junk), 3))
    return dict(kf, flags=fl, points=pts)


def pnp_gauges():
    """name -> (G, sign of w of the PnP pose; 0: the PnP pose lies within its own error, 1e-7, of the tr = 0 switch, so either
    branch and sign may come out -- in the model the two cases take one each): the three gauges of tests/gauge.py, and four that put the camera (true pose:
    the identity) onto poses of the se3_ref grid -- either side of the tr = 0 switch about -x, 3.0 rad about an axis led by
    -z, 1e-7 short of pi about -y"""
    import gauge
    import se3_ref as ref
    th = 2 * ref.PI / 3
    grid = lambda angle, axis: [(c["R"], c["t"]) for c in ref.cases() if c["th"] == angle and c["axis"] == axis and c["tn"] == 0.3][0]
    out = {"skew_2.6_w_negative": (gauge.GAUGES["skew_2.6_w_negative"], -1), "skew_2.4_w_positive": (gauge.GAUGES["skew_2.4_w_positive"], 1),
           "y_pi_minus_0.02": (gauge.GAUGES["y_pi_minus_0.02"], -1)}
    for name, pose, w in (("grid_beyond_tr_switch", grid(th + 1e-9, 3), 0), ("grid_before_tr_switch", grid(th - 1e-9, 3), 0),
                          ("grid_3.0", grid(3.0, 8), -1), ("grid_pi", grid(ref.PI - 1e-7, 4), -1)):
        out[name] = (gauge.from_Tcw(pose, gauge.IDENTITY), w)
    return out


@pytest.mark.parametrize("name", ["skew_2.6_w_negative", "skew_2.4_w_positive", "y_pi_minus_0.02", "grid_beyond_tr_switch",
                                  "grid_before_tr_switch", "grid_3.0", "grid_pi"])
def test_pnp_pose_of_a_rejected_candidate_against_mpmath(vo, orc, ctx, name):
    """The frame's only candidate gets 9 PnP inliers (outcome 2), so results()["pose"] is the device's se3 of the PnP pose.
    It is compared with the mpmath logarithm of the Tcw that the library's PnP (vo_pnp_ransac on the route's
    correspondences, as tests/test_gpu_reloc.py takes it) returns, within 1e-12, the log bound of tests/test_se3_ref.py; and
    with the model's (scipy logarithm of tests/pnp_ref.py's pose) within 1e-9 as (R, t).  Four of the seven cases have
    w < 0 out of the matrix -> quaternion step for certain, one w > 0 beyond 120 degrees, two sit on the tr = 0 switch."""
    import torch
    import gauge
    import se3_ref as ref
    from vo_slam_test_amd import synth
    c = ctx
    G, w = pnp_gauges()[name]
    if "rejected" not in c.cache:
        c.cache["rejected"] = rejected_by_pnp(orc, c.fx, c.sub)
    kf = _with_observed(dict(c.cache["rejected"], points=gauge.points(G, c.cache["rejected"]["points"])), ALL)
    fr = c.sub["frames"][0]
    model = reloc_ref.relocalize(orc, fr[0], fr[1], fr[2], fr[3], fr[4], c.sub["fnodes"][0], [kf], c.fx["cam5"], c.fx["sf"])
    assert model["trace"][0] == ["few_pnp_leak"] and model["bow"][0] >= 15 and 1 <= model["pnp"][0] <= 9
    trk = _tracker(vo, c)
    store = vo.KeyFrameStore(1, c.fx["nk"])
    store.insert(kf)
    cand = np.array([[0], [-1], [-1]], np.int32)
    trk.relocalize_store(store, c.voc, torch.tensor([1, 0, 0], dtype=torch.int32).cuda(), torch.from_numpy(cand).cuda(), c.imgs, c.raw)
    res = trk.results()
    npnp, code = trk.get(trk.RELOC_PNP_INLIERS)[0, 0], trk.get(trk.RELOC_OUTCOME)[0, 0]
    trk.close(), store.close()
    assert npnp == model["pnp"][0] and code == 2 and res["status"][0] & 4
    src, mask = model["pnp_problems"][0]
    m = bow_matches(orc, fr, c.sub["fnodes"][0], kf)
    p3 = np.asarray(kf["points"])[m[src]].astype(np.float32)
    p2 = np.stack([fr[2][src], fr[3][src]], 1).astype(np.float32)
    pnp = vo.pnp_ransac([(p3, p2)], np.asarray(c.fx["cam5"], np.float32)[:4])
    assert pnp["status"][0] == 1 and pnp["n_inliers"][0] == npnp
    T = pnp["Tcw"][0]
    assert w == 0 or gauge.quat_w_sign(T[:, :3]) == w
    e = ref.err(res["pose"][0], ref.log(T[:, :3], T[:, 3]))
    print(f"{name}: w {gauge.quat_w_sign(T[:, :3]):+.0f}, tr {np.trace(T[:, :3]):+.3g}, {npnp} PnP inliers, device se3 of the PnP pose - mpmath {e:.3g}")
    assert e < 1e-12, e
    assert gauge.pose_distance(synth.se3_exp(res["pose"][0]), synth.se3_exp(model["pose"])) < 1e-9
