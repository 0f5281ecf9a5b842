"""The model of vo_tracker_end_frame_store / vo_tracker_point_stats_store (tests/handover_store_ref.py) on hand-written tables,
and the two chains of tests/test_gpu_handover_store.py under the CPU oracle with the model between the steps: the oracle's
relocalisation + local map (tests/reloc_local_ref.py) and its trackRefKeyFrame + local map (tests/track_ref.py) are handed over
by the model, and the same image is tracked again by the oracle's motion route against the handed-over list.  The camera does
not move, so the start pose VELOCITY * last pose with the identity VELOCITY of an invalid last pose is the frame's own."""
import numpy as np
import pytest

import handover_store_ref as hs
from handover_ref import IDENTITY, HandoverModel

f32 = np.float32
CAM4 = [500.0, 500.0, 320.0, 240.0]
D = lambda k, i: np.full(32, 16 * k + i + 1, np.uint8)      # key-frame k's copy of feature i's point descriptor
STORE = [dict(ids=[10, 11, 12, 13], flags=[3, 3, 1, 3], point_desc=[D(0, i) for i in range(4)]),
         dict(ids=[11, 20, 21, 13], flags=[3, 3, 3, 0], point_desc=[D(1, i) for i in range(4)]),
         dict(ids=[30, 10], flags=[3, 3], point_desc=[D(2, i) for i in range(2)])]
SIZE = 2                                                       # key-frame 2 lies beyond the store's size
POSE = np.tile(IDENTITY, (2, 1))


def _state(**kw):
    """two frames of 8 slots (n = 7) -> the state end_state takes; every slot observed, no outlier, unless given"""
    B, cap = 2, 8
    s = dict(n=[7, 7], has_point=np.zeros((B, cap), np.uint8), assigned_local=np.full((B, cap), -1, np.int32), observed=np.ones((B, cap), np.uint8),
             outlier=np.zeros((B, cap), np.uint8), points=np.arange(B * cap * 3, dtype=np.float64).reshape(B, cap, 3) + 1,
             octave=np.tile(np.arange(cap, dtype=np.int32) % 4, (B, 1)), angle=np.tile(np.arange(cap, dtype=f32), (B, 1)), status=[0, 0],
             n_tracked=[40, 40], local_ids=np.tile(np.array([21, 20, 10], np.int32), (B, 1)))
    s.update({k: np.array(v) for k, v in kw.items()})
    return s


def _reloc_table():
    #                    0 kept | 1 claimed | 2 outlier | 3 unobserved | 4 held beyond size | 5 null | 6 no id | 7 beyond n
    fid = np.array([[10, 20, 11, 12, 30, 99, -1, 10]] * 2, np.int32)
    has = np.array([[1, 1, 1, 1, 1, 0, 1, 1]] * 2, np.uint8)
    a1 = np.array([[-1, 1, -1, -1, -1, -1, -1, -1]] * 2, np.int32)
    obs = np.array([[1, 1, 1, 0, 1, 1, 1, 1]] * 2, np.uint8)
    out = np.array([[0, 0, 1, 0, 0, 0, 0, 0]] * 2, np.uint8)
    return _state(frame_ids=fid, has_point=has, assigned_local=a1, observed=obs, outlier=out, winner=[0, -1], status=[0, 4])


def test_relocalisation_slots_by_hand():
    s = _reloc_table()
    m = HandoverModel(2, 8, 8, CAM4)
    e = hs.end_frame(m, hs.ROUTE_RELOC, s, STORE, POSE, size=SIZE)
    assert e["slot_ids"][0].tolist() == [10, 20, 11, -1, -1, -1, -1, -1]
    assert e["last_flags"][0].tolist() == [3, 3, 2, 0, 0, 0, 0, 0]
    assert np.array_equal(e["slot_desc"][0][0], D(0, 0)) and np.array_equal(e["slot_desc"][0][1], D(1, 1))
    assert np.array_equal(e["slot_desc"][0][2], D(0, 1))                  # two holders with different copies: the lowest key wins
    assert not e["slot_desc"][0][3:].any()
    assert np.array_equal(e["last_points"][0][:3], s["points"][0][:3]) and not e["last_points"][0][3:].any()
    assert e["last_ids"][0].tolist() == [10, 20, 11, -1, -1, -1, -1, -1] and e["last_octave"][0].tolist() == [0, 1, 2, 3, 0, 1, 2, 0]
    # a failed relocalisation: every slot null, an empty list, the last pose invalid, no motion
    assert (e["slot_ids"][1] == -1).all() and not e["last_flags"][1].any() and not e["slot_desc"][1].any()
    assert m.last_valid.tolist() == [1, 0] and e["motion_state"].tolist() == [0, 0] and np.array_equal(e["velocity"][1], IDENTITY)
    # with the whole store in reach, id 30 is held (key-frame 2) and id 10's first key is still key-frame 0's
    e = hs.end_frame(HandoverModel(2, 8, 8, CAM4), hs.ROUTE_RELOC, s, STORE, POSE)
    assert e["slot_ids"][0].tolist() == [10, 20, 11, -1, 30, -1, -1, -1] and np.array_equal(e["slot_desc"][0][4], D(2, 0))
    assert np.array_equal(e["slot_desc"][0][0], D(0, 0))
    # a valid last pose and a good frame: the motion is on; min_tracked above the count turns it off
    for mt, state in ((0, 1), (50, 0)):
        m = HandoverModel(2, 8, 8, CAM4)
        m.set_last_pose(POSE, [1, 1])
        assert hs.end_frame(m, hs.ROUTE_RELOC, s, STORE, POSE, min_tracked=mt, size=SIZE)["motion_state"].tolist() == [state, 0]


def test_first_key_ignores_a_feature_without_bit_0():
    assert hs.first_holder(STORE, 13, SIZE) == (0, 3) and hs.first_holder(STORE, 12, SIZE) == (0, 2)
    assert hs.first_holder(STORE, 30, SIZE) is None and hs.first_holder(STORE, 30) == (2, 0) and hs.first_holder(STORE, 99) is None
    assert hs.first_holder([dict(ids=[13], flags=[2], point_desc=[D(0, 0)])] + STORE, 13) == (1, 3)


def test_reference_keyframe_slots_by_hand():
    #                 0 kept | 1 claimed | 2 a0 beyond the count | 3 culled by the first solve | 4 kept, outlier | 5 none | 6 claimed over a match
    a0 = np.array([[0, -1, 5, 1, 3, -1, 2, 0]] * 2, np.int32)
    has = np.array([[1, 1, 1, 0, 1, 0, 1, 1]] * 2, np.uint8)
    a1 = np.array([[-1, 1, -1, -1, -1, -1, 0, -1]] * 2, np.int32)
    out = np.array([[0, 0, 0, 0, 1, 0, 0, 0]] * 2, np.uint8)
    s = _state(assigned_last=a0, has_point=has, assigned_local=a1, outlier=out, ref_kf=[0, 7])
    e = hs.end_frame(HandoverModel(2, 8, 8, CAM4), hs.ROUTE_REF, s, STORE, POSE, size=SIZE)
    assert e["slot_ids"][0].tolist() == [10, 20, -1, -1, 13, -1, 21, -1] and e["last_flags"][0].tolist() == [3, 3, 0, 0, 2, 0, 3, 0]
    assert np.array_equal(e["slot_desc"][0][4], D(0, 3)) and np.array_equal(e["slot_desc"][0][6], D(1, 2))
    # ref_kf out of range: only the local search's claims are left
    assert e["slot_ids"][1].tolist() == [-1, 20, -1, -1, -1, -1, 21, -1] and e["motion_state"].tolist() == [0, 0] and m_valid(e)
    k0 = hs.kept_ids(hs.ROUTE_REF, 7, has[0], STORE, SIZE, assigned_last=a0[0], ref_kf=0)
    assert k0.tolist() == [10, -1, -1, -1, 13, -1, 12, -1]
    assert hs.kept_ids(hs.ROUTE_REF, 7, has[0], STORE, SIZE, assigned_last=a0[0], ref_kf=2).tolist() == [-1] * 8      # beyond size
    ids, vis, fnd = hs.stats_rows(hs.ROUTE_REF, 7, k0, a1[0], out[0], [21, 20, 10], [1, 1, 0], 3)
    assert ids.tolist() == [10, -1, -1, -1, 13, -1, -1, -1, 21, 20, -1]
    assert vis.tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0] and fnd.tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0]


def m_valid(e):
    return e["last_n"].tolist() == [8]


def test_stat_rows_by_hand():
    s = _reloc_table()
    kept = hs.kept_ids(hs.ROUTE_RELOC, 7, s["has_point"][0], STORE, SIZE, frame_ids=s["frame_ids"][0])
    assert kept.tolist() == [10, 20, 11, 12, 30, -1, -1, -1]
    # local point 2 carries id 10, which slot 0 holds: skipped by id, not visible; local point 1 was claimed by slot 1
    ids, vis, fnd = hs.stats_rows(hs.ROUTE_RELOC, 7, kept, s["assigned_local"][0], s["outlier"][0], [21, 20, 10], [1, 1, 0], 3)
    assert ids.tolist() == [10, -1, 11, 12, 30, -1, -1, -1, 21, 20, -1]
    assert vis.tolist() == [1, 0, 1, 1, 1, 0, 0, 0, 1, 1, 0] and fnd.tolist() == [1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0]
    ids, vis, fnd = hs.stats_rows(hs.ROUTE_RELOC, 7, kept, s["assigned_local"][1], s["outlier"][1], [21, 20, 10], [1, 1, 0], 3, failed=True)
    assert (ids == -1).all() and not vis.any() and not fnd.any() and len(ids) == 11
    assert hs.kept_ids(hs.ROUTE_RELOC, 7, s["has_point"][1], STORE, SIZE, frame_ids=s["frame_ids"][1], failed=True).tolist() == [-1] * 8


# ------------------------------------------------------------------------------------------------------- the oracle continuation
MAX_LOCAL = 3000
RELOC_FRAME = 0     # of tests/reloc_inputs.py: relocalises straight after the first solve
REF_FRAME = 0       # of tests/test_gpu_ref_keyframe_store.py: the frame whose reference key-frame shares its features


def _kf(k, **kw):
    P = np.asarray(k["points"], np.float64)
    out = dict(bad=False, neighbors=[], children=[], parent=-1, normals=P / np.maximum(np.linalg.norm(P, axis=1, keepdims=True), 1e-9))
    out.update(k)
    out.update(kw)
    return out


def _motion_step(orc, fr, e, store_kfs, cam5, sf, W=640, H=480):
    """the frame tracked again by the oracle's motion route against the list the model handed over: track_first, the local map
    built from the last ids (tests/motion_store_ref.py), the local stage -> (status, n_tracked)"""
    import motion_store_inputs as mi
    from motion_store_ref import build, link
    from track_ref import local_map_stage, track_first
    from vo_slam_test_amd import synth
    k, d, ux, uy, ur, dep = fr
    n = len(k)
    last = {key: e["last_" + key][0][:n] for key in ("points", "flags", "octave", "angle", "desc", "ids")}
    T = e["frame_pose"][0]                                   # VELOCITY = identity: the start pose is the last pose
    assert np.array_equal(e["velocity"][0], IDENTITY)
    s1 = track_first(orc, k, d, ux, uy, ur, T, synth.se3_log(T[:9].reshape(3, 3), T[9:]), last, cam5, sf, W, H)
    w, first_ids, has = build(n, s1["has"], s1["assigned_last"], last["ids"], mi.model_store(store_kfs), MAX_LOCAL)
    fobs = np.where(has != 0, s1["fobs"], 0).astype(np.uint8)
    loc = mi.local_map(w, store_kfs, MAX_LOCAL)
    loc["link"] = link(last["flags"], last["ids"], loc["ids"])
    s2 = local_map_stage(orc, s1["of"], k, ux, uy, ur, s1["fpt"], has.astype(bool), fobs, s1["pose_1"], s1["assigned_last"], s1["n_last_list"],
                         loc, cam5, sf, W, H, 3.0, 0.8, s1["solve"])
    return s1["status"], s2["n_tracked"], int((first_ids >= 0).sum())


def reloc_chain(orc):
    """-> (status, n_tracked, handed-over ids) of the motion step behind relocalise -> local map -> the model's hand-over"""
    import reloc_inputs
    import reloc_ref
    from reloc_local_ref import local_map_after_reloc, make_local_map
    fx = reloc_inputs.build(orc, n_frames=RELOC_FRAME + 1)
    fr = fx["frames"][RELOC_FRAME]
    k = fr[0]
    n = len(k)
    cands = fx["candidates"][RELOC_FRAME]
    end = reloc_ref.relocalize(orc, fr[0], fr[1], fr[2], fr[3], fr[4], fx["fnodes"][RELOC_FRAME], cands, fx["cam5"], fx["sf"])
    assert end["winner"] >= 0
    local = make_local_map(fr, end, fx["cam5"])
    got = local_map_after_reloc(orc, fr, end, lambda ids: np.ones(len(ids), bool), local, fx["cam5"], fx["sf"])
    # the store: the candidates (every held point observed) and the local map as one more key-frame
    kfs = [_kf(c, flags=(np.asarray(c["flags"], np.uint8) & 1) * 3) for c in cands]
    kfs.append(_kf(dict(ids=np.asarray(local["ids"], np.int32), flags=np.asarray(local["valid"], np.uint8), points=local["points"],
                        normals=local["normals"], min_dist=local["min_dist"], max_dist=local["max_dist"], point_desc=local["desc"])))
    s = dict(n=[n], has_point=got["has"].astype(np.uint8)[None], assigned_local=got["assigned_local"][None], observed=got["has"].astype(np.uint8)[None],
             outlier=got["outlier"][None], points=got["points"][None], octave=k["octave"].astype(np.int32)[None], angle=k["angle"].astype(f32)[None],
             status=[0], n_tracked=[got["n_tracked"]], local_ids=np.asarray(local["ids"], np.int32)[None], frame_ids=got["ids"].astype(np.int32)[None],
             winner=[end["winner"]])
    return _hand_over_and_track(orc, fr, hs.ROUTE_RELOC, s, kfs, got["pose"], fx["cam5"], fx["sf"])


def _hand_over_and_track(orc, fr, route, s, kfs, pose6, cam5, sf):
    from vo_slam_test_amd import synth
    n = len(fr[0])
    R, t = synth.se3_exp(np.asarray(pose6, np.float64))
    m = HandoverModel(1, n, n, [float(c) for c in cam5[:4]])       # (no last pose: VELOCITY is the identity)
    e = hs.end_frame(m, route, s, kfs, [np.concatenate([R.reshape(-1), t])], min_tracked=50)
    assert m.last_valid[0] == 1 and e["motion_state"][0] == 0
    status, n_tracked, n_voting = _motion_step(orc, fr, e, kfs, cam5, sf)
    return status, n_tracked, int((e["last_ids"][0] >= 0).sum()), n_voting


def ref_chain(orc):
    """the same behind trackRefKeyFrame from the 5-key-frame store of tests/test_gpu_local_map.py's reference-key-frame test"""
    import reloc_inputs
    import test_gpu_ref_keyframe_store as rk
    from local_map_ref import build_local_map
    from track_ref import track_frame_ref_keyframe
    from vo_slam_test_amd import synth
    vd = synth.make_vocabulary(3, k=8, L=4)
    c = rk.route_inputs(orc, lambda desc: reloc_inputs.bow_transform(orc, vd, desc))
    order = (c.others[0], c.kfs[1], c.others[1], c.kfs[0])
    # (every key-frame's map points are its own: an id space per key-frame, so that a kept slot's descriptor is its key-frame's)
    kfs = [_kf(dict(ids=(100000 * j + np.arange(len(k["flags"]))).astype(np.int32), flags=np.asarray(k["flags"], np.uint8), points=k["points"],
                    min_dist=np.full(len(k["flags"]), 0.5, f32), max_dist=np.full(len(k["flags"]), 20.0, f32), point_desc=np.asarray(k["desc"], np.uint8)))
           for j, k in enumerate(order)]
    f, ref = REF_FRAME, rk.REF_KF[REF_FRAME]
    fr = c.ofr[f]
    k, d, ux, uy, ur, _ = fr
    n = len(k)
    kf = {kk: (rk._pad(v, c.nk) if kk != "nodes" else rk._pad_nodes(v, c.nk)) for kk, v in c.kfs[f].items()}
    nodes = reloc_inputs.bow_transform(orc, vd, d)
    none = dict(points=np.zeros((1, 3)), normals=np.zeros((1, 3)), min_dist=np.zeros(1, f32), max_dist=np.zeros(1, f32), valid=np.zeros(1, np.uint8),
                desc=np.zeros((1, 32), np.uint8), link=np.full(1, -1, np.int32))
    first = track_frame_ref_keyframe(orc, k, d, ux, uy, ur, c.maps[f][1], kf, nodes, none, c.cam5, c.sf, rk.W, rk.H)
    slots = np.where(first["has"] & (first["assigned_first"] >= 0), kfs[ref]["ids"][np.clip(first["assigned_first"], 0, None)], -1)
    w = build_local_map([int(x) for x in slots], [dict(q, ids=[int(x) for x in q["ids"]], flags=[int(x) for x in q["flags"]]) for q in kfs],
                        MAX_LOCAL, int(ref))
    assert w["slots"] == [int(x) for x in slots]
    kk, ii = [p[0] for p in w["points"]], [p[1] for p in w["points"]]
    col = lambda name, dt: np.array([kfs[a][name][b] for a, b in zip(kk, ii)], dt)
    loc = dict(points=col("points", np.float64), normals=col("normals", np.float64), min_dist=col("min_dist", f32), max_dist=col("max_dist", f32),
               valid=(col("flags", np.uint8) & 3).astype(np.uint8), desc=col("point_desc", np.uint8), link=np.array([p[3] for p in w["points"]], np.int32))
    lids = np.array([p[2] for p in w["points"]], np.int32)
    got = track_frame_ref_keyframe(orc, k, d, ux, uy, ur, c.maps[f][1], kf, nodes, loc, c.cam5, c.sf, rk.W, rk.H)
    a0, a1 = got["assigned_first"], got["assigned_local"]
    kept = got["has"] & (a1 < 0)
    obs = np.where(a1 >= 0, (got["local_flags"][np.clip(a1, 0, None)] >> 1) & 1, np.where(kept, (np.asarray(kf["flags"])[np.clip(a0, 0, None)] >> 1) & 1, 0))
    pts = np.where((a1 >= 0)[:, None], loc["points"][np.clip(a1, 0, None)], np.asarray(kf["points"], np.float64)[np.clip(a0, 0, None)])
    s = dict(n=[n], has_point=got["has"].astype(np.uint8)[None], assigned_local=a1[None], assigned_last=a0[None], observed=obs.astype(np.uint8)[None],
             outlier=got["feature_outlier"][None], points=pts[None], octave=k["octave"].astype(np.int32)[None], angle=k["angle"].astype(f32)[None],
             status=[0], n_tracked=[got["n_tracked"]], local_ids=lids[None], ref_kf=[ref])
    assert got["n_first"] >= 15 and got["observed_inliers_1"] >= 10           # (:268, :274: trackRefKeyFrame itself succeeded)
    return _hand_over_and_track(orc, fr, hs.ROUTE_REF, s, kfs, got["pose_2"], c.cam5, c.sf)


@pytest.mark.parametrize("chain", [reloc_chain, ref_chain])
def test_chain_precondition_under_the_oracle(orc, chain):
    """what tests/test_gpu_handover_store.py relies on: the frame handed over by the model is tracked again by the motion route"""
    status, n_tracked, n_handed, n_voting = chain(orc)
    print(chain.__name__, dict(status=status, n_tracked=n_tracked, n_handed=n_handed, n_voting=n_voting))
    assert n_handed >= 50 and n_voting >= 30
    assert status == 0 and n_tracked >= 30
