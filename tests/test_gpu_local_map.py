"""vo_tracker_build_local_map (updateLocalKeyFrames + updateLocalMapPoints on the device, visualOdometry.cpp:595-724)
against the model tests/local_map_ref.py.  All comparisons are exact: the outputs are integers and copied values.

The slot ids are injected through the smallest route that leaves them in place: a relocalisation from the key-frame store
on four frames of the relocalisation fixture (three relocalise, one fails).  The ids the frames end up with are whatever the
store's key-frames carry, so the synthetic stores of the tests below are built FROM the downloaded slot ids: any store in
the same id space serves vo_tracker_build_local_map after a relocalisation."""
import numpy as np
import pytest

import reloc_db_inputs
import reloc_inputs
from local_map_ref import build_local_map
from reloc_local_ref import local_map_after_reloc, make_local_map

pytestmark = pytest.mark.gpu

FRAMES = (0, 1, 2, 4)   # of the fixture: three that relocalise, one whose candidates all fail
W, H = reloc_inputs.W, reloc_inputs.H
ARRAYS = ("LOCAL_POINTS", "LOCAL_NORMALS", "LOCAL_MIN_DISTANCE", "LOCAL_MAX_DISTANCE", "LOCAL_DESC", "LOCAL_MAP_FLAGS", "LOCAL_POINT_IDS",
          "LOCAL_LINK")


class _Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(vo, orc):
    fx = reloc_inputs.build(orc)
    c = _Ctx()
    c.fx = fx
    c.sub = dict(fx, frames=[fx["frames"][f] for f in FRAMES], fnodes=[fx["fnodes"][f] for f in FRAMES],
                 candidates=[fx["candidates"][f] for f in FRAMES])
    c.imgs = np.ascontiguousarray(fx["imgs"][list(FRAMES)])
    c.raw = np.ascontiguousarray(fx["raw"][list(FRAMES)]).view(np.uint16)
    vd = fx["vocab"]
    c.voc = vo.Vocabulary(vd["L"], vd["child_start"], vd["children"], vd["node_desc"], vd["node_weight"], vd["word_id"])
    kfs, c.lists = reloc_db_inputs.keyframes(c.sub)
    c.kfs = [dict(k, flags=(np.asarray(k["flags"], np.uint8) & 1) * 3) for k in kfs]   # (observed: bit 1 wherever bit 0)
    c.slots = None
    yield c
    c.voc.close()


def _relocalized(vo, c, max_local, G=None):
    """a tracker behind vo_tracker_relocalize_store on the fixture (G: in that gauge of tests/gauge.py -- the slot ids must be
    the same) -> (tracker, the store it read, slot ids [B][cap], status)"""
    import torch
    import gauge
    trk = vo.Tracker(len(FRAMES), c.fx["cam5"], None, W, H, max_last=8, max_local=max_local, inv_depth_scale=float(c.fx["inv"]),
                     max_reloc_candidates=reloc_inputs.MAX_CAND, max_reloc_features=c.fx["nk"])
    store = vo.KeyFrameStore(len(c.kfs) + 4, c.fx["nk"])
    for k in c.kfs:
        store.insert(k if G is None else dict(k, points=gauge.points(G, k["points"])))
    stride = max(len(ls) for ls in c.lists)
    cand = np.full((len(c.lists), stride), -1, np.int32)
    for f, ls in enumerate(c.lists):
        cand[f, :len(ls)] = ls
    trk.relocalize_store(store, c.voc, torch.tensor([len(ls) for ls in c.lists], dtype=torch.int32).cuda(), torch.from_numpy(cand).cuda(),
                         c.imgs, c.raw)
    status = trk.results()["status"]
    slots = np.where(trk.get(trk.FEATURE_HAS_POINT) != 0, trk.get(trk.RELOC_POINT_IDS), -1)
    assert list(status & 4) == [0, 0, 0, 4] and all((slots[f] >= 0).sum() >= 50 for f in range(3))
    if c.slots is None:
        c.slots = slots
    ok = np.ones(len(FRAMES), bool) if G is None else (status & 4) == 0
    # the same injection every time; in another gauge for the frames that relocalise -- what the failed frame keeps is the
    # leak of candidates whose PnP found a few inliers, and RANSAC's masks hang on the float32 rounding of the points
    assert np.array_equal(slots[ok], c.slots[ok])
    return trk, store, slots, status


def _synthetic(rng, K, feat_lo, feat_hi, pool, foreign=5000, p_bad=0.1, empty=()):
    """K key-frames of feat_lo .. feat_hi features with ids drawn from `pool` (and a few nobody else holds), random map
    side, random graph -> list of dicts: the model's fields and the arrays the store takes"""
    out = []
    for k in range(K):
        n = 0 if k in empty else int(rng.integers(feat_lo, feat_hi + 1))
        ids = np.where(rng.random(n) < 0.9, rng.choice(pool, n), foreign + rng.integers(0, 50, n)).astype(np.int32)
        others = [x for x in range(K) if x != k]
        pick = lambda m: [int(x) for x in rng.permutation(others)[:int(rng.integers(0, m + 1))]]
        out.append(dict(ids=ids, flags=rng.choice(np.array([0, 1, 1, 3, 3, 2], np.uint8), n), bad=bool(rng.random() < p_bad),
                        neighbors=pick(10), children=sorted(pick(6)), parent=int(rng.choice(others)) if rng.random() < 0.7 else -1,
                        points=rng.normal(0, 2, (n, 3)), normals=rng.normal(0, 1, (n, 3)), min_dist=rng.uniform(0.1, 1, n).astype(np.float32),
                        max_dist=rng.uniform(2, 9, n).astype(np.float32), point_desc=rng.integers(0, 256, (n, 32), dtype=np.uint8)))
    return out


def _device_store(vo, kfs, max_features, max_keyframes=None, batch=True):
    s = vo.KeyFrameStore(max_keyframes or len(kfs), max_features)
    for k in kfs:
        n = len(k["ids"])
        s.insert(dict(angle=np.zeros(n, np.float32), desc=np.zeros((n, 32), np.uint8), nodes=np.zeros(n, np.int32), flags=k["flags"],
                      points=k["points"], ids=k["ids"], point_desc=k["point_desc"], min_dist=k["min_dist"], max_dist=k["max_dist"],
                      bad=k["bad"]))
    if batch:
        s.set_graph_batch(0, [k["neighbors"] for k in kfs], [k["children"] for k in kfs], [k["parent"] for k in kfs])
    for i, k in enumerate(kfs):
        if not batch:
            s.set_graph(i, k["neighbors"], k["children"], k["parent"])
        s.set_normals(i, k["normals"])
    return s


def _model(kfs):
    return [dict(k, ids=[int(x) for x in k["ids"]], flags=[int(x) for x in k["flags"]]) for k in kfs]


def _compare(trk, kfs, slots, failed, max_local, ref_kf=None, expect_capacity=False):
    """every output of the builder against the model -> the slots after the nulling"""
    want = [build_local_map([int(x) for x in slots[f]], _model(kfs), max_local, None if ref_kf is None else int(ref_kf[f]), bool(failed[f]))
            for f in range(len(slots))]
    assert any(w["capacity"] for w in want) == expect_capacity
    if expect_capacity:
        with pytest.raises(Exception, match="status -4"):
            trk.results()
        trk.results()   # sticky: reported once
    else:
        trk.results()
    lk, nk, npts, best = (trk.get(getattr(trk, key)) for key in ("LOCAL_KEYFRAMES", "LOCAL_N_KEYFRAMES", "LOCAL_N_POINTS", "LOCAL_REF_KF"))
    got = {key: trk.get(getattr(trk, key)) for key in ARRAYS}
    has = trk.get(trk.FEATURE_HAS_POINT)
    after = []
    for f, w in enumerate(want):
        assert list(lk[f]) == w["keyframes"] + [-1] * (84 - len(w["keyframes"])), f
        assert (nk[f], npts[f], best[f]) == (w["n_keyframes"], w["n_points"], w["best"]), f
        n = len(w["points"])
        kk, ii = [p[0] for p in w["points"]], [p[1] for p in w["points"]]
        col = lambda name: np.array([kfs[k][name][i] for k, i in zip(kk, ii)], np.asarray(kfs[0][name]).dtype).reshape(
            (n,) + np.asarray(kfs[0][name]).shape[1:])
        assert np.array_equal(got["LOCAL_POINTS"][f, :n], col("points")) and np.array_equal(got["LOCAL_NORMALS"][f, :n], col("normals")), f
        assert np.array_equal(got["LOCAL_MIN_DISTANCE"][f, :n], col("min_dist")) and np.array_equal(got["LOCAL_MAX_DISTANCE"][f, :n], col("max_dist"))
        assert np.array_equal(got["LOCAL_DESC"][f, :n], col("point_desc")) and np.array_equal(got["LOCAL_MAP_FLAGS"][f, :n], col("flags") & 3)
        assert list(got["LOCAL_POINT_IDS"][f, :n]) == [p[2] for p in w["points"]] and list(got["LOCAL_LINK"][f, :n]) == [p[3] for p in w["points"]]
        assert (got["LOCAL_MAP_FLAGS"][f, n:max_local] == 0).all() and (got["LOCAL_POINT_IDS"][f, n:max_local] == -1).all()
        ws = np.array(w["slots"])
        assert np.array_equal(has[f] != 0, ws >= 0), f
        after.append(ws)
    if ref_kf is None:
        ids = trk.get(trk.RELOC_POINT_IDS)
        for f, ws in enumerate(after):
            assert np.array_equal(ids[f][ws >= 0], ws[ws >= 0]) and (ids[f][(slots[f] >= 0) & (ws < 0)] == -1).all()
    return np.array(after), want


def _pool(slots, rng, m):
    live = np.unique(slots[slots >= 0])
    return rng.choice(live, min(m, len(live)), replace=False)


def test_store_index_and_its_lazy_rebuild(vo, ctx):
    """12 key-frames of 16-64 features over ~200 shared ids; update_points on two key-frames (bit 0 cleared, ids changed)
    must show in the next build"""
    rng = np.random.default_rng(1)
    trk, keep, slots, status = _relocalized(vo, ctx, 900)
    kfs = _synthetic(rng, 12, 16, 64, _pool(slots, rng, 200), p_bad=0.0)
    store = _device_store(vo, kfs, 64, batch=False)
    trk.build_local_map(store)
    slots, want = _compare(trk, kfs, slots, status & 4, 900)
    assert sum(w["n_keyframes"] for w in want) >= 12 and sum(w["n_points"] for w in want) >= 100
    for k in (int(want[0]["best"]), 5):
        kf = kfs[k]
        kf["flags"] = np.where(rng.random(len(kf["flags"])) < 0.5, kf["flags"] & 2, kf["flags"]).astype(np.uint8)
        kf["ids"] = np.where(rng.random(len(kf["ids"])) < 0.5, kf["ids"][::-1], kf["ids"]).astype(np.int32)
        store.update_points(k, kf["flags"], kf["points"], kf["ids"], kf["point_desc"], kf["min_dist"], kf["max_dist"])
    trk.build_local_map(store)
    _, again = _compare(trk, kfs, slots, status & 4, 900)
    assert [w["points"] for w in again] != [w["points"] for w in want]   # else the update shows nothing
    trk.close()


def test_builder_on_a_batch_of_four(vo, ctx):
    """bad key-frames, a key-frame without features, max_features no multiple of 64, orphan ids, a failed frame"""
    rng = np.random.default_rng(2)
    trk, keep, slots, status = _relocalized(vo, ctx, 1500)
    pool = np.concatenate([_pool(slots[f:f + 1], rng, 120) for f in range(3)])
    kfs = _synthetic(rng, 40, 5, 50, pool, p_bad=0.15, empty=(3, 17))
    store = _device_store(vo, kfs, 50, max_keyframes=45)
    trk.build_local_map(store)
    after, want = _compare(trk, kfs, slots, status & 4, 1500)
    assert (after < 0).sum() > (slots < 0).sum()   # orphan ids were nulled
    assert want[3]["keyframes"] == [] and all(len(w["keyframes"]) > 0 for w in want[:3])
    assert any(kfs[k]["bad"] for k in range(40)) and all(w["best"] >= 0 for w in want[:3])
    trk.close()


def test_more_than_80_voters_and_the_list_bound(vo, ctx):
    """100 key-frames x 16 features: frame 0 has exactly 80 voters (the expansion reaches 83 and stops), frame 1 has 82 (no
    expansion), frame 2 has 90 (the first 84 kept, the true count and the sticky VO_ERR_CAPACITY reported)"""
    rng = np.random.default_rng(3)
    trk, keep, slots, status = _relocalized(vo, ctx, 1700)
    kfs = _synthetic(rng, 100, 16, 16, np.array([9000]), foreign=9100, p_bad=0.0)
    own = [_pool(slots[f:f + 1], rng, 40) for f in range(3)]
    for k in range(100):
        for f, nv in enumerate((80, 82, 90)):
            if k < nv:
                kfs[k]["ids"][f], kfs[k]["flags"][f] = own[f][k % len(own[f])], 1
        kfs[k].update(neighbors=[90 + k % 10, (k + 1) % 100], children=[95] if k < 95 else [], parent=99 if k < 99 else -1)
    store = _device_store(vo, kfs, 16)
    trk.build_local_map(store)
    _, want = _compare(trk, kfs, slots, status & 4, 1700, expect_capacity=True)
    assert [w["n_keyframes"] for w in want] == [83, 82, 90, 0] and len(want[2]["keyframes"]) == 84
    trk.close()


def test_max_local_one_below_a_frames_count(vo, ctx):
    rng = np.random.default_rng(4)
    kfs = None
    for max_local in (4000, None):
        if max_local is None:
            counts = [w["n_points"] for w in want]
            max_local = max(counts) - 1
            assert sorted(counts)[-2] < max_local   # the other frames stay below it
        trk, keep, slots, status = _relocalized(vo, ctx, max_local)
        if kfs is None:   # a group of key-frames per frame, linked among themselves: frame 0's is the large one
            kfs = []
            for f, K in enumerate((20, 5, 5)):
                grp = _synthetic(rng, K, 30, 60, _pool(slots[f:f + 1], rng, 150 if f == 0 else 30), foreign=5000 + 100 * f, p_bad=0.0)
                for k in grp:
                    k.update(neighbors=[x + len(kfs) for x in k["neighbors"]], children=[x + len(kfs) for x in k["children"]],
                             parent=k["parent"] + len(kfs) if k["parent"] >= 0 else -1)
                kfs = kfs + grp
        store = _device_store(vo, kfs, 60)
        trk.build_local_map(store)
        _, want = _compare(trk, kfs, slots, status & 4, max_local, expect_capacity=max_local < 4000)
        trk.close()
    assert max(w["n_points"] for w in want) == max_local + 1 and max(len(w["points"]) for w in want) == max_local


def test_invalid_after_a_route_without_ids(vo, ctx):
    c = ctx
    trk, keep, slots, status = _relocalized(vo, c, 600)
    rng = np.random.default_rng(5)
    kfs = _synthetic(rng, 6, 8, 20, _pool(slots, rng, 60))
    store = _device_store(vo, kfs, 20)
    trk.set_last_frame(np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64), (4, 1)), np.zeros((4, 0, 3)), np.zeros((4, 0), np.uint8),
                       np.zeros((4, 0), np.int32), np.zeros((4, 0), np.float32), np.zeros((4, 0, 32), np.uint8))
    trk.track_first(c.imgs, c.raw)   # a route that leaves no ids
    with pytest.raises(vo.VoError, match="status -1"):
        trk.build_local_map(store)
    # the tracker is still usable: the relocalisation again, then the build
    trk.close()
    trk, keep, slots, status = _relocalized(vo, c, 600)
    with pytest.raises(vo.VoError, match="status -1"):
        store.set_graph(0, [99], [], -1)          # an id outside the store
    with pytest.raises(vo.VoError, match="status -4"):
        vo.check(vo.lib().vo_kfstore_set_graph(store._h, 0, 0, None, 65, vo._p(np.zeros(65, np.int32)), -1), "vo_kfstore_set_graph")
    trk.build_local_map(store)
    _compare(trk, kfs, slots, status & 4, 600)
    trk.close()


def _local_kf(fr, local, normals=True):
    """the local map of reloc_local_ref.make_local_map as one more key-frame of the store"""
    n = len(local["valid"])
    return dict(ids=np.asarray(local["ids"], np.int32), flags=np.asarray(local["valid"], np.uint8), bad=False, neighbors=[], children=[], parent=-1,
                points=local["points"], normals=local["normals"], min_dist=local["min_dist"], max_dist=local["max_dist"],
                point_desc=local["desc"], angle=np.zeros(n, np.float32), desc=np.zeros((n, 32), np.uint8), nodes=np.zeros(n, np.int32))


def _snapshot(trk):
    out = dict(trk.results())
    for key in ("ASSIGNED_LOCAL", "RELOC_POINT_IDS", "FEATURE_HAS_POINT", "FEATURE_OUTLIER"):
        out[key] = trk.get(getattr(trk, key))
    out["FEATURE_POINTS"] = np.where(out["FEATURE_HAS_POINT"][..., None] != 0, trk.get(trk.FEATURE_POINTS), 0.0)
    return out


def test_end_to_end_after_relocalize_db_dev(vo, orc, ctx):
    """relocalize_db_dev -> build_local_map -> track_local_map against the same relocalisation followed by download,
    local_map_ref, set_local_map + ids, track_local_map: bit-identical, and the host-built form finds new local matches"""
    import torch
    c = ctx
    nk, B, max_local = c.fx["nk"], len(FRAMES), 3000
    kfs, lists = reloc_db_inputs.db_keyframes(orc, c.sub)
    kfs = [dict(k, ids=(np.asarray(k["ids"], np.int64) + nk).astype(np.int32), flags=(np.asarray(k["flags"], np.uint8) & 1) * 3) for k in kfs]
    dbi = reloc_db_inputs.database(orc, c.sub, kfs, lists)
    words = [c.voc.transform(k["desc"])[:2] for k in kfs]
    d_img, d_raw = torch.from_numpy(c.imgs).cuda(), torch.from_numpy(c.raw.view(np.int16)).cuda()
    extra = None
    snaps = []
    for way in ("device", "host"):
        trk = vo.Tracker(B, c.fx["cam5"], None, W, H, max_last=8, max_local=max_local, inv_depth_scale=float(c.fx["inv"]),
                         max_reloc_candidates=4, max_reloc_features=nk)
        store = vo.KeyFrameStore(len(kfs) + B, nk)
        db = vo.KeyFrameDatabase(dbi["n_words"], len(kfs), nk, B)
        for k in kfs:
            store.insert(k)
        for w, v in vo.bow_vector([w for w, _ in words], [v for _, v in words]):
            db.insert(w, v)
        db.set_neighbors_batch(0, dbi["neighbors"])
        trk.relocalize_db(db, store, c.voc, d_img, d_raw)
        before = _snapshot(trk)
        ok = np.nonzero((before["status"] & 4) == 0)[0]
        assert len(ok) >= 1
        slots = np.where(before["FEATURE_HAS_POINT"] != 0, before["RELOC_POINT_IDS"], -1)
        if extra is None:   # one more key-frame per relocalised frame: its local map, sharing ids with the frame's slots
            extra = []
            for f in ok:
                fr = c.sub["frames"][f]
                n = len(fr[0])
                end = dict(ids=slots[f, :n], outlier=before["FEATURE_OUTLIER"][f, :n])
                lm = make_local_map(fr, end, c.fx["cam5"], seed=int(f))
                lm["ids"] = np.where(lm["ids"] >= (1 << 20), lm["ids"] + (int(f) << 16), lm["ids"])   # fresh ids distinct per frame
                extra.append(_local_kf(fr, lm))
        model_store = [dict(k, bad=bool(k.get("bad", False)), neighbors=[], children=[], parent=-1) for k in kfs] + extra
        for j, k in enumerate(extra):
            at = store.insert(k)
            store.set_normals(at, k["normals"])
            store.set_graph(at, [0], [], -1)
            model_store[at] = dict(k, neighbors=[0])
        if way == "device":
            trk.build_local_map(store)
        else:
            want = [build_local_map([int(x) for x in slots[f]], _model(model_store), max_local, None, bool(before["status"][f] & 4)) for f in range(B)]
            assert all(w["slots"] == [int(x) for x in slots[f]] for f, w in enumerate(want))   # no orphan: the host form cannot null slots
            z = lambda shape, dt: np.zeros((B, max_local) + shape, dt)
            arr = dict(points=z((3,), np.float64), min_dist=z((), np.float32), max_dist=z((), np.float32), flags=z((), np.uint8),
                       point_desc=z((32,), np.uint8))
            ids = np.full((B, max_local), -1, np.int32)
            for f, w in enumerate(want):
                for q, (k, i, p, _) in enumerate(w["points"]):
                    for key in arr:
                        arr[key][f, q] = np.asarray(model_store[k][key])[i] if key != "flags" else model_store[k]["flags"][i] & 3
                    ids[f, q] = p
            nrm0 = z((3,), np.float64)   # (the candidates' normals were never set: the column is zero)
            for f, w in enumerate(want):
                for q, (k, i, p, _) in enumerate(w["points"]):
                    if k >= len(kfs):
                        nrm0[f, q] = model_store[k]["normals"][i]
            trk.set_local_map(arr["points"], nrm0, arr["min_dist"], arr["max_dist"], arr["flags"], arr["point_desc"])
            trk.set_local_map_ids(ids)
        trk.track_local_map(th_radius=5.0)
        snaps.append(_snapshot(trk))
        if way == "host":   # the comparison is not between two empty results: the CPU oracle on the host-built local map of one frame
            f = int(ok[0])
            fr = c.sub["frames"][f]
            n = len(fr[0])
            nq = len(want[f]["points"])
            loc = dict(points=arr["points"][f, :nq], normals=nrm0[f, :nq], min_dist=arr["min_dist"][f, :nq], max_dist=arr["max_dist"][f, :nq],
                       valid=arr["flags"][f, :nq], desc=arr["point_desc"][f, :nq], ids=ids[f, :nq])
            end = dict(ids=slots[f, :n], outlier=before["FEATURE_OUTLIER"][f, :n], pose=before["pose"][f],
                       points=before["FEATURE_POINTS"][f, :n])
            oracle = local_map_after_reloc(orc, fr, end, lambda i_: np.ones(len(i_), bool), loc, c.fx["cam5"], c.fx["sf"])
            assert oracle["n_local"] > 0 and oracle["n_local"] == snaps[-1]["n_matches_local"][f]
            assert np.array_equal(oracle["assigned_local"], snaps[-1]["ASSIGNED_LOCAL"][f, :n])
        trk.close()
    assert (snaps[1]["n_matches_local"] > 0).any()
    for key in snaps[0]:
        assert np.array_equal(snaps[0][key], snaps[1][key]), key


# ---- the reference-key-frame route: the inputs of tests/test_gpu_ref_keyframe_store.py ------------------------------------
import test_gpu_ref_keyframe_store as rk  # noqa: E402

rk_ctx = rk.ctx   # (its module fixture: frames, key-frames, store, tracker)


def test_after_track_ref_keyframe_store_first_stage(vo, orc, rk_ctx):
    """slot ids = store.ids[ref_kf][assigned_last] of the slots that survive the culling; `link` = the lowest feature of the
    reference key-frame with the id; then track_local_map on the built map against the same map set from the host"""
    c = rk_ctx
    order = (c.others[0], c.kfs[1], c.others[1], c.kfs[0])   # the store's insertion order (rk's ctx.store)
    kfs = []
    for k in order:
        n = len(k["flags"])
        P = np.asarray(k["points"], np.float64)
        kfs.append(dict(ids=np.arange(n, dtype=np.int32), flags=np.asarray(k["flags"], np.uint8), bad=False, neighbors=[], children=[], parent=-1,
                        points=P, normals=P / np.maximum(np.linalg.norm(P, axis=1, keepdims=True), 1e-9), min_dist=np.full(n, 0.5, np.float32),
                        max_dist=np.full(n, 20.0, np.float32), point_desc=np.asarray(k["desc"], np.uint8)))
    kfs[0].update(neighbors=[2], parent=1)
    ref = np.array(rk.REF_KF)
    # one more key-frame: the first 1000 points of frame 0's synthetic local map (the one the route's own tests search).  A
    # point linked to a last-frame entry is the map point of the reference key-frame's feature with the same position and
    # carries its id; the others get ids nobody else holds.
    last, loc = c.maps[0][2], c.maps[0][3]
    m = min(1000, len(loc["valid"]), c.nk)
    at = {tuple(p): i for i, p in enumerate(np.asarray(c.kfs[0]["points"]))}
    lid = np.array([at[tuple(last["points"][L])] if L >= 0 else 100000 + j for j, L in enumerate(loc["link"][:m])], np.int32)
    kfs.append(dict(ids=lid, flags=np.asarray(loc["valid"][:m], np.uint8), bad=False, neighbors=[], children=[], parent=-1,
                    points=np.asarray(loc["points"][:m], np.float64), normals=np.asarray(loc["normals"][:m], np.float64),
                    min_dist=np.asarray(loc["min_dist"][:m], np.float32), max_dist=np.asarray(loc["max_dist"][:m], np.float32),
                    point_desc=np.asarray(loc["desc"][:m], np.uint8)))
    snaps = []
    for way in ("device", "host"):
        trk, st = c.tracker(), c.store()
        k = kfs[4]
        st.insert(dict(angle=np.zeros(m, np.float32), desc=np.zeros((m, 32), np.uint8), nodes=np.zeros(m, np.int32), flags=k["flags"],
                       points=k["points"], ids=k["ids"], point_desc=k["point_desc"], min_dist=k["min_dist"], max_dist=k["max_dist"]))
        for i, k in enumerate(kfs):
            st.set_normals(i, k["normals"])
            st.set_graph(i, k["neighbors"], k["children"], k["parent"])
        trk.track_ref_keyframe_store(st, c.voc, c.d_ref, c.d_Tcw, c.imgs, c.depth, first_stage_only=True)
        trk.results()
        a0, has = trk.get(trk.ASSIGNED_LAST), trk.get(trk.FEATURE_HAS_POINT)
        slots = np.full(a0.shape, -1, np.int64)
        for f in range(len(ref)):
            held = (has[f] != 0) & (a0[f] >= 0)
            slots[f, held] = kfs[ref[f]]["ids"][a0[f, held]]
        max_local = trk.max_local
        if way == "device":
            trk.build_local_map(st)
            _, want = _compare(trk, kfs, slots, np.zeros(len(ref), int), max_local, ref_kf=ref)
            assert any(p[3] >= 0 for p in want[0]["points"]) and any(p[3] < 0 for p in want[0]["points"])   # `link` both ways
        else:
            want = [build_local_map([int(x) for x in slots[f]], _model(kfs), max_local, int(ref[f])) for f in range(len(ref))]
            z = lambda shape, dt: np.zeros((len(ref), max_local) + shape, dt)
            arr = dict(points=z((3,), np.float64), normals=z((3,), np.float64), min_dist=z((), np.float32), max_dist=z((), np.float32),
                       flags=z((), np.uint8), point_desc=z((32,), np.uint8))
            link = np.full((len(ref), max_local), -1, np.int32)
            for f, w in enumerate(want):
                for q, (k, i, p, lk) in enumerate(w["points"]):
                    for key in arr:
                        arr[key][f, q] = kfs[k][key][i] & 3 if key == "flags" else kfs[k][key][i]
                    link[f, q] = lk
            trk.set_local_map(arr["points"], arr["normals"], arr["min_dist"], arr["max_dist"], arr["flags"], arr["point_desc"], link=link)
        trk.track_local_map()
        snaps.append(rk._collect(trk))
        trk.close()
    # the comparison is not between two empty results: the CPU oracle's trackRefKeyFrame + trackLocalMap on frame 0 with the
    # host-built local map finds new local matches, the ones the host form found on the device
    from track_ref import track_frame_ref_keyframe
    k, d, ux, uy, ur, _ = c.ofr[0]
    nq = len(want[0]["points"])
    lo = dict(points=arr["points"][0, :nq], normals=arr["normals"][0, :nq], min_dist=arr["min_dist"][0, :nq], max_dist=arr["max_dist"][0, :nq],
              valid=arr["flags"][0, :nq], desc=arr["point_desc"][0, :nq], link=link[0, :nq])
    kf = {kk: (rk._pad(v, c.nk) if kk != "nodes" else rk._pad_nodes(v, c.nk)) for kk, v in c.kfs[0].items()}
    oracle = track_frame_ref_keyframe(orc, k, d, ux, uy, ur, c.maps[0][1], kf, c.voc.transform(d, 3)[2], lo, c.cam5, c.sf, rk.W, rk.H)
    assert oracle["n_local"] > 0 and oracle["n_local"] == snaps[1]["n_matches_local"][0]
    assert np.array_equal(oracle["assigned_local"], snaps[1]["ASSIGNED_LOCAL"][0, :len(k)])
    for key in snaps[0]:
        assert np.array_equal(snaps[0][key], snaps[1][key]), key


# ---------------------------------------------------------------------------------------------------------------------
# The builder after a rigid change of the world frame (tests/gauge.py).  Its outputs are integers and copied values, so
# the model comparison stays exact; the relocalisation that injects the slot ids runs in the new gauge too.
RELOC_GAUGE_POSE_TOL = 1.54e-5


def reloc_models(orc, fx, sub, lists, kfs, G):
    """the CPU model of the relocalisation of every frame of the batch on the store's key-frames in gauge G"""
    import gauge
    import reloc_ref
    out = []
    for f, fr in enumerate(sub["frames"]):
        cands = [dict(kfs[g], points=gauge.points(G, kfs[g]["points"])) for g in lists[f]]
        out.append(reloc_ref.relocalize(orc, fr[0], fr[1], fr[2], fr[3], fr[4], sub["fnodes"][f], cands, fx["cam5"], fx["sf"]))
    return out


@pytest.mark.parametrize("name", ["skew_2.6_w_negative", "skew_2.4_w_positive", "y_pi_minus_0.02"])
def test_builder_in_a_rotated_world_frame(vo, orc, ctx, name):
    """the batch of test_builder_on_a_batch_of_four with every point at G P and every normal at R_G n.
    1. Device against the model in the new gauge, exactly (_compare); the relocalised poses against reloc_ref within 1e-9.
    2. Against the identity gauge: the slot ids after the relocalisation, the key-frame lists, counts, reference key-frames,
    point ids, links and flags identical; the copied points and normals mapped back through G equal the identity gauge's to
    the rounding of the two rigid maps (4e-15 at |P| < 20 m); the relocalised poses mapped back within
    RELOC_GAUGE_POSE_TOL = 1.54e-5, ten times the worst deviation of the corrected model between the gauges on these frames,
    1.54e-6, measured on the CPU (PnP reads float32 points, see tests/test_gpu_reloc_local_map.py).
    The frame whose candidates all fail is compared with the model in its own gauge only: the slots it keeps are the leak
    of PnP inlier masks, which the float32 rounding of the moved points changes in the model as well (y gauge)."""
    import gauge
    from vo_slam_test_amd import synth
    c = ctx
    G = gauge.GAUGES[name]
    results = []
    for g in (None, G):
        rng = np.random.default_rng(2)
        trk, keep, slots, status = _relocalized(vo, c, 1500, g)   # (asserts the slot ids of the identity gauge)
        poses = trk.results()["pose"].copy()
        pool = np.concatenate([_pool(slots[f:f + 1], rng, 120) for f in range(3)])
        kfs = _synthetic(rng, 40, 5, 50, pool, p_bad=0.15, empty=(3, 17))
        if g is not None:
            kfs = [dict(k, points=gauge.points(g, k["points"]), normals=gauge.directions(g, k["normals"])) for k in kfs]
        store = _device_store(vo, kfs, 50, max_keyframes=45)
        trk.build_local_map(store)
        after, want = _compare(trk, kfs, slots, status & 4, 1500)
        got = {key: trk.get(getattr(trk, key)) for key in ARRAYS + ("LOCAL_KEYFRAMES", "LOCAL_N_KEYFRAMES", "LOCAL_N_POINTS", "LOCAL_REF_KF")}
        results.append((after, want, got, poses, status.copy()))
        trk.close(), store.close(), keep.close()
    (a0, w0, g0, p0, s0), (a1, w1, g1, p1, s1) = results
    models = reloc_models(orc, c.fx, c.sub, c.lists, c.kfs, G)
    ok = (s0 & 4) == 0
    assert np.array_equal(a0[ok], a1[ok]) and np.array_equal(s0, s1)
    for f in range(len(FRAMES)):
        for key in ("keyframes", "n_keyframes", "n_points", "best", "points", "capacity") + (("slots",) if ok[f] else ()):
            assert w0[f][key] == w1[f][key], (f, key)
    for key in ("LOCAL_KEYFRAMES", "LOCAL_N_KEYFRAMES", "LOCAL_N_POINTS", "LOCAL_REF_KF", "LOCAL_POINT_IDS", "LOCAL_LINK", "LOCAL_MAP_FLAGS",
                "LOCAL_MIN_DISTANCE", "LOCAL_MAX_DISTANCE", "LOCAL_DESC"):
        assert np.array_equal(g0[key], g1[key]), key
    for f in range(len(FRAMES)):
        n = len(w1[f]["points"])
        back = (g1["LOCAL_POINTS"][f, :n] - G[1]) @ G[0]
        assert n > 0 or s1[f] & 4   # (the failed frame has no local map)
        assert n == 0 or np.abs(back - g0["LOCAL_POINTS"][f, :n]).max() < 4e-15 * 20 and np.abs(g1["LOCAL_NORMALS"][f, :n] @ G[0] - g0["LOCAL_NORMALS"][f, :n]).max() < 4e-15 * 20
        # (the failed frame too: its pose is what the last solve of a rejected candidate left, test_control_plane_parity)
        assert gauge.pose_distance(synth.se3_exp(p1[f]), synth.se3_exp(models[f]["pose"])) < 1e-9, f
        if s1[f] & 4:
            continue
        d = gauge.pose_distance(gauge.pose6_back(G, p1[f]), synth.se3_exp(p0[f]))
        print(f"{name} frame {f}: relocalised pose, rotated gauge mapped back - identity gauge {d:.3g}")
        assert d < RELOC_GAUGE_POSE_TOL, (f, d)
