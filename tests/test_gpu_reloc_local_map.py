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
    c.sub = dict(fx, frames=[fx["frames"][f] for f in FRAMES], fnodes=[fx["fnodes"][f] for f in FRAMES],
                 candidates=[fx["candidates"][1], fx["candidates"][4][:1], []])
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
