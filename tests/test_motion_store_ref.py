"""The model of the motion route from the key-frame store (tests/motion_store_ref.py) on hand-written tables, and the chain of
tests/test_gpu_motion_store.py run under the CPU oracle's tracker with the model between the steps.  The chain validates the
inputs of the device tests where no GPU is needed: the two good streams stay tracked over the synthetic store, every built local
map gains a key-frame through the expansion, the builder nulls slots, and the link makes the local search skip points."""
import numpy as np
import pytest

import handover_inputs as hi
import motion_store_inputs as mi
from handover_ref import IDENTITY, HandoverModel, compose, inverse
from motion_store_ref import RefPoseModel, build, link, slot_ids, stats
from vo_slam_test_amd import synth

f32 = np.float32
MAX_LOCAL = 2048


def test_stats_table():
    s, want, over = mi.stats_table()
    w, first, has = build(s["n"], s["has_point"], s["assigned_last"], s["last_ids"], s["store"], 3)
    assert first.tolist() == want["first_ids"] and has.tolist() == want["has_point"]
    assert [p[2] for p in w["points"]] == [200, 201, 202] and w["best"] == 0 and w["n_points"] == 5
    ids, vis, fnd = stats(s["n"], first, s["assigned_local"], s["outlier"], s["local_ids"], s["local_visible"])
    assert (ids.tolist(), vis.tolist(), fnd.tolist()) == (want["ids"], want["visible"], want["found"])
    # a slot the local search overwrote: visible on the id it held, found on the one it holds now
    ids, vis, fnd = stats(s["n"], over["first_ids"], over["assigned_local"], over["outlier"], s["local_ids"], s["local_visible"])
    assert (ids.tolist(), vis.tolist(), fnd.tolist()) == (over["want_ids"], over["want_visible"], over["want_found"])
    # entries beyond the local map's n are absent; a max_local below a claimed index ignores the claim
    ids, vis, fnd = stats(s["n"], first, s["assigned_local"], s["outlier"], s["local_ids"][:1], s["local_visible"][:1], max_local=3)
    assert ids[8:].tolist() == [200, -1, -1] and fnd[8:].tolist() == [1, 0, 0]


def test_slot_ids_take_the_last_ids_of_the_slots_that_hold_a_point():
    s, _, _ = mi.stats_table()
    assert slot_ids(s["n"], s["has_point"], s["assigned_last"], s["last_ids"]).tolist() == [100, 100, 101, -1, 103, -1, -1, -1]
    assert slot_ids(0, s["has_point"], s["assigned_last"], s["last_ids"]).tolist() == [-1] * 8


@pytest.mark.parametrize("name", list(mi.link_tables()))
def test_link_tables(name):
    t = mi.link_tables()[name]
    assert link(t["last_flags"], t["last_ids"], t["local_ids"]).tolist() == t["want"]
    # the rule of vo_tracker_begin_frame step 3 (tests/handover_ref.py) on the same list
    n = len(t["last_flags"])
    m = HandoverModel(1, n, n, hi.CAM5[:4])
    m.last = dict(points=np.zeros((1, n, 3)), flags=t["last_flags"][None].copy(), octave=np.zeros((1, n), np.int32), angle=np.zeros((1, n), f32),
                  desc=np.zeros((1, n, 32), np.uint8), ids=t["last_ids"][None].copy())
    b = m.begin_frame(dict(n=[n], x=np.zeros((1, n), f32), y=np.zeros((1, n), f32), depth=np.zeros((1, n), f32), desc=np.zeros((1, n, 32), np.uint8)),
                      2.0, is_keyframe=[1], local_ids=t["local_ids"][None])
    assert b["link"][0].tolist() == t["want"]


def test_ref_pose_pairs():
    """a pair is recorded with a valid last pose and a usable key-frame, else the previous one stands; the refresh moves the
    last pose with the key-frame"""
    pose = lambda xi: np.concatenate([synth.se3_exp(np.array(xi))[0].reshape(-1), synth.se3_exp(np.array(xi))[1]])
    K0, K1 = pose([0.1, 0.0, -0.1, 0.01, 0.02, 0.0]), pose([0.3, 0.1, 0.0, -0.02, 0.0, 0.01])
    F = np.stack([pose([0.2, 0.1, 0.0, 0.0, 0.01, 0.0])] * 5)
    m = RefPoseModel(5)
    #            a usable ref | -1 | out of range | pose unset | last pose invalid
    m.record(F, [1, 1, 1, 1, 0], [0, -1, 7, 2, 0], [K0, K1, None])
    assert m.kf.tolist() == [0, -1, -1, -1, -1]
    assert np.abs(compose(m.tcr[0], K0) - F[0]).max() < 1e-15 and np.array_equal(m.tcr[0], compose(F[0], inverse(K0)))
    m.record(F, [1, 1, 1, 1, 1], [1, 0, 0, 0, 0], [K0, K1, None])
    assert m.kf.tolist() == [1, 0, 0, 0, 0]
    m.record(F, [1, 1, 1, 1, 0], [-1, 9, 2, 1, 1], [K0, K1, None])          # -1, out of range, unset keep the remembered one
    assert m.kf.tolist() == [1, 0, 0, 1, 0] and np.array_equal(m.tcr[1], compose(F[1], inverse(K0)))
    K0b = compose(pose([0.0, 0.0, 0.0, 0.001, -0.002, 0.0005]), K0)
    out = m.refresh(F, [K0b, K1, None])
    assert np.array_equal(out[1], compose(m.tcr[1], K0b)) and np.abs(out[1] - F[1]).max() > 1e-4
    assert np.abs(out[0] - F[0]).max() < 1e-15                                # key-frame 1 did not move
    none = RefPoseModel(2)
    assert np.array_equal(none.refresh(F[:2], [K0]), F[:2])                    # no pair: left alone


# ---------------------------------------------------------------------------------------------------------------- the chain
def oracle_chain(orc):
    """the streams of handover_inputs.streams() under the oracle's tracker over motion_store_inputs.store(): per good stream a list
    of dict(status, n_tracked, keyframes, n_nulled, n_skipped, stats)"""
    from reloc_inputs import oracle_frames
    from track_ref import local_map_stage, track_first
    imgs, raw = hi.streams()
    sf = np.array(list(orc.orb_params().scale)[:8], f32)
    frames = [oracle_frames(orc, imgs[:, s] if s != hi.LOST else imgs[:1, s], raw[:, s] if s != hi.LOST else raw[:1, s], hi.INV, hi.CAM5)
              for s in range(hi.B)]
    first = [(fr[0][2], fr[0][3], fr[0][0]["octave"], fr[0][0]["angle"], fr[0][1], fr[0][5]) for fr in frames]
    maps = mi.stream_maps([hi.tracking_map(fr, seed=s) for s, fr in enumerate(first)])
    kfs = mi.store(maps)
    mstore = mi.model_store(kfs)
    log = []
    for s in range(hi.B):
        if s == hi.LOST:
            continue
        fr = frames[s]
        T, last, _ = maps[s]
        poses = [compose(IDENTITY, T) for _ in kfs]
        cap = max(len(f[0]) for f in fr)
        m = HandoverModel(1, cap, cap, hi.CAM5[:4])
        m.set_last_pose([T], [1])
        rp = RefPoseModel(1)
        dep0 = fr[0][5]
        th = float(np.median(dep0[dep0 > 0]))
        steps = []
        for k in range(hi.N_STEPS):
            kp, d, ux, uy, ur, dep = fr[k]
            n = len(kp)
            s1 = track_first(orc, kp, d, ux, uy, ur, T, synth.se3_log(T[:9].reshape(3, 3), T[9:]), last, hi.CAM5, sf)
            before = slot_ids(n, s1["has"], s1["assigned_last"], last["ids"])
            w, first_ids, has = build(n, s1["has"], s1["assigned_last"], last["ids"], mstore, MAX_LOCAL)
            fobs = np.where(has != 0, s1["fobs"], 0).astype(np.uint8)
            loc = mi.local_map(w, kfs, MAX_LOCAL)
            loc["link"] = link(last["flags"], last["ids"], loc["ids"])
            matched = np.zeros(len(last["flags"]), bool)
            matched[s1["assigned_last"][s1["assigned_last"] >= 0]] = True
            s2 = local_map_stage(orc, s1["of"], kp, ux, uy, ur, s1["fpt"], has.astype(bool), fobs, s1["pose_1"], s1["assigned_last"],
                                 s1["n_last_list"], loc, hi.CAM5, sf, hi.W, hi.H, 3.0, 0.8, s1["solve"])
            rows = stats(n, first_ids, s2["assigned_local"], s2["feature_outlier"], loc["ids"], s2["local_flags"])
            pad = lambda a, fill=0: np.concatenate([a, np.full((cap - n,) + a.shape[1:], fill, a.dtype)])[None]
            st = dict(n=[n], assigned_last=pad(s1["assigned_last"], -1), assigned_local=pad(s2["assigned_local"], -1),
                      has_point=pad(s2["has"].astype(np.uint8)), outlier=pad(s2["feature_outlier"]), points=pad(s1["fpt"]),
                      octave=pad(kp["octave"].astype(np.int32)), angle=pad(kp["angle"].astype(f32)), status=[s1["status"]],
                      n_tracked=[s2["n_tracked"]], last={k_: np.asarray(last[k_])[None] for k_ in ("flags", "desc", "ids")},
                      local=dict(flags=loc["valid"][None], desc=loc["desc"][None], ids=loc["ids"][None]))
            R, t = synth.se3_exp(s2["pose_2"])
            e = m.end_frame(st, [np.concatenate([R.reshape(-1), t])])
            rp.record(e["frame_pose"], m.last_valid, [w["best"]], poses)
            m.last_pose = rp.refresh(m.last_pose, poses)
            b = m.begin_frame(dict(n=[n], x=pad(ux), y=pad(uy), depth=pad(dep), desc=pad(d)), th)
            steps.append(dict(status=s1["status"], n_tracked=s2["n_tracked"], keyframes=w["keyframes"], n_points=w["n_points"],
                              n_nulled=int(((before >= 0) & (first_ids < 0)).sum()), n_voting=int((first_ids >= 0).sum()),
                              n_skipped=int(((loc["link"] >= 0) & matched[np.clip(loc["link"], 0, None)]).sum()), ref_kf=int(rp.kf[0]),
                              found=int(rows[2].sum()), visible=int(rows[1].sum()), n_local=s2["n_local"]))
            last = {k_: b["last_" + k_][0] for k_ in ("points", "flags", "octave", "angle", "desc", "ids")}
            T = b["Tcw"][0]
        log.append((s, steps))
    return log


def test_chain_precondition_under_the_oracle(orc):
    """what tests/test_gpu_motion_store.py relies on"""
    nulled = skipped = 0
    for s, steps in oracle_chain(orc):
        assert len(steps) == hi.N_STEPS
        for k, r in enumerate(steps):
            print(s, k, {key: v for key, v in r.items() if key != "keyframes"}, r["keyframes"])
            assert r["status"] == 0 and r["n_tracked"] >= 30, (s, k, r)
            # the key-frame that never holds a point enters through the expansion, behind at least one voter
            assert mi.KF_PER_STREAM * s + 3 in r["keyframes"] and len(r["keyframes"]) >= 2, (s, k, r)
            assert r["n_points"] <= MAX_LOCAL and r["ref_kf"] >= 0 and 0 < r["found"] <= r["visible"], (s, k, r)
            nulled, skipped = nulled + r["n_nulled"], skipped + r["n_skipped"]
    assert nulled >= 1 and skipped >= 1
