#!/usr/bin/env python3
"""updateLocalKeyFrames + updateLocalMapPoints for a batch, both forms in one process run on the same tracker and store
(DESIGN.md sections 4g, 7):
  device  vo_tracker_build_local_map (two launches behind the route; the observation index warm, or rebuilt first)
  host    download VO_TRACKER_ASSIGNED_LAST / _FEATURE_HAS_POINT, a numpy build over a host copy of the store (votes by
          bincount over a prebuilt id -> holders table, points by np.unique), vo_tracker_set_local_map + _ids
Setup: the six synthetic frames tiled to the batch, each behind vo_tracker_track_ref_keyframe_store(first_stage_only) against
its own features as reference key-frame; a store of --keyframes key-frames of ~1000 features: the six reference key-frames
and, per frame, a group of key-frames that share ids with it (so that a frame has ~ keyframes / 6 voters), random graph.
Per form and repetition the time until the stream has drained (`total_ms`) and, for the device form, the time between two
events on the tracker's stream around the call (`event_ms`); medians after a warm-up call and the spread as (max - min) /
median.  The index rebuild on its own: the store works on the tracker's stream here, so the events around a call that finds
the index stale (an update_points before the first event: its copies and its synchronisation are outside) span the rebuild's
launches and the builder's; `index_rebuild_ms` is that minus the warm call's event time.  Per-kernel times come from a
profiler run of this tool (rocprofv3 --kernel-trace --stats), not from the tool.  The two forms' local maps are compared
first and the tool stops if they differ.
usage: tools/local_map_bench.py [--batch 1024] [--keyframes 500] [--max-local 4096] [--reps 7] [--out FILE]"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

IDS_PER_GROUP = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--keyframes", type=int, default=500)
    ap.add_argument("--max-local", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from vo_slam_test_amd import _lib as vo
    from vo_slam_test_amd import synth
    B, W, H, NB, K, ML = a.batch, 640, 480, 6, a.keyframes, a.max_local
    cam5 = synth.CAM.astype(np.float32)
    inv = float(np.float32(1.0) / np.float32(synth.DEPTH_SCALE))
    imgs6 = synth.make_frames(NB, start=80)
    raw6 = np.stack([synth.make_depth(80 + i) for i in range(NB)]).view(np.uint16)
    vd = synth.make_vocabulary(3, k=8, L=4)
    voc = vo.Vocabulary(vd["L"], vd["child_start"], vd["children"], vd["node_desc"], vd["node_weight"], vd["word_id"])
    t6 = vo.Tracker(NB, cam5, None, W, H, max_last=8, max_local=8, inv_depth_scale=inv)
    t6.track_first(imgs6, raw6)
    t6.sync()
    base = [t6.download_frame(f) for f in range(NB)]
    t6.close()
    rng = np.random.default_rng(1)
    nk = max(len(fr["x"]) for fr in base)
    kfs = []
    for f in range(NB):   # the reference key-frames: the frame's own features, shuffled, 1 % descriptor noise
        fr = base[f]
        idx = rng.permutation(len(fr["x"]))
        z = np.where(fr["depth"][idx] > 0, fr["depth"][idx], 2.5).astype(np.float64)
        P = np.stack([(fr["x"][idx].astype(np.float64) - cam5[2]) * z / cam5[0], (fr["y"][idx].astype(np.float64) - cam5[3]) * z / cam5[1], z], 1)
        desc = fr["desc"][idx].copy()
        flip = rng.random(desc.shape) < 0.01
        desc[flip] ^= rng.integers(1, 256, int(flip.sum()), dtype=np.uint8)
        n = len(idx)
        kfs.append(dict(angle=fr["angle"][idx].astype(np.float32), desc=desc, nodes=voc.transform(desc)[2], flags=np.full(n, 3, np.uint8), points=P,
                        ids=(f * IDS_PER_GROUP + np.arange(n)).astype(np.int32), point_desc=desc, min_dist=np.full(n, 0.1, np.float32),
                        max_dist=np.full(n, 50.0, np.float32)))
    for k in range(NB, K):   # the rest: a group per frame, ids half the reference key-frame's, half their own
        n = nk
        kfs.append(dict(angle=np.zeros(n, np.float32), desc=np.zeros((n, 32), np.uint8), nodes=np.zeros(n, np.int32), flags=np.full(n, 3, np.uint8),
                        points=rng.normal(0, 2, (n, 3)), ids=((k % NB) * IDS_PER_GROUP + rng.integers(0, 2000, n)).astype(np.int32),
                        point_desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), min_dist=np.full(n, 0.1, np.float32),
                        max_dist=np.full(n, 50.0, np.float32)))
    for k, kf in enumerate(kfs):
        others = np.setdiff1d(np.arange(K), [k])
        kf["normals"] = kf["points"] / np.maximum(np.linalg.norm(kf["points"], axis=1, keepdims=True), 1e-9)
        kf["neighbors"] = [int(x) for x in rng.choice(others, min(10, len(others)), replace=False)]
        kf["children"] = sorted(int(x) for x in rng.choice(others, min(3, len(others)), replace=False))
        kf["parent"] = int(rng.choice(others)) if len(others) else -1
    which = np.arange(B) % NB
    imgs = torch.from_numpy(np.ascontiguousarray(imgs6[which])).cuda()
    raw = torch.from_numpy(np.ascontiguousarray(raw6[which]).view(np.int16)).cuda()
    Tcw = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64), (B, 1))
    trk = vo.Tracker(B, cam5, None, W, H, max_last=nk, max_local=ML, inv_depth_scale=inv)
    store = vo.KeyFrameStore(K, nk, stream=trk.st)
    for kf in kfs:
        store.insert(kf)
    store.set_graph_batch(0, [kf["neighbors"] for kf in kfs], [kf["children"] for kf in kfs], [kf["parent"] for kf in kfs])
    for k, kf in enumerate(kfs):
        store.set_normals(k, kf["normals"])
    d_ref, d_Tcw = torch.from_numpy(which.astype(np.int32)).cuda(), torch.from_numpy(Tcw).cuda()
    trk.track_ref_keyframe_store(store, voc, d_ref, d_Tcw, imgs, raw, first_stage_only=True)
    trk.results()

    # ---- the host form's copy of the store: flat per-feature columns, per key-frame ranges, id -> holders (ascending)
    n_of = np.array([len(kf["flags"]) for kf in kfs])
    start = np.concatenate([[0], np.cumsum(n_of)])
    flat = {key: np.concatenate([np.asarray(kf[key]) for kf in kfs]) for key in ("ids", "flags", "points", "normals", "min_dist", "max_dist", "point_desc")}
    kf_of = np.repeat(np.arange(K), n_of)
    pairs = np.unique(np.stack([flat["ids"][(flat["flags"] & 1) == 1], kf_of[(flat["flags"] & 1) == 1]], 1), axis=0)
    n_ids = NB * IDS_PER_GROUP
    h_start = np.concatenate([[0], np.cumsum(np.bincount(pairs[:, 0], minlength=n_ids))])
    h_kf = pairs[:, 1]
    bad = np.zeros(K, bool)
    link_of = np.full((NB, n_ids), -1, np.int32)   # lowest feature of reference key-frame r that holds the id
    for r in range(NB):
        ids_r = kfs[r]["ids"]
        link_of[r, ids_r[::-1]] = np.arange(len(ids_r))[::-1]

    def host():
        a0, has = trk.get(trk.ASSIGNED_LAST), trk.get(trk.FEATURE_HAS_POINT)
        out = dict(points=np.zeros((B, ML, 3)), normals=np.zeros((B, ML, 3)), min_dist=np.zeros((B, ML), np.float32),
                   max_dist=np.zeros((B, ML), np.float32), flags=np.zeros((B, ML), np.uint8), point_desc=np.zeros((B, ML, 32), np.uint8))
        ids_out, link = np.full((B, ML), -1, np.int32), np.full((B, ML), -1, np.int32)
        lists = np.full((B, 84), -1, np.int32)
        for f in range(B):
            r = which[f]
            m = (has[f] != 0) & (a0[f] >= 0)
            sid = kfs[r]["ids"][a0[f][m]]
            lo, hi = h_start[sid], h_start[sid + 1]
            take = np.repeat(lo, hi - lo) + (np.arange((hi - lo).sum()) - np.repeat(np.cumsum(hi - lo) - (hi - lo), hi - lo))
            cnt = np.bincount(h_kf[take], minlength=K)
            voters = np.nonzero((cnt > 0) & ~bad)[0]
            lst = list(voters)
            marked = set(lst)
            for k in voters:
                if len(lst) > 80:
                    break
                kf = kfs[k]
                for cands in (kf["neighbors"], kf["children"], [kf["parent"]] if kf["parent"] >= 0 else []):
                    for x in cands:
                        if x not in marked and not bad[x]:
                            lst.append(x)
                            marked.add(x)
                            break
            lst = lst[:84]
            lists[f, :len(lst)] = lst
            e = np.concatenate([np.arange(start[k], start[k + 1]) for k in lst]) if lst else np.zeros(0, np.int64)
            e = e[(flat["flags"][e] & 1) == 1]
            _, first = np.unique(flat["ids"][e], return_index=True)
            e = e[np.sort(first)][:ML]
            n = len(e)
            for key in out:
                out[key][f, :n] = flat[key][e] & 3 if key == "flags" else flat[key][e]
            ids_out[f, :n] = flat["ids"][e]
            link[f, :n] = link_of[r, flat["ids"][e]]
        trk.set_local_map(out["points"], out["normals"], out["min_dist"], out["max_dist"], out["flags"], out["point_desc"], link=link)
        trk.set_local_map_ids(ids_out)
        return ids_out, lists

    def dev_warm():
        trk.build_local_map(store)

    def stale():   # the same map side again: the observation index is stale, the call that follows rebuilds it
        kf = kfs[K - 1]
        store.update_points(K - 1, kf["flags"], kf["points"], kf["ids"], kf["point_desc"], kf["min_dist"], kf["max_dist"])

    stream = torch.cuda.ExternalStream(trk.st)

    def timed(fn, reps, before=None):
        fn()
        trk.sync()
        rows = []
        for _ in range(reps):
            if before:
                before()
                trk.sync()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            fn()
            e1.record(stream)
            trk.sync()
            rows.append(((time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)))
        r = np.array(rows)
        med = np.median(r, 0)
        return dict(total_ms=float(med[0]), event_ms=float(med[1]), spread=float((r[:, 0].max() - r[:, 0].min()) / med[0]),
                    spread_event=float((r[:, 1].max() - r[:, 1].min()) / med[1]), runs_total_ms=[float(v) for v in r[:, 0]])

    res = dict(tool="local_map_bench", batch=B, keyframes=K, features_per_keyframe=int(n_of.mean()), max_local=ML, reps=a.reps,
               version=vo.lib().vo_version().decode())
    h_ids, h_lists = host()
    trk.build_local_map(store)
    trk.results()
    res["maps_equal"] = bool(np.array_equal(trk.get(trk.LOCAL_POINT_IDS), h_ids) and np.array_equal(trk.get(trk.LOCAL_KEYFRAMES), h_lists))
    if not res["maps_equal"]:
        sys.exit("local_map_bench: the device form and the host form built different local maps; nothing is reported")
    res["keyframes_median"] = int(np.median(trk.get(trk.LOCAL_N_KEYFRAMES)))
    res["points_median"] = int(np.median(trk.get(trk.LOCAL_N_POINTS)))
    res["device_warm_index"] = timed(dev_warm, a.reps)
    res["device_stale_index"] = timed(dev_warm, a.reps, before=stale)
    res["index_rebuild_ms"] = res["device_stale_index"]["event_ms"] - res["device_warm_index"]["event_ms"]
    res["host_form"] = timed(host, max(1, min(a.reps, 3)))
    del res["host_form"]["event_ms"], res["host_form"]["spread_event"]   # (the host form's work is not on the stream)
    res["speedup_total_warm"] = res["host_form"]["total_ms"] / res["device_warm_index"]["total_ms"]
    print(json.dumps(res))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
