#!/usr/bin/env python3
"""The hand-over behind the store's relocalisation and reference-key-frame routes, both forms in one process on one tracker
(DESIGN.md sections 4w, 7):
  device  vo_tracker_point_stats_store + vo_tracker_end_frame_store: two launches, nothing else
  host    what the library offered before for the same frames: vo_tracker_results, the vo_tracker_get reads (ASSIGNED_LOCAL,
          FEATURE_HAS_POINT, FEATURE_OUTLIER, FEATURE_POINTS and RELOC_POINT_IDS + RELOC_WINNER, or ASSIGNED_LAST +
          LOCAL_POINT_IDS), the slot rule and both cullings in numpy over the whole batch, the descriptor of every id by
          np.searchsorted in a table of first holders, vo_tracker_set_last_frame + _set_last_frame_ids + _set_last_pose.  The
          table, the reference key-frames' ids and the frames' octave / angle columns are taken BEFORE the timed window (a caller
          of the host route keeps them), and the observed mark is taken as set (every point of the bench's store is observed):
          both favour this side.  The counter rows are not formed on this side at all.
Batch: --batch frames built from --unique synthetic frames; per unique frame two key-frames: its synth.make_tracking_map last
list (the relocalisation candidate and the reference key-frame) and the first NK points of its local map, joined in the graph.
A repetition is front (relocalize_store_dev, or track_ref_keyframe_store_dev first stage) | build_local_map | track_local_map |
HAND-OVER; only the part in capitals is timed, until the tracker's stream has drained.  Per route both forms alternate after
--warmup repetitions of each; medians of --reps, spread = (max - min) / median.
usage: tools/handover_store_bench.py [--batch 1024] [--unique 32] [--reps 9] [--warmup 2] [--max-local 4096] [--bench-fps F] [--out FILE]"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

f32 = np.float32
TH, STRIDE, FRESH, MIN_TRACKED = 2.6, 100000, 50000, 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--unique", type=int, default=32)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-local", type=int, default=4096)
    ap.add_argument("--bench-fps", type=float, default=None,
                    help="bench.py's headline (tracked frames per second) measured in the same session: one tracked step = batch / this; "
                         "without it no ratio to a tracked step is recorded")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "handover_store_bench.json"))
    args = ap.parse_args()
    import torch
    from vo_slam_test_amd import _lib as vo
    from vo_slam_test_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("handover_store_bench: no GPU (a measurement path does not fall back)")
    B, W, H, U, ML = args.batch, 640, 480, max(1, min(args.batch, args.unique)), args.max_local
    cam5, inv = synth.CAM.astype(f32), float(f32(1.0) / f32(synth.DEPTH_SCALE))
    uniq = synth.make_frames(U, start=3000)
    udep = np.stack([synth.make_depth(3000 + i) for i in range(U)])
    probe = vo.Tracker(U, cam5, None, W, H, max_last=1, max_local=1, inv_depth_scale=inv)
    probe.track_first(uniq, udep)
    probe.results()
    fr = [probe.download_frame(i) for i in range(U)]
    cap = probe.cap
    probe.close()
    maps = [synth.make_tracking_map(d["x"], d["y"], d["octave"], d["angle"], d["desc"], d["depth"], seed=i) for i, d in enumerate(fr)]
    vd = synth.make_vocabulary(3, k=8, L=4)
    voc = vo.Vocabulary(vd["L"], vd["child_start"], vd["children"], vd["node_desc"], vd["node_weight"], vd["word_id"])
    # ---- the store: key-frame 2 u = unique frame u's last list, 2 u + 1 = the first NK points of its local map
    NK = max(len(m[2]["flags"]) for m in maps)
    kfs = []
    for u, (_, _, last, local) in enumerate(maps):
        n, m = len(last["flags"]), min(NK, len(local["valid"]))
        P = np.asarray(last["points"], np.float64)
        kfs.append(dict(angle=last["angle"].astype(f32), desc=last["desc"], nodes=voc.transform(last["desc"], 3)[2], flags=((last["flags"] & 1) * 3).astype(np.uint8),
                        points=P, ids=(u * STRIDE + np.arange(n)).astype(np.int32), point_desc=last["desc"], min_dist=np.full(n, 0.05, f32),
                        max_dist=np.full(n, 60.0, f32), normals=P / np.maximum(np.linalg.norm(P, axis=1, keepdims=True), 1e-9),
                        graph=([2 * u + 1], [], -1)))
        link = local["link"][:m]
        kfs.append(dict(angle=np.zeros(m, f32), desc=np.zeros((m, 32), np.uint8), nodes=np.zeros(m, np.int32), flags=((local["valid"][:m] & 1) * 3).astype(np.uint8),
                        points=np.asarray(local["points"][:m], np.float64), ids=(u * STRIDE + np.where(link >= 0, link, FRESH + np.arange(m))).astype(np.int32),
                        point_desc=local["desc"][:m], min_dist=local["min_dist"][:m].astype(f32), max_dist=local["max_dist"][:m].astype(f32),
                        normals=np.asarray(local["normals"][:m], np.float64), graph=([2 * u], [], 2 * u)))
    store = vo.KeyFrameStore(len(kfs), NK)
    for k in kfs:
        store.insert({key: k[key] for key in ("angle", "desc", "nodes", "flags", "points", "ids", "point_desc", "min_dist", "max_dist")})
    for i, k in enumerate(kfs):
        store.set_normals(i, k["normals"])
        store.set_graph(i, *k["graph"])
    # the host side's table of first holders: id -> descriptor (ascending key-frame, feature)
    tid, tdesc = [], []
    for k in kfs:
        on = (k["flags"] & 1) != 0
        tid.append(k["ids"][on]), tdesc.append(np.asarray(k["point_desc"])[on])
    tid, tdesc = np.concatenate(tid), np.concatenate(tdesc)
    uid, first = np.unique(tid, return_index=True)
    udesc = tdesc[first]
    ref_ids = np.full((B, NK), -1, np.int32)
    for f in range(B):
        k = kfs[2 * (f % U)]
        ref_ids[f, :len(k["ids"])] = k["ids"]
    trk = vo.Tracker(B, cam5, None, W, H, max_last=max(cap, NK), max_local=ML, inv_depth_scale=inv, single_stream=True, max_reloc_candidates=2,
                     max_reloc_features=NK)
    frames = torch.from_numpy(np.stack([uniq[f % U] for f in range(B)])).cuda()
    depth = torch.from_numpy(np.stack([udep[f % U] for f in range(B)]).view(np.int16)).cuda()
    n_feat = np.array([fr[f % U]["n"] for f in range(B)])
    in_n = np.arange(cap)[None, :] < n_feat[:, None]
    col = lambda key, dt: np.stack([np.concatenate([fr[f % U][key][:cap], np.zeros(cap - len(fr[f % U][key][:cap]), dt)]).astype(dt) for f in range(B)])
    octave, angle = col("octave", np.int32), col("angle", f32)
    T0 = np.stack([maps[f % U][0] for f in range(B)])
    d_T0 = torch.from_numpy(T0).cuda()
    d_ref = torch.from_numpy(np.array([2 * (f % U) for f in range(B)], np.int32)).cuda()
    d_nc, d_cand = torch.ones(B, dtype=torch.int32).cuda(), d_ref.clone().reshape(B, 1)

    def timed(call):
        trk.sync()
        t0 = time.perf_counter()
        call()
        trk.sync()
        return (time.perf_counter() - t0) * 1e3

    def front(route):
        trk.set_last_pose(T0, np.ones(B, np.uint8))
        if route == "reloc":
            trk.relocalize_store(store, voc, d_nc, d_cand, frames, depth)
        else:
            trk.track_ref_keyframe_store(store, voc, d_ref, d_T0, frames, depth, first_stage_only=True)
        trk.build_local_map(store)
        trk.track_local_map(th_radius=5.0 if route == "reloc" else 3.0)

    def device(route):
        front(route)
        return timed(lambda: (trk.point_stats_store(store), trk.end_frame_store(store, TH, MIN_TRACKED)))

    def host_handover(route):
        res = trk.results()
        a1, has, outl, pts = trk.get(trk.ASSIGNED_LOCAL), trk.get(trk.FEATURE_HAS_POINT), trk.get(trk.FEATURE_OUTLIER), trk.get(trk.FEATURE_POINTS)
        if route == "reloc":
            fid, win = trk.get(trk.RELOC_POINT_IDS), trk.get(trk.RELOC_WINNER)
            sid = np.where(in_n & (has != 0) & (win >= 0)[:, None], fid, -1)
        else:
            a0, lids = trk.get(trk.ASSIGNED_LAST), trk.get(trk.LOCAL_POINT_IDS)
            rows = np.arange(B)[:, None]
            kept = np.where(in_n & (has != 0) & (a0 >= 0) & (a0 < NK), ref_ids[rows, np.clip(a0, 0, NK - 1)], -1)
            sid = np.where(in_n & (a1 >= 0), lids[rows, np.clip(a1, 0, lids.shape[1] - 1)], kept)
        pos = np.clip(np.searchsorted(uid, sid), 0, len(uid) - 1)
        held = (sid >= 0) & (uid[pos] == sid)                              # (every point observed: cullingTempMapPoints removes none)
        ids = np.where(held, sid, -1).astype(np.int32)
        flags = np.where(held, np.where(outl != 0, 2, 3), 0).astype(np.uint8)
        desc = np.where(held[..., None], udesc[pos], 0).astype(np.uint8)
        points = np.where(held[..., None], pts, 0.0)
        ok = (res["status"] == 0) & (res["n_tracked"] >= MIN_TRACKED)
        trk.set_last_frame(res["Tcw"], points, flags, octave, angle, desc)
        trk.set_last_frame_ids(ids)
        trk.set_last_pose(res["Tcw"], ok.astype(np.uint8))
        return ids

    def host(route):
        front(route)
        return timed(lambda: host_handover(route))

    out = dict(tool="handover_store_bench", batch=B, unique_frames=U, max_features=cap, max_local=ML, keyframes=len(kfs), store_max_features=NK,
               reps=args.reps, version=vo.lib().vo_version().decode(), launches=dict(device=2, source="read off the code, not traced"),
               host_note="interpreted Python over numpy arrays of the whole batch; the device side is two kernel launches", routes={})
    summary = lambda v: dict(ms=float(np.median(v)), spread=float((max(v) - min(v)) / np.median(v)), runs_ms=[float(x) for x in v])
    for route in ("reloc", "ref"):
        for _ in range(args.warmup):
            device(route), host(route)
        dev_ms, host_ms = [], []
        for _ in range(args.reps):            # interleaved: both see the same machine
            dev_ms.append(device(route)), host_ms.append(host(route))
        device(route)
        res = trk.results()
        dev_ids, found = trk.get(trk.LAST_IDS)[:, :cap], trk.get(trk.STAT_FOUND)
        front(route)
        host_ids = host_handover(route)
        r = dict(device=summary(dev_ms), host=summary(host_ms), tracked=int(((res["status"] == 0) & (res["n_tracked"] >= MIN_TRACKED)).sum()),
                 handed_over_per_frame=float((dev_ids >= 0).sum() / B), found_per_frame=float(found.sum() / B),
                 host_ids_equal_device=bool(np.array_equal(dev_ids, host_ids[:, :cap])))
        r["host_over_device"] = r["host"]["ms"] / r["device"]["ms"]
        if args.bench_fps:
            step = 1e3 * B / args.bench_fps
            r["device_over_tracked_step"], r["host_over_tracked_step"] = r["device"]["ms"] / step, r["host"]["ms"] / step
        out["routes"][route] = r
    if args.bench_fps:
        out["tracked_step"] = dict(ms=1e3 * B / args.bench_fps, bench_fps=args.bench_fps,
                                   source="not measured by this tool: batch / the --bench-fps argument, bench.py's headline of the same session")
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({route: {k: (v if not isinstance(v, dict) else dict(ms=v["ms"], spread=v["spread"])) for k, v in r.items()}
                      for route, r in out["routes"].items()} | dict(batch=B, max_features=cap)))
    trk.close(), store.close(), voc.close()


if __name__ == "__main__":
    main()
