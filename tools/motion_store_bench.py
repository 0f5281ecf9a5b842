#!/usr/bin/env python3
"""What a motion-tracked batch needs of the key-frame store between and behind its two stages, both routes in one process on one
tracker (DESIGN.md sections 4v, 7):
  device  vo_tracker_build_local_map after vo_tracker_track_first_dev, vo_tracker_point_stats, vo_tracker_record_ref_pose +
          vo_tracker_refresh_last_pose: seven launches, nothing else
  host    what the library offered before: ASSIGNED_LAST and FEATURE_HAS_POINT read, updateLocalKeyFrames / updateLocalMapPoints
          in numpy per frame over a host copy of the store (votes by bincount, the expansion, first occurrences by np.unique),
          vo_tracker_set_local_map + _ids; the counter lists from three reads (ASSIGNED_LOCAL, FEATURE_OUTLIER, LOCAL_FLAGS);
          FRAME_POSE read, Tcr * ref pose in numpy, vo_tracker_set_last_pose.  The host copy of the store, its id index and the
          last ids are taken BEFORE the timed window (a caller of the host route keeps them), which favours this side.
Batch: --batch frames built from --unique synthetic frames with their synth.make_tracking_map maps; four key-frames per unique
frame hold local points of its map.  A repetition is track_first_dev | BUILD | track_local_map | STATS | end_frame | POSES; only
the parts in capitals are timed, each until the tracker's stream has drained, and summed.  Both routes alternate after --warmup
repetitions of each; medians of --reps, spread = (max - min) / median.
--bench-fps F (bench.py's headline of the same session) adds the ratios to one tracked step = batch / F; the tool does not measure it.
usage: tools/motion_store_bench.py [--batch 1024] [--unique 32] [--reps 9] [--warmup 2] [--bench-fps F] [--out FILE]"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

f32 = np.float32
TH, STRIDE, NK, KF = 2.6, 100000, 300, 4


def make_store(maps, seed=5):
    """per unique frame KF key-frames over its local map: two of 40 .. NK features from 60 % of the map, one reached through the
    graph, one that holds nothing -> list of dicts (ids, flags, points, normals, min_dist, max_dist, point_desc, graph)"""
    rng = np.random.default_rng(seed)
    kfs = []
    for u, (_, _, last, local) in enumerate(maps):
        n, m = len(last["flags"]), len(local["valid"])
        ids = np.where(local["link"] >= 0, local["link"], n + np.arange(m)).astype(np.int32) + u * STRIDE
        perm = rng.permutation(m)
        pool, rest = perm[:int(0.6 * m)], perm[int(0.6 * m):]
        base = KF * u
        kf = lambda idx, pid, fl, **g: dict(ids=np.asarray(pid, np.int32), flags=np.asarray(fl, np.uint8), points=local["points"][idx],
                                            normals=local["normals"][idx], min_dist=local["min_dist"][idx], max_dist=local["max_dist"][idx],
                                            point_desc=local["desc"][idx], **g)
        for j, size in enumerate((NK, 150)):
            idx = rng.choice(pool, min(size, len(pool)), replace=False)
            kfs.append(kf(idx, ids[idx], local["valid"][idx], neighbors=[base + 1, base + 2] if j == 0 else [base], children=[base + 3],
                          parent=-1 if j == 0 else base))
        idx = rest[:80]
        kfs.append(kf(idx, u * STRIDE + 50000 + np.arange(len(idx)), local["valid"][idx], neighbors=[base], children=[base + 3], parent=base))
        idx = rest[80:120]
        kfs.append(kf(idx, ids[idx], np.full(len(idx), 2), neighbors=[], children=[], parent=base))
    return kfs


def host_local_map(kfs, holders, slot_ids, last_first, max_local):
    """updateLocalKeyFrames + updateLocalMapPoints for one frame -> (arrays of its local points, best key-frame)"""
    votes = np.zeros(len(kfs), np.int64)
    for p in slot_ids[slot_ids >= 0]:
        hs = holders.get(int(p))
        if hs is not None:
            votes[hs] += 1
    voters = np.nonzero(votes)[0]
    if len(voters) == 0:
        return None, -1
    best = int(voters[np.argmax(votes[voters])])
    lst, marked = list(voters), set(int(v) for v in voters)
    for k in voters:
        if len(lst) > 80:
            break
        g = kfs[k]
        for group in (g["neighbors"], g["children"]):
            for x in group:
                if x not in marked:
                    lst.append(x), marked.add(x)
                    break
        if g["parent"] >= 0 and g["parent"] not in marked:
            lst.append(g["parent"]), marked.add(g["parent"])
    cat = lambda key: np.concatenate([kfs[k][key] for k in lst])
    ids, fl = cat("ids"), cat("flags")
    on = np.nonzero(fl & 1)[0]
    _, first = np.unique(ids[on], return_index=True)
    sel = on[np.sort(first)][:max_local]
    pid = ids[sel]
    link = np.array([last_first.get(int(p), -1) for p in pid], np.int32)
    return dict(points=cat("points")[sel], normals=cat("normals")[sel], min_dist=cat("min_dist")[sel], max_dist=cat("max_dist")[sel],
                valid=fl[sel] & 3, desc=cat("point_desc")[sel], ids=pid, link=link), best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--unique", type=int, default=32)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-local", type=int, default=1024)
    ap.add_argument("--bench-fps", type=float, default=None,
                    help="bench.py's headline (tracked frames per second) measured in the same session: one tracked step = batch / this; "
                         "without it no ratio to a tracked step is recorded")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "motion_store_bench.json"))
    args = ap.parse_args()
    import torch
    from vo_slam_test_amd import _lib as vo
    from vo_slam_test_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("motion_store_bench: no GPU (a measurement path does not fall back)")
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
    kfs = make_store(maps)
    # ---- the two stores: the map side (graph set by the caller) and the pose side (the mapping layer)
    store, pstore = vo.KeyFrameStore(len(kfs), NK), vo.KeyFrameStore(len(kfs), NK)
    pstore.enable_connections(), pstore.enable_culling(), pstore.enable_mapping(np.array([*cam5[:4], cam5[4], cam5[4] / cam5[0]], f32), 1.2 ** np.arange(8), 0)
    for s in (store, pstore):
        for k in kfs:
            n = len(k["ids"])
            s.insert(dict(angle=np.zeros(n, f32), desc=np.zeros((n, 32), np.uint8), nodes=np.zeros(n, np.int32), flags=k["flags"], points=k["points"],
                          ids=k["ids"], point_desc=k["point_desc"], min_dist=k["min_dist"], max_dist=k["max_dist"], bad=False))
    store.set_graph_batch(0, [k["neighbors"] for k in kfs], [k["children"] for k in kfs], [k["parent"] for k in kfs])
    kf_pose = []
    for i, k in enumerate(kfs):
        store.set_normals(i, k["normals"])
        T = maps[i // KF][0]
        pstore.set_pose(i, T)
        kf_pose.append(np.asarray(T, np.float64))
    kf_pose = np.stack(kf_pose)
    holders = {}
    for i, k in enumerate(kfs):
        for p in np.unique(k["ids"][(k["flags"] & 1) != 0]):
            holders.setdefault(int(p), []).append(i)
    holders = {p: np.array(v) for p, v in holders.items()}
    # ---- the tracker, its last-frame list with ids
    n_last = max(len(m[2]["flags"]) for m in maps)
    trk = vo.Tracker(B, cam5, None, W, H, max_last=cap, max_local=ML, inv_depth_scale=inv, single_stream=True)
    stack = lambda key, fill=0: np.stack([np.concatenate([maps[f % U][2][key], np.full((n_last - len(maps[f % U][2][key]),) + maps[f % U][2][key].shape[1:],
                                                                                      fill, maps[f % U][2][key].dtype)]) for f in range(B)])
    T0 = np.stack([maps[f % U][0] for f in range(B)])
    last_ids = np.stack([np.concatenate([np.arange(len(maps[f % U][2]["flags"])) + (f % U) * STRIDE, np.full(n_last - len(maps[f % U][2]["flags"]), -1)])
                         for f in range(B)]).astype(np.int32)
    last_flags = stack("flags")
    la = {key: stack(key) for key in ("points", "octave", "angle", "desc")}

    def reset():
        trk.set_last_frame(T0, la["points"], last_flags, la["octave"], la["angle"], la["desc"])
        trk.set_last_frame_ids(last_ids)
        trk.set_last_pose(T0, np.ones(B, np.uint8))
    last_first = []
    for f in range(U):
        d = {}
        for i in range(n_last - 1, -1, -1):
            if last_flags[f, i] & 1 and last_ids[f, i] >= 0:
                d[int(last_ids[f, i])] = i
        last_first.append(d)
    frames = torch.from_numpy(np.stack([uniq[f % U] for f in range(B)])).cuda()
    depth = torch.from_numpy(np.stack([udep[f % U] for f in range(B)]).view(np.int16)).cuda()
    n_feat = np.array([fr[f % U]["n"] for f in range(B)])
    ref = torch.from_numpy(np.array([KF * (f % U) for f in range(B)], np.int32)).cuda()

    def timed(call):
        trk.sync()
        t0 = time.perf_counter()
        call()
        trk.sync()
        return (time.perf_counter() - t0) * 1e3

    def device():
        reset()
        trk.track_first_dev(frames, depth)
        ms = timed(lambda: trk.build_local_map(store))
        trk.track_local_map()
        ms += timed(trk.point_stats)
        trk.end_frame(TH)
        ms += timed(lambda: (trk.record_ref_pose(pstore), trk.refresh_last_pose(pstore)))
        return ms

    def host_build():
        a0, has = trk.get(trk.ASSIGNED_LAST), trk.get(trk.FEATURE_HAS_POINT)
        in_n = np.arange(cap)[None, :] < n_feat[:, None]
        sid = np.where(in_n & (has != 0) & (a0 >= 0), last_ids[np.arange(B)[:, None], np.clip(a0, 0, None)], -1)
        z = lambda shape, dt, fill=0: np.full((B, ML) + shape, fill, dt)
        arr = dict(points=z((3,), np.float64), normals=z((3,), np.float64), min_dist=z((), f32), max_dist=z((), f32), valid=z((), np.uint8),
                   desc=z((32,), np.uint8), link=z((), np.int32, -1), ids=z((), np.int32, -1))
        best = np.full(B, -1, np.int32)
        for f in range(B):
            loc, best[f] = host_local_map(kfs, holders, sid[f], last_first[f % U], ML)
            if loc is not None:
                for key in arr:
                    arr[key][f, :len(loc[key])] = loc[key]
        trk.set_local_map(arr["points"], arr["normals"], arr["min_dist"], arr["max_dist"], arr["valid"], arr["desc"], link=arr["link"])
        trk.set_local_map_ids(arr["ids"])
        return sid, arr["ids"], best

    def host_stats(sid, lids):
        a1, outl, lfl = trk.get(trk.ASSIGNED_LOCAL), trk.get(trk.FEATURE_OUTLIER), trk.get(trk.LOCAL_FLAGS)
        vis_a = sid >= 0
        fnd_a = vis_a & (a1 < 0) & (outl == 0)
        fnd_b = np.zeros((B, ML), bool)
        fi, ii = np.nonzero((a1 >= 0) & (outl == 0))
        fnd_b[fi, a1[fi, ii]] = True
        vis_b = ((lfl[:, :ML] & 1) != 0) & (lids >= 0)
        ids = np.concatenate([np.where(vis_a, sid, -1), np.where(vis_b | fnd_b, lids, -1)], axis=1).astype(np.int32)
        return ids, np.concatenate([vis_a, vis_b], axis=1).astype(np.int32), np.concatenate([fnd_a, fnd_b], axis=1).astype(np.int32)

    def host_poses(best):
        T = trk.get(trk.FRAME_POSE)
        P = kf_pose[np.clip(best, 0, None)]
        R, t, Rp, tp = T[:, :9].reshape(B, 3, 3), T[:, 9:], P[:, :9].reshape(B, 3, 3), P[:, 9:]
        Rcr = R @ Rp.transpose(0, 2, 1)
        tcr = t - (Rcr @ tp[:, :, None])[:, :, 0]
        Rn, tn = Rcr @ Rp, (Rcr @ tp[:, :, None])[:, :, 0] + tcr
        new = np.where((best >= 0)[:, None], np.concatenate([Rn.reshape(B, 9), tn], axis=1), T)
        trk.set_last_pose(new, np.ones(B, np.uint8))

    def host():
        reset()
        trk.track_first_dev(frames, depth)
        keep = {}
        ms = timed(lambda: keep.update(zip(("sid", "lids", "best"), host_build())))
        trk.track_local_map()
        ms += timed(lambda: host_stats(keep["sid"], keep["lids"]))
        trk.end_frame(TH)
        ms += timed(lambda: host_poses(keep["best"]))
        return ms

    for _ in range(args.warmup):
        device(), host()
    dev_ms, host_ms = [], []
    for _ in range(args.reps):            # interleaved: both see the same machine
        dev_ms.append(device()), host_ms.append(host())
    device()
    res = trk.results()
    npts, found = trk.get(trk.LOCAL_N_POINTS), trk.get(trk.STAT_FOUND)
    summary = lambda v: dict(ms=float(np.median(v)), spread=float((max(v) - min(v)) / np.median(v)), runs_ms=[float(x) for x in v])
    out = dict(tool="motion_store_bench", batch=B, unique_frames=U, max_features=cap, max_local=ML, keyframes=len(kfs), store_max_features=NK,
               reps=args.reps, version=vo.lib().vo_version().decode(), tracked=int((res["status"] == 0).sum()), local_points_per_frame=float(npts.mean()),
               found_per_frame=float(found.sum() / B), launches=dict(device=7, source="read off the code, not traced"),
               device=summary(dev_ms), host=summary(host_ms))
    out["host_over_device"] = out["host"]["ms"] / out["device"]["ms"]
    if args.bench_fps:
        step = 1e3 * B / args.bench_fps
        out["tracked_step"] = dict(ms=step, bench_fps=args.bench_fps,
                                   source="not measured by this tool: batch / the --bench-fps argument, bench.py's headline of the same session")
        out["device_over_tracked_step"] = out["device"]["ms"] / step
        out["host_over_tracked_step"] = out["host"]["ms"] / step
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("device", "host")} | dict(device_ms=out["device"]["ms"], host_ms=out["host"]["ms"],
                                                                                         device_spread=out["device"]["spread"],
                                                                                         host_spread=out["host"]["spread"])))
    trk.close()


if __name__ == "__main__":
    main()
