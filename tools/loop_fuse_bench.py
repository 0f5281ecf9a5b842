#!/usr/bin/env python3
"""LoopClosing::searchAndFuse for a key-frame store (DESIGN.md sections 4q, 7):
  device  vo_kfstore_search_and_fuse_dev: nothing but launches (three memsets, k_lf_begin and two launches per corrected
          key-frame; the index is fresh when the call begins)
  host    the only route a store caller had before: vo_kfstore_get_points and get_point_refs for the corrected key-frames, the
          replay of searchAndFuse / fuseByPose / replaceMapPoint on that copy in numpy / Python (the gates of a pass's loop points
          at once, the window search per candidate over the target's features, adds at once, the replaces in list order with an
          index of the copy by id -- tools/fuse_bench.py's HostMap), then vo_kfstore_update_points, set_normals and
          set_point_refs for the same key-frames and add_point_stats for the counters that grew.
The two forms' records, flags, ids, points, point_desc, normals, min / max, ref_kf and recent lists are compared first and the
tool stops if they differ.
Store: tools/fuse_bench.py's -- --keyframes key-frames of --features features, the last 12 the scene with poses and a map side,
a seeded third of whose map-point features came in without their map point.  The corrected key-frames are the scene's (the
only ones of this store with a pose column; each corrected to the Sim3 of its own pose, which is what finds the missing third),
the loop points the distinct live points of the scene's first --loop-keyframes key-frames, in key-frame and feature order: what
compute_sim3 collects from a match and its neighbours.  A call cannot be undone, so every repetition runs on a freshly built
store (not timed).  Reported: median, min and max of --reps calls, until the stream has drained (`total_ms`) and between two
events (`event_ms`), and the call's record.
--once builds one store and runs a single call, --build-only builds the store alone: the difference of the kernel counts of two
kernel-trace runs is the call's launches (k_obs_fill: one per index rebuild); --stale makes the index stale first.
usage: tools/loop_fuse_bench.py [--keyframes 500] [--features 1000] [--reps 20] [--once [--stale] | --build-only] [--out FILE]"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402

from fuse_bench import BOUNDS, GRID_COLS, GRID_ROWS, POP, TH_LOW, HostMap, host_replace  # noqa: E402
from new_points_bench import CAM6, FIRST_ID, SCENE, SF, scene_keyframes  # noqa: E402

f32 = np.float32
TH = f32(4.0)


def host_fuse_by_pose(T, Tm, ids, hm, static, threshold=TH):
    """Matcher::fuseByPose (matcher.cpp:1135-1238) on the copy under the pose Tm: the gates of every loop point at once in numpy
    (they read nothing an earlier hit of the pass changes: section 4q's derivation 1), then the search in list order; a hit on an
    empty feature is added at once -> (passed, matches, adds, [(A, B)] in list order)"""
    st, kfT = hm.st[T], static[T]
    cand = []
    for p in ids:
        c = hm.carriers(int(p)) if p >= 0 else []
        if c and not any(k == T for k, _ in c):
            cand.append((int(p), c[0]))
    if not cand:
        return 0, 0, 0, []
    P = np.array([hm.st[k]["points"][i] for _, (k, i) in cand], np.float64).reshape(-1, 3)
    N = np.array([hm.st[k]["normals"][i] for _, (k, i) in cand], np.float64).reshape(-1, 3)
    mind = np.array([hm.st[k]["min_dist"][i] for _, (k, i) in cand], f32)
    maxd = np.array([hm.st[k]["max_dist"][i] for _, (k, i) in cand], f32)
    pc = [((Tm[3 * r] * P[:, 0] + Tm[3 * r + 1] * P[:, 1]) + Tm[3 * r + 2] * P[:, 2]) + Tm[9 + r] for r in range(3)]
    Ow = [-((Tm[i] * Tm[9] + Tm[3 + i] * Tm[10]) + Tm[6 + i] * Tm[11]) for i in range(3)]
    with np.errstate(all="ignore"):
        z = pc[2].astype(f32)
        invz = f32(1.0) / z
        u = CAM6[0] * (pc[0].astype(f32) * invz) + CAM6[2]
        v = CAM6[1] * (pc[1].astype(f32) * invz) + CAM6[3]
        line = [P[:, c] + -Ow[c] for c in range(3)]
        dist = np.sqrt((line[0] * line[0] + line[1] * line[1]) + line[2] * line[2]).astype(f32)
        dot = (line[0] * N[:, 0] + line[1] * N[:, 1]) + line[2] * N[:, 2]
        q = np.log((maxd / dist).astype(np.float64)).astype(f32) / f32(np.log(np.float64(SF[1])))
        level = np.clip(np.ceil(q), 0, len(SF) - 1).astype(np.int32)
        ok = (z >= 0) & (u >= BOUNDS[0]) & (v >= BOUNDS[2]) & (u < BOUNDS[1]) & (v < BOUNDS[3]) & ~(dist < f32(0.8) * mind) & \
            ~(dist > f32(1.2) * maxd) & ~(dot < 0.5 * dist.astype(np.float64))
    gpw, gph = f32(GRID_COLS) / f32(BOUNDS[1] - BOUNDS[0]), f32(GRID_ROWS) / f32(BOUNDS[3] - BOUNDS[2])
    x, y, octave, desc, gx, gy = kfT["x"], kfT["y"], kfT["octave"], kfT["desc"], kfT["gx"], kfT["gy"]
    matches = adds = 0
    replaces = []
    for c in np.nonzero(ok)[0]:
        p = cand[c][0]
        lv, uu, vv = int(level[c]), u[c], v[c]
        r = threshold * SF[lv]
        x0, x1 = max(0, int(np.floor((uu - f32(BOUNDS[0]) - r) * gpw))), min(GRID_COLS - 1, int(np.floor((uu - f32(BOUNDS[0]) + r) * gpw)))
        y0, y1 = max(0, int(np.floor((vv - f32(BOUNDS[2]) - r) * gph))), min(GRID_ROWS - 1, int(np.floor((vv - f32(BOUNDS[2]) + r) * gph)))
        if x0 >= GRID_COLS or x1 < 0 or y0 >= GRID_ROWS or y1 < 0:
            continue
        w = (gx >= x0) & (gx <= x1) & (gy >= y0) & (gy <= y1) & (np.abs(uu - x) < r) & (np.abs(vv - y) < r) & (octave >= lv - 1) & (octave <= lv)
        idx = np.nonzero(w)[0]
        if not len(idx):
            continue
        d = POP[desc[idx] ^ hm.st[cand[c][1][0]]["point_desc"][cand[c][1][1]][None, :]].sum(1, dtype=np.int32)
        order = np.lexsort((idx, gy[idx], gx[idx], d))          # the strictly smallest distance in the visiting order
        best = int(idx[order[0]])
        if d[order[0]] > TH_LOW:
            continue
        matches += 1
        org = int(st["ids"][best])
        if (st["flags"][best] & 1) and org >= 0:
            replaces.append((org, p))
        else:
            hm.take(T, best, p, hm.attributes(p))
            adds += 1
    return int(ok.sum()), matches, adds, replaces


def host_search_and_fuse(store, corr, poses12, ids, static, n):
    """the route a store caller had: get_points / get_point_refs for the corrected key-frames, the replay of
    LoopClosing::searchAndFuse (loopClosing.cpp:496-516) on that copy, update_points / set_normals / set_point_refs back"""
    st = {}
    for k in corr:
        st[k] = store.points(k, n)
        st[k]["ref"] = store.point_refs(k, n)
    hm = HostMap(st)
    hm.recent = {e[0]: [e[1], e[2], e[3]] for e in store.recent_points()}
    before = {p: list(e) for p, e in hm.recent.items()}
    per = []
    for T in corr:
        passed, matches, adds, replaces = host_fuse_by_pose(T, poses12[T], ids, hm, static)
        moved = cleared = 0
        for A, B in replaces:
            if A == B:
                continue
            car = hm.carriers(A)
            holds_b = {k for k, _ in hm.carriers(B)}
            takes = sum(1 for k, _ in hm.observations(car) if k not in holds_b)
            moved, cleared = moved + (1 if takes else 0), cleared + len(car) - takes
            host_replace(A, B, hm, static, hm.recent)
        per.append((passed, matches, adds, len(replaces), moved, cleared))
    for k in corr:
        s = st[k]
        store.update_points(k, s["flags"], s["points"], s["ids"], s["point_desc"], s["min_dist"], s["max_dist"])
        store.set_normals(k, s["normals"])
        store.set_point_refs(k, s["ref"])
    grown = [(p, e[2] - before[p][2], e[1] - before[p][1]) for p, e in hm.recent.items() if e != before[p]]
    if grown:
        store.add_point_stats([g[0] for g in grown], [g[1] for g in grown], [g[2] for g in grown])
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=500)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--loop-keyframes", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--stale", action="store_true", help="with --once: the index is stale when the call begins (an update_points before it)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from vo_slam_test_amd import _lib as vo
    import pose_graph_store_ref as pr
    from loop_fuse_ref import pose_from_sim3
    K, n, R = a.keyframes, a.features, 4096
    assert K >= SCENE
    rng = np.random.default_rng(1)
    kfs = scene_keyframes(rng, K, n)
    for k in range(K - SCENE, K):      # the map side of tools/point_upkeep_bench.py
        kf = kfs[k]
        T = np.array(kf["pose"])
        Rm, t = T[:9].reshape(3, 3), T[9:]
        z = np.where(kf["depth"] >= 0, kf["depth"], f32(6.0)).astype(np.float64)
        pc = np.stack([(kf["xy"][:, 0] - 320.0) * z / 500.0, (kf["xy"][:, 1] - 240.0) * z / 500.0, z], 1)
        kf["points"] = np.where((kf["flags"] & 1)[:, None] > 0, (pc - t) @ Rm, 0.0)
    krng = np.random.default_rng(3)    # a seeded third of the scene's map-point features comes in WITHOUT its map point
    for k in range(K - SCENE, K):
        kf = kfs[k]
        gone = ((kf["flags"] & 1) > 0) & (krng.random(n) < 1 / 3)
        kf["flags"], kf["ids"] = np.where(gone, 0, kf["flags"]).astype(kf["flags"].dtype), np.where(gone, -1, kf["ids"]).astype(kf["ids"].dtype)
        kf["points"] = np.where(gone[:, None], 0.0, kf["points"])
    corr = list(range(K - SCENE, K))
    S_corr = np.array([pr.from_pose([float(x) for x in kfs[k]["pose"]]) for k in corr], np.float64)
    poses12 = {k: pose_from_sim3([float(x) for x in S]) for k, S in zip(corr, S_corr)}
    ids = []
    for k in corr[:a.loop_keyframes]:
        ids += [int(p) for p, f in zip(kfs[k]["ids"], kfs[k]["flags"]) if (f & 1) and p >= 0]
    ids = np.array(list(dict.fromkeys(ids)), np.int32)
    stream = torch.cuda.Stream()
    arrays = lambda kf: {key: kf[key] for key in ("angle", "desc", "nodes", "flags", "points", "ids", "point_desc", "min_dist", "max_dist")}
    with torch.cuda.stream(stream):
        dev = tuple(torch.from_numpy(x).cuda() for x in (np.array(corr, np.int32), S_corr, ids))
    stream.synchronize()

    def build():
        s = vo.KeyFrameStore(K, n, stream=stream.cuda_stream)
        s.enable_connections(), s.enable_culling(), s.enable_mapping(CAM6, SF, FIRST_ID), s.enable_local_ba(64, 8192, 65536)
        s.enable_point_upkeep(R), s.enable_fuse(BOUNDS, 60 * n), s.enable_loop_fuse(len(corr), len(ids))
        for k, kf in enumerate(kfs):
            s.insert(arrays(kf))
            s.set_keypoints(k, kf["octave"], kf["depth"], kf["u_right"])
            s.set_keypoint_xy(k, kf["xy"])
            if kf["pose"] is not None:
                s.set_pose(k, kf["pose"])
                s.process_new_keyframe(k)
        s.update_connections(corr)     # (the index is fresh when the timed call begins)
        stream.synchronize()
        return s

    def timed(fn, reps):
        rows = []
        for r in range(reps + 1):
            s = build()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            fn(s)
            e1.record(stream)
            stream.synchronize()
            if r:                      # (the first run is the warm-up)
                rows.append(((time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)))
        r = np.array(rows)
        return dict(total_ms=dict(median=float(np.median(r[:, 0])), min=float(r[:, 0].min()), max=float(r[:, 0].max())),
                    event_ms=dict(median=float(np.median(r[:, 1])), min=float(r[:, 1].min()), max=float(r[:, 1].max())))

    device_call = lambda st: st.search_and_fuse(dev[0], dev[1], dev[2], float(TH))
    s = build()
    if a.build_only:
        return
    if a.stale:
        p0 = s.points(0, n)
        s.update_points(0, p0["flags"], p0["points"], p0["ids"], p0["point_desc"], p0["min_dist"], p0["max_dist"])
    device_call(s)
    stream.synchronize()
    if a.once:
        return
    result = s.loop_fuse_result()
    if s.connections_status() != 0 or not result["totals"][1]:
        sys.exit(f"loop_fuse_bench: the call matched nothing or raised a sticky bit ({result['totals']}); nothing is reported")

    # ---- the host route on a second store with the same history: it must leave the same store
    gpw, gph = f32(GRID_COLS) / f32(BOUNDS[1] - BOUNDS[0]), f32(GRID_ROWS) / f32(BOUNDS[3] - BOUNDS[2])
    cell = lambda c, lo, g: np.floor(((c - f32(lo)) * g).astype(np.float64) + 0.5).astype(np.int32)      # round(), half away from zero (c >= lo)
    static = {k: dict(desc=kfs[k]["desc"], u_right=kfs[k]["u_right"], octave=kfs[k]["octave"].astype(np.int32), x=kfs[k]["xy"][:, 0].astype(f32),
                      y=kfs[k]["xy"][:, 1].astype(f32), gx=cell(kfs[k]["xy"][:, 0].astype(f32), BOUNDS[0], gpw),
                      gy=cell(kfs[k]["xy"][:, 1].astype(f32), BOUNDS[2], gph)) for k in corr}
    host_step = lambda st: host_search_and_fuse(st, corr, poses12, ids, static, n)
    h = build()
    per = host_step(h)
    stream.synchronize()
    diff = [] if per == result["per_pass"] else [("per_pass", per[:3], result["per_pass"][:3])]
    for k in corr:
        pd, ph = s.points(k, n), h.points(k, n)
        diff += [(k, key) for key in pd if pd[key].tobytes() != ph[key].tobytes()]
        diff += [(k, "ref_kf")] if s.point_refs(k, n).tobytes() != h.point_refs(k, n).tobytes() else []
    diff += [] if s.recent_points() == h.recent_points() else ["recent list"]
    if diff:
        sys.exit(f"loop_fuse_bench: the device call and the host route left different stores ({diff[:6]}); nothing is reported")

    res = dict(tool="loop_fuse_bench", keyframes=K, features_per_keyframe=n, reps=a.reps, version=vo.lib().vo_version().decode(),
               corrected_keyframes=len(corr), loop_points=int(len(ids)), totals=dict(zip(vo.KeyFrameStore.LOOP_FUSE_COLUMNS, result["totals"])))
    res["search_and_fuse_device"] = timed(device_call, a.reps)
    res["search_and_fuse_host_route"] = timed(host_step, a.reps)
    del res["search_and_fuse_host_route"]["event_ms"]
    res["speedup"] = res["search_and_fuse_host_route"]["total_ms"]["median"] / res["search_and_fuse_device"]["total_ms"]["median"]
    print(json.dumps(res))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
