#!/usr/bin/env python3
"""LocalMapping::searchInNeighbors for a key-frame store (DESIGN.md sections 4m, 7):
  device  vo_kfstore_search_in_neighbors: nothing but launches (one memset, the fixed 61 fuse steps, the closing rebuild,
          descriptors, refresh and connection update)
  host    the only route a store caller had before: the ordered lists, vo_kfstore_get_points and get_point_refs for `current`
          and every distinct key-frame of the target list, the replay of searchInNeighbors / fuseMapPoints / replaceMapPoint on
          that copy in numpy / Python (what include/myslam_shim/matcher_hip.inl replays on the reference's objects: the gates of
          a step's candidates at once, the window search per candidate over the target's features, the mutation in list order
          with an index of the copy by id), then vo_kfstore_update_points, set_normals and set_point_refs for the same
          key-frames and vo_kfstore_update_connections for `current`.
The two forms' target lists, match counts, flags, ids, points, point_desc, normals, min / max, ref_kf, recent lists and
connections are compared first and the tool stops if they differ.
Store: --keyframes key-frames of --features features; the last 12 are tools/new_points_bench.py's scene with the map side of
tools/point_upkeep_bench.py, every scene key-frame processed as it came in; the timed call is the last key-frame's.  A call
cannot be undone, so every repetition runs on a freshly built store (not timed).  Reported: median, min and max of --reps
calls, until the stream has drained (`total_ms`) and between two events (`event_ms`), and the call's result record.
--once builds one store and runs a single call, --build-only builds the store alone: the difference of the kernel counts of
two kernel-trace runs is the call's launches (k_obs_fill: one per index rebuild); --stale makes the index stale first.
usage: tools/fuse_bench.py [--keyframes 500] [--features 1000] [--reps 20] [--once [--stale] | --build-only] [--out FILE]"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402

from new_points_bench import CAM6, FIRST_ID, SCENE, SF, scene_keyframes  # noqa: E402
from point_upkeep_bench import host_refresh  # noqa: E402

f32 = np.float32
BOUNDS = (0.0, 640.0, 0.0, 480.0)


POP = np.array([bin(x).count("1") for x in range(256)], np.uint8)
GRID_COLS, GRID_ROWS, TH_LOW = 64, 48, 50


class HostMap:
    """the host copy of the downloaded key-frames indexed by id: the live carriers of every id, ascending in (key-frame, feature),
    kept current through the replay (what the reference's observedKFs_ / mappoints_ pointers are)"""

    def __init__(self, st):
        self.st, self.car = st, {}
        for k in sorted(st):
            live = np.nonzero(((st[k]["flags"] & 1) > 0) & (st[k]["ids"] >= 0))[0]
            for i in live:
                self.car.setdefault(int(st[k]["ids"][i]), []).append((k, int(i)))

    def carriers(self, p):
        return self.car.get(p, [])

    @staticmethod
    def observations(carriers):
        out, prev = [], -1
        for k, i in carriers:
            if k != prev:
                out.append((k, i))
            prev = k
        return out

    def attributes(self, p):
        k, i = self.car[p][0]
        s = self.st[k]
        return tuple(np.array(s[key][i]) for key in ("points", "normals", "min_dist", "max_dist", "ref", "point_desc"))

    def take(self, k, i, p, a):
        s = self.st[k]
        s["ids"][i] = p
        s["flags"][i] |= 1
        for key, v in zip(("points", "normals", "min_dist", "max_dist", "ref", "point_desc"), a):
            s[key][i] = v
        lst = self.car.setdefault(p, [])
        lst.append((k, i))
        lst.sort()

    def clear(self, k, i, p):
        self.st[k]["flags"][i] &= 0xFE
        self.car[p].remove((k, i))


def host_descriptor(p, hm, static):
    """MapPoint::computeDescriptor (mappoint.cpp:118-179) on the copy (no key-frame of the bench is bad)"""
    live = hm.carriers(p)
    holders = hm.observations(live)
    if not holders:
        return
    desp = np.stack([static[j]["desc"][i] for j, i in holders])
    n = len(desp)
    dist = POP[desp[:, None, :] ^ desp[None, :, :]].sum(2, dtype=np.int32)
    win = desp[int(np.argmin(np.sort(dist, 1)[:, int(0.5 * (n - 1))]))]
    for j, i in live:
        hm.st[j]["point_desc"][i] = win


def host_replace(A, B, hm, static, recent):
    """MapPoint::replaceMapPoint (mappoint.cpp:214-253) on the copy, with DESIGN.md section 4m's choices"""
    a = hm.attributes(B)
    all_a = list(hm.carriers(A))
    obs_a = hm.observations(all_a)
    holds_b = {k for k, _ in hm.carriers(B)}
    for k, i in all_a:
        hm.clear(k, i, A)
        if (k, i) in obs_a and k not in holds_b:
            hm.take(k, i, B, a)
    if A in recent and B in recent:
        recent[B][1] += recent[A][1]
        recent[B][2] += recent[A][2]
    host_descriptor(B, hm, static)


def host_fuse(T, ids, hm, static, poses, threshold=f32(3.0)):
    """Matcher::fuseMapPoints (matcher.cpp:1012-1133) on the copy: the gates of every first occurrence at once in numpy (they
    read nothing an earlier match of the call changes: section 4m's derivations), then search and mutation in list order"""
    st, kfT = hm.st[T], static[T]
    cand, seen = [], set()
    for p in ids:
        p = int(p)
        if p < 0 or p in seen:
            continue
        seen.add(p)
        c = hm.carriers(p)
        if c and not any(k == T for k, _ in c):
            cand.append((p, c[0]))
    if not cand:
        return 0
    P = np.array([hm.st[k]["points"][i] for _, (k, i) in cand], np.float64).reshape(-1, 3)
    N = np.array([hm.st[k]["normals"][i] for _, (k, i) in cand], np.float64).reshape(-1, 3)
    mind = np.array([hm.st[k]["min_dist"][i] for _, (k, i) in cand], f32)
    maxd = np.array([hm.st[k]["max_dist"][i] for _, (k, i) in cand], f32)
    Tm = [float(x) for x in poses[T]]
    pc = [((Tm[3 * r] * P[:, 0] + Tm[3 * r + 1] * P[:, 1]) + Tm[3 * r + 2] * P[:, 2]) + Tm[9 + r] for r in range(3)]
    Ow = [-((Tm[i] * Tm[9] + Tm[3 + i] * Tm[10]) + Tm[6 + i] * Tm[11]) for i in range(3)]
    with np.errstate(all="ignore"):
        z = pc[2].astype(f32)
        invz = f32(1.0) / z
        u = CAM6[0] * (pc[0].astype(f32) * invz) + CAM6[2]
        v = CAM6[1] * (pc[1].astype(f32) * invz) + CAM6[3]
        ur = u - CAM6[4] * invz
        line = [P[:, c] + -Ow[c] for c in range(3)]
        dist = np.sqrt((line[0] * line[0] + line[1] * line[1]) + line[2] * line[2]).astype(f32)
        dot = (line[0] * N[:, 0] + line[1] * N[:, 1]) + line[2] * N[:, 2]
        q = np.log((maxd / dist).astype(np.float64)).astype(f32) / f32(np.log(np.float64(SF[1])))
        level = np.clip(np.ceil(q), 0, len(SF) - 1).astype(np.int32)
        ok = (z >= 0) & (u >= BOUNDS[0]) & (v >= BOUNDS[2]) & (u < BOUNDS[1]) & (v < BOUNDS[3]) & ~(dist < f32(0.8) * mind) & \
            ~(dist > f32(1.2) * maxd) & ~(dot < 0.5 * dist.astype(np.float64))
    gpw, gph = f32(GRID_COLS) / f32(BOUNDS[1] - BOUNDS[0]), f32(GRID_ROWS) / f32(BOUNDS[3] - BOUNDS[2])
    x, y, octave, uright, desc = kfT["x"], kfT["y"], kfT["octave"], kfT["u_right"], kfT["desc"]
    gx, gy = kfT["gx"], kfT["gy"]
    inv = f32(1.0) / SF[np.clip(octave, 0, len(SF) - 1)]
    cnt = 0
    for c in np.nonzero(ok)[0]:
        p = cand[c][0]
        lv, uu, vv = int(level[c]), u[c], v[c]
        r = threshold * SF[lv]
        x0, x1 = max(0, int(np.floor((uu - f32(BOUNDS[0]) - r) * gpw))), min(GRID_COLS - 1, int(np.floor((uu - f32(BOUNDS[0]) + r) * gpw)))
        y0, y1 = max(0, int(np.floor((vv - f32(BOUNDS[2]) - r) * gph))), min(GRID_ROWS - 1, int(np.floor((vv - f32(BOUNDS[2]) + r) * gph)))
        if x0 >= GRID_COLS or x1 < 0 or y0 >= GRID_ROWS or y1 < 0:
            continue
        ex, ey = uu - x, vv - y
        w = (gx >= x0) & (gx <= x1) & (gy >= y0) & (gy <= y1) & (np.abs(ex) < r) & (np.abs(ey) < r) & (octave >= lv - 1) & (octave <= lv)
        if not w.any():
            continue
        er = ur[c] - uright
        stereo = uright >= 0
        chi = np.where(stereo, (ex * ex + ey * ey + er * er) * inv * inv, (ex * ex + ey * ey) * inv * inv)
        w &= ~(chi > np.where(stereo, f32(7.815), f32(5.991)))
        idx = np.nonzero(w)[0]
        if not len(idx):
            continue
        d = POP[desc[idx] ^ hm.st[cand[c][1][0]]["point_desc"][cand[c][1][1]][None, :]].sum(1, dtype=np.int32)
        order = np.lexsort((idx, gy[idx], gx[idx], d))          # the strictly smallest distance in the visiting order
        best = int(idx[order[0]])
        if d[order[0]] > TH_LOW:
            continue
        cnt += 1
        cur_c = hm.carriers(p)
        if not cur_c or any(k == T for k, _ in cur_c):
            continue
        org = int(st["ids"][best])
        if (st["flags"][best] & 1) and org >= 0:
            obs = lambda car: sum(2 if static[k]["u_right"][i] >= 0 else 1 for k, i in hm.observations(car))
            if obs(hm.carriers(org)) > obs(cur_c):
                host_replace(p, org, hm, static, hm.recent)
            else:
                host_replace(org, p, hm, static, hm.recent)
        else:
            hm.take(T, best, p, hm.attributes(p))
    return cnt


def host_search_in_neighbors(store, cur, static, poses, n, host_refresh):
    """the route a store caller had: the ordered lists, get_points / get_point_refs for `current` and every target, the replay
    of LocalMapping::searchInNeighbors (localMapping.cpp:363-432) on that copy, update_points / set_normals / set_point_refs back,
    and the connection update"""
    order = lambda k: store.connections(k)["ordered"]
    targets, marked = [], set()
    for kfn in order(cur)[:10]:
        if kfn in marked:
            continue
        targets.append(kfn)
        marked.add(kfn)
        targets += [kfs for kfs in order(kfn)[:5] if kfs not in marked and kfs != cur]
    touched = sorted(set(targets) | {cur})
    st = {}
    for k in touched:
        st[k] = store.points(k, n)
        st[k]["ref"] = store.point_refs(k, n)
    hm = HostMap(st)
    hm.recent = {e[0]: [e[1], e[2], e[3]] for e in store.recent_points()}
    before = {p: list(e) for p, e in hm.recent.items()}
    live = lambda k: [int(p) for p, f in zip(st[k]["ids"], st[k]["flags"]) if (f & 1) and p >= 0]
    snapshot = live(cur)
    matches = sum(host_fuse(T, snapshot, hm, static, poses) for T in targets)
    cand = list(dict.fromkeys(p for T in targets for p in live(T)))
    matches += host_fuse(cur, cand, hm, static, poses)
    for p in dict.fromkeys(live(cur)):
        host_descriptor(p, hm, static)
        host_refresh(p, hm, st, static, poses)
    for k in touched:
        s = st[k]
        store.update_points(k, s["flags"], s["points"], s["ids"], s["point_desc"], s["min_dist"], s["max_dist"])
        store.set_normals(k, s["normals"])
        store.set_point_refs(k, s["ref"])
    grown = [(p, e[2] - before[p][2], e[1] - before[p][1]) for p, e in hm.recent.items() if e != before[p]]
    if grown:
        store.add_point_stats([g[0] for g in grown], [g[1] for g in grown], [g[2] for g in grown])
    store.update_connections([cur])
    return targets, touched, matches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=500)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--stale", action="store_true", help="with --once: the index is stale when the call begins (an update_points before it)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from vo_slam_test_amd import _lib as vo
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
    # a seeded third of the scene's map-point features comes in WITHOUT its map point: what the fuse steps find and add
    krng = np.random.default_rng(3)
    for k in range(K - SCENE, K):
        kf = kfs[k]
        gone = ((kf["flags"] & 1) > 0) & (krng.random(n) < 1 / 3)
        kf["flags"], kf["ids"] = np.where(gone, 0, kf["flags"]).astype(kf["flags"].dtype), np.where(gone, -1, kf["ids"]).astype(kf["ids"].dtype)
        kf["points"] = np.where(gone[:, None], 0.0, kf["points"])
    cur = K - 1
    stream = torch.cuda.Stream()
    arrays = lambda kf: {key: kf[key] for key in ("angle", "desc", "nodes", "flags", "points", "ids", "point_desc", "min_dist", "max_dist")}

    def build():
        s = vo.KeyFrameStore(K, n, stream=stream.cuda_stream)
        s.enable_connections(), s.enable_culling(), s.enable_mapping(CAM6, SF, FIRST_ID), s.enable_local_ba(64, 8192, 65536)
        s.enable_point_upkeep(R), s.enable_fuse(BOUNDS, 60 * n)
        for k, kf in enumerate(kfs):
            s.insert(arrays(kf))
            s.set_keypoints(k, kf["octave"], kf["depth"], kf["u_right"])
            s.set_keypoint_xy(k, kf["xy"])
            if kf["pose"] is not None:
                s.set_pose(k, kf["pose"])
                s.process_new_keyframe(k)
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

    s = build()
    if a.build_only:
        return
    if a.stale:
        p0 = s.points(0, n)
        s.update_points(0, p0["flags"], p0["points"], p0["ids"], p0["point_desc"], p0["min_dist"], p0["max_dist"])
    s.search_in_neighbors(cur)
    stream.synchronize()
    if a.once:
        return
    result = s.fuse_result()
    touched = sorted(set(result["targets"]))
    if s.connections_status() != 0 or not result["totals"][1]:
        sys.exit(f"fuse_bench: the call matched nothing or raised a sticky bit ({result['totals']}); nothing is reported")

    # ---- the host route on a second store with the same history: it must leave the same store
    gpw, gph = f32(GRID_COLS) / f32(BOUNDS[1] - BOUNDS[0]), f32(GRID_ROWS) / f32(BOUNDS[3] - BOUNDS[2])
    cell = lambda c, lo, g: np.floor(((c - f32(lo)) * g).astype(np.float64) + 0.5).astype(np.int32)      # round(), half away from zero (c >= lo)
    static = {k: dict(desc=kfs[k]["desc"], u_right=kfs[k]["u_right"], octave=kfs[k]["octave"].astype(np.int32), x=kfs[k]["xy"][:, 0].astype(f32),
                      y=kfs[k]["xy"][:, 1].astype(f32), gx=cell(kfs[k]["xy"][:, 0].astype(f32), BOUNDS[0], gpw),
                      gy=cell(kfs[k]["xy"][:, 1].astype(f32), BOUNDS[2], gph)) for k in range(K - SCENE, K)}
    poses = {k: kfs[k]["pose"] for k in range(K - SCENE, K)}
    host_step = lambda st: host_search_in_neighbors(st, cur, static, poses, n, host_refresh)
    h = build()
    targets, touched_h, host_matches = host_step(h)
    stream.synchronize()
    diff = [] if targets + [cur] == result["targets"] and touched_h == touched else ["target list"]
    diff += [] if host_matches == result["totals"][1] else [("matches", host_matches, result["totals"][1])]
    for k in touched:
        pd, ph = s.points(k, n), h.points(k, n)
        diff += [(k, key) for key in pd if pd[key].tobytes() != ph[key].tobytes()]
        diff += [(k, "ref_kf")] if s.point_refs(k, n).tobytes() != h.point_refs(k, n).tobytes() else []
    diff += [] if s.recent_points() == h.recent_points() else ["recent list"]
    diff += [] if [s.connections(k) for k in touched] == [h.connections(k) for k in touched] else ["connections"]
    if diff:
        sys.exit(f"fuse_bench: the device call and the host route left different stores ({diff[:6]}); nothing is reported")

    res = dict(tool="fuse_bench", keyframes=K, features_per_keyframe=n, reps=a.reps, version=vo.lib().vo_version().decode(),
               targets=len(result["targets"]) - 1, distinct_keyframes=len(touched), totals=dict(zip(vo.KeyFrameStore.FUSE_COLUMNS, result["totals"])))
    res["search_in_neighbors_device"] = timed(lambda st: st.search_in_neighbors(cur), a.reps)
    res["search_in_neighbors_host_route"] = timed(host_step, a.reps)
    del res["search_in_neighbors_host_route"]["event_ms"]
    res["speedup"] = res["search_in_neighbors_host_route"]["total_ms"]["median"] / res["search_in_neighbors_device"]["total_ms"]["median"]
    print(json.dumps(res))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
