#!/usr/bin/env python3
"""LocalMapping::processNewKeyFrame + cullingMapPoints and MapPoint::computeDescriptor for a key-frame store, both forms in
one process run on stores with the same history (DESIGN.md sections 4l, 7):
  device  vo_kfstore_process_new_keyframe + vo_kfstore_cull_map_points, and vo_kfstore_compute_descriptors_dev for --ids ids:
          nothing but launches
  host    the only route of a store caller before the device form existed: vo_kfstore_get_points (and get_point_refs) for every
          touched key-frame -- the current one and the key-frames connected to it or to one of the four before it --, the steps
          in numpy / Python on that copy (an index of the copy by id, the refresh in section 4k's operation order, the median
          by a popcount table), then vo_kfstore_update_points, set_normals and set_point_refs for the touched key-frames and
          vo_kfstore_update_connections for the current one (first: its weights name the touched key-frames).  The host keeps
          its own recent list.  In this scene every scene key-frame sees the same world, so the touched set is the scene so far.
Store: --keyframes key-frames of --features features; the last 12 are tools/new_points_bench.py's scene, the others filler
with ids of their own.  History: every scene key-frame but the last has been processed, counted (a seeded third of the listed
points is seen five times more and never found) and culled as it came in; the timed call is the last key-frame's.
The calls cannot be undone, so every repetition runs on a freshly built pair of stores (not timed).  The two forms' flags,
point_desc, normals, min / max, ref_kf and recent lists are compared first and the tool stops if they differ.
Measured as the median of --reps: `total_ms` until the stream has drained and (device) `event_ms` between two events.
usage: tools/point_upkeep_bench.py [--keyframes 500] [--features 1000] [--ids 1000] [--reps 5] [--out FILE]"""
import argparse
import json
import math
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402

from new_points_bench import CAM6, FIRST_ID, SCENE, SF, scene_keyframes  # noqa: E402

f32 = np.float32
POP = np.array([bin(x).count("1") for x in range(256)], np.uint8)
MAP_KEYS = ("flags", "ids", "points", "point_desc", "min_dist", "max_dist", "normals")


def median_row(desp):
    """mappoint.cpp:145-173 on an [N][32] array -> index"""
    n = len(desp)
    dist = POP[desp[:, None, :] ^ desp[None, :, :]].sum(2, dtype=np.int32)
    return int(np.argmin(np.sort(dist, 1)[:, int(0.5 * (n - 1))]))


class HostIndex:
    """the host copy of the touched key-frames indexed by id: carriers (every live feature) and observations (the lowest
    feature per key-frame), both ascending in (key-frame, feature)"""

    def __init__(self, T, st):
        kf = np.concatenate([np.full(len(st[k]["ids"]), k, np.int64) for k in T])
        ft = np.concatenate([np.arange(len(st[k]["ids"]), dtype=np.int64) for k in T])
        ids = np.concatenate([st[k]["ids"] for k in T]).astype(np.int64)
        live = (np.concatenate([st[k]["flags"] for k in T]) & 1).astype(bool) & (ids >= 0)
        order = np.lexsort((ft[live], kf[live], ids[live]))
        self.ids, self.kf, self.ft = ids[live][order], kf[live][order], ft[live][order]

    def carriers(self, p):
        lo, hi = np.searchsorted(self.ids, p, "left"), np.searchsorted(self.ids, p, "right")
        return [(int(self.kf[s]), int(self.ft[s])) for s in range(lo, hi)]

    @staticmethod
    def observations(carriers):
        out, prev = [], -1
        for k, i in carriers:
            if k != prev:
                out.append((k, i))
            prev = k
        return out


def center(T):
    return [-((T[i] * T[9] + T[3 + i] * T[10]) + T[6 + i] * T[11]) for i in range(3)]


def host_refresh(p, ix, st, static, poses):
    live = ix.carriers(p)
    holders = ix.observations(live)
    j0, i0 = live[0]
    pos = [float(x) for x in st[j0]["points"][i0]]
    r0 = int(st[j0]["ref"][i0])
    ref = r0 if any(j == r0 for j, _ in holders) else holders[0][0]
    s, lens = [0.0, 0.0, 0.0], {}
    for j, _ in holders:
        Ow = center(poses[j])
        d = [pos[c] + -Ow[c] for c in range(3)]
        ln = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        s = [s[c] + d[c] / ln for c in range(3)]
        lens[j] = ln
    iref = dict(holders)[ref]
    maxd = f32(lens[ref]) * SF[min(max(int(static[ref]["octave"][iref]), 0), len(SF) - 1)]
    nrm = [s[c] / float(len(holders)) for c in range(3)]
    for j, i in live:
        st[j]["ref"][i], st[j]["normals"][i] = ref, nrm
        st[j]["max_dist"][i], st[j]["min_dist"][i] = maxd, maxd / SF[len(SF) - 1]


def host_descriptor(p, ix, st, static):
    live = ix.carriers(p)
    holders = ix.observations(live)          # (no key-frame of the bench is bad)
    if not holders:
        return
    desp = np.stack([static[j]["desc"][i] for j, i in holders])
    win = desp[median_row(desp)]
    for j, i in live:
        st[j]["point_desc"][i] = win


def host_process_and_cull(store, T, static, poses, cur, recent, n, between=None):
    """get_points for the touched key-frames, the two steps on the copy (between: the counters of the history, which belong
    behind the process step), the copy back"""
    st = {}
    for k in T:
        st[k] = store.points(k, n)
        st[k]["ref"] = store.point_refs(k, n)
    ix = HostIndex(T, st)
    seen = set()
    for i in range(n):
        p = int(st[cur]["ids"][i])
        if not (st[cur]["flags"][i] & 1) or p < 0 or p in seen:
            continue
        seen.add(p)
        if any(j != cur for j, _ in ix.carriers(p)):
            host_refresh(p, ix, st, static, poses)
            host_descriptor(p, ix, st, static)
        elif p not in recent:
            recent[p] = [cur, 1, 1]
    if between:
        between(recent)
    for p in sorted(recent):
        first, found, visible = recent[p]
        live = ix.carriers(p)
        holders = ix.observations(live)
        obs = sum(2 if static[j]["u_right"][i] >= 0 else 1 for j, i in holders)
        with np.errstate(all="ignore"):
            low = bool(f32(found) / f32(visible) < f32(0.25))
        if not holders:
            del recent[p]
        elif low or (cur > first + 2 and obs <= 3):
            for j, i in live:
                st[j]["flags"][i] &= 0xFE
            del recent[p]
        elif cur > first + 3:
            del recent[p]
    for k in T:
        s = st[k]
        store.update_points(k, s["flags"], s["points"], s["ids"], s["point_desc"], s["min_dist"], s["max_dist"])
        store.set_normals(k, s["normals"])
        store.set_point_refs(k, s["ref"])


def host_descriptors(store, T, static, ids, n):
    st = {k: store.points(k, n) for k in T}
    ix = HostIndex(T, st)
    for p in ids:
        host_descriptor(int(p), ix, st, static)
    for k in T:
        s = st[k]
        store.update_points(k, s["flags"], s["points"], s["ids"], s["point_desc"], s["min_dist"], s["max_dist"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=500)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--ids", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from vo_slam_test_amd import _lib as vo
    K, n, R = a.keyframes, a.features, 4096
    assert K >= SCENE
    rng = np.random.default_rng(1)
    kfs = scene_keyframes(rng, K, n)
    for k in range(K - SCENE, K):      # a map side for the mapped points: the key-frame's own back-projection (6 m without a depth)
        kf = kfs[k]
        T = np.array(kf["pose"])
        Rm, t = T[:9].reshape(3, 3), T[9:]
        z = np.where(kf["depth"] >= 0, kf["depth"], f32(6.0)).astype(np.float64)
        pc = np.stack([(kf["xy"][:, 0] - 320.0) * z / 500.0, (kf["xy"][:, 1] - 240.0) * z / 500.0, z], 1)
        kf["points"] = np.where((kf["flags"] & 1)[:, None] > 0, (pc - t) @ Rm, 0.0)
    cur, first = K - 1, K - SCENE
    static = {k: dict(desc=kfs[k]["desc"], u_right=kfs[k]["u_right"], octave=kfs[k]["octave"]) for k in range(K)}
    poses = {k: kfs[k]["pose"] for k in range(first, K)}
    stream = torch.cuda.Stream()
    arrays = lambda kf: {key: kf[key] for key in ("angle", "desc", "nodes", "flags", "points", "ids", "point_desc", "min_dist", "max_dist")}
    srng = np.random.default_rng(2)
    stats = {k: srng.random(R) < 1 / 3 for k in range(first, K)}

    def touched(store, k):
        t = {k}
        for j in range(max(first, k - 4), k + 1):
            w = store.connections(j)["weights"]
            t |= {x for x in range(len(w)) if w[x] > 0}
        return sorted(t)

    def build(upkeep):
        """a store with the history; upkeep: the device form keeps the list, else the host does -> (store, host recent list)"""
        s = vo.KeyFrameStore(K, n, stream=stream.cuda_stream)
        s.enable_connections(), s.enable_culling(), s.enable_mapping(CAM6, SF, FIRST_ID), s.enable_local_ba(64, 8192, 65536)
        if upkeep:
            s.enable_point_upkeep(R)
        recent = {}
        for k, kf in enumerate(kfs):
            s.insert(arrays(kf))
            s.set_keypoints(k, kf["octave"], kf["depth"], kf["u_right"])
            s.set_keypoint_xy(k, kf["xy"])
            if kf["pose"] is None:
                continue
            s.set_pose(k, kf["pose"])
            if k == cur:
                break
            def counters(ids):
                low = stats[k][:len(ids)]
                return np.where(low, 5, 2).astype(np.int32), np.where(low, 0, 2).astype(np.int32)

            if upkeep:
                s.process_new_keyframe(k)
                ids = np.array([e[0] for e in s.recent_points()], np.int32)
                s.add_point_stats(ids, *counters(ids))
                s.cull_map_points(k)
            else:
                def between(rec):
                    ids = sorted(rec)
                    for p, v, f in zip(ids, *counters(ids)):
                        rec[p][2] += int(v)
                        rec[p][1] += int(f)

                s.update_connections([k])
                host_process_and_cull(s, touched(s, k), static, poses, k, recent, n, between)
        stream.synchronize()
        return s, recent

    def timed(make, fn, reps):
        rows = []
        for r in range(reps + 1):
            ctx = make()
            stream.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            fn(ctx)
            e1.record(stream)
            stream.synchronize()
            if r:                      # (the first run is the warm-up)
                rows.append(((time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)))
        r = np.array(rows)
        med = np.median(r, 0)
        return dict(total_ms=float(med[0]), event_ms=float(med[1]), spread=float((r[:, 0].max() - r[:, 0].min()) / med[0]),
                    runs_total_ms=[float(v) for v in r[:, 0]])

    def dev_step(ctx):
        ctx[0].process_new_keyframe(cur)
        ctx[0].cull_map_points(cur)

    def host_step(ctx):
        s, recent = ctx
        s.update_connections([cur])
        host_process_and_cull(s, touched(s, cur), static, poses, cur, recent, n)

    # ---- the two forms leave the same stores
    d, _ = build(True)
    h, recent = build(False)
    dev_step((d, None)), host_step((h, recent))
    stream.synchronize()
    T = touched(h, cur)
    diff = [] if d.recent_points() == [(p, e[0], e[1], e[2]) for p, e in sorted(recent.items())] else ["recent list"]
    for k in T:
        pd, ph = d.points(k, n), h.points(k, n)
        diff += [(k, key) for key in MAP_KEYS if pd[key].tobytes() != ph[key].tobytes()]
        diff += [(k, "ref_kf")] if d.point_refs(k, n).tobytes() != h.point_refs(k, n).tobytes() else []
    rec = d.upkeep_result()
    rec["erased"] = len(rec["erased"])
    if diff or d.connections_status() != 0:
        sys.exit(f"point_upkeep_bench: the device form and the host form left different stores ({diff[:6]}); nothing is reported")
    res = dict(tool="point_upkeep_bench", keyframes=K, features_per_keyframe=n, reps=a.reps, version=vo.lib().vo_version().decode(),
               max_recent=R, touched_keyframes=len(T), last_cull=rec, recent_after=len(recent))
    res["process_cull_device"] = timed(lambda: build(True), dev_step, a.reps)
    res["process_cull_host"] = timed(lambda: build(False), host_step, a.reps)
    del res["process_cull_host"]["event_ms"]
    res["process_cull_speedup"] = res["process_cull_host"]["total_ms"] / res["process_cull_device"]["total_ms"]
    # ---- compute_descriptors for --ids ids of the scene (idempotent: one pair of stores)
    held = np.unique(np.concatenate([kfs[k]["ids"][(kfs[k]["flags"] & 1) > 0] for k in range(first, K)]))
    ids = np.ascontiguousarray(np.resize(held, a.ids), np.int32)
    dev_ids = torch.from_numpy(ids).cuda()
    scene = list(range(first, K))
    d.compute_descriptors(dev_ids), host_descriptors(h, scene, static, ids, n)
    stream.synchronize()
    if any(d.points(k, n)["point_desc"].tobytes() != h.points(k, n)["point_desc"].tobytes() for k in scene):
        sys.exit("point_upkeep_bench: the two forms chose different descriptors; nothing is reported")
    res["descriptor_ids"] = int(a.ids)
    res["descriptors_device"] = timed(lambda: d, lambda s: s.compute_descriptors(dev_ids), a.reps)
    res["descriptors_host"] = timed(lambda: h, lambda s: host_descriptors(s, scene, static, ids, n), a.reps)
    del res["descriptors_host"]["event_ms"]
    res["descriptors_speedup"] = res["descriptors_host"]["total_ms"] / res["descriptors_device"]["total_ms"]
    print(json.dumps(res))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
