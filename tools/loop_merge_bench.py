#!/usr/bin/env python3
"""The merge of the loop matches (loopClosing.cpp:439-455) that the loop-merge layer runs on the device (DESIGN.md sections 4s, 7),
beside the route a store caller had before it existed:
  device   vo_kfstore_merge_loop_matches_dev: two memsets and four launches (the observation index is built beforehand, outside
           the timed call), timed until the stream has drained and between two events on it
  host     the same work driven from the host with the entry points of the parent commit: get_points / get_point_refs of every
           key-frame that carries an A or a B (the caller knows who holds what), replaceMapPoint / addMapPoint / computeDescriptor
           replayed in numpy, update_points / set_normals / set_point_refs back
Store: --keyframes key-frames of --features features on a line, each seeing a window of the points that moves by a twentieth per
key-frame (a point has about twenty holders).  The last key-frame is current; --matches of its features are matched to points
of the first key-frames' windows, half of them live features (replaces: every holder of the feature's point goes over) and half
features without a point (adds).  A merge cannot be undone, so every repetition runs on a freshly built store (not timed).
Before timing, one store of each route is held against the other byte for byte -- flags, ids, points, normals, min / max,
point_desc and ref_kf of every key-frame -- and the tool stops if they differ.
usage: tools/loop_merge_bench.py [--keyframes 500] [--features 1000] [--matches 300] [--reps 5] [--no-host] [--out FILE]"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

f32 = np.float32
CAM6 = np.array([500.0, 500.0, 320.0, 240.0, 40.0, 0.08], f32)
SF = np.cumprod(np.array([1.0] + [1.2] * 7, f32), dtype=f32)
FIRST_ID, BA_CAPS = 1 << 24, (64, 8192, 65536)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int32)


def make_keyframes(K, n, n_match):
    """-> (key-frames, match_ids of the last one)"""
    step = max(n // 20, 1)
    rng = np.random.default_rng(2)
    P = np.stack([rng.uniform(-3, 3, step * K + n), rng.uniform(-2, 2, step * K + n), rng.uniform(4, 9, step * K + n)], 1)
    kfs = []
    for k in range(K):
        ids = (step * k + np.arange(n)).astype(np.int32)
        flags = np.full(n, 3, np.uint8)
        if k == K - 1:      # the second half of the matched features holds no point
            ids[n - n_match // 2:], flags[n - n_match // 2:] = -1, 0
        c = np.array([0.02 * k, 0.0, 0.0])
        nrm = P[np.maximum(ids, 0)] - c
        kfs.append(dict(angle=np.zeros(n, f32), desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), nodes=np.zeros(n, np.int32),
                        point_desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), min_dist=np.full(n, 0.1, f32) + f32(0.001) * f32(k % 7),
                        max_dist=np.full(n, 50.0, f32), flags=flags, points=P[np.maximum(ids, 0)] + 1e-6 * k, ids=ids,
                        normals=nrm / np.linalg.norm(nrm, axis=1)[:, None], octave=np.zeros(n, np.int32), depth=np.full(n, -1.0, f32),
                        u_right=np.full(n, -1.0, f32), xy=np.zeros((n, 2), f32), refs=np.where(ids >= 0, k, -1).astype(np.int32),
                        pose=[1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, -0.02 * k, 0.0, 0.0]))
    match = np.full(n, -1, np.int32)
    match[n - n_match:] = rng.permutation(n)[:n_match]      # distinct points of the first key-frames' windows
    return kfs, match


def build_store(vo, kfs, stream, merge):
    K, n = len(kfs), len(kfs[0]["ids"])
    s = vo.KeyFrameStore(K, n, stream=stream.cuda_stream)
    s.enable_connections(), s.enable_culling(), s.enable_mapping(CAM6, SF, FIRST_ID), s.enable_local_ba(*BA_CAPS)
    s.enable_point_upkeep(64), s.enable_fuse(BOUNDS, 1024), s.enable_loop_fuse(64, 4096)
    if merge:
        s.enable_loop_merge()
    for k, kf in enumerate(kfs):
        s.insert({key: kf[key] for key in ("angle", "desc", "nodes", "flags", "points", "ids", "point_desc", "min_dist", "max_dist")})
        s.set_keypoints(k, kf["octave"], kf["depth"], kf["u_right"])
        s.set_keypoint_xy(k, kf["xy"])
        s.set_pose(k, kf["pose"])
        s.set_normals(k, kf["normals"])
        s.set_point_refs(k, kf["refs"])
    s.update_connections([0])   # (the index is built here, outside the timed calls)
    return s


def median_row(rows):
    """MapPoint::computeDescriptor's choice (mappoint.cpp:145-173): the first row with the least median distance"""
    D = POPCOUNT[rows[:, None, :] ^ rows[None, :, :]].sum(2)
    return int(np.argmin(np.sort(D, 1)[:, (len(rows) - 1) // 2]))


def host_merge(s, kfs, curr, match):
    """the merge with the parent commit's entry points -> (adds, replaces)"""
    K, n = len(kfs), len(kfs[0]["ids"])
    cur_ids, cur_live = kfs[curr]["ids"], (kfs[curr]["flags"] & 1).astype(bool)
    steps = np.nonzero(match >= 0)[0]
    wanted = set(int(b) for b in match[steps]) | set(int(cur_ids[i]) for i in steps if cur_live[i])
    want = np.array(sorted(wanted), np.int32)
    held = {}
    for k, kf in enumerate(kfs):      # every key-frame that carries an A or a B comes down
        if k == curr or np.isin(kf["ids"], want).any():
            held[k] = dict(s.points(k, n), ref=s.point_refs(k, n))
    cols = ("points", "normals", "min_dist", "max_dist", "ref", "point_desc")

    def carriers(p):
        return [(k, int(i)) for k in sorted(held) for i in np.nonzero((held[k]["ids"] == p) & ((held[k]["flags"] & 1) != 0))[0]]

    def descriptor(p):
        c = carriers(p)
        obs = {}
        for k, i in c:
            obs.setdefault(k, i)
        rows = np.stack([kfs[k]["desc"][i] for k, i in sorted(obs.items())])
        win = rows[median_row(rows)]
        for k, i in c:
            held[k]["point_desc"][i] = win

    adds = replaces = 0
    for i in steps:
        B, h = int(match[i]), held[curr]
        cb = carriers(B)
        if not cb:
            continue
        src = {c: held[cb[0][0]][c][cb[0][1]].copy() for c in cols}
        if (h["flags"][i] & 1) and h["ids"][i] >= 0:
            A = int(h["ids"][i])
            if A == B:
                continue
            replaces += 1
            holds_b, seen = {k for k, _ in cb}, set()
            for k, f in carriers(A):
                if k in seen or k in holds_b:
                    held[k]["flags"][f] &= 0xfe
                else:
                    held[k]["ids"][f] = B
                    for c in cols:
                        held[k][c][f] = src[c]
                seen.add(k)
        else:
            adds += 1
            h["ids"][i], h["flags"][i] = B, h["flags"][i] | 1
            for c in cols:
                h[c][i] = src[c]
        descriptor(B)
    for k, h in held.items():
        s.update_points(k, h["flags"], h["points"], h["ids"], h["point_desc"], h["min_dist"], h["max_dist"])
        s.set_normals(k, h["normals"])
        s.set_point_refs(k, h["ref"])
    return adds, replaces


def state(s, K, n):
    out = []
    for k in range(K):
        p = s.points(k, n)
        out.append({key: np.asarray(v).tobytes() for key, v in p.items()})
        out[-1]["ref"] = s.point_refs(k, n).tobytes()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=500)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--matches", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from vo_slam_test_amd import _lib as vo
    K, n = a.keyframes, a.features
    kfs, match = make_keyframes(K, n, a.matches)
    curr = K - 1
    stream = torch.cuda.Stream()
    dev_match = torch.from_numpy(match).cuda()

    def clock(fn):
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        out = fn()
        e1.record(stream)
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1), out

    rows = {key: [] for key in ("device", "device_event", "host")}
    rec = None
    for rep in range(a.reps + 1):   # (the first repetition warms up and holds the two routes against each other)
        s = build_store(vo, kfs, stream, True)
        t, ev, _ = clock(lambda: s.merge_loop_matches(curr, dev_match))
        rows["device"].append(t), rows["device_event"].append(ev)
        rec = s.loop_merge_result()["record"]
        if rec["undone"] or rec["n_dead"] or s.connections_status() != 0:
            sys.exit("loop_merge_bench: the device call left steps undone (%r); nothing is reported" % (rec,))
        if not a.no_host:
            h = build_store(vo, kfs, stream, False)
            t, _, (adds, replaces) = clock(lambda: host_merge(h, kfs, curr, match))
            rows["host"].append(t)
            if rep == 0 and ((adds, replaces) != (rec["adds"], rec["replaces"]) or state(s, K, n) != state(h, K, n)):
                sys.exit("loop_merge_bench: the device's store and the host route's differ; nothing is reported")
            h.close()
        s.close()
    med = {key: float(np.median(v[1:])) for key, v in rows.items() if len(v) > 1}
    spread = {key: float((max(v[1:]) - min(v[1:])) / np.median(v[1:])) for key, v in rows.items() if len(v) > 1}
    res = dict(tool="loop_merge_bench", keyframes=K, features_per_keyframe=n, matches=a.matches, reps=a.reps, version=vo.lib().vo_version().decode(),
               record=rec, launches=dict(memsets=2, kernels=4), median_ms=med, spread=spread, stores_equal=not a.no_host)
    if not a.no_host:
        res["host_route_over_device"] = med["host"] / med["device"]
    print(json.dumps(res))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
