#!/usr/bin/env python3
"""Optimizer::solveLocalBAPoseAndPoint for a key-frame store, stage by stage, and the gather a store caller had to do
before the device form existed (DESIGN.md sections 4k, 7):
  window   vo_kfstore_local_ba_window: the observation index rebuilt (the write-back before it left it stale), then five
           launches on the store's stream (timed until the stream has drained, and between two events on it); and once more
           with the index in place
  solve    the round trip and the solver: vo_kfstore_local_ba_window_result (one copy of the whole window), vo_ba_reset,
           vo_ba_local_ba, vo_ba_get_state
  apply    vo_kfstore_local_ba_apply: one copy, two launches
  composed vo_kfstore_local_ba, all of it in one call
  host     the same window gathered on the host: vo_kfstore_get_points for EVERY key-frame (who holds a local point is
           not known before) and vo_kfstore_get_connections for the current one, then numpy (sort-based, no Python loop
           over features); poses, key-point columns and positions are the host's own copies, which such a caller keeps
Store: --keyframes key-frames of --features features.  The last 12 are views of one scene (1.6 x features points 4 .. 9 m in
front of cameras 0.3 m apart, 40 % of them mapped with a centimetre of noise, a third of the features stereo, half a pixel
of noise); the others are filler with ids of their own.  The current key-frame is the last one; its window has about ten
local cameras.  An apply cannot be undone, so before every repetition the map side and the poses of the scene's key-frames
are put back (not timed).  The host gather's cameras, points and edges are compared with the device window first and the
tool stops if they differ.  Per-kernel times come from a profiler run of this tool (rocprofv3 --kernel-trace --stats).
usage: tools/local_ba_store_bench.py [--keyframes 500] [--features 1000] [--reps 7] [--out FILE]"""
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
SCENE, FIRST_ID, CAPS = 12, 1 << 20, (64, 8192, 65536)


def scene_keyframes(rng, K, n):
    n_world = int(1.6 * n)
    Wp = np.stack([rng.uniform(-3, 6, n_world), rng.uniform(-2, 2, n_world), rng.uniform(4, 9, n_world)], 1)
    Wn = Wp + rng.normal(0, 0.01, Wp.shape)
    mapped = rng.random(n_world) < 0.4
    level = rng.integers(0, 4, n_world)
    kfs = []
    for k in range(K):
        s = k - (K - SCENE)
        kf = dict(angle=np.zeros(n, f32), desc=np.zeros((n, 32), np.uint8), nodes=np.zeros(n, np.int32), point_desc=np.zeros((n, 32), np.uint8),
                  min_dist=np.full(n, 0.1, f32), max_dist=np.full(n, 50.0, f32))
        if s < 0:   # filler: ids nobody else holds, no pose needed
            kf.update(flags=np.full(n, 3, np.uint8), points=np.zeros((n, 3)), ids=(FIRST_ID // 2 + k * n + np.arange(n)).astype(np.int32),
                      octave=np.zeros(n, np.int32), depth=np.full(n, -1.0, f32), u_right=np.full(n, -1.0, f32), xy=np.zeros((n, 2), f32), pose=None)
        else:
            c = np.array([0.3 * s, 0.02 * (s % 3), 0.0])
            th = 0.01 * (s - 6)
            R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
            seen = rng.permutation(n_world)[:n]
            pc = (R @ (Wp[seen] - c).T).T
            noise = rng.normal(0, 0.5, (n, 2))
            u, v = (500.0 * pc[:, 0] / pc[:, 2] + 320.0 + noise[:, 0]).astype(f32), (500.0 * pc[:, 1] / pc[:, 2] + 240.0 + noise[:, 1]).astype(f32)
            z = pc[:, 2].astype(f32)
            stereo = rng.random(n) < 0.33
            kf.update(flags=np.where(mapped[seen], 3, 0).astype(np.uint8), points=np.where(mapped[seen][:, None], Wn[seen], 0.0),
                      ids=np.where(mapped[seen], seen, -1).astype(np.int32), octave=level[seen].astype(np.int32),
                      depth=np.where(stereo, z, f32(-1)).astype(f32), u_right=np.where(stereo, u - f32(40.0) / z, f32(-1)).astype(f32),
                      xy=np.stack([u, v], 1).astype(f32), pose=[float(x) for x in R.reshape(-1)] + [float(x) for x in -(R @ c)])
        kfs.append(kf)
    return kfs


def host_gather(store, kfs, cur, n):
    """-> (cameras, point ids, e_cam, e_pt, e_feature) from downloads of the store"""
    K = len(kfs)
    held = [store.points(k, n) for k in range(K)]                      # every key-frame: flags, ids, points, ... come down
    ids = np.stack([h["ids"] for h in held])
    live = np.stack([(h["flags"] & 1).astype(bool) for h in held]) & (ids >= 0)
    bad = np.array([store.flags(k, 0)[1] for k in range(K)], bool)
    ordered = store.connections(cur)["ordered"]
    local = [cur] + [j for j in ordered if not bad[j]]
    cat = np.concatenate([ids[k][live[k]] for k in local])
    _, first = np.unique(cat, return_index=True)
    pids = cat[np.sort(first)]                                          # first occurrence order
    kk, ff = np.nonzero(live & np.isin(ids, pids))
    order = np.argsort(pids, kind="stable")
    pt = order[np.searchsorted(pids[order], ids[kk, ff])]
    key = np.lexsort((ff, kk, pt))
    pt, kk, ff = pt[key], kk[key], ff[key]
    keep = np.ones(len(pt), bool)
    keep[1:] = (pt[1:] != pt[:-1]) | (kk[1:] != kk[:-1])                # a key-frame's observation: its lowest feature
    pt, kk, ff = pt[keep], kk[keep], ff[keep]
    marked = np.zeros(K, bool)
    marked[[cur] + list(ordered)] = True
    cams = local + [int(k) for k in np.unique(kk) if not marked[k] and not bad[k]]
    index = np.full(K, -1)
    index[cams] = np.arange(len(cams))
    has = index[kk] >= 0
    return cams, pids, index[kk][has], pt[has], ff[has]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=500)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from vo_slam_test_amd import _lib as vo
    K, n = a.keyframes, a.features
    assert K >= SCENE
    kfs = scene_keyframes(np.random.default_rng(1), K, n)
    cur = K - 1
    stream = torch.cuda.Stream()
    s = vo.KeyFrameStore(K, n, stream=stream.cuda_stream)
    s.enable_connections()
    s.enable_culling()
    s.enable_mapping(CAM6, SF, FIRST_ID)
    s.enable_local_ba(*CAPS)
    arrays = lambda kf: {key: kf[key] for key in ("angle", "desc", "nodes", "flags", "points", "ids", "point_desc", "min_dist", "max_dist")}
    for k, kf in enumerate(kfs):
        s.insert(arrays(kf))
        s.set_keypoints(k, kf["octave"], kf["depth"], kf["u_right"])
        s.set_keypoint_xy(k, kf["xy"])
        if kf["pose"] is not None:
            s.set_pose(k, kf["pose"])
    scene = list(range(K - SCENE, K))
    s.update_connections(scene)

    def restore():
        for k in scene:
            kf = kfs[k]
            s.update_points(k, kf["flags"], kf["points"], kf["ids"], kf["point_desc"], kf["min_dist"], kf["max_dist"])
            s.set_pose(k, kf["pose"])

    def clock(fn):
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        out = fn()
        e1.record(stream)
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1), out

    cam5 = np.array([float(c) for c in CAM6[:5]])
    problem = lambda w: dict({k: w[k] for k in ("poses", "fixed", "points", "e_cam", "e_pt", "e_obs", "e_inv_sigma")}, cam=cam5)
    # ---- the host gather and the device window agree
    s.local_ba_window(cur)
    w = s.local_ba_window_result()
    cams, pids, e_cam, e_pt, e_feat = host_gather(s, kfs, cur, n)
    same = w["record"]["status"] == 0 and list(w["cam_keyframe"]) == cams and np.array_equal(w["point_id"], pids) and \
        np.array_equal(w["e_cam"], e_cam) and np.array_equal(w["e_pt"], e_pt) and np.array_equal(w["e_feature"], e_feat)
    if not same or s.connections_status() != 0:
        sys.exit("local_ba_store_bench: the device window and the host gather differ; nothing is reported")
    ba = vo.BundleAdjuster(problem(w))
    rows = {key: [] for key in ("window", "window_event", "window_index_fresh", "window_index_fresh_event", "solve", "apply", "apply_event", "composed", "host")}
    for rep in range(a.reps + 1):   # (the first repetition warms up)
        restore()
        t, ev, _ = clock(lambda: s.local_ba_window(cur))
        rows["window"].append(t), rows["window_event"].append(ev)
        t, ev, _ = clock(lambda: s.local_ba_window(cur))   # again: the observation index is not stale this time
        rows["window_index_fresh"].append(t), rows["window_index_fresh_event"].append(ev)

        def solve():
            ww = s.local_ba_window_result()
            ba.reset(problem(ww))
            erase, _, rc = ba.local_ba()
            return (erase,) + ba.state() + (rc,)
        t, _, (erase, poses, pts, rc) = clock(solve)
        rows["solve"].append(t)
        t, ev, _ = clock(lambda: s.local_ba_apply(poses, pts, erase))
        rows["apply"].append(t), rows["apply_event"].append(ev)
        rec = s.local_ba_window_result()["record"]
        restore()
        t, _, _ = clock(lambda: s.local_ba(ba, cur))
        rows["composed"].append(t)
        restore()
        t, _, _ = clock(lambda: host_gather(s, kfs, cur, n))
        rows["host"].append(t)
    med = {key: float(np.median(v[1:])) for key, v in rows.items()}
    spread = {key: float((max(v[1:]) - min(v[1:])) / np.median(v[1:])) for key, v in rows.items()}
    res = dict(tool="local_ba_store_bench", keyframes=K, features_per_keyframe=n, reps=a.reps, version=vo.lib().vo_version().decode(),
               capacities=list(CAPS), window={k: w["record"][k] for k in ("n_cams", "n_local", "n_fixed", "n_points", "n_edges", "n_dropped")},
               write_back={k: rec[k] for k in ("n_erased", "n_feature0", "n_dead")}, launches=dict(window=5, apply=2),
               median_ms=med, spread=spread, host_gather_over_device_window=med["host"] / med["window"])
    print(json.dumps(res))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    ba.close()


if __name__ == "__main__":
    main()
