#!/usr/bin/env python3
"""LocalMapping::createNewMapPoints for a key-frame store, both forms in one process run on stores with the same key-frames
(DESIGN.md sections 4j, 7):
  device  vo_kfstore_create_map_points on a store with connections, culling and mapping enabled: three launches per
          neighbour (walk, replay, create), ten neighbours, nothing but launches
  host    the interface before the device form existed: a host copy of ids, flags, poses and key-point columns; per
          neighbour the geometry on the host, one vo_match_triangulation with the flags as the neighbours before left them,
          vo_triangulate for the matches the parallax test sends there, the gates in numpy, the flags and points updated on
          the host (the geometry is tests/new_points_ref.py's interpreted Python, about 150 scalar operations a neighbour); at the end vo_kfstore_update_points for every key-frame that received a point (a store without mapping)
Store: --keyframes key-frames of --features features.  The last 12 are views of one scene (1600 points 4 .. 9 m in front of
cameras 0.3 m apart, 40 % of them mapped already, a third of the features stereo); the others are filler with ids of their
own.  Connections are built by one update call over the last 12.  The current key-frame is the last one.
A create call cannot be undone, so before every repetition the map side of the current key-frame and its neighbours is put
back with vo_kfstore_update_points (not timed).  Measured as the median of --reps after a warm-up: `total_ms` until the
stream has drained and (device) `event_ms` between two events on the store's stream.
The two forms' created (neighbour, idx1, idx2) lists are compared first and the tool stops if they differ.
Per-kernel times come from a profiler run of this tool (rocprofv3 --kernel-trace --stats), not from the tool.
usage: tools/new_points_bench.py [--keyframes 500] [--features 1000] [--reps 5] [--out FILE]"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))   # the geometry in the documented operation order (tests/new_points_ref.py)

import numpy as np  # noqa: E402

f32 = np.float32
CAM6 = np.array([500.0, 500.0, 320.0, 240.0, 40.0, 0.08], f32)
SF = np.cumprod(np.array([1.0] + [1.2] * 7, f32), dtype=f32)
SCENE, FIRST_ID = 12, 1 << 20


def scene_keyframes(rng, K, n):
    """-> list of dicts: the arrays KeyFrameStore.insert takes plus octave, depth, u_right, xy, pose"""
    n_world = int(1.6 * n)
    Wp = np.stack([rng.uniform(-3, 6, n_world), rng.uniform(-2, 2, n_world), rng.uniform(4, 9, n_world)], 1)
    mapped = rng.random(n_world) < 0.4
    base = rng.integers(0, 256, (n_world, 32), dtype=np.uint8)
    node, level = rng.integers(0, max(n // 6, 1), n_world), rng.integers(0, 4, n_world)
    kfs = []
    for k in range(K):
        s = k - (K - SCENE)
        if s < 0:   # filler: ids nobody else holds, no pose needed
            ids = (FIRST_ID // 2 + k * n + np.arange(n)).astype(np.int32)
            kfs.append(dict(angle=np.zeros(n, f32), desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), nodes=rng.integers(0, 50, n).astype(np.int32),
                            flags=np.full(n, 3, np.uint8), points=np.zeros((n, 3)), ids=ids, point_desc=np.zeros((n, 32), np.uint8),
                            min_dist=np.full(n, 0.1, f32), max_dist=np.full(n, 50.0, f32), octave=np.zeros(n, np.int32),
                            depth=np.full(n, -1.0, f32), u_right=np.full(n, -1.0, f32), xy=np.zeros((n, 2), f32), pose=None))
            continue
        c = np.array([0.3 * s, 0.02 * (s % 3), 0.0])
        th = 0.01 * (s - 6)
        R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
        seen = rng.permutation(n_world)[:n]
        pc = (R @ (Wp[seen] - c).T).T
        u, v, z = (500.0 * pc[:, 0] / pc[:, 2] + 320.0).astype(f32), (500.0 * pc[:, 1] / pc[:, 2] + 240.0).astype(f32), pc[:, 2].astype(f32)
        stereo = rng.random(n) < 0.33
        desc = base[seen].copy()
        flip = rng.integers(0, 256, (n, 3))
        for j in range(3):
            desc[np.arange(n), flip[:, j] // 8] ^= (1 << (flip[:, j] % 8)).astype(np.uint8)
        kfs.append(dict(angle=np.zeros(n, f32), desc=desc, nodes=node[seen].astype(np.int32), flags=np.where(mapped[seen], 3, 0).astype(np.uint8),
                        points=np.zeros((n, 3)), ids=np.where(mapped[seen], seen, -1).astype(np.int32), point_desc=np.zeros((n, 32), np.uint8),
                        min_dist=np.full(n, 0.1, f32), max_dist=np.full(n, 50.0, f32), octave=level[seen].astype(np.int32),
                        depth=np.where(stereo, z, f32(-1)).astype(f32), u_right=np.where(stereo, u - f32(40.0) / z, f32(-1)).astype(f32),
                        xy=np.stack([u, v], 1).astype(f32), pose=[float(x) for x in R.reshape(-1)] + [float(x) for x in -(R @ c)]))
    return kfs


def host_gates(T1, T2, Ow1, Ow2, f1, f2, p):
    """the gates of localMapping.cpp:262-341 for arrays of matches -> (accepted, dist1)"""
    fx, fy, cx, cy, bf = (f32(c) for c in CAM6[:5])
    ok = np.ones(len(p), bool)
    zs = []
    for T in (T1, T2):
        zs.append((p @ np.array(T[6:9]) + T[11]).astype(f32))
        ok &= zs[-1] > 0
    for T, z, f in ((T1, zs[0], f1), (T2, zs[1], f2)):
        with np.errstate(all="ignore"):
            x, y = (p @ np.array(T[0:3]) + T[9]).astype(f32), (p @ np.array(T[3:6]) + T[10]).astype(f32)
            invz, inv_sigma = f32(1.0) / z, f32(1.0) / SF[f["octave"]]
            u, v = fx * x * invz + cx, fy * y * invz + cy
            e = (u - f["u"]) ** 2 + (v - f["v"]) ** 2
            er = (u - bf * invz) - f["ur"]
            stereo = f["ur"] >= 0
            ok &= np.where(stereo, ~((e + er * er) * inv_sigma * inv_sigma > f32(7.815)), ~(e * inv_sigma * inv_sigma > f32(5.991)))
    d1, d2 = np.linalg.norm(p - np.array(Ow1), axis=1).astype(f32), np.linalg.norm(p - np.array(Ow2), axis=1).astype(f32)
    ok &= ~((d1 < 1e-6) | (d2 < 1e-6))
    with np.errstate(all="ignore"):
        ratio, scale_ratio, factor = d2 / d1, SF[f1["octave"]] / SF[f2["octave"]], f32(1.5) * SF[1]
        ok &= ~((ratio * factor < scale_ratio) | (ratio > scale_ratio * factor))
    return ok, d1


def host_create(vo, kfs, cur, order, state, plain, geometry):
    """the host form -> created [(neighbour, idx1, idx2)]; state: {key-frame: dict(flags, ids, points, min_dist, max_dist,
    point_desc)} of the host's copy, edited in place"""
    A = kfs[cur]
    fa = vo.FrameArrays(A["xy"][:, 0], A["xy"][:, 1], A["octave"], A["angle"], A["u_right"], A["desc"])
    na = vo.BowNodes(A["nodes"])
    created, touched, next_id = [], set(), FIRST_ID
    m = vo.Matcher(0.6)
    b = float(CAM6[5])
    for k in order[:10]:
        B = kfs[k]
        G = geometry(A["pose"], B["pose"], CAM6)
        if G["bl"] < CAM6[5]:
            continue
        fb = vo.FrameArrays(B["xy"][:, 0], B["xy"][:, 1], B["octave"], B["angle"], B["u_right"], B["desc"])
        n_m, match = m.searchForTriangulation(fa, state[cur]["flags"] & 1, na, fb, state[k]["flags"] & 1, vo.BowNodes(B["nodes"]),
                                              np.array(G["F"]).reshape(3, 3), float(G["ex"]), float(G["ey"]), SF, True)
        i1 = np.nonzero(match >= 0)[0]
        if len(i1) == 0:
            continue
        i2 = match[i1]
        f1 = dict(u=A["xy"][i1, 0], v=A["xy"][i1, 1], ur=A["u_right"][i1], depth=A["depth"][i1], octave=A["octave"][i1])
        f2 = dict(u=B["xy"][i2, 0], v=B["xy"][i2, 1], ur=B["u_right"][i2], depth=B["depth"][i2], octave=B["octave"][i2])
        T1, T2 = np.array(G["T1"]), np.array(G["T2"])
        R1, R2 = T1[:9].reshape(3, 3), T2[:9].reshape(3, 3)
        xn = [np.stack([(f["u"] - CAM6[2]) * f32(1.0) / CAM6[0], (f["v"] - CAM6[3]) * f32(1.0) / CAM6[1]], 1).astype(f32) for f in (f1, f2)]
        rays = [np.concatenate([x.astype(np.float64), np.ones((len(x), 1))], 1) @ R for x, R in zip(xn, (R1, R2))]
        cos_ray = ((rays[0] * rays[1]).sum(1) / (np.linalg.norm(rays[0], axis=1) * np.linalg.norm(rays[1], axis=1))).astype(f32)
        s1, s2 = f1["ur"] >= 0, f2["ur"] >= 0
        with np.errstate(all="ignore"):
            cd1 = np.where(s1, np.cos((2 * np.arctan2(0.5 * b, f1["depth"].astype(np.float64))).astype(f32)), f32(2.0)).astype(f32)
            cd2 = np.where(~s1 & s2, np.cos((2 * np.arctan2(0.5 * b, f2["depth"].astype(np.float64))).astype(f32)), f32(2.0)).astype(f32)
        svd = (cos_ray > 0) & (cos_ray < np.minimum(cd1, cd2)) & (s1 | s2 | (cos_ray.astype(np.float64) < 0.9998))
        d1p, d2p = ~svd & s1 & (cd1 < cd2), ~svd & ~(s1 & (cd1 < cd2)) & s2 & (cd2 < cd1)
        p, have = np.zeros((len(i1), 3)), np.zeros(len(i1), bool)
        if svd.any():
            T1f = np.concatenate([R1, T1[9:, None]], 1).astype(f32)
            T2f = np.concatenate([R2, T2[9:, None]], 1).astype(f32)
            pts, good = vo.triangulate(xn[0][svd], xn[1][svd], T1f, T2f)
            p[svd], have[svd] = pts.astype(np.float64), good != 0
        for sel, f, R, Ow in ((d1p, f1, R1, G["Ow1"]), (d2p, f2, R2, G["Ow2"])):
            if sel.any():
                z = f["depth"][sel]
                pc = np.stack([(f["u"][sel] - CAM6[2]) * z / CAM6[0], (f["v"][sel] - CAM6[3]) * z / CAM6[1], z], 1).astype(np.float64)
                p[sel], have[sel] = pc @ R + np.array(Ow), True
        ok, dist1 = host_gates(T1, T2, G["Ow1"], G["Ow2"], f1, f2, p)
        ok &= have
        for j in np.nonzero(ok)[0]:
            a, c = int(i1[j]), int(i2[j])
            maxd = dist1[j] * SF[A["octave"][a]]
            for key, i in ((cur, a), (k, c)):
                s = state[key]
                s["flags"][i], s["ids"][i], s["points"][i] = 3, next_id, p[j]
                s["max_dist"][i], s["min_dist"][i] = maxd, maxd / SF[-1]
                s["point_desc"][i] = (A["desc"][a] if cur < k else B["desc"][c])
            created.append((int(k), a, c))
            next_id += 1
            touched |= {cur, int(k)}
    for k in sorted(touched):
        s = state[k]
        plain.update_points(k, s["flags"], s["points"], s["ids"], s["point_desc"], s["min_dist"], s["max_dist"])
    return created


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=500)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from new_points_ref import geometry
    from vo_slam_test_amd import _lib as vo
    K, n = a.keyframes, a.features
    assert K >= SCENE
    kfs = scene_keyframes(np.random.default_rng(1), K, n)
    cur = K - 1
    stream = torch.cuda.Stream()
    dev = vo.KeyFrameStore(K, n, stream=stream.cuda_stream)
    dev.enable_connections()
    dev.enable_culling()
    dev.enable_mapping(CAM6, SF, FIRST_ID)
    plain = vo.KeyFrameStore(K, n, stream=stream.cuda_stream)
    arrays = lambda kf: {key: kf[key] for key in ("angle", "desc", "nodes", "flags", "points", "ids", "point_desc", "min_dist", "max_dist")}
    for k, kf in enumerate(kfs):
        dev.insert(arrays(kf))
        plain.insert(arrays(kf))
        dev.set_keypoints(k, kf["octave"], kf["depth"], kf["u_right"])
        dev.set_keypoint_xy(k, kf["xy"])
        if kf["pose"] is not None:
            dev.set_pose(k, kf["pose"])
    dev.update_connections(list(range(K - SCENE, K)))
    order = dev.connections(cur)["ordered"][:10]
    touched = [cur] + order
    fresh = lambda: {k: {key: kfs[k][key].copy() for key in ("flags", "ids", "points", "point_desc", "min_dist", "max_dist")} for k in touched}

    def restore():
        for store in (dev, plain):
            for k in touched:
                kf = kfs[k]
                store.update_points(k, kf["flags"], kf["points"], kf["ids"], kf["point_desc"], kf["min_dist"], kf["max_dist"])

    def timed(fn, reps):
        """fn(state): state is a fresh host copy of the touched key-frames, made outside the timing"""
        restore()
        fn(fresh())
        stream.synchronize()
        rows = []
        for _ in range(reps):
            restore()
            state = fresh()
            stream.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            fn(state)
            e1.record(stream)
            stream.synchronize()
            rows.append(((time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)))
        r = np.array(rows)
        med = np.median(r, 0)
        return dict(total_ms=float(med[0]), event_ms=float(med[1]), spread=float((r[:, 0].max() - r[:, 0].min()) / med[0]),
                    runs_total_ms=[float(v) for v in r[:, 0]])

    # ---- the two forms create the same points
    restore()
    dev.create_map_points(cur, 10)
    got = dev.new_points_result()
    want = host_create(vo, kfs, cur, order, fresh(), plain, geometry)
    same = [(k, i1, i2) for k, i1, i2, _ in got["created"]] == want and all(dev.flags(k) == plain.flags(k) for k in touched)
    if not same or dev.connections_status() != 0 or not want:
        sys.exit("new_points_bench: the device form and the host form created different points; nothing is reported")
    res = dict(tool="new_points_bench", keyframes=K, features_per_keyframe=n, reps=a.reps, version=vo.lib().vo_version().decode(),
               neighbors=[list(x) for x in got["neighbors"]], created=len(want), launches_per_call=30,
               mapping_bytes_before_rounding=8 * K * n + 104 * K + 197 * n + 848)
    res["device"] = timed(lambda state: dev.create_map_points(cur, 10), a.reps)
    res["host"] = timed(lambda state: host_create(vo, kfs, cur, order, state, plain, geometry), a.reps)
    del res["host"]["event_ms"]   # (the host form's work is not on one stream)
    res["speedup"] = res["host"]["total_ms"] / res["device"]["total_ms"]
    res["alternative_layout"] = None   # the speculative step layout is not built: there is no figure for it
    print(json.dumps(res))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
