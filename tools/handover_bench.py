#!/usr/bin/env python3
"""frame_last_ = frame_curr_ for a batch of tracked frames, both routes in one process on one tracker (DESIGN.md sections 4u, 7):
  device  vo_tracker_end_frame + vo_tracker_begin_frame: two launches, nothing else
  host    the hand-over the library offered before: six reads (vo_tracker_results and vo_tracker_get of ASSIGNED_LAST,
          ASSIGNED_LOCAL, FEATURE_HAS_POINT, FEATURE_OUTLIER, FEATURE_POINTS), the slot rule, the two cullings, Tcl_ and the
          start pose, the depth walk and the back-projection in numpy (vectorised over the batch), vo_tracker_set_last_frame.
          The frames' feature columns, the local map and the old list are host copies taken BEFORE the timed window (a caller of
          the host route keeps them), which favours this side.
Batch: --batch frames built from --unique synthetic frames with their synth.make_tracking_map maps, tracked once
(vo_tracker_track_dev); both routes hand that same tracked state over, alternating, after --warmup calls of each.  `ms` is
wall time around the calls until the tracker's stream has drained; medians of --reps, spread = (max - min) / median.
usage: tools/handover_bench.py [--batch 1024] [--unique 32] [--reps 15] [--warmup 3] [--out FILE]"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

f32 = np.float32
TH = 2.6


def exp_batch(xi):
    """[B, 6] -> Tcw [B, 3, 4] (Rodrigues and V, vectorised)"""
    u, w = xi[:, :3], xi[:, 3:]
    th = np.linalg.norm(w, axis=1)
    th = np.where(th < 1e-12, 1e-12, th)
    K = np.zeros((len(xi), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    K2 = K @ K
    a, b, c = (np.sin(th) / th)[:, None, None], ((1 - np.cos(th)) / th ** 2)[:, None, None], ((th - np.sin(th)) / th ** 3)[:, None, None]
    R, V = np.eye(3) + a * K + b * K2, np.eye(3) + b * K + c * K2
    return np.concatenate([R, (V @ u[:, :, None])], axis=2)


def host_route(trk, keep, last_T, cam):
    """-> the arrays handed to vo_tracker_set_last_frame"""
    res = trk.results()
    a0, a1 = trk.get(trk.ASSIGNED_LAST), trk.get(trk.ASSIGNED_LOCAL)
    has, outl, pts = trk.get(trk.FEATURE_HAS_POINT), trk.get(trk.FEATURE_OUTLIER), trk.get(trk.FEATURE_POINTS)
    B, cap = a0.shape
    rows = np.arange(B)[:, None]
    in_n = np.arange(cap)[None, :] < keep["n"][:, None]
    from_local = (a1 >= 0) & in_n
    from_last = ~from_local & (a0 >= 0) & (has != 0) & in_n
    i1, i0 = np.clip(a1, 0, None), np.clip(a0, 0, None)
    obs = np.where(from_local, keep["local_flags"][rows, i1] >> 1, np.where(from_last, keep["last_flags"][rows, i0] >> 1, 0)) & 1
    held = (from_local | from_last) & (obs != 0)                      # cullingTempMapPoints
    flags = np.where(held, np.where(outl != 0, 2, 3), 0).astype(np.uint8)  # cullingOutliersOfFrame: bit 0 off
    desc = np.where(from_local[:, :, None], keep["local_desc"][rows, i1], keep["last_desc"][rows, i0]) * held[:, :, None].astype(np.uint8)
    points = np.where(held[:, :, None], pts, 0.0)
    # Tcl_ = Tcw * Tlw^-1 and the start pose Tcl_ * Tcw
    T = exp_batch(res["pose"])
    ok = (res["status"] == 0) & (res["n_tracked"] >= 30)
    Rl, tl = last_T[:, :, :3], last_T[:, :, 3]
    Vr = T[:, :, :3] @ Rl.transpose(0, 2, 1)
    Vt = T[:, :, 3] - (Vr @ tl[:, :, None])[:, :, 0]
    Vr, Vt = np.where(ok[:, None, None], Vr, np.eye(3)), np.where(ok[:, None], Vt, 0.0)
    Pr, Pt = Vr @ T[:, :, :3], (Vr @ T[:, :, 3:])[:, :, 0] + Vt
    # updateLastFrame's temporary points: pairs (d, i) ascending, the walk as a scan
    d = np.where(in_n & (keep["depth"] > 0), keep["depth"], np.inf).astype(f32)
    order = np.argsort(d, axis=1, kind="stable")
    ds, null = d[rows, order], (flags[rows, order] & 3) != 3
    valid = np.isfinite(ds)
    C = np.cumsum(null & valid, axis=1)
    stop = valid & (ds > f32(TH)) & (C > 100)
    J = np.where(stop.any(axis=1), stop.argmax(axis=1), cap)
    made_sorted = null & valid & (np.arange(cap)[None, :] <= J[:, None])
    made = np.zeros_like(made_sorted)
    made[rows, order] = made_sorted
    z = keep["depth"].astype(np.float64)
    pc = np.stack([(keep["x"] - cam[2]) * z / cam[0], (keep["y"] - cam[3]) * z / cam[1], z], axis=2)
    pw = np.einsum("bji,bnj->bni", T[:, :, :3], pc - T[:, None, :, 3])
    points = np.where(made[:, :, None], pw, points)
    flags = np.where(made, 1, flags).astype(np.uint8)
    desc = np.where(made[:, :, None], keep["desc"], desc)
    Tpred = np.concatenate([Pr.reshape(B, 9), Pt], axis=1)
    trk.set_last_frame(Tpred, points, flags, keep["octave"], keep["angle"], desc)
    return T, int(made.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--unique", type=int, default=32)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "handover_bench.json"))
    args = ap.parse_args()
    import torch
    from vo_slam_test_amd import _lib as vo
    from vo_slam_test_amd import synth
    from vo_slam_test_amd.tracking import load_maps, stack_maps
    if not torch.cuda.is_available():
        raise SystemExit("handover_bench: no GPU (a measurement path does not fall back)")
    B, W, H, U = args.batch, 640, 480, max(1, min(args.batch, args.unique))
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
    n_local = max(len(m[3]["flags"]) for m in maps)
    trk = vo.Tracker(B, cam5, None, W, H, max_last=cap, max_local=n_local, inv_depth_scale=inv, single_stream=True)
    all_maps = [maps[f % U] for f in range(B)]
    last, local = load_maps(trk, all_maps, cap, n_local)
    T0 = np.stack([m[0] for m in all_maps])
    trk.set_last_pose(T0, np.ones(B, np.uint8))
    frames = torch.from_numpy(np.stack([uniq[f % U] for f in range(B)])).cuda()
    depth = torch.from_numpy(np.stack([udep[f % U] for f in range(B)]).view(np.int16)).cuda()
    trk.track_dev(frames, depth)
    res = trk.results()
    pad = lambda key, dt: np.stack([np.concatenate([fr[f % U][key], np.zeros((cap - fr[f % U]["n"],) + fr[f % U][key].shape[1:], dt)]) for f in range(B)])
    keep = dict(n=np.array([fr[f % U]["n"] for f in range(B)]), x=pad("x", f32), y=pad("y", f32), depth=pad("depth", f32), desc=pad("desc", np.uint8),
                octave=pad("octave", np.int32), angle=pad("angle", f32), local_flags=local["valid"], local_desc=local["desc"],
                last_flags=last["flags"], last_desc=last["desc"])
    last_T = T0.reshape(B, 12)
    last_T = np.concatenate([last_T[:, :9].reshape(B, 3, 3), last_T[:, 9:, None]], axis=2)

    def device():
        t0 = time.perf_counter()
        trk.end_frame(TH), trk.begin_frame(TH)
        trk.sync()
        return (time.perf_counter() - t0) * 1e3

    def host():
        t0 = time.perf_counter()
        host_route(trk, keep, last_T, cam5)
        trk.sync()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(args.warmup):
        device(), host()
    dev_ms, host_ms = [], []
    for _ in range(args.reps):            # interleaved: both see the same machine
        dev_ms.append(device()), host_ms.append(host())
    trk.end_frame(TH), trk.begin_frame(TH)
    temp = trk.get(trk.TEMP_COUNT)
    summary = lambda v: dict(ms=float(np.median(v)), spread=float((max(v) - min(v)) / np.median(v)), runs_ms=[float(x) for x in v])
    out = dict(tool="handover_bench", batch=B, unique_frames=U, max_features=cap, max_local=n_local, reps=args.reps, th_depth=TH,
               version=vo.lib().vo_version().decode(), tracked=int((res["status"] == 0).sum()), temp_points_per_frame=float(temp.mean()),
               launches=dict(device=2, source="read off the code, not traced"), device=summary(dev_ms), host=summary(host_ms))
    out["host_over_device"] = out["host"]["ms"] / out["device"]["ms"]
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("device", "host")} | dict(device_ms=out["device"]["ms"], host_ms=out["host"]["ms"],
                                                                                         device_spread=out["device"]["spread"],
                                                                                         host_spread=out["host"]["spread"])))
    trk.close()


if __name__ == "__main__":
    main()
