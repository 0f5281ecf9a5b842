#!/usr/bin/env python3
"""trackRefKeyFrame for a batch, both forms in one process run (DESIGN.md sections 4b, 4f, 7):
  host   vo_tracker_set_ref_keyframe (the key-frames' features uploaded from host arrays) + vo_tracker_track_ref_keyframe_dev
         (the common-node walk on the host: one synchronisation inside the call)
  store  vo_tracker_track_ref_keyframe_store_dev (key-frames read from a vo_kfstore by number: launches only)
Batch = the six synthetic frames tiled; frame f's reference key-frame = its own features shuffled with 1 % descriptor
noise, map points = the features back-projected with their depth, pose = identity.  Per form and repetition: the host-side
time until the call returns (`host_ms`), the time between two events recorded on the tracker's stream around the call
(`event_ms`) and the time until the stream has drained (`total_ms`).  Medians after a warm-up call, and the spread as
(max - min) / median.  A library without the store form (an older build, VO_HIP_LIB) reports the host form alone.
usage: tools/ref_keyframe_bench.py [--batch 1024] [--reps 7] [--first-stage-only] [--out FILE]"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--first-stage-only", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ref_keyframe_bench.json"))
    a = ap.parse_args()
    import torch
    from vo_slam_test_amd import _lib as vo
    from vo_slam_test_amd import synth
    B, W, H, NB = a.batch, 640, 480, 6
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
    pad = lambda x: np.concatenate([x, np.zeros((nk - len(x),) + x.shape[1:], x.dtype)])
    kfs = []
    for f in range(NB):
        fr = base[f]
        idx = rng.permutation(len(fr["x"]))
        z = np.where(fr["depth"][idx] > 0, fr["depth"][idx], 2.5).astype(np.float64)
        P = np.stack([(fr["x"][idx].astype(np.float64) - cam5[2]) * z / cam5[0], (fr["y"][idx].astype(np.float64) - cam5[3]) * z / cam5[1], z], 1)
        desc = fr["desc"][idx].copy()
        flip = rng.random(desc.shape) < 0.01
        desc[flip] ^= rng.integers(1, 256, int(flip.sum()), dtype=np.uint8)
        node = voc.transform(desc)[2]
        n = len(idx)
        kfs.append(dict(angle=fr["angle"][idx].astype(np.float32), desc=desc, nodes=node, flags=np.full(n, 3, np.uint8), points=P,
                        ids=np.arange(n, dtype=np.int32), point_desc=desc, min_dist=np.full(n, 0.1, np.float32),
                        max_dist=np.full(n, 50.0, np.float32)))
    which = np.arange(B) % NB
    imgs = torch.from_numpy(np.ascontiguousarray(imgs6[which])).cuda()
    raw = torch.from_numpy(np.ascontiguousarray(raw6[which]).view(np.int16)).cuda()
    Tcw = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64), (B, 1))
    # the host form's arrays [B][nk]: what a caller without a store hands over per batch
    h = {k: np.ascontiguousarray(np.stack([pad(kfs[f][k]) for f in range(NB)])[which]) for k in ("points", "flags", "angle", "desc")}
    h_nodes = np.ascontiguousarray(np.stack([np.concatenate([kfs[f]["nodes"], np.full(nk - len(kfs[f]["nodes"]), 2 ** 30, np.int32)])
                                              for f in range(NB)])[which])
    trk = vo.Tracker(B, cam5, None, W, H, max_last=nk, max_local=8, inv_depth_scale=inv)
    stream = torch.cuda.ExternalStream(trk.st)
    fso = bool(a.first_stage_only)
    have_store = hasattr(vo.lib(), "vo_tracker_track_ref_keyframe_store_dev")

    def host():
        trk.set_ref_keyframe(voc, Tcw, h["points"], h["flags"], h["angle"], h["desc"], h_nodes)
        trk.track_ref_keyframe_dev(imgs, raw, first_stage_only=fso)

    if have_store:
        store = vo.KeyFrameStore(NB, nk, stream=trk.st)
        for k in kfs:
            store.insert(k)
        d_ref = torch.from_numpy(which.astype(np.int32)).cuda()
        d_Tcw = torch.from_numpy(Tcw).cuda()

        def dev():
            trk.track_ref_keyframe_store(store, voc, d_ref, d_Tcw, imgs, raw, first_stage_only=fso)

    def timed(fn):
        fn()  # warm-up (first-use allocations)
        trk.sync()
        rows = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            e1.record(stream)
            trk.sync()
            t2 = time.perf_counter()
            rows.append(((t1 - t0) * 1e3, e0.elapsed_time(e1), (t2 - t0) * 1e3))
        r = np.array(rows)
        med = np.median(r, 0)
        out = {k: float(med[i]) for i, k in enumerate(("host_ms", "event_ms", "total_ms"))}
        out["spread"] = {k: float((r[:, i].max() - r[:, i].min()) / med[i]) for i, k in enumerate(("host_ms", "event_ms", "total_ms"))}
        out["runs_total_ms"] = [float(v) for v in r[:, 2]]
        return out

    res = dict(tool="ref_keyframe_bench", batch=B, features_per_keyframe=int(np.mean([len(k["flags"]) for k in kfs])), max_last=nk,
               frame_capacity=trk.cap, first_stage_only=fso, reps=a.reps, version=vo.lib().vo_version().decode())
    res["host_form"] = timed(host)
    r_host = trk.results()
    res["host_form"]["matches_median"] = int(np.median(r_host["n_matches_last"]))
    if have_store:
        res["store_form"] = timed(dev)
        r_dev = trk.results()
        res["store_form"]["matches_median"] = int(np.median(r_dev["n_matches_last"]))
        res["results_equal"] = bool(all(np.array_equal(r_host[k], r_dev[k]) for k in r_host))
        res["speedup_total"] = res["host_form"]["total_ms"] / res["store_form"]["total_ms"]
    print(json.dumps(res))
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
