#!/usr/bin/env python3
"""Relocalisation from the key-frame database, both routes in one process run:
  parent  vo_kfdb_query_reloc_dev + copy-out + the candidates' features gathered on the host +
          vo_tracker_set_reloc_candidates + vo_tracker_relocalize_dev (the route as it was before the device store)
  device  vo_tracker_relocalize_db_dev (vo_kfstore + k_featvec + k_bow_walk: no host step)
Batch of lost frames (the six synthetic frames tiled), a store of key-frames made from those frames' own features
(shuffled, 1 % descriptor noise, map points = the features back-projected with their depth).  The parent route is handed
the frames' BoW vectors ready-made (it has no call that produces them on the device); the device route computes them.
Medians after warm-up; the per-stage event times of the new kernels come from vo_tracker_get_reloc_timing.
usage: tools/reloc_db_bench.py [--batch 1024] [--keyframes 500] [--cand 4] [--reps 5] [--parent-reps 3] [--out FILE]"""
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
    ap.add_argument("--keyframes", type=int, default=500)
    ap.add_argument("--cand", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-reps", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "reloc_db_bench.json"))
    a = ap.parse_args()
    import torch
    from vo_slam_test_amd import _lib as vo
    from vo_slam_test_amd import synth
    B, MC, NKF, W, H, NB = a.batch, a.cand, a.keyframes, 640, 480, 6
    cam5 = synth.CAM.astype(np.float32)
    inv = float(np.float32(1.0) / np.float32(synth.DEPTH_SCALE))
    imgs6 = synth.make_frames(NB, start=80)
    raw6 = np.stack([synth.make_depth(80 + i) for i in range(NB)]).view(np.uint16)
    vd = synth.make_vocabulary(3, k=8, L=4)
    voc = vo.Vocabulary(vd["L"], vd["child_start"], vd["children"], vd["node_desc"], vd["node_weight"], vd["word_id"])
    n_words = int((np.asarray(vd["word_id"]) >= 0).sum())
    # the base frames' features, as the tracker builds them
    t6 = vo.Tracker(NB, cam5, None, W, H, max_last=8, max_local=8, inv_depth_scale=inv)
    t6.track_first(imgs6, raw6)
    t6.sync()
    base = [t6.download_frame(f) for f in range(NB)]
    cap = t6.cap
    t6.close()
    rng = np.random.default_rng(1)
    kfs, vecs = [], []
    for j in range(NKF):
        f = j % NB
        fr = base[f]
        idx = rng.permutation(len(fr["x"]))
        z = np.where(fr["depth"][idx] > 0, fr["depth"][idx], 2.5).astype(np.float64)
        P = np.stack([(fr["x"][idx].astype(np.float64) - cam5[2]) * z / cam5[0], (fr["y"][idx].astype(np.float64) - cam5[3]) * z / cam5[1], z], 1)
        desc = fr["desc"][idx].copy()
        flip = rng.random(desc.shape) < 0.01
        desc[flip] ^= rng.integers(1, 256, int(flip.sum()), dtype=np.uint8)
        word, weight, node = voc.transform(desc)
        maxd = (np.linalg.norm(P, axis=1) * 1.2 ** fr["octave"][idx].astype(np.float64)).astype(np.float32)
        kfs.append(dict(angle=fr["angle"][idx].astype(np.float32), desc=desc, nodes=node, flags=np.ones(len(idx), np.uint8), points=P,
                        ids=(f * 100000 + idx).astype(np.int32), point_desc=desc, min_dist=(maxd / np.float32(1.2 ** 7)).astype(np.float32),
                        max_dist=maxd))
        vecs.append(vo.bow_vector([word], [weight])[0])
    nfeat = int(np.mean([len(k["flags"]) for k in kfs]))
    imgs = torch.from_numpy(np.ascontiguousarray(imgs6[np.arange(B) % NB])).cuda()
    raw = torch.from_numpy(np.ascontiguousarray(raw6[np.arange(B) % NB]).view(np.int16)).cuda()
    trk = vo.Tracker(B, cam5, None, W, H, max_last=8, max_local=8, inv_depth_scale=inv, max_reloc_candidates=MC, max_reloc_features=cap)
    stream = trk.st
    db = vo.KeyFrameDatabase(n_words, NKF, cap, B, stream=stream)
    store = vo.KeyFrameStore(NKF, cap, stream=stream)
    for k, (w, v) in zip(kfs, vecs):
        db.insert(w, v)
        store.insert(k)
    # the frames' BoW vectors for the parent route (ready-made, device memory)
    qv = []
    for f in range(NB):
        word, weight, _ = voc.transform(base[f]["desc"])
        qv.append(vo.bow_vector([word], [weight])[0])
    qs = np.zeros(B + 1, np.int32)
    for i in range(B):
        qs[i + 1] = qs[i] + len(qv[i % NB][0])
    q_start = torch.from_numpy(qs).cuda()
    q_words = torch.from_numpy(np.concatenate([qv[i % NB][0] for i in range(B)]).astype(np.int32)).cuda()
    q_vals = torch.from_numpy(np.concatenate([qv[i % NB][1] for i in range(B)]).astype(np.float64)).cuda()
    n_cand, cand = torch.zeros(B, dtype=torch.int32).cuda(), torch.zeros((B, MC), dtype=torch.int32).cuda()

    def parent():
        db.query_reloc_dev(B, q_start, q_words, q_vals, None, MC, n_cand, cand)
        trk.sync()
        nc, cd = n_cand.cpu().numpy(), cand.cpu().numpy()
        lists = []
        for f in range(B):  # the host gather, with the ids made dense per frame (what vo_tracker_set_reloc_candidates accepts)
            cl = [kfs[g] for g in cd[f, :min(nc[f], MC)]]
            if cl:
                _, inv_ = np.unique(np.concatenate([k["ids"] for k in cl]), return_inverse=True)
                o, out = 0, []
                for k in cl:
                    out.append(dict(k, ids=inv_[o:o + len(k["ids"])].astype(np.int32)))
                    o += len(k["ids"])
                cl = out
            lists.append(cl)
        trk.set_reloc_candidates(voc, lists)
        trk.relocalize_dev(imgs, raw)
        trk.sync()

    def device():
        trk.relocalize_db(db, store, voc, imgs, raw)
        trk.sync()

    def timed(fn, reps):
        fn()  # warm-up (first-use allocations)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), ts

    p_ms, p_all = timed(parent, a.parent_reps)
    w_parent = trk.get(trk.RELOC_WINNER)
    d_ms, d_all = timed(device, a.reps)
    w_device = trk.get(trk.RELOC_WINNER)
    trk.set_timing(True)
    stages = []
    for _ in range(a.reps):
        device()
        stages.append(trk.get_reloc_timing())
    trk.set_timing(False)
    st_ms = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
    res = dict(tool="reloc_db_bench", batch=B, keyframes=NKF, max_candidates=MC, features_per_keyframe=nfeat, frame_capacity=cap,
               parent_ms=p_ms, parent_runs_ms=p_all, device_ms=d_ms, device_runs_ms=d_all, speedup=p_ms / d_ms,
               frames_per_s_parent=B / p_ms * 1e3, frames_per_s_device=B / d_ms * 1e3, new_stage_ms=st_ms,
               mean_true_candidates=float(trk.get(trk.RELOC_N_CANDIDATES).mean()), relocalised_parent=int((w_parent >= 0).sum()),
               relocalised_device=int((w_device >= 0).sum()), winners_equal=bool(np.array_equal(w_parent, w_device)))
    print(json.dumps(res))
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
