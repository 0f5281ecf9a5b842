#!/usr/bin/env python3
"""LoopClosing::detectLoop for the newest key-frame of a key-frame store, both routes in one process run on the same store and
database (DESIGN.md sections 4t, 7):
  device  vo_kfstore_detect_loop: six launches on the store's stream, nothing read back; and vo_kfstore_loop_closing_step for the
          same key-frame, which adds compute_sim3_detected's launches and the ONE synchronising read
  host    the route before the layer existed: vo_kfstore_get_connections of the current key-frame (synchronises), excl and conn
          assembled on the host, vo_kfdb_query_loop in its host form (uploads, synchronises, reads the candidates back),
          vo_kfstore_get_connections of every candidate and the consistency groups of loopClosing.cpp:95-165 as Python sets; the
          database's neighbour rows of the current key-frame and of its connected key-frames refreshed with vo_kfdb_set_neighbors
          is timed on its own (`host_set_neighbors`)
Store: --keyframes key-frames of --features features, ids as tools/connections_bench.py draws them (six groups, a key-frame is
connected to every key-frame of its group).  BoW vectors: --words words per key-frame drawn from a pool of 600 that starts at
300 x group, so that a key-frame shares words with its own group (excluded: connected) and with the two neighbouring ones; the
five key-frames from K / 5 on revisit the current key-frame's place: its words, the weights redrawn within 10 %.
The two routes' candidates and groups are compared first and the tool stops if they differ.  Each figure is the median of --reps
after a warm-up: `enqueue_ms` the host time of the call alone, `event_ms` between two events on the store's stream, `total_ms`
until the stream has drained.
usage: tools/detect_loop_bench.py [--keyframes 500] [--features 1000] [--words 150] [--reps 7] [--out FILE]"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

IDS_PER_GROUP, NB, N_WORDS, D, G = 4096, 6, 2400, 64, 256
LAUNCHES = dict(detect_loop=6, detect_loop_after_insert=10, k_dl_begin=1, k_dl_neighbors=1, k_kfdb_min_score=1, k_kfdb_query=1, k_dl_groups=1,
                k_dl_resolve=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=500)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--words", type=int, default=150)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from vo_slam_test_amd import _lib as vo
    K, n = a.keyframes, a.features
    rng = np.random.default_rng(1)
    stream = torch.cuda.Stream()
    s = vo.KeyFrameStore(K, n, stream=stream.cuda_stream)
    s.enable_connections(), s.enable_culling()
    s.enable_mapping([500.0, 500.0, 320.0, 240.0, 40.0, 0.08], np.cumprod([1.0] + [1.2] * 7).astype(np.float32), 1 << 20)
    s.enable_local_ba(8, 64, 256), s.enable_pose_graph(4096, 64, 4096), s.enable_point_upkeep(64), s.enable_fuse((0.0, 640.0, 0.0, 480.0), 1024)
    s.enable_loop(4, 1024, 3600), s.enable_loop_fuse(64, 1024), s.enable_loop_correct(64, 4096, 4096), s.enable_loop_merge()
    s.enable_detect_loop(D, G)
    db = vo.KeyFrameDatabase(N_WORDS, K, a.words, 1, stream=stream.cuda_stream)
    vectors = []
    for k in range(K):
        g = k % NB
        s.insert(dict(angle=np.zeros(n, np.float32), desc=np.zeros((n, 32), np.uint8), nodes=np.zeros(n, np.int32), flags=np.full(n, 3, np.uint8),
                      points=rng.normal(0, 2, (n, 3)), ids=(g * IDS_PER_GROUP + rng.integers(0, 2000, n)).astype(np.int32),
                      point_desc=np.zeros((n, 32), np.uint8), min_dist=np.full(n, 0.1, np.float32), max_dist=np.full(n, 50.0, np.float32)))
        words = np.sort(300 * g + rng.choice(600, a.words, replace=False)).astype(np.int32)
        vals = rng.uniform(0.5, 1.5, a.words)
        vectors.append((words, vals / vals.sum()))
    for k in range(K // 5, K // 5 + 5):       # the old pass through the current key-frame's place
        vals = vectors[K - 1][1] * rng.uniform(0.9, 1.1, a.words)
        vectors[k] = (vectors[K - 1][0], vals / vals.sum())
    lonely = K - 3                            # words nobody shares: a call for it finds no candidate and clears the groups
    vectors[lonely] = (np.arange(N_WORDS - a.words, N_WORDS, dtype=np.int32), np.full(a.words, 1.0 / a.words))
    for k in range(K):
        db.insert(*vectors[k])
    s.update_connections(list(range(K)))
    cur = K - 1
    rand = np.arange(12, dtype=np.int32)
    stream.synchronize()

    def timed(fn, reps, sync_inside=False, before=None):
        fn()
        stream.synchronize()
        rows = []
        for _ in range(reps):
            if before:
                before()
                stream.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            e1.record(stream)
            stream.synchronize()
            rows.append(((t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)))
        med = np.median(np.array(rows), 0)
        out = dict(enqueue_ms=float(med[0]), total_ms=float(med[1]), event_ms=float(med[2]), runs_total_ms=[float(r[1]) for r in rows])
        if sync_inside:
            del out["enqueue_ms"]   # (the call waits for the device itself)
        return out

    # ---- the host route: the groups as the caller kept them before the layer existed
    host = dict(groups=[])

    def host_route():
        con = s.connections(cur)                                        # synchronises
        excl = sorted(set(j for j, w in enumerate(con["weights"]) if w != 0) | {cur})
        conn = list(con["ordered"])                                     # (no key-frame of this store is bad)
        cands = [int(c) for c in db.query_loop([vectors[cur]], [excl], connected=[conn], max_out=D)[0]]
        prev, curr, enough = host["groups"], [], []
        flags = [False] * len(prev)
        for c in cands:
            cc = s.connections(c)                                       # getConnectKFs of the candidate: one more read each
            group = set(j for j, w in enumerate(cc["weights"]) if w != 0) | {c}
            some = enough_c = False
            for j, (pg, cnt) in enumerate(prev):
                if group & pg:
                    some = True
                    if not flags[j]:
                        curr.append((group, cnt + 1))
                        flags[j] = True
                    if cnt + 1 >= 3 and not enough_c:
                        enough.append(c)
                        enough_c = True
            if not some:
                curr.append((group, 0))
        host["groups"] = curr if cands else []
        host.update(candidates=cands, enough=enough, n_excl=len(excl), n_conn=len(conn))

    def host_set_neighbors():
        for k in [cur] + host["touched"]:
            db.set_neighbors(k, s.connections(k)["ordered"][:10])
        stream.synchronize()

    res = dict(tool="detect_loop_bench", keyframes=K, features_per_keyframe=n, words_per_keyframe=a.words, reps=a.reps, D=D, G=G,
               version=vo.lib().vo_version().decode(), launches=LAUNCHES)
    # the two routes side by side from the same (empty) group state: candidates and groups must agree call by call
    for call in range(4):
        s.detect_loop(db, cur, 0)
        r = s.detect_loop_result()
        counts, members = s.detect_loop_groups()
        host_route()
        same = (r["candidates"] == host["candidates"] and r["enough"] == host["enough"] and counts == [c for _, c in host["groups"]] and
                [set(int(j) for j in np.flatnonzero(mm)) for mm in members] == [g for g, _ in host["groups"]])
        if not same or s.connections_status() != 0:
            sys.exit("detect_loop_bench: the device route and the host route disagree at call %d; nothing is reported" % call)
    res.update(routes_equal=True, n_excl=r["n_excl"], n_conn=r["n_conn"], n_candidates=r["n_candidates"], outcome_of_call_4=r["outcome"],
               groups=len(counts))
    host["touched"] = [j for j, w in enumerate(s.connections(cur)["weights"]) if w != 0]
    res["device_detect_loop"] = timed(lambda: s.detect_loop(db, cur, 0), a.reps)
    s.last_loop_keyframe = 0
    res["outcome_of_the_timed_calls"] = s.detect_loop_result()["outcome"]
    # the composed step for a key-frame that does not detect: the groups are cleared before every call (a key-frame without
    # candidates does that), so that its candidates are never seen a third time
    quiet = K - 2
    outcomes = set()

    def step_not_detecting():
        outcomes.add(s.loop_closing_step(db, quiet, rand, 2147483647, True, 1)[1]["outcome"])

    res["device_loop_closing_step_one_sync"] = timed(step_not_detecting, a.reps, sync_inside=True, before=lambda: s.detect_loop(db, lonely, 0))
    res["step_record"] = s.loop_closing_record
    if outcomes != {vo.KeyFrameStore.DETECT_NOT_CONSISTENT}:
        sys.exit("detect_loop_bench: the composed step was meant to end NOT_CONSISTENT, it ended %s" % sorted(outcomes))
    res["host_route"] = timed(host_route, a.reps, sync_inside=True)
    res["host_set_neighbors"] = timed(host_set_neighbors, max(1, min(a.reps, 3)), sync_inside=True)
    res["host_set_neighbors"]["rows"] = len(host["touched"]) + 1
    res["host_over_device_total"] = res["host_route"]["total_ms"] / res["device_detect_loop"]["total_ms"]
    res["host_over_step_total"] = res["host_route"]["total_ms"] / res["device_loop_closing_step_one_sync"]["total_ms"]
    print(json.dumps(res))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
