#!/usr/bin/env python3
"""KeyFrame::updateConnections for a key-frame store, both forms in one process run on stores with the same key-frames
(DESIGN.md sections 4h, 7):
  device  vo_kfstore_update_connections_dev on a store with vo_kfstore_enable_connections (three launches; the observation
          index warm, or rebuilt first)
  host    the interface before the device form existed: a host copy of every key-frame's ids and flags kept as the tables F
          and M (built once, not timed), a numpy count matrix C = F M^T (float32 GEMM, exact for these counts), the
          sequential rule over that matrix (weights, mode bits, parents; np.lexsort per touched key-frame), and
          vo_kfstore_set_graph_batch for all key-frames
Store: --keyframes key-frames of --features features, ids as tools/local_map_bench.py draws them: six groups, a key-frame's
ids uniform over 2000 of its group's, so that a key-frame is connected to every key-frame of its group.
Measured, each as the median of --reps after a warm-up, `total_ms` until the stream has drained and (device) `event_ms`
between two events on the store's stream:
  one   update of the last key-frame on the graph of all key-frames (the local-mapping call)
  all   one call listing every key-frame in order on a fresh graph -- the device form cannot reset its state, so the call is
        repeated on the built graph, where it does the same work: the same counts, every step of the sequence, every
        key-frame re-ordered (the first call on the fresh state is reported as `all_first_call`)
  index the one-key-frame call behind an update_points (stale index) minus the warm call: the rebuild's launches
The two forms' graphs (neighbours, parent, children of every key-frame) are compared first and the tool stops if they differ.
Per-kernel times come from a profiler run of this tool (rocprofv3 --kernel-trace --stats), not from the tool.
usage: tools/connections_bench.py [--keyframes 500] [--features 1000] [--reps 7] [--out FILE]"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

IDS_PER_GROUP, NB, THRESHOLD = 4096, 6, 15


def host_tables(ids, flags):
    """F[k][p]: the flagged features of k that carry p; M = F > 0 (the host's resident copy of the store, built once)"""
    F = np.zeros((len(ids), NB * IDS_PER_GROUP), np.float32)
    for k in range(len(ids)):
        np.add.at(F[k], ids[k][(flags[k] & 1) == 1], 1.0)
    return F, (F > 0).astype(np.float32)


def host_counts(F, M, rows):
    """C[rows] = F[rows] M^T with the diagonal zeroed"""
    Cm = (F[rows] @ M.T).astype(np.int32)
    Cm[np.arange(len(rows)), rows] = 0
    return Cm


class HostGraph:
    """the sequential rule over count rows: dense weights, a mode bit per key-frame, parents; lists sorted on demand"""

    def __init__(self, K):
        self.K = K
        self.W = np.zeros((K, K), np.int32)
        self.whole = np.ones(K, bool)
        self.first = np.ones(K, bool)
        self.parent = np.full(K, -1, np.int32)
        self.touched = np.zeros(K, bool)

    def apply(self, k, c):
        if not c.any():
            return
        T = np.nonzero(c >= THRESHOLD)[0]
        if len(T) == 0:
            T = np.array([int(np.argmax(c))])
        ch = T[self.W[T, k] != c[T]]
        self.W[ch, k] = c[ch]
        self.whole[ch] = True
        self.touched[ch] = True
        self.W[k] = c
        self.whole[k] = False
        self.touched[k] = True
        if self.first[k] and k != 0:
            w = c[T]
            self.parent[k] = T[np.lexsort((T, w))[-1]]
            self.first[k] = False
            self.touched[self.parent[k]] = True

    def rows(self):
        """neighbours, children, parents of every key-frame for set_graph_batch"""
        nb, chd = [], []
        for k in range(self.K):
            w = self.W[k]
            sel = np.nonzero(w > 0 if self.whole[k] else w >= THRESHOLD)[0]
            if len(sel) == 0 and not self.whole[k] and w.any():
                sel = np.array([int(np.argmax(w))])
            order = sel[np.lexsort((sel, w[sel]))[::-1]]
            nb.append([int(x) for x in order[:10]])
            chd.append([int(x) for x in np.nonzero(self.parent == k)[0][:64]])
        return nb, chd, [int(x) for x in self.parent]


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
    rng = np.random.default_rng(1)
    kfs = []
    for k in range(K):
        kfs.append(dict(angle=np.zeros(n, np.float32), desc=np.zeros((n, 32), np.uint8), nodes=np.zeros(n, np.int32), flags=np.full(n, 3, np.uint8),
                        points=rng.normal(0, 2, (n, 3)), ids=((k % NB) * IDS_PER_GROUP + rng.integers(0, 2000, n)).astype(np.int32),
                        point_desc=np.zeros((n, 32), np.uint8), min_dist=np.full(n, 0.1, np.float32), max_dist=np.full(n, 50.0, np.float32)))
    F, M = host_tables([kf["ids"] for kf in kfs], [kf["flags"] for kf in kfs])
    stream = torch.cuda.Stream()
    dev = vo.KeyFrameStore(K, n, stream=stream.cuda_stream)
    dev.enable_connections()
    plain = vo.KeyFrameStore(K, n, stream=stream.cuda_stream)
    for kf in kfs:
        dev.insert(kf)
        plain.insert(kf)
    d_all = torch.arange(K, dtype=torch.int32).cuda()
    d_one = torch.tensor([K - 1], dtype=torch.int32).cuda()
    torch.cuda.synchronize()

    def timed(fn, reps, before=None, warm=True):
        if warm:
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
            e1.record(stream)
            stream.synchronize()
            rows.append(((time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)))
        r = np.array(rows)
        med = np.median(r, 0)
        return dict(total_ms=float(med[0]), event_ms=float(med[1]), spread=float((r[:, 0].max() - r[:, 0].min()) / med[0]),
                    runs_total_ms=[float(v) for v in r[:, 0]])

    host_graph = [None]

    def host_all():
        g = HostGraph(K)
        Cm = host_counts(F, M, np.arange(K))
        for k in range(K):
            g.apply(k, Cm[k])
        plain.set_graph_batch(0, *g.rows())
        host_graph[0] = g

    def host_one():
        g = host_graph[0]
        g.apply(K - 1, host_counts(F, M, np.array([K - 1]))[0])
        plain.set_graph_batch(0, *g.rows())

    def stale():   # the same map side again: the observation index is stale, the call that follows rebuilds it
        kf = kfs[K - 1]
        dev.update_points(K - 1, kf["flags"], kf["points"], kf["ids"], kf["point_desc"], kf["min_dist"], kf["max_dist"])

    res = dict(tool="connections_bench", keyframes=K, features_per_keyframe=n, reps=a.reps, version=vo.lib().vo_version().decode(),
               state_bytes=8 * K * K + 20 * K + 16)
    res["all_first_call"] = timed(lambda: dev.update_connections(d_all), 1, warm=False)   # (includes the first index build)
    host_all()
    nb, chd, par = host_graph[0].rows()
    got = [dev.connections(k) for k in range(K)]
    res["graphs_equal"] = bool(all(g["ordered"][:10] == nb[k] and g["children"] == chd[k] and g["parent"] == par[k] for k, g in enumerate(got)))
    if not res["graphs_equal"] or dev.connections_status() != 0:
        sys.exit("connections_bench: the device form and the host form built different graphs; nothing is reported")
    res["connected_median"] = int(np.median([g["n_connected"] for g in got]))
    res["device_all"] = timed(lambda: dev.update_connections(d_all), a.reps)
    res["device_one"] = timed(lambda: dev.update_connections(d_one), a.reps)
    res["device_one_stale_index"] = timed(lambda: dev.update_connections(d_one), a.reps, before=stale)
    res["index_rebuild_ms"] = res["device_one_stale_index"]["event_ms"] - res["device_one"]["event_ms"]
    for key, fn in (("host_all", host_all), ("host_one", host_one)):
        res[key] = timed(fn, max(1, min(a.reps, 3)))
        del res[key]["event_ms"]   # (the host form's work is not on the stream)
    res["speedup_all"] = res["host_all"]["total_ms"] / res["device_all"]["total_ms"]
    res["speedup_one"] = res["host_one"]["total_ms"] / res["device_one"]["total_ms"]
    print(json.dumps(res))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
