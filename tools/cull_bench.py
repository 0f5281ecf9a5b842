#!/usr/bin/env python3
"""LocalMapping::cullingKeyFrames for a key-frame store, both forms in one process run on stores with the same key-frames
(DESIGN.md sections 4i, 7):
  device  vo_kfstore_cull_keyframes on a store with connections and culling enabled (count, apply, order; the observation
          index rebuilt in front, as every cull call leaves it stale)
  host    the interface before the device form existed: a host copy of the store (ids, flags, the key-point columns; per id
          the padded table of its holders' key-frame, octave and stereo weight, built once, not timed), the counts in
          numpy, and for an erase the tables edited on the host and the result pushed with vo_kfstore_update_points for every
          key-frame that lost a flag, vo_kfstore_set_bad and vo_kfstore_set_graph_batch on a store without connections
Store: --keyframes key-frames of --features features in groups of --group key-frames (a key-frame's ids uniform over 2000 of
its group's), octaves uniform over 0 .. 7, a tenth of the features without depth, a third stereo; connections built by one
update call that lists every key-frame.  The current key-frame is the last one; its list holds the rest of its group.
Measured, each as the median of --reps after a warm-up, `total_ms` until the stream has drained and (device) `event_ms`
between two events on the store's stream:
  keep   the call as the store stands: the random octaves leave every candidate well below nine tenths, nothing is erased
  erase  the same call after two candidates' octave columns were raised to 7 (every observer passes the gate): both are
         erased.  An erase cannot be undone, so every repetition runs on a fresh pair of stores (--reps of them, built
         first; their index is warm except the first pair's) and there is no warm-up call
  index  the rebuild alone.  Every cull call leaves the index stale, so the keep call always includes it; it is timed
         through vo_kfstore_update_connections_dev for one key-frame, stale minus warm, as tools/connections_bench.py does
The two forms' decisions (key-frame, mp_cnt, re_obs, decision per candidate) and, after the erase, the flags bytes and bad
flags of every key-frame are compared first and the tool stops if they differ.
Per-kernel times come from a profiler run of this tool (rocprofv3 --kernel-trace --stats), not from the tool.
usage: tools/cull_bench.py [--keyframes 500] [--features 1000] [--group 21] [--reps 5] [--out FILE]"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402

from connections_bench import HostGraph, host_counts  # noqa: E402

IDS_PER_GROUP, SPAN, TH = 4096, 2000, 5.0


class HostStore:
    """the host's resident copy: per key-frame ids, flags, octave, depth, u_right; per id the holders' table"""

    def __init__(self, kfs, n_ids):
        self.kfs = [dict(ids=k["ids"].copy(), flags=k["flags"].copy(), octave=k["octave"].copy(), depth=k["depth"].copy(),
                         u_right=k["u_right"].copy()) for k in kfs]
        K = len(kfs)
        self.bad, self.erased = np.zeros(K, bool), np.zeros(K, bool)
        rows = [[] for _ in range(n_ids)]
        for k, kf in enumerate(self.kfs):
            seen = set()
            for i in np.nonzero(kf["flags"] & 1)[0]:
                p = int(kf["ids"][i])
                if p not in seen:   # the observation: the lowest-numbered flagged feature
                    seen.add(p)
                    rows[p].append((k, int(kf["octave"][i]), 2 if kf["u_right"][i] >= 0 else 1))
        width = max(len(r) for r in rows)
        self.hk = np.full((n_ids, width), -1, np.int32)    # holder key-frames, ascending; -1: none
        self.ho = np.zeros((n_ids, width), np.int32)       # their observation's octave
        self.hw = np.zeros((n_ids, width), np.int32)       # 2 stereo / 1 mono
        for p, r in enumerate(rows):
            for c, (k, o, w) in enumerate(r):
                self.hk[p, c], self.ho[p, c], self.hw[p, c] = k, o, w

    def count(self, k):
        kf = self.kfs[k]
        sel = ((kf["flags"] & 1) == 1) & ~((kf["depth"] < 0) | (kf["depth"] > np.float32(TH)))
        ids, lvl = kf["ids"][sel], kf["octave"][sel]
        hk, live = self.hk[ids], self.hk[ids] >= 0
        obs = (self.hw[ids] * live).sum(1)
        others = live & (hk != k) & ~self.bad[np.where(live, hk, 0)] & (self.ho[ids] <= (lvl + 1)[:, None])
        return int(sel.sum()), int(((obs > 3) & (others.sum(1) >= 3)).sum())

    def erase(self, k, g):
        """eraseKeyFrame on the tables and the graph g -> the key-frames that lost a flag"""
        nb = np.nonzero(g.W[k])[0]
        rec = nb[g.W[nb, k] != 0]
        g.W[rec, k] = 0
        g.whole[rec] = True
        kf = self.kfs[k]
        flagged = np.nonzero(kf["flags"] & 1)[0]
        ids = np.unique(kf["ids"][flagged])
        mine = self.hk[ids] == k
        left = (self.hw[ids] * (self.hk[ids] >= 0) * ~mine).sum(1)
        dead = ids[left <= 2]
        changed = set()
        for p in dead:
            for j in self.hk[p][self.hk[p] >= 0]:
                f = self.kfs[j]
                f["flags"][f["ids"] == p] &= 0xfe
                changed.add(int(j))
            self.hk[p] = -1
        r, c = np.nonzero(mine)
        self.hk[ids[r], c] = -1
        g.W[k] = 0
        g.whole[k] = True
        # the spanning tree: the rule of keyframe.cpp:429-485 over the children's lists
        parent = int(g.parent[k])
        cands = [parent] if parent >= 0 else []
        children = [int(c) for c in np.nonzero((g.parent == k) & ~self.erased)[0]]
        lists = {}
        for ch in children:
            w = g.W[ch]
            s = np.nonzero(w > 0 if g.whole[ch] else w >= 15)[0]
            if len(s) == 0 and not g.whole[ch] and w.any():
                s = np.array([int(np.argmax(w))])
            lists[ch] = s[np.lexsort((s, w[s]))[::-1]]
        while children:
            best, pick = -1, None
            for ch in children:
                if self.bad[ch]:
                    continue
                for x in lists[ch]:
                    if x in cands and g.W[ch, x] > best:
                        best, pick = g.W[ch, x], (ch, int(x))
            if pick is None:
                break
            g.parent[pick[0]] = pick[1]
            cands.append(pick[0])
            children.remove(pick[0])
        for ch in children:
            g.parent[ch] = parent
        self.erased[k] = self.bad[k] = True
        return changed

    def cull(self, cur, order, g, push):
        """-> [(key-frame, mp_cnt, re_obs, decision)]; push(changed key-frames, erased key-frames) uploads an erase"""
        out, changed, gone = [], set(), []
        for k in order:
            if k == 0 or self.bad[k]:
                out.append((k, 0, 0, 3))
                continue
            mp, re = self.count(k)
            if re > 0.9 * mp:
                changed |= self.erase(k, g)
                gone.append(k)
            out.append((k, mp, re, 1 if k in gone else 0))
        if gone:
            push(sorted(changed), gone)
        return out


def graph_rows(g, erased):
    saved = g.parent.copy()
    g.parent = np.where(erased, -2, saved)   # (an erased key-frame has left its parent's children)
    nb, chd, _ = g.rows()
    g.parent = saved
    return nb, chd, [int(x) for x in saved]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=500)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--group", type=int, default=21)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from vo_slam_test_amd import _lib as vo
    K, n = a.keyframes, a.features
    NB = (K + a.group - 1) // a.group   # groups: key-frame k belongs to k % NB
    rng = np.random.default_rng(1)
    kfs = []
    for k in range(K):
        kfs.append(dict(angle=np.zeros(n, np.float32), desc=np.zeros((n, 32), np.uint8), nodes=np.zeros(n, np.int32), flags=np.full(n, 3, np.uint8),
                        points=rng.normal(0, 2, (n, 3)), ids=((k % NB) * IDS_PER_GROUP + rng.integers(0, SPAN, n)).astype(np.int32),
                        point_desc=np.zeros((n, 32), np.uint8), min_dist=np.full(n, 0.1, np.float32), max_dist=np.full(n, 50.0, np.float32),
                        octave=rng.integers(0, 8, n).astype(np.int32),
                        depth=np.where(rng.random(n) < 0.1, -1.0, rng.uniform(0.5, TH, n)).astype(np.float32),
                        u_right=np.where(rng.random(n) < 0.33, rng.uniform(1, 600, n), -1.0).astype(np.float32)))
    cur = K - 1
    stream = torch.cuda.Stream()
    d_all = torch.arange(K, dtype=torch.int32).cuda()
    d_one = torch.tensor([cur], dtype=torch.int32).cuda()

    def build_pair():
        dev = vo.KeyFrameStore(K, n, stream=stream.cuda_stream)
        dev.enable_connections()
        dev.enable_culling()
        plain = vo.KeyFrameStore(K, n, stream=stream.cuda_stream)
        for k, kf in enumerate(kfs):
            dev.insert(kf)
            dev.set_keypoints(k, kf["octave"], kf["depth"], kf["u_right"])
            plain.insert(kf)
        dev.update_connections(d_all)
        return dev, plain

    def host_graph():
        F = np.zeros((K, NB * IDS_PER_GROUP), np.float32)
        for k in range(K):
            np.add.at(F[k], kfs[k]["ids"], 1.0)
        Cm = host_counts(F, (F > 0).astype(np.float32), np.arange(K))
        g = HostGraph(K)
        for k in range(K):
            g.apply(k, Cm[k])
        return g

    def timed(fn, reps, before=None, warm=True):
        if warm:
            fn()
            stream.synchronize()
        rows = []
        for r in range(reps):
            if before:
                before()
                stream.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            fn(r) if not warm else fn()
            e1.record(stream)
            stream.synchronize()
            rows.append(((time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)))
        r = np.array(rows)
        med = np.median(r, 0)
        return dict(total_ms=float(med[0]), event_ms=float(med[1]), spread=float((r[:, 0].max() - r[:, 0].min()) / med[0]),
                    runs_total_ms=[float(v) for v in r[:, 0]])

    dev, plain = build_pair()
    torch.cuda.synchronize()
    order = dev.connections(cur)["ordered"]
    res = dict(tool="cull_bench", keyframes=K, features_per_keyframe=n, reps=a.reps, version=vo.lib().vo_version().decode(),
               candidates=len(order), culling_bytes=12 * K * n + 28 * K + 16)
    host = HostStore(kfs, NB * IDS_PER_GROUP)
    g = host_graph()
    # ---- keep: nothing is erased
    dev.cull_keyframes(cur, TH)
    got = dev.cull_result()
    want = host.cull(cur, order, g, None)
    if got != want or any(r[3] == 1 for r in got):
        sys.exit("cull_bench: the two forms decide differently, or the keep call erased something; nothing is reported")
    res["keep_ratio_max"] = max(r[2] / max(r[1], 1) for r in got)
    res["device_keep"] = timed(lambda: dev.cull_keyframes(cur, TH), a.reps)
    res["host_keep"] = timed(lambda: host.cull(cur, order, g, None), max(1, min(a.reps, 3)))
    del res["host_keep"]["event_ms"]   # (the host form's work is not on the stream)
    stale = lambda: dev.update_points(cur, kfs[cur]["flags"], kfs[cur]["points"], kfs[cur]["ids"], kfs[cur]["point_desc"], kfs[cur]["min_dist"],
                                      kfs[cur]["max_dist"])
    one_warm = timed(lambda: dev.update_connections(d_one), a.reps)
    one_stale = timed(lambda: dev.update_connections(d_one), a.reps, before=stale)
    res["index_rebuild_ms"] = one_stale["event_ms"] - one_warm["event_ms"]
    # ---- erase: two candidates made redundant, a fresh pair of stores per repetition
    victims = [k for k in order if k != 0][1:3]
    pairs = [(dev, plain)] + [build_pair() for _ in range(a.reps - 1)]
    hosts, graphs = [], []
    for d, _ in pairs:
        for v in victims:
            kfs_v = dict(kfs[v], octave=np.full(n, 7, np.int32))
            d.set_keypoints(v, kfs_v["octave"], kfs_v["depth"], kfs_v["u_right"])
        hosts.append(HostStore([dict(kf, octave=np.full(n, 7, np.int32)) if k in victims else kf for k, kf in enumerate(kfs)],
                               NB * IDS_PER_GROUP))
        graphs.append(host_graph())
    torch.cuda.synchronize()

    def push_to(r):
        def push(changed, gone):
            p, h = pairs[r][1], hosts[r]
            for j in changed:
                p.update_points(j, h.kfs[j]["flags"], kfs[j]["points"], kfs[j]["ids"], kfs[j]["point_desc"], kfs[j]["min_dist"], kfs[j]["max_dist"])
            for k in gone:
                p.set_bad(k)
            p.set_graph_batch(0, *graph_rows(graphs[r], h.erased))
        return push

    results = [None] * len(pairs)

    def host_erase(r):
        results[r] = hosts[r].cull(cur, order, graphs[r], push_to(r))

    res["device_erase"] = timed(lambda r: pairs[r][0].cull_keyframes(cur, TH), len(pairs), warm=False)
    res["host_erase"] = timed(host_erase, len(pairs), warm=False)
    del res["host_erase"]["event_ms"]
    for r, (d, p) in enumerate(pairs):
        same = d.cull_result() == results[r] and sorted(k for k, _, _, dec in results[r] if dec == 1) == sorted(victims)
        same = same and all(d.flags(k) == p.flags(k) for k in range(K))
        same = same and all(d.connections(k)["parent"] == int(graphs[r].parent[k]) for k in range(K))
        if not same or d.connections_status() != 0:
            sys.exit("cull_bench: the device form and the host form erased differently; nothing is reported")
    res["erased"] = victims
    res["flags_changed_keyframes"] = int(sum(1 for k in range(K) if not np.array_equal(hosts[0].kfs[k]["flags"], kfs[k]["flags"])))
    res["speedup_keep"] = res["host_keep"]["total_ms"] / res["device_keep"]["total_ms"]
    res["speedup_erase"] = res["host_erase"]["total_ms"] / res["device_erase"]["total_ms"]
    print(json.dumps(res))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
