"""Inputs of the motion-store tests (tests/test_motion_store_ref.py, tests/test_gpu_motion_store.py):
hand-written tables for vo_tracker_point_stats and for `link` by id, and a synthetic key-frame store over the maps
handover_inputs.tracking_map attaches to the three streams of handover_inputs.streams()."""
import numpy as np

import handover_inputs as hi

ID_STRIDE = 100000      # stream s carries map-point ids s * ID_STRIDE + (tracking_map's id)
FRESH = 50000           # ids of the points only the expansion's key-frame holds
NK = 300                # the store's max_features
KF_PER_STREAM = 4       # two key-frames that vote, one reached through the graph, one that never holds a point


def stats_table():
    """one frame of 8 slots (n = 7) over a 4-entry last list and a 3-entry local map -> (state, want).  state: the slots as
    vo_tracker_track_first left them (has_point, assigned_last), the ids of the last list, the key-frames of a one-key-frame
    store (it holds 100, 102, 200, 201, 202 -- not 103), and what vo_tracker_track_local_map then did"""
    s = dict(n=7, last_ids=np.array([100, 101, -1, 103], np.int32),
             #                      0   1   2   3   4   5   6   7 (beyond n)
             assigned_last=np.array([0, 0, 1, 2, 3, -1, 1, 0], np.int32),
             has_point=np.array([1, 1, 1, 1, 1, 0, 0, 1], np.uint8),
             store=[dict(ids=[200, 201, 202, 100, 102], flags=[3, 1, 3, 1, 3], bad=False, neighbors=[], children=[], parent=-1)],
             local_ids=np.array([200, 201, 202], np.int32), local_visible=np.array([1, 1, 0], np.uint8),
             assigned_local=np.array([-1, -1, 0, -1, -1, 2, -1, 1], np.int32),
             outlier=np.array([0, 1, 0, 0, 0, 1, 0, 0], np.uint8))
    # slot 0 kept (100: visible, found); 1 the same point, an outlier of the second solve (visible only); 2 held 101, which the
    # store does not hold any more: nulled by the builder, then claimed by local point 0 (200: found there); 3 a temporary point
    # (id -1: nothing); 4 held 103, nulled by the builder; 5 never held a point, claimed by local point 2 as an outlier; 6 culled
    # by the first solve; 7 beyond n.  Local point 1 is visible and unclaimed; local point 2 is invisible, claimed, an outlier: gone
    want = dict(first_ids=[100, 100, -1, -1, -1, -1, -1, -1], has_point=[1, 1, 0, 1, 0, 0, 0, 1],
                ids=[100, 100, -1, -1, -1, -1, -1, -1, 200, 201, -1],
                visible=[1, 1, 0, 0, 0, 0, 0, 0, 1, 1, 0],
                found=[1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0])
    # the same frame over a local map the host set, where the local search overwrote slot 1's unobserved point: its old id stays
    # visible, the new one is found
    over = dict(first_ids=np.array([100, 101, -1, -1, -1, -1, -1, -1], np.int32), assigned_local=np.array([-1, 0, -1, -1, -1, -1, -1, -1], np.int32),
                outlier=np.zeros(8, np.uint8), want_ids=[100, 101, -1, -1, -1, -1, -1, -1, 200, 201, -1],
                want_visible=[1, 1, 0, 0, 0, 0, 0, 0, 1, 1, 0], want_found=[1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0])
    return s, want, over


def link_tables():
    """name -> dict(last_flags, last_ids, local_ids, want)"""
    u8, i32 = (lambda a: np.array(a, np.uint8)), (lambda a: np.array(a, np.int32))
    return {
        "duplicate_ids_take_the_lowest_index": dict(last_flags=u8([3, 3, 1, 3, 3]), last_ids=i32([7, 9, 9, 7, 5]), local_ids=i32([9, 7, 5, 4]),
                                                    want=[1, 0, 4, -1]),
        "an_id_with_bit_0_clear_links_to_nothing": dict(last_flags=u8([2, 0, 3, 2]), last_ids=i32([7, 8, 9, 9]), local_ids=i32([7, 8, 9, -1]),
                                                        want=[-1, -1, 2, -1]),
        "a_later_entry_with_bit_0_set_is_taken": dict(last_flags=u8([2, 3, 1]), last_ids=i32([7, 7, -1]), local_ids=i32([7]), want=[1]),
    }


def stream_maps(maps):
    """maps: per stream (Tcw12, last, local) of handover_inputs.tracking_map(first frame's features, seed = stream) -> the same
    with the stream's id offset applied: the three streams share one store"""
    return [(T, dict(last, ids=(last["ids"] + s * ID_STRIDE).astype(np.int32)), dict(local, ids=(local["ids"] + s * ID_STRIDE).astype(np.int32)))
            for s, (T, last, local) in enumerate(maps)]


def store(maps, seed=11):
    """the synthetic store: per stream KF_PER_STREAM key-frames whose features are local points of the stream's map (id, position,
    normal, distances, descriptor, flags = the local point's).  Key-frame 4 s and 4 s + 1 draw 40 .. NK features from 60 % of the
    map (stream 0 the most), so that some slot ids are held by nobody; 4 s + 2 holds points outside that pool under fresh ids
    and is the first neighbour of 4 s; 4 s + 3 holds nothing (every flag has bit 0 clear) and is every other one's child.
    -> list of key-frame dicts in the layout of tests/test_gpu_local_map.py"""
    rng = np.random.default_rng(seed)
    kfs = []
    for s, (_, last, local) in enumerate(maps):
        m = len(local["ids"])
        perm = rng.permutation(m)
        pool, rest = perm[:int(0.6 * m)], perm[int(0.6 * m):]
        base = KF_PER_STREAM * s

        def kf(idx, ids, flags, **graph):
            return dict(ids=np.asarray(ids, np.int32), flags=np.asarray(flags, np.uint8), bad=False,
                        points=np.asarray(local["points"][idx], np.float64), normals=np.asarray(local["normals"][idx], np.float64),
                        min_dist=np.asarray(local["min_dist"][idx], np.float32), max_dist=np.asarray(local["max_dist"][idx], np.float32),
                        point_desc=np.asarray(local["desc"][idx], np.uint8), **graph)
        sizes = [(NK, 220), (150, 90), (60, 40)][s % 3]
        for j, size in enumerate(sizes):
            idx = rng.choice(pool, min(size, len(pool)), replace=False)
            kfs.append(kf(idx, local["ids"][idx], local["valid"][idx], neighbors=[base + 1 - j, base + 2] if j == 0 else [base],
                          children=[base + 3], parent=-1 if j == 0 else base))
        idx = rest[:80]
        kfs.append(kf(idx, s * ID_STRIDE + FRESH + np.arange(len(idx)), local["valid"][idx], neighbors=[base], children=[base + 3], parent=base))
        idx = rest[80:120]
        kfs.append(kf(idx, local["ids"][idx], np.full(len(idx), 2), neighbors=[], children=[], parent=base))
    return kfs


def local_map(w, kfs, max_local):
    """build_local_map's points as the arrays vo_tracker_set_local_map takes -> dict(points, normals, min_dist, max_dist, valid,
    desc, ids), each of len(w["points"]) entries"""
    kk, ii = [p[0] for p in w["points"]], [p[1] for p in w["points"]]
    n = len(kk)
    col = lambda name, shape, dt: np.array([kfs[k][name][i] for k, i in zip(kk, ii)], dt).reshape((n,) + shape)
    return dict(points=col("points", (3,), np.float64), normals=col("normals", (3,), np.float64), min_dist=col("min_dist", (), np.float32),
                max_dist=col("max_dist", (), np.float32), valid=(col("flags", (), np.uint8) & 3).astype(np.uint8),
                desc=col("point_desc", (32,), np.uint8), ids=np.array([p[2] for p in w["points"]], np.int32))


def model_store(kfs):
    return [dict(k, ids=[int(x) for x in k["ids"]], flags=[int(x) for x in k["flags"]]) for k in kfs]
