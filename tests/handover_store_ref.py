"""Model of vo_tracker_end_frame_store / vo_tracker_point_stats_store (test infrastructure): the hand-over
and the addVisible / addFound rows behind a relocalisation from the key-frame store and behind trackRefKeyFrame from the store.
What is new against tests/handover_ref.py is step 1 only -- where a slot's map point comes from (the two slot-source rules) and
its descriptor (the store's point descriptor at the lowest holder of the id) --; steps 2-5 are HandoverModel.end_frame's,
called unchanged on a state in which every slot's source is written out as a one-entry-per-slot table.

store: list of key-frames, each dict(ids, flags, point_desc) (the layout of tests/test_gpu_local_map.py); size: the store's
size (default: all of them).  ROUTE_RELOC = 1, ROUTE_REF = 2 are vo_tracker_build_local_map's route numbers."""
import numpy as np

from handover_ref import HandoverModel
from motion_store_ref import stats

ROUTE_RELOC, ROUTE_REF = 1, 2


def first_holder(store, pid, size=None):
    """the id's first key of the observation index: the lowest (key-frame, feature) with flags bit 0 that holds it, below size ->
    (k, i) or None"""
    return holders(store, size).get(int(pid))


def holders(store, size=None):
    """id -> its first key (k, i), for every id a key-frame below size holds with flags bit 0"""
    size = len(store) if size is None else size
    out = {}
    for k in range(min(size, len(store)) - 1, -1, -1):
        ids, flags = np.asarray(store[k]["ids"]), np.asarray(store[k]["flags"])
        for i in range(len(ids) - 1, -1, -1):
            if int(flags[i]) & 1:
                out[int(ids[i])] = (k, i)
    return out


def kept_ids(route, n, has_point, store, size=None, frame_ids=None, failed=False, assigned_last=None, ref_kf=-1):
    """one frame: the id of every non-null slot as the route left it before the local search -> int32 [cap], -1: null / no id.
    relocalisation: frame_ids (VO_TRACKER_RELOC_POINT_IDS), nothing when the relocalisation failed; reference key-frame:
    store[ref_kf].ids[assigned_last[i]], the key-frame in [0, size) and the match below its feature count"""
    cap = len(has_point)
    size = len(store) if size is None else size
    out = np.full(cap, -1, np.int32)
    if failed:
        return out
    for i in range(min(max(int(n), 0), cap)):
        if not has_point[i]:
            continue
        if route == ROUTE_RELOC:
            p = int(frame_ids[i])
        else:
            a0, p = int(assigned_last[i]), -1
            if 0 <= int(ref_kf) < size and 0 <= a0 < len(store[int(ref_kf)]["ids"]):
                p = int(store[int(ref_kf)]["ids"][a0])
        out[i] = p if p >= 0 else -1
    return out


def slot_ids(route, kept, n, assigned_local, local_ids, failed=False):
    """one frame: the id slot i is handed over with, before the cullings.  Reference key-frame: local over kept; relocalisation:
    kept alone (the local search's claims are in the frame's id array already)"""
    out = np.asarray(kept, np.int32).copy()
    if route == ROUTE_REF and not failed:
        for i in range(min(max(int(n), 0), len(out))):
            a1 = int(assigned_local[i])
            if a1 >= 0:
                out[i] = local_ids[a1] if a1 < len(local_ids) and local_ids[a1] >= 0 else -1
    return out


def end_state(route, s, store, size=None):
    """s: the tracker's state before the call, [B, ..] arrays -- n, has_point, assigned_local, observed, outlier, points, octave,
    angle, status, n_tracked, local_ids, and frame_ids + winner (relocalisation) or assigned_last + ref_kf (reference key-frame).
    -> the state HandoverModel.end_frame takes: slot i's source is entry i of a table of its own (id, descriptor of the lowest
    holder, observed mark); a slot whose id nobody holds is null (the deviation of section 4w)"""
    B, cap = np.asarray(s["has_point"]).shape
    ids, desc = np.full((B, cap), -1, np.int32), np.zeros((B, cap, 32), np.uint8)
    flags, a1 = np.zeros((B, cap), np.uint8), np.full((B, cap), -1, np.int32)
    status = np.array(s["status"], np.int32).copy()
    index = holders(store, size)
    for f in range(B):
        failed = route == ROUTE_RELOC and int(s["winner"][f]) < 0
        if failed:
            status[f] = status[f] if status[f] != 0 else 4      # (VO_TRACK_RELOC_FAILED: ok = 0 whatever else the block says)
        kept = kept_ids(route, s["n"][f], s["has_point"][f], store, size, frame_ids=None if route != ROUTE_RELOC else s["frame_ids"][f],
                        failed=failed, assigned_last=None if route != ROUTE_REF else s["assigned_last"][f],
                        ref_kf=-1 if route != ROUTE_REF else s["ref_kf"][f])
        sid = slot_ids(route, kept, s["n"][f], s["assigned_local"][f], s["local_ids"][f], failed)
        for i in range(min(max(int(s["n"][f]), 0), cap)):
            at = index.get(int(sid[i])) if sid[i] >= 0 else None
            if at is None:
                continue
            ids[f, i], desc[f, i], a1[f, i] = sid[i], store[at[0]]["point_desc"][at[1]], i
            flags[f, i] = 1 | (2 if s["observed"][f][i] else 0)
    table = dict(flags=flags, desc=desc, ids=ids)
    none = dict(flags=np.zeros((B, 1), np.uint8), desc=np.zeros((B, 1, 32), np.uint8), ids=None)
    return dict(n=s["n"], assigned_local=a1, assigned_last=np.full((B, cap), -1, np.int32), has_point=(a1 >= 0).astype(np.uint8),
                outlier=s["outlier"], points=s["points"], octave=s["octave"], angle=s["angle"], status=status, n_tracked=s["n_tracked"],
                local=table, last=none)


def end_frame(model, route, s, store, frame_pose, min_tracked=0, size=None):
    """vo_tracker_end_frame_store on HandoverModel `model` -> every array the call writes"""
    assert isinstance(model, HandoverModel)
    return model.end_frame(end_state(route, s, store, size), frame_pose, min_tracked)


def stats_rows(route, n, kept, assigned_local, outlier, local_ids, local_visible, max_local, failed=False):
    """one frame -> (ids, visible, found) int32 [cap + max_local].  Segment A: a kept slot the local search did not claim, visible,
    found iff no outlier; segment B: tests/motion_store_ref.py's (local_visible: bit 0 of VO_TRACKER_LOCAL_FLAGS -- behind a
    relocalisation a point skipped by id has it clear).  A failed relocalisation: -1 / 0"""
    cap = len(kept)
    ids, vis, fnd = stats(0 if failed else n, np.full(cap, -1, np.int32), assigned_local, outlier, [] if failed else local_ids,
                          [] if failed else local_visible, max_local=max_local)
    if not failed:
        for i in range(min(max(int(n), 0), cap)):
            if kept[i] >= 0 and assigned_local[i] < 0:
                ids[i], vis[i], fnd[i] = kept[i], 1, 0 if outlier[i] else 1
    return ids, vis, fnd
