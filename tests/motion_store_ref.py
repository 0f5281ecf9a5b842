"""Model of the motion route from the key-frame store (test infrastructure): the slot ids
vo_tracker_build_local_map gathers from the last-frame list after vo_tracker_track_first, the builder itself (tests/local_map_ref.py,
unchanged) on those slots, `link` by id, vo_tracker_point_stats' three rows, and vo_tracker_record_ref_pose /
vo_tracker_refresh_last_pose in csrc/handover_geom.h's operation order (tests/handover_ref.py's compose and inverse)."""
import numpy as np

from handover_ref import compose, inverse
from local_map_ref import build_local_map

f64 = np.float64


def slot_ids(n, has_point, assigned_last, last_ids):
    """one frame: id of slot i when the local-map stage starts -> int32 [cap]; -1: null, a temporary point, beyond n"""
    cap = len(has_point)
    out = np.full(cap, -1, np.int32)
    for i in range(min(max(int(n), 0), cap)):
        a = int(assigned_last[i])
        if has_point[i] and 0 <= a < len(last_ids) and last_ids[a] >= 0:
            out[i] = last_ids[a]
    return out


def build(n, has_point, assigned_last, last_ids, store, max_local):
    """one frame -> (build_local_map's dict, FIRST_SLOT_IDS after the nulling, FEATURE_HAS_POINT after it).  A slot without an id
    (a temporary point) keeps its point; a slot whose id no key-frame holds loses it"""
    ids = slot_ids(n, has_point, assigned_last, last_ids)
    w = build_local_map([int(x) for x in ids], store, max_local)
    after = np.array(w["slots"], np.int32)
    has = np.where((ids >= 0) & (after < 0), 0, np.asarray(has_point)).astype(np.uint8)
    return w, after, has


def link(last_flags, last_ids, local_ids):
    """one frame: per local point the lowest index of the WHOLE last list with its id and bit 0 set, or -1"""
    first = {}
    for i in range(len(last_flags) - 1, -1, -1):
        if (int(last_flags[i]) & 1) and last_ids[i] >= 0:
            first[int(last_ids[i])] = i
    return np.array([first.get(int(p), -1) if p >= 0 else -1 for p in local_ids], np.int32)


def stats(n, first_ids, assigned_local, outlier, local_ids, local_visible, max_local=None):
    """one frame -> (ids, visible, found) int32 [cap + max_local].  first_ids [cap]: the slots when searchLocalMapPoints started;
    local_ids / local_visible: the local map's ids and bit 0 of VO_TRACKER_LOCAL_FLAGS (entries beyond them count as absent)"""
    cap = len(first_ids)
    ml = len(local_ids) if max_local is None else max_local
    ids, vis, fnd = np.full(cap + ml, -1, np.int32), np.zeros(cap + ml, np.int32), np.zeros(cap + ml, np.int32)
    n = min(max(int(n), 0), cap)
    for i in range(n):
        p = int(first_ids[i])
        if p < 0:
            continue
        ids[i], vis[i] = p, 1
        fnd[i] = 1 if assigned_local[i] < 0 and not outlier[i] else 0
    claimed = {}
    for i in range(n):
        a = int(assigned_local[i])
        if 0 <= a < ml and not outlier[i]:
            claimed[a] = True
    for j in range(min(ml, len(local_ids))):
        p = int(local_ids[j])
        if p < 0:
            continue
        v, fd = int(local_visible[j]) & 1, 1 if j in claimed else 0
        if v or fd:
            ids[cap + j], vis[cap + j], fnd[cap + j] = p, v, fd
    return ids, vis, fnd


class RefPoseModel:
    """TcrDB_ and the key-frame it refers to, per frame of the batch"""

    def __init__(self, B):
        self.tcr, self.kf = np.zeros((B, 12)), np.full(B, -1, np.int32)

    @staticmethod
    def _usable(poses, k):
        return 0 <= k < len(poses) and poses[k] is not None

    def record(self, frame_pose, last_valid, ref, poses):
        """ref [B]: dev_ref_kf or LOCAL_REF_KF; poses: per key-frame of the store its Tcw12, None where unset"""
        for f in range(len(self.kf)):
            k = int(ref[f])
            if not self._usable(poses, k):
                k = int(self.kf[f])
            if not self._usable(poses, k) or not last_valid[f]:
                continue
            self.tcr[f], self.kf[f] = compose(frame_pose[f], inverse(poses[k])), k

    def refresh(self, last_pose, poses):
        """-> the last poses [B, 12] after vo_tracker_refresh_last_pose"""
        out = np.array(last_pose, f64).copy()
        for f in range(len(self.kf)):
            k = int(self.kf[f])
            if self._usable(poses, k):
                out[f] = compose(self.tcr[f], poses[k])
        return out
