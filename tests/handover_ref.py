"""Model of vo_tracker_end_frame / vo_tracker_begin_frame (test infrastructure): what VisualOdometry::run does
between two frames (src/visualOdometry.cpp:80-128: cullingTempMapPoints :844-853, Tcl_ :94-103 / :115-118, cullingOutliersOfFrame
:888-895, frame_last_ = frame_curr_ :128) and the preamble of trackWithMotion (:233-236: updateLastFrame's temporary points
:555-592, the start pose), restated per frame of a batch on the arrays the tracker's getters return.

np.float32 scalars are the reference's float, np.float64 scalars its double, every operation rounded on its own, in the order
csrc/handover_geom.h and csrc/keyframe_geom.h write down: compose(), inverse() and the back-projection reproduce the device's
bytes.  exp and log are NOT restated: the model takes the frame's pose as R, t (the device's own FRAME_POSE in the device tests),
and the device's FRAME_POSE / POSE_START are compared with tests/se3_ref.py within the bounds of tests/test_se3_ref.py."""
import numpy as np

from keyframe_create_ref import camera2world, depth_walk, pixel2camera
from new_points_ref import _center, _dot3

f64 = np.float64
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], f64)


def inverse(T):
    """T^-1 of R row-major (9) then t (3): R^T and -(R^T t) (handover_geom.h: ho_inverse)"""
    T = [f64(x) for x in T]
    return np.array([T[3 * j + i] for i in range(3) for j in range(3)] + _center(T), f64)


def compose(A, B):
    """A * B (handover_geom.h: ho_compose)"""
    A, B = [f64(x) for x in A], [f64(x) for x in B]
    R = [_dot3(A[3 * i], B[j], A[3 * i + 1], B[3 + j], A[3 * i + 2], B[6 + j]) for i in range(3) for j in range(3)]
    t = [_dot3(A[3 * i], B[9], A[3 * i + 1], B[10], A[3 * i + 2], B[11]) + A[9 + i] for i in range(3)]
    return np.array(R + t, f64)


def slots(n, assigned_local, assigned_last, has_point, outlier, local, last):
    """steps 1 and 2 of vo_tracker_end_frame for one frame -> (ids, desc, flags) per slot [cap]: the slot rule (local over last),
    observed = bit 1 of the source's flags, cullingTempMapPoints.  flags: 0 null, 3 held, 2 held and an outlier of the second
    solve.  local / last: dict(flags, desc, ids or None); outlier None: the local-map stage did not run"""
    cap = len(assigned_local)
    ids, desc, flags = np.full(cap, -1, np.int32), np.zeros((cap, 32), np.uint8), np.zeros(cap, np.uint8)
    for i in range(n):
        a1, a0 = int(assigned_local[i]), int(assigned_last[i])
        if a1 >= 0:
            src, a = local, a1
        elif a0 >= 0 and has_point[i]:
            src, a = last, a0
        else:
            continue
        if not (int(src["flags"][a]) >> 1) & 1:      # (:848) an unobserved point is a temporary one: the slot becomes null
            continue
        if src.get("ids") is not None and src["ids"][a] >= 0:
            ids[i] = src["ids"][a]
        desc[i] = src["desc"][a]
        flags[i] = 2 if outlier is not None and outlier[i] else 3
    return ids, desc, flags


class HandoverModel:
    """the hand-over state of a tracker of `B` frames: the last pose with its validity, the velocity, the last-frame list"""

    def __init__(self, B, cap, max_last, cam4):
        self.B, self.cap, self.ml, self.cam = B, cap, max_last, [np.float32(c) for c in cam4]
        self.last_pose, self.last_valid = np.zeros((B, 12)), np.zeros(B, np.uint8)
        self.velocity, self.state = np.zeros((B, 12)), np.zeros(B, np.int32)
        self.last = None

    def set_last_pose(self, T, valid):
        self.last_pose, self.last_valid = np.array(T, f64).reshape(self.B, 12), np.array(valid, np.uint8)

    def end_frame(self, s, frame_pose, min_tracked=0):
        """s: the tracker's state before the call -- n [B], assigned_last, assigned_local, has_point, outlier (or None), points
        [B, cap, ..], octave, angle (the frames' columns [B, cap]), status, n_tracked [B], last / local: dict(flags, desc, ids or
        None) of [B, ..] arrays.  frame_pose [B, 12]: R, t of exp(pose).  -> dict of every array the call writes"""
        B, cap, ml = self.B, self.cap, self.ml
        mt = min_tracked if min_tracked > 0 else 30
        out = dict(slot_ids=np.full((B, cap), -1, np.int32), slot_desc=np.zeros((B, cap, 32), np.uint8), frame_pose=np.array(frame_pose, f64),
                   velocity=np.tile(IDENTITY, (B, 1)), motion_state=np.zeros(B, np.int32), last_points=np.zeros((B, ml, 3)),
                   last_flags=np.zeros((B, ml), np.uint8), last_octave=np.zeros((B, ml), np.int32), last_angle=np.zeros((B, ml), np.float32),
                   last_desc=np.zeros((B, ml, 32), np.uint8), last_ids=np.full((B, ml), -1, np.int32), last_n=np.array([cap], np.int32))
        for f in range(B):
            n = min(max(int(s["n"][f]), 0), cap)
            pick = lambda d: {k: (None if v is None else v[f]) for k, v in d.items()}
            ids, desc, flags = slots(n, s["assigned_local"][f], s["assigned_last"][f], s["has_point"][f],
                                     None if s.get("outlier") is None else s["outlier"][f], pick(s["local"]), pick(s["last"]))
            out["slot_ids"][f], out["slot_desc"][f] = ids, desc
            ok = int(s["status"][f]) == 0 and int(s["n_tracked"][f]) >= mt
            if ok and self.last_valid[f]:
                out["velocity"][f] = compose(out["frame_pose"][f], inverse(self.last_pose[f]))
                out["motion_state"][f] = 1
            self.last_pose[f], self.last_valid[f] = out["frame_pose"][f], int(ok)
            held = flags[:n] != 0
            out["last_flags"][f, :n] = flags[:n]
            out["last_ids"][f, :n] = np.where(held, ids[:n], -1)
            out["last_desc"][f, :n] = desc[:n]
            out["last_points"][f, :n] = np.where(held[:, None], np.asarray(s["points"][f][:n], f64), 0.0)
            out["last_octave"][f, :n], out["last_angle"][f, :n] = s["octave"][f][:n], s["angle"][f][:n]
        self.velocity, self.state = out["velocity"].copy(), out["motion_state"].copy()
        self.last = {k[5:]: out[k].copy() for k in ("last_points", "last_flags", "last_octave", "last_angle", "last_desc", "last_ids")}
        return out

    def begin_frame(self, fr, th_depth, is_keyframe=None, local_ids=None):
        """fr: the frame handed over -- n [B], x, y, depth [B, cap], desc [B, cap, 32].  local_ids [B, nq_local] or None (no ids on
        the local map: no link).  -> dict(last_* as they stand now, temp_count, Tcw, link or None)"""
        B, L = self.B, self.last
        out = dict(temp_count=np.zeros(B, np.int32), Tcw=np.zeros((B, 12)), link=None)
        for f in range(B):
            n = min(max(int(fr["n"][f]), 0), self.cap)
            if is_keyframe is None or not is_keyframe[f]:
                null = [(int(L["flags"][f, i]) & 3) != 3 for i in range(n)]
                _, _, made = depth_walk(fr["depth"][f][:n], null, th_depth)
                for i in made:
                    pc = pixel2camera(self.cam, fr["x"][f][i], fr["y"][f][i], fr["depth"][f][i])
                    L["points"][f, i] = camera2world(self.last_pose[f], pc)
                    L["flags"][f, i], L["ids"][f, i], L["desc"][f, i] = 1, -1, fr["desc"][f][i]
                out["temp_count"][f] = len(made)
            out["Tcw"][f] = compose(self.velocity[f], self.last_pose[f])
        if local_ids is not None:
            out["link"] = np.full(np.asarray(local_ids).shape, -1, np.int32)
            for f in range(B):
                first = {}
                for i in range(self.cap - 1, -1, -1):
                    if (L["flags"][f, i] & 1) and L["ids"][f, i] >= 0:
                        first[int(L["ids"][f, i])] = i
                out["link"][f] = [first.get(int(p), -1) if p >= 0 else -1 for p in local_ids[f]]
        out.update({"last_" + k: v.copy() for k, v in L.items()})
        return out
