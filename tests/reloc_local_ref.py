"""trackLocalMap behind a relocalisation on the CPU oracle (test infrastructure): what VisualOdometry::run does to a frame
after a successful relocalization() (src/visualOdometry.cpp:61, :74, :82-83 -> searchLocalMapPoints :726-774, the solve and
the count :287-303).  It starts from the frame state at the end of reloc_ref.relocalize's walk -- slots (ids, -1 = null),
points, outliers, pose -- and runs the oracle's local-map pieces in the order of track_ref.track_frame_ref_keyframe:
isInFrame, the id skip, the search with `occupied`, the solve, the count."""
import ctypes as C

import numpy as np

from track_ref import is_in_frame

FRESH_BASE = 1 << 20  # ids of local points no key-frame of the fixture carries


def local_map_after_reloc(orc, fr, end, observed, local, cam5, sf, W=640, H=480, th_radius=5.0, ratio=0.8):
    """fr: the oracle frame (k, d, ux, uy, ur, depth); end: reloc_ref.relocalize's result; observed(ids) -> bool array:
    observe_cnt_ > 0 of the map points with these ids (bit 1 of the key-frame features' flags); local: dict(points, normals,
    min_dist, max_dist, valid (bit 0 exists, bit 1 observed), desc[, ids]).  -> dict(assigned_local, n_local, pose, inliers,
    n_tracked, outlier, ids, has, n_skipped, n_searched)"""
    k, d, ux, uy, ur = fr[:5]
    n = len(k)
    of = orc.FrameData(ux, uy, k["octave"], k["angle"], ur, d)
    ids = np.asarray(end["ids"], np.int64).copy()
    has = ids >= 0
    fpt = np.asarray(end["points"], np.float64).copy()
    outl = np.asarray(end["outlier"], np.uint8).copy()
    fobs = np.zeros(n, np.uint8)
    fobs[has] = np.asarray(observed(ids[has]), bool)
    valid = np.asarray(local["valid"], np.uint8).copy()
    lid = None if local.get("ids") is None else np.asarray(local["ids"], np.int64)
    skip = np.zeros(len(valid), bool)
    if lid is not None:  # `mp->visualIdxOfFrame_ == frame_curr_->id_` (:753): held by a non-null, non-outlier slot
        held = ids[has & (outl == 0)]
        skip = (valid & 1).astype(bool) & (lid >= 0) & np.isin(lid, held)
    n_searched = int(((valid & 1) != 0).sum() - skip.sum())
    valid[skip] = 0
    pose0 = np.asarray(end["pose"], np.float64)
    a1 = np.full(n, -1, np.int32)
    n1 = 0
    if len(valid) > 0:
        fl, lu, lv, lur, llev, lvc = is_in_frame(orc, pose0, local, valid, cam5, W, H, sf[1])
        n1 = orc.lib().orc_match_local_map(C.byref(of.c), len(fl), fl, lu, lv, lur, llev, lvc, np.ascontiguousarray(local["desc"]),
                                           float(th_radius), float(ratio), sf, fobs, a1)
        new = a1 >= 0
        fpt[new] = np.asarray(local["points"])[a1[new]]
        fobs[new] = (fl[a1[new]] >> 1) & 1
        ids[new] = lid[a1[new]] if lid is not None else -1
        has = has | new
    idx = np.nonzero(has)[0]
    pr = dict(pts=np.ascontiguousarray(fpt[idx]), obs=np.ascontiguousarray(np.stack([ux[idx], uy[idx], ur[idx]], 1).astype(np.float64)),
              inv_sigma=np.ascontiguousarray(1.0 / sf[k["octave"][idx]].astype(np.float64)), cam=np.asarray(cam5, np.float64), pose0=pose0.copy())
    pose, o, ninl, _, _ = orc.pose_only(pr)
    o = np.asarray(o, bool)
    outl[idx] = o  # outliers_ of the problem's features; the others keep their value
    return dict(assigned_local=a1, n_local=int(n1), pose=np.asarray(pose, np.float64), inliers=int(ninl), n_tracked=int(fobs[idx[~o]].sum()),
                outlier=outl, ids=ids, has=has, points=fpt, n_skipped=int(skip.sum()), n_searched=n_searched)


def make_local_map(fr, end, cam5, n_held=60, n_occupied=30, seed=0):
    """A local map around one relocalised frame (true pose = identity): n_held points that carry the id of a slot the frame
    holds (to be skipped), a fresh point behind every null slot (to be found) and n_occupied fresh points in front of slots
    that hold a point (found only where the slot's point has no observations).  -> dict as local_map_after_reloc takes"""
    k, d, ux, uy, ur, dep = fr
    rng = np.random.default_rng(seed)
    ids = np.asarray(end["ids"], np.int64)
    good = np.nonzero((ids >= 0) & (np.asarray(end["outlier"]) == 0))[0]
    held = rng.choice(good, min(n_held, len(good)), replace=False)
    occ = rng.choice(np.setdiff1d(good, held), min(n_occupied, len(good) - len(held)), replace=False)
    null = np.nonzero(ids < 0)[0]
    feat = np.concatenate([held, null, occ])
    z = np.where(dep[feat] > 0, dep[feat], 2.5).astype(np.float64)
    fx, fy, cx, cy = (float(c) for c in cam5[:4])
    P = np.stack([(ux[feat].astype(np.float64) - cx) * z / fx, (uy[feat].astype(np.float64) - cy) * z / fy, z], 1)
    dist = np.linalg.norm(P, axis=1)
    maxd = (dist * 1.2 ** k["octave"][feat].astype(np.float64)).astype(np.float32)
    lid = np.concatenate([ids[held], FRESH_BASE + null, FRESH_BASE + occ]).astype(np.int32)
    order = rng.permutation(len(feat))
    return dict(points=P[order], normals=(P / dist[:, None])[order], min_dist=(maxd / np.float32(1.2 ** 7)).astype(np.float32)[order],
                max_dist=maxd[order], valid=np.full(len(feat), 3, np.uint8), desc=np.ascontiguousarray(d[feat][order]), ids=lid[order])
