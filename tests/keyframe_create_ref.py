"""Model of vo_kfstore_create_keyframe / vo_kfstore_keyframe_need_stats (test infrastructure): VisualOdometry::createNewKeyFrame
(src/visualOdometry.cpp:463-517) with cullingTempMapPoints' slot rule (:844-853), the first key-frame of initVisualOdometry
(:170-198), Camera::pixel2world (src/camera.cpp:82-94), the MapPoint(KeyFrame*) constructor with addObservation, computeDescriptor
and updateNormalAndDepth for one holder (src/mappoint.cpp:36-179) and the counts of needNewKeyFrame (:406-428), restated on top
of tests/point_upkeep_ref.py's UpkeepModel (the store, the connections, processNewKeyFrame, createNewMapPoints, the refresh).

The definitions are tests/cull_ref.py's: j HOLDS p, j's OBSERVATION of p, obs(p), bad(j).  np.float32 scalars are the reference's
float, Python floats its double, every operation rounded on its own.  The steps are numbered as include/vo_hip.h numbers them.
IEEE leaves the sign and payload of a generated NaN open (x86 produces the negative quiet NaN, the device the positive one), so
the model's outputs carry every NaN as THE positive quiet NaN (canonical()), and the device tests compare after the same step."""
import numpy as np

from new_points_ref import _center, _dot3, feature_vector
from point_upkeep_ref import UpkeepModel

f32 = np.float32
STICKY_INVALID = 1
RECORD = ("keyframe", "n", "n_pairs", "n_walked", "n_created", "n_tracked", "first_id", "next_id", "ended_early", "status")


def canonical(a):
    """every NaN of a float array as the positive quiet NaN"""
    a = np.array(a)
    if a.dtype.kind == "f":
        a[np.isnan(a)] = np.nan
    return a


def pixel2camera(cam, u, v, d):
    """x = ((u - cx) * d) / fx in float (camera.cpp:87-94), widened"""
    fx, fy, cx, cy = (f32(c) for c in cam[:4])
    u, v, d = f32(u), f32(v), f32(d)
    with np.errstate(all="ignore"):
        return [float(((u - cx) * d) / fx), float(((v - cy) * d) / fy), float(d)]


def camera2world(T, pc):
    """p_w = R^T (p_c - t): q = p_c + (-t), p_w[i] = (R[0][i] q[0] + R[1][i] q[1]) + R[2][i] q[2]"""
    with np.errstate(all="ignore"):
        q = [np.float64(pc[c]) + -np.float64(T[9 + c]) for c in range(3)]
        return [float(_dot3(np.float64(T[i]), q[0], np.float64(T[3 + i]), q[1], np.float64(T[6 + i]), q[2])) for i in range(3)]


def single_view(T, p, sf_level, sf_last):
    """updateNormalAndDepth with one holder, in LocalBaModel.refresh's operation order -> (normal, min, max)"""
    with np.errstate(all="ignore"):
        Ow = _center([np.float64(x) for x in T])
        d = [np.float64(p[c]) + -Ow[c] for c in range(3)]
        ln = np.sqrt(_dot3(d[0], d[0], d[1], d[1], d[2], d[2]))
        s = [np.float64(0.0) + d[c] / ln for c in range(3)]
        maxd = f32(ln) * f32(sf_level)
        return [float(s[c] / np.float64(1.0)) for c in range(3)], maxd / f32(sf_last), maxd


def depth_walk(depth, null, th_depth):
    """step 2 -> (pairs sorted, J, [feature of every created pair in walk order]); J = -1 without pairs"""
    th = f32(th_depth)
    pairs = sorted((f32(d), i) for i, d in enumerate(depth) if f32(d) > 0)
    C, J, made = 0, len(pairs) - 1, []
    for j, (d, i) in enumerate(pairs):
        if null[i]:
            C += 1
            made.append(i)
        if d > th and C > 100:
            J = j
            break
    return pairs, J, made


class KeyframeCreateModel(UpkeepModel):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.kc_record = {k: 0 for k in RECORD}
        self.kc_created = []

    def first_observation(self, p):
        """(key-frame, feature) of the lowest non-erased key-frame that holds p, or None"""
        o = self.observations(p) if p >= 0 else []
        return o[0] if o else None

    def create_keyframe(self, f, th_depth, initial=False, nodes=None):
        """f: dict(Tcw12, x, y, octave, angle, depth, u_right, desc, slot_ids); nodes: k_bow_transform's node per feature"""
        n = len(f["depth"])
        T = [float(x) for x in np.asarray(f["Tcw12"], np.float64).reshape(12)]
        depth = [f32(d) for d in f["depth"]]
        octave = [int(o) for o in f["octave"]]
        desc = np.array(f["desc"], np.uint8).reshape(n, 32)
        new = len(self.store)
        # 1 the temp cull
        slot = [-1] * n if initial else [int(p) if self.first_observation(int(p)) else -1 for p in f["slot_ids"]]
        # 2 / 3 the walk
        if initial:
            made = [i for i in range(n) if not depth[i] < 0]
            n_pairs = walked = len(made)
            early = 0
        else:
            pairs, J, made = depth_walk(depth, [s < 0 for s in slot], th_depth)
            n_pairs, walked, early = len(pairs), J + 1, int(J < len(pairs) - 1)
        first_id = self.next_id
        newid = {i: first_id + c for c, i in enumerate(made)}
        self.next_id += len(made)
        # 4 - 6 the map side
        ids, flags, ref = [-1] * n, [0] * n, [-1] * n
        points, normals, pdesc = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 32), np.uint8)
        mind, maxd = np.zeros(n, f32), np.zeros(n, f32)
        for i in range(n):
            if i in newid:
                p = camera2world(T, pixel2camera(self.cam, f["x"][i], f["y"][i], depth[i]))
                nrm, lo, hi = single_view(T, p, self.sf[min(max(octave[i], 0), 15)], self.sf[len(self.sf) - 1])
                ids[i], flags[i], ref[i], points[i], normals[i], pdesc[i], mind[i], maxd[i] = newid[i], 3, new, p, nrm, desc[i], lo, hi
            elif slot[i] >= 0:
                j, g = self.first_observation(slot[i])
                src = self.store[j]
                ids[i], flags[i], ref[i] = slot[i], 3, src["ref"][g]
                points[i], normals[i], pdesc[i], mind[i], maxd[i] = src["points"][g], src["normals"][g], src["pdesc"][g], src["mind"][g], src["maxd"][g]
        # 7 the feature side
        k = self.insert(ids, flags, False, desc, f["angle"], [0] * n if nodes is None else nodes)
        assert k == new
        self.set_keypoints(k, octave, depth, f["u_right"])
        self.set_xy(k, np.stack([np.asarray(f["x"], f32), np.asarray(f["y"], f32)], 1).reshape(n, 2))
        self.set_pose(k, T)
        self.set_point_refs(k, ref)
        kf = self.store[k]
        kf["points"], kf["normals"], kf["pdesc"] = canonical(points), canonical(normals), pdesc
        kf["mind"], kf["maxd"] = canonical(mind), canonical(maxd)
        self.kc_record = dict(keyframe=k, n=n, n_pairs=n_pairs, n_walked=walked, n_created=len(made), n_tracked=sum(1 for s in slot if s >= 0),
                              first_id=first_id, next_id=self.next_id, ended_early=early, status=0)
        self.kc_created = [(i, newid[i]) for i in made]
        return k

    def keyframe_result(self):
        return dict(self.kc_record, created=list(self.kc_created))

    def need_stats(self, ref_kf, min_obs, depth, slot_ids, th_depth):
        """(trackedMapPoints(min_obs) of ref_kf, map_cnt, total_cnt) (:406-428, keyframe.cpp:210-226)"""
        if not 0 <= ref_kf < len(self.store) or self.erased[ref_kf]:
            self.sticky |= STICKY_INVALID
            return 0, 0, 0
        kf, th = self.store[ref_kf], f32(th_depth)
        tracked = sum(1 for i in range(len(kf["ids"])) if (kf["flags"][i] & 1) and kf["ids"][i] >= 0 and self.obs(kf["ids"][i]) >= min_obs)
        near = [i for i, d in enumerate(depth) if f32(d) > 0 and f32(d) < th]
        return tracked, sum(1 for i in near if self.first_observation(int(slot_ids[i]))), len(near)

    def feature_vector(self, k):
        return feature_vector(self.store[k]["nodes"])

    def state(self, k):
        kf = self.store[k]
        return dict(super().state(k), angle=np.array(kf["angle"], f32), desc=np.array(kf["desc"], np.uint8),
                    octave=np.array(kf["octave"], np.int32), depth=np.array(kf["depth"], f32), u_right=np.array(kf["u_right"], f32),
                    xy=np.array(kf["xy"], f32).reshape(-1, 2), feature_vector=[(nd, list(ft)) for nd, ft in self.feature_vector(k)])
