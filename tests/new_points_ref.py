"""Model of vo_kfstore_create_map_points (test infrastructure): LocalMapping::createNewMapPoints (src/localMapping.cpp:132-361)
with computeF12 (:526-536), Matcher::searchForTriangulation (src/matcher.cpp:867-1010) and, for a point with two holders, the
MapPoint constructor, computeDescriptor and updateNormalAndDepth (src/mappoint.cpp:36-179), restated in numpy on top of
tests/cull_ref.py's CullModel (the store, the connections, the erase).

Types: a Python float is the reference's double (IEEE, every operation rounded on its own, no contraction); np.float32 scalars
are its float.  geometry() follows the operation order DESIGN.md section 4j writes down for the device function, so that F12,
the epipole and the baseline agree with the device bit for bit.  The linear triangulation is np.linalg.svd of the float32
matrix (the device restates it as a Jacobi eigen-decomposition of A^T A: parity within TAU, include/vo_hip.h vo_triangulate).

Every evaluated match carries its DECISIVENESS (evaluate): whether a device result within the stated tolerances could decide
a gate differently.  The GPU inputs contain no match that is not decisive (tests/test_new_points_ref.py asserts that)."""
import math

import numpy as np

from cull_ref import CullModel

f32 = np.float32
TAU = 1e-4   # the relative tolerance include/vo_hip.h states for vo_triangulate against cv::SVD
SEARCHED, SKIPPED_BAD, SKIPPED_BASELINE, SKIPPED_NO_POSE, NOT_REACHED = range(5)
TH_LOW, HISTO_LENGTH = 50, 30


# ---- geometry: the documented operation order -------------------------------------------------------------------------------
def _dot3(a, b, c, d, e, f):
    return (a * b + c * d) + e * f


def _center(T):
    return [-_dot3(T[i], T[9], T[3 + i], T[10], T[6 + i], T[11]) for i in range(3)]


def geometry(T1, T2, cam):
    """T: 12 doubles, R row-major then t.  -> dict(F [9], ex, ey, bl (float32), Ow1, Ow2)"""
    T1, T2 = [float(x) for x in T1], [float(x) for x in T2]
    fx, fy, cx, cy = (float(f32(c)) for c in cam[:4])
    Ow1, Ow2 = _center(T1), _center(T2)
    d = [Ow2[i] + -Ow1[i] for i in range(3)]
    bl = f32(math.sqrt(_dot3(d[0], d[0], d[1], d[1], d[2], d[2])))
    R12 = [_dot3(T1[3 * i], T2[3 * j], T1[3 * i + 1], T2[3 * j + 1], T1[3 * i + 2], T2[3 * j + 2]) for i in range(3) for j in range(3)]
    t12 = [T1[9 + i] + -_dot3(R12[3 * i], T2[9], R12[3 * i + 1], T2[10], R12[3 * i + 2], T2[11]) for i in range(3)]
    M = [0.0] * 9
    for j in range(3):
        M[j] = (-t12[2]) * R12[3 + j] + t12[1] * R12[6 + j]
        M[3 + j] = t12[2] * R12[j] + (-t12[0]) * R12[6 + j]
        M[6 + j] = (-t12[1]) * R12[j] + t12[0] * R12[3 + j]
    ifx, ify = 1.0 / fx, 1.0 / fy
    mcx, mcy = -(cx * ifx), -(cy * ify)
    N = [0.0] * 9
    for i in range(3):
        N[3 * i] = M[3 * i] * ifx
        N[3 * i + 1] = M[3 * i + 1] * ify
        N[3 * i + 2] = (M[3 * i] * mcx + M[3 * i + 1] * mcy) + M[3 * i + 2]
    F = [0.0] * 9
    for j in range(3):
        F[j] = ifx * N[j]
        F[3 + j] = ify * N[3 + j]
        F[6 + j] = (mcx * N[j] + mcy * N[3 + j]) + N[6 + j]
    C2 = [_dot3(T2[3 * i], Ow1[0], T2[3 * i + 1], Ow1[1], T2[3 * i + 2], Ow1[2]) + T2[9 + i] for i in range(3)]
    with np.errstate(all="ignore"):
        ex = f32(np.float64(fx * C2[0]) / np.float64(C2[2]) + cx)
        ey = f32(np.float64(fy * C2[1]) / np.float64(C2[2]) + cy)
    return dict(F=F, ex=ex, ey=ey, bl=bl, Ow1=Ow1, Ow2=Ow2, T1=T1, T2=T2)


# ---- searchForTriangulation ---------------------------------------------------------------------------------------------------
def feature_vector(nodes):
    """DBoW3::FeatureVector: [(node id, [features in index order])] in ascending node id"""
    fv = {}
    for i, nd in enumerate(nodes):
        fv.setdefault(int(nd), []).append(i)
    return sorted(fv.items())


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def _epipolar_ok(x1, y1, x2, y2, F, sigma):
    x1, y1, x2, y2 = float(x1), float(y1), float(x2), float(y2)
    l0, l1, l2 = x1 * F[0] + y1 * F[3] + F[6], x1 * F[1] + y1 * F[4] + F[7], x1 * F[2] + y1 * F[5] + F[8]
    num, den = f32(l0 * x2 + l1 * y2 + l2), f32(l0 * l0 + l1 * l1)
    if den == 0:
        return False
    return num * num / den < f32(3.84) * sigma * sigma


def three_max(sizes):
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(sizes):
        if s > m1:
            m3, i3, m2, i2, m1, i1 = m2, i2, m1, i1, s, i
        elif s > m2:
            m3, i3, m2, i2 = m2, i2, s, i
        elif s > m3:
            m3, i3 = s, i
    if f32(m2) < f32(0.1) * f32(m1):
        i2 = i3 = -1
    elif f32(m3) < f32(0.1) * f32(m1):
        i3 = -1
    return i1, i2, i3


def search(A, B, a_has, b_has, F, ex, ey, sf, check_rot=True):
    """A, B: dict(x, y, u_right, octave, angle (float32 arrays), desc [n, 32], nodes) -> (match12 [nA], match_cnt, claims): claims
    = every (idx1, idx2) the walk claimed, those the rotation check removed included"""
    nA = len(A["x"])
    match12, matched2 = [-1] * nA, [False] * len(B["x"])
    hist = [[] for _ in range(HISTO_LENGTH)]
    pdf = f32(HISTO_LENGTH) / f32(360.0)
    fvB = dict(feature_vector(B["nodes"]))
    claims, cnt = [], 0
    for node, feats in feature_vector(A["nodes"]):
        if node not in fvB:
            continue
        for i1 in feats:
            if a_has[i1]:
                continue
            stereo1 = A["u_right"][i1] >= 0
            best, bidx = TH_LOW, -1
            for i2 in fvB[node]:
                if matched2[i2] or b_has[i2]:
                    continue
                d = hamming(A["desc"][i1], B["desc"][i2])
                if d > TH_LOW or d > best:
                    continue
                sigma = f32(sf[B["octave"][i2]])
                if not stereo1 and not (B["u_right"][i2] >= 0):
                    dx, dy = f32(ex) - f32(B["x"][i2]), f32(ey) - f32(B["y"][i2])
                    if dx * dx + dy * dy < f32(100) * sigma:
                        continue
                if _epipolar_ok(A["x"][i1], A["y"][i1], B["x"][i2], B["y"][i2], F, sigma):
                    best, bidx = d, i2
            if bidx >= 0:
                match12[i1], matched2[bidx] = bidx, True
                claims.append((i1, bidx))
                if check_rot:
                    rot = f32(A["angle"][i1]) - f32(B["angle"][bidx])
                    if rot < 0:
                        rot = rot + f32(360.0)
                    b = int(math.floor(float(rot * pdf) + 0.5))
                    hist[0 if b == HISTO_LENGTH else b].append(i1)
                cnt += 1
    if check_rot:
        keep = three_max([len(h) for h in hist])
        for b in range(HISTO_LENGTH):
            if b not in keep:
                for i1 in hist[b]:
                    match12[i1] = -1
                    cnt -= 1
    return match12, cnt, claims


# ---- one match (:197-341) -----------------------------------------------------------------------------------------------------
def _pixel2camera(cam, u, v, z):
    fx, fy, cx, cy = (f32(c) for c in cam[:4])
    z = f32(z)
    return [float((f32(u) - cx) * z / fx), float((f32(v) - cy) * z / fy), float(z)]


def _back_project(cam, u, v, depth, T, Ow):
    pc = _pixel2camera(cam, u, v, depth)
    return [(T[i] * pc[0] + T[3 + i] * pc[1] + T[6 + i] * pc[2]) + Ow[i] for i in range(3)]


def triangulate_svd(pc1, pc2, T1, T2):
    """the float32 4 x 4 system of :234-238 through np.linalg.svd -> (point as 3 doubles, or None when |x3| < 1e-8)"""
    T1f = np.array([[T1[3 * r], T1[3 * r + 1], T1[3 * r + 2], T1[9 + r]] for r in range(3)], f32)
    T2f = np.array([[T2[3 * r], T2[3 * r + 1], T2[3 * r + 2], T2[9 + r]] for r in range(3)], f32)
    A = np.stack([f32(pc1[0]) * T1f[2] - T1f[0], f32(pc1[1]) * T1f[2] - T1f[1], f32(pc2[0]) * T2f[2] - T2f[0], f32(pc2[1]) * T2f[2] - T2f[1]])
    x = np.linalg.svd(A.astype(f32))[2][3]
    if abs(float(x[3])) < 1e-8:
        return None
    return [float(f32(x[i]) / f32(x[3])) for i in range(3)]


def _far(a, b):
    """the operands of a float comparison differ by more than 4 ulps (atan2, cos, the cast, the dot product: one each)"""
    a, b = float(a), float(b)
    return abs(a - b) > 4 * float(np.spacing(f32(max(abs(a), abs(b)))))


def gates(G, cam, sf, f1, f2, p):
    """the decisions behind the choice of the point, in order, up to the first that rejects -> (accepted, signature, dist1)"""
    fx, fy, cx, cy, bf = (f32(c) for c in cam[:5])
    T1, T2 = G["T1"], G["T2"]
    sig = []

    def decide(ok):
        sig.append(bool(ok))
        return bool(ok)

    z1 = f32((T1[6] * p[0] + T1[7] * p[1] + T1[8] * p[2]) + T1[11])
    if not decide(z1 > 0):
        return False, sig, None
    z2 = f32((T2[6] * p[0] + T2[7] * p[1] + T2[8] * p[2]) + T2[11])
    if not decide(z2 > 0):
        return False, sig, None
    s1, s2 = f32(sf[f1["octave"]]), f32(sf[f2["octave"]])
    for T, z, s, f in ((T1, z1, s1, f1), (T2, z2, s2, f2)):
        x = f32((T[0] * p[0] + T[1] * p[1] + T[2] * p[2]) + T[9])
        y = f32((T[3] * p[0] + T[4] * p[1] + T[5] * p[2]) + T[10])
        invz, inv_sigma = f32(1.0) / z, f32(1.0) / s
        u, v = fx * x * invz + cx, fy * y * invz + cy
        eu, ev = u - f32(f["u"]), v - f32(f["v"])
        e = eu * eu + ev * ev
        if not (f["ur"] >= 0):
            ok = not (e * inv_sigma * inv_sigma > f32(5.991))
        else:
            er = (u - bf * invz) - f32(f["ur"])
            ok = not ((e + er * er) * inv_sigma * inv_sigma > f32(7.815))
        if not decide(ok):
            return False, sig, None
    dist1 = f32(math.sqrt(sum((p[i] - G["Ow1"][i]) ** 2 for i in range(3))))
    dist2 = f32(math.sqrt(sum((p[i] - G["Ow2"][i]) ** 2 for i in range(3))))
    if not decide(not (float(dist1) < 1e-6 or float(dist2) < 1e-6)):
        return False, sig, None
    ratio, scale_ratio, factor = dist2 / dist1, s1 / s2, f32(1.5) * f32(sf[1])
    if not decide(not (ratio * factor < scale_ratio)):
        return False, sig, None
    if not decide(not (ratio > scale_ratio * factor)):
        return False, sig, None
    return True, sig, dist1


def evaluate(G, cam, sf, f1, f2):
    """f: dict(u, v, ur, depth, octave) -> dict(kind: 'svd' | 'depth1' | 'depth2' | 'none' | 'degenerate', accepted, p, dist1,
    decisive)"""
    b = float(f32(cam[5]))
    stereo1, stereo2 = f1["ur"] >= 0, f2["ur"] >= 0
    pc1, pc2 = _pixel2camera(cam, f1["u"], f1["v"], 1.0), _pixel2camera(cam, f2["u"], f2["v"], 1.0)
    T1, T2 = G["T1"], G["T2"]
    r1 = [T1[i] * pc1[0] + T1[3 + i] * pc1[1] + T1[6 + i] * pc1[2] for i in range(3)]
    r2 = [T2[i] * pc2[0] + T2[3 + i] * pc2[1] + T2[6 + i] * pc2[2] for i in range(3)]
    dot = r1[0] * r2[0] + r1[1] * r2[1] + r1[2] * r2[2]
    n1 = math.sqrt(r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2])
    n2 = math.sqrt(r2[0] * r2[0] + r2[1] * r2[1] + r2[2] * r2[2])
    cos_ray = f32(dot / (n1 * n2))
    cd1 = cd2 = f32(2.0)
    if stereo1:
        cd1 = f32(math.cos(float(f32(2 * math.atan2(0.5 * b, float(f32(f1["depth"])))))))
    elif stereo2:   # the `else if` of :222: cosParallaxDepth2 only when !stereo1
        cd2 = f32(math.cos(float(f32(2 * math.atan2(0.5 * b, float(f32(f2["depth"])))))))
    cd = min(cd1, cd2)
    decisive = _far(cos_ray, 0.0) and _far(cos_ray, cd) and (stereo1 or stereo2 or _far(cos_ray, 0.9998)) and \
        ((cd1 == 2.0 and cd2 == 2.0) or _far(cd1, cd2))
    out = dict(cos_ray=cos_ray, cd1=cd1, cd2=cd2, accepted=False, p=None, dist1=None)
    if cos_ray > 0 and cos_ray < cd and (stereo1 or stereo2 or float(cos_ray) < 0.9998):
        p = triangulate_svd(pc1, pc2, T1, T2)
        if p is None:
            return dict(out, kind="degenerate", decisive=decisive)
        kind = "svd"
    elif stereo1 and cd1 < cd2:
        p, kind = _back_project(cam, f1["u"], f1["v"], f1["depth"], T1, G["Ow1"]), "depth1"
    elif stereo2 and cd2 < cd1:
        p, kind = _back_project(cam, f2["u"], f2["v"], f2["depth"], T2, G["Ow2"]), "depth2"
    else:
        return dict(out, kind="none", decisive=decisive)
    accepted, sig, dist1 = gates(G, cam, sf, f1, f2, p)
    h = [TAU * math.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])] * 3   # tau |p|, the point's magnitude, on every axis
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                corner = [p[0] + sx * h[0], p[1] + sy * h[1], p[2] + sz * h[2]]
                decisive = decisive and gates(G, cam, sf, f1, f2, corner)[1] == sig
    return dict(out, kind=kind, accepted=accepted, p=p, dist1=dist1, decisive=decisive, signature=sig)


def median_descriptor(descs):
    """MapPoint::computeDescriptor's selection (mappoint.cpp:145-173) restated literally -> index into descs"""
    n = len(descs)
    dist = [[hamming(descs[i], descs[j]) for j in range(n)] for i in range(n)]
    best_mid, best = 256, 0
    for i in range(n):
        mid = sorted(dist[i])[int(0.5 * (n - 1))]
        if mid < best_mid:
            best_mid, best = mid, i
    return best


# ---- the store ----------------------------------------------------------------------------------------------------------------
class NewPointsModel(CullModel):
    def __init__(self, cam6=None, scale_factors=None, first_point_id=0):
        super().__init__()
        self.cam = None if cam6 is None else [f32(c) for c in cam6]
        self.sf = None if scale_factors is None else [f32(s) for s in scale_factors]
        self.next_id = int(first_point_id)
        self.np_result = dict(neighbors=[], created=[])
        self.evals = []   # (current, neighbour, idx1, idx2, evaluate()'s dict) of every match of every create call
        self.searches = []   # (current, neighbour, a_has, b_has, F, ex, ey, match12, match_cnt, claims) of every search
        self.sticky = 0

    def insert(self, ids, flags, bad=False, desc=None, angle=None, nodes=None):
        k = super().insert(ids, flags, bad)
        n = len(ids)
        kf = self.store[k]
        kf["desc"] = np.zeros((n, 32), np.uint8) if desc is None else np.array(desc, np.uint8).reshape(n, 32)
        kf["angle"] = np.zeros(n, f32) if angle is None else np.array(angle, f32)
        kf["nodes"] = [0] * n if nodes is None else [int(x) for x in nodes]
        kf["xy"], kf["pose"] = np.zeros((n, 2), f32), None
        kf["points"], kf["pdesc"] = np.zeros((n, 3)), np.zeros((n, 32), np.uint8)
        kf["mind"], kf["maxd"], kf["normals"] = np.full(n, 0.5, f32), np.full(n, 9.0, f32), np.zeros((n, 3))
        return k

    def set_pose(self, k, T12):
        self.store[k]["pose"] = [float(x) for x in np.asarray(T12, np.float64).reshape(12)]

    def set_xy(self, k, xy):
        self.store[k]["xy"] = np.array(xy, f32).reshape(-1, 2)

    def _view(self, k):
        kf = self.store[k]
        return dict(x=kf["xy"][:, 0], y=kf["xy"][:, 1], u_right=np.array(kf["u_right"], f32), octave=kf["octave"], angle=kf["angle"],
                    desc=kf["desc"], nodes=kf["nodes"])

    def _feature(self, k, i):
        kf = self.store[k]
        return dict(u=kf["xy"][i, 0], v=kf["xy"][i, 1], ur=kf["u_right"][i], depth=kf["depth"][i], octave=kf["octave"][i])

    def create(self, current, max_neighbors=10):
        res = dict(neighbors=[], created=[])
        self.np_result = res
        cur = self.store[current]
        if self.erased[current] or cur["pose"] is None:
            self.sticky |= 1
            return res
        nbs = list(self.conn.ordered[current][:10])   # the graph row: getBestCovisibleKFs(10), copied at :136
        for i, k in enumerate(nbs):
            if i >= max_neighbors:
                res["neighbors"].append((k, NOT_REACHED, 0, 0))
                continue
            kf = self.store[k]
            if kf["bad"]:
                res["neighbors"].append((k, SKIPPED_BAD, 0, 0))
                continue
            if kf["pose"] is None:
                self.sticky |= 1
                res["neighbors"].append((k, SKIPPED_NO_POSE, 0, 0))
                continue
            G = geometry(cur["pose"], kf["pose"], self.cam)
            if G["bl"] < self.cam[5]:
                res["neighbors"].append((k, SKIPPED_BASELINE, 0, 0))
                continue
            a_has, b_has = [f & 1 for f in cur["flags"]], [f & 1 for f in kf["flags"]]
            match12, cnt, claims = search(self._view(current), self._view(k), a_has, b_has, G["F"], G["ex"], G["ey"], self.sf)
            self.searches.append((current, k, a_has, b_has, G["F"], G["ex"], G["ey"], match12, cnt, claims))
            made = 0
            for i1, i2 in enumerate(match12):
                if i2 < 0:
                    continue
                f1, f2 = self._feature(current, i1), self._feature(k, i2)
                e = evaluate(G, self.cam, self.sf, f1, f2)
                self.evals.append((current, k, i1, i2, e))
                if not e["accepted"]:
                    continue
                self._commit(current, k, i1, i2, e, G)
                res["created"].append((k, i1, i2, self.next_id))
                self.next_id += 1
                made += 1
            res["neighbors"].append((k, SEARCHED, cnt, made))
        return res

    def _commit(self, current, k, i1, i2, e, G):
        cur, kf = self.store[current], self.store[k]
        p = e["p"]
        lo, ilo = (cur, i1) if current < k else (kf, i2)   # computeDescriptor with two holders: the lower-numbered one's
        pdesc = lo["desc"][ilo].copy()
        maxd = e["dist1"] * f32(self.sf[cur["octave"][i1]])
        mind = maxd / f32(self.sf[len(self.sf) - 1])
        units = []
        for Ow in ((G["Ow1"], G["Ow2"]) if current < k else (G["Ow2"], G["Ow1"])):
            d = [p[i] - Ow[i] for i in range(3)]
            ln = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            units.append([d[i] / ln for i in range(3)])
        normal = [(units[0][i] + units[1][i]) / 2 for i in range(3)]
        for s, i in ((cur, i1), (kf, i2)):
            s["flags"][i], s["ids"][i] = 3, self.next_id
            s["points"][i], s["pdesc"][i], s["mind"][i], s["maxd"][i], s["normals"][i] = p, pdesc, mind, maxd, normal

    def points(self, k):
        kf = self.store[k]
        return dict(flags=np.array(kf["flags"], np.uint8), ids=np.array(kf["ids"], np.int32), points=kf["points"], point_desc=kf["pdesc"],
                    min_dist=kf["mind"], max_dist=kf["maxd"], normals=kf["normals"])
