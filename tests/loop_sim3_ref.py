"""Model of vo_kfstore_compute_sim3 (test infrastructure): LoopClosing::computeSim3 (src/loopClosing.cpp:178-348) restated as
plain Python / numpy bookkeeping around the oracle's functions -- orc_match_bow, orc_sim3_ransac_eval (one hypothesis per call,
the order of the shim), orc_match_sim3_mutual, orc_sim3_solve, orc_match_sim3_projection -- over the list-of-dicts store of
tests/loop_sim3_inputs.py.  It never imports the device library; the oracle binding is handed over by the caller.

The model keeps a LOG of what happened -- ("front", position, reason, matches), ("construct", position, N, max_iters),
("trip", position, iterations_global, count, best), ("stop", position), ("return", position, count), ("verify", position,
searched, n, inliers, phase), ("resume",), ("match", position), ("end",), ("rand_short",), ("loop_points", n), ("capacity",),
("projection", claims, match_cnt), ("undecided",) -- from which tests/test_loop_sim3_ref.py proves that a scenario reaches its
branch, and the smallest MARGIN with which each kind of float gate decided (self.margin[kind])."""
import ctypes as C
import math

import numpy as np

import connections_ref

f32 = np.float32
UNDECIDED, NO_MATCH, REJECTED, ACCEPTED = 0, 1, 2, 3
LIVE, BAD, FEW_MATCHES, STOPPED = 0, 1, 2, 3
STICKY_INVALID, STICKY_RAND_SHORT, STICKY_CAPACITY = 1, 32, 64
MAX_CANDIDATES = 16
MIN_INLIERS, MAX_ITERATIONS, TRIPS = 20, 300, 5
RECORD = ("state", "match_pos", "match_kf", "rounds", "verifications", "rand_used", "refine_inliers", "match_cnt", "n_loop_points")
PER_CANDIDATE = ("kf", "reason", "bow_matches", "n", "max_iters", "iterations", "inliers_best", "verifications")
# the floors tests/test_loop_sim3_ref.py holds the inputs to (a pose off by 1e-8 moves a pixel by about 1e-5 at these focal
# lengths: 2 |e| 1e-5 <~ 2e-4 px^2 for |e| <~ 7 px)
FLOORS = dict(ransac=1e-3, chi2=1e-3, z=1e-3, in_img=1e-3, distance=1e-4, cosine=1e-4, level=1e-3, radius=1e-3, cell=1e-4)


def ransac_max_iters(N):
    """Sim3Solver::setRansacParameters(0.99, 20, 300) (sim3Solver.cpp:76-96) for N >= 20"""
    if N == MIN_INLIERS:
        return 1
    eps = float(f32(MIN_INLIERS) / f32(N))
    return max(1, min(int(math.ceil(math.log(1 - 0.99) / math.log(1 - eps ** 3))), MAX_ITERATIONS))


def se3_point(T, p):
    """Tcw * p in the operation order the device fixes: ((r0 p0 + r1 p1) + r2 p2) + t"""
    return np.array([((T[3 * r] * p[0] + T[3 * r + 1] * p[1]) + T[3 * r + 2] * p[2]) + T[9 + r] for r in range(3)])


def sim3_point(S, p):
    R, t, s = S
    return np.array([s * ((R[r, 0] * p[0] + R[r, 1] * p[1]) + R[r, 2] * p[2]) + t[r] for r in range(3)])


def sim3_inverse(S):
    R, t, s = S
    return R.T.copy(), -(1.0 / s) * (R.T @ t), 1.0 / s


def sim13(S):
    return np.concatenate([np.asarray(S[0]).reshape(-1), np.asarray(S[1]).reshape(-1), [S[2]]])


def observation(kf, f):
    """the key-frame's lowest-numbered feature that carries the id of its feature f with bit 0; -1 without one"""
    if not (kf["flags"][f] & 1) or kf["ids"][f] < 0:
        return -1
    for j in range(len(kf["ids"])):
        if kf["ids"][j] == kf["ids"][f] and (kf["flags"][j] & 1):
            return j
    return -1


class LoopModel:
    def __init__(self, orc, store, cam6, sf, bounds, max_candidates, max_loop_points, max_rand):
        self.orc, self.store, self.cam, self.sf, self.bounds = orc, store, [f32(c) for c in cam6], np.asarray(sf, f32), bounds
        self.caps = (max_candidates, max_loop_points, max_rand)
        self.sticky = 0
        self.conn = connections_ref.Connections()
        self.log, self.margin = [], {}
        self.frames, self.bows = {}, {}
        self.reset()

    # ---- plumbing
    def reset(self):
        self.rec = dict.fromkeys(RECORD, 0)
        self.rec.update(match_pos=-1, match_kf=-1)
        self.per = [dict.fromkeys(PER_CANDIDATE, 0) for _ in range(self.caps[0])]
        self.Scm, self.Scw = np.zeros(13), np.zeros(13)
        self.match_ids, self.loop_ids = None, []
        self.phase = "halt"

    def update_connections(self, keyframes):
        live = [dict(ids=k["ids"], flags=[0 if k.get("erased") else fl for fl in k["flags"]]) for k in self.store]
        self.conn.update_list(live, keyframes)

    def _note(self, kind, value):
        self.margin[kind] = min(self.margin.get(kind, np.inf), float(value))

    def frame(self, k):
        if k not in self.frames:
            kf = self.store[k]
            w, h = self.bounds[1] - self.bounds[0], self.bounds[3] - self.bounds[2]
            self.frames[k] = self.orc.FrameData(kf["x"], kf["y"], kf["octave"], kf["angle"], kf["uright"], kf["desc"], w, h)
            self.bows[k] = self.orc.BowData(kf["nodes"])
        return self.frames[k], self.bows[k]

    def usable(self, k):
        return 0 <= k < len(self.store) and not self.store[k].get("erased")

    def result(self):
        out = dict(self.rec)
        n_cur = len(self.store[self.current]["ids"]) if self.usable(self.current) and self.phase != "invalid" else 0
        mids = self.match_ids if self.match_ids is not None else np.full(n_cur, -1, np.int32)
        lids = self.loop_ids if self.rec["state"] >= REJECTED else []
        out.update(per_candidate=[dict(p) for p in self.per], Scm=self.Scm.copy(), Scw=self.Scw.copy(),
                   match_ids=np.asarray(mids, np.int32), loop_point_ids=np.asarray(lids, np.int32))
        return out

    # ---- the call
    def compute_sim3(self, current, cand, fix_scale, rand_values, rand_max, max_rounds):
        self.reset()
        self.current, self.cand, self.fix_scale = current, list(cand), bool(fix_scale)
        self.rand, self.rand_max = [int(r) for r in rand_values], int(rand_max)
        cur = self.store[current] if self.usable(current) else None
        if cur is None or cur["pose"] is None:
            self.sticky |= STICKY_INVALID
            self.phase = "invalid"
            for i, k in enumerate(cand):
                self.per[i]["kf"] = k
            self.log.append(("invalid",))
            return
        self.solvers = [None] * len(cand)
        for i, k in enumerate(cand):
            self._front(i, k)
        self.live = sum(1 for i in range(len(cand)) if self.per[i]["reason"] == LIVE)
        self.cursor, self.phase = 0, "walk"
        self.continue_(max_rounds)

    def continue_(self, max_rounds):
        for _ in range(max_rounds):
            if self.phase != "walk":
                break
            self._round()
        if self.phase == "after":
            self._after_match()
        if self.phase == "walk":
            self.log.append(("undecided",))

    # ---- 1. the front and 2. Sim3Solver's constructor
    def _front(self, i, k):
        per, cur = self.per[i], self.store[self.current]
        per["kf"] = k
        if not self.usable(k) or self.store[k]["bad"]:
            per["reason"] = BAD
            self.log.append(("front", i, BAD, 0))
            return
        kf = self.store[k]
        fa, ba = self.frame(self.current)
        fb, bb = self.frame(k)
        va = np.ascontiguousarray([fl & 1 for fl in cur["flags"]], np.uint8)
        vb = np.ascontiguousarray([fl & 1 for fl in kf["flags"]], np.uint8)
        match = np.full(max(len(va), 1), -1, np.int32)
        nm = self.orc.lib().orc_match_bow(C.byref(fa.c), va, C.byref(ba.c), C.byref(fb.c), vb, C.byref(bb.c), 1, f32(0.75), 1, match)
        per["bow_matches"] = int(nm)
        if nm < MIN_INLIERS:
            per["reason"] = FEW_MATCHES
            self.log.append(("front", i, FEW_MATCHES, int(nm)))
            return
        self.log.append(("front", i, LIVE, int(nm)))
        fx, fy, cx, cy = (float(c) for c in self.cam[:4])
        rows = []
        for f in range(len(cur["ids"])):
            f2 = int(match[f])
            if f2 < 0 or kf["pose"] is None:
                continue
            idx1, idx2 = observation(cur, f), observation(kf, f2)
            if idx1 < 0 or idx2 < 0:
                continue
            a, b = se3_point(cur["pose"], cur["points"][f]), se3_point(kf["pose"], kf["points"][f2])
            s1, s2 = float(self.sf[cur["octave"][idx1]]), float(self.sf[kf["octave"][idx2]])
            rows.append((f, a, b, (fx * a[0] / a[2] + cx, fy * a[1] / a[2] + cy), (fx * b[0] / b[2] + cx, fy * b[1] / b[2] + cy),
                         int(9.210 * s1 * s1), int(9.210 * s2 * s2)))
        N = len(rows)
        sol = dict(match=match, index=np.array([r[0] for r in rows], np.int32), pc1=np.array([r[1] for r in rows]).reshape(N, 3),
                   pc2=np.array([r[2] for r in rows]).reshape(N, 3), px1=np.array([r[3] for r in rows]).reshape(N, 2),
                   px2=np.array([r[4] for r in rows]).reshape(N, 2), me1=np.array([r[5] for r in rows], np.int32),
                   me2=np.array([r[6] for r in rows], np.int32))
        self.solvers[i] = sol
        per["n"] = N
        per["max_iters"] = ransac_max_iters(N) if N >= MIN_INLIERS else 1
        self.log.append(("construct", i, N, per["max_iters"]))

    # ---- 3. one round of the walk
    def _draw(self, N):
        """three draws of randomInt over the shrinking index list (sim3Solver.cpp:125-141), or None when the values run out"""
        used = self.rec["rand_used"]
        if used + 3 > len(self.rand):
            return None
        avail, out = list(range(N)), []
        for k in range(3):
            ri = int((float(self.rand[used + k]) / (float(self.rand_max) + 1.0)) * len(avail))
            out.append(avail[ri])
            avail[ri] = avail[-1]
            avail.pop()
        self.rec["rand_used"] = used + 3
        return out

    def _hypothesis(self, sol, triplet):
        N = len(sol["index"])
        cnt, flags, sims = np.zeros(1, np.int32), np.zeros(N, np.uint8), np.zeros(13)
        cam = np.array([float(c) for c in self.cam[:4]], f32)
        self.orc.lib().orc_sim3_ransac_eval(N, np.ascontiguousarray(sol["pc1"]), np.ascontiguousarray(sol["pc2"]),
                                            np.ascontiguousarray(sol["px1"]), np.ascontiguousarray(sol["px2"]), sol["me1"], sol["me2"], cam, 1,
                                            np.ascontiguousarray(triplet, np.int32), int(self.fix_scale), cnt, flags, sims)
        # the margin of checkInliers: both squared errors against their thresholds, restated in float64
        R, t, s = sims[:9].reshape(3, 3), sims[9:12], sims[12]
        camd = cam.astype(np.float64)
        px = lambda p: np.stack([camd[0] * p[:, 0] / p[:, 2] + camd[2], camd[1] * p[:, 1] / p[:, 2] + camd[3]], 1)
        e1 = ((px(s * sol["pc2"] @ R.T + t) - sol["px1"]) ** 2).sum(1)
        e2 = ((px(((sol["pc1"] - t) @ R) / s) - sol["px2"]) ** 2).sum(1)
        self._note("ransac", min(np.abs(e1 - sol["me1"]).min(), np.abs(e2 - sol["me2"]).min()))
        return int(cnt[0]), flags, sims

    def _round(self):
        self.rec["rounds"] += 1
        n_cand = len(self.cand)
        while True:
            if self.live <= 0:
                self.rec["state"], self.phase = NO_MATCH, "done"
                self.log.append(("end",))
                return
            i = self.cursor
            while True:
                if i >= n_cand:
                    i = 0
                if self.per[i]["reason"] == LIVE:
                    break
                i += 1
            per, sol = self.per[i], self.solvers[i]
            if per["n"] < MIN_INLIERS or per["iterations"] >= per["max_iters"]:
                per["reason"] = STOPPED
                self.live -= 1
                self.cursor = i + 1
                self.log.append(("stop", i))
                continue
            ret = None
            for _ in range(TRIPS):
                if per["iterations"] >= per["max_iters"]:
                    break
                tri = self._draw(per["n"])
                if tri is None:
                    self.sticky |= STICKY_RAND_SHORT
                    self.phase = "halt"
                    self.log.append(("rand_short",))
                    return
                per["iterations"] += 1
                cnt, flags, sims = self._hypothesis(sol, tri)
                self.log.append(("trip", i, per["iterations"], cnt, per["inliers_best"]))
                if cnt >= per["inliers_best"]:
                    per["inliers_best"] = cnt
                    if cnt > MIN_INLIERS:
                        ret = (flags, sims)
                        break
            self.cursor = i + 1
            if ret is None:
                if per["iterations"] >= per["max_iters"]:
                    per["reason"] = STOPPED
                    self.live -= 1
                    self.log.append(("stop", i))
                continue
            self.log.append(("return", i, int(ret[0].sum())))
            self._verify(i, *ret)
            return

    # ---- the verification of a non-empty return (:259-286)
    def _project(self, src, f, T_src, S, strict_zero, dst_kind):
        """the gates of searchBySim3 for the map point at feature f of `src` -> (u, v, level) in float32, or None"""
        fx, fy, cx, cy = self.cam[:4]
        pb = sim3_point(S, se3_point(T_src, src["points"][f]))
        z = f32(pb[2])
        self._note("z", abs(float(pb[2])))
        if (z <= 0) if strict_zero else (z < 0):
            return None
        invz = f32(1.0) / z
        u, v = fx * (f32(pb[0]) * invz) + cx, fy * (f32(pb[1]) * invz) + cy
        return self._gates(u, v, f32(math.sqrt((pb[0] * pb[0] + pb[1] * pb[1]) + pb[2] * pb[2])), src["min_dist"][f], src["max_dist"][f])

    def _gates(self, u, v, dist, mind, maxd, th=7.5):
        b = self.bounds
        self._note("in_img", min(abs(float(u) - b[0]), abs(float(u) - b[1]), abs(float(v) - b[2]), abs(float(v) - b[3])))
        if not (u >= b[0] and v >= b[2] and u < b[1] and v < b[3]):
            return None
        lo, hi = f32(0.8) * f32(mind), f32(1.2) * f32(maxd)
        self._note("distance", min(abs(float(dist) - float(lo)), abs(float(dist) - float(hi))) / float(dist))
        if dist < lo or dist > hi:
            return None
        return u, v, dist

    def _level(self, maxd, dist):
        x = f32(math.log(float(f32(maxd) / dist))) / f32(math.log(float(self.sf[1])))
        if -0.5 < float(x) < len(self.sf) - 1.5:
            self._note("level", abs(float(x) - round(float(x))))
        return int(min(max(math.ceil(float(x)), 0), len(self.sf) - 1))

    def _window_margin(self, kf, u, v, radius):
        gw, gh = f32(64.0) / f32(self.bounds[1] - self.bounds[0]), f32(48.0) / f32(self.bounds[3] - self.bounds[2])
        for a in ((u - f32(self.bounds[0]) - radius) * gw, (u - f32(self.bounds[0]) + radius) * gw, (v - f32(self.bounds[2]) - radius) * gh,
                  (v - f32(self.bounds[2]) + radius) * gh):
            self._note("cell", abs(float(a) - round(float(a))) if abs(float(a) - round(float(a))) < 0.5 else 0.5)
        dx, dy = np.abs(kf["x"] - u), np.abs(kf["y"] - v)
        near = (dx < radius + 1) & (dy < radius + 1)
        if near.any():
            self._note("radius", min(np.abs(dx[near] - radius).min(), np.abs(dy[near] - radius).min()))

    def _verify(self, i, flags, sims):
        cur, kf = self.store[self.current], self.store[self.cand[i]]
        sol, sf = self.solvers[i], self.sf
        n1, n2 = len(cur["ids"]), len(kf["ids"])
        inl = np.full(n1, -1, np.int32)
        for k in np.nonzero(flags)[0]:
            inl[sol["index"][k]] = sol["match"][sol["index"][k]]
        S12 = (sims[:9].reshape(3, 3).copy(), sims[9:12].copy(), float(sims[12]))
        S21 = sim3_inverse(S12)
        matched2 = np.zeros(n2, bool)
        for f in range(n1):
            if inl[f] >= 0:
                o2 = observation(kf, int(inl[f]))
                if o2 >= 0:
                    matched2[o2] = True

        def queries(src, n, skip, T, S, strict, dst):
            ok, qu, qv, ql = np.zeros(n, np.uint8), np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, np.int32)
            for f in range(n):
                if not (src["flags"][f] & 1) or skip(f):
                    continue
                g = self._project(src, f, T, S, strict, dst)
                if g is None:
                    continue
                u, v, dist = g
                ql[f] = self._level(src["max_dist"][f], dist)
                ok[f], qu[f], qv[f] = 1, u, v
                self._window_margin(dst, u, v, f32(7.5) * sf[ql[f]])
            return ok, qu, qv, ql

        q1 = queries(cur, n1, lambda f: inl[f] >= 0, cur["pose"], S21, False, kf)
        q2 = queries(kf, n2, lambda f: matched2[f], kf["pose"], S12, True, cur)
        fa, _ = self.frame(self.current)
        fb, _ = self.frame(self.cand[i])
        m12 = np.full(max(n1, 1), -1, np.int32)
        self.orc.lib().orc_match_sim3_mutual(C.byref(fa.c), C.byref(fb.c), q1[0], q1[1], q1[2], q1[3],
                                             np.ascontiguousarray(cur["point_desc"], np.uint8), q2[0], q2[1], q2[2], q2[3],
                                             np.ascontiguousarray(kf["point_desc"], np.uint8), f32(7.5), sf, sf, m12)
        searched = int((m12[:n1] >= 0).sum())
        for f in range(n1):
            if m12[f] >= 0:
                inl[f] = m12[f]
        # solveLoopSim3 (optimizer_ceres.cpp:810-1030)
        rows = []
        for f in range(n1):
            f2 = int(inl[f])
            if f2 < 0 or not (cur["flags"][f] & 1):
                continue
            im = observation(kf, f2)
            if im < 0:
                continue
            rows.append((f, se3_point(kf["pose"], kf["points"][f2]), (float(cur["x"][f]), float(cur["y"][f])), 1.0 / float(sf[cur["octave"][f]]),
                         se3_point(cur["pose"], cur["points"][f]), (float(kf["x"][im]), float(kf["y"][im])), 1.0 / float(sf[kf["octave"][im]])))
        n = len(rows)
        col = lambda j, w: np.ascontiguousarray(np.array([r[j] for r in rows], np.float64).reshape(n, w) if w > 1 else
                                                np.array([r[j] for r in rows], np.float64))
        from scipy.spatial.transform import Rotation
        pose = np.concatenate([Rotation.from_matrix(S12[0]).as_rotvec(), S12[1]])
        scale = np.array([S12[2]])
        outl = np.zeros(max(n, 1), np.uint8)
        sums = (self.orc.LmSummary * 2)()
        cam4 = np.array([float(c) for c in self.cam[:4]])
        inliers = self.orc.lib().orc_sim3_solve(n, col(1, 3), col(2, 2), col(3, 1), col(4, 3), col(5, 2), col(6, 1), cam4, int(self.fix_scale), pose,
                                                scale, outl, C.cast(sums, C.c_void_p))
        phase = 2 if sums[1].max_iterations > 0 else 1
        for k in range(n):
            if outl[k]:
                inl[rows[k][0]] = -1
        Scm = S12
        if phase == 2:
            Scm = (Rotation.from_rotvec(pose[:3]).as_matrix(), pose[3:].copy(), float(scale[0]))
        if n > 0:
            self._chi2_margin(Scm if phase == 2 else (Rotation.from_rotvec(pose[:3]).as_matrix(), pose[3:], float(scale[0])), rows, cam4)
        self.Scm = sim13(Scm)
        self.rec["verifications"] += 1
        self.per[i]["verifications"] += 1
        self.rec["refine_inliers"] = int(inliers)
        self.log.append(("verify", i, searched, n, int(inliers), phase))
        if inliers >= 20:
            T = np.asarray(kf["pose"])
            Rm, tm = T[:9].reshape(3, 3), T[9:]
            self.Scw = sim13((Scm[0] @ Rm, Scm[2] * (Scm[0] @ tm) + Scm[1], Scm[2]))
            self.rec.update(match_pos=i, match_kf=self.cand[i])
            self.inl, self.phase = inl, "after"
            self.log.append(("match", i))
        elif self.live <= 0:
            self.rec["state"], self.phase = NO_MATCH, "done"
            self.log.append(("end",))
        else:
            self.log.append(("resume",))

    def _chi2_margin(self, S, rows, cam):
        R, t, s = S
        for _, Pm, pc, isc, Pc, pm, ism in rows:
            p = s * (R @ Pm) + t
            q = (R.T @ (Pc - t)) / s
            e1 = ((cam[0] * p[0] / p[2] + cam[2] - pc[0]) ** 2 + (cam[1] * p[1] / p[2] + cam[3] - pc[1]) ** 2) * isc * isc
            e2 = ((cam[0] * q[0] / q[2] + cam[2] - pm[0]) ** 2 + (cam[1] * q[1] / q[2] + cam[3] - pm[1]) ** 2) * ism * ism
            self._note("chi2", min(abs(e1 - 10.0), abs(e2 - 10.0)))

    # ---- 5. after a match (:298-347)
    def _after_match(self):
        cur, mk = self.store[self.current], self.rec["match_kf"]
        kfc = self.store[mk]
        n1 = len(cur["ids"])
        self.match_ids = np.array([kfc["ids"][self.inl[f]] if self.inl[f] >= 0 else -1 for f in range(n1)], np.int32)
        self.conn.grow(len(self.store))
        seen, pts = set(), []
        for k in list(self.conn.ordered[mk]) + [mk]:
            kf = self.store[k]
            for f in range(len(kf["ids"])):
                if (kf["flags"][f] & 1) and kf["ids"][f] >= 0 and not kf.get("erased") and kf["ids"][f] not in seen:
                    seen.add(kf["ids"][f])
                    pts.append((k, f))
        self.loop_ids = [self.store[k]["ids"][f] for k, f in pts]
        self.rec["n_loop_points"] = len(pts)
        self.log.append(("loop_points", len(pts)))
        if len(pts) > self.caps[1]:
            self.sticky |= STICKY_CAPACITY
            self.phase = "halt"
            self.log.append(("capacity",))
            return
        # searchByProjection (matcher.cpp:356-447)
        R, t, s = self.Scw[:9].reshape(3, 3), self.Scw[9:12], self.Scw[12]
        T = np.concatenate([(R / s).reshape(-1), t / s])
        Ow = np.array([-((T[i] * T[9] + T[3 + i] * T[10]) + T[6 + i] * T[11]) for i in range(3)])
        found = set(int(x) for x in self.match_ids if x >= 0)
        nq = len(pts)
        ok, qu, qv, ql = np.zeros(max(nq, 1), np.uint8), np.zeros(max(nq, 1), f32), np.zeros(max(nq, 1), f32), np.zeros(max(nq, 1), np.int32)
        qd = np.zeros((max(nq, 1), 32), np.uint8)
        fx, fy, cx, cy = self.cam[:4]
        for q, (k, f) in enumerate(pts):
            kf = self.store[k]
            qd[q] = kf["point_desc"][f]
            if kf["ids"][f] in found:
                continue
            pw = kf["points"][f]
            pc = se3_point(T, pw)
            z = f32(pc[2])
            self._note("z", abs(float(pc[2])))
            if z < 0:
                continue
            invz = f32(1.0) / z
            u, v = fx * (f32(pc[0]) * invz) + cx, fy * (f32(pc[1]) * invz) + cy
            line = pw - Ow
            g = self._gates(u, v, f32(math.sqrt((line[0] * line[0] + line[1] * line[1]) + line[2] * line[2])), kf["min_dist"][f], kf["max_dist"][f])
            if g is None:
                continue
            dist, nrm = g[2], kf["normals"][f]
            dot = (line[0] * nrm[0] + line[1] * nrm[1]) + line[2] * nrm[2]
            self._note("cosine", abs(dot - 0.5 * float(dist)))
            if dot < 0.5 * float(dist):
                continue
            ql[q] = self._level(kf["max_dist"][f], dist)
            ok[q], qu[q], qv[q] = 1, u, v
            self._window_margin(cur, u, v, f32(10.0) * self.sf[ql[q]])
        fa, _ = self.frame(self.current)
        occ = np.ascontiguousarray((self.match_ids >= 0).astype(np.uint8)) if n1 else np.zeros(1, np.uint8)
        assigned = np.full(max(n1, 1), -1, np.int32)
        claims = self.orc.lib().orc_match_sim3_projection(C.byref(fa.c), nq, ok, qu, qv, ql, np.ascontiguousarray(qd), 10, self.sf, occ, assigned)
        for f in range(n1):
            if assigned[f] >= 0:
                self.match_ids[f] = self.loop_ids[assigned[f]]
        cnt = int((self.match_ids >= 0).sum())
        self.rec["match_cnt"] = cnt
        self.rec["state"], self.phase = (ACCEPTED if cnt >= 40 else REJECTED), "done"
        self.log.append(("projection", int(claims), cnt))
