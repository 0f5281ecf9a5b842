"""Model of the store's map-point fusion (test infrastructure): LocalMapping::searchInNeighbors (src/localMapping.cpp:363-432),
Matcher::fuseMapPoints (src/matcher.cpp:1012-1133) and MapPoint::replaceMapPoint (src/mappoint.cpp:214-253) restated on the
store, strictly sequential, in numpy on top of tests/point_upkeep_ref.py's UpkeepModel (the store, the connections, the
refresh, computeDescriptor, the recent list).

The definitions are tests/cull_ref.py's: j HOLDS p, j's OBSERVATION of p, obs(p), bad(j).  A map point "isBad" when nobody
holds it, its attributes (position, normal, min / max distance, ref_kf, point_desc) are the ones of its first live carrier.
np.float32 scalars are the reference's float, Python floats its double, every operation rounded on its own.  project() and
search() also return the margin of every float gate they decide, for the conditions of tests/test_fuse_ref.py."""
import math

import numpy as np

from new_points_ref import TH_LOW, _center, _dot3, hamming
from point_upkeep_ref import UpkeepModel

f32 = np.float32
STICKY_INVALID, STICKY_FUSE = 1, 16
GRID_COLS, GRID_ROWS = 64, 48
MAX_TARGETS = 60
CARRIERS_MAX = 1024
STEP = ("passed", "matches", "adds", "kept_org", "kept_candidate", "cleared")
CHI2_STEREO, CHI2_MONO = f32(7.815), f32(5.991)
MARGIN, LEVEL_MARGIN = 1e-4, 1e-3   # what tests/test_fuse_ref.py asks of every scene


def _rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(a), abs(b), 1e-30)


def _round_half_away(x):
    """C's round() on a float"""
    x = float(x)
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


class FuseModel(UpkeepModel):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.bounds = None
        self.fuse_targets, self.fuse_steps = [], []
        self.fuse_log = []      # (target, candidate, feature, kind, org) of every match, for the tests' non-vacuity conditions
        self.fuse_log_call, self.n_fuse = [], 0     # the number of the fuse call of every fuse_log entry
        self.margins = []       # (gate, relative margin) of every float gate decided
        self.level_fracs = []   # distance of log(ratio) / log(sf[1]) from an integer
        self.queries = []       # (target, dict) of every candidate that passed the gates
        self.margin, self.level_margin = MARGIN, LEVEL_MARGIN    # (a scene search may ask for more)
        self.undone = []        # (target, limit) of every step a capacity left undone
        self.weak = set()       # the candidates one of whose gates decided with less than MARGIN / LEVEL_MARGIN

    def enable_fuse(self, bounds, max_candidates):
        self.bounds = [f32(b) for b in bounds]
        self.max_candidates = int(max_candidates)
        self.gpw = f32(GRID_COLS) / f32(self.bounds[1] - self.bounds[0])
        self.gph = f32(GRID_ROWS) / f32(self.bounds[3] - self.bounds[2])

    # ---- a map point's attributes --------------------------------------------------------------------------------------
    def attributes(self, p):
        j, i = self.carriers(p)[0]
        kf = self.store[j]
        return dict(point=np.array(kf["points"][i], np.float64), normal=np.array(kf["normals"][i], np.float64), mind=f32(kf["mind"][i]),
                    maxd=f32(kf["maxd"][i]), ref=int(kf["ref"][i]), pdesc=np.array(kf["pdesc"][i], np.uint8))

    def _take(self, j, i, p, a):
        kf = self.store[j]
        kf["ids"][i] = int(p)
        kf["points"][i], kf["normals"][i], kf["mind"][i], kf["maxd"][i] = a["point"], a["normal"], a["mind"], a["maxd"]
        kf["ref"][i], kf["pdesc"][i] = a["ref"], a["pdesc"]

    # ---- the gates of a candidate (:1029-1062) -------------------------------------------------------------------------
    def project(self, T, p, threshold, attrs=None):
        """-> the query of candidate p in key-frame T, or None (attrs: the attributes of a caller that keeps its own map points
        and has checked isBad / beObserved itself)"""
        if attrs is None and (not self.observations(p) or self.observation(T, p) >= 0):
            return None
        a, pose = attrs or self.attributes(p), self.store[T]["pose"]
        fx, fy, cx, cy, bf = self.cam[:5]
        pw = [float(x) for x in a["point"]]
        pc = [_dot3(pose[3 * r], pw[0], pose[3 * r + 1], pw[1], pose[3 * r + 2], pw[2]) + pose[9 + r] for r in range(3)]
        z = f32(pc[2])
        if z < 0:
            return None
        with np.errstate(all="ignore"):
            invz = f32(1.0) / z
            x, y = f32(pc[0]) * invz, f32(pc[1]) * invz
            u, v = fx * x + cx, fy * y + cy
        b, m, n0 = self.bounds, self.margins, len(self.margins)
        m += [("img", _rel(u, b[0])), ("img", _rel(u, b[1])), ("img", _rel(v, b[2])), ("img", _rel(v, b[3]))]
        if not (u >= b[0] and v >= b[2] and u < b[1] and v < b[3]):
            return self._weak(p, n0)
        ur = u - bf * invz
        Ow = _center(pose)
        line = [pw[c] + -Ow[c] for c in range(3)]
        dist = f32(math.sqrt(_dot3(line[0], line[0], line[1], line[1], line[2], line[2])))
        lo, hi = f32(0.8) * a["mind"], f32(1.2) * a["maxd"]
        m += [("dist", _rel(dist, lo)), ("dist", _rel(dist, hi))]
        if dist < lo or dist > hi:
            return self._weak(p, n0)
        n = [float(c) for c in a["normal"]]
        dot, half = _dot3(line[0], n[0], line[1], n[1], line[2], n[2]), 0.5 * float(dist)
        m.append(("normal", _rel(dot, half)))
        if dot < half:
            return self._weak(p, n0)
        ratio = a["maxd"] / dist
        q = f32(math.log(float(ratio))) / f32(math.log(float(self.sf[1])))
        self.level_fracs.append(abs(float(q) - round(float(q))))
        level = min(max(int(math.ceil(float(q))), 0), len(self.sf) - 1)
        if self.level_fracs[-1] < self.level_margin:
            self.weak.add(int(p))
        self._weak(p, n0)
        return dict(p=int(p), u=u, v=v, ur=ur, level=level, radius=f32(threshold) * self.sf[level], pdesc=a["pdesc"])

    def _log_match(self, entry):
        self.fuse_log.append(entry)
        self.fuse_log_call.append(self.n_fuse)

    def _weak(self, p, n0):
        if any(x < self.margin for _, x in self.margins[n0:]):
            self.weak.add(int(p))
        return None

    # ---- the window and the best match (keyframe.cpp:268-309, matcher.cpp:1068-1109) ---------------------------------------
    def cell(self, x, y):
        cx, cy = _round_half_away((x - self.bounds[0]) * self.gpw), _round_half_away((y - self.bounds[2]) * self.gph)
        return (cx, cy) if 0 <= cx < GRID_COLS and 0 <= cy < GRID_ROWS else None

    def features_in_area(self, T, q):
        """the features getFeaturesInArea returns, in its order"""
        kf, b, r, u, v = self.store[T], self.bounds, q["radius"], q["u"], q["v"]
        x0 = max(0, int(math.floor(float((u - b[0] - r) * self.gpw))))
        x1 = min(GRID_COLS - 1, int(math.floor(float((u - b[0] + r) * self.gpw))))
        y0 = max(0, int(math.floor(float((v - b[2] - r) * self.gph))))
        y1 = min(GRID_ROWS - 1, int(math.floor(float((v - b[2] + r) * self.gph))))
        if x0 >= GRID_COLS or x1 < 0 or y0 >= GRID_ROWS or y1 < 0:
            return []
        out = []
        for i in range(len(kf["ids"])):
            c = self.cell(kf["xy"][i, 0], kf["xy"][i, 1])
            if c is None or not (x0 <= c[0] <= x1 and y0 <= c[1] <= y1):
                continue
            dx, dy = abs(kf["xy"][i, 0] - u), abs(kf["xy"][i, 1] - v)
            self.margins += [("radius", _rel(dx, r)), ("radius", _rel(dy, r))]
            if dx < r and dy < r:
                out.append((c[0], c[1], i))
        return [i for _, _, i in sorted(out)]

    def search(self, T, q):
        """-> the feature of T candidate q matches, or -1"""
        kf, best, best_i, n0 = self.store[T], 256, -1, len(self.margins)
        for i in self.features_in_area(T, q):
            o = kf["octave"][i]
            if o < q["level"] - 1 or o > q["level"]:
                continue
            ex, ey = q["u"] - kf["xy"][i, 0], q["v"] - kf["xy"][i, 1]
            inv = f32(1.0) / self.sf[min(max(o, 0), 15)]
            if kf["u_right"][i] >= 0:
                er = q["ur"] - f32(kf["u_right"][i])
                chi, th = (ex * ex + ey * ey + er * er) * inv * inv, CHI2_STEREO
            else:
                chi, th = (ex * ex + ey * ey) * inv * inv, CHI2_MONO
            self.margins.append(("chi2", _rel(chi, th)))
            if chi > th:
                continue
            d = hamming(q["pdesc"], kf["desc"][i])
            if d < best:
                best, best_i = d, i
        self._weak(q["p"], n0)
        return best_i if best <= TH_LOW else -1

    # ---- MapPoint::replaceMapPoint (mappoint.cpp:214-253) ----------------------------------------------------------------
    def replace(self, A, B, step):
        if A == B:
            return
        a = self.attributes(B)
        obs_a, all_a = self.observations(A), self.carriers(A)
        for j, i in obs_a:
            if self.observation(j, B) < 0:
                self._take(j, i, B, a)
            else:
                self.store[j]["flags"][i] &= ~1
                step["cleared"] += 1
        for j, i in all_a:
            if (j, i) not in obs_a:          # a second feature of a holder: the pointer model leaves a dangling bad pointer
                self.store[j]["flags"][i] &= ~1
                step["cleared"] += 1
        if A in self.recent and B in self.recent:
            self.recent[B][1] += self.recent[A][1]
            self.recent[B][2] += self.recent[A][2]
        self.compute_descriptors([B])

    # ---- Matcher::fuseMapPoints ----------------------------------------------------------------------------------------
    def fuse(self, T, ids, threshold=3.0):
        step = {k: 0 for k in STEP}
        self.n_fuse += 1
        if self.erased[T] or self.store[T]["pose"] is None:
            self.sticky |= STICKY_INVALID
            return step
        kf = self.store[T]
        # what the step would do, counted on the state it starts from: a match reserves a node of the overlay, and a call whose
        # matches exceed max_candidates leaves the step that meets the limit, and every later one, undone
        first = list(dict.fromkeys(int(p) for p in ids if int(p) >= 0))
        dry = [self.project(T, p, threshold) for p in first]
        dry_matches = sum(1 for q in dry if q is not None and self.search(T, q) >= 0)
        dry_passed = sum(1 for q in dry if q is not None)
        self.reserved += dry_matches
        if dry_passed > self.max_candidates or self.reserved > self.max_candidates:
            self.sticky |= STICKY_FUSE
            self.undone.append((T, "candidates" if dry_passed > self.max_candidates else "matches"))
            return dict(step, passed=dry_passed, matches=dry_matches)
        for p in ids:
            p = int(p)
            if p < 0:
                continue
            q = self.project(T, p, threshold)
            if q is None:
                continue
            step["passed"] += 1
            self.queries.append((T, q))
            i = self.search(T, q)
            if i < 0:
                continue
            step["matches"] += 1
            if (kf["flags"][i] & 1) and kf["ids"][i] >= 0:
                org = kf["ids"][i]
                if max(len(self.carriers(org)), len(self.carriers(p))) > CARRIERS_MAX:
                    self.sticky |= STICKY_FUSE
                    self._log_match((T, p, i, "capacity", org))
                    continue
                if self.obs(org) > self.obs(p):
                    self.replace(p, org, step)
                    step["kept_org"] += 1
                    self._log_match((T, p, i, "kept_org", org))
                else:
                    self.replace(org, p, step)
                    step["kept_candidate"] += 1
                    self._log_match((T, p, i, "kept_candidate", org))
            else:
                self._take(T, i, p, self.attributes(p))
                kf["flags"][i] |= 1
                step["adds"] += 1
                self._log_match((T, p, i, "add", -1))
        # the two derivations of DESIGN.md section 4m: gates and matches can be decided before any mutation
        assert (step["passed"], step["matches"]) == (sum(1 for q in dry if q is not None), dry_matches)
        return step

    def fuse_map_points(self, T, ids, threshold=3.0):
        self.reserved = 0
        self.fuse_targets, self.fuse_steps = [int(T)], [self.fuse(T, ids, threshold)]

    # ---- LocalMapping::searchInNeighbors -------------------------------------------------------------------------------
    def target_list(self, current):
        marked, out = set(), []
        for kfn in self.conn.ordered[current][:10]:
            if self.store[kfn]["bad"] or kfn in marked:
                continue
            out.append(kfn)
            marked.add(kfn)
            for kfs in self.conn.ordered[kfn][:5]:
                if self.store[kfs]["bad"] or kfs in marked or kfs == current:
                    continue
                out.append(kfs)
        return out

    def live_ids(self, k):
        kf = self.store[k]
        return [kf["ids"][i] for i in range(len(kf["ids"])) if (kf["flags"][i] & 1) and kf["ids"][i] >= 0]

    def search_in_neighbors(self, current):
        self.fuse_targets, self.fuse_steps, self.reserved = [], [], 0
        if self.erased[current] or self.store[current]["pose"] is None:
            self.sticky |= STICKY_INVALID
            self.update_connections([current])
            return
        targets = self.target_list(current)
        snapshot = self.live_ids(current)
        for T in targets:
            self.fuse_targets.append(T), self.fuse_steps.append(self.fuse(T, snapshot))
        cand, seen = [], set()
        for T in targets:
            if self.erased[T]:
                continue
            for p in self.live_ids(T):
                if p not in seen and self.observations(p):
                    seen.add(p), cand.append(p)
        self.fuse_targets.append(current), self.fuse_steps.append(self.fuse(current, cand))
        live = []
        for p in self.live_ids(current):
            if p not in live:
                live.append(p)
        self.compute_descriptors(live)
        self.refresh(live)
        self.update_connections([current])

    def fuse_result(self):
        steps = [tuple(s[k] for k in STEP) for s in self.fuse_steps]
        return dict(targets=list(self.fuse_targets), per_target=steps, totals=tuple(sum(s[c] for s in steps) for c in range(len(STEP))))
