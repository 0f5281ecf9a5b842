"""Model of the store's loop fusion (test infrastructure): LoopClosing::searchAndFuse (src/loopClosing.cpp:496-516),
Matcher::fuseByPose (src/matcher.cpp:1135-1238) and MapPoint::replaceMapPoint (src/mappoint.cpp:214-253) restated on the store,
strictly sequential, on top of tests/fuse_ref.py's FuseModel (the store, the gates of a candidate, the window, replace, the
recent list, the margins of every float gate).

A pass is fuseByPose(T, S, ids, replace, threshold) and the replace loop behind it.  The pose of a pass comes from its Sim3 by
csrc/sim3_compose.h's operations (tests/pose_graph_store_ref.py), with the translation NOT divided by the scale
(matcher.cpp:1144); divide_t = True is the variant without that quirk, for the test that pins it.

Every pass asserts the two derivations of DESIGN.md section 4q: (1) the gates and the match of every candidate can be decided
on the state the pass starts from -- hits interact only through the feature they hit; (2) in the replace phase the As and the
Bs are disjoint and the Bs distinct."""
import pose_graph_store_ref as pr
from fuse_ref import CARRIERS_MAX, STICKY_FUSE, STICKY_INVALID, FuseModel
from new_points_ref import TH_LOW, hamming

PASS = ("passed", "matches", "adds", "replaces", "moved", "cleared")
ACCEPTED = 3


def pose_from_sim3(S, divide_t=False):
    """Tcw12 = SE3(R(q), t) of a Sim3 as an entry point receives it"""
    S = pr.load(S)
    t = [S[4 + c] / S[7] for c in range(3)] if divide_t else S[4:7]
    return pr.matrix(S) + list(t)


class LoopFuseModel(FuseModel):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.lf_passes, self.lf_targets = [], []
        self.lf_log = []        # (pass, list position, candidate, feature, kind, A) of every match: add / replace / capacity
        self.lf_moved = []      # (pass, A, B, features that took B) of every replace carried out
        self.lf_gates = []      # (pass, list position, candidate, "negative" / "bad" / "held" / "gates" / "passed")
        self.divide_t = False

    def enable_loop_fuse(self, max_corrected, max_loop_points):
        self.max_corrected, self.max_loop_points = int(max_corrected), int(max_loop_points)

    # ---- the window search of fuseByPose (:1193-1218): no chi-square gate, no u_right -------------------------------------
    def search_by_pose(self, T, q):
        kf, best, best_i, n0 = self.store[T], 256, -1, len(self.margins)
        for i in self.features_in_area(T, q):
            o = kf["octave"][i]
            if o < q["level"] - 1 or o > q["level"]:
                continue
            d = hamming(q["pdesc"], kf["desc"][i])
            if d < best:
                best, best_i = d, i
        self._weak(q["p"], n0)
        return best_i if best <= TH_LOW else -1

    def _candidate(self, T, p, threshold):
        """-> (reason, query or None) of loop point p against T under the pose set for the pass"""
        if p < 0:
            return "negative", None
        if not self.observations(p):
            return "bad", None
        if self.observation(T, p) >= 0:
            return "held", None
        q = self.project(T, p, threshold)
        return ("passed", q) if q is not None else ("gates", None)

    # ---- one pass ------------------------------------------------------------------------------------------------------------
    def fuse_by_pose(self, n_pass, T, S, ids, threshold):
        step = {k: 0 for k in PASS}
        if not (0 <= T < len(self.store)) or self.erased[T] or self.store[T]["pose"] is None:
            self.sticky |= STICKY_INVALID
            return step
        kf = self.store[T]
        stored, kf["pose"] = kf["pose"], pose_from_sim3(S, self.divide_t)
        try:
            self._pass(n_pass, T, kf, [int(p) for p in ids], threshold, step)
        finally:
            kf["pose"] = stored
        return step

    def _pass(self, n_pass, T, kf, ids, threshold, step):
        # derivation 1: decided on the state the pass starts from
        dry = []
        for p in ids:
            reason, q = self._candidate(T, p, threshold)
            dry.append((reason, self.search_by_pose(T, q) if q is not None else -1))
        dry_passed, dry_matches = sum(1 for r, _ in dry if r == "passed"), sum(1 for _, f in dry if f >= 0)
        self.reserved += dry_matches
        if dry_passed > self.max_candidates or self.reserved > self.max_candidates:
            self.sticky |= STICKY_FUSE
            self.undone.append((T, "candidates" if dry_passed > self.max_candidates else "matches"))
            step.update(passed=dry_passed, matches=dry_matches)
            return
        replace = [None] * len(ids)
        for i, p in enumerate(ids):
            reason, q = self._candidate(T, p, threshold)
            f = self.search_by_pose(T, q) if q is not None else -1
            assert (reason, f) == dry[i], ("derivation 1", n_pass, i, p)
            self.lf_gates.append((n_pass, i, p, reason))
            if q is None:
                continue
            step["passed"] += 1
            self.queries.append((T, q))
            if f < 0:
                continue
            step["matches"] += 1
            if (kf["flags"][f] & 1) and kf["ids"][f] >= 0:
                replace[i] = int(kf["ids"][f])                     # (:1224-1227) nothing is written yet
            else:
                self._take(T, f, p, self.attributes(p))            # (:1229-1232) at once
                kf["flags"][f] |= 1
                step["adds"] += 1
                self.lf_log.append((n_pass, i, p, f, "add", -1))
        # derivation 2
        As, Bs = {a for a in replace if a is not None}, [ids[i] for i, a in enumerate(replace) if a is not None]
        assert not (As & set(Bs)) and len(set(Bs)) == len(Bs), ("derivation 2", n_pass)
        for i, A in enumerate(replace):                            # loopClosing.cpp:508-513
            if A is None:
                continue
            B = ids[i]
            step["replaces"] += 1
            if A == B:
                continue
            if max(len(self.carriers(A)), len(self.carriers(B))) > CARRIERS_MAX:
                self.sticky |= STICKY_FUSE
                self.lf_log.append((n_pass, i, B, -1, "capacity", A))
                continue
            takes = sum(1 for j, _ in self.observations(A) if self.observation(j, B) < 0)
            self.replace(A, B, step)
            step["moved"] += 1 if takes else 0
            self.lf_log.append((n_pass, i, B, -1, "replace", A))
            self.lf_moved.append((n_pass, A, B, takes))

    # ---- LoopClosing::searchAndFuse ------------------------------------------------------------------------------------------
    def search_and_fuse(self, corr_kf, S_corr, ids, threshold=4.0, state=ACCEPTED):
        """state: the _loop form's state of the last compute_sim3; anything but ACCEPTED changes nothing"""
        self.reserved, self.lf_passes, self.lf_targets = 0, [], []
        if state != ACCEPTED:
            self.sticky |= STICKY_INVALID
            return
        corr_kf = [int(k) for k in corr_kf]
        assert all(a < b for a, b in zip(corr_kf, corr_kf[1:])) and len(corr_kf) <= self.max_corrected and len(ids) <= self.max_loop_points
        for n, (T, S) in enumerate(zip(corr_kf, S_corr)):
            self.lf_targets.append(T)
            self.lf_passes.append(self.fuse_by_pose(n, T, [float(x) for x in S], ids, threshold))

    def loop_fuse_result(self):
        per = [tuple(s[k] for k in PASS) for s in self.lf_passes]
        return dict(passes=len(per), per_pass=per, totals=tuple(sum(s[c] for s in per) for c in range(len(PASS))))
