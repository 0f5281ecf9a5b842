"""Model of the store's loop correction (test infrastructure): the propagation of the loop Sim3 with the point correction
(src/loopClosing.cpp:364-437) and the loop connections (:461-479), restated in plain Python on top of
tests/pose_graph_store_ref.py's PoseGraphModel (the store, the connections, the refresh, csrc/sim3_compose.h line by line), as
the contract block of include/vo_hip.h states them.

The model is the contract's closed form, not the reference's loop: which key-frame corrects a point is a minimum over its
holders, and the pose a holder is refreshed with is chosen by comparing positions in corr_kf.  tests/test_loop_correct_ref.py
holds it against a pointer-object transcription that really runs in the reference's order.

LoopCorrectModel is a mix-in in front of any model of that family (tests/loop_correct_inputs.py puts it in front of the loop
fusion's chain model)."""
import pose_graph_store_ref as pr
from local_ba_store_ref import EMPTY, OK, OVERFLOW, STICKY_INVALID
from new_points_ref import _center, _dot3

import math

import numpy as np

f32 = np.float32
STICKY_LC_CAPACITY = 256
ACCEPTED = 3
LC_RECORD = ("n_corr", "n_cp", "n_lc", "curr", "status", "n_rows_moved", "connections_status")


def scw8_from13(Scw13):
    """compute_sim3's Scw (R row-major, t, s) in the 8-double form: s3_from_pose on R, t with the scale appended"""
    S = pr.from_pose([float(x) for x in Scw13[:12]])
    return S[:7] + [float(Scw13[12])]


def pose_of_sim3(S):
    """step 6: SE3(s3_matrix(q), t / s), q as it stands"""
    return pr.matrix(S) + [S[4 + c] / S[7] for c in range(3)]


class LoopCorrectModel:
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.lc_caps = None
        self.lc_record = {k: 0 for k in LC_RECORD}
        self.lc_record.update(curr=-1, status=EMPTY, connections_status=EMPTY)
        self.lc = None            # dict(list, corr_kf, S_corr, S_uncorr, cp_id, cp_ref) of the last successful propagate
        self.lc_rows = None       # {key-frame: sorted loop connections} of the last loop_connections
        self.lc_log = []          # (id, key-frame it was corrected through, its position, [(holder, its position or -1)])

    def enable_loop_correct(self, max_corrected, max_corrected_points, max_loop_connections):
        self.lc_caps = (int(max_corrected), int(max_corrected_points), int(max_loop_connections))

    def update_connections(self, keyframes):
        """as the device does it: a listed key-frame outside the store or erased is skipped and raises the sticky bit"""
        for k in keyframes:
            if not (0 <= k < len(self.store)) or self.erased[k]:
                self.sticky |= STICKY_INVALID
        super().update_connections(keyframes)

    # ---- loopClosing.cpp:364-437 -------------------------------------------------------------------------------------------
    def propagate_loop(self, curr, Scw, state=ACCEPTED):
        rec = {k: 0 for k in LC_RECORD}
        rec.update(curr=int(curr), status=EMPTY, connections_status=EMPTY)
        self.lc_record, self.lc, self.lc_rows, self.lc_log = rec, None, None, []
        size = len(self.store)
        if state != ACCEPTED:
            self.sticky |= STICKY_INVALID
            return None
        self.update_connections([curr])                                    # 1. (:364)
        if not (0 <= curr < size) or self.erased[curr]:
            return None
        lst = [int(k) for k in self.conn.ordered[curr]] + [int(curr)]     # 2. (:367-368) no isBad test
        rec["n_corr"] = len(lst)
        if len(lst) > self.lc_caps[0]:
            self.sticky |= STICKY_LC_CAPACITY
            rec["status"] = OVERFLOW
            return None
        if not (float(Scw[7]) > 0.0) or any(not (0 <= k < size) or self.erased[k] or self.store[k]["pose"] is None for k in lst):
            self.sticky |= STICKY_INVALID
            return None
        corr = sorted(lst)
        pos_of = {k: j for j, k in enumerate(corr)}
        Scw = pr.load(Scw)                                                 # 3. (:378-398)
        Swc = pr.inv(pr.from_pose(self.store[curr]["pose"]))
        S_unc = [pr.from_pose(self.store[k]["pose"]) for k in corr]
        S_corr = [Scw if k == curr else pr.mul(pr.mul(S_unc[j], Swc), Scw) for j, k in enumerate(corr)]
        T_new = [pose_of_sim3(S) for S in S_corr]
        # 4. which key-frame corrects a point: the lowest-numbered corrected holder, at its first carrying feature
        through = {}
        for j, k in enumerate(corr):
            kf = self.store[k]
            for f in range(len(kf["ids"])):
                p = kf["ids"][f]
                if (kf["flags"][f] & 1) and p >= 0 and p not in through:
                    through[p] = (k, f)
        rec["n_cp"] = len(through)
        if len(through) > self.lc_caps[1]:
            self.sticky |= STICKY_LC_CAPACITY
            rec["status"] = OVERFLOW
            return None
        stored = [kf["pose"] for kf in self.store]
        rows = 0
        for p in sorted(through):
            k, f = through[p]
            j = pos_of[k]
            new = pr.act(pr.inv(S_corr[j]), pr.act(S_unc[j], [float(x) for x in self.store[k]["points"][f]]))
            live = self.carriers(p)
            for jj, i in live:
                self.store[jj]["points"][i] = new
            rows += len(live)
            # 5. the mixed state: corrected poses below position j, stored poses at j, above it and outside the set -- and since
            # k is the LOWEST corrected holder, no holder (the reference key-frame is one) lies below j: every pose is the stored one
            holders = [(h, pos_of.get(h, -1)) for h, _ in self.observations(p)]
            assert all(q < 0 or q >= j for _, q in holders), ("a corrected holder below the correcting key-frame", p, k, holders)
            self._refresh_with(p, lambda h: stored[h])
            self.lc_log.append((p, k, j, holders))
        for j, k in enumerate(corr):                                       # 6. (:430-435)
            self.store[k]["pose"] = T_new[j]
        self.update_connections(corr)                                      # 7. (:436)
        rec.update(status=OK, n_rows_moved=rows)
        ids = sorted(through)
        self.lc = dict(list=lst, corr_kf=corr, S_corr=S_corr, S_uncorr=S_unc, cp_id=ids, cp_ref=[through[p][0] for p in ids])
        return self.lc

    def _refresh_with(self, p, pose):
        """LocalBaModel.refresh for one point with the pose of holder h given by pose(h) (section 4k's operation order)"""
        live = self.carriers(p)
        if not live:
            return
        holders = self.observations(p)
        j0, i0 = live[0]
        pos = [float(x) for x in self.store[j0]["points"][i0]]
        r0 = self.store[j0]["ref"][i0]
        ref = r0 if any(j == r0 for j, _ in holders) else holders[0][0]
        s, n, lens = [0.0, 0.0, 0.0], 0, {}
        for j, i in holders:
            T = pose(j)
            if T is None:
                self.sticky |= STICKY_INVALID
                continue
            Ow = _center(T)
            d = [pos[c] + -Ow[c] for c in range(3)]
            ln = math.sqrt(_dot3(d[0], d[0], d[1], d[1], d[2], d[2]))
            s = [s[c] + d[c] / ln for c in range(3)]
            n += 1
            lens[j] = ln
        iref = dict(holders)[ref]
        for j, i in live:
            kf = self.store[j]
            kf["ref"][i] = ref
            if n:
                kf["normals"][i] = [s[c] / float(n) for c in range(3)]
            if ref in lens:
                maxd = f32(lens[ref]) * f32(self.sf[min(max(self.store[ref]["octave"][iref], 0), 15)])
                kf["maxd"][i], kf["mind"][i] = maxd, maxd / f32(self.sf[len(self.sf) - 1])

    # ---- loopClosing.cpp:461-479 -------------------------------------------------------------------------------------------
    def loop_connections(self):
        rec = self.lc_record
        rec.update(n_lc=0, connections_status=EMPTY)
        self.lc_rows = None
        if self.lc is None:
            self.sticky |= STICKY_INVALID
            return None
        inside = set(self.lc["list"])
        rows = {}
        for kf in self.lc["list"]:                                         # LIST order (:464)
            ok = 0 <= kf < len(self.store) and not self.erased[kf]
            old = set(self.conn.ordered[kf]) if ok else set()
            self.update_connections([kf])
            new = {j for j, w in self.conn.W[kf].items() if w != 0} if ok else set()
            rows[kf] = sorted(new - old - inside)
        n_lc = sum(len(r) for r in rows.values())
        rec["n_lc"] = n_lc
        if n_lc > self.lc_caps[2]:
            self.sticky |= STICKY_LC_CAPACITY
            rec["connections_status"] = OVERFLOW
            return None
        rec["connections_status"] = OK
        self.lc_rows = rows
        return rows

    def lc_inputs(self):
        """the arrays of the last propagate_loop / loop_connections as pose_graph_window takes them"""
        L = self.lc
        corr = {k: (L["S_corr"][j], L["S_uncorr"][j]) for j, k in enumerate(L["corr_kf"])}
        return pr.make_inputs(corr, self.lc_rows or {}, dict(zip(L["cp_id"], L["cp_ref"])))
