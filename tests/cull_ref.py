"""Model of vo_kfstore_cull_keyframes / vo_kfstore_erase_keyframe (test infrastructure): LocalMapping::cullingKeyFrames
(src/localMapping.cpp:434-494) with KeyFrame::eraseKeyFrame, eraseConnection (src/keyframe.cpp:400-526) and
MapPoint::eraseObservedKF / eraseMapPoint (src/mappoint.cpp:333-381), restated in plain Python over the list-of-dicts store
of tests/local_map_ref.py together with tests/connections_ref.py's Connections.

A key-frame is a dict with ids, flags, bad (local_map_ref) and octave, depth, u_right per feature; CullModel adds erased,
locked and pending per key-frame.  The definitions the contract in include/vo_hip.h states:
  j HOLDS p          one of j's features has ids == p and bit 0 set, and j is not erased
  j's OBSERVATION    its lowest-numbered such feature
  obs(p)             the sum over the holders of 2 where u_right >= 0 at the observation, else 1
  bad(j)             the dict's bad flag
Pointer-keyed containers are walked in ascending key-frame number (connections_ref)."""
import numpy as np

from connections_ref import Connections, _sorted, holder_index

KEPT, ERASED, PENDING, SKIPPED = 0, 1, 2, 3


class CullModel:
    def __init__(self):
        self.store, self.conn = [], Connections()
        self.erased, self.locked, self.pending = [], [], []
        self.result = []
        # what the calls did, for the tests' non-vacuity conditions
        # calls: (kind, [key-frames erased]) per cull / erase call; reparented: (child, new parent, the erased one's parent)
        # skipped_updates: listed key-frames update_connections left out (the device's sticky INVALID bit)
        self.log = dict(calls=[], dead_points=0, reparented=[], skipped_updates=0)

    # ---- the store -----------------------------------------------------------------------------------------------------
    def insert(self, ids, flags, bad=False):
        n = len(ids)
        self.store.append(dict(ids=[int(x) for x in ids], flags=[int(x) for x in flags], bad=bool(bad), octave=[0] * n,
                               depth=[np.float32(-1)] * n, u_right=[np.float32(-1)] * n))
        self.erased.append(0), self.locked.append(0), self.pending.append(0)
        self.conn.grow(len(self.store))
        return len(self.store) - 1

    def set_keypoints(self, k, octave, depth, u_right):
        kf = self.store[k]
        kf["octave"] = [int(x) for x in octave]
        kf["depth"] = [np.float32(x) for x in depth]
        kf["u_right"] = [np.float32(x) for x in u_right]

    def update_points(self, k, ids, flags):
        self.store[k]["ids"], self.store[k]["flags"] = [int(x) for x in ids], [int(x) for x in flags]

    def set_bad(self, k, bad=True):
        self.store[k]["bad"] = bool(bad)

    def set_erase_lock(self, k, on=True):
        self.locked[k] = int(bool(on))

    def _visible(self):
        """the store as the observation index sees it: an erased key-frame holds nothing"""
        return [dict(ids=[], flags=[]) if self.erased[k] else kf for k, kf in enumerate(self.store)]

    def update_connections(self, keyframes):
        """update(k) in list order; a number outside the store or an erased key-frame is skipped"""
        vis = self._visible()
        index = holder_index(vis)
        for k in keyframes:
            if 0 <= k < len(self.store) and not self.erased[k]:
                self.conn.update(vis, k, index)
            else:
                self.log["skipped_updates"] += 1

    # ---- the definitions -----------------------------------------------------------------------------------------------
    def observation(self, j, p):
        """feature index of j's observation of p, or -1"""
        if self.erased[j]:
            return -1
        kf = self.store[j]
        for i in range(len(kf["ids"])):
            if kf["ids"][i] == p and (kf["flags"][i] & 1):
                return i
        return -1

    def observations(self, p):
        """[(holder, feature)] in ascending key-frame number"""
        out = []
        for j in range(len(self.store)):
            i = self.observation(j, p)
            if i >= 0:
                out.append((j, i))
        return out

    def obs(self, p, without=-1):
        return sum(2 if self.store[j]["u_right"][i] >= 0 else 1 for j, i in self.observations(p) if j != without)

    # ---- cullingKeyFrames ----------------------------------------------------------------------------------------------
    def count(self, k, th_depth):
        """(mp_cnt, re_obs) of candidate k (:449-485)"""
        th = np.float32(th_depth)
        kf = self.store[k]
        mp_cnt = re_obs = 0
        for i in range(len(kf["ids"])):
            if not (kf["flags"][i] & 1):
                continue
            if kf["depth"][i] < 0 or kf["depth"][i] > th:
                continue
            mp_cnt += 1
            p = kf["ids"][i]
            if self.obs(p) > 3:
                seen = 0
                for j, f in self.observations(p):
                    if j == k or self.store[j]["bad"]:
                        continue
                    if self.store[j]["octave"][f] <= kf["octave"][i] + 1:
                        seen += 1
                if seen >= 3:
                    re_obs += 1
        return mp_cnt, re_obs

    def cull(self, current, th_depth):
        """-> [(key-frame, mp_cnt, re_obs, decision)] per candidate, also kept as self.result"""
        self.result = []
        self.log["calls"].append(("cull", []))
        if self.erased[current]:
            return self.result
        for k in list(self.conn.ordered[current]):   # the copy of :439
            if k == 0 or self.store[k]["bad"] or self.erased[k]:
                self.result.append((k, 0, 0, SKIPPED))
                continue
            mp_cnt, re_obs = self.count(k, th_depth)
            decision = KEPT
            if re_obs > 0.9 * mp_cnt:
                decision = PENDING if self.locked[k] else ERASED
                self.erase(k)
            self.result.append((k, mp_cnt, re_obs, decision))
        return self.result

    # ---- eraseKeyFrame -------------------------------------------------------------------------------------------------
    def erase(self, k):
        c = self.conn
        if k == 0 or self.erased[k]:
            return
        if self.locked[k]:
            self.pending[k] = 1
            return
        # (:415-416) eraseConnection over k's own map: quirk Q-E1
        for j in sorted(c.W[k]):
            if k in c.W[j]:
                del c.W[j][k]
                c.ordered[j], c.weights[j] = _sorted([(w, x) for x, w in c.W[j].items()])
        # (:418-420) eraseObservedKF per map point of k, in feature order
        kf = self.store[k]
        done = {}
        for i in range(len(kf["ids"])):
            p = kf["ids"][i]
            if not (kf["flags"][i] & 1) or p in done:
                continue
            done[p] = True   # k's observation of p; a later feature with p finds k gone from the holders
            if self.obs(p, without=k) <= 2:
                self.log["dead_points"] += 1
                for j, other in enumerate(self.store):
                    if self.erased[j]:
                        continue   # (k itself is not erased yet)
                    for f in range(len(other["ids"])):
                        if other["ids"][f] == p:
                            other["flags"][f] &= ~1
        c.W[k], c.ordered[k], c.weights[k] = {}, [], []
        # (:429-483) the spanning tree
        parent = c.parent[k]
        cands = [parent] if parent >= 0 else []
        children = set(c.children[k])
        while children:
            best, pick = -1, None
            for ch in sorted(children):
                if self.store[ch]["bad"]:
                    continue
                for x in c.ordered[ch]:
                    if x in cands and c.W[ch][x] > best:
                        best, pick = c.W[ch][x], (ch, x)
            if pick is None:
                break
            ch, x = pick
            c.parent[ch] = x
            c.children[x].add(ch)
            cands.append(ch)
            children.discard(ch)
            self.log["reparented"].append((ch, x, parent))
        for ch in children:
            c.parent[ch] = parent
            if parent >= 0:
                c.children[parent].add(ch)
        c.children[k] = set()
        if parent >= 0:
            c.children[parent].discard(k)
        self.erased[k], kf["bad"] = 1, True
        if self.log["calls"]:
            self.log["calls"][-1][1].append(k)

    def erase_keyframe(self, k):
        """the explicit call"""
        self.log["calls"].append(("erase", []))
        self.erase(k)

    # ---- what the entry points return ----------------------------------------------------------------------------------
    def state(self, k):
        return dict(erased=self.erased[k], locked=self.locked[k], pending=self.pending[k])

    def connections(self, k):
        return self.conn.state(k, len(self.store))

    def flags(self, k):
        return list(self.store[k]["flags"]), int(self.store[k]["bad"])
