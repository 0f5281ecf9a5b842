"""Model of vo_kfstore_detect_loop and of the loop thread's erase locks (test infrastructure): LoopClosing::detectLoop
(src/loopClosing.cpp:52-175) transcribed line by line, with pointer-like key-frame objects and set / vector semantics, over
tests/kfdb_ref.py's Database (Map::detectLoopCandidates, Map::score) and tests/cull_ref.py's CullModel (the connection state of
tests/connections_ref.py with erased / locked / pending per key-frame).  setNotEraseLoopDetectingKF / setEraseLoopDetectingKF
(src/keyframe.cpp:541-557) are modelled without the erase: the store reports `pending` and the caller erases.

What the store adds to the reference is modelled as include/vo_hip.h states it: the capacities D and G with the sticky
DETECT_CAPACITY, the record, the refresh of the database's neighbour rows from the store's graph rows, an erased `current`."""
import numpy as np

NONE, GATED, NO_CANDIDATES, NOT_CONSISTENT, DETECTED, OVERFLOW = range(6)
STICKY_INVALID, STICKY_LOOP_CAPACITY, STICKY_DETECT_CAPACITY = 1, 64, 512
UNDECIDED, NO_MATCH, REJECTED, ACCEPTED = range(4)
DL_RECORD = ("outcome", "current", "n_excl", "n_conn", "min_score_bits", "n_candidates", "groups_before", "groups_after", "n_enough",
             "locked", "pending")


class KeyFrame:
    """what detectLoop touches of a KeyFrame*: id_, isBad(), orderedConnectKFs_, getConnectKFs(), bowVec_, the lock"""

    def __init__(self, model, k):
        self.m, self.id_ = model, k

    def __repr__(self):
        return "KF%d" % self.id_

    def isBad(self):
        return bool(self.m.cull.store[self.id_]["bad"])

    @property
    def orderedConnectKFs_(self):
        return [self.m.kfs[j] for j in self.m.cull.conn.ordered[self.id_]]

    def getConnectKFs(self):
        """set<KeyFrame*> of connectedKFWts_'s keys: nothing is filtered"""
        return set(self.m.kfs[j] for j, w in self.m.cull.conn.W[self.id_].items() if w != 0)

    @property
    def bowVec_(self):
        kf = self.m.db.kfs[self.id_]
        return kf.words, kf.values

    def setNotEraseLoopDetectingKF(self):
        self.m.cull.locked[self.id_] = 1

    def setEraseLoopDetectingKF(self):
        if not self.m.loop_edges[self.id_]:
            self.m.cull.locked[self.id_] = 0
        # (toBeEraseAfterLoopDetect_: reported, the caller erases)


class DetectModel:
    def __init__(self, cull, db, D, G):
        self.cull, self.db, self.D, self.G = cull, db, D, G
        self.kfs = []
        self.loop_edges = []
        self.prevConsistentGroups_ = []       # [(set of KeyFrame, count)]
        self.enoughConCandidates_ = []
        self.keyframe_curr_ = None
        self.sticky = 0
        self.record = dict.fromkeys(DL_RECORD, 0)
        self.candidates = []
        self.last_loop_keyframe = 0
        self.lock_result = (0, [])
        self.grow()

    def grow(self):
        while len(self.kfs) < len(self.cull.store):
            self.kfs.append(KeyFrame(self, len(self.kfs)))
            self.loop_edges.append(set())

    def add_loop_edge(self, a, b):
        """KeyFrame::addLoopEdge on both (keyframe.cpp:528-533)"""
        self.loop_edges[a].add(b), self.loop_edges[b].add(a)
        self.cull.locked[a] = self.cull.locked[b] = 1

    # ---- the store's side of the query ---------------------------------------------------------------------------------
    def refresh_neighbors(self):
        """getBestCovisibleKFs(10) of every key-frame as the store's graph rows hold it"""
        for k in range(len(self.kfs)):
            self.db.set_neighbors(k, self.cull.conn.graph(k)[0])

    def _rec(self, **kw):
        cur = self.keyframe_curr_.id_
        self.record.update(kw)
        self.record.update(groups_after=len(self.prevConsistentGroups_), n_enough=len(self.enoughConCandidates_),
                           locked=self.cull.locked[cur], pending=self.cull.pending[cur])
        return self.record["outcome"]

    def _overflow(self):
        self.sticky |= STICKY_DETECT_CAPACITY
        self.prevConsistentGroups_ = []
        self.enoughConCandidates_ = []
        self.keyframe_curr_.setEraseLoopDetectingKF()
        return self._rec(outcome=OVERFLOW)

    # ---- LoopClosing::detectLoop -----------------------------------------------------------------------------------------
    def detect_loop(self, current, lastLoopKFId_):
        self.grow()
        self.record = dict.fromkeys(DL_RECORD, 0)
        self.record.update(current=current, groups_before=len(self.prevConsistentGroups_), groups_after=len(self.prevConsistentGroups_))
        self.candidates = []
        self.enoughConCandidates_ = []       # (the store's enough list is per call; the reference clears it at :95)
        if self.cull.erased[current]:
            self.sticky |= STICKY_INVALID
            self.keyframe_curr_ = self.kfs[current]
            return NONE
        self.keyframe_curr_ = self.kfs[current]                      # :56
        self.keyframe_curr_.setNotEraseLoopDetectingKF()             # :59
        if self.keyframe_curr_.id_ < lastLoopKFId_ + 10:             # :62
            self.keyframe_curr_.setEraseLoopDetectingKF()
            return self._rec(outcome=GATED)
        connectKFs = self.keyframe_curr_.orderedConnectKFs_          # :68
        currBowVec = self.keyframe_curr_.bowVec_
        conn = []
        for kf in connectKFs:                                        # :72-83 (Database.min_score takes the kept ones)
            if kf.isBad():
                continue
            conn.append(kf.id_)
        minScore = self.db.min_score(currBowVec[0], currBowVec[1], conn)
        excl = set(kf.id_ for kf in self.keyframe_curr_.getConnectKFs()) | {current}    # map.cpp:212-215
        self.refresh_neighbors()
        cands, _ = self.db.query_loop(currBowVec[0], currBowVec[1], sorted(excl), min_score=minScore)
        candidates = [self.kfs[c] for c in cands]                    # :85
        self.candidates = list(cands[:self.D])
        self.record.update(n_excl=len(excl), n_conn=len(conn), min_score_bits=int(np.float32(minScore).view(np.int32)),
                           n_candidates=len(cands))
        if not candidates:                                           # :87-93
            self.prevConsistentGroups_ = []
            self.keyframe_curr_.setEraseLoopDetectingKF()
            return self._rec(outcome=NO_CANDIDATES)
        if len(candidates) > self.D:
            return self._overflow()
        self.enoughConCandidates_ = []                               # :95
        currConsistentGroups = []
        prevConsistentGroupFlags = [False] * len(self.prevConsistentGroups_)
        for kf in candidates:                                        # :108
            candidateGroup = kf.getConnectKFs()
            candidateGroup.add(kf)
            enoughConsistent = False
            someConsistent = False
            for j in range(len(self.prevConsistentGroups_)):         # :121
                prevGroup = self.prevConsistentGroups_[j][0]
                consist = False
                for it in candidateGroup:
                    if it in prevGroup:
                        consist = True
                        someConsistent = True
                        break
                if consist:
                    prevCnt = self.prevConsistentGroups_[j][1]
                    currCnt = prevCnt + 1
                    if not prevConsistentGroupFlags[j]:
                        currConsistentGroups.append((set(candidateGroup), currCnt))
                        prevConsistentGroupFlags[j] = True
                    if currCnt >= 3 and not enoughConsistent:
                        self.enoughConCandidates_.append(kf)
                        enoughConsistent = True
            if not someConsistent:                                   # :158
                currConsistentGroups.append((set(candidateGroup), 0))
        if len(currConsistentGroups) > self.G:
            return self._overflow()
        self.prevConsistentGroups_ = currConsistentGroups            # :165
        if not self.enoughConCandidates_:                            # :167
            self.keyframe_curr_.setEraseLoopDetectingKF()
            return self._rec(outcome=NOT_CONSISTENT)
        return self._rec(outcome=DETECTED)

    # ---- what the result calls return --------------------------------------------------------------------------------------
    def result(self):
        out = dict(self.record)
        out.update(candidates=list(self.candidates), enough=[kf.id_ for kf in self.enoughConCandidates_])
        return out

    def groups(self, size=None):
        """-> (counts, members uint8 [n, size])"""
        size = len(self.kfs) if size is None else size
        members = np.zeros((len(self.prevConsistentGroups_), size), np.uint8)
        for g, (group, _) in enumerate(self.prevConsistentGroups_):
            for kf in group:
                members[g, kf.id_] = 1
        return [cnt for _, cnt in self.prevConsistentGroups_], members

    def groups_as_sets(self):
        return [(sorted(kf.id_ for kf in group), cnt) for group, cnt in self.prevConsistentGroups_]

    # ---- computeSim3's lock side (:208, :290-296, :331-346) ---------------------------------------------------------------------
    def lock_candidates(self, cands):
        for c in cands:
            self.kfs[c].setNotEraseLoopDetectingKF()

    def release_loop_locks(self, state, cands, current, match=-1):
        released, pending = 0, []
        todo = [] if state == UNDECIDED else [c for c in cands if not (state == ACCEPTED and c == match)]
        if state in (NO_MATCH, REJECTED):
            todo.append(current)
        for k in todo:
            if not self.cull.locked[k]:
                continue
            self.kfs[k].setEraseLoopDetectingKF()
            if self.cull.locked[k]:
                continue
            released += 1
            if self.cull.pending[k]:
                pending.append(k)
        self.lock_result = (released, pending)
        return self.lock_result
