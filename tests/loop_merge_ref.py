"""Model of the store's merge of the loop matches (test infrastructure): the loop of LoopClosing::correctLoop that gives the
current key-frame the loop's map points (src/loopClosing.cpp:439-455), restated on the store as the contract block of
include/vo_hip.h states it, strictly sequential, on tests/fuse_ref.py's replace, attributes and descriptor code.

LoopMergeModel is a mix-in in front of any model of tests/loop_correct_inputs.py's ChainModel family.

Every call asserts the derivation of DESIGN.md section 4s: a step reads and writes only what belongs to its own ids {A0_i, B_i}
(A0_i: the id feature i of curr carries as the call begins), so steps with disjoint id sets commute.  The steps that share no id
with any other step (ALONE) are re-run first, in DESCENDING feature order, the others (ORDERED) behind them in ascending order,
on a copy of the state the call began with: the store, the recent list, the sticky word, the record and the branches must come
out the same."""
import copy

import numpy as np

from fuse_ref import CARRIERS_MAX, STICKY_FUSE, STICKY_INVALID

STICKY_UPKEEP = 8
ACCEPTED = 3
LM_RECORD = ("steps", "adds", "noops", "replaces", "moved", "cleared", "n_dead", "undone", "ordered", "curr")
NONE, ADD, NOOP, REPLACE, DEAD, UNDONE = range(6)
ALONE, ORDERED = 1, 2


def store_bytes(m):
    """everything a merge may write, as bytes"""
    out = []
    for kf in m.store:
        out.append({k: (None if v is None else np.asarray(v).tobytes()) for k, v in kf.items()})
    return out, copy.deepcopy(m.recent), m.sticky


class LoopMergeModel:
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.lm_record = {k: 0 for k in LM_RECORD}
        self.lm_branch = []       # the branch at every feature of curr
        self.lm_kind = []         # 0 no step, ALONE, ORDERED
        self.lm_log = []          # (feature, branch, A or -1, B, features that took B)

    def enable_loop_merge(self):
        pass

    def _has(self, curr, i):
        kf = self.store[curr]
        return bool(kf["flags"][i] & 1) and kf["ids"][i] >= 0

    # ---- the plan: which steps share an id -------------------------------------------------------------------------------------
    def merge_plan(self, curr, match_ids):
        n = min(len(match_ids), len(self.store[curr]["ids"]))
        sets = {i: {int(match_ids[i])} | ({int(self.store[curr]["ids"][i])} if self._has(curr, i) else set())
                for i in range(n) if match_ids[i] >= 0}
        count = {}
        for s in sets.values():
            for p in s:
                count[p] = count.get(p, 0) + 1
        return [0 if i not in sets else (ORDERED if any(count[p] > 1 for p in sets[i]) else ALONE) for i in range(n)]

    # ---- one step (:443-454) ---------------------------------------------------------------------------------------------------
    def _merge_step(self, curr, i, B, rec, branch, log):
        kf = self.store[curr]
        rec["steps"] += 1
        has = self._has(curr, i)
        A = int(kf["ids"][i]) if has else -1
        if has and A == B:                                                 # mappoint.cpp:216
            rec["noops"] += 1
            branch[i] = NOOP
        elif not self.carriers(B):                                         # nobody holds B: no attributes to restate
            rec["n_dead"] += 1
            branch[i] = DEAD
        elif has:                                                          # A->replaceMapPoint(B) (:447)
            rec["replaces"] += 1
            if max(len(self.carriers(A)), len(self.carriers(B))) > CARRIERS_MAX:
                self.sticky |= STICKY_FUSE
                rec["undone"] += 1
                branch[i] = UNDONE
            else:
                takes = sum(1 for j, _ in self.observations(A) if self.observation(j, B) < 0)
                step = dict(cleared=0)
                self.replace(A, B, step)
                rec["cleared"] += step["cleared"]
                rec["moved"] += 1 if takes else 0
                branch[i] = REPLACE
                log.append((i, REPLACE, A, B, takes))
                return
        else:                                                              # addMapPoint + addObservation + computeDescriptor (:450-452)
            self._take(curr, i, B, self.attributes(B))
            kf["flags"][i] |= 1
            rec["adds"] += 1
            branch[i] = ADD
            if len(self.carriers(B)) > CARRIERS_MAX:
                self.sticky |= STICKY_UPKEEP
            else:
                self.compute_descriptors([B])
        log.append((i, branch[i], A, B, 0))

    def _merge_run(self, curr, match_ids, order, kinds):
        n = len(kinds)
        rec, branch, log = {k: 0 for k in LM_RECORD}, [NONE] * len(self.store[curr]["ids"]), []
        rec["curr"] = int(curr)
        for i in order:
            self._merge_step(curr, i, int(match_ids[i]), rec, branch, log)
        rec["ordered"] = sum(1 for i in range(n) if kinds[i] == ORDERED)
        return rec, branch, log

    # ---- loopClosing.cpp:439-455 -----------------------------------------------------------------------------------------------
    def merge_loop_matches(self, curr, match_ids, state=ACCEPTED):
        """state: the _loop form's state of the last compute_sim3; anything but ACCEPTED changes nothing"""
        rec = {k: 0 for k in LM_RECORD}
        rec["curr"] = int(curr)
        self.lm_record, self.lm_branch, self.lm_kind, self.lm_log = rec, [], [], []
        if state != ACCEPTED or not (0 <= curr < len(self.store)) or self.erased[curr]:
            self.sticky |= STICKY_INVALID
            return rec
        match_ids = [int(p) for p in match_ids]
        kinds = self.merge_plan(curr, match_ids)
        steps = [i for i, k in enumerate(kinds) if k]
        begin = (copy.deepcopy(self.store), copy.deepcopy(self.recent), self.sticky)
        # the derivation: the alone steps first, backwards, the ordered ones behind them
        other = [i for i in reversed(steps) if kinds[i] == ALONE] + [i for i in steps if kinds[i] == ORDERED]
        permuted = self._merge_run(curr, match_ids, other, kinds)
        permuted_state = store_bytes(self)
        self.store, self.recent, self.sticky = begin
        rec, branch, log = self._merge_run(curr, match_ids, steps, kinds)
        assert (rec, branch) == permuted[:2] and sorted(log) == sorted(permuted[2]), ("derivation: the record", rec, permuted[0])
        assert store_bytes(self) == permuted_state, "derivation: the store"
        self.lm_record, self.lm_branch, self.lm_kind, self.lm_log = rec, branch, kinds, log
        return rec

    def loop_merge_result(self, max_features):
        per = np.zeros(max_features, np.int32)
        per[:len(self.lm_branch)] = self.lm_branch
        return dict(record=dict(self.lm_record), per_feature=per)
