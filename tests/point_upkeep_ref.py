"""Model of the store's map-point upkeep (test infrastructure): LocalMapping::processNewKeyFrame (src/localMapping.cpp:100-130)
and cullingMapPoints (:496-524) with MapPoint::computeDescriptor (src/mappoint.cpp:118-179) and eraseMapPoint (:362-381),
restated in numpy on top of tests/local_ba_store_ref.py's LocalBaModel (the store, the connections, createNewMapPoints, the
refresh) and tests/new_points_ref.py's median_descriptor.

The definitions are tests/cull_ref.py's: j HOLDS p, j's OBSERVATION of p, obs(p), bad(j); pointer-keyed containers are walked
in ascending key-frame number.  The found ratio is a float32 division compared in float32.  The recent list is a dict keyed
by id: no outcome depends on its order."""
import numpy as np

from local_ba_store_ref import LocalBaModel
from new_points_ref import median_descriptor

f32 = np.float32
STICKY_INVALID, STICKY_UPKEEP = 1, 8
PROCESS, CULL, CREATED = 1, 2, 3
DESC_MAX_HOLDERS = 1024
RECORD = ("kind", "current", "n_tracked", "n_new", "n_appended", "n_dead", "n_ratio", "n_few_obs", "n_matured", "n_kept", "n_erased",
          "n_recent")
DEAD, RATIO, FEW_OBS, MATURED, KEPT = 1, 2, 3, 4, 5


def found_ratio_low(found, visible):
    """`getFoundRatio() < 0.25f` (localMapping.cpp:507, mappoint.cpp:330)"""
    with np.errstate(all="ignore"):
        return bool(f32(found) / f32(visible) < f32(0.25))


class UpkeepModel(LocalBaModel):
    def __init__(self, cam6=None, scale_factors=None, first_point_id=0, caps=(64, 8192, 65536), exp=None, log=None, max_recent=None):
        super().__init__(cam6, scale_factors, first_point_id, caps, exp, log)
        self.max_recent = max_recent      # None: no opt-in
        self.recent = {}                  # id -> [first_kf, found, visible]
        self.up_record = {k: 0 for k in RECORD}
        self.up_erased = []
        self.outcomes = {}                # id -> branch of the last cull call (for the tests' non-vacuity conditions)

    # ---- MapPoint::computeDescriptor -----------------------------------------------------------------------------------
    def descriptor_set(self, p):
        """desp (:133-140): the desc rows of p's holders that are not bad, ascending, each at its observation"""
        return [self.store[j]["desc"][i] for j, i in self.observations(p) if not self.store[j]["bad"]]

    def compute_descriptors(self, ids):
        for p in ids:
            if p < 0:
                continue
            desp = self.descriptor_set(int(p))
            if not desp:
                continue
            if len(desp) > DESC_MAX_HOLDERS:
                self.sticky |= STICKY_UPKEEP
                continue
            win = np.array(desp[median_descriptor(desp)], np.uint8)
            for j, i in self.carriers(int(p)):
                self.store[j]["pdesc"][i] = win

    # ---- processNewKeyFrame --------------------------------------------------------------------------------------------
    def _record(self, kind, current, **kw):
        self.up_record = dict({k: 0 for k in RECORD}, kind=kind, current=current, n_recent=len(self.recent), **kw)
        self.up_erased = []

    def _append(self, kind, current, ids, **kw):
        fits = len(self.recent) + len(ids) <= self.max_recent
        if fits:
            for p in ids:
                self.recent[p] = [current, 1, 1]       # (mappoint.cpp:38-41)
        else:
            self.sticky |= STICKY_UPKEEP
        self._record(kind, current, n_new=len(ids), n_appended=len(ids) if fits else 0, **kw)

    def split(self, current):
        """-> (tracked, created-with) ids of the current key-frame, each once, in feature order"""
        kf, seen, tracked, alone = self.store[current], set(), [], []
        for i in range(len(kf["ids"])):
            p = kf["ids"][i]
            if not (kf["flags"][i] & 1) or p < 0 or p in seen:
                continue
            seen.add(p)
            (tracked if any(j != current for j, _ in self.observations(p)) else alone).append(p)
        return tracked, alone

    def process_new_keyframe(self, current):
        if self.erased[current]:
            self.sticky |= STICKY_INVALID
            self._record(PROCESS, current)
            self.update_connections([current])          # (skipped there: an erased key-frame)
            return
        tracked, alone = self.split(current)
        self.refresh(tracked)
        self.compute_descriptors(tracked)
        self._append(PROCESS, current, [p for p in alone if p not in self.recent], n_tracked=len(tracked))
        self.update_connections([current])

    def create(self, current, max_neighbors=10):
        res = super().create(current, max_neighbors)
        if self.max_recent is not None:
            self._append(CREATED, current, [row[3] for row in res["created"]])     # addedMapPoints_.push_back (:355)
        return res

    # ---- the counters --------------------------------------------------------------------------------------------------
    def add_point_stats(self, ids, visible, found):
        for p, v, f in zip(ids, visible, found):
            if p >= 0 and p in self.recent:
                self.recent[p][2] += int(v)
                self.recent[p][1] += int(f)

    # ---- cullingMapPoints ----------------------------------------------------------------------------------------------
    def branch(self, p, current):
        first, found, visible = self.recent[p]
        if not self.observations(p):
            return DEAD
        if found_ratio_low(found, visible):
            return RATIO
        if current > first + 2 and self.obs(p) <= 3:
            return FEW_OBS
        if current > first + 3:
            return MATURED
        return KEPT

    def erase_map_point(self, p):
        for j, kf in enumerate(self.store):
            if not self.erased[j]:
                for i in range(len(kf["ids"])):
                    if kf["ids"][i] == p:
                        kf["flags"][i] &= ~1

    def cull_map_points(self, current):
        self.outcomes = {p: self.branch(p, current) for p in sorted(self.recent)}
        erased = [p for p, b in self.outcomes.items() if b in (RATIO, FEW_OBS)]
        for p in erased:
            self.erase_map_point(p)
        self.recent = {p: e for p, e in self.recent.items() if self.outcomes[p] == KEPT}
        cnt = [sum(1 for b in self.outcomes.values() if b == x) for x in range(6)]
        self._record(CULL, current, n_dead=cnt[DEAD], n_ratio=cnt[RATIO], n_few_obs=cnt[FEW_OBS], n_matured=cnt[MATURED], n_kept=cnt[KEPT],
                     n_erased=len(erased))
        self.up_erased = erased

    # ---- what the entry points return ----------------------------------------------------------------------------------
    def recent_points(self):
        return [(p, e[0], e[1], e[2]) for p, e in sorted(self.recent.items())]

    def upkeep_result(self):
        return dict(self.up_record, erased=list(self.up_erased))

    def state(self, k):
        return dict(super().state(k), point_desc=np.array(self.store[k]["pdesc"], np.uint8))
