"""Model of vo_tracker_build_local_map (test infrastructure): VisualOdometry::updateLocalKeyFrames + updateLocalMapPoints
(src/visualOdometry.cpp:595-724) restated over a key-frame store, in plain Python over dicts and lists.

A store is a list of key-frames in insertion order; key-frame k is a dict with
  ids, flags   per feature: map-point id, flags (bit 0: the map point exists and is not bad)
  bad          KeyFrame::isBad()
  neighbors    getBestCovisibleKFs(10) in its order (key-frame numbers)
  children     getChildren() in ascending key-frame number
  parent       key-frame number or -1
Key-frame k HOLDS id p when one of its features has ids == p and bit 0 set: the stand-in for MapPoint::getObservedKFs().

The four steps, as the contract in include/vo_hip.h states them:
 1 votes: every non-null slot gives one vote to every key-frame that holds its id; an id in two slots votes twice; a slot
   whose id no key-frame holds is nulled.
 2 voters in ascending key-frame number, bad ones skipped; best = the first with the strictly largest count; no voter: the
   local map is empty and best is -1.
 3 expansion over the original voters in order, stopping once the list holds more than 80: the first non-bad unmarked
   neighbour, the first non-bad unmarked child, the parent if unmarked and not bad.
 4 points: the list's key-frames in list order, their features in index order with bit 0 set, first occurrence of an id.
Capacities: the list keeps 84 entries (more voters: the first 84, `n_keyframes` the true count), the points max_local."""

MAX_KEYFRAMES = 84
STOP = 80


def holders(store, p):
    """key-frame numbers that hold id p, ascending"""
    out = []
    for k in range(len(store)):
        kf = store[k]
        for i in range(len(kf["ids"])):
            if kf["ids"][i] == p and (kf["flags"][i] & 1):
                out.append(k)
                break
    return out


def build_local_map(slots, store, max_local, ref_kf=None, failed=False):
    """slots: the frame's slot ids (-1: null).  ref_kf: the frame's reference key-frame on the reference-key-frame route
    (`link` is taken against it) or None after a relocalisation.  failed: VO_TRACK_RELOC_FAILED.
    -> dict(slots: after the nulling, keyframes: the list (at most 84), n_keyframes, best, points: [(key-frame, feature,
    id, link)] (at most max_local), n_points: the true distinct count, capacity: a bound was exceeded)"""
    slots = list(slots)
    if failed:
        return dict(slots=slots, keyframes=[], n_keyframes=0, best=-1, points=[], n_points=0, capacity=False)
    # 1. votes
    counter = {}
    for i in range(len(slots)):
        p = slots[i]
        if p < 0:
            continue
        hs = holders(store, p)
        if not hs:
            slots[i] = -1
            continue
        for k in hs:
            counter[k] = counter.get(k, 0) + 1
    # 2. voters
    voters, best, most = [], -1, 0
    for k in sorted(counter):
        if store[k]["bad"]:
            continue
        if counter[k] > most:
            most, best = counter[k], k
        voters.append(k)
    # 3. expansion
    lst = list(voters)
    marked = {}
    for k in voters:
        marked[k] = True
    for k in voters:
        if len(lst) > STOP:
            break
        kf = store[k]
        for kn in kf["neighbors"]:
            if store[kn]["bad"]:
                continue
            if kn not in marked:
                lst.append(kn)
                marked[kn] = True
                break
        for kc in kf["children"]:
            if store[kc]["bad"]:
                continue
            if kc not in marked:
                lst.append(kc)
                marked[kc] = True
                break
        kp = kf["parent"]
        if kp >= 0 and kp not in marked and not store[kp]["bad"]:
            lst.append(kp)
            marked[kp] = True
    capacity = len(lst) > MAX_KEYFRAMES
    n_keyframes = len(lst)
    lst = lst[:MAX_KEYFRAMES]
    # 4. points
    seen = {}
    points = []
    for k in lst:
        kf = store[k]
        for i in range(len(kf["ids"])):
            if not (kf["flags"][i] & 1):
                continue
            p = kf["ids"][i]
            if p in seen:
                continue
            seen[p] = True
            link = -1
            if ref_kf is not None and 0 <= ref_kf < len(store):
                r = store[ref_kf]
                for j in range(len(r["ids"])):
                    if r["ids"][j] == p and (r["flags"][j] & 1):
                        link = j
                        break
            points.append((k, i, p, link))
    n_points = len(points)
    capacity = capacity or n_points > max_local
    return dict(slots=slots, keyframes=lst, n_keyframes=n_keyframes, best=best, points=points[:max_local], n_points=n_points,
                capacity=capacity)
