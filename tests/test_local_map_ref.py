"""The model of vo_tracker_build_local_map (tests/local_map_ref.py) against a second, independently written formulation
(numpy, set-based, no shared helpers) on random small graphs, hand-made cases for every rule of the contract, and the ABI
of the new entry points."""
import pathlib
import re
import subprocess

import numpy as np
import pytest

from local_map_ref import build_local_map

ROOT = pathlib.Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("vo_kfstore_set_graph", "vo_kfstore_set_graph_batch", "vo_kfstore_set_normals", "vo_tracker_build_local_map")


def kf(ids, flags=None, bad=False, neighbors=(), children=(), parent=-1):
    return dict(ids=list(ids), flags=[1] * len(ids) if flags is None else list(flags), bad=bad, neighbors=list(neighbors),
                children=list(children), parent=parent)


# ---- the second formulation: arrays and sets -------------------------------------------------------------------------
def second(slots, store, max_local, ref_kf=None, failed=False):
    slots = np.array(slots, np.int64)
    empty = dict(slots=slots.tolist(), keyframes=[], n_keyframes=0, best=-1, points=[], n_points=0, capacity=False)
    if failed:
        return empty
    K = len(store)
    nf = max([len(k["ids"]) for k in store] + [1])
    ids = np.full((K, nf), -1, np.int64)
    ok = np.zeros((K, nf), bool)
    for k, s in enumerate(store):
        ids[k, :len(s["ids"])] = s["ids"]
        ok[k, :len(s["ids"])] = (np.array(s["flags"], np.int64) & 1) == 1
    bad = np.array([s["bad"] for s in store], bool)
    held = [set(ids[k][ok[k]].tolist()) for k in range(K)]
    everything = set().union(*held) if held else set()
    orphan = np.array([p >= 0 and p not in everything for p in slots.tolist()], bool)
    slots[orphan] = -1
    live = slots[slots >= 0]
    votes = np.array([sum(int((live == p).sum()) for p in held[k]) for k in range(K)], np.int64)
    voters = np.nonzero((votes > 0) & ~bad)[0]
    out = dict(empty, slots=slots.tolist())
    best = -1 if len(voters) == 0 else int(voters[np.argmax(votes[voters])])   # argmax: the first of equal maxima
    out["best"] = best
    chosen = set(voters.tolist())
    order = voters.tolist()
    for k in voters.tolist():
        if len(order) > 80:
            break
        s = store[k]
        picks = [[c for c in s["neighbors"] if not bad[c]], [c for c in s["children"] if not bad[c]],
                 [s["parent"]] if s["parent"] >= 0 and not bad[s["parent"]] else []]
        for cands in picks:
            fresh = [c for c in cands if c not in chosen]
            if fresh:
                order.append(fresh[0])
                chosen.add(fresh[0])
    out["n_keyframes"] = len(order)
    order = order[:84]
    out["keyframes"] = order
    if order:
        kk = np.concatenate([np.full(int(ok[k].sum()), k) for k in order])
        ii = np.concatenate([np.nonzero(ok[k])[0] for k in order])
        pp = ids[kk, ii] if len(kk) else np.zeros(0, np.int64)
        _, firsts = np.unique(pp, return_index=True)
        firsts.sort()
        link = np.full(len(firsts), -1, np.int64)
        if ref_kf is not None and 0 <= ref_kf < K:
            for n, p in enumerate(pp[firsts]):
                at = np.nonzero(ok[ref_kf] & (ids[ref_kf] == p))[0]
                link[n] = at[0] if len(at) else -1
        pts = [(int(kk[j]), int(ii[j]), int(pp[j]), int(link[n])) for n, j in enumerate(firsts)]
        out["n_points"] = len(pts)
        out["points"] = pts[:max_local]
    out["capacity"] = out["n_keyframes"] > 84 or out["n_points"] > max_local
    return out


def random_case(rng, big=False):
    K = int(rng.integers(1, 120 if big else 14))
    pool = int(rng.integers(4, 60))
    store = []
    for k in range(K):
        n = int(rng.integers(0, 9))
        others = [c for c in range(K) if c != k]
        pick = lambda m: [int(c) for c in rng.permutation(others)[:int(rng.integers(0, m + 1))]]
        store.append(kf(rng.integers(0, pool, n).tolist(), rng.integers(0, 4, n).tolist(), bool(rng.random() < 0.15), pick(10), sorted(pick(5)),
                        int(rng.choice(others)) if others and rng.random() < 0.6 else -1))
    slots = [int(p) if rng.random() < 0.8 else -1 for p in rng.integers(0, pool + 5, int(rng.integers(0, 40)))]
    return slots, store, int(rng.integers(1, 30)), (int(rng.integers(0, K)) if rng.random() < 0.5 else None)


@pytest.mark.parametrize("seed", range(8))
def test_model_against_the_set_formulation(seed):
    rng = np.random.default_rng(seed)
    for n in range(40):
        slots, store, max_local, ref = random_case(rng, big=(n % 8 == 7))
        assert build_local_map(slots, store, max_local, ref) == second(slots, store, max_local, ref)


def test_tie_for_best_takes_the_lowest_number():
    store = [kf([7]), kf([1, 2]), kf([1, 2]), kf([1])]
    r = build_local_map([1, 2], store, 10)
    assert r["best"] == 1 and r["keyframes"] == [1, 2, 3]
    assert second([1, 2], store, 10)["best"] == 1


def test_bad_voter_bad_neighbour_bad_parent():
    store = [kf([1], neighbors=[1, 2], parent=3), kf([9], bad=True), kf([9]), kf([9], bad=True), kf([1, 1, 1], bad=True)]
    r = build_local_map([1, 1], store, 10)
    # key-frame 4 holds the id (it still collects votes) but is bad: no voter, not the best; neighbour 1 is bad -> 2; parent 3 is bad
    assert r["keyframes"] == [0, 2] and r["best"] == 0 and r["slots"] == [1, 1]
    assert [p[:3] for p in r["points"]] == [(0, 0, 1), (2, 0, 9)]


def test_a_marked_neighbour_is_passed_over():
    store = [kf([1], neighbors=[1, 2]), kf([1], neighbors=[0, 2]), kf([5]), kf([6])]
    r = build_local_map([1], store, 10)
    assert r["keyframes"] == [0, 1, 2]   # voter 0 takes 2 (1 is a voter); voter 1 finds 0 and 2 marked
    store[1]["children"] = [2, 3]
    assert build_local_map([1], store, 10)["keyframes"] == [0, 1, 2, 3]


def test_the_stop_beyond_80():
    # 79 voters, every one with three fresh links: voter 0 -> 82 entries, which is more than 80: stop
    K = 79
    store = [kf([k], neighbors=[K + 3 * k], children=[K + 3 * k + 1], parent=K + 3 * k + 2) for k in range(K)]
    store += [kf([1000 + j]) for j in range(3 * K)]
    r = build_local_map(list(range(K)), store, 1000)
    assert r["keyframes"] == list(range(K)) + [K, K + 1, K + 2] and not r["capacity"]
    # 80 voters: 80 is not more than 80, voter 0 expands to 83 -- the most a list reaches by expansion
    store80 = [kf([k], neighbors=[80 + 3 * k], children=[81 + 3 * k], parent=82 + 3 * k) for k in range(80)] + [kf([2000 + j]) for j in range(240)]
    assert build_local_map(list(range(80)), store80, 1000)["n_keyframes"] == 83
    # 82 voters: no expansion at all; 90 voters: the first 84 kept, the true count reported
    for nv, kept in ((82, 82), (90, 84)):
        st = [kf([k], neighbors=[nv]) for k in range(nv)] + [kf([5000])]
        r = build_local_map(list(range(nv)), st, 1000)
        assert r["keyframes"] == list(range(kept)) and r["n_keyframes"] == nv and r["capacity"] == (nv > 84)
        assert second(list(range(nv)), st, 1000) == r


def test_an_id_in_two_slots_votes_twice():
    store = [kf([1, 2, 3]), kf([4])]
    assert build_local_map([1, 2, 3], store, 10)["best"] == 0
    assert build_local_map([1, 2, 3, 4, 4, 4, 4], store, 10)["best"] == 1


def test_an_orphan_id_nulls_its_slot_and_unflagged_features_hold_nothing():
    store = [kf([1, 2], flags=[1, 2])]   # id 2 sits on a feature without bit 0
    r = build_local_map([2, 1, 77, -1], store, 10)
    assert r["slots"] == [-1, 1, -1, -1] and r["keyframes"] == [0] and [p[2] for p in r["points"]] == [1]


def test_no_voters_and_failed_frames_get_an_empty_map():
    store = [kf([1], bad=True), kf([2])]
    for r in (build_local_map([1], store, 10), build_local_map([-1, -1], store, 10), build_local_map([2], store, 10, failed=True)):
        assert r["keyframes"] == [] and r["best"] == -1 and r["points"] == [] and r["n_points"] == 0


def test_first_occurrence_link_and_the_point_capacity():
    store = [kf([5, 6, 5]), kf([6, 7, 8], flags=[1, 3, 1]), kf([8, 5])]
    r = build_local_map([5, 7], store, 3, ref_kf=2)
    assert r["keyframes"] == [0, 1, 2] and r["n_points"] == 4 and r["capacity"]
    assert r["points"] == [(0, 0, 5, 1), (0, 1, 6, -1), (1, 1, 7, -1)]


# ---- the ABI of the new entry points (fails on the parent commit) ------------------------------------------------------
def test_header_declares_and_library_exports_the_new_symbols(vo):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "vo_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(vo_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", str(vo.SO)], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (vo_[a-z0-9_]+)", out))
    for s in NEW_SYMBOLS:
        assert s in declared and s in exported and s in vo.SYMBOLS and hasattr(vo.lib(), s), s
    full = (ROOT / "include" / "vo_hip.h").read_text()
    for name, value in (("VO_TRACKER_LOCAL_KEYFRAMES", 23), ("VO_TRACKER_LOCAL_N_KEYFRAMES", 24), ("VO_TRACKER_LOCAL_N_POINTS", 25),
                        ("VO_TRACKER_LOCAL_REF_KF", 26), ("VO_TRACKER_LOCAL_POINT_IDS", 27)):
        assert re.search(rf"\b{name} = {value}\b", full), name
        assert getattr(vo.Tracker, name[len("VO_TRACKER_"):]) == value
    assert vo.Tracker.LOCAL_MAX_KEYFRAMES == int(re.search(r"#define VO_TRACKER_LOCAL_MAX_KEYFRAMES (\d+)", full).group(1)) == 84
    assert vo.KeyFrameStore.MAX_CHILDREN == int(re.search(r"#define VO_KFSTORE_MAX_CHILDREN (\d+)", full).group(1))
