"""Inputs of the updateConnections tests (test infrastructure): the hand-made cases, shared by the model's CPU tests and
the device's GPU tests, and the synthetic stores of the GPU tests.

A case is dict(name, store, script, check): `store` a list of dict(ids, flags) (tests/local_map_ref.py's store), `script` a
list of steps -- ("update", [key-frame numbers]) or ("points", key-frame, ids, flags), the latter replacing the map side of a
key-frame -- and `check(snap)` ONE assertion on `snap`, a list with one entry per update step holding the state of every
key-frame behind that step (Connections.state / KeyFrameStore.connections: n_connected, weights, ordered, ordered_weights,
parent, children)."""
import numpy as np

K_HAND, NK_HAND = 12, 64


class _Builder:
    """K key-frames with two ids of their own each; share(a, b, n) gives a and b n fresh common ids"""

    def __init__(self, K=K_HAND):
        self.next = 1000
        self.store = [dict(ids=[], flags=[]) for _ in range(K)]
        for k in range(K):
            self.own(k, 2)

    def fresh(self, n):
        ids = list(range(self.next, self.next + n))
        self.next += n
        return ids

    def own(self, k, n):
        self.add(k, self.fresh(n))

    def add(self, k, ids, flag=1):
        self.store[k]["ids"] += ids
        self.store[k]["flags"] += [flag] * len(ids)
        assert len(self.store[k]["ids"]) <= NK_HAND

    def share(self, a, b, n):
        ids = self.fresh(n)
        self.add(a, ids)
        self.add(b, ids)
        return ids


def _cleared(kf):
    return list(kf["ids"]), [0] * len(kf["flags"])


def hand_cases():
    cases = []

    def case(name, b, script, check):
        cases.append(dict(name=name, store=b.store, script=script, check=check))

    b = _Builder()
    b.share(0, 1, 15), b.share(0, 2, 14)
    case("weight_15_connects_14_does_not", b, [("update", [0])],
         lambda s: (s[-1][0]["ordered"], s[-1][1]["weights"][0], s[-1][2]["n_connected"], s[-1][0]["weights"][2]) == ([1], 15, 0, 14))

    b = _Builder()
    b.share(3, 0, 5), b.share(3, 1, 7), b.share(3, 2, 7)
    case("nobody_reaches_15_single_maximum_tie_to_lowest", b, [("update", [3])],
         lambda s: (s[-1][3]["ordered"], s[-1][3]["ordered_weights"], s[-1][1]["weights"][3], s[-1][2]["n_connected"]) == ([1], [7], 7, 0))

    b = _Builder()
    b.share(0, 1, 16), b.share(0, 2, 16), b.share(0, 3, 20)
    case("equal_weights_in_descending_number", b, [("update", [0])],
         lambda s: (s[-1][0]["ordered"], s[-1][0]["ordered_weights"]) == ([3, 2, 1], [20, 16, 16]))

    b = _Builder()
    ids = b.share(0, 1, 15)
    b.add(1, ids[:1])   # the id a second time in key-frame 1: C[1][0] = 16, C[0][1] = 15
    b.share(0, 2, 5)
    case("neighbours_update_turns_the_list_into_the_whole_map", b, [("update", [0]), ("update", [1])],
         lambda s: (s[0][0]["ordered"], s[1][0]["ordered"], s[1][0]["ordered_weights"]) == ([1], [1, 2], [16, 5]))
    case("duplicated_id_makes_the_counts_asymmetric", b, [("update", [0]), ("update", [1])],
         lambda s: (s[0][0]["weights"][1], s[1][1]["weights"][0]) == (15, 16))

    b = _Builder()
    b.share(0, 1, 15), b.share(0, 2, 5)
    case("unchanged_weight_leaves_the_list_thresholded", b, [("update", [0]), ("update", [1])],
         lambda s: (s[1][0]["ordered"], s[1][0]["weights"][1], s[1][0]["weights"][2]) == ([1], 15, 5))

    b = _Builder()
    b.share(0, 1, 15), b.share(0, 2, 3)
    case("update_without_a_connection_changes_nothing", b, [("update", [0]), ("points", 0) + _cleared(b.store[0]), ("update", [0, 5])],
         lambda s: s[1] == s[0] and s[0][0]["ordered"] == [1] and s[0][0]["n_connected"] == 2)

    b = _Builder()
    b.share(1, 0, 15), b.share(1, 2, 20)
    case("parent_on_first_connection_only_never_for_key_frame_0", b,
         [("update", [1, 0]), ("points", 2) + _cleared(b.store[2]), ("update", [1])],
         lambda s: ([s[0][1]["parent"], s[0][0]["parent"]], s[1][1]["ordered"], [s[1][1]["parent"], s[1][0]["parent"]]) ==
         ([2, -1], [0], [2, -1]))

    b = _Builder()
    for k in (1, 2, 3):
        b.share(0, k, 15)
    case("children_ascending", b, [("update", [3, 1, 2])],
         lambda s: (s[-1][0]["children"], [s[-1][k]["parent"] for k in (1, 2, 3)]) == ([1, 2, 3], [0, 0, 0]))
    return cases


def run_model(store, script):
    """the script on the model -> (Connections, snap)"""
    from connections_ref import Connections
    store = [dict(ids=list(k["ids"]), flags=list(k["flags"])) for k in store]
    c = Connections()
    c.grow(len(store))
    snap = []
    for step in script:
        if step[0] == "points":
            store[step[1]] = dict(ids=list(step[2]), flags=list(step[3]))
        else:
            c.update_list(store, step[1])
            snap.append([c.state(k, len(store)) for k in range(len(store))])
    return c, snap


def sliding_window_store(rng, K, n_feat, span, step_lo, step_hi, p_dup=0.05, p_clear=0.1):
    """K key-frames of n_feat features whose ids come from a window of `span` ids that slides by step_lo .. step_hi - 1 per
    key-frame, so that adjacent key-frames share many ids and distant ones none; some ids twice in a key-frame, some
    features with bit 0 clear"""
    store = []
    start = 0
    for k in range(K):
        start += int(rng.integers(step_lo, step_hi))
        ids = start + rng.choice(span, n_feat, replace=False)
        ids = np.where(rng.random(n_feat) < p_dup, rng.choice(ids, n_feat), ids)
        flags = np.where(rng.random(n_feat) < p_clear, rng.choice(np.array([0, 2], np.uint8), n_feat), rng.choice(np.array([1, 3], np.uint8), n_feat))
        store.append(dict(ids=[int(x) for x in ids], flags=[int(x) for x in flags]))
    return store


def device_arrays(kf, rng=None):
    """the arrays KeyFrameStore.insert takes for a model key-frame (everything but ids and flags is filler)"""
    n = len(kf["ids"])
    return dict(angle=np.zeros(n, np.float32), desc=np.zeros((n, 32), np.uint8), nodes=np.zeros(n, np.int32),
                flags=np.asarray(kf["flags"], np.uint8), points=np.zeros((n, 3)) if rng is None else rng.normal(0, 2, (n, 3)),
                ids=np.asarray(kf["ids"], np.int32), point_desc=np.zeros((n, 32), np.uint8), min_dist=np.full(n, 0.5, np.float32),
                max_dist=np.full(n, 9.0, np.float32))
