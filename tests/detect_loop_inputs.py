"""Inputs of the loop-detection tests (test infrastructure): small hand-made worlds shared by the model's CPU tests
(tests/test_detect_loop_ref.py) and the device's GPU tests (tests/test_gpu_detect_loop.py), the runner of a script on the model,
and the loop scenes of tests/loop_sim3_inputs.py behind padding key-frames.

A world is K key-frames of at most NK = 16 features: who shares map points with whom (the covisibility weights, hence the
groups), and a synthetic BoW vector per key-frame put straight into the database.  The PLACES: a key-frame "at" place p carries
the four words of p; a current key-frame at p finds exactly the old key-frames at p.  Old key-frames carry the noise words of the
currents as well, so that an old key-frame at the current's place scores above the current's own neighbours (minScore).

A script is a list of steps: ("detect", current, last_loop_keyframe), ("bad", k), ("erase", k), ("lock", k, on), ("edge", a, b).
A hand case is dict(world, script, D, G, want): want holds, per detect step, (outcome, [(sorted members, count)], enough)."""
import numpy as np

import detect_loop_ref as dr

NK = 16
N_WORDS = 2048
K_HAND = 16
CURRENTS = (12, 13, 14, 15)
PLACE = dict(A=0, B=20, C=40, D=60, E=80)
AT = {2: "A", 4: "B", 6: "C", 8: "D", 9: "E"}      # the old key-frames at a place


def noise(k):
    return 1000 + k


class World:
    def __init__(self, K=K_HAND):
        self.K = K
        self.next = 5000
        self.store = [dict(ids=[], flags=[]) for _ in range(K)]
        self.bow = [dict() for _ in range(K)]
        self.update_order = list(range(K))

    def share(self, a, b, n=1):
        ids = list(range(self.next, self.next + n))
        self.next += n
        for k in (a, b):
            self.store[k]["ids"] += ids
            self.store[k]["flags"] += [1] * n
            assert len(self.store[k]["ids"]) <= NK
        return ids

    def words(self, k, vec):
        self.bow[k] = dict(vec)

    def vector(self, k):
        ws = sorted(self.bow[k])
        return np.array(ws, np.int32), np.array([self.bow[k][w] for w in ws], np.float64)


def at_places(places, weight):
    return {PLACE[p] + i: weight for p in places for i in range(4)}


def old_vector(place, currents=CURRENTS):
    """an old key-frame at `place`: 0.2 per place word, 0.03 per current's noise word"""
    v = at_places(place, 0.2)
    v.update({noise(c): 0.03 for c in currents})
    return v


def current_vector(k, places):
    """a current key-frame at one place (0.2 per word) or two (0.1 per word), and its own noise word; at no place: a word nobody
    else carries"""
    if not places:
        return {1900 + k: 1.0}
    v = at_places(places, 0.2 if len(places) == 1 else 0.1)
    v[noise(k)] = 0.2
    return v


def standard_world(currents_at, extra_shares=()):
    """key-frames 2, 4, 6, 8, 9 at the places A .. E with the groups {1,2,3}, {3,4,5}, {6,7}, {1,8,9}, {8,9}; the currents 12 .. 15
    at the places currents_at[k] (a string of place letters), connected to each other by one map point a pair"""
    w = World()
    for a, b in ((2, 1), (2, 3), (4, 3), (4, 5), (6, 7), (8, 1), (8, 9)) + tuple(extra_shares):
        w.share(a, b, 2)
    for i, a in enumerate(CURRENTS):
        for b in CURRENTS[i + 1:]:
            w.share(a, b, 1)
    for k in range(w.K):
        w.words(k, {noise(k): 1.0})
    for k, p in AT.items():
        w.words(k, old_vector(p))
    for k, places in currents_at.items():
        w.words(k, current_vector(k, places))
    return w


def min_score_world():
    """the current key-frame 12 with the ordered list [11, 10] (key-frame 11 holds one shared point twice: its update re-sorts 12's
    list over the whole map); scores against 12: key-frame 10 0.25, 11 0.9, the old key-frames 2 0.8 and 4 1.0"""
    w = World()
    for a, b in ((2, 1), (2, 3), (4, 3), (4, 5)):
        w.share(a, b, 2)
    w.share(12, 10, 3)
    ids = w.share(12, 11, 2)
    w.store[11]["ids"].append(ids[0]), w.store[11]["flags"].append(1)
    w.update_order = [12] + [k for k in range(w.K) if k != 12]
    for k in range(w.K):
        w.words(k, {noise(k): 1.0})
    A = PLACE["A"]
    w.words(12, {A + i: 0.25 for i in range(4)})
    w.words(2, {**{A + i: 0.2 for i in range(4)}, 500: 0.2})
    w.words(4, {A + i: 0.25 for i in range(4)})
    w.words(10, {A: 0.25, 501: 0.75})
    w.words(11, {**{A + i: 0.225 for i in range(4)}, 502: 0.1})
    return w


G123, G345, G67, G189 = [1, 2, 3], [3, 4, 5], [6, 7], [1, 8, 9]


def hand_cases():
    c = {}
    N, D_, NC, GT = dr.NOT_CONSISTENT, dr.DETECTED, dr.NO_CANDIDATES, dr.GATED

    def case(name, world, script, want, D=4, G=8):
        assert sum(1 for s in script if s[0] == "detect") == len(want)
        c[name] = dict(world=world, script=script, want=want, D=D, G=G)

    one_place = standard_world({k: "A" for k in CURRENTS})
    case("gate_at_last_plus_9_and_10", one_place, [("detect", 13, 0), ("detect", 12, 3), ("detect", 13, 3)],
         [(N, [(G123, 0)], []), (GT, [(G123, 0)], []), (N, [(G123, 1)], [])])
    case("no_candidates_clear_the_groups", standard_world({12: "A", 13: ""}), [("detect", 12, 0), ("detect", 13, 0)],
         [(N, [(G123, 0)], []), (NC, [], [])])
    case("one_candidate_four_calls", one_place, [("detect", k, 0) for k in CURRENTS],
         [(N, [(G123, 0)], []), (N, [(G123, 1)], []), (N, [(G123, 2)], []), (D_, [(G123, 3)], [2])])
    case("consistent_through_a_neighbour_only", standard_world({12: "A", 13: "B"}), [("detect", 12, 0), ("detect", 13, 0)],
         [(N, [(G123, 0)], []), (N, [(G345, 1)], [])])
    g3457 = [3, 4, 5, 7]
    case("one_candidate_two_previous_groups", standard_world({12: "AC", 13: "B"}, extra_shares=((4, 7),)), [("detect", 12, 0), ("detect", 13, 0)],
         [(N, [(G123, 0), (G67, 0)], []), (N, [(g3457, 1), (g3457, 1)], [])])
    case("two_candidates_one_previous_group", standard_world({12: "A", 13: "BD"}), [("detect", 12, 0), ("detect", 13, 0)],
         [(N, [(G123, 0)], []), (N, [(G345, 1)], [])])
    case("consistent_only_with_flagged_groups", standard_world({12: "A", 13: "A", 14: "A", 15: "AD"}), [("detect", k, 0) for k in CURRENTS],
         [(N, [(G123, 0)], []), (N, [(G123, 1)], []), (N, [(G123, 2)], []), (D_, [(G123, 3)], [2, 8])])
    case("bad_and_erased_members", one_place, [("detect", 12, 0), ("bad", 1), ("erase", 3), ("detect", 13, 0)],
         [(N, [(G123, 0)], []), (N, [([1, 2], 1)], [])])
    case("conn_skips_a_bad_neighbour", min_score_world(), [("detect", 12, 0), ("bad", 10), ("detect", 12, 0)],
         [(N, [(G123, 0), (G345, 0)], []), (N, [(G345, 1), (G345, 1)], [])])
    return c


HAND_CASES = ("gate_at_last_plus_9_and_10", "no_candidates_clear_the_groups", "one_candidate_four_calls", "consistent_through_a_neighbour_only",
              "one_candidate_two_previous_groups", "two_candidates_one_previous_group", "consistent_only_with_flagged_groups",
              "bad_and_erased_members", "conn_skips_a_bad_neighbour")


def overflow_world():
    """current 12 finds two candidates (2 and 6, disjoint groups); current 13 finds 4 (consistent with both groups: two pushes)
    and 9 (consistent with neither: a third)"""
    return standard_world({12: "AC", 13: "BE"}, extra_shares=((4, 7),))


def big_world():
    """130 key-frames, three bitset words with a ragged tail: the candidates 64 (group {63, 64, 127, 128, 129}) and 129 (group
    {0, 64, 128, 129}), both at the places A and C, as the currents 100 .. 103 are"""
    w = World(130)
    for b in (63, 127, 128, 129):
        w.share(64, b, 1)
    w.share(129, 128, 1), w.share(129, 0, 1)
    cur = (100, 101, 102, 103)
    for i, a in enumerate(cur):
        for b in cur[i + 1:]:
            w.share(a, b, 1)
    for k in range(w.K):
        w.words(k, {noise(k): 1.0})
    w.words(64, old_vector("AC", cur)), w.words(129, old_vector("AC", cur))   # (0.83 each against the currents' own 0.8)
    for k in cur:
        w.words(k, current_vector(k, "AC"))
    return w


# ---- the model side ---------------------------------------------------------------------------------------------------------------
def build_model(world, D, G):
    from cull_ref import CullModel
    from kfdb_ref import Database
    cull, db = CullModel(), Database()
    for k in range(world.K):
        cull.insert(world.store[k]["ids"], world.store[k]["flags"])
        db.insert(*world.vector(k))
    cull.update_connections(world.update_order)
    return dr.DetectModel(cull, db, D, G)


def model_step(m, s):
    if s[0] == "detect":
        m.detect_loop(s[1], s[2])
    elif s[0] == "bad":
        m.cull.set_bad(s[1])
    elif s[0] == "erase":
        m.cull.erase_keyframe(s[1])
    elif s[0] == "lock":
        m.cull.set_erase_lock(s[1], s[2])
    elif s[0] == "edge":
        m.add_loop_edge(s[1], s[2])
    else:
        raise ValueError(s)


def run_model(case):
    """-> (model, [(outcome, groups as sets, enough) per detect step])"""
    m = build_model(case["world"], case["D"], case["G"])
    got = []
    for s in case["script"]:
        model_step(m, s)
        if s[0] == "detect":
            got.append((m.record["outcome"], m.groups_as_sets(), m.result()["enough"]))
    return m, got


# ---- the loop scenes of tests/loop_sim3_inputs.py behind padding key-frames ----------------------------------------------------
PAD = 10


def padded_scene(sc, tail=0):
    """a loop scene (loop_sim3_inputs.scene / loop_merge_inputs.loop_scene) with PAD key-frames in front, so that its current
    key-frame passes detectLoop's gate, and `tail` behind: -> the scene with every key-frame number moved up by PAD, and `world`,
    the World (ids, flags, BoW vectors) of tests/detect_loop_ref.py's model -- vectors with which the scene's `current` finds
    exactly the scene's candidates, in their order, at a score of 1 against a minScore of 1 (`current` has no neighbour)"""
    f32 = np.float32
    pad = lambda: dict(ids=[-1], flags=[0], x=np.full(1, 320, f32), y=np.full(1, 240, f32), octave=np.zeros(1, np.int32),
                       angle=np.zeros(1, f32), uright=np.full(1, -1, f32), depth=np.full(1, -1, f32), desc=np.zeros((1, 32), np.uint8),
                       nodes=np.zeros(1, np.int32), points=np.zeros((1, 3)), point_desc=np.zeros((1, 32), np.uint8), min_dist=np.ones(1, f32),
                       max_dist=np.ones(1, f32), normals=np.zeros((1, 3)), pose=np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]), bad=False,
                       erased=False, seen=[])   # one feature without a map point; a pose, which the pose graph asks of every key-frame
    out = dict(sc, store=[pad() for _ in range(PAD)] + list(sc["store"]) + [pad() for _ in range(tail)], current=sc["current"] + PAD,
               cand=[c + PAD for c in sc["cand"]])
    w = World(len(out["store"]))
    w.store = [dict(ids=[int(i) for i in kf["ids"]], flags=[int(f) for f in kf["flags"]]) for kf in out["store"]]
    for k in range(w.K):
        w.words(k, {noise(k): 1.0})
    for k in [out["current"]] + out["cand"]:
        w.words(k, {PLACE["A"] + i: 0.25 for i in range(4)})
    out["world"] = w
    return out
