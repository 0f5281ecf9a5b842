"""Inputs of the key-frame culling tests (test infrastructure): the script format, its runner on the model
(tests/cull_ref.py), the hand-made cases a .. l shared by the model's CPU tests and the device's GPU tests, and the seeded
random sequence of the GPU test.

A script is a list of steps:
  ("insert", ids, flags, octave, depth, u_right)   a key-frame with its key-point columns
  ("update", [key-frame numbers])                  update_connections
  ("points", key-frame, ids, flags)                update_points
  ("bad", key-frame)                               set_bad
  ("lock", key-frame, on)                          set_erase_lock
  ("cull", current, th_depth)                      cull_keyframes
  ("erase", key-frame)                             erase_keyframe
snapshot(x) after a cull or erase step is dict(result, state [K], connections [K], flags [K]) of the model or the device
store; a case is dict(name, script, check): check(snaps) ONE assertion on the list of snapshots, its right-hand side worked
out by hand."""
import numpy as np

from cull_ref import CullModel

NK_HAND = 128
TH = 5.0


def snapshot(x, size):
    """x: a CullModel, or anything with cull_result / cull_state / connections / flags of the same shapes"""
    return dict(result=x.cull_result(), state=[x.cull_state(k) for k in range(size)],
                connections=[x.connections(k) for k in range(size)], flags=[x.flags_of(k) for k in range(size)])


class ModelRunner:
    """the script's steps on the model, under the names snapshot() uses"""

    def __init__(self):
        self.m = CullModel()

    def step(self, s):
        m = self.m
        if s[0] == "insert":
            k = m.insert(s[1], s[2])
            m.set_keypoints(k, s[3], s[4], s[5])
        elif s[0] == "update":
            m.update_connections(s[1])
        elif s[0] == "points":
            m.update_points(s[1], s[2], s[3])
        elif s[0] == "bad":
            m.set_bad(s[1])
        elif s[0] == "lock":
            m.set_erase_lock(s[1], s[2])
        elif s[0] == "cull":
            m.cull(s[1], s[2])
        elif s[0] == "erase":
            m.erase_keyframe(s[1])   # (the record of the last cull call stays)
        else:
            raise ValueError(s[0])
        return s[0] in ("cull", "erase")

    def __len__(self):
        return len(self.m.store)

    def cull_result(self):
        return list(self.m.result)

    def cull_state(self, k):
        return self.m.state(k)

    def connections(self, k):
        return self.m.connections(k)

    def flags_of(self, k):
        return self.m.flags(k)


def run(runner, script):
    """-> the snapshots behind every cull and erase step"""
    snaps = []
    for s in script:
        if runner.step(s):
            snaps.append(snapshot(runner, len(runner)))
    return snaps


def run_model(script):
    r = ModelRunner()
    return r.m, run(r, script)


class _Builder:
    """K key-frames; see(p-count, key-frames, ...) gives them fresh common ids, one feature each"""

    def __init__(self, K):
        self.next = 1000
        self.kf = [dict(ids=[], flags=[], octave=[], depth=[], u_right=[]) for _ in range(K)]

    def feature(self, k, p, octave=0, depth=1.0, u_right=-1.0, flag=1):
        f = self.kf[k]
        f["ids"].append(p), f["flags"].append(flag), f["octave"].append(octave), f["depth"].append(depth), f["u_right"].append(u_right)
        assert len(f["ids"]) <= NK_HAND
        return len(f["ids"]) - 1

    def see(self, n, kfs, octave=None, depth=None, u_right=None):
        """n fresh ids, each observed by every key-frame of kfs; octave / depth / u_right: {key-frame: value} overrides"""
        ids = list(range(self.next, self.next + n))
        self.next += n
        for p in ids:
            for k in kfs:
                self.feature(k, p, (octave or {}).get(k, 0), (depth or {}).get(k, 1.0), (u_right or {}).get(k, -1.0))
        return ids

    def filler(self, a, b, n=15):
        """a and b connected with weight n through points that count for nothing: no depth in either"""
        return self.see(n, [a, b], depth={a: -1.0, b: -1.0})

    def grow(self):
        """the reference's order: every key-frame inserted, then updated on its own"""
        script = []
        for k, f in enumerate(self.kf):
            script.append(("insert", list(f["ids"]), list(f["flags"]), list(f["octave"]), list(f["depth"]), list(f["u_right"])))
        for k in range(len(self.kf)):
            script.append(("update", [k]))
        return script

    def grow_in_turn(self):
        """insert k, update k, insert k + 1, ...: a key-frame's parent comes from the key-frames before it"""
        script = []
        for k, f in enumerate(self.kf):
            script.append(("insert", list(f["ids"]), list(f["flags"]), list(f["octave"]), list(f["depth"]), list(f["u_right"])))
            script.append(("update", [k]))
        return script


def _five():
    """key-frames 0 .. 4 that all see the same 20 points: a chain 0 <- 1 <- 2 <- 3 <- 4, every weight 20"""
    b = _Builder(5)
    b.see(20, [0, 1, 2, 3, 4])
    return b


def _two_candidates(n1, n2, extra1=0, extra2=0, octave=None):
    """0: the root; candidates 1 and 2 with n1 / n2 points that 3, 4, 5 see too, and extra1 / extra2 points of their own;
    6: the current key-frame, connected to both with weight 15 through fillers (its list: [2, 1])"""
    b = _Builder(7)
    b.see(n1, [1, 3, 4, 5], octave=octave)
    b.see(n2, [2, 3, 4, 5], octave=octave)
    b.see(extra1, [1]), b.see(extra2, [2])
    b.filler(6, 1), b.filler(6, 2)
    return b


def hand_cases():
    cases = []

    def case(name, script, check):
        cases.append(dict(name=name, script=script, check=check))

    res = lambda s: s["result"]
    par = lambda s, ks: [s["connections"][k]["parent"] for k in ks]

    # a, f, l: candidates 3, 2, 1, 0 of key-frame 4.  3: every point has the observers 0, 1, 2, 4 -> erased.  2: holders 0, 1, 2,
    # 4, obs 4 > 3, observers 0, 1, 4 -> erased.  1: holders 0, 1, 4, obs 3 -> nothing redundant.  0: never.
    b = _five()
    case("a_fully_redundant_is_erased", b.grow_in_turn() + [("cull", 4, TH)],
         lambda s: (res(s[0])[0], s[0]["state"][3]["erased"], s[0]["flags"][3][1], s[0]["connections"][3]["ordered"]) == ((3, 20, 20, 1), 1, 1, []))
    case("f_redundant_through_each_other_first_in_list_goes", b.grow_in_turn() + [("cull", 4, TH)],
         lambda s: res(s[0]) == [(3, 20, 20, 1), (2, 20, 20, 1), (1, 20, 0, 0), (0, 0, 0, 3)])
    case("l_candidate_list_is_the_snapshot", b.grow_in_turn() + [("cull", 4, TH)],
         lambda s: ([r[0] for r in res(s[0])], s[0]["connections"][4]["ordered"], par(s[0], [4, 3, 2])) == ([3, 2, 1, 0], [1, 0], [1, 2, 1]))

    # b: 2 has 11 counted points, 10 redundant: 10 > 9.9; 1 has 10 counted, 9 redundant: 9 > 9.0 is false
    b = _two_candidates(9, 10, 1, 1)
    case("b_nine_of_ten_kept_ten_of_eleven_erased", b.grow_in_turn() + [("cull", 6, TH)],
         lambda s: res(s[0]) == [(2, 11, 10, 1), (1, 10, 9, 0)])

    # c: the candidates' features at octave 2; observers 3, 4 at octave 3 (level + 1); observer 5 at octave 3 for the points of 1
    # and at octave 4 (level + 2) for the points of 2
    b = _Builder(7)
    b.see(10, [1, 3, 4, 5], octave={1: 2, 3: 3, 4: 3, 5: 3})
    b.see(10, [2, 3, 4, 5], octave={2: 2, 3: 3, 4: 3, 5: 4})
    b.filler(6, 1), b.filler(6, 2)
    case("c_octave_level_plus_one_counts_plus_two_does_not", b.grow_in_turn() + [("cull", 6, TH)],
         lambda s: res(s[0]) == [(2, 10, 0, 0), (1, 10, 10, 1)])

    # d: 12 redundant points of candidate 1: 4 at depth -0.5, 4 at 7.5 > th, 3 at th itself (counted), 1 at 1.0; and one counted
    # point of its own: mp_cnt 5, re_obs 4 -> kept (without the gates: 12 of 13, erased)
    b = _Builder(7)
    for n, d in ((4, -0.5), (4, 7.5), (3, TH), (1, 1.0)):
        b.see(n, [1, 3, 4, 5], depth={1: d})
    b.see(1, [1])
    b.filler(6, 1)
    case("d_depth_gate_both_sides_and_the_threshold_itself", b.grow_in_turn() + [("cull", 6, TH)],
         lambda s: res(s[0]) == [(1, 5, 4, 0)])

    # e: candidate 1 is erased (10 redundant points).  Its further points, without depth in 1: pA with 5 (stereo): 2 left, dies;
    # pB with 5 (stereo) and 6 (mono): 3 left, lives; pC with 5 and 6 (both mono): 2 left, dies
    b = _Builder(8)
    b.see(10, [1, 2, 3, 4])
    pa = b.see(1, [1, 5], depth={1: -1.0}, u_right={5: 30.0})
    pb = b.see(1, [1, 5, 6], depth={1: -1.0}, u_right={5: 30.0})
    pc = b.see(1, [1, 5, 6], depth={1: -1.0})
    b.filler(7, 1, 20)
    case("e_stereo_observation_counts_two_mono_one", b.grow_in_turn() + [("cull", 7, TH)],
         lambda s: (res(s[0]), s[0]["flags"][5][0], s[0]["flags"][6][0]) == ([(1, 10, 10, 1)], [0, 1, 0], [1, 0]))

    # g: 2 goes first (10 of 11).  Its 11th point q is held by 2 and 1 alone and dies with 2; 1 had 9 of 10 (kept) and has 9 of 9
    b = _Builder(7)
    b.see(9, [1, 3, 4, 5])
    b.see(10, [2, 3, 4, 5])
    b.see(1, [1, 2])
    b.filler(6, 1), b.filler(6, 2)
    case("g_point_death_flips_a_later_decision", b.grow_in_turn() + [("cull", 6, TH)],
         lambda s: res(s[0]) == [(2, 11, 10, 1), (1, 9, 9, 1)])

    # h: 0 <- 1 <- 2 (erased); children of 2: 3 and 4 (weight 16 to 1 each: the tie goes to 3), then 4 (16 to 1 and to 3: the tie
    # goes to the first of its list, 3), 5 (no connection to a candidate: gets 1), 6 (bad: skipped, gets 1)
    b = _Builder(7)
    b.see(20, [0, 1]), b.see(20, [1, 2])
    for c in (3, 4, 5, 6):
        b.see(20, [2, c])
    b.see(16, [3, 1]), b.see(16, [4, 1]), b.see(16, [4, 3]), b.see(17, [6, 1])
    case("h_reparenting_ties_no_candidate_and_a_bad_child", b.grow_in_turn() + [("bad", 6), ("erase", 2)],
         lambda s: (par(s[0], [1, 2, 3, 4, 5, 6]), s[0]["connections"][1]["children"], s[0]["connections"][3]["children"],
                    s[0]["connections"][2]["children"]) == ([0, 1, 1, 3, 1, 1], [3, 5, 6], [4], []))

    # h (no parent): 1 is never updated, 2's first update makes 1 its parent; erasing 1 leaves 2 without one
    b = _Builder(3)
    b.see(20, [1, 2])
    ins = b.grow()[:3]
    case("h_erased_key_frame_without_a_parent", ins + [("update", [2]), ("erase", 1)],
         lambda s: (par(s[0], [1, 2]), s[0]["connections"][1]["children"], s[0]["state"][1]["erased"], s[0]["connections"][2]["weights"]) ==
         ([-1, -1], [], 1, [0, 0, 0]))

    # i: 2 and 1 share 15; then 2's points change to share 15 with 3 instead and 2 is updated again: W[2] = {3}, W[1][2] stays
    b = _Builder(4)
    b.see(15, [1, 2])
    with3 = list(range(5000, 5015))
    for p in with3:
        b.feature(3, p)
    script = b.grow_in_turn() + [("points", 2, with3, [1] * 15), ("update", [2]), ("erase", 2)]
    case("i_quirk_e1_one_sided_connection_survives", script,
         lambda s: (s[0]["connections"][1]["weights"][2], s[0]["connections"][1]["ordered"], s[0]["connections"][3]["weights"][2],
                    s[0]["connections"][2]["n_connected"]) == (15, [2], 0, 0))

    # j: as a, with 3 locked: 3 pending; 2: observers 0, 1, 3, 4 -> erased; 1: holders 0, 1, 3, 4, observers 0, 3, 4 -> erased.
    # Then the lock comes off and the caller erases 3
    b = _five()
    case("j_lock_and_pending", b.grow_in_turn() + [("lock", 3, 1), ("cull", 4, TH), ("lock", 3, 0), ("erase", 3)],
         lambda s: (res(s[0]), s[0]["state"][3], s[1]["state"][3], s[1]["flags"][3][1]) ==
         ([(3, 20, 20, 2), (2, 20, 20, 1), (1, 20, 20, 1), (0, 0, 0, 3)], dict(erased=0, locked=1, pending=1),
          dict(erased=1, locked=0, pending=1), 1))

    # k: as a, with 2 bad: 3: observers 0, 1, 4 -> erased; 2 skipped; 1: holders 0, 1, 2, 4 (obs 4), observers 0, 4 -> kept; 0 skipped
    b = _five()
    case("k_key_frame_0_and_bad_candidates_are_skipped", b.grow_in_turn() + [("bad", 2), ("cull", 4, TH)],
         lambda s: res(s[0]) == [(3, 20, 20, 1), (2, 0, 0, 3), (1, 20, 0, 0), (0, 0, 0, 3)])
    return cases


# ---- the seeded random sequence of the GPU test ------------------------------------------------------------------------------
def random_keyframe(rng, n_feat, level, p_clear=0.08, p_dup=0.04):
    """n_feat features with ids from the pool [0, len(level)): a point's octave is its level[id] -1 / +0 / +1 (within 0 .. 7), so
    that most observers pass the octave gate and some do not; depths with -1 and values beyond TH; a third stereo"""
    ids = rng.choice(len(level), n_feat, replace=False)
    ids = np.where(rng.random(n_feat) < p_dup, rng.choice(ids, n_feat), ids)
    flags = np.where(rng.random(n_feat) < p_clear, 2, rng.choice(np.array([1, 3]), n_feat))
    octave = np.clip(level[ids] + rng.integers(-1, 2, n_feat), 0, 7)
    depth = np.where(rng.random(n_feat) < 0.1, -1.0, np.where(rng.random(n_feat) < 0.1, TH + 2.5, rng.uniform(0.5, TH, n_feat))).astype(np.float32)
    u_right = np.where(rng.random(n_feat) < 0.35, rng.uniform(1, 600, n_feat), -1.0).astype(np.float32)
    return ("insert", [int(x) for x in ids], [int(x) for x in flags], [int(x) for x in octave], [float(x) for x in depth],
            [float(x) for x in u_right])


def random_script(seed, K=12, pool=80):
    """K key-frames of 48 .. 64 features with ids from a pool of `pool`, grown in turn with a cull after every insert from the
    fifth on, one set_bad, one lock, one update_points and one explicit erase"""
    rng = np.random.default_rng(seed)
    level = rng.integers(0, 8, pool)
    script = []
    for k in range(K):
        script.append(random_keyframe(rng, int(rng.integers(48, 65)), level))
        script.append(("update", [k]))
        if k == 6:
            script.append(("lock", 3, 1))
        if k == 8:
            script.append(("bad", 5))
        if k >= 4:
            script.append(("cull", k, TH))
            script.append(("update", [int(x) for x in rng.permutation(k + 1)[:4]]))
        if k == 9:
            script += [("lock", 3, 0), ("erase", 3), ("erase", 7)]
    script.append(("cull", K - 1, TH))
    return script


SEED = 147   # chosen on the CPU (tests/test_cull_ref.py checks it): the model meets assert_not_vacuous on this sequence


def assert_not_vacuous(m):
    """the conditions on the MODEL's run of the random sequence under which the device comparison means something"""
    culls = [e for kind, e in m.log["calls"] if kind == "cull"]
    assert sum(1 for e in culls if e) >= 3                       # three cull calls erase something
    assert any(len(e) >= 2 for e in culls)                        # one erases two: the recount path
    assert m.log["dead_points"] >= 1                              # a point dies
    assert any(x != gp for _, x, gp in m.log["reparented"])       # a re-parenting picks somebody other than the grandparent
    assert any(m.pending) and any(kind == "erase" and e for kind, e in m.log["calls"])
