"""Inputs of the key-frame creation tests (test infrastructure): the vocabulary and its descent, the 6-key-frame store of the
holder rules, the hand-made depth tables that hit every rule of the walk (include/vo_hip.h, step 2), seeded random frames and
the seeded 5 x 256 chain.  Shared by tests/test_keyframe_create_ref.py (the model against a pointer transcription) and
tests/test_gpu_keyframe_create.py (the device against the model).

A frame is the dict KeyFrameStore.create_keyframe takes: Tcw12, x, y, octave, angle, depth, u_right, desc, slot_ids."""
import numpy as np

import new_points_inputs as ni
from vo_slam_test_amd import synth

f32 = np.float32
NK = 256
TH = f32(3.0)                     # th_depth of the tables
CAM6, SF, FIRST_ID = ni.CAM6, ni.SF, ni.FIRST_ID
CAPS = (16, 4096, 32768)
MAX_RECENT = 4096
_POP = np.array([bin(x).count("1") for x in range(256)], np.int32)


def vocabulary():
    return synth.make_vocabulary(3, k=8, L=4)


def node_of(vd, desc, levelsup=3):
    """DBoW3's descent per descriptor (the first of equal minima wins) -> the node at level L - levelsup"""
    cs, ch, nd, wid = vd["child_start"], vd["children"], np.asarray(vd["node_desc"], np.uint8), vd["word_id"]
    out = []
    for d in np.asarray(desc, np.uint8).reshape(-1, 32):
        node, level, nid = 0, 0, 0
        while wid[node] < 0 and cs[node + 1] > cs[node]:
            level += 1
            kids = ch[cs[node]:cs[node + 1]]
            node = int(kids[int(np.argmin(_POP[nd[kids] ^ d].sum(1)))])
            if level == vd["L"] - levelsup:
                nid = node
        out.append(nid)
    return out


# ---- the store of the holder rules ------------------------------------------------------------------------------------------
# six key-frames of 24 features; key-frame 2 is erased and key-frame 4 bad before the frame comes in.
#   ids 0 .. 11   held by the key-frames 0, 1, 3 and 5 (tracked)          id 40   held by key-frame 2 alone (erased: null)
#   id 41         held by the key-frames 2, 3, 4 and 5 (first observation: 3) id 42   held by the bad key-frame 4 alone (tracked)
#   id 43         carried by key-frame 1 with bit 0 clear (not held: null) id 44   twice in key-frame 0 (observation: the lower feature)
#   id 45         held by key-frame 0 only through its SECOND feature (the first has bit 0 clear)
HELD, ERASED_ONLY, ERASED_AND_3, BAD_ONLY, UNFLAGGED, TWICE, SECOND, NOBODY = list(range(12)), 40, 41, 42, 43, 44, 45, 77


def holder_store(seed=2):
    rng = np.random.default_rng(seed)
    rows = {k: [] for k in range(6)}     # (id, flag)
    for k in (0, 1, 3, 5):
        rows[k] += [(p, 1) for p in HELD]
    rows[2] += [(ERASED_ONLY, 1), (ERASED_AND_3, 1)] + [(p, 1) for p in range(20, 36)]
    rows[3] += [(ERASED_AND_3, 3)]
    rows[4] += [(BAD_ONLY, 1), (ERASED_AND_3, 1)] + [(p, 1) for p in range(20, 36)]
    rows[5] += [(ERASED_AND_3, 1)]
    rows[1] += [(UNFLAGGED, 2)]
    rows[0] += [(TWICE, 1), (TWICE, 1), (SECOND, 0), (SECOND, 1)]
    script = []
    for k in range(6):
        r = rows[k] + [(-1, 0)] * (24 - len(rows[k]))
        n = len(r)
        stereo = rng.random(n) < 0.5
        depth = np.where(stereo, rng.uniform(1, 6, n), -1.0).astype(f32)
        ur = np.where(stereo, rng.uniform(10, 600, n), -1.0).astype(f32)
        pts = rng.uniform(-2, 8, (n, 3))
        script.append(("insert", [p for p, _ in r], [f for _, f in r], [int(x) for x in rng.integers(0, 8, n)], list(depth), list(ur),
                       dict(desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), angle=list(rng.uniform(0, 360, n).astype(f32)),
                            nodes=[int(x) for x in rng.integers(0, 8, n)], points=pts, refs=[k if p >= 0 else -1 for p, _ in r])))
        script.append(("pose", k, ni.se3(rng.normal(0, 0.05, 3), rng.uniform(-1, 1, 3))))
        script.append(("xy", k, rng.uniform(0, 640, (n, 2)).astype(f32)))
    return script + [("erase", 2), ("bad", 4)]


# ---- frames -----------------------------------------------------------------------------------------------------------------
def frame(rng, depth, slot_ids):
    """a frame around the given depth and slot columns: a pose a few degrees and a metre off the origin, key-points over the image"""
    n = len(depth)
    depth = np.asarray(depth, f32)
    x, y = rng.uniform(0, 640, n).astype(f32), rng.uniform(0, 480, n).astype(f32)
    with np.errstate(all="ignore"):
        ur = np.where(depth > 0, x - f32(40.0) / depth, f32(-1.0)).astype(f32)
    return dict(Tcw12=np.array(ni.se3(rng.normal(0, 0.05, 3), rng.uniform(-1, 1, 3))), x=x, y=y,
                octave=rng.integers(0, 8, n).astype(np.int32), angle=rng.uniform(0, 360, n).astype(f32), depth=depth, u_right=ur,
                desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), slot_ids=np.asarray(slot_ids, np.int32))


def _table(rng, pairs, extra=()):
    """pairs: (depth, slot id) in any order, extra: more of them; shuffled into feature order"""
    rows = list(pairs) + list(extra)
    order = rng.permutation(len(rows))
    return frame(rng, [rows[i][0] for i in order], [rows[i][1] for i in order])


def tables(seed=4):
    """name -> (frame, n_created the rule gives, worked out by hand).  Slot ids are those of holder_store(); -1, NOBODY, ERASED_ONLY
    and UNFLAGGED are null, HELD / BAD_ONLY / ERASED_AND_3 / TWICE / SECOND tracked.  near < TH < far"""
    rng = np.random.default_rng(seed)
    near = lambda k: [(f32(rng.uniform(0.5, 2.9)), -1) for _ in range(k)]
    far = lambda k, slot=-1: [(f32(rng.uniform(3.1, 9.0)), slot) for _ in range(k)]
    mono = lambda k: [(f32(-1.0), int(rng.choice(HELD + [-1]))) for _ in range(k)]
    t = {}
    t["all_below"] = (_table(rng, near(150), mono(20)), 150)
    for k in (100, 101, 102):     # the first far pair is created, then the count is past 100 and it is far: the walk ends
        t[f"near_{k}_then_far"] = (_table(rng, near(k) + far(20), mono(10)), k + 1)
    t["fewer_than_101_near"] = (_table(rng, near(50) + far(80)), 101)             # far points are created until the count passes 100
    t["far_tracked_ends"] = (_table(rng, near(101) + [(f32(3.05), HELD[0])] + [(f32(3.2 + 0.1 * i), -1) for i in range(10)]), 101)
    t["depth_equals_th"] = (_table(rng, near(101) + [(TH, -1), (TH, HELD[1]), (f32(3.5), -1), (f32(3.6), -1)]), 103)
    t["equal_depths"] = (_table(rng, [(f32(1.25), -1)] * 40 + [(f32(3.75), -1)] * 70 + [(f32(1.25), HELD[2])] * 5), 40 + 61)
    t["special_depths"] = (_table(rng, [(f32(-1.0), -1), (f32(-0.0), -1), (f32(0.0), -1), (f32(np.nan), -1), (f32(np.inf), -1),
                                        (f32(np.inf), HELD[3]), (f32(-0.0), HELD[4]), (f32(np.nan), HELD[5])] + near(6)), 7)
    t["holder_rules"] = (_table(rng, [(f32(1.0 + 0.1 * i), s) for i, s in enumerate(
        [ERASED_ONLY, ERASED_AND_3, BAD_ONLY, UNFLAGGED, TWICE, SECOND, NOBODY, -1, -7, HELD[6], HELD[6], HELD[7]])] +
        [(f32(-1.0), ERASED_ONLY), (f32(-1.0), ERASED_AND_3), (f32(-1.0), TWICE)]), 5)
    return t


def initial_table(seed=6):
    """initial == 1: every feature with !(d < 0) gets a point, d == 0, -0 and NaN included; (frame, n_created)"""
    rng = np.random.default_rng(seed)
    depth = [f32(0.0), f32(-0.0), f32(np.nan), f32(-1.0), f32(-0.5)] + [f32(rng.uniform(0.5, 9.0)) for _ in range(140)]
    f = _table(rng, [(d, -1) for d in depth])
    return f, 143


def random_frame(seed, n, ids, p_null=0.4, p_mono=0.3):
    """n features: depths 0.5 .. 9 m (TH in between), a slot drawn from `ids` or null"""
    rng = np.random.default_rng(seed)
    depth = np.where(rng.random(n) < p_mono, -1.0, rng.uniform(0.5, 9.0, n)).astype(f32)
    ids = np.asarray(ids, np.int32)
    slots = np.where(rng.random(n) < p_null, -1, ids[rng.integers(0, len(ids), n)])
    return frame(rng, depth, slots)


# ---- the chain --------------------------------------------------------------------------------------------------------------
K_CHAIN, N_CHAIN = 5, 256
CHAIN_TH = f32(7.0)


def chain_frames(vd, seed, K=K_CHAIN, n_feat=N_CHAIN, n_world=420):
    """new_points_inputs.random_scene's geometry as frames: K frames of n_feat features over a slab of points 4 .. 9 m in front of
    cameras that move sideways.  60 % of the features are stereo (depth = z, exact); a point's descriptor is a word of the
    vocabulary with up to three bits flipped, so that the views of a point share a node.  -> [(frame without slot_ids, world point
    per feature)]: the slots are drawn while the chain runs, from the ids the earlier key-frames gave the points"""
    rng = np.random.default_rng(seed)
    W = np.stack([rng.uniform(-3, 4, n_world), rng.uniform(-2, 2, n_world), rng.uniform(4, 9, n_world)], 1)
    leaves = np.flatnonzero(np.asarray(vd["word_id"]) >= 0)
    base = np.asarray(vd["node_desc"], np.uint8)[rng.choice(leaves, n_world)]
    level = rng.integers(0, 4, n_world)
    rot0 = rng.uniform(0, 360, n_world)
    stereo_pt = rng.random(n_world) < 0.6
    out, c = [], np.zeros(3)
    for k in range(K):
        c = c + np.array([rng.uniform(0.25, 0.45), rng.uniform(-0.05, 0.05), 0.0])
        T = ni.se3(rng.normal(0, 0.02, 3), c)
        seen = rng.permutation(np.sort(rng.choice(n_world, n_feat, replace=False)))
        x, y, depth, ur, desc, angle, octave = [], [], [], [], [], [], []
        for p in seen:
            pc = [T[3 * r] * W[p][0] + T[3 * r + 1] * W[p][1] + T[3 * r + 2] * W[p][2] + T[9 + r] for r in range(3)]
            u, v, z = f32(500.0 * pc[0] / pc[2] + 320.0), f32(500.0 * pc[1] / pc[2] + 240.0), f32(pc[2])
            st = bool(stereo_pt[p])
            x.append(u), y.append(v), depth.append(z if st else f32(-1.0)), ur.append(u - f32(40.0) / z if st else f32(-1.0))
            desc.append(ni.flip_bits(rng, base[p], int(rng.integers(0, 4))))
            angle.append(f32((rot0[p] + 20.0 * k + rng.uniform(-2, 2)) % 360.0)), octave.append(int(level[p]))
        out.append((dict(Tcw12=np.array(T), x=np.array(x, f32), y=np.array(y, f32), octave=np.array(octave, np.int32),
                         angle=np.array(angle, f32), depth=np.array(depth, f32), u_right=np.array(ur, f32), desc=np.array(desc, np.uint8)),
                    [int(p) for p in seen]))
    return out


def chain_slots(store_ids, world, rng):
    """the slots of a frame: the id an earlier key-frame gave the world point, for four features in five that have one"""
    return np.array([store_ids.get(p, -1) if rng.random() < 0.8 else -1 for p in world], np.int32)


CHAIN_SEED = 0   # chosen on the CPU (tests/test_keyframe_create_ref.py checks it): every gate of the chain's create_map_points decisive


def model_chain(seed=CHAIN_SEED, exp=None, log=None):
    """create (initial) -> process, then four times need_stats -> create -> process, then create_map_points and the local-BA
    window of the last key-frame, on the model -> (model, dict(frames with their slot_ids, records, created, stats, window))"""
    from keyframe_create_ref import KeyframeCreateModel
    vd = vocabulary()
    m = KeyframeCreateModel(CAM6, SF, FIRST_ID, CAPS, exp, log, MAX_RECENT)
    rng = np.random.default_rng(seed + 1000)
    store_ids, out = {}, dict(frames=[], nodes=[], records=[], stats=[], vd=vd)
    for k, (f, world) in enumerate(chain_frames(vd, seed)):
        f = dict(f, slot_ids=chain_slots(store_ids, world, rng) if k else np.full(len(world), -1, np.int32))
        nodes = node_of(vd, f["desc"])
        if k:
            out["stats"].append(m.need_stats(k - 1, 2 if k <= 2 else 3, f["depth"], f["slot_ids"], CHAIN_TH))
        kk = m.create_keyframe(f, CHAIN_TH, initial=k == 0, nodes=nodes)
        out["records"].append(m.keyframe_result())
        m.process_new_keyframe(kk)
        for i, p in enumerate(m.store[kk]["ids"]):
            if p >= 0:
                store_ids.setdefault(world[i], p)
        out["frames"].append(f), out["nodes"].append(nodes)
    m.create(K_CHAIN - 1, 10)
    m.window(K_CHAIN - 1)
    out["window"] = dict(m.record)
    return m, out
