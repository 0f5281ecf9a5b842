"""Inputs of the loop Sim3 tests (test infrastructure): synthetic stores of 6 - 12 key-frames with at most 320 features each,
shared by the model's CPU tests and the device's GPU tests.  Plain numpy; nothing here imports the device library or the oracle
(build_device takes the binding from its caller).

The world is a cloud of physical points in front of cameras that look down +z.  Two id populations name the same points: the
OLD pass (id = point number, positions in the world frame) and the NEW pass (id = NEW + point number), whose map has drifted
by the Sim3 DRIFT -- a few degrees, 0.1 - 0.3 units: a new-pass position is DRIFT(p), a new-pass pose is Tcw o DRIFT^-1, so that
every key-frame sees a point at the pixel its true camera sees it.  Descriptors of one point differ by a few bits between
observations; FeatureVector node ids are assigned directly (point number modulo N_NODES, no vocabulary).  Octaves, normals
and min / max distances are set by hand so that the gates decide with a margin: normal = the unit vector from the point's
reference camera, max_distance = d_ref * scale[octave] / sqrt(1.2) (the predicted level of a camera at about that distance is
the octave, half a level from either rounding), min_distance = max_distance / scale[7]."""
import numpy as np

f32 = np.float32
CAM6 = [f32(500.0), f32(500.0), f32(320.0), f32(240.0), f32(40.0), f32(40.0) / f32(500.0)]
SF = np.cumprod([f32(1.0)] + [f32(1.2)] * 7, dtype=f32)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
NK = 320
NEW = 10000
N_NODES = 37
RAND_MAX = 2147483647
LOOP_CAPS = dict(max_candidates=4, max_loop_points=1024, max_rand=3 * 300 * 4)
BA_CAPS = (8, 64, 256)
MAX_RECENT, FUSE_CANDIDATES = 32, 64


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


DRIFT = (rodrigues([0.03, -0.05, 0.02]), np.array([0.2, -0.1, 0.15]), 1.0)   # (R, t, s): about 3.5 degrees, 0.27 units


def rand_values(seed, n):
    return np.random.default_rng(0x51300 + seed).integers(0, RAND_MAX, n, dtype=np.int64).astype(np.int32)


class World:
    def __init__(self, seed, n_points=700):
        self.rng = rng = np.random.default_rng(0x10095 + seed)
        self.P = np.stack([rng.uniform(-2.2, 2.2, n_points), rng.uniform(-1.6, 1.6, n_points), rng.uniform(5.0, 8.0, n_points)], 1)
        self.desc = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
        self.octave = rng.integers(0, 4, n_points)
        self.angle = rng.uniform(0, 360, n_points).astype(f32)
        self.store = []

    def keyframe(self, centre, points, new=False, rot=(0.0, 0.0, 0.0), bad=False, scramble=(), displace=(), unmapped=(), noise=0.3,
                 no_pose=False):
        """a key-frame at `centre` (world frame) that sees the world points `points`, in that order.  scramble: points whose map
        position is somewhere else (descriptor and pixel stay); displace: points whose key-point sits 30 px away from where the
        camera sees them; unmapped: features without a map point; no_pose: the key-frame's pose is never set"""
        rng, k = self.rng, len(self.store)
        R = rodrigues(rot)
        t = -R @ np.asarray(centre, np.float64)
        n = len(points)
        assert n <= NK
        pc = self.P[points] @ R.T + t
        uv = np.stack([500.0 * pc[:, 0] / pc[:, 2] + 320.0, 500.0 * pc[:, 1] / pc[:, 2] + 240.0], 1) + rng.normal(0, noise, (n, 2))
        assert (uv[:, 0] > 20).all() and (uv[:, 0] < 620).all() and (uv[:, 1] > 20).all() and (uv[:, 1] < 460).all(), "a point leaves the image"
        pos = self.P[points].copy()
        for p in scramble:
            j = list(points).index(p)
            pos[j] = [rng.uniform(-2.2, 2.2), rng.uniform(-1.6, 1.6), rng.uniform(5.0, 8.0)]
        for p in displace:
            uv[list(points).index(p)] += [30.0, -30.0]
        d_ref = np.linalg.norm(pos - np.asarray(centre), axis=1)
        normals = (pos - np.asarray(centre)) / d_ref[:, None]
        octave = self.octave[points].astype(np.int32)
        maxd = (d_ref * SF[octave].astype(np.float64) / np.sqrt(1.2))
        ids = np.array([(NEW + p if new else p) for p in points], np.int32)
        flags = np.ones(n, np.uint8)
        for p in unmapped:
            j = list(points).index(p)
            ids[j], flags[j] = -1, 0
        Tcw = np.concatenate([R.reshape(-1), t])
        if new:   # the drifted map: positions D(p), normals rotated, distances scaled, the pose composed with D^-1
            Rd, td, sd = DRIFT
            pos = sd * pos @ Rd.T + td
            normals = normals @ Rd.T
            maxd = maxd * sd
            Rn = R @ Rd.T
            Tcw = np.concatenate([Rn.reshape(-1), sd * t - Rn @ td])
            assert sd == 1.0     # (a pose is an SE3: a drift with a scale would need the cameras' centres rescaled as well)
        desc = self.desc[points].copy()
        for j in range(n):
            bits = np.unpackbits(desc[j])
            bits[rng.choice(256, int(rng.integers(0, 4)), replace=False)] ^= 1
            desc[j] = np.packbits(bits)
        kf = dict(ids=[int(i) for i in ids], flags=[int(fl) for fl in flags], x=uv[:, 0].astype(f32), y=uv[:, 1].astype(f32), octave=octave,
                  angle=self.angle[points].astype(f32), uright=np.full(n, -1.0, f32), depth=np.full(n, -1.0, f32), desc=desc,
                  nodes=np.array([p % N_NODES for p in points], np.int32), points=np.ascontiguousarray(pos), point_desc=self.desc[points].copy(),
                  min_dist=(maxd / float(SF[7])).astype(f32), max_dist=maxd.astype(f32), normals=np.ascontiguousarray(normals),
                  pose=None if no_pose else np.ascontiguousarray(Tcw), bad=bool(bad), erased=False, seen=list(points))
        self.store.append(kf)
        return k


def scene(name, seed=1):
    """-> dict(store, current, cand, fix_scale, rand, max_rounds, caps) of a named scenario.  Key-frames: 0 and 2 the old-pass
    neighbours of the candidate 1; further candidates and fillers behind; the current key-frame (new pass) last."""
    w = World(seed)
    c_old, c_cur = np.array([0.0, 0.0, 0.0]), np.array([0.08, 0.03, -0.1])
    n_shared, n_extra, n_own = 30, 30, 6
    sizes = dict(n63=63, n65=65, n255=255, n257=257)
    if name in sizes:
        n_shared, n_extra = sizes[name], 20
    if name == "rejected":
        n_shared, n_extra = 26, 5
    # every camera of a scene sees the whole cloud (World.keyframe checks it); who holds what is decided here
    A, E = list(range(n_shared)), list(range(n_shared, n_shared + n_extra))
    own = list(range(n_shared + n_extra, n_shared + n_extra + n_own))
    B = list(range(n_shared + n_extra + n_own, n_shared + n_extra + n_own + 12))
    nb = (A + E)[:NK - 8]
    w.keyframe(c_old + [-0.12, 0.0, 0.0], nb)                     # 0
    out = dict(fix_scale=True, max_rounds=8, caps=dict(LOOP_CAPS))
    cand = [1]
    if name == "fails_then_wins":
        # 16 of the first candidate's 30 matched key-points sit 30 px from where its camera sees their points.  Sim3Solver works on
        # projected positions (sim3Solver.cpp:66-67) and counts 30 inliers; solveLoopSim3 reads the candidate's key-point at the
        # observation (optimizer_ceres.cpp:862) and keeps 14
        w.keyframe(c_old, A + B, displace=A[:16])                 # 1
        w.keyframe(c_old + [0.12, 0.02, 0.0], nb)                 # 2
        w.keyframe(c_old + [0.05, -0.03, 0.02], A + B)            # 3: the one that wins
        cand = [1, 3]
    elif name == "three_candidates":
        w.keyframe(c_old, A + B, bad=True)                        # 1: bad
        w.keyframe(c_old + [0.12, 0.02, 0.0], nb)                 # 2
        w.keyframe(c_old + [0.03, 0.0, 0.0], A[:19] + B)          # 3: 19 BoW matches
        w.keyframe(c_old + [0.05, -0.03, 0.02], A + B)            # 4: wins
        cand = [1, 3, 4]
    elif name == "filtered_below_20":
        # the store refuses a negative id under bit 0 and one call changes nothing, so every match of a call has both its
        # observations; the correspondences of a candidate fall below 20 -- to none -- when it has no pose to transform them with
        w.keyframe(c_old, A[:25] + B, no_pose=True)               # 1: 25 matches, no correspondence
        w.keyframe(c_old + [0.12, 0.02, 0.0], nb)                 # 2
    elif name == "outliers_only":
        # candidate 1: 21 matches whose map points are elsewhere -- three trips, then its solver stops; candidate 3: 24 good
        # ones among 60, which keeps walking until a triplet of good ones comes up
        w.keyframe(c_old, A[:21] + B, scramble=A[:21])            # 1
        w.keyframe(c_old + [0.12, 0.02, 0.0], nb)                 # 2
        w.keyframe(c_old + [0.05, -0.03, 0.02], (A + E)[:60] + B, scramble=(A + E)[24:60])   # 3
        cand = [1, 3]
        out["max_rounds"] = 16
    else:
        w.keyframe(c_old, A + B)                                  # 1
        w.keyframe(c_old + [0.12, 0.02, 0.0], nb)                 # 2
    while len(w.store) < 6:                                       # fillers: old-pass key-frames elsewhere
        k = len(w.store)
        w.keyframe(c_old + [0.3, 0.1 * (k % 2), 0.0], B + own[:0])
    cur_pts = own + A + E
    current = w.keyframe(c_cur, cur_pts, new=True, rot=(0.01, -0.02, 0.015), unmapped=E[::2])
    out.update(store=w.store, current=current, cand=cand, rand=rand_values(seed, 3 * 300 * len(cand)), A=A, E=E)
    if name == "free_scale":
        out["fix_scale"] = False
    return out


SCENARIOS = ("accepted", "three_candidates", "filtered_below_20", "outliers_only", "fails_then_wins", "rejected", "n63", "n65", "n255", "n257",
             "free_scale")


def make_model(orc, sc, **caps):
    from loop_sim3_ref import LoopModel
    c = dict(sc["caps"], **caps)
    m = LoopModel(orc, sc["store"], CAM6, SF, BOUNDS, c["max_candidates"], c["max_loop_points"], c["max_rand"])
    m.update_connections(list(range(len(sc["store"]))))
    return m


def run_model(orc, sc, rand=None, max_rounds=None, **caps):
    m = make_model(orc, sc, **caps)
    m.compute_sim3(sc["current"], sc["cand"], sc["fix_scale"], sc["rand"] if rand is None else rand, RAND_MAX,
                   sc["max_rounds"] if max_rounds is None else max_rounds)
    return m


def build_device(vo, sc, loop=True, **caps):
    """the scenario's store on the device, every opt-in block enabled (the loop block unless loop=False)"""
    store = sc["store"]
    s = vo.KeyFrameStore(len(store), NK)
    s.enable_connections()
    s.enable_culling()
    s.enable_mapping(CAM6, SF, 50000)
    s.enable_local_ba(*BA_CAPS)
    s.enable_point_upkeep(MAX_RECENT)
    s.enable_fuse((BOUNDS[0], BOUNDS[1], BOUNDS[2], BOUNDS[3]), FUSE_CANDIDATES)
    if loop:
        s.enable_loop(**dict(sc["caps"], **caps))
    for k, kf in enumerate(store):
        s.insert(dict(angle=kf["angle"], desc=kf["desc"], flags=kf["flags"], points=kf["points"], ids=kf["ids"], point_desc=kf["point_desc"],
                      min_dist=kf["min_dist"], max_dist=kf["max_dist"], nodes=kf["nodes"], bad=kf["bad"]))
        s.set_keypoints(k, kf["octave"], kf["depth"], kf["uright"])
        s.set_keypoint_xy(k, np.stack([kf["x"], kf["y"]], 1))
        if kf["pose"] is not None:
            s.set_pose(k, kf["pose"])
        s.set_normals(k, kf["normals"])
    s.update_connections(list(range(len(store))))
    return s
