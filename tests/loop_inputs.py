"""Inputs of the loop-closure solvers away from the corner the older tests sit in: true rotations of 0.5 ... pi about a
skew axis and about y, scales of 0.25 ... 4, sizes on either side of the block widths.  Plain numpy (and scipy's Rotation
as the independent rotation code); nothing here imports the device library or the oracle -- the two helpers at the end
take the oracle's binding from their caller.

The *_ORACLE_* constants are what the CPU oracle reaches on exactly these inputs (tests/test_loop_inputs_ref.py measures
them again, prints them and holds them to the values here); the device bounds of tests/test_gpu_loop_rotated.py are
derived from them.

Conventions (those of synth.py): a Sim3 is (s, R, t) with S p = s R p + t; the refinement's pose is [angle-axis (3), t (3)];
pose-graph quaternions are (x, y, z, w).
"""
import numpy as np

import gauge
from vo_slam_test_amd import synth

ANGLES = [0.5, 2.2, 2.6, 3.0, np.pi - 0.01]
AXES = {"skew": gauge.SKEW, "y": np.array([0.0, 1.0, 0.0])}
CENTRE = np.array([0.0, 0.0, 4.0])

# oracle (cyclic Jacobi) against LAPACK's eigh over ransac_cases(), relative to max(1, |entry|): measured 3.43e-11
HORN_ORACLE_WORST = 3.5e-11
# oracle pose graph under a rotation-plus-scale change of the world frame over frame_graphs() x frame_changes():
# measured 1.50e-15 (quaternion coefficients) and 2.31e-14 (translations)
FRAME_ORACLE_Q, FRAME_ORACLE_T = 1.6e-15, 2.4e-14
# oracle pose graph, re-fed until its cost stops falling, against scipy's least_squares on scipy_graph(): cost without the
# scale rows 1.70e-7 above scipy's (relative), poses 1.84e-4 from scipy's (the constant scale rows make up 99.3 % of the
# cost, so Ceres' relative function tolerance of 1e-6 stops every solve that far short)
PG_SCIPY_COST_GAP, PG_SCIPY_POSE_GAP = 2e-7, 2e-4
# half extents of the cloud about CENTRE in the frame the Sim3 maps FROM, divided by max(1, s): its image s R (p - c) + c
# then stays within |(1.5, 1.2, 1.5)| = 2.44 of c whatever R is, i.e. at z > 1.56 - 0.3 (the jitter of t) in the other camera
HALF_BOX = np.array([1.5, 1.2, 1.5])


def rotations(with_pi=False):
    """[(label, R)]: the shared grid, axis-major; with_pi adds exactly pi about the skew axis"""
    out = [(f"{name}_{th:.3f}", gauge.rotation(a, th)) for name, a in AXES.items() for th in ANGLES]
    if with_pi:
        out.append(("skew_pi", gauge.rotation(gauge.SKEW, np.pi)))
    return out


def place_t(rng, R, s):
    """t = c - s R c + U(-0.3, 0.3)^3: the cloud about c = (0, 0, 4) stays about c, in front of the other camera"""
    return CENTRE - s * R @ CENTRE + rng.uniform(-0.3, 0.3, 3)


def cloud(rng, n, s):
    return CENTRE + rng.uniform(-1, 1, (n, 3)) * HALF_BOX / max(1.0, s)


def _px(p, cam):
    return np.stack([cam[0] * p[:, 0] / p[:, 2] + cam[2], cam[1] * p[:, 1] / p[:, 2] + cam[3]], 1)


# ------------------------------------------------------------------------------------------------- A. Sim3 hypotheses
RANSAC_SIZES = [3, 64, 255, 256, 257, 300]
RANSAC_SCALES = [(0.25, False), (1.0, False), (4.0, False), (1.0, True)]
RANSAC_K = 40


def sim3_ransac_data(seed, R, scale, n, outliers=0.2, K=RANSAC_K):
    """The tuple of test_gpu_loop._sim3_data for a given true (R, scale): pc1 = s R pc2 + t + N(0, 4 mm), a fifth of the
    rows displaced by U(-0.5, 0.5)^3 (bounded, so that every pc1 stays in front of its camera), integer thresholds of
    random octaves, K triplets of distinct indices."""
    rng = np.random.default_rng(0xA5130000 + seed)
    cam = synth.CAM[:4].astype(np.float32)
    camd = cam.astype(np.float64)
    pc2 = cloud(rng, n, scale)
    t = place_t(rng, R, scale)
    pc1 = scale * pc2 @ R.T + t + rng.normal(0, 0.004, (n, 3))
    bad = rng.random(n) < outliers
    pc1[bad] += rng.uniform(-0.5, 0.5, (int(bad.sum()), 3))
    me1 = (9.210 * (1.2 ** rng.integers(0, 8, n)) ** 2).astype(np.int32)
    me2 = (9.210 * (1.2 ** rng.integers(0, 8, n)) ** 2).astype(np.int32)
    tri = np.stack([rng.choice(n, 3, replace=False) for _ in range(K)]).astype(np.int32)
    return (np.ascontiguousarray(pc1), np.ascontiguousarray(pc2), np.ascontiguousarray(_px(pc1, camd)),
            np.ascontiguousarray(_px(pc2, camd)), me1, me2, cam, tri, (R, t))


def ransac_cases():
    """[(label, data tuple, fix_scale, scale)]: 11 rotations x 4 scale settings, the six sizes spread so that every size
    meets both fix_scale values"""
    out = []
    for ir, (label, R) in enumerate(rotations(with_pi=True)):
        for isc, (scale, fix) in enumerate(RANSAC_SCALES):
            n = RANSAC_SIZES[(ir + isc) % len(RANSAC_SIZES)]
            out.append((f"{label}_s{scale}_{'fixed' if fix else 'free'}_n{n}", sim3_ransac_data(4 * ir + isc, R, scale, n), fix, scale))
    return out


def degenerate_ransac_data():
    """n = 64 correspondences of an identity-rotation case whose first six rows are replaced: 0..2 exactly collinear in both
    clouds (coordinates that are exact in binary), 3..5 within 1e-12 of one another.  Triplets: the collinear one, the
    coincident one, and two ordinary ones."""
    pc1, pc2, _, _, me1, me2, cam, _, _ = sim3_ransac_data(900, np.eye(3), 1.0, 64)
    camd = cam.astype(np.float64)
    for k in range(3):
        pc2[k] = [0.5 * k - 0.5, 0.25, 3.5]
        pc1[k] = [0.5 * k - 0.25, 0.5, 3.75]
    base = np.array([0.3, -0.2, 4.1])
    off = 1e-12 * np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]])
    for k in range(3):
        pc2[3 + k] = base + off[k]
        pc1[3 + k] = base + 0.125 + off[k][::-1]
    tri = np.array([[0, 1, 2], [3, 4, 5], [10, 20, 30], [7, 40, 63]], np.int32)
    return pc1, pc2, np.ascontiguousarray(_px(pc1, camd)), np.ascontiguousarray(_px(pc2, camd)), me1, me2, cam, tri


def horn_numpy(P1, P2, fix_scale):
    """Horn's closed form as Sim3Solver::computeSim3 writes it (sim3Solver.cpp:179-240), with numpy's LAPACK eigh instead
    of the Jacobi sweeps the device and the oracle share: P1 = s R P2 + t for the three sampled correspondences"""
    O1, O2 = P1.mean(0), P2.mean(0)
    Pr1, Pr2 = (P1 - O1).T, (P2 - O2).T
    M = Pr2 @ Pr1.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    w, V = np.linalg.eigh(N)
    q = V[:, -1]                                   # (w, x, y, z) of the largest eigenvalue
    vec, nv = q[1:], np.linalg.norm(q[1:])
    rv = 2.0 * np.arctan2(nv, q[0]) * vec / nv     # the reference goes through the angle-axis vector and cv::Rodrigues
    th = np.linalg.norm(rv)
    k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    P3 = R @ Pr2
    s = 1.0 if fix_scale else float((Pr1 * P3).sum() / (P3 * P3).sum())
    return R, O1 - s * R @ O2, s


def horn_all(data, fix_scale):
    """[K, 13] (R row-major, t, s) of every triplet with horn_numpy"""
    pc1, pc2, tri = data[0], data[1], data[7]
    out = np.zeros((len(tri), 13))
    for k, idx in enumerate(tri):
        R, t, s = horn_numpy(pc1[idx], pc2[idx], fix_scale)
        out[k, :9], out[k, 9:12], out[k, 12] = R.reshape(-1), t, s
    return out


def sims_distance(a, b):
    """largest difference of two [K, 13] hypothesis arrays relative to max(1, |entry|) (translations reach 25 at scale 4)"""
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


def check_inliers_numpy(data, sims):
    """Sim3Solver::checkInliers restated in float64 (no project code): pc2 through (s, R, t) into image 1, pc1 through the
    inverse into image 2, squared pixel errors against the integer thresholds -> (flags [K, n], near [K, n]) where
    `near` marks the pairs with an error within 0.1 % of its threshold (float32 steps of the library may decide those
    either way)"""
    pc1, pc2, px1, px2, me1, me2, cam = data[:7]
    cam = cam.astype(np.float64)
    K, n = len(sims), len(pc1)
    flags, near = np.zeros((K, n), np.uint8), np.zeros((K, n), bool)
    for k in range(K):
        R, t, s = sims[k, :9].reshape(3, 3), sims[k, 9:12], sims[k, 12]
        a = s * pc2 @ R.T + t
        b = ((pc1 - t) @ R) / s                    # rows: R^T (p - t) / s
        e1 = ((_px(a, cam) - px1) ** 2).sum(1)
        e2 = ((_px(b, cam) - px2) ** 2).sum(1)
        flags[k] = (e1 < me1) & (e2 < me2)
        near[k] = (np.abs(e1 - me1) <= 1e-3 * me1) | (np.abs(e2 - me2) <= 1e-3 * me2)
    return flags, near


# ------------------------------------------------------------------------------------------------- B. Sim3 refinement
REFINE_SCALES = [0.5, 1.0, 2.0]
REFINE_SIZES = [10, 11, 37, 256, 257, 1000]


def sim3_refine_problem(seed, R, scale, n, fix_scale, outliers=0.1, pix_noise=1.0, point_noise=0.01, unit_sigma=False):
    """synth.make_sim3_problem's recipe for a given true (R, scale): t placed as for the hypotheses; the initial guess is
    the truth with 0.03 rad about a random axis composed on the left, up to 0.05 per coordinate in t and -- where the scale
    is free -- 3 % in the scale (a fixed scale starts, and stays, at the truth: 3 % of a 1.5 m cloud would be 6 px).  The
    angle-axis vectors come from scipy's Rotation.as_rotvec, so |w| <= pi at the start."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(0xB5130000 + seed)
    cam = np.array(synth.CAM, np.float64)
    Pm = cloud(rng, n, scale)
    t = place_t(rng, R, scale)
    Pc = scale * Pm @ R.T + t
    octs = np.zeros((2, n), np.int64) if unit_sigma else rng.integers(0, 8, (2, n))
    sig = 1.2 ** octs
    pix_m = _px(Pm, cam) + rng.normal(0, pix_noise, (n, 2)) * sig[0][:, None]
    pix_c = _px(Pc, cam) + rng.normal(0, pix_noise, (n, 2)) * sig[1][:, None]
    bad = rng.random(n) < outliers
    pix_c[bad] += rng.uniform(-60, 60, (int(bad.sum()), 2))
    Pm_n = Pm + rng.normal(0, point_noise, Pm.shape)
    Pc_n = Pc + rng.normal(0, point_noise, Pc.shape)
    ax = rng.normal(size=3)
    R0 = Rotation.from_rotvec(0.03 * ax / np.linalg.norm(ax)).as_matrix() @ R
    pose0 = np.concatenate([Rotation.from_matrix(R0).as_rotvec(), t + rng.uniform(-0.05, 0.05, 3)])
    return dict(cam_match=np.ascontiguousarray(Pm_n), pix_curr=np.ascontiguousarray(pix_c),
                isig_curr=np.ascontiguousarray(1.0 / sig[1]), cam_curr=np.ascontiguousarray(Pc_n),
                pix_match=np.ascontiguousarray(pix_m), isig_match=np.ascontiguousarray(1.0 / sig[0]), cam=cam, pose0=pose0,
                scale0=float(scale if fix_scale else 1.03 * scale), true=(R, t, float(scale)), is_outlier=bad,
                clean_points=(Pm, Pc))


def refine_problems(fix_scale):
    """[(label, problem)]: every rotation x scale x size for one fix_scale value (180 ragged problems of one call)"""
    out = []
    for ir, (label, R) in enumerate(rotations()):
        for isc, s in enumerate(REFINE_SCALES):
            for isz, n in enumerate(REFINE_SIZES):
                seed = (ir * 3 + isc) * 6 + isz + (1000 if fix_scale else 0)
                out.append((f"{label}_s{s}_n{n}", sim3_refine_problem(seed, R, s, n, fix_scale)))
    return out


def consistent_refine_problems():
    """[(label, problem, fix_scale)] for the comparison with scipy: every rotation at n = 256, scale 2 free and scale 1
    fixed; unit sigmas (the Jacobians of the reference lack the 1 / sigma of its residuals), no outliers, 0.3 px pixel
    noise and 1 mm point noise, so that no block comes near the Huber threshold sqrt(10) and nothing is rejected"""
    out = []
    for ir, (label, R) in enumerate(rotations()):
        for s, fix in ((2.0, False), (1.0, True)):
            pr = sim3_refine_problem(2000 + 2 * ir + int(fix), R, s, 256, fix, outliers=0.0, pix_noise=0.3, point_noise=0.001,
                                     unit_sigma=True)
            out.append((f"{label}_s{s}_{'fixed' if fix else 'free'}", pr, fix))
    return out


def sim3_block_residuals(pr, R, t, s):
    """the two reprojection blocks of every match at (R, t, s), written out independently: [n, 4] in sigma units"""
    cam = pr["cam"]
    p = s * pr["cam_match"] @ R.T + t
    q = ((pr["cam_curr"] - t) @ R) / s
    rf = (pr["pix_curr"] - _px(p, cam)) * pr["isig_curr"][:, None]
    ri = (pr["pix_match"] - _px(q, cam)) * pr["isig_match"][:, None]
    return np.concatenate([rf, ri], 1)


def sim3_scipy_minimum(pr, fix_scale):
    """scipy.optimize.least_squares on sim3_block_residuals about the true Sim3: a left rotation-vector perturbation, an
    additive translation and (free scale) an additive scale offset -> ((R, t, s), cost)"""
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation
    Rt, tt, st = pr["true"]
    s_fixed = pr["scale0"]

    def unpack(d):
        return Rotation.from_rotvec(d[:3]).as_matrix() @ Rt, tt + d[3:6], (s_fixed if fix_scale else st + d[6])

    ref = least_squares(lambda d: sim3_block_residuals(pr, *unpack(d)).reshape(-1), np.zeros(6 if fix_scale else 7), method="trf",
                        xtol=1e-14, ftol=1e-14, gtol=1e-14)
    return unpack(ref.x), 0.5 * float((ref.fun ** 2).sum())


def sim3_of(pose, scale):
    """(R, t, s) of a refinement result, the rotation through scipy"""
    from scipy.spatial.transform import Rotation
    return Rotation.from_rotvec(pose[:3]).as_matrix(), np.asarray(pose[3:], np.float64), float(scale)


def survivor_problem(k, n=40):
    """a clean n-match problem (0.5 rad about the skew axis, 0.3 px and 1 mm of noise, so that no clean match comes near
    chi2 = 10) whose pix_curr is moved by 500 px on all but the first k matches -- by +500 and -500 in turn: the Huber loss
    bounds each moved block's pull but does not remove it, and thirty pulls in one direction drag the first solve far
    enough to fail some of the clean matches as well"""
    pr = sim3_refine_problem(3000, gauge.rotation(gauge.SKEW, 0.5), 1.0, n, True, outliers=0.0, pix_noise=0.3, point_noise=0.001)
    pix = pr["pix_curr"].copy()
    pix[k:] += 500.0 * np.where(np.arange(n - k) % 2 == 0, 1.0, -1.0)[:, None]
    return dict(pr, pix_curr=np.ascontiguousarray(pix))


def clean_problem():
    """a problem on which nothing is rejected after the first solve: no outliers, 0.3 px noise, mixed octaves, 150 matches"""
    return sim3_refine_problem(3100, gauge.rotation(AXES["y"], 2.2), 1.0, 150, True, outliers=0.0, pix_noise=0.3, point_noise=0.001)


# ------------------------------------------------------------------------------------------------- C. pose graph
def q_mul(a, b):
    """Hamilton product of (x, y, z, w) quaternions"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def q_conj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def q_matrix(q):
    from scipy.spatial.transform import Rotation
    return Rotation.from_quat(q).as_matrix()


def sim3_pose_graph(g, seed, fixed, consistent=True):
    """A synth.make_pose_graph dict with per-node scales log-uniform in [0.7, 1.4] and every measurement recomputed as the
    Sim3 S_ji = S_j S_i^-1 (i = e_i, j = e_j): q_ji = q_j q_i^-1, s_ji = s_j / s_i, t_ji = t_j - s_ji R_ji t_i -- from the
    drifted map, except the loop edge (the last one), which comes from the true trajectory.  consistent=False multiplies
    every s_meas by exp(N(0, 0.02)): r[6] leaves 1 and the translation rows of every edge get a residual."""
    rng = np.random.default_rng(0xC5130000 + seed)
    n, ne = len(g["quats"]), len(g["e_i"])
    scales = np.exp(rng.uniform(np.log(0.7), np.log(1.4), n))
    qm, tm, sm = np.zeros((ne, 4)), np.zeros((ne, 3)), np.zeros(ne)
    for e in range(ne):
        i, j = int(g["e_i"][e]), int(g["e_j"][e])
        Q, T = (g["true_quats"], g["true_trans"]) if e == ne - 1 else (g["quats"], g["trans"])
        qm[e] = q_mul(Q[j], q_conj(Q[i]))
        sm[e] = scales[j] / scales[i]
        tm[e] = T[j] - sm[e] * q_matrix(qm[e]) @ T[i]
    if not consistent:
        sm = sm * np.exp(rng.normal(0, 0.02, ne))
    return dict(g, scales=scales, fixed=int(fixed), q_meas=np.ascontiguousarray(qm), t_meas=np.ascontiguousarray(tm),
                s_meas=np.ascontiguousarray(sm))


POSE_GRAPH_CASES = [(2, 1), (3, 1), (12, 5), (40, 39), (90, 0)]


def pose_graph_cases():
    """[(label, graph)]: (n_kf, fixed) of POSE_GRAPH_CASES with both `consistent` settings, and a 13-node graph whose last
    node no edge touches"""
    out = []
    for k, (n_kf, fixed) in enumerate(POSE_GRAPH_CASES):
        for c in (True, False):
            out.append((f"n{n_kf}_fixed{fixed}_{'consistent' if c else 'inconsistent'}",
                        sim3_pose_graph(synth.make_pose_graph(20 + k, n_kf=n_kf), 2 * k + int(c), fixed, c)))
    out.append(("n13_one_node_without_edges", with_isolated_node(sim3_pose_graph(synth.make_pose_graph(30, n_kf=12), 40, 5, False))))
    return out


def with_isolated_node(g):
    """one more node at the end that no edge touches"""
    return dict(g, quats=np.ascontiguousarray(np.vstack([g["quats"], [[0.5, -0.5, 0.5, -0.5]]])),
                trans=np.ascontiguousarray(np.vstack([g["trans"], [[1.0, 2.0, 3.0]]])), scales=np.append(g["scales"], 1.25),
                true_quats=np.vstack([g["true_quats"], [[0.5, -0.5, 0.5, -0.5]]]), true_trans=np.vstack([g["true_trans"], [[1.0, 2.0, 3.0]]]))


def negate_signs(g):
    """the quaternions of the odd nodes and of every third measurement negated -> (graph, node signs)"""
    sn = np.where(np.arange(len(g["quats"])) % 2 == 1, -1.0, 1.0)
    se = np.where(np.arange(len(g["e_i"])) % 3 == 0, -1.0, 1.0)
    return dict(g, quats=np.ascontiguousarray(g["quats"] * sn[:, None]), q_meas=np.ascontiguousarray(g["q_meas"] * se[:, None])), sn


def frame_graphs():
    """[(label, graph)] of the world-frame check: n_kf = 12 and 40 at drift 0.01, 30 at drift 0.05, non-unit scales"""
    return [("n12", sim3_pose_graph(synth.make_pose_graph(50, n_kf=12), 50, 3, False)),
            ("n40", sim3_pose_graph(synth.make_pose_graph(51, n_kf=40), 51, 0, False)),
            ("n30_drift0.05", sim3_pose_graph(synth.make_pose_graph(5, n_kf=30, drift=0.05), 52, 29, False))]


def frame_changes():
    """[(label, q_T, s_T)]: every rotation of gauge.GAUGES (q_T with w < 0 for the third) x s_T in {1, 1.7}"""
    from scipy.spatial.transform import Rotation
    out = []
    for k, (name, (R, _)) in enumerate(gauge.GAUGES.items()):
        qT = Rotation.from_matrix(R).as_quat()
        qT = qT * np.sign(qT[3]) * (-1.0 if k == 2 else 1.0)       # w < 0 for the third, w > 0 otherwise
        for sT in (1.0, 1.7):
            out.append((f"{name}_s{sT}", qT, sT))
    return out


def change_frame(g, qT, sT):
    """every node right-multiplied by T = (s_T, R_T, 0): q_i -> q_i q_T, t_i unchanged, s_i -> s_i s_T"""
    return dict(g, quats=np.ascontiguousarray([q_mul(q, qT) for q in g["quats"]]), scales=g["scales"] * sT)


def frame_back(q, qT):
    return np.array([q_mul(qi, q_conj(qT)) for qi in q])


def quat_distance(qa, qb):
    """largest coefficient difference of two quaternion arrays, each pair taken at its closer sign"""
    qa, qb = np.asarray(qa), np.asarray(qb)
    return float(np.minimum(np.abs(qa - qb).max(1), np.abs(qa + qb).max(1)).max())


def pose_graph_residuals(g, R, t):
    """rows 0..5 of every edge's residual at node rotations R [n, 3, 3] and translations t [n, 3], written with matrices
    and scipy's quaternion code: 2 vec(q_ji q_i q_j^-1) and the translation of S_ji (S_i S_j^-1) -> [E, 6]"""
    from scipy.spatial.transform import Rotation
    s = g["scales"]
    out = np.zeros((len(g["e_i"]), 6))
    for e in range(len(g["e_i"])):
        i, j = int(g["e_i"][e]), int(g["e_j"][e])
        Rm, tm, sm = q_matrix(g["q_meas"][e]), g["t_meas"][e], g["s_meas"][e]
        dq = Rotation.from_matrix(Rm @ R[i] @ R[j].T).as_quat()
        dq = dq if dq[3] >= 0 else -dq
        # the sign of vec(dq) is that of the product of the three quaternions handed over; the cost does not see it
        t_ij = t[i] - (s[i] / s[j]) * R[i] @ R[j].T @ t[j]
        out[e, :3] = 2.0 * dq[:3]
        out[e, 3:] = sm * Rm @ t_ij + tm
    return out


def pose_graph_scale_constant(g):
    """what the constant r[6] = s_ji s_i / s_j rows add to the cost"""
    r6 = g["s_meas"] * g["scales"][g["e_i"]] / g["scales"][g["e_j"]]
    return 0.5 * float((r6 ** 2).sum())


def pose_graph_scipy_minimum(g):
    """least_squares on pose_graph_residuals about the graph's start: a left rotation vector and an additive translation
    per free node (6 per node, the fixed one left out) -> (R [n, 3, 3], t [n, 3], cost without the scale rows)"""
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation
    n, fixed = len(g["quats"]), g["fixed"]
    R0 = np.array([q_matrix(q) for q in g["quats"]])
    free = [a for a in range(n) if a != fixed]

    def unpack(d):
        R, t = R0.copy(), g["trans"].copy()
        for k, a in enumerate(free):
            R[a] = Rotation.from_rotvec(d[6 * k:6 * k + 3]).as_matrix() @ R0[a]
            t[a] = g["trans"][a] + d[6 * k + 3:6 * k + 6]
        return R, t

    ref = least_squares(lambda d: pose_graph_residuals(g, *unpack(d)).reshape(-1), np.zeros(6 * len(free)), method="trf",
                        xtol=1e-15, ftol=1e-15, gtol=1e-15)
    R, t = unpack(ref.x)
    return R, t, 0.5 * float((ref.fun ** 2).sum())


def scipy_graph():
    return sim3_pose_graph(synth.make_pose_graph(60, n_kf=8, drift=0.02), 60, 3, False)


# ------------------------------------------------------------------------------------------------- D. re-anchoring
def reanchor_inputs(seed, n, scale):
    """n points, 6 nodes of random unit quaternions (every second one with w < 0) and scales `scale` and 1 / scale"""
    rng = np.random.default_rng(0xD5130000 + seed)
    k = 6

    def sims(s):
        q = rng.normal(size=(k, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        q *= (np.where(np.arange(k) % 2 == 0, -1.0, 1.0) * np.sign(q[:, 3]))[:, None]   # w < 0 for the even nodes
        return np.concatenate([q, rng.normal(size=(k, 3)), np.full((k, 1), s) * rng.uniform(0.9, 1.1, (k, 1))], 1)

    S1, S2 = sims(scale), sims(1.0 / scale)
    pts = rng.normal(size=(n, 3)) * 3
    ref = rng.integers(-1, k, n).astype(np.int32)
    exp = pts.copy()
    for i in range(n):
        r = ref[i]
        if r >= 0:
            a = S1[r, 7] * q_matrix(S1[r, :4]) @ pts[i] + S1[r, 4:7]
            exp[i] = S2[r, 7] * q_matrix(S2[r, :4]) @ a + S2[r, 4:7]
    return pts, ref, S1, S2, exp


# ------------------------------------------------------------------------------------------------- E. triangulation
def triangulation_inputs(seed, n, angle):
    """n points about (0, 0, 4) seen from a first camera near the identity and a second one turned `angle` about y and
    placed beyond the points (t = c - R c + a small offset), so that every point is in front of both"""
    rng = np.random.default_rng(0xE5130000 + seed)
    P = CENTRE + rng.uniform(-1, 1, (n, 3)) * np.array([1.2, 1.0, 1.0])
    R1, t1 = synth.se3_exp(np.array([0.03, -0.01, 0.02, 0.01, -0.02, 0.01]))
    R2 = gauge.rotation(AXES["y"], angle)
    t2 = CENTRE - R2 @ CENTRE + np.array([0.1, 0.05, 0.3])
    T1 = np.concatenate([R1, t1[:, None]], 1).astype(np.float32)
    T2 = np.concatenate([R2, t2[:, None]], 1).astype(np.float32)
    p1, p2 = P @ R1.T + t1, P @ R2.T + t2
    xn1, xn2 = (p1[:, :2] / p1[:, 2:]).astype(np.float32), (p2[:, :2] / p2[:, 2:]).astype(np.float32)
    return P, T1, T2, xn1, xn2, (p1[:, 2], p2[:, 2])


# ------------------------------------------------------------------------------------------------- oracle calls
# (the binding, tests/oracle_lib.py, is handed over by the caller: this module imports neither it nor the device library)
def oracle_ransac(orc, data, fix_scale):
    """orc_sim3_ransac_eval on a data tuple -> (counts [K], flags [K, n], sims [K, 13])"""
    pc1, pc2, px1, px2, me1, me2, cam, tri = data[:8]
    n, K = len(pc1), len(tri)
    oc, of, osim = np.zeros(K, np.int32), np.zeros((K, n), np.uint8), np.zeros((K, 13))
    orc.lib().orc_sim3_ransac_eval(n, pc1, pc2, px1, px2, me1, me2, cam, K, np.ascontiguousarray(tri), int(fix_scale), oc, of, osim)
    return oc, of, osim


def oracle_phase(osums):
    """the phase orc_sim3_solve reached: its second summary stays zeroed when fewer than 10 matches survive problem 1"""
    return 2 if osums[1].max_iterations > 0 else 1
