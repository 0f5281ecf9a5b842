"""numpy restatement of the PnP RANSAC contract of DESIGN.md §4c: cv::solvePnPRansac(..., 100, 8.0, 0.99, inliers,
SOLVEPNP_EPNP) as poseEstimateByPnP calls it (reference visualOdometry.cpp:778-830), written from the published EPnP
(Lepetit et al. 2009) and OpenCV 3.x's ptsetreg.cpp / solvepnp.cpp / epnp.cpp conventions.  The checker of
vo_pnp_ransac: LAPACK eigen-decompositions and SVDs where the kernels run Jacobi sweeps and a polar iteration, so the two
agree to rounding, not bit for bit (the samples, the float gate and the ordered replay are exact)."""
from __future__ import annotations

import math

import numpy as np

MODEL_POINTS = 5
DBL_MIN = 2.2250738585072014e-308
MASK64 = (1 << 64) - 1


# ----------------------------------------------------------------------------------------------------------------- RNG
def rng_next(state: int) -> tuple[int, int]:
    """cv::RNG::next: state = (uint64)(uint32)state * 4164903690 + (state >> 32); returns (new state, low 32 bits)"""
    state = ((state & 0xFFFFFFFF) * 4164903690 + (state >> 32)) & MASK64
    return state, state & 0xFFFFFFFF


def samples(n: int, iters: int) -> np.ndarray:
    """getSubset's 5-tuples of iterations 0..iters-1 for n correspondences (fresh cv::RNG((uint64)-1); no checkSubset)"""
    st = MASK64
    out = np.zeros((iters, MODEL_POINTS), np.int32)
    for it in range(iters):
        idx: list[int] = []
        while len(idx) < MODEL_POINTS:
            st, r = rng_next(st)
            c = r % n  # uniform(0, n)
            if c not in idx:
                idx.append(c)
        out[it] = idx
    return out


def ransac_update_num_iters(p: float, ep: float, model_points: int, max_iters: int) -> int:
    """RANSACUpdateNumIters (ptsetreg.cpp)"""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - math.pow(1.0 - ep, model_points)
    if denom < DBL_MIN:
        return 0
    num = math.log(num)
    denom = math.log(denom)
    return max_iters if (denom >= 0 or -num >= max_iters * (-denom)) else int(np.rint(num / denom))  # cvRound


# ---------------------------------------------------------------------------------------------------------------- EPnP
def _qr_solve(A: np.ndarray, b: np.ndarray) -> np.ndarray:
    """epnp.cpp qr_solve (Householder) for a batch: A [B, nr, nc], b [B, nr] -> X [B, nc]"""
    A, b = A.copy(), b.copy()
    B, nr, nc = A.shape
    X = np.zeros((B, nc))
    A1, A2 = np.zeros((B, nc)), np.zeros((B, nc))
    ok = np.ones(B, bool)
    for k in range(nc):
        eta = np.abs(A[:, k:, k]).max(axis=1)
        ok &= eta != 0
        eta = np.where(ok, eta, 1.0)
        A[:, k:, k] /= eta[:, None]
        sigma = np.sqrt((A[:, k:, k] ** 2).sum(axis=1))
        sigma = np.where(A[:, k, k] < 0, -sigma, sigma)
        A[:, k, k] += sigma
        A1[:, k] = sigma * A[:, k, k]
        A2[:, k] = -eta * sigma
        for j in range(k + 1, nc):
            tau = (A[:, k:, k] * A[:, k:, j]).sum(axis=1) / A1[:, k]
            A[:, k:, j] -= tau[:, None] * A[:, k:, k]
    for j in range(nc):
        tau = (A[:, j:, j] * b[:, j:]).sum(axis=1) / A1[:, j]
        b[:, j:] -= tau[:, None] * A[:, j:, j]
    X[:, nc - 1] = b[:, nc - 1] / A2[:, nc - 1]
    for i in range(nc - 2, -1, -1):
        X[:, i] = (b[:, i] - (A[:, i, i + 1:] * X[:, i + 1:]).sum(axis=1)) / A2[:, i]
    return np.where(ok[:, None], X, 0.0)


_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def epnp(pw: np.ndarray, us: np.ndarray, cam4) -> tuple[np.ndarray, np.ndarray]:
    """epnp::compute_pose for a batch of point sets of one size m: pw [B, m, 3], us [B, m, 2] (double) -> R [B, 3, 3], t [B, 3].
    Conventions fixed where OpenCV's are its solver's rounding: principal axes descending with their
    largest-magnitude component positive; for every five-point solve (all RANSAC hypotheses, and n == 5) the
    two-dimensional null space of M is rotated so that v1[0] = 0."""
    fu, fv, uc, vc = (float(np.float32(c)) for c in cam4[:4])
    pw, us = np.asarray(pw, np.float64), np.asarray(us, np.float64)
    B, m, _ = pw.shape
    c0 = pw.mean(axis=1)
    d = pw - c0[:, None]
    w, U = np.linalg.eigh(np.einsum("bik,bil->bkl", d, d))
    w, U = w[:, ::-1], U[:, :, ::-1]  # descending; U[:, :, i] axis i
    big = np.abs(U).argmax(axis=1)
    sg = np.where(np.take_along_axis(U, big[:, None, :], axis=1)[:, 0] < 0, -1.0, 1.0)
    U = U * sg[:, None, :]
    k = np.sqrt(np.maximum(w, 0.0) / m)  # (a rounding-negative eigenvalue: 0)
    cws = np.zeros((B, 4, 3))
    cws[:, 0] = c0
    for i in range(1, 4):
        cws[:, i] = c0 + k[:, i - 1, None] * U[:, :, i - 1]
    # CC (column j = k_j u_j) inverted as cvInvert(CV_SVD) does: CC^+ = diag(1/k) U^T, k <= 2 eps sum(k) dropped
    thr = 2.0 * np.finfo(np.float64).eps * k.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        ik = np.where(k > thr, 1.0 / np.where(k > thr, k, 1.0), 0.0)
    ci = np.transpose(U, (0, 2, 1)) * ik[:, :, None]
    al = np.zeros((B, m, 4))
    al[:, :, 1:] = np.einsum("bjk,bik->bij", ci, d)
    al[:, :, 0] = 1.0 - al[:, :, 1] - al[:, :, 2] - al[:, :, 3]
    M = np.zeros((B, 2 * m, 12))
    for j in range(4):
        M[:, 0::2, 3 * j] = al[:, :, j] * fu
        M[:, 0::2, 3 * j + 2] = al[:, :, j] * (uc - us[:, :, 0])
        M[:, 1::2, 3 * j + 1] = al[:, :, j] * fv
        M[:, 1::2, 3 * j + 2] = al[:, :, j] * (vc - us[:, :, 1])
    _, V = np.linalg.eigh(np.einsum("bri,brj->bij", M, M))
    v = np.transpose(V[:, :, :4], (0, 2, 1)).copy()  # v[:, 0] smallest
    if m == MODEL_POINTS:
        g = np.hypot(v[:, 0, 0], v[:, 1, 0])
        gs = np.where(g > 0, g, 1.0)
        c, s = np.where(g > 0, v[:, 0, 0] / gs, 1.0), np.where(g > 0, v[:, 1, 0] / gs, 0.0)
        a, b = v[:, 0].copy(), v[:, 1].copy()
        v[:, 0], v[:, 1] = c[:, None] * a + s[:, None] * b, c[:, None] * b - s[:, None] * a
        v[:, 1, 0] = np.where(g > 0, 0.0, v[:, 1, 0])
    dv = np.stack([v[:, :, 3 * a:3 * a + 3] - v[:, :, 3 * b:3 * b + 3] for a, b in _PAIRS], axis=2)  # [B, 4, 6, 3]
    dot = lambda i, j: (dv[:, i] * dv[:, j]).sum(axis=2)  # noqa: E731
    L = np.stack([dot(0, 0), 2 * dot(0, 1), dot(1, 1), 2 * dot(0, 2), 2 * dot(1, 2), dot(2, 2), 2 * dot(0, 3), 2 * dot(1, 3),
                  2 * dot(2, 3), dot(3, 3)], axis=2)  # [B, 6, 10]
    rho = np.stack([((cws[:, a] - cws[:, b]) ** 2).sum(axis=1) for a, b in _PAIRS], axis=1)

    def gauss_newton(betas):
        for _ in range(5):
            b0, b1, b2, b3 = betas.T
            l = [L[:, :, k] for k in range(10)]
            A = np.stack([2 * l[0] * b0[:, None] + l[1] * b1[:, None] + l[3] * b2[:, None] + l[6] * b3[:, None],
                          l[1] * b0[:, None] + 2 * l[2] * b1[:, None] + l[4] * b2[:, None] + l[7] * b3[:, None],
                          l[3] * b0[:, None] + l[4] * b1[:, None] + 2 * l[5] * b2[:, None] + l[8] * b3[:, None],
                          l[6] * b0[:, None] + l[7] * b1[:, None] + l[8] * b2[:, None] + 2 * l[9] * b3[:, None]], axis=2)
            bb = [b0 * b0, b0 * b1, b1 * b1, b0 * b2, b1 * b2, b2 * b2, b0 * b3, b1 * b3, b2 * b3, b3 * b3]
            r = rho - sum(l[k] * bb[k][:, None] for k in range(10))
            betas = betas + _qr_solve(A, r)
        return betas

    def r_and_t(betas):
        ccs = np.einsum("bi,bijk->bjk", betas, v.reshape(B, 4, 4, 3))
        pcs = np.einsum("bij,bjk->bik", al, ccs)
        pcs = np.where((pcs[:, 0, 2] < 0)[:, None, None], -pcs, pcs)
        pc0, pw0 = pcs.mean(axis=1), pw.mean(axis=1)
        H = np.einsum("bij,bik->bjk", pcs - pc0[:, None], pw - pw0[:, None])
        bad = ~np.isfinite(H).all(axis=(1, 2))  # (LAPACK refuses non-finite input; the kernel's pose is then not finite)
        Uh, _, Vt = np.linalg.svd(np.where(bad[:, None, None], 0.0, H))
        R = np.where(bad[:, None, None], np.nan, Uh @ Vt)
        R[:, 2] = np.where((np.linalg.det(R) < 0)[:, None], -R[:, 2], R[:, 2])
        t = pc0 - np.einsum("bij,bj->bi", R, pw0)
        pc = np.einsum("bij,bmj->bmi", R, pw) + t[:, None]
        ue, ve = uc + fu * pc[:, :, 0] * (1.0 / pc[:, :, 2]), vc + fv * pc[:, :, 1] * (1.0 / pc[:, :, 2])
        err = np.sqrt((us[:, :, 0] - ue) ** 2 + (us[:, :, 1] - ve) ** 2).mean(axis=1)
        return R, t, err

    with np.errstate(all="ignore"):
        x = _qr_solve(L[:, :, [0, 1, 3, 6]], rho)  # approx 1: [B11 B12 B13 B14]
        b0 = np.sqrt(np.abs(x[:, 0]))
        sg = np.where(x[:, 0] < 0, -1.0, 1.0)
        beta1 = np.stack([b0, sg * x[:, 1] / b0, sg * x[:, 2] / b0, sg * x[:, 3] / b0], axis=1)
        x = _qr_solve(L[:, :, [0, 1, 2]], rho)  # approx 2: [B11 B12 B22]
        neg = x[:, 0] < 0
        b0 = np.sqrt(np.abs(x[:, 0]))
        b1 = np.where(neg, np.where(x[:, 2] < 0, np.sqrt(np.abs(x[:, 2])), 0.0), np.where(x[:, 2] > 0, np.sqrt(np.abs(x[:, 2])), 0.0))
        b0 = np.where(x[:, 1] < 0, -b0, b0)
        beta2 = np.stack([b0, b1, 0 * b0, 0 * b0], axis=1)
        x = _qr_solve(L[:, :, [0, 1, 2, 3, 4]], rho)  # approx 3: [B11 B12 B22 B13 B23]
        neg = x[:, 0] < 0
        b0 = np.sqrt(np.abs(x[:, 0]))
        b1 = np.where(neg, np.where(x[:, 2] < 0, np.sqrt(np.abs(x[:, 2])), 0.0), np.where(x[:, 2] > 0, np.sqrt(np.abs(x[:, 2])), 0.0))
        b0 = np.where(x[:, 1] < 0, -b0, b0)
        beta3 = np.stack([b0, b1, x[:, 3] / b0, 0 * b0], axis=1)
        best = None
        for betas in (beta1, beta2, beta3):
            R, t, err = r_and_t(gauss_newton(betas))
            if best is None:
                best = [R, t, err]
            else:
                take = err < best[2]  # ties: the lower N
                best[0] = np.where(take[:, None, None], R, best[0])
                best[1] = np.where(take[:, None], t, best[1])
                best[2] = np.where(take, err, best[2])
    return best[0], best[1]


# -------------------------------------------------------------------------------------------------------------- scoring
def reproj_err(R, t, pts3d, pts2d, cam4) -> np.ndarray:
    """computeError: projectPoints in double (no distortion), stored as float, float dx^2 + dy^2.  R [.., 3, 3], t [.., 3]"""
    fu, fv, uc, vc = (float(np.float32(c)) for c in cam4[:4])
    X = np.asarray(pts3d, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        # ((R0 X + R1 Y) + R2 Z) + t, like the kernel and cvProjectPoints2
        x = R[..., 0, 0, None] * X[:, 0] + R[..., 0, 1, None] * X[:, 1] + R[..., 0, 2, None] * X[:, 2] + t[..., 0, None]
        y = R[..., 1, 0, None] * X[:, 0] + R[..., 1, 1, None] * X[:, 1] + R[..., 1, 2, None] * X[:, 2] + t[..., 1, None]
        z = R[..., 2, 0, None] * X[:, 0] + R[..., 2, 1, None] * X[:, 1] + R[..., 2, 2, None] * X[:, 2] + t[..., 2, None]
        z = np.where(z != 0, 1.0 / np.where(z != 0, z, 1.0), 1.0)
        pu, pv = (x * z * fu + uc).astype(np.float32), (y * z * fv + vc).astype(np.float32)
        p2 = np.asarray(pts2d, np.float32)
        dx, dy = p2[:, 0] - pu, p2[:, 1] - pv
        return dx * dx + dy * dy


def inlier_counts(hyp, pts3d, pts2d, cam4, reproj_error=8.0, chunk=4) -> np.ndarray:
    """reproj_err <= the float gate, counted per hypothesis, `chunk` hypotheses at a time (memory bounded by chunk x n).
    hyp [H, 3, 4] -> int64 [H]"""
    th2 = np.float32(float(np.float32(reproj_error)) ** 2)
    hyp = np.asarray(hyp, np.float64)
    out = np.zeros(len(hyp), np.int64)
    for h0 in range(0, len(hyp), chunk):
        hc = hyp[h0:h0 + chunk]
        out[h0:h0 + chunk] = (reproj_err(hc[:, :, :3], hc[:, :, 3], pts3d, pts2d, cam4) <= th2).sum(axis=1)
    return out


def ransac_hypotheses(pts3d, pts2d, cam4, iterations) -> np.ndarray:
    """the RANSAC hypotheses [iterations, 3, 4] of a problem with n > 5 (EPnP on samples(n, iterations)); iteration k's
    depends on n alone, so a prefix of a longer run is the run with fewer iterations"""
    p3 = np.asarray(pts3d, np.float32).reshape(-1, 3).astype(np.float64)
    p2 = np.asarray(pts2d, np.float32).reshape(-1, 2).astype(np.float64)
    S = samples(len(p3), int(iterations))
    R, t = epnp(p3[S], p2[S], cam4)
    return np.concatenate([R, t[:, :, None]], axis=2)


def pnp_ransac(pts3d, pts2d, cam4, iterations=100, reproj_error=8.0, confidence=0.99, hypotheses=None):
    """The contract for one problem -> dict(status, Tcw [3, 4], inliers bool [n], n_inliers, samples, counts, hyp_Tcw,
    best_iter, final_niters).  hypotheses: [iterations, 3, 4] to replay given poses instead of solving them (the test
    feeds the device's, so that the replay and the refit are checked on the same counts)."""
    p3 = np.asarray(pts3d, np.float32).reshape(-1, 3)
    p2 = np.asarray(pts2d, np.float32).reshape(-1, 2)
    n = len(p3)
    th2 = np.float32(float(np.float32(reproj_error)) ** 2)
    out = dict(status=0, Tcw=np.zeros((3, 4)), inliers=np.zeros(n, bool), n_inliers=0, samples=None, counts=None, hyp_Tcw=None,
               best_iter=-1, final_niters=0)
    if n < MODEL_POINTS:
        return out
    niters = max(int(iterations), 1)
    if n == MODEL_POINTS:
        mask = np.ones(n, bool)
        out.update(final_niters=niters)
    else:
        S = samples(n, int(iterations))
        if hypotheses is None:
            R, t = epnp(p3.astype(np.float64)[S], p2.astype(np.float64)[S], cam4)
            hyp = np.concatenate([R, t[:, :, None]], axis=2)
        else:
            hyp = np.asarray(hypotheses, np.float64)
        counts = inlier_counts(hyp, p3, p2, cam4, reproj_error).astype(np.int32)
        best, max_good = -1, 0
        it = 0
        while it < niters:
            g = int(counts[it])
            if g > max(max_good, MODEL_POINTS - 1):
                best, max_good = it, g
                niters = ransac_update_num_iters(confidence, (n - g) / n, MODEL_POINTS, niters)
            it += 1
        out.update(samples=S, counts=counts, hyp_Tcw=hyp, best_iter=best, final_niters=niters)
        if best < 0:
            return out
        mask = reproj_err(hyp[best, :, :3], hyp[best, :, 3], p3, p2, cam4) <= th2
    R, t = epnp(p3.astype(np.float64)[mask][None], p2.astype(np.float64)[mask][None], cam4)
    if not (np.isfinite(R).all() and np.isfinite(t).all()):  # a refit that is not finite fails the problem
        out.update(inliers=np.zeros(n, bool))
        return out
    out.update(status=1, Tcw=np.concatenate([R[0], t[0][:, None]], axis=1), inliers=mask, n_inliers=int(mask.sum()))
    return out


# ------------------------------------------------------------------------------------------------------------ fixtures
CAM4 = np.array([517.3, 516.5, 318.6, 255.3], np.float32)


def random_pose(rng):
    w = rng.normal(size=3)
    w *= rng.uniform(0.05, 0.6) / np.linalg.norm(w)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx
    return R, rng.normal(0, 0.3, 3)


def make_problem(rng, n, outlier_frac=0.3, noise=0.5, cam4=CAM4, W=640, H=480):
    """n correspondences of a random pose: camera-frame points at depth 1..6 m inside the image, back to the world; a
    fraction of the 2-D points replaced by uniform pixels.  -> pts3d f32 [n, 3], pts2d f32 [n, 2], R, t, outlier mask"""
    fu, fv, uc, vc = (float(c) for c in cam4[:4])
    R, t = random_pose(rng)
    u, v = rng.uniform(0, W, n), rng.uniform(0, H, n)
    z = rng.uniform(1.0, 6.0, n)
    pc = np.stack([(u - uc) / fu * z, (v - vc) / fv * z, z], axis=1)
    pw = (pc - t) @ R  # R^T (pc - t)
    uv = np.stack([u, v], axis=1) + rng.normal(0, noise, (n, 2)) if noise > 0 else np.stack([u, v], axis=1)
    out = rng.random(n) < outlier_frac
    uv[out] = np.stack([rng.uniform(0, W, out.sum()), rng.uniform(0, H, out.sum())], axis=1)
    return pw.astype(np.float32), uv.astype(np.float32), R, t, out


# the geometry of relocalisation, which make_problem never reaches: any heading, far from the world origin, near and far
# points, fx != fy, an off-centre principal point, a second camera
CAM_VGA = np.array([521.7, 498.3, 301.9, 263.4], np.float32)  # 640 x 480, fx != fy, principal point off-centre
CAM_HD = np.array([903.6, 911.2, 652.8, 351.5], np.float32)   # 1280 x 720
WIDE_CAMS = ((CAM_VGA, 640, 480), (CAM_HD, 1280, 720))


def rotation(axis, angle) -> np.ndarray:
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * Kx @ Kx


def random_pose_wide(rng, near_pi=False, centre=(10.0, 1000.0)):
    """Tcw of any heading: rotation angle uniform in [0, pi - 1e-3], or within 1e-3 of pi (near_pi); camera centre
    |C| in `centre` metres from the world origin (t = -R C)"""
    th = rng.uniform(math.pi - 1e-3, math.pi) if near_pi else rng.uniform(0.0, math.pi - 1e-3)
    R = rotation(rng.normal(size=3), th)
    d = rng.normal(size=3)
    C = d / np.linalg.norm(d) * rng.uniform(*centre)
    return R, -R @ C


def project(p3, R, t, cam4) -> np.ndarray:
    """the pixels of float32 world points under (R, t) in double, rounded once to float32 (noise-free data: their only
    error is that rounding)"""
    fu, fv, uc, vc = (float(c) for c in cam4[:4])
    pc = np.asarray(p3, np.float32).astype(np.float64) @ R.T + t
    return np.stack([fu * pc[:, 0] / pc[:, 2] + uc, fv * pc[:, 1] / pc[:, 2] + vc], axis=1).astype(np.float32)


def make_problem_wide(rng, n, outlier_frac=0.3, noise=0.5, cam4=CAM_VGA, W=640, H=480, near_pi=False, centre=(10.0, 1000.0),
                      depth=(0.2, 80.0)):
    """make_problem on relocalisation geometry (random_pose_wide; depths log-uniform in `depth`).  noise == 0 and
    outlier_frac == 0: the pixels are project() of the float32 world points, exact up to one float32 rounding"""
    fu, fv, uc, vc = (float(c) for c in cam4[:4])
    R, t = random_pose_wide(rng, near_pi, centre)
    u, v = rng.uniform(0, W, n), rng.uniform(0, H, n)
    z = np.exp(rng.uniform(math.log(depth[0]), math.log(depth[1]), n))
    pc = np.stack([(u - uc) / fu * z, (v - vc) / fv * z, z], axis=1)
    pw = ((pc - t) @ R).astype(np.float32)
    out = rng.random(n) < outlier_frac
    if noise == 0 and not out.any():
        return pw, project(pw, R, t, cam4), R, t, out
    uv = project(pw, R, t, cam4).astype(np.float64) + rng.normal(0, noise, (n, 2))
    uv[out] = np.stack([rng.uniform(0, W, out.sum()), rng.uniform(0, H, out.sum())], axis=1)
    return pw, uv.astype(np.float32), R, t, out


def rounding_pose_bound(p3, R, t, cam4, safety=4.0):
    """A bound on |R_est - R|max and |t_est - t|max for EPnP on noise-free data whose pixels carry only their float32
    rounding (project()).  Derivation, to first order in the pixel error e (2n-vector):
      * |e_i| <= half an ulp of the pixel coordinate, so |e|_2 <= sqrt(2n) h, h = max over the pixels of ulp / 2;
      * the pose perturbation x = (w, dt') with R' = exp([w]x) R, pc' = pc + w x pc + dt' moves the pixels by J x, J the
        2n x 6 Jacobian of (fu X/Z + uc, fv Y/Z + vc) at the true pose; the reprojection least squares gives
        |x|_2 <= |e|_2 / sigma_min(J);
      * EPnP minimises an algebraic error, the reprojection residual of point i scaled by its depth Z_i: a weighted least
        squares, whose sensitivity is at most cond(W) = Z_max / Z_min times the unweighted one;
      * `safety` covers EPnP's linearisation (an unconstrained 12-vector, then betas and Procrustes) against the
        constrained 6-parameter fit above, and the second-order terms.
    Then |R' - R|max <= |w|_2 and t' - t = dt' - w x t, so |t' - t|max <= |x|_2 (1 + |t|_2).  -> (bound_R, bound_t)
    This is a worst case and it is loose: on the fixtures of test_wide_geometry_noise_free it lies 1e3 to 1e5 times
    above EPnP's actual error (sqrt(2n) h takes every pixel at its largest rounding, Z_max / Z_min the worst weighting,
    and `safety` multiplies both).  So it catches a pose that is wrong, not one that is imprecise; the kernels'
    precision is pinned by their 1e-8 agreement with epnp()."""
    fu, fv = float(cam4[0]), float(cam4[1])
    pc = np.asarray(p3, np.float32).astype(np.float64) @ R.T + t
    X, Y, Z = pc[:, 0], pc[:, 1], pc[:, 2]
    px = project(p3, R, t, cam4)
    h = float(np.spacing(np.abs(px)).max()) / 2
    du = np.stack([fu / Z, 0 * Z, -fu * X / Z ** 2], axis=1)  # d(u)/d(pc)
    dv = np.stack([0 * Z, fv / Z, -fv * Y / Z ** 2], axis=1)
    cx = np.zeros((len(Z), 3, 3))  # d(w x pc)/dw = -[pc]x
    cx[:, 0, 1], cx[:, 0, 2], cx[:, 1, 2] = Z, -Y, X
    cx[:, 1, 0], cx[:, 2, 0], cx[:, 2, 1] = -Z, Y, -X
    J = np.zeros((2 * len(Z), 6))
    J[0::2, :3], J[1::2, :3] = np.einsum("ik,ikj->ij", du, cx), np.einsum("ik,ikj->ij", dv, cx)
    J[0::2, 3:], J[1::2, 3:] = du, dv
    smin = np.linalg.svd(J, compute_uv=False)[-1]
    x = safety * (Z.max() / Z.min()) * math.sqrt(J.shape[0]) * h / smin
    return x, x * (1.0 + float(np.linalg.norm(t)))
