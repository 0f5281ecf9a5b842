"""CPU checks of tests/pnp_ref.py, the numpy restatement of the PnP RANSAC contract that
tests/test_gpu_pnp.py holds the kernels to."""
import math

import numpy as np
import pytest

import pnp_ref as pr


def _plain_mwc(n_draws):
    """cv::RNG::next in plain integers: state = low32(state) * 4164903690 + high32(state), mod 2^64"""
    st, out = 2 ** 64 - 1, []
    for _ in range(n_draws):
        lo, hi = st % 2 ** 32, st // 2 ** 32
        st = (lo * 4164903690 + hi) % 2 ** 64
        out.append(st % 2 ** 32)
    return out


def test_mwc_matches_plain_integer_form():
    st, got = pr.MASK64, []
    for _ in range(1000):
        st, r = pr.rng_next(st)
        got.append(r)
    assert got == _plain_mwc(1000)


@pytest.mark.parametrize("n", [6, 7, 50, 1000])
def test_samples_are_distinct_and_follow_the_stream(n):
    S = pr.samples(n, 100)
    assert S.shape == (100, 5) and S.min() >= 0 and S.max() < n
    assert all(len(set(r)) == 5 for r in S)
    draws = iter(_plain_mwc(100000))
    for r in S[:20]:  # getSubset: redraw an index already in the tuple
        idx = []
        while len(idx) < 5:
            c = next(draws) % n
            if c not in idx:
                idx.append(c)
        assert list(r) == idx


def test_ransac_update_num_iters_edges():
    assert pr.ransac_update_num_iters(0.99, 0.0, 5, 100) == 0  # ep = 0: 1 - 1^5 = 0 < DBL_MIN
    assert pr.ransac_update_num_iters(0.99, 1.0, 5, 100) == 100  # ep = 1: denom = 1, log = 0 >= 0
    assert pr.ransac_update_num_iters(0.99, 1.5, 5, 100) == 100  # clamped to 1
    # denom >= 0 branch versus the rounded quotient
    ep = 0.3
    want = math.log(0.01) / math.log(1 - 0.7 ** 5)
    assert pr.ransac_update_num_iters(0.99, ep, 5, 100) == int(np.rint(want)) < 100
    assert pr.ransac_update_num_iters(0.99, 0.9, 5, 100) == 100  # -num >= maxIters * -denom
    # p = 1: num = log(DBL_MIN), the quotient exceeds max_iters -> max_iters
    assert pr.ransac_update_num_iters(1.0, 0.3, 5, 100) == 100
    # only shrinks: the result never exceeds max_iters
    for e in np.linspace(0, 1, 41):
        assert pr.ransac_update_num_iters(0.99, float(e), 5, 37) <= 37


@pytest.mark.parametrize("m", [5, 6, 12, 200])
def test_epnp_noise_free_recovers_the_pose(m):
    rng = np.random.default_rng(m)
    pws, uss, Rs, ts = [], [], [], []
    for _ in range(8):
        p3, p2, R, t, _ = pr.make_problem(rng, m, outlier_frac=0.0, noise=0.0)
        # exact pixels of the float-rounded world points, so that the data are noise-free in double
        pc = p3.astype(np.float64) @ R.T + t
        uv = np.stack([pr.CAM4[0] * pc[:, 0] / pc[:, 2] + pr.CAM4[2], pr.CAM4[1] * pc[:, 1] / pc[:, 2] + pr.CAM4[3]], axis=1)
        pws.append(p3.astype(np.float64)), uss.append(uv), Rs.append(R), ts.append(t)
    R, t = pr.epnp(np.stack(pws), np.stack(uss), pr.CAM4.astype(np.float64))
    assert np.abs(R - np.stack(Rs)).max() <= 1e-9
    assert np.abs(t - np.stack(ts)).max() <= 1e-9


def test_epnp_with_noise_lands_near_the_reprojection_minimum():
    least_squares = pytest.importorskip("scipy.optimize").least_squares
    rng = np.random.default_rng(7)
    fu, fv, uc, vc = (float(c) for c in pr.CAM4)
    for _ in range(4):
        p3, p2, Rt, tt, _ = pr.make_problem(rng, 150, outlier_frac=0.0, noise=1.0)
        R, t = pr.epnp(p3.astype(np.float64)[None], p2.astype(np.float64)[None], pr.CAM4)
        R, t = R[0], t[0]

        def rodrigues(w):
            th = np.linalg.norm(w)
            if th < 1e-15:
                return np.eye(3)
            k = w / th
            K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
            return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K

        def resid(x):
            pc = p3.astype(np.float64) @ rodrigues(x[:3]).T + x[3:]
            return np.concatenate([fu * pc[:, 0] / pc[:, 2] + uc - p2[:, 0], fv * pc[:, 1] / pc[:, 2] + vc - p2[:, 1]])

        # start the minimiser at the true pose (independent of EPnP)
        ang = math.acos(max(-1.0, min(1.0, (np.trace(Rt) - 1) / 2)))
        w0 = np.array([Rt[2, 1] - Rt[1, 2], Rt[0, 2] - Rt[2, 0], Rt[1, 0] - Rt[0, 1]]) * (ang / (2 * math.sin(ang)))
        sol = least_squares(resid, np.concatenate([w0, tt]), method="lm", xtol=1e-14, ftol=1e-14)
        Rm, tm = rodrigues(sol.x[:3]), sol.x[3:]
        assert np.abs(R - Rm).max() < 5e-3 and np.abs(t - tm).max() < 5e-3
        pc = p3.astype(np.float64) @ R.T + t
        r = np.concatenate([fu * pc[:, 0] / pc[:, 2] + uc - p2[:, 0], fv * pc[:, 1] / pc[:, 2] + vc - p2[:, 1]])
        assert np.sqrt(np.mean(r ** 2)) <= 1.05 * np.sqrt(np.mean(sol.fun ** 2))


def test_ransac_finds_the_pose_through_outliers():
    rng = np.random.default_rng(3)
    p3, p2, R, t, out = pr.make_problem(rng, 200, outlier_frac=0.3, noise=0.5)
    res = pr.pnp_ransac(p3, p2, pr.CAM4)
    assert res["status"] == 1 and res["best_iter"] >= 0 and res["final_niters"] <= 100
    assert np.abs(res["Tcw"][:, :3] - R).max() < 1e-2 and np.abs(res["Tcw"][:, 3] - t).max() < 2e-2
    assert not res["inliers"][out].any() or res["inliers"][out].mean() < 0.05
    assert res["inliers"][~out].mean() > 0.95
    # the replay's choice: the first iteration whose count beats max(maxGood, 4) and is the largest before niters
    c = res["counts"]
    assert c[res["best_iter"]] == res["inliers"].sum()


def test_small_and_degenerate_sizes():
    rng = np.random.default_rng(4)
    p3, p2, *_ = pr.make_problem(rng, 5, outlier_frac=0.0, noise=0.0)
    r5 = pr.pnp_ransac(p3, p2, pr.CAM4)
    assert r5["status"] == 1 and r5["n_inliers"] == 5 and r5["best_iter"] == -1
    for n in (0, 1, 4):
        r = pr.pnp_ransac(p3[:n], p2[:n], pr.CAM4)
        assert r["status"] == 0 and r["n_inliers"] == 0
    # all outliers: no hypothesis beats 4
    p3, p2, *_ = pr.make_problem(rng, 60, outlier_frac=1.0, noise=0.0)
    r = pr.pnp_ransac(p3, p2, pr.CAM4)
    assert r["status"] == 0 and r["best_iter"] == -1


def test_degenerate_sets_give_finite_poses_or_fail():
    """coplanar / collinear / coincident world points: no LAPACK error, and a found pose is finite (a refit that is not
    finite fails the problem with no inliers)"""
    rng = np.random.default_rng(41)
    for kind in ("plane", "line", "point", "plane", "plane"):
        p3, p2, R, t, _ = pr.make_problem(rng, 80, outlier_frac=0.2, noise=0.3)
        if kind == "plane":
            p3[:, 2] = np.float32(2.0)
        elif kind == "line":
            p3[:, 1:] = p3[:, :1]
        else:
            p3[:] = p3[0]
        r = pr.pnp_ransac(p3, p2, pr.CAM4)
        if r["status"] == 1:
            assert np.isfinite(r["Tcw"]).all() and r["n_inliers"] == r["inliers"].sum() > 4
        else:
            assert r["n_inliers"] == 0 and not r["inliers"].any()


@pytest.mark.parametrize("cam_i", [0, 1])
def test_epnp_wide_geometry_recovers_the_pose(cam_i):
    """any heading (within 1e-3 of pi too), 10-1000 m from the origin, depths 0.2-80 m, fx != fy, off-centre principal
    points: noise-free data recover the true pose within the float32 pixel-rounding bound of rounding_pose_bound"""
    rng = np.random.default_rng(200 + cam_i)
    cam, W, H = pr.WIDE_CAMS[cam_i]
    for i, m in enumerate((5, 6, 7, 12, 40, 300, 2000)):
        for near_pi in (False, True):
            p3, p2, R, t, _ = pr.make_problem_wide(rng, m, outlier_frac=0.0, noise=0.0, cam4=cam, W=W, H=H, near_pi=near_pi)
            Re, te = pr.epnp(p3.astype(np.float64)[None], p2.astype(np.float64)[None], cam)
            bR, bt = pr.rounding_pose_bound(p3, R, t, cam)
            assert np.abs(Re[0] - R).max() <= bR and np.abs(te[0] - t).max() <= bt, (m, near_pi)
    # the generator's promises
    R, t = pr.random_pose_wide(rng, near_pi=True)
    assert math.acos(max(-1.0, min(1.0, (np.trace(R) - 1) / 2))) > math.pi - 2e-3 and 10 <= np.linalg.norm(R.T @ t) <= 1000


def test_epnp_wide_geometry_lands_near_the_reprojection_minimum():
    """any heading, far from the origin, both cameras, at the depths of make_problem (1-6 m).  (At depths of 0.2-80 m
    EPnP's algebraic error, the pixel residual scaled by depth, is far from the reprojection minimum under 1 px of noise:
    4-27 px RMS against 1 px.  That is EPnP, not the restatement; the noise-free test above covers that range.)"""
    least_squares = pytest.importorskip("scipy.optimize").least_squares
    rng = np.random.default_rng(17)
    for i in range(6):
        cam, W, H = pr.WIDE_CAMS[i % 2]
        fu, fv, uc, vc = (float(c) for c in cam)
        p3, p2, Rt, tt, _ = pr.make_problem_wide(rng, 200, outlier_frac=0.0, noise=1.0, cam4=cam, W=W, H=H, near_pi=i % 3 == 0,
                                               depth=(1.0, 6.0))
        R, t = pr.epnp(p3.astype(np.float64)[None], p2.astype(np.float64)[None], cam)
        R, t = R[0], t[0]
        X = p3.astype(np.float64)

        def resid(x, R0=Rt, t0=tt):  # the pose as a small rotation and translation about the true one
            pc = X @ (pr.rotation(x[:3], np.linalg.norm(x[:3])) if np.linalg.norm(x[:3]) > 0 else np.eye(3)).dot(R0).T + t0 + x[3:]
            return np.concatenate([fu * pc[:, 0] / pc[:, 2] + uc - p2[:, 0], fv * pc[:, 1] / pc[:, 2] + vc - p2[:, 1]])

        sol = least_squares(resid, np.zeros(6), method="lm", xtol=1e-15, ftol=1e-15)
        w = sol.x[:3]
        Rm = (pr.rotation(w, np.linalg.norm(w)) if np.linalg.norm(w) > 0 else np.eye(3)) @ Rt
        tm = tt + sol.x[3:]
        tscale = max(1.0, float(np.linalg.norm(tt)))
        assert np.abs(R - Rm).max() < 5e-3 and np.abs(t - tm).max() < 5e-3 * tscale, i
        pc = X @ R.T + t
        r = np.concatenate([fu * pc[:, 0] / pc[:, 2] + uc - p2[:, 0], fv * pc[:, 1] / pc[:, 2] + vc - p2[:, 1]])
        assert np.sqrt(np.mean(r ** 2)) <= 1.1 * np.sqrt(np.mean(sol.fun ** 2)), i  # (the 1280 x 720 camera: up to 1.055)


def test_ransac_wide_geometry_finds_the_pose_through_outliers():
    rng = np.random.default_rng(19)
    for i in range(4):
        cam, W, H = pr.WIDE_CAMS[i % 2]
        p3, p2, R, t, out = pr.make_problem_wide(rng, 300, outlier_frac=0.3, noise=0.5, cam4=cam, W=W, H=H, near_pi=i % 2 == 1)
        res = pr.pnp_ransac(p3, p2, cam)
        assert res["status"] == 1
        assert np.abs(res["Tcw"][:, :3] - R).max() < 1e-2 and np.abs(res["Tcw"][:, 3] - t).max() < 1e-2 * max(1.0, np.linalg.norm(t))
        assert res["inliers"][~out].mean() > 0.9


def test_chunked_counts_equal_the_full_replay():
    rng = np.random.default_rng(23)
    p3, p2, *_ = pr.make_problem(rng, 3000)
    hyp = pr.ransac_hypotheses(p3, p2, pr.CAM4, 37)
    for g in (0.5, 8.0, 30.0):
        full = (pr.reproj_err(hyp[:, :, :3], hyp[:, :, 3], p3, p2, pr.CAM4) <= np.float32(np.float32(g) ** 2)).sum(axis=1)
        assert np.array_equal(pr.inlier_counts(hyp, p3, p2, pr.CAM4, g, chunk=5), full)
    ref = pr.pnp_ransac(p3, p2, pr.CAM4, iterations=37)
    assert np.array_equal(pr.pnp_ransac(p3, p2, pr.CAM4, iterations=37, hypotheses=hyp)["counts"], ref["counts"])
