"""vo_pnp_ransac / vo_pnp_ransac_dev against tests/pnp_ref.py (the contract of DESIGN.md §4c): samples bit-exact,
hypothesis poses to 1e-9, counts / masks / chosen iteration / final niters exact, refit to 1e-8, ragged batches,
host and device forms bit for bit, capacity errors."""
import numpy as np
import pytest

import pnp_ref as pr

pytestmark = pytest.mark.gpu

CAM = pr.CAM4


def _exact_pixels(p3, R, t):
    pc = p3.astype(np.float64) @ R.T + t
    return np.stack([CAM[0] * pc[:, 0] / pc[:, 2] + CAM[2], CAM[1] * pc[:, 1] / pc[:, 2] + CAM[3]], axis=1).astype(np.float32)


def _rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


@pytest.mark.parametrize("n", [5, 6, 7, 50, 1000])
def test_samples_bit_exact(vo, n):
    rng = np.random.default_rng(n)
    p3, p2, *_ = pr.make_problem(rng, n)
    res = vo.pnp_ransac([(p3, p2)], CAM, diagnostics=True)
    if n == 5:
        assert not res["samples"].any() and res["best_iter"][0] == -1
    else:
        assert np.array_equal(res["samples"][0], pr.samples(n, 100))


def test_hypothesis_poses_on_all_inlier_samples(vo):
    rng = np.random.default_rng(11)
    probs = []
    for n in (6, 9, 40, 300):
        p3, _, R, t, _ = pr.make_problem(rng, n, outlier_frac=0.0, noise=0.0)
        probs.append((p3, _exact_pixels(p3, R, t)))
    res = vo.pnp_ransac(probs, CAM, diagnostics=True)
    for k, (p3, p2) in enumerate(probs):
        S = pr.samples(len(p3), 100)
        R, t = pr.epnp(p3.astype(np.float64)[S], p2.astype(np.float64)[S], CAM)
        want = np.concatenate([R, t[:, :, None]], axis=2)
        got = res["hyp_Tcw"][k]
        for h in range(100):
            assert _rel(got[h], want[h]) <= 1e-9, (k, h)
        assert res["n_inliers"][k] == len(p3) and res["status"][k] == 1


def _margin_ok(p3, p2, ref):
    """every evaluated hypothesis keeps each residual 1e-3 px^2 away from the gate (64)"""
    if ref["hyp_Tcw"] is None:
        return True
    hyp = ref["hyp_Tcw"]
    err = pr.reproj_err(hyp[:, :, :3], hyp[:, :, 3], p3, p2, CAM)
    err2 = pr.reproj_err(ref["Tcw"][None, :, :3], ref["Tcw"][None, :, 3], p3, p2, CAM)
    return not (np.abs(err - 64.0) < 1e-3).any() and not (np.abs(err2 - 64.0) < 1e-3).any()


def _fixtures(seed, sizes, outlier_frac=0.3, noise=0.7):
    rng = np.random.default_rng(seed)
    probs, refs = [], []
    while len(probs) < len(sizes):
        n = sizes[len(probs)]
        p3, p2, *_ = pr.make_problem(rng, n, outlier_frac=outlier_frac, noise=noise)
        ref = pr.pnp_ransac(p3, p2, CAM)
        if _margin_ok(p3, p2, ref):
            probs.append((p3, p2)), refs.append(ref)
    return probs, refs


def test_counts_masks_replay_and_refit(vo):
    probs, refs = _fixtures(5, [6, 8, 12, 30, 50, 80, 150, 400, 1000, 3000] * 2)
    res = vo.pnp_ransac(probs, CAM, diagnostics=True)
    for k, ((p3, p2), ref) in enumerate(zip(probs, refs)):
        assert np.array_equal(res["counts"][k], ref["counts"]), k
        assert res["best_iter"][k] == ref["best_iter"] and res["final_niters"][k] == ref["final_niters"], k
        assert res["status"][k] == ref["status"] and res["n_inliers"][k] == ref["n_inliers"], k
        assert np.array_equal(res["inliers"][k], ref["inliers"]), k
        if ref["status"] == 1:
            assert _rel(res["Tcw"][k], ref["Tcw"]) <= 1e-8, k
        # the replay and the mask exactly, on the device's own hypotheses
        rep = pr.pnp_ransac(p3, p2, CAM, hypotheses=res["hyp_Tcw"][k])
        assert np.array_equal(rep["counts"], res["counts"][k]) and rep["best_iter"] == res["best_iter"][k]
        assert rep["final_niters"] == res["final_niters"][k] and np.array_equal(rep["inliers"], res["inliers"][k])


def test_ragged_batch_host_and_device_forms(vo):
    import torch
    rng = np.random.default_rng(21)
    sizes = [0, 4, 5, 6, 7, 1, 5, 60, 200, 0, 33]
    sizes += list(rng.integers(0, 400, 2048 - len(sizes)))
    probs = []
    for i, n in enumerate(sizes):
        frac = 1.0 if i == 7 else 0.3  # problem 7: every correspondence an outlier
        p3, p2, R, t, _ = pr.make_problem(rng, int(n), outlier_frac=frac)
        if n == 5:
            p2 = _exact_pixels(p3, R, t)
        probs.append((p3, p2))
    res = vo.pnp_ransac(probs, CAM, diagnostics=True)
    st, ni = res["status"], res["n_inliers"]
    for k, n in enumerate(sizes):
        if n < 5:
            assert st[k] == 0 and ni[k] == 0 and not res["Tcw"][k].any()
        elif n == 5:
            assert st[k] == 1 and ni[k] == 5 and res["best_iter"][k] == -1
            R, t = pr.epnp(probs[k][0].astype(np.float64)[None], probs[k][1].astype(np.float64)[None], CAM)
            assert _rel(res["Tcw"][k], np.concatenate([R[0], t[0][:, None]], axis=1)) <= 1e-8
    assert st[7] == 0 and res["best_iter"][7] == -1 and ni[7] == 0
    # a spot check of the whole contract on a few members of the batch
    for k in (3, 4, 8, 10, 100, 2047):
        p3, p2 = probs[k]
        rep = pr.pnp_ransac(p3, p2, CAM, hypotheses=res["hyp_Tcw"][k])
        assert rep["best_iter"] == res["best_iter"][k] and np.array_equal(rep["inliers"], res["inliers"][k])
    # the device form on the same arrays: bit for bit
    off = np.zeros(len(sizes) + 1, np.int32)
    off[1:] = np.cumsum(sizes)
    N, P = int(off[-1]), len(sizes)
    d = torch.device("cuda")
    p3 = torch.from_numpy(np.concatenate([a for a, _ in probs])).to(d)
    p2 = torch.from_numpy(np.concatenate([b for _, b in probs])).to(d)
    T = torch.zeros(P, 12, dtype=torch.float64, device=d)
    m = torch.zeros(N, dtype=torch.uint8, device=d)
    ni_d, st_d = torch.zeros(P, dtype=torch.int32, device=d), torch.zeros(P, dtype=torch.int32, device=d)
    diag = dict(counts=torch.zeros(P, 100, dtype=torch.int32, device=d), hyp_Tcw12=torch.zeros(P, 100, 12, dtype=torch.float64, device=d))
    stream = torch.cuda.current_stream().cuda_stream
    vo.pnp_ransac_dev(P, torch.from_numpy(off).to(d), p3, p2, CAM, T, m, ni_d, st_d, diag=diag, stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(T.cpu().numpy().view(np.uint64), res["Tcw"].reshape(P, 12).view(np.uint64))
    assert np.array_equal(m.cpu().numpy().astype(bool), np.concatenate(res["inliers"]))
    assert np.array_equal(ni_d.cpu().numpy(), ni) and np.array_equal(st_d.cpu().numpy(), st)
    assert np.array_equal(diag["counts"].cpu().numpy(), res["counts"])
    assert np.array_equal(diag["hyp_Tcw12"].cpu().numpy().view(np.uint64), res["hyp_Tcw"].reshape(P, 100, 12).view(np.uint64))


def test_pose6_is_the_se3_log(vo):
    probs, refs = _fixtures(9, [120])
    res = vo.pnp_ransac(probs, CAM)
    T = res["Tcw"][0]
    assert np.abs(res["pose6"][0] - vo.se3_log(T[:, :3], T[:, 3])).max() == 0.0


def test_capacity_and_invalid_arguments(vo):
    import ctypes as C
    L = vo.lib()
    cam = np.ascontiguousarray(CAM)
    T, ni, st = np.zeros(12), np.zeros(1, np.int32), np.zeros(1, np.int32)
    off = np.array([0, 0], np.int32)
    f, d = C.c_float(8.0), C.c_double(0.99)
    assert L.vo_pnp_ransac(1, vo._p(off), None, None, vo._p(cam), 1001, f, d, vo._p(T), None, None, vo._p(ni), vo._p(st), None) == -4
    assert L.vo_pnp_ransac(65537, vo._p(np.zeros(65538, np.int32)), None, None, vo._p(cam), 1, f, d, vo._p(np.zeros(12 * 65537)), None,
                           None, vo._p(np.zeros(65537, np.int32)), vo._p(np.zeros(65537, np.int32)), None) == -4
    assert L.vo_pnp_ransac(1, vo._p(off), None, None, vo._p(cam), 100, f, C.c_double(1.0), vo._p(T), None, None, vo._p(ni), vo._p(st), None) == -1
    big = np.array([0, (1 << 20) + 1], np.int32)
    assert L.vo_pnp_ransac(1, vo._p(big), None, None, vo._p(cam), 100, f, d, vo._p(T), None, None, vo._p(ni), vo._p(st), None) == -4
    with pytest.raises(vo.VoError):
        vo.pnp_ransac([(np.zeros((3, 3), np.float32), np.zeros((3, 2), np.float32))] * 30000, CAM, iterations=100)


def test_device_form_two_streams_with_their_own_workspaces(vo):
    """two _dev calls in flight at once on two streams of one host thread: each has its own workspace and matches the host
    form bit for bit"""
    import torch
    d = torch.device("cuda")
    sets = [_fixtures(31, [200] * 64, noise=0.7)[0], _fixtures(32, [90] * 96, noise=0.7)[0]]
    want = [vo.pnp_ransac(s, CAM) for s in sets]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for s, stm in zip(sets, streams):
        P = len(s)
        off = np.zeros(P + 1, np.int32)
        off[1:] = np.cumsum([len(a) for a, _ in s])
        with torch.cuda.stream(stm):
            p3 = torch.from_numpy(np.concatenate([a for a, _ in s])).to(d, non_blocking=False)
            p2 = torch.from_numpy(np.concatenate([b for _, b in s])).to(d)
            o = dict(off=torch.from_numpy(off).to(d), T=torch.zeros(P, 12, dtype=torch.float64, device=d),
                     m=torch.zeros(int(off[-1]), dtype=torch.uint8, device=d), ni=torch.zeros(P, dtype=torch.int32, device=d),
                     st=torch.zeros(P, dtype=torch.int32, device=d),
                     ws=torch.empty(vo.pnp_workspace_bytes(P), dtype=torch.uint8, device=d), p3=p3, p2=p2)
        outs.append(o)
    torch.cuda.synchronize()
    for s, stm, o in zip(sets, streams, outs):  # both enqueued before either is waited for
        vo.pnp_ransac_dev(len(s), o["off"], o["p3"], o["p2"], CAM, o["T"], o["m"], o["ni"], o["st"], workspace=o["ws"],
                          stream=stm.cuda_stream)
    torch.cuda.synchronize()
    for s, o, w in zip(sets, outs, want):
        P = len(s)
        assert np.array_equal(o["T"].cpu().numpy().view(np.uint64), w["Tcw"].reshape(P, 12).view(np.uint64))
        assert np.array_equal(o["m"].cpu().numpy().astype(bool), np.concatenate(w["inliers"]))
        assert np.array_equal(o["ni"].cpu().numpy(), w["n_inliers"]) and np.array_equal(o["st"].cpu().numpy(), w["status"])
    # a workspace smaller than vo_pnp_workspace_bytes is refused (VO_ERR_CAPACITY), nothing enqueued
    o, P = outs[0], len(sets[0])
    small = torch.empty(vo.pnp_workspace_bytes(P) - 1, dtype=torch.uint8, device=d)
    with pytest.raises(vo.VoError, match="status -4"):
        vo.pnp_ransac_dev(P, o["off"], o["p3"], o["p2"], CAM, o["T"], o["m"], o["ni"], o["st"], workspace=small)


def test_degenerate_point_sets_give_finite_poses_or_fail(vo):
    """coplanar, collinear and coincident world points: CC^-1 is the pseudo-inverse, so a found pose is finite; a refit
    that is not finite fails the problem with no inliers"""
    rng = np.random.default_rng(41)
    probs = []
    for kind in ("plane", "line", "point", "plane", "plane"):
        p3, p2, R, t, _ = pr.make_problem(rng, 80, outlier_frac=0.2, noise=0.3)
        if kind == "plane":
            p3[:, 2] = np.float32(2.0)
        elif kind == "line":
            p3[:, 1:] = p3[:, :1]
        else:
            p3[:] = p3[0]
        probs.append((p3, _exact_pixels(p3, R, t) if kind == "plane" else p2))
    res = vo.pnp_ransac(probs, CAM, diagnostics=True)
    for k in range(len(probs)):
        if res["status"][k] == 1:
            assert np.isfinite(res["Tcw"][k]).all() and res["n_inliers"][k] == res["inliers"][k].sum() > 4
        else:
            assert res["n_inliers"][k] == 0 and not res["inliers"][k].any() and not res["Tcw"][k].any()
