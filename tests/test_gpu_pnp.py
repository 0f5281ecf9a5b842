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


def _margin_ok(p3, p2, ref, gates=(8.0,), cam=CAM):
    """every evaluated hypothesis keeps each residual away from each gate g^2: 1e-3 px^2 at g = 8 (64), scaled by g / 8
    elsewhere (a pixel coordinate's float rounding moves err = d^2 by about 2 d ulp, so the gap that can flip a residual
    grows with d = g)"""
    if ref["hyp_Tcw"] is None:
        return True
    hyp = np.concatenate([ref["hyp_Tcw"], ref["Tcw"][None]])
    for h0 in range(0, len(hyp), 8):
        err = pr.reproj_err(hyp[h0:h0 + 8, :, :3], hyp[h0:h0 + 8, :, 3], p3, p2, cam)
        for g in gates:
            th2 = float(np.float32(float(np.float32(g)) ** 2))
            if (np.abs(err - th2) < 1e-3 * g / 8.0).any():
                return False
    return True


def _fixtures(seed, sizes, outlier_frac=0.3, noise=0.7, make=pr.make_problem, cam=CAM, **kw):
    rng = np.random.default_rng(seed)
    probs, refs = [], []
    while len(probs) < len(sizes):
        n = sizes[len(probs)]
        p3, p2, *_ = make(rng, n, outlier_frac=outlier_frac, noise=noise, **kw)
        ref = pr.pnp_ransac(p3, p2, cam)
        if _margin_ok(p3, p2, ref, cam=cam):
            probs.append((p3, p2)), refs.append(ref)
    return probs, refs


def _check_contract(vo, probs, refs, res, cam=CAM, **params):
    """the whole contract per problem: counts, chosen iteration, final niters, status, mask exactly; refit <= 1e-8; and
    the replay of the device's own hypotheses exactly"""
    for k, ((p3, p2), ref) in enumerate(zip(probs, refs)):
        if ref["samples"] is not None:
            assert np.array_equal(res["samples"][k], ref["samples"]), k
            assert np.array_equal(res["counts"][k], ref["counts"]), k
        assert res["best_iter"][k] == ref["best_iter"] and res["final_niters"][k] == ref["final_niters"], k
        assert res["status"][k] == ref["status"] and res["n_inliers"][k] == ref["n_inliers"], k
        assert np.array_equal(res["inliers"][k], ref["inliers"]), k
        if ref["status"] == 1:
            assert _rel(res["Tcw"][k], ref["Tcw"]) <= 1e-8, k
        rep = pr.pnp_ransac(p3, p2, cam, hypotheses=res["hyp_Tcw"][k], **params)
        if rep["counts"] is not None:
            assert np.array_equal(rep["counts"], res["counts"][k]), k
        assert rep["best_iter"] == res["best_iter"][k] and rep["final_niters"] == res["final_niters"][k], k
        assert np.array_equal(rep["inliers"], res["inliers"][k]), k


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
    # parameters outside the contract: VO_ERR_INVALID (-1)
    p3, p2 = np.zeros((8, 3), np.float32), np.zeros((8, 2), np.float32)
    off8, m8 = np.array([0, 8], np.int32), np.zeros(8, np.uint8)

    def call(P=1, offs=off8, iters=100, reproj=8.0, conf=0.99):
        return L.vo_pnp_ransac(P, vo._p(offs), vo._p(p3), vo._p(p2), vo._p(cam), iters, C.c_float(reproj), C.c_double(conf),
                               vo._p(T), None, vo._p(m8), vo._p(ni), vo._p(st), None)
    for kw in (dict(iters=0), dict(iters=-3), dict(reproj=float("nan")), dict(reproj=-1.0), dict(conf=0.0),
               dict(conf=float("nan"))):
        assert call(**kw) == -1, kw
    T2, ni2, st2 = np.zeros(24), np.zeros(2, np.int32), np.zeros(2, np.int32)
    for offs in (np.array([0, 8, 5], np.int32), np.array([2, 5, 8], np.int32)):  # decreasing; offsets[0] != 0
        assert L.vo_pnp_ransac(2, vo._p(offs), vo._p(p3), vo._p(p2), vo._p(cam), 100, f, d, vo._p(T2), None, vo._p(m8), vo._p(ni2),
                               vo._p(st2), None) == -1, offs
    # P = 0: VO_OK, nothing written (host and device forms)
    T.fill(3.5), ni.fill(7), st.fill(7), m8.fill(9)
    assert call(P=0) == 0 and (T == 3.5).all() and ni[0] == 7 and st[0] == 7 and (m8 == 9).all()
    import torch
    dev = torch.device("cuda")
    Td, nd, sd, md = (torch.full((k,), 7, dtype=dt, device=dev) for k, dt in ((12, torch.float64), (1, torch.int32), (1, torch.int32),
                                                                             (8, torch.uint8)))
    vo.pnp_ransac_dev(0, torch.zeros(1, dtype=torch.int32, device=dev), torch.from_numpy(p3).to(dev), torch.from_numpy(p2).to(dev), CAM,
                      Td, md, nd, sd, workspace=torch.empty(1, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    assert (Td == 7).all() and (nd == 7).all() and (sd == 7).all() and (md == 7).all()


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


# ------------------------------------------------------------------------------------------- batch-composition invariance
_BITS = ("samples", "counts", "hyp_Tcw", "best_iter", "final_niters", "Tcw", "n_inliers", "status")


def _member(res, k):
    return {key: np.ascontiguousarray(res[key][k]) for key in _BITS} | {"inliers": res["inliers"][k]}


def _same_bits(a, b):
    for key in _BITS:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        if x.dtype == np.float64:
            x, y = x.view(np.uint64), y.view(np.uint64)
        if not np.array_equal(x, y):
            return key
    return None if np.array_equal(a["inliers"], b["inliers"]) else "inliers"


def _invariance_problems(seed):
    """24 problems of 6 .. 3000 correspondences whose Jacobi sweeps end at different counts: ordinary scenes, exactly
    coplanar ones, noise-free ones, scenes far from the origin and turned by nearly pi, an all-outlier set"""
    rng = np.random.default_rng(seed)
    probs = []
    for n in (6, 7, 9, 13, 30, 64, 150, 400, 1000, 3000):
        probs.append(pr.make_problem(rng, n)[:2])
    for n in (40, 300, 2000):  # coplanar
        p3, _, R, t, _ = pr.make_problem(rng, n, outlier_frac=0.0, noise=0.0)
        p3[:, 2] = np.float32(2.0)
        probs.append((p3, _exact_pixels(p3, R, t)))
    for n in (8, 80, 800, 2500, 12, 500, 50, 1200):  # far from the origin; noise-free; turned by nearly pi
        kw = dict(outlier_frac=0.0, noise=0.0) if n in (12, 500) else {}
        probs.append(pr.make_problem_wide(rng, n, cam4=CAM, near_pi=n in (50, 1200), **kw)[:2])
    probs.append(pr.make_problem(rng, 100, outlier_frac=1.0)[:2])
    p3, _, R, t, _ = pr.make_problem(rng, 5, outlier_frac=0.0, noise=0.0)
    probs.append((p3, _exact_pixels(p3, R, t)))
    probs.append(pr.make_problem(rng, 4)[:2])
    return probs


@pytest.mark.parametrize("iters", [100, 7, 13, 1])
def test_results_do_not_depend_on_batch_composition(vo, iters):
    """a problem's every output bit is the same alone, in a batch, in a permuted batch and between other problems: the
    EPnP kernel packs 4 solves per workgroup (refit: 4 problems; iterations % 4 != 0: hypotheses of two problems)"""
    probs = _invariance_problems(61)
    fill = _invariance_problems(62)
    P = len(probs)
    alone = [_member(vo.pnp_ransac([p], CAM, iterations=iters, diagnostics=True), 0) for p in probs]
    perm = np.random.default_rng(iters).permutation(P)
    batch = vo.pnp_ransac(probs, CAM, iterations=iters, diagnostics=True)
    permuted = vo.pnp_ransac([probs[i] for i in perm], CAM, iterations=iters, diagnostics=True)
    mixed = []  # each problem at a different slot between fillers
    for k, p in enumerate(probs):
        mixed += [fill[(k + j) % len(fill)] for j in range(1 + k % 3)] + [p]
    where = np.cumsum([1 + k % 3 + 1 for k in range(P)]) - 1
    inter = vo.pnp_ransac(mixed, CAM, iterations=iters, diagnostics=True)
    bad = []
    for k in range(P):
        for name, res, j in (("batch", batch, k), ("permuted", permuted, int(np.where(perm == k)[0][0])), ("interleaved", inter, int(where[k]))):
            key = _same_bits(alone[k], _member(res, j))
            if key:
                bad.append((k, len(probs[k][0]), name, key))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------- parameter sweep
_SWEEP_GATES = (0.5, 2.0, 8.0, 30.0)
_SWEEP_CACHE = {}


def _sweep_set(max_iters):
    """a ragged batch with pnp_ref's own hypotheses for max_iters iterations (a prefix is the run with fewer), whose
    residuals keep the margin from every gate of the sweep"""
    if max_iters not in _SWEEP_CACHE:
        rng = np.random.default_rng(70 + max_iters)
        sizes = [6, 9, 20, 64, 150, 400] if max_iters <= 100 else [6, 9, 40, 150, 700, 2000]
        gates = _SWEEP_GATES if max_iters <= 100 else (8.0,)
        out = []
        while len(out) < len(sizes):
            p3, p2, *_ = pr.make_problem(rng, sizes[len(out)], outlier_frac=0.3, noise=0.7)
            hyp = pr.ransac_hypotheses(p3, p2, CAM, max_iters)
            ref = pr.pnp_ransac(p3, p2, CAM, iterations=max_iters, hypotheses=hyp)
            if _margin_ok(p3, p2, ref, gates):
                out.append((p3, p2, hyp))
        _SWEEP_CACHE[max_iters] = out
    return _SWEEP_CACHE[max_iters]


def _sweep(vo, iters, reproj, conf, max_iters):
    data = _sweep_set(max_iters)
    probs = [(p3, p2) for p3, p2, _ in data]
    kw = dict(iterations=iters, reproj_error=reproj, confidence=conf)
    refs = [pr.pnp_ransac(p3, p2, CAM, hypotheses=hyp[:iters], **kw) for p3, p2, hyp in data]
    res = vo.pnp_ransac(probs, CAM, diagnostics=True, **kw)
    _check_contract(vo, probs, refs, res, **kw)
    return res


@pytest.mark.parametrize("iters", [1, 2, 7, 64, 255, 256, 257, 1000])
def test_iterations_sweep(vo, iters):
    """the counters beyond 256, iterations % 4 != 0, one and two iterations, the capacity of 1000"""
    _sweep(vo, iters, 8.0, 0.99, 1000)


@pytest.mark.parametrize("reproj,conf", [(0.5, 0.99), (2.0, 0.99), (30.0, 0.99), (8.0, 0.5), (8.0, 0.9), (8.0, 0.999999),
                                         (2.0, 0.999999), (30.0, 0.5), (0.5, 0.9)])
def test_gate_and_confidence_sweep(vo, reproj, conf):
    """other float gates, and RANSACUpdateNumIters (device pow / log / rint) at other confidences: final niters exact"""
    _sweep(vo, 100, reproj, conf, 100)


# ----------------------------------------------------------------------------------------- sizes at the scoring edges
def test_sizes_at_the_scoring_kernels_edges(vo):
    """64-lane ballots, LDS chunks of 2048, and sizes far beyond the fixtures"""
    sizes = [63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 4095, 4096, 4097, 20000, 262144]
    probs, refs = _fixtures(81, sizes)
    res = vo.pnp_ransac(probs, CAM, diagnostics=True)
    _check_contract(vo, probs, refs, res)


@pytest.mark.timeout(600)
def test_max_points_problem_through_the_host_form(vo):
    """one problem of exactly VO_PNP_MAX_POINTS = 2^20: accepted; counts and mask equal a chunked numpy replay of the
    device's hypotheses; the refit (one 16-lane group over the inliers) equals pnp_ref.epnp on the same mask to 1e-8 and
    is the true pose within rounding_pose_bound.
    The inliers are noise-free up to their float32 rounding and the outliers are moved 20-100 px, so a near-exact
    hypothesis separates them exactly and the refit runs on rounding-only data."""
    n = 1 << 20
    rng = np.random.default_rng(91)
    p3, _, R, t, _ = pr.make_problem(rng, n, outlier_frac=0.0, noise=0.0)
    p2 = pr.project(p3, R, t, CAM)
    out = rng.random(n) < 0.3
    ang, r = rng.uniform(0, 2 * np.pi, out.sum()), rng.uniform(20, 100, out.sum())
    p2[out] += np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1).astype(np.float32)
    res = vo.pnp_ransac([(p3, p2)], CAM, diagnostics=True)
    hyp = res["hyp_Tcw"][0]
    counts = pr.inlier_counts(hyp, p3, p2, CAM, 8.0)
    assert np.array_equal(res["counts"][0], counts)
    best = res["best_iter"][0]
    assert best >= 0 and res["status"][0] == 1 and counts[best] == res["n_inliers"][0]
    mask = pr.reproj_err(hyp[best, :, :3], hyp[best, :, 3], p3, p2, CAM) <= np.float32(64.0)
    assert np.array_equal(res["inliers"][0], mask) and np.array_equal(mask, ~out)
    T = res["Tcw"][0]
    Rr, tr = pr.epnp(p3[mask].astype(np.float64)[None], p2[mask].astype(np.float64)[None], CAM)
    assert _rel(T, np.concatenate([Rr[0], tr[0][:, None]], axis=1)) <= 1e-8
    bR, bt = pr.rounding_pose_bound(p3[~out], R, t, CAM)
    assert np.abs(T[:, :3] - R).max() <= bR and np.abs(T[:, 3] - t).max() <= bt


# ----------------------------------------------------------------------------------- geometry the fixtures never reach
@pytest.mark.parametrize("cam_i", [0, 1])
def test_wide_geometry_noise_free(vo, cam_i):
    """any heading (within 1e-3 of pi too), 10-1000 m from the origin, depths 0.2-80 m, fx != fy, off-centre principal
    points, two cameras: hypotheses equal pnp_ref.epnp to 1e-9 (R absolute, t relative to |t|), the refit is the true
    pose within rounding_pose_bound and pnp_ref's refit to 1e-8"""
    rng = np.random.default_rng(100 + cam_i)
    cam, W, H = pr.WIDE_CAMS[cam_i]
    probs, truth = [], []
    for i, n in enumerate((6, 9, 20, 80, 600, 7, 40)):
        p3, p2, R, t, _ = pr.make_problem_wide(rng, n, outlier_frac=0.0, noise=0.0, cam4=cam, W=W, H=H, near_pi=i % 2 == 0)
        probs.append((p3, p2)), truth.append((R, t))
    res = vo.pnp_ransac(probs, cam, diagnostics=True)
    for k, ((p3, p2), (R, t)) in enumerate(zip(probs, truth)):
        want = pr.ransac_hypotheses(p3, p2, cam, 100)
        got = res["hyp_Tcw"][k]
        tscale = np.maximum(1.0, np.abs(want[:, :, 3]).max(axis=1))
        assert (np.abs(got[:, :, :3] - want[:, :, :3]).max(axis=(1, 2)) <= 1e-9).all(), k
        assert (np.abs(got[:, :, 3] - want[:, :, 3]).max(axis=1) <= 1e-9 * tscale).all(), k
        assert res["status"][k] == 1 and res["n_inliers"][k] == len(p3), k
        ref = pr.pnp_ransac(p3, p2, cam)
        assert _rel(res["Tcw"][k], ref["Tcw"]) <= 1e-8, k
        bR, bt = pr.rounding_pose_bound(p3, R, t, cam)
        T = res["Tcw"][k]
        assert np.abs(T[:, :3] - R).max() <= bR and np.abs(T[:, 3] - t).max() <= bt, k


@pytest.mark.parametrize("cam_i", [0, 1])
def test_wide_geometry_noisy_contract(vo, cam_i):
    cam, W, H = pr.WIDE_CAMS[cam_i]
    probs, refs = _fixtures(110 + cam_i, [6, 12, 50, 200, 900, 3000], make=pr.make_problem_wide, cam=cam, cam4=cam, W=W, H=H,
                            near_pi=cam_i == 1)
    res = vo.pnp_ransac(probs, cam, diagnostics=True)
    _check_contract(vo, probs, refs, res, cam=cam)


# --------------------------------------------------------------------------------------------- device-form contract
def test_device_form_sub_range_canaries_and_diag_members(vo):
    """offsets[0] != 0 (problems from the middle of larger arrays), canary bytes around every written range, each diag
    member alone equal to the same member of a full-diag call, a workspace of exactly vo_pnp_workspace_bytes"""
    import torch
    d = torch.device("cuda")
    probs, _ = _fixtures(121, [6, 40, 300, 5, 4, 1200, 77])
    want = vo.pnp_ransac(probs, CAM, diagnostics=True)
    P, iters, pad = len(probs), 100, 3
    lead, tail = pr.make_problem(np.random.default_rng(122), 333)[:2], pr.make_problem(np.random.default_rng(123), 211)[:2]
    allp = [lead] + probs + [tail]
    off = np.concatenate([[0], np.cumsum([len(a) for a, _ in allp])]).astype(np.int32)
    o0, o1 = int(off[1]), int(off[-2])
    p3 = torch.from_numpy(np.concatenate([a for a, _ in allp])).to(d)
    p2 = torch.from_numpy(np.concatenate([b for _, b in allp])).to(d)
    offs = torch.from_numpy(off[1:P + 2].copy()).to(d)  # offsets[0] = o0 > 0
    CANARY = 0xA5

    def canvas(shape_bytes):
        return torch.full((shape_bytes,), CANARY, dtype=torch.uint8, device=d)

    Tb, mb = canvas((P + 2 * pad) * 96), canvas(int(off[-1]))
    nb, sb = canvas((P + 2 * pad) * 4), canvas((P + 2 * pad) * 4)
    T = Tb[pad * 96:(pad + P) * 96].view(torch.float64)
    ni, st = nb[pad * 4:(pad + P) * 4].view(torch.int32), sb[pad * 4:(pad + P) * 4].view(torch.int32)
    names = dict(samples=((P, iters, 5), torch.int32), counts=((P, iters), torch.int32), hyp_Tcw12=((P, iters, 12), torch.float64),
                 best_iter=((P,), torch.int32), final_niters=((P,), torch.int32))
    full = {k: torch.full(s, -7, dtype=dt, device=d) for k, (s, dt) in names.items()}
    ws = torch.empty(vo.pnp_workspace_bytes(P, iters), dtype=torch.uint8, device=d)  # exactly the size asked for
    vo.pnp_ransac_dev(P, offs, p3, p2, CAM, T, mb, ni, st, diag=full, workspace=ws)
    torch.cuda.synchronize()
    Tb, mb, nb, sb = (x.cpu().numpy() for x in (Tb, mb, nb, sb))
    for buf, lo, hi in ((Tb, pad * 96, (pad + P) * 96), (mb, o0, o1), (nb, pad * 4, (pad + P) * 4), (sb, pad * 4, (pad + P) * 4)):
        assert (buf[:lo] == CANARY).all() and (buf[hi:] == CANARY).all()
    assert np.array_equal(Tb[pad * 96:(pad + P) * 96].view(np.uint64), want["Tcw"].reshape(-1).view(np.uint64))
    assert np.array_equal(mb[o0:o1].astype(bool), np.concatenate(want["inliers"]))
    assert np.array_equal(nb[pad * 4:(pad + P) * 4].view(np.int32), want["n_inliers"])
    assert np.array_equal(sb[pad * 4:(pad + P) * 4].view(np.int32), want["status"])
    key = dict(hyp_Tcw12="hyp_Tcw")
    for k, v in full.items():
        w = want[key.get(k, k)].reshape(v.shape)
        assert np.array_equal(v.cpu().numpy().view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), k
    for k, (s, dt) in names.items():  # one member at a time, the others NULL
        one = {k: torch.full(s, -7, dtype=dt, device=d)}
        vo.pnp_ransac_dev(P, offs, p3, p2, CAM, torch.zeros(P, 12, dtype=torch.float64, device=d),
                          torch.zeros(int(off[-1]), dtype=torch.uint8, device=d), torch.zeros(P, dtype=torch.int32, device=d),
                          torch.zeros(P, dtype=torch.int32, device=d), diag=one, workspace=ws)
        torch.cuda.synchronize()
        assert torch.equal(one[k].view(torch.uint8), full[k].view(torch.uint8)), k


def test_host_form_from_three_threads_at_once(vo):
    """the host form keeps thread_local scratch: three threads, each its own batch, all equal to the serial calls"""
    import threading
    sets = [_fixtures(131 + i, sz)[0] for i, sz in enumerate(([30, 400, 6], [1000, 8, 90, 2500], [64] * 40))]
    serial = [vo.pnp_ransac(s, CAM, diagnostics=True) for s in sets]
    got = [None] * 3
    barrier = threading.Barrier(3)

    def run(i):
        barrier.wait()
        for _ in range(3):
            got[i] = vo.pnp_ransac(sets[i], CAM, diagnostics=True)

    th = [threading.Thread(target=run, args=(i,)) for i in range(3)]
    for x in th:
        x.start()
    for x in th:
        x.join(120)
    for s, a, b in zip(sets, serial, got):
        assert b is not None
        for k in range(len(s)):
            assert _same_bits(_member(a, k), _member(b, k)) is None, k
