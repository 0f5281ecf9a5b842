"""The loop-closure solvers on the device away from the corner the older tests sit in (inputs: tests/loop_inputs.py; the
conditions those inputs meet, and every oracle figure a bound below is derived from: tests/test_loop_inputs_ref.py).

 A. vo.sim3_ransac_eval  -- true rotations of 0.5 ... pi, scales 0.25 / 1 / 4, n = 3 ... 300 on either side of the block width
 B. vo.Optimizer.solveLoopSim3 -- the same rotations, scales 0.5 / 1 / 2, 10 ... 1000 matches in ragged batches
 C. vo.Optimizer.solvePoseGraphLoop -- non-unit scales and measurements, a fixed node anywhere, either quaternion sign,
    graphs of 2 ... 90 nodes
 D. vo.sim3_reanchor_points

Rotations are compared as matrices, never as angle-axis vectors.  Each test prints its worst distances (pytest -s).
"""
import numpy as np
import pytest

import gauge
import loop_inputs as li

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------- A. Sim3 hypotheses
@pytest.fixture(scope="module")
def ransac(orc):
    """[(label, data, fix_scale, oracle counts, oracle flags, oracle sims)] over the grid, the oracle run once"""
    return [(label, data, fix) + li.oracle_ransac(orc, data, fix) for label, data, fix, _ in li.ransac_cases()]


def _device_ransac(vo, data, fix):
    return vo.sim3_ransac_eval(*data[:8], fix)


def test_sim3_hypotheses_over_rotations_scales_and_sizes(vo, ransac):
    """44 calls of 40 hypotheses.  Against the oracle: identical counts and flags, sims within the project's 1e-11 relative
    to max(1, |entry|).  Against LAPACK (loop_inputs.horn_numpy): the oracle's worst distance on exactly these inputs is
    3.43e-11 (recorded as 3.5e-11, measured again by test_loop_inputs_ref.py); the device gets ten times that, 3.5e-10 --
    the ten for the reduction order and the Jacobi-versus-QR eigenvectors -- which is inside the 1e-9 of
    test_sim3_hypotheses_against_an_independent_eigen_solver.  Flags against a float64 numpy restatement of checkInliers
    for every pair whose two errors are both further than 0.1 % from their thresholds (fewer than 1 % of the pairs are not)."""
    worst_o = worst_l = 0.0
    good = hyps = 0
    for label, data, fix, oc, of, osim in ransac:
        counts, flags, sims = _device_ransac(vo, data, fix)
        assert np.array_equal(counts, oc) and np.array_equal(flags, of), label
        d = li.sims_distance(sims, osim)
        worst_o = max(worst_o, d)
        assert d < 1e-11, (label, d)
        ref = li.horn_all(data, fix)
        d = li.sims_distance(sims, ref)
        worst_l = max(worst_l, d)
        assert d < 10 * li.HORN_ORACLE_WORST, (label, d)
        want, near = li.check_inliers_numpy(data, ref)
        assert np.array_equal(flags[~near], want[~near]), label
        assert np.array_equal(counts, flags.sum(1)), label
        if fix:
            assert np.all(sims[:, 12] == 1.0), label
        good, hyps = good + int((counts > len(data[0]) / 2).sum()), hyps + len(counts)
    assert 3 * good >= hyps        # not a comparison of all-zero rows
    print(f"A: worst device - oracle {worst_o:.3g} (bound 1e-11), worst device - LAPACK {worst_l:.3g} (bound {10 * li.HORN_ORACLE_WORST:.3g}); "
          f"{good} of {hyps} hypotheses with a count above n / 2")


def test_sim3_hypotheses_resident_path_at_257(vo, ransac):
    """resident_n at n = 257 (one correspondence into the second trip of the strided loop): bit for bit the uploaded call"""
    done = 0
    for label, data, fix, oc, of, osim in ransac:
        if len(data[0]) != 257 or done == 2:
            continue
        counts, flags, sims = _device_ransac(vo, data, fix)
        c1, f1, s1 = vo.sim3_ransac_eval(None, None, None, None, None, None, data[6], data[7], fix, resident_n=257)
        assert np.array_equal(c1, counts) and np.array_equal(f1, flags) and np.array_equal(s1, sims), label
        done += 1
    assert done == 2


@pytest.mark.parametrize("fix_scale", [True, False])
def test_sim3_hypotheses_on_degenerate_triplets(vo, orc, fix_scale):
    """three exactly collinear points, and three points 1e-12 apart: parity with the oracle, NaNs equal -- no claim about
    what Horn's form should answer there"""
    data = li.degenerate_ransac_data()
    counts, flags, sims = vo.sim3_ransac_eval(*data, fix_scale)
    oc, of, osim = li.oracle_ransac(orc, data, fix_scale)
    print(f"A: degenerate triplets, fix_scale={fix_scale}: counts {counts.tolist()}, oracle {oc.tolist()}; "
          f"worst finite difference {np.nanmax(np.abs(sims - osim)):.3g}")
    assert np.array_equal(np.isnan(sims), np.isnan(osim))
    assert np.allclose(sims, osim, rtol=0, atol=1e-11, equal_nan=True)
    assert np.array_equal(counts, oc) and np.array_equal(flags, of)


# ------------------------------------------------------------------------------------------------- B. Sim3 refinement
@pytest.mark.parametrize("fix_scale", [True, False])
def test_sim3_refinement_over_rotations_scales_and_sizes(vo, orc, fix_scale):
    """180 ragged problems in one call (10 ... 1000 matches: one to four trips of the strided loops), against the oracle with
    the bounds of test_sim3_solve_matches_oracle: Sim3 within 1e-8 as (R, t) and scale, identical masks, inlier counts,
    iteration counts of both problems and phase, final cost within 1e-9 relative.  16 of the 360 oracle solves end with
    |w| > pi, 101 stop after problem 1 (fewer than ten survivors)."""
    probs = li.refine_problems(fix_scale)
    poses, scales, masks, ninl, sums = vo.Optimizer.solveLoopSim3([pr for _, pr in probs], fixScaleFlag=fix_scale, summaries=True)
    worst_p = worst_s = worst_c = 0.0
    beyond = 0
    for i, (label, pr) in enumerate(probs):
        op, osc, oout, oinl, osums = orc.sim3_solve(pr, fix_scale=fix_scale)
        phase = li.oracle_phase(osums)
        assert sums[2 * i].reserved == phase, label
        assert np.array_equal(masks[i], oout) and ninl[i] == oinl, label
        assert [sums[2 * i].iterations, sums[2 * i + 1].iterations] == [osums[0].iterations, osums[1].iterations], label
        Rd, td, sd = li.sim3_of(poses[i], scales[i])
        Ro, to, so = li.sim3_of(op, osc)
        d = gauge.pose_distance((Rd, td), (Ro, to))
        worst_p, worst_s = max(worst_p, d), max(worst_s, abs(sd - so))
        assert d < 1e-8 and abs(sd - so) < 1e-8, (label, d, sd - so)
        k = phase - 1
        c = abs(sums[2 * i + k].final_cost - osums[k].final_cost) / max(1.0, osums[k].final_cost)
        worst_c = max(worst_c, c)
        assert c <= 1e-9, (label, c)
        if fix_scale:
            assert scales[i] == pr["scale0"]
        if phase == 1:
            assert np.array_equal(poses[i], pr["pose0"]) and scales[i] == pr["scale0"], label
        beyond += np.linalg.norm(poses[i][:3]) > np.pi
    assert beyond >= 2
    print(f"B: fix_scale={fix_scale}: worst device - oracle pose {worst_p:.3g}, scale {worst_s:.3g} (bounds 1e-8), final cost {worst_c:.3g} "
          f"(bound 1e-9); {beyond} solves end with |w| > pi")


def test_sim3_refinement_reaches_the_minimum_of_scipy_least_squares(vo):
    """consistent problems (unit sigmas, no outliers, 0.3 px noise, 256 matches) at every rotation, scale 2 free and scale 1
    fixed; the device solve iterated from its own result, at most 6 calls; scipy's least_squares on an independently written
    residual of the two reprojection blocks (scipy's Rotation, 7 or 6 unknowns).  Bounds of
    test_rotated_pose_only_reaches_the_minimum_of_scipy_least_squares: cost within 1 - 1e-12 ... 1 + 5e-5, Sim3 within 5e-5.
    The oracle meets them on the same chain (worst cost ratio 1 + 3.2e-7, pose 6.4e-6, scale 2.3e-7), so they stand as they are."""
    wc = wp = ws = 0.0
    for label, pr, fix in li.consistent_refine_problems():
        pose, sc = pr["pose0"], pr["scale0"]
        for _ in range(6):
            out = vo.Optimizer.solveLoopSim3([dict(pr, pose0=pose, scale0=sc)], fixScaleFlag=fix)
            pose, sc = out[0][0], float(out[1][0])
        assert out[3][0] == 256 and not out[2][0].any(), label
        R, t, s = li.sim3_of(pose, sc)
        res = li.sim3_block_residuals(pr, R, t, s)
        assert max((res[:, :2] ** 2).sum(1).max(), (res[:, 2:] ** 2).sum(1).max()) < 10.0, label   # below the Huber threshold
        (Rr, tr, sr), c_ref = li.sim3_scipy_minimum(pr, fix)
        c = 0.5 * float((res ** 2).sum())
        dp = gauge.pose_distance((R, t), (Rr, tr))
        wc, wp, ws = max(wc, c / c_ref - 1), max(wp, dp), max(ws, abs(s - sr))
        assert c_ref * (1 - 1e-12) <= c <= c_ref * (1 + 5e-5), (label, c, c_ref)
        assert dp < 5e-5 and abs(s - sr) < 5e-5, (label, dp, s - sr)
    print(f"B: worst device - scipy: cost ratio - 1 {wc:.3g}, pose {wp:.3g}, scale {ws:.3g} (bounds 5e-5)")


def test_sim3_refinement_ten_survivor_rule(vo, orc):
    """a clean 40-match problem with pix_curr moved by 500 px on all but k matches: k = 9 returns after problem 1 with the
    pose and scale it was given, bit for bit; k = 10 and 11 go on"""
    probs = [li.survivor_problem(k) for k in (9, 10, 11)]
    poses, scales, masks, ninl, sums = vo.Optimizer.solveLoopSim3(probs, summaries=True)
    for i, k in enumerate((9, 10, 11)):
        op, osc, oout, oinl, osums = orc.sim3_solve(probs[i])
        assert sums[2 * i].reserved == li.oracle_phase(osums) == (1 if k == 9 else 2), k
        assert np.array_equal(masks[i], oout) and int((masks[i] == 0).sum()) == k, k
        assert ninl[i] == oinl == (0 if k == 9 else k), k
        assert [sums[2 * i].iterations, sums[2 * i + 1].iterations] == [osums[0].iterations, osums[1].iterations], k
    assert np.array_equal(poses[0], probs[0]["pose0"]) and scales[0] == probs[0]["scale0"]
    assert not np.array_equal(poses[1], probs[1]["pose0"])


def test_sim3_refinement_five_iteration_branch(vo, orc):
    """nothing rejected after problem 1, so problem 2 gets 5 iterations (optimizer_ceres.cpp:962-968): the oracle uses all
    five on this problem, and a device that allowed ten would go on"""
    pr = li.clean_problem()
    poses, scales, masks, ninl, sums = vo.Optimizer.solveLoopSim3([pr], summaries=True)
    op, osc, oout, oinl, osums = orc.sim3_solve(pr)
    assert not oout.any() and not masks[0].any() and ninl[0] == oinl == len(oout)
    assert sums[1].iterations == osums[1].iterations and sums[1].iterations <= 5
    assert sums[0].iterations == osums[0].iterations
    assert gauge.pose_distance(li.sim3_of(poses[0], scales[0])[:2], li.sim3_of(op, osc)[:2]) < 1e-8


# ------------------------------------------------------------------------------------------------- C. pose graph
@pytest.fixture(scope="module")
def graphs():
    return li.pose_graph_cases()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def test_pose_graph_with_scales_fixed_nodes_and_small_graphs(vo, orc, graphs):
    """(n_kf, fixed) in (2, 1), (3, 1), (12, 5), (40, 39), (90, 0), consistent and inconsistent scale measurements, and a
    graph with a node no edge touches; bounds of test_pose_graph_matches_oracle"""
    worst_q = worst_t = worst_c = 0.0
    for label, g in graphs:
        q, t, s = vo.Optimizer.solvePoseGraphLoop(g)
        oq, ot, os_ = orc.pose_graph_solve(g)
        assert (s.iterations, s.accepted, s.termination) == (os_.iterations, os_.accepted, os_.termination), label
        dq, dt, dc = np.abs(q - oq).max(), np.abs(t - ot).max(), abs(s.final_cost - os_.final_cost) / os_.final_cost
        worst_q, worst_t, worst_c = max(worst_q, dq), max(worst_t, dt), max(worst_c, dc)
        assert dc <= 1e-10 and dq < 1e-9 and dt < 1e-8, (label, dq, dt, dc)
        f = g["fixed"]
        assert _same_bits(q[f], g["quats"][f]) and _same_bits(t[f], g["trans"][f]), label
        assert np.abs(np.linalg.norm(q, axis=1) - 1).max() < 1e-12, label
        assert os_.iterations >= 1 and np.abs(t - g["trans"]).max() > 1e-6, label     # something was solved
    g = graphs[-1][1]
    q, t, _ = vo.Optimizer.solvePoseGraphLoop(g)
    assert _same_bits(q[-1], g["quats"][-1]) and _same_bits(t[-1], g["trans"][-1])
    print(f"C: worst device - oracle quaternions {worst_q:.3g} (bound 1e-9), translations {worst_t:.3g} (bound 1e-8), cost {worst_c:.3g} (bound 1e-10)")


def test_pose_graph_quaternion_signs(vo, graphs):
    """the quaternions of the odd nodes and of every third measurement negated: the result is the un-negated solve with the
    same signs, bit for bit (negation is exact and H and g get the same bits; the oracle is bit-identical, CPU test)"""
    for label, g in graphs:
        q, t, s = vo.Optimizer.solvePoseGraphLoop(g)
        qa, ta, sa = vo.Optimizer.solvePoseGraphLoop(g)
        assert _same_bits(q, qa) and _same_bits(t, ta), label          # the same graph twice: identical
        g2, sn = li.negate_signs(g)
        q2, t2, s2 = vo.Optimizer.solvePoseGraphLoop(g2)
        assert _same_bits(q2, q * sn[:, None]) and _same_bits(t2, t), label
        assert (s2.iterations, s2.accepted, s2.termination) == (s.iterations, s.accepted, s.termination), label
        assert s2.final_cost == s.final_cost, label


def test_pose_graph_under_a_change_of_world_frame(vo):
    """every node right-multiplied by T = (s_T, R_T, 0): q_i -> q_i q_T, t_i unchanged, s_i -> s_i s_T, for every rotation of
    gauge.GAUGES (one q_T with w < 0) and s_T in {1, 1.7}.  In exact arithmetic the LM iterates are X_k T, so the solved
    nodes mapped back are the original solve, with the same iteration and acceptance counts.  Bounds: ten times the
    oracle's worst on these graphs -- measured 1.50e-15 (quaternion coefficients, recorded 1.6e-15) and 2.31e-14
    (translations, recorded 2.4e-14) -- i.e. 1.6e-14 and 2.4e-13.

    T carries NO translation on purpose: the translation update is additive, which is not equivariant under a translated
    frame, and the oracle itself moves by 1e-4 ... 1e-3 there.  That is a property of the reference's parameterisation,
    not a defect to be fixed here."""
    wq = wt = 0.0
    for label, g in li.frame_graphs():
        q, t, s = vo.Optimizer.solvePoseGraphLoop(g)
        for cl, qT, sT in li.frame_changes():
            q2, t2, s2 = vo.Optimizer.solvePoseGraphLoop(li.change_frame(g, qT, sT))
            assert (s2.iterations, s2.accepted, s2.termination) == (s.iterations, s.accepted, s.termination), (label, cl)
            dq, dt = li.quat_distance(li.frame_back(q2, qT), q), float(np.abs(t2 - t).max())
            wq, wt = max(wq, dq), max(wt, dt)
            assert dq < 10 * li.FRAME_ORACLE_Q and dt < 10 * li.FRAME_ORACLE_T, (label, cl, dq, dt)
    print(f"C: worst change-of-frame deviation: quaternions {wq:.3g} (bound {10 * li.FRAME_ORACLE_Q:.3g}), translations {wt:.3g} "
          f"(bound {10 * li.FRAME_ORACLE_T:.3g})")


def test_pose_graph_reaches_the_minimum_of_scipy_least_squares(vo):
    """n_kf = 8, fixed = 3, non-unit scales and scale measurements; the residual written with scipy's Rotation (a left
    rotation vector and an additive translation per free node, 42 unknowns); the device result re-fed until the cost stops
    falling, at most 8 calls (the constant scale rows are 99.3 % of the cost, so Ceres' relative function tolerance stops
    every solve early).  Compared: the cost without the scale rows, and the poses as (R, t).  The oracle on the same chain
    ends 1.70e-7 (relative) above scipy's cost and 1.84e-4 from its poses (recorded 2e-7 and 2e-4); the device bound is
    that gap plus the device-versus-oracle bounds (1e-10 relative on the whole cost, 1e-8 on poses)."""
    g = li.scipy_graph()
    Rr, tr, c_ref = li.pose_graph_scipy_minimum(g)
    const = li.pose_graph_scale_constant(g)
    q, t, prev = g["quats"], g["trans"], np.inf
    for _ in range(8):
        q, t, s = vo.Optimizer.solvePoseGraphLoop(dict(g, quats=q, trans=t))
        if not s.final_cost < prev:
            break
        prev = s.final_cost
    R = np.array([li.q_matrix(x) for x in q])
    c = 0.5 * float((li.pose_graph_residuals(g, R, t) ** 2).sum())
    gap_p = max(gauge.pose_distance((R[a], t[a]), (Rr[a], tr[a])) for a in range(8))
    print(f"C: device - scipy: cost without the scale rows {c!r} against {c_ref!r} (ratio - 1 = {c / c_ref - 1:.3g}), poses {gap_p:.3g}")
    assert abs((s.final_cost - const) - c) < 1e-12 * s.final_cost
    assert c_ref * (1 - 1e-12) <= c <= c_ref * (1 + li.PG_SCIPY_COST_GAP) + 1e-10 * s.final_cost
    assert gap_p <= li.PG_SCIPY_POSE_GAP + 1e-8


# ------------------------------------------------------------------------------------------------- D. re-anchoring
@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("scale", [0.25, 4.0])
def test_sim3_reanchor_points_scales_signs_and_sizes(vo, n, scale):
    """corrected = S_wr (S_rw p) with random unit quaternions (every second one with w < 0) against the formula written with
    scipy's Rotation, within 1e-12 max(1, |expected|); all references -1: the input comes back bit for bit"""
    pts, ref, S1, S2, exp = li.reanchor_inputs(n, n, scale)
    out = vo.sim3_reanchor_points(pts, ref, S1, S2)
    d = float((np.abs(out - exp) / np.maximum(1.0, np.abs(exp))).max())
    print(f"D: n {n}, scale {scale}: worst device - formula {d:.3g} (bound 1e-12)")
    assert d < 1e-12
    same = vo.sim3_reanchor_points(pts, np.full(n, -1, np.int32), S1, S2)
    assert _same_bits(same, pts)
