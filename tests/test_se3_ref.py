"""The Lie-group layer against an independent reference (tests/se3_ref.py: mpmath, 60 digits) over a grid of poses that
reaches every branch: the oracle (orc_se3_exp / orc_se3_log / orc_se3_plus), the library's host entry points
(vo_se3_exp / vo_se3_log, csrc/ba_math.h compiled for the host) and synth.se3_exp / synth.se3_log.  Oracle and kernels
share their formulas, so parity between them says nothing about the formulas themselves.

log is compared on the tangent; within 1e-6 of pi, where the sign of the axis is free, exp(log(T)) is compared with T.
Bounds: 1e-14 for exp and 1e-12 for log and plus, the bounds of test_se3_helpers; the corrected
functions stay inside them over the whole grid, so no wider bound near pi was needed.
"""
import mpmath as mp
import numpy as np
import pytest

import se3_ref as ref
from gauge import quat_w_sign
from vo_slam_test_amd import synth

EXP_TOL = 1e-14
LOG_TOL = 1e-12


@pytest.fixture(scope="module")
def cases():
    return ref.cases()


def _report(worst):
    e, c = worst
    return f"worst {e:.3g} at angle {c['th']!r}, axis {c['axis']}, |t| {c['tn']}"


def test_the_reference_agrees_with_scipy_logm_and_inverts_itself():
    """the reference checked against a third party (the matrix logarithm of the 4 x 4 pose, double precision) and
    against itself (log(exp(xi)) = xi to 50 digits), across the pi / small-angle switches of its own"""
    from scipy.linalg import expm, logm
    rng = np.random.default_rng(3)
    for th in [1e-7, 0.5e-6, 2e-6, 1e-3, 0.7, 2.2, 3.0, ref.PI - 0.5e-3, ref.PI - 2e-3, ref.PI - 1e-7]:
        a = rng.normal(size=3)
        xi = np.concatenate([rng.uniform(-2, 2, 3), th * a / np.linalg.norm(a)])
        back = ref.log(*ref.exp(xi))
        assert ref.err(xi, back) < 1e-40 * max(1.0, 1.0 / (ref.PI - th)), th
        X = np.zeros((4, 4))
        X[:3, :3] = [[0, -xi[5], xi[4]], [xi[5], 0, -xi[3]], [-xi[4], xi[3], 0]]
        X[:3, 3] = xi[:3]
        T = expm(X)
        R, t = ref.exp(xi)
        assert ref.err(T[:3, :3], R) < 1e-14 and ref.err(T[:3, 3], t) < 1e-14, th
        if th < 3.1:  # logm loses digits at the cut
            L = np.real(logm(T))
            got = np.array([L[0, 3], L[1, 3], L[2, 3], L[2, 1], L[0, 2], L[1, 0]])
            assert ref.err(got, ref.log(T[:3, :3], T[:3, 3])) < 1e-11 * max(1.0, 1e-7 / th), th


def test_the_grid_reaches_both_hemispheres_and_every_branch(cases):
    w = np.array([quat_w_sign(c["R"]) for c in cases])
    tr = np.array([np.trace(c["R"]) for c in cases])
    assert (w < 0).sum() >= 100 and (w > 0).sum() >= 100
    for i in range(3):  # each i case of the tr <= 0 branch, with w of both signs
        sel = np.array([t <= 0 and int(np.argmax(np.diag(c["R"]))) == i for t, c in zip(tr, cases)])
        assert (w[sel] < 0).any() and (w[sel] > 0).any(), i
    th = np.array([c["th"] for c in cases])
    assert (th < 1e-10).any() and ((th > 1e-10) & (th < 1.2e-10)).any() and (ref.PI - th < ref.NEAR_PI).any()
    assert ((tr > 0) & (th > 2.09)).any() and ((tr <= 0) & (th < 2.1)).any()  # either side of the tr switch


# ------------------------------------------------------------------------------------------------------------ oracle
def test_oracle_exp(orc, cases):
    worst = (0.0, None)
    for c in cases:
        q, t = np.zeros(4), np.zeros(3)
        orc.lib().orc_se3_exp(c["xi_d"], q, t)
        qr, tr = ref.quat(c["xi_d"])
        e = max(ref.err(q, qr), ref.err(t, tr))
        worst = max(worst, (e, c), key=lambda x: x[0])
    print(_report(worst))
    assert worst[0] < EXP_TOL, _report(worst)


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["q", "minus_q"])
def test_oracle_log(orc, cases, sign):
    worst = (0.0, None)
    for c in cases:
        q = ref.quat_wxyz(c["R"])
        got = np.zeros(6)
        orc.lib().orc_se3_log(np.ascontiguousarray(sign * q), np.ascontiguousarray(c["t"]), got)
        e = ref.log_error(got, c, R_ref=ref.R_from_quat(q))
        worst = max(worst, (e, c), key=lambda x: x[0])
    print(_report(worst))
    assert worst[0] < LOG_TOL, _report(worst)


def test_oracle_plus(orc, cases):
    """x over the grid, delta an LM-sized step (0.05): at pi - 1e-3 and pi - 1e-7 about half of the steps cross pi"""
    rng = np.random.default_rng(11)
    worst, crossed = (0.0, None), 0
    for c in cases:
        d = rng.uniform(-0.05, 0.05, 6)
        got = np.zeros(6)
        orc.lib().orc_se3_plus(c["xi_d"], d, got)
        Rw, tw = ref.compose(ref.exp(d), ref.exp(c["xi_d"]))
        want = ref.log(Rw, tw)
        th = float(mp.sqrt(sum(v * v for v in want[3:])))
        crossed += c["th"] > 3.1 and float(np.dot(got[3:], c["xi_d"][3:])) < 0
        if ref.PI - th < ref.NEAR_PI:
            R, t = ref.exp(got)
            e = max(ref.err(ref.to_float(R), Rw), ref.err(ref.to_float(t), tw))
        else:
            e = ref.err(got, want)
        worst = max(worst, (e, c), key=lambda x: x[0])
    assert crossed >= 10
    print(_report(worst))
    assert worst[0] < LOG_TOL, _report(worst)


# ----------------------------------------------------------------------------------------------- library (host code)
def test_library_exp(vo, cases):
    worst = (0.0, None)
    for c in cases:
        R, t = vo.se3_exp(c["xi_d"])
        Rr, tr = ref.exp(c["xi_d"])
        e = max(ref.err(R, Rr), ref.err(t, tr))
        worst = max(worst, (e, c), key=lambda x: x[0])
    print(_report(worst))
    assert worst[0] < EXP_TOL, _report(worst)


def test_library_log(vo, cases):
    worst = (0.0, None)
    for c in cases:
        e = ref.log_error(vo.se3_log(c["R"], c["t"]), c)
        worst = max(worst, (e, c), key=lambda x: x[0])
    print(_report(worst))
    assert worst[0] < LOG_TOL, _report(worst)


def test_library_log_where_w_is_negative(vo, cases):
    """the cases that the missing fabs got wrong, on their own: a camera turned more than 120 degrees"""
    sel = [c for c in cases if quat_w_sign(c["R"]) < 0 and c["tn"] > 0]
    assert len(sel) >= 50
    worst = (0.0, None)
    for c in sel:
        worst = max(worst, (ref.log_error(vo.se3_log(c["R"], c["t"]), c), c), key=lambda x: x[0])
    print(_report(worst))
    assert worst[0] < LOG_TOL, _report(worst)


# ------------------------------------------------------------------------------------------------------------- synth
def test_synth_exp(cases):
    worst = (0.0, None)
    for c in cases:
        R, t = synth.se3_exp(c["xi_d"])
        Rr, tr = ref.exp(c["xi_d"])
        e = max(ref.err(R, Rr), ref.err(t, tr))
        worst = max(worst, (e, c), key=lambda x: x[0])
    print(_report(worst))
    assert worst[0] < EXP_TOL, _report(worst)


def test_synth_log(cases):
    worst = (0.0, None)
    for c in cases:
        worst = max(worst, (ref.log_error(synth.se3_log(c["R"], c["t"]), c), c), key=lambda x: x[0])
    print(_report(worst))
    assert worst[0] < LOG_TOL, _report(worst)
