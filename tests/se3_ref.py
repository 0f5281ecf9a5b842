"""SE(3) exp / log / plus in mpmath at 60 digits: the reference for the Lie-group layer that shares no formula with
csrc/ba_math.h, oracle/ba_oracle.c or synth.py (tests/test_se3_ref.py, the device tests at large rotations).

Tangent order [upsilon; omega], T = (R, t) with t = V upsilon:
  R = I + A W + B W^2,  V = I + B W + C W^2,  W = hat(omega), theta = |omega|,
  A = sin(theta) / theta,  B = (1 - cos(theta)) / theta^2,  C = (theta - sin(theta)) / theta^3,
each from its Taylor series below theta = 1e-6 (the omitted term is below 1e-60).  log takes the angle from
atan2(|vee(R - R^T)| / 2, (tr R - 1) / 2), the axis from the skew part of R = sin(theta) hat(a) -- or, beyond 2 rad,
from the symmetric part (R + R^T) / 2 - cos(theta) I = (1 - cos(theta)) a a^T, its sign from the skew part -- and
upsilon = V^-1 t by a linear solve, so that no closed form of V^-1 is involved.  The rotation returned has theta in
[0, pi]; at exactly pi the sign of the axis is free.  The inputs of the tests are rotations rounded to double, which are
orthogonal to 1e-16 only; each part is used where it is well conditioned (the skew part near pi would turn that 1e-16
into 1e-16 / sin(theta) of axis error that belongs to the input, not to the code under test).

Also the grid of poses that the tests walk (grid()): every branch of the matrix -> quaternion step and of the small-angle
selections, both quaternion hemispheres.
"""
import functools

import mpmath as mp
import numpy as np

mp.mp.dps = 60

SERIES_BELOW = mp.mpf("1e-6")


def _hat(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def _coefficients(theta):
    """A = sin t / t, B = (1 - cos t) / t^2, C = (t - sin t) / t^3"""
    t2 = theta * theta
    if theta < SERIES_BELOW:
        A = sum((-t2) ** k / mp.factorial(2 * k + 1) for k in range(8))
        B = sum((-t2) ** k / mp.factorial(2 * k + 2) for k in range(8))
        C = sum((-t2) ** k / mp.factorial(2 * k + 3) for k in range(8))
        return A, B, C
    s, c = mp.sin(theta), mp.cos(theta)
    return s / theta, (1 - c) / t2, (theta - s) / (t2 * theta)


def _mpv(x):
    return [mp.mpf(float(v)) if not isinstance(v, mp.mpf) else v for v in x]


def _V(om):
    theta = mp.sqrt(sum(v * v for v in om))
    _, B, C = _coefficients(theta)
    W = _hat(om)
    return mp.eye(3) + B * W + C * (W * W)


def exp(xi):
    """tangent [upsilon; omega] (floats or mpf) -> (R 3x3 mp.matrix, t 3x1 mp.matrix)"""
    xi = _mpv(xi)
    ups, om = mp.matrix(xi[:3]), xi[3:]
    theta = mp.sqrt(sum(v * v for v in om))
    A, B, _ = _coefficients(theta)
    W = _hat(om)
    R = mp.eye(3) + A * W + B * (W * W)
    return R, _V(om) * ups


def so3_log(R):
    """rotation matrix (mp.matrix or array of floats) -> omega (list of 3 mpf), |omega| in [0, pi]"""
    R = mp.matrix([[mp.mpf(float(R[i][j])) if not isinstance(R, mp.matrix) else R[i, j] for j in range(3)] for i in range(3)])
    vee = [(R[2, 1] - R[1, 2]) / 2, (R[0, 2] - R[2, 0]) / 2, (R[1, 0] - R[0, 1]) / 2]  # sin(theta) a
    s = mp.sqrt(sum(v * v for v in vee))
    c = (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2
    theta = mp.atan2(s, c)
    if theta < SERIES_BELOW:
        # vee = A(theta) omega
        A, _, _ = _coefficients(theta)
        return [v / A for v in vee]
    if theta < 2:
        return [v * theta / s for v in vee]
    S = (R + R.T) / 2 - mp.cos(theta) * mp.eye(3)  # (1 - cos) a a^T
    i = max(range(3), key=lambda k: S[k, k])
    a = [S[k, i] for k in range(3)]
    n = mp.sqrt(sum(v * v for v in a))
    a = [v / n for v in a]
    if sum(a[k] * vee[k] for k in range(3)) < 0:
        a = [-v for v in a]
    return [theta * v for v in a]


def log(R, t):
    """(R, t) -> tangent [upsilon; omega] (list of 6 mpf)"""
    om = so3_log(R)
    tv = mp.matrix(_mpv([t[i] for i in range(3)]))
    ups = mp.lu_solve(_V(om), tv)
    return [ups[0], ups[1], ups[2]] + om


def compose(Ta, Tb):
    return Ta[0] * Tb[0], Ta[0] * Tb[1] + Ta[1]


def plus(x, d):
    """PoseLocalParameterization::Plus: log(exp(d) exp(x))"""
    return log(*compose(exp(d), exp(x)))


def quat(xi):
    """unit quaternion (w, x, y, z) with w >= 0 of exp(xi)'s rotation, and its translation (mpf lists)"""
    xi = _mpv(xi)
    om = xi[3:]
    theta = mp.sqrt(sum(v * v for v in om))
    half = theta / 2
    k = mp.mpf(1) / 2 * _coefficients(half)[0]  # sin(theta / 2) / theta
    _, t = exp(xi)
    return [mp.cos(half)] + [k * v for v in om], [t[0], t[1], t[2]]


def R_from_quat(q):
    """rotation matrix (mp.matrix) of a quaternion (w, x, y, z) of floats, normalised here; q and -q give the same"""
    q = _mpv(q)
    n = mp.sqrt(sum(v * v for v in q))
    w, x, y, z = [v / n for v in q]
    return mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def to_float(x):
    """mp.matrix or list of mpf -> float64 array (correctly rounded)"""
    if isinstance(x, mp.matrix):
        return np.array([[float(x[i, j]) for j in range(x.cols)] for i in range(x.rows)]).squeeze()
    return np.array([float(v) for v in x])


def err(got, want):
    """largest absolute difference of a float array from an mpf list / matrix, as a float"""
    got = np.asarray(got, np.float64).reshape(-1)
    want = [want[i, j] for i in range(want.rows) for j in range(want.cols)] if isinstance(want, mp.matrix) else list(want)
    assert len(want) == got.size
    return float(max(abs(mp.mpf(float(g)) - w) for g, w in zip(got, want)))


# ---------------------------------------------------------------------------------------------------------------- grid
PI = float(mp.pi)
ANGLES = [0.0, 1e-12, 0.9e-10, 1.1e-10, 1e-5, PI / 2 - 1e-9, PI / 2 + 1e-9, 2 * PI / 3 - 1e-9, 2 * PI / 3 + 1e-9, 2.2, 2.6, 3.0,
          PI - 1e-3, PI - 1e-7]
NEAR_PI = 1e-6  # within this of pi the axis sign is free: compare exp(log(T)) with T
T_NORMS = [0.0, 0.3, 2.0]


def axes():
    """the coordinate axes, their negatives, one axis dominated by each of x, y, z (the three i cases of the matrix ->
    quaternion step's tr <= 0 branch, with components of both signs), four random axes"""
    rng = np.random.default_rng(20240611)
    a = [np.eye(3)[i] for i in range(3)] + [-np.eye(3)[i] for i in range(3)]
    a += [np.array([0.9, -0.3, 0.2]), np.array([0.25, 0.85, -0.4]), np.array([-0.3, 0.2, -0.9])]
    a += list(rng.normal(size=(4, 3)))
    return [v / np.linalg.norm(v) for v in a]


def grid():
    """[(angle, axis index, translation norm, R [3, 3] f64, t [3] f64)]: the pose exp(theta a) with a translation of the
    given norm, rounded to double.  The reference value of anything computed from a case is the mpmath function of these
    doubles, so that the rounding of the input is not charged to the code under test."""
    rng = np.random.default_rng(7)
    out = []
    for ia, a in enumerate(axes()):
        for th in ANGLES:
            R = to_float(exp([0, 0, 0] + list(th * a))[0])
            for tn in T_NORMS:
                d = rng.normal(size=3)
                out.append((th, ia, tn, R, tn * d / np.linalg.norm(d)))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """the grid with its reference values, computed once per process: dicts of th, axis, tn, R, t, xi (the log as mpf
    list), xi_d (the same rounded to double: the input of the exp tests), near_pi"""
    out = []
    for th, ia, tn, R, t in grid():
        xi = log(R, t)
        out.append(dict(th=th, axis=ia, tn=tn, R=R, t=t, xi=xi, xi_d=to_float(xi), near_pi=PI - th < NEAR_PI))
    return out


def log_error(got, c, R_ref=None):
    """error of a log computed for case c (R_ref: the rotation actually handed over where it was not c["R"]): on the
    tangent, or -- within NEAR_PI of pi -- of exp(got) on the group"""
    if not c["near_pi"]:
        return err(got, c["xi"] if R_ref is None else log(R_ref, c["t"]))
    R, t = exp(got)
    Rw = mp.matrix(c["R"].tolist()) if R_ref is None else R_ref
    return max(err(to_float(R), Rw), err(to_float(t), list(c["t"])))


def quat_wxyz(R):
    """float64 unit quaternion with w >= 0 of a grid rotation, through mpmath (so3_log), for the oracle's quaternion forms"""
    om = so3_log(R)
    theta = mp.sqrt(sum(v * v for v in om))
    k = mp.mpf(1) / 2 * _coefficients(theta / 2)[0]
    return to_float([mp.cos(theta / 2)] + [k * v for v in om])
