"""CPU tests of the model of vo_kfstore_create_map_points (tests/new_points_ref.py) and of the inputs the GPU tests use
(tests/new_points_inputs.py): the model's search against the built oracle, its triangulation against the oracle's, F12 and the
created points against independent float64 restatements, the two-holder descriptor rule against the median loop, the
hand-made cases on the model, and the condition under which the device comparison is exact: no GPU script contains a match
that is not decisive."""
import ctypes as C
import math

import numpy as np
import pytest

import new_points_inputs as ni
import new_points_ref as ref

f32 = np.float32


@pytest.fixture(scope="module")
def scene():
    return ni.run_model(ni.random_scene(ni.SEED))


@pytest.fixture(scope="module")
def hand():
    return [(c, *ni.run_model(c["script"])) for c in ni.hand_cases()]


def _gpu_models(scene, hand):
    return [("random_scene", scene[0])] + [(c["name"], m) for c, m, _ in hand]


def test_search_equals_the_oracle(orc, scene, hand):
    """every search of every script, given the model's F12 and epipole: match12 and the count, exactly"""
    n_searches = 0
    sf = np.array(ni.SF + [ni.SF[-1]] * 8, f32)
    for name, m in _gpu_models(scene, hand):
        for cur, k, a_has, b_has, F, ex, ey, match12, cnt, _ in m.searches:
            va, vb = m._view(cur), m._view(k)
            oa, ob = (orc.FrameData(v["x"], v["y"], v["octave"], v["angle"], v["u_right"], v["desc"]) for v in (va, vb))
            ba, bb = orc.BowData(va["nodes"]), orc.BowData(vb["nodes"])
            om = np.full(len(va["x"]), -1, np.int32)
            on = orc.lib().orc_match_triangulation(C.byref(oa.c), np.array(a_has, np.uint8), C.byref(ba.c), C.byref(ob.c), np.array(b_has, np.uint8),
                                                   C.byref(bb.c), np.array(F, np.float64), float(ex), float(ey), sf, 1, om)
            assert on == cnt and [int(x) for x in om] == match12, (name, cur, k)
            n_searches += 1
    assert n_searches >= 30


def test_svd_points_agree_with_the_oracle_within_tau(orc, scene):
    m = scene[0]
    n = 0
    for cur, k, i1, i2, e in m.evals:
        if e["kind"] != "svd":
            continue
        G = ref.geometry(m.store[cur]["pose"], m.store[k]["pose"], m.cam)
        f1, f2 = m._feature(cur, i1), m._feature(k, i2)
        pc1, pc2 = ref._pixel2camera(m.cam, f1["u"], f1["v"], 1.0), ref._pixel2camera(m.cam, f2["u"], f2["v"], 1.0)
        T1f = np.array([[G["T1"][3 * r], G["T1"][3 * r + 1], G["T1"][3 * r + 2], G["T1"][9 + r]] for r in range(3)], f32).reshape(-1)
        T2f = np.array([[G["T2"][3 * r], G["T2"][3 * r + 1], G["T2"][3 * r + 2], G["T2"][9 + r]] for r in range(3)], f32).reshape(-1)
        o = np.zeros(3, f32)
        assert orc.lib().orc_triangulate(np.array(pc1[:2], f32), np.array(pc2[:2], f32), T1f, T2f, o) == 1
        assert np.abs(o - np.array(e["p"])).max() <= ref.TAU * max(1.0, np.abs(o).max())
        n += 1
    assert n >= 100


def test_f12_annihilates_projections_of_common_points():
    """x1^T F12 x2 = 0 for the projections of a world point into the two cameras (float64, independent of the model's order)"""
    rng = np.random.default_rng(3)
    for _ in range(20):
        T1, T2 = ni.se3(rng.normal(0, 0.2, 3), rng.normal(0, 1, 3)), ni.se3(rng.normal(0, 0.2, 3), rng.normal(0, 1, 3))
        G = ref.geometry(T1, T2, ni.CAM6)
        F = np.array(G["F"]).reshape(3, 3)
        K = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1.0]])
        for _ in range(10):
            P = rng.uniform(-2, 2, 3) + np.array([0, 0, 8.0])
            x = [K @ (np.array(T[:9]).reshape(3, 3) @ P + np.array(T[9:])) for T in (T1, T2)]
            x = [v / v[2] for v in x]
            scale = np.abs(F).max() * np.linalg.norm(x[0]) * np.linalg.norm(x[1])
            assert abs(x[0] @ F @ x[1]) < 1e-9 * scale
        # the centres and the epipole
        R1, t1, R2, t2 = np.array(T1[:9]).reshape(3, 3), np.array(T1[9:]), np.array(T2[:9]).reshape(3, 3), np.array(T2[9:])
        assert np.allclose(G["Ow1"], -R1.T @ t1, atol=1e-12) and np.allclose(G["Ow2"], -R2.T @ t2, atol=1e-12)
        c2 = K @ (R2 @ (-R1.T @ t1) + t2)
        assert abs(float(G["ex"]) - c2[0] / c2[2]) <= 1e-6 * max(1.0, abs(c2[0] / c2[2]))
        assert abs(float(G["bl"]) - np.linalg.norm(R1.T @ t1 - R2.T @ t2)) < 1e-6


def test_created_points_reproject_inside_their_gates(scene):
    """every created point, in both key-frames: z > 0 and the chi-square of the reprojection (float64, written independently of
    gates()) below 5.991 / 7.815 at the feature's scale"""
    m = scene[0]
    n = 0
    for cur, k, i1, i2, e in m.evals:
        if not e["accepted"]:
            continue
        for kf, i in ((cur, i1), (k, i2)):
            T = np.array(m.store[kf]["pose"])
            pc = T[:9].reshape(3, 3) @ np.array(e["p"]) + T[9:]
            f = m._feature(kf, i)
            u, v = 500.0 * pc[0] / pc[2] + 320.0, 500.0 * pc[1] / pc[2] + 240.0
            chi2 = ((u - float(f["u"])) ** 2 + (v - float(f["v"])) ** 2) / float(ni.SF[f["octave"]]) ** 2
            gate = 5.991
            if f["ur"] >= 0:
                chi2 += (u - 40.0 / pc[2] - float(f["ur"])) ** 2 / float(ni.SF[f["octave"]]) ** 2
                gate = 7.815
            assert pc[2] > 0 and chi2 < gate
            n += 1
    assert n >= 300


def test_two_holder_descriptor_rule_is_the_median_loop(scene):
    """computeDescriptor with two holders, in ascending key-frame number: int(0.5 * 1) = 0, both medians are the 0 of the
    diagonal, the strict test keeps index 0 -- the lower-numbered key-frame's descriptor, whatever the two descriptors are"""
    rng = np.random.default_rng(0)
    for _ in range(50):
        a, b = rng.integers(0, 256, 32, dtype=np.uint8), rng.integers(0, 256, 32, dtype=np.uint8)
        assert ref.median_descriptor([a, b]) == 0 and ref.median_descriptor([a, a]) == 0
    m = scene[0]
    for cur, k, i1, i2, e in m.evals[:200]:
        if e["accepted"] and m.store[cur]["ids"][i1] == m.store[k]["ids"][i2]:   # (not overwritten by a later step)
            lo, ilo = (cur, i1) if cur < k else (k, i2)
            assert m.store[cur]["pdesc"][i1].tobytes() == m.store[lo]["desc"][ilo].tobytes()


def test_no_gpu_script_has_a_match_that_is_not_decisive(scene, hand):
    for name, m in _gpu_models(scene, hand):
        assert [(cur, k, i1, i2) for cur, k, i1, i2, e in m.evals if not e["decisive"]] == [], name


def test_random_scene_is_not_vacuous(scene):
    ni.assert_not_vacuous(scene[0])
    m, snaps = scene
    assert len(snaps) == 3 and all(s["result"]["created"] for s in snaps)
    # the sequential dependence shows: a later neighbour's search starts from flags an earlier one's points set
    assert any(sum(a) > sum(m.searches[0][2]) for cur, k, a, *_ in m.searches[1:10])


@pytest.mark.parametrize("case", ni.hand_cases(), ids=lambda c: c["name"])
def test_hand_made_case_on_the_model(case):
    m, snaps = ni.run_model(case["script"])
    assert case["check"](snaps)
    assert m.sticky == case.get("sticky", 0)
    if "rejects" in case:   # case e: which gate rejected which match
        assert [(k, e["signature"]) for _, k, _, _, e in m.evals] == case["rejects"]


def test_case_a_differs_from_independent_searches():
    """neighbour 1 searched against the flags the call started with (what vo_match_triangulation_batch does) matches c0 to b0
    and leaves c1 alone; the sequential call gives b0 to c1"""
    case = [c for c in ni.hand_cases() if c["name"].startswith("a_")][0]
    m, snaps = ni.run_model(case["script"][:-1])
    G = ref.geometry(m.store[2]["pose"], m.store[1]["pose"], m.cam)
    a_has, b_has = [f & 1 for f in m.store[2]["flags"]], [f & 1 for f in m.store[1]["flags"]]
    match12, cnt, _ = ref.search(m._view(2), m._view(1), a_has, b_has, G["F"], G["ex"], G["ey"], m.sf)
    a = case["a"]
    assert (match12[a["c0"]], match12[a["c1"]], cnt) == (a["b0"], -1, 1)
    m.create(2, 10)
    assert [(k, i1, i2) for k, i1, i2, _ in m.np_result["created"]][1] == (1, a["c1"], a["b0"])


def test_triangulation_fixture_matches_its_inputs():
    """tests/golden/new_points_triangulate.npz holds vo_triangulate's output on tests/test_gpu_loop.py's inputs, recorded
    before the arithmetic moved into csrc/triangulate.h: the shapes fit the inputs and the points are the scene's"""
    import pathlib
    g = np.load(pathlib.Path(__file__).resolve().parent / "golden" / "new_points_triangulate.npz")
    xn1, xn2, T1, T2s = ni.triangulation_inputs()
    assert g["points"].shape == (len(xn1), 3) and g["ok"].shape == (len(xn1),) and g["ok"].all() and g["one"].shape == (4, 3)
    z = g["points"][:, 2]
    assert 1.9 < z.min() and z.max() < 7.1 and math.isfinite(float(g["points"].sum()))
