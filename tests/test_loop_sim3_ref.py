"""The conditions tests/test_gpu_loop_sim3.py rests on, checked on the CPU with the model alone (tests/loop_sim3_ref.py over the
oracle): every scenario of tests/loop_sim3_inputs.py reaches the branch it is named after -- proved from the model's log --,
every float gate of every scenario decides with a margin above the floors of loop_sim3_ref.FLOORS, the results do not depend
on how rounds are split, and the library's ransacMaxIters equals the reference's formula evaluated in Python.

The floors.  The device's Sim3 agrees with the model's within 1e-8 (the bound of the GPU test).  A pose off by 1e-8 moves a pixel
by about 1e-5 at these focal lengths and depths, a squared error e^2 by 2 |e| 1e-5 <~ 2e-4 px^2 for |e| <~ 7 px: the RANSAC and
chi-square floors of 1e-3 leave room.  Pixels, depths and distances move by less than 1e-5: the floors of z, isInImg and the
window radius are 1e-3, those of the relative distance gates and the cosine 1e-4, a cell boundary (1 / 10 cell per pixel) 1e-4
cells, the predicted level 1e-3 levels.  The 0.75 ratio test compares two integers in float: both sides decide it exactly."""
import numpy as np
import pytest

import loop_sim3_inputs as li
import oracle_lib as orc
from loop_sim3_ref import (ACCEPTED, BAD, FEW_MATCHES, FLOORS, LIVE, NO_MATCH, REJECTED, STICKY_CAPACITY, STICKY_RAND_SHORT, STOPPED,
                           UNDECIDED, ransac_max_iters)


@pytest.fixture(scope="module")
def models():
    return {name: li.run_model(orc, li.scene(name)) for name in li.SCENARIOS}


def _kinds(m, kind):
    return [e for e in m.log if e[0] == kind]


def test_every_gate_decides_with_a_margin(models):
    worst = {}
    for name, m in models.items():
        for kind, v in m.margin.items():
            if v < worst.get(kind, (np.inf, ""))[0]:
                worst[kind] = (v, name)
    print("smallest margins:", {k: (float(f"{v:.3g}"), n) for k, (v, n) in worst.items()})
    assert set(worst) == set(FLOORS)          # every kind of gate was met
    for kind, (v, name) in worst.items():
        assert v >= FLOORS[kind], (kind, v, name)


def test_a_success_at_the_first_iterate(models):
    m = models["accepted"]
    r = m.result()
    assert r["state"] == ACCEPTED and r["rounds"] == 1 and r["verifications"] == 1 and r["rand_used"] == 3
    assert [e[0] for e in m.log] == ["front", "construct", "trip", "return", "verify", "match", "loop_points", "projection"]
    assert r["match_cnt"] >= 40 and _kinds(m, "projection")[0][1] > 0          # searchByProjection claimed features


def test_a_bad_candidate_one_with_19_matches_and_one_that_wins(models):
    m = models["three_candidates"]
    assert [e[2:] for e in _kinds(m, "front")] == [(BAD, 0), (FEW_MATCHES, 19), (LIVE, 30)]
    r = m.result()
    assert r["state"] == ACCEPTED and r["match_pos"] == 2 and [p["reason"] for p in r["per_candidate"][:3]] == [BAD, FEW_MATCHES, LIVE]


def test_correspondences_below_20_behind_enough_matches(models):
    m = models["filtered_below_20"]
    r = m.result()
    assert _kinds(m, "front")[0][2:] == (LIVE, 25) and _kinds(m, "construct")[0][2] < 20
    assert ("stop", 0) in m.log and r["state"] == NO_MATCH and r["per_candidate"][0]["reason"] == STOPPED and r["rand_used"] == 0


def test_a_solver_runs_out_while_another_keeps_walking(models):
    m = models["outliers_only"]
    r = m.result()
    p0, p1 = r["per_candidate"][:2]
    assert p0["reason"] == STOPPED and p0["iterations"] == p0["max_iters"] == 3 and p0["inliers_best"] <= 20
    stop = m.log.index(("stop", 0))
    assert [e for e in m.log[stop:] if e[0] == "trip" and e[1] == 1], "the other candidate walks on behind the stop"
    assert p1["iterations"] > 1 and r["state"] == ACCEPTED and r["match_pos"] == 1


def test_a_failed_verification_and_a_later_winner(models):
    m = models["fails_then_wins"]
    v = _kinds(m, "verify")
    assert len(v) == 2 and v[0][1] == 0 and v[0][4] < 20 and v[0][5] == 2 and v[1][1] == 1 and v[1][4] >= 20
    assert _kinds(m, "return")[0][2] > 20                                       # more than 20 became fewer than 20
    assert m.log[m.log.index(v[0]) + 1] == ("resume",)
    r = m.result()
    assert r["state"] == ACCEPTED and r["match_pos"] == 1 and r["rounds"] == 2 and r["per_candidate"][0]["reason"] == LIVE


def test_matched_but_below_40(models):
    r = models["rejected"].result()
    assert r["state"] == REJECTED and r["refine_inliers"] >= 20 and r["match_cnt"] < 40 and r["match_pos"] == 0


@pytest.mark.parametrize("n", [63, 65, 255, 257])
def test_wave_and_block_edges(models, n):
    r = models[f"n{n}"].result()
    assert r["per_candidate"][0]["n"] == n and r["state"] == ACCEPTED


def test_free_scale(models):
    r = models["free_scale"].result()
    assert r["state"] == ACCEPTED and r["Scm"][12] != 1.0 and abs(r["Scm"][12] - 1.0) < 1e-2


def test_rounds_can_be_split():
    sc = li.scene("fails_then_wins")
    whole = li.run_model(orc, sc).result()
    m = li.run_model(orc, sc, max_rounds=1)
    assert m.result()["state"] == UNDECIDED and m.sticky == 0 and m.log[-1] == ("undecided",)
    m.continue_(1)
    split = m.result()
    assert split["state"] == ACCEPTED and split["rounds"] == whole["rounds"] and split["Scw"].tobytes() == whole["Scw"].tobytes()
    assert np.array_equal(split["match_ids"], whole["match_ids"])


def test_rand_values_one_short_and_loop_points_one_short():
    sc = li.scene("outliers_only")
    need = li.run_model(orc, sc).result()["rand_used"]
    m = li.run_model(orc, sc, rand=sc["rand"][:need - 1])
    assert m.result()["state"] == UNDECIDED and m.sticky == STICKY_RAND_SHORT and m.result()["rand_used"] == need - 3
    sc = li.scene("accepted")
    n = li.run_model(orc, sc).result()["n_loop_points"]
    m = li.run_model(orc, sc, max_loop_points=n - 1)
    assert m.result()["state"] == UNDECIDED and m.sticky == STICKY_CAPACITY


def test_the_tabulated_ransac_iterations_equal_the_formula(vo):
    f = vo.lib().vo_kfstore_loop_ransac_max_iters
    got = [f(N) for N in range(20, 401)]
    assert got == [ransac_max_iters(N) for N in range(20, 401)]
    below = [N for N in range(20, 401) if got[N - 20] < 300]
    print("ransacMaxIters below 300 for N =", below[0], "..", below[-1], "; first N at the cap:", below[-1] + 1)
    assert got[0] == 1 and got[1] == 3 and below == list(range(20, below[-1] + 1)) and 70 <= below[-1] <= 90   # the cap is reached near 80
    assert all(f(N) == 1 for N in range(0, 21))
