"""The CPU model of trackLocalMap behind a relocalisation (tests/reloc_local_ref.py) on the relocalisation fixture
(tests/reloc_inputs.py): the id skip, the count, and the empty-map property."""
import numpy as np
import pytest

import reloc_inputs
import reloc_ref
from reloc_local_ref import local_map_after_reloc, make_local_map

FRAME = 1  # relocalises through the first top-up


@pytest.fixture(scope="module")
def case(orc):
    fx = reloc_inputs.build(orc, n_frames=FRAME + 1)
    fr = fx["frames"][FRAME]
    end = reloc_ref.relocalize(orc, fr[0], fr[1], fr[2], fr[3], fr[4], fx["fnodes"][FRAME], fx["candidates"][FRAME], fx["cam5"], fx["sf"])
    assert end["winner"] >= 0
    return fx, fr, end


def test_local_points_the_frame_holds_are_skipped(orc, case):
    fx, fr, end = case
    local = make_local_map(fr, end, fx["cam5"])
    all_obs = lambda ids: np.ones(len(ids), bool)
    got = local_map_after_reloc(orc, fr, end, all_obs, local, fx["cam5"], fx["sf"])
    held = set(int(i) for i in end["ids"][(end["ids"] >= 0) & (end["outlier"] == 0)])
    n_held = sum(int(i) in held for i in local["ids"])
    assert got["n_skipped"] == n_held >= 20 and got["n_searched"] >= 20
    claimed = got["assigned_local"][got["assigned_local"] >= 0]
    assert len(claimed) == got["n_local"] > 0
    assert not any(int(local["ids"][a]) in held for a in claimed)   # a skipped point is never assigned
    assert got["n_tracked"] <= got["inliers"]
    # without ids nothing is skipped: the held points are searched too (their slots are occupied, so few are found)
    free = local_map_after_reloc(orc, fr, end, all_obs, dict(local, ids=None), fx["cam5"], fx["sf"])
    assert free["n_skipped"] == 0 and free["n_searched"] == len(local["valid"])
    # observed on half of the ids: fewer slots are occupied, so the search finds more, and fewer inliers count
    half = local_map_after_reloc(orc, fr, end, lambda ids: ids % 2 == 0, local, fx["cam5"], fx["sf"])
    assert half["n_local"] > got["n_local"] and half["n_tracked"] <= half["inliers"]


def test_empty_local_map_is_a_re_solve_of_the_end_state(orc, case):
    fx, fr, end = case
    k, d, ux, uy, ur = fr[:5]
    empty = dict(points=np.zeros((0, 3)), normals=np.zeros((0, 3)), min_dist=np.zeros(0, np.float32), max_dist=np.zeros(0, np.float32),
                 valid=np.zeros(0, np.uint8), desc=np.zeros((0, 32), np.uint8), ids=np.zeros(0, np.int32))
    observed = lambda ids: ids % 3 != 0
    got = local_map_after_reloc(orc, fr, end, observed, empty, fx["cam5"], fx["sf"])
    idx = np.nonzero(end["ids"] >= 0)[0]
    pr = dict(pts=np.ascontiguousarray(end["points"][idx]), obs=np.ascontiguousarray(np.stack([ux[idx], uy[idx], ur[idx]], 1).astype(np.float64)),
              inv_sigma=np.ascontiguousarray(1.0 / fx["sf"][k["octave"][idx]].astype(np.float64)), cam=np.asarray(fx["cam5"], np.float64),
              pose0=np.asarray(end["pose"], np.float64).copy())
    pose, o, ninl, _, _ = orc.pose_only(pr)
    o = np.asarray(o, bool)
    assert got["n_local"] == 0 and (got["assigned_local"] == -1).all()
    assert np.array_equal(got["pose"], np.asarray(pose)) and got["inliers"] == ninl
    assert got["n_tracked"] == int(observed(end["ids"][idx[~o]]).sum()) <= got["inliers"]
