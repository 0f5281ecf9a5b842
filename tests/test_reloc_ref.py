"""The relocalisation model (tests/reloc_ref.py) on the seeded fixture (tests/reloc_inputs.py), CPU only: the batch must walk
every branch of visualOdometry.cpp:313-395, and the invariants that need no device must hold."""
import numpy as np
import pytest

import reloc_inputs
import reloc_ref


@pytest.fixture(scope="module")
def walked(orc):
    fx = reloc_inputs.build(orc)
    out = []
    for f, fr in enumerate(fx["frames"]):
        k, d, ux, uy, ur, _ = fr
        out.append(reloc_ref.relocalize(orc, k, d, ux, uy, ur, fx["fnodes"][f], fx["candidates"][f], fx["cam5"], fx["sf"]))
    return fx, out


def test_every_branch_is_walked(walked):
    fx, res = walked
    traces = [tuple(t) for r in res for t in r["trace"]]
    has = lambda pred: any(pred(t) for t in traces)
    for r in res:
        print(r["winner"], r["inliers"], r["bow"], r["pnp"], r["code"], r["trace"], r["steps"])
    assert has(lambda t: "success" in t and "top_up_1" not in t), "success straight after the first solve"
    assert has(lambda t: "success" in t and "solve_2" in t and "top_up_2" not in t), "success through the first top-up only"
    assert has(lambda t: "bad" in t) and has(lambda t: "few_bow" in t) and has(lambda t: "few_solve" in t)
    assert has(lambda t: "few_pnp_leak" in t), "a candidate rejected with 0 < PnP inliers < 10"
    lk = res[reloc_inputs.LEAK_FRAME]
    assert lk["code"][reloc_inputs.LEAK_CAND] == reloc_ref.FEW_PNP and lk["winner"] > reloc_inputs.LEAK_CAND
    assert (lk["ids"] >= fx["nk"]).any(), "the winner's frame holds an id only the rejected candidate could have supplied"
    assert any(r["winner"] < 0 and len(r["code"]) > 0 for r in res), "a frame whose candidates all fail"
    assert any(len(r["code"]) == 0 for r in res), "a frame with zero candidates"
    assert has(lambda t: "success" in t and "solve_3" in t), "success through both top-ups"


def test_walk_invariants(walked):
    _, res = walked
    for r in res:
        code = r["code"]
        wins = np.nonzero(code == reloc_ref.SUCCESS)[0]
        if r["winner"] >= 0:
            assert wins[0] == r["winner"] and (code[r["winner"] + 1:] == reloc_ref.NOT_REACHED).all() and r["inliers"] >= 50
            assert (code[:r["winner"]] != reloc_ref.NOT_REACHED).all()
        else:
            assert len(wins) == 0 and (code != reloc_ref.NOT_REACHED).all()
