"""The end-to-end fixture of tests/test_gpu_reloc_db.py on the CPU models alone: kfdb_ref chooses every frame's candidates
from the database built by tests/reloc_db_inputs.py, reloc_ref walks them.  Asserts that the fixture is worth running."""
import pytest

import reloc_db_inputs
import reloc_inputs
import reloc_ref


@pytest.fixture(scope="module")
def fx(orc):
    return reloc_inputs.build(orc)


def test_database_fixture_walks_the_branches(orc, fx):
    kfs, lists = reloc_db_inputs.db_keyframes(orc, fx)
    db = reloc_db_inputs.database(orc, fx, kfs, lists)
    chosen = reloc_db_inputs.model_candidates(db)
    res = []
    for f, fr in enumerate(fx["frames"]):
        k, d, ux, uy, ur, _ = fr
        cands, _ = reloc_db_inputs.dense_ids([kfs[g] for g in chosen[f]])
        r = reloc_ref.relocalize(orc, k, d, ux, uy, ur, fx["fnodes"][f], cands, fx["cam5"], fx["sf"])
        print(f, "chosen", chosen[f], "own", lists[f], "winner", r["winner"], "code", r["code"], r["trace"])
        res.append(r)
    assert any(len(c) >= 2 for c in chosen), "a frame that receives two candidates or more"
    assert any(r["winner"] > 0 for r in res), "a frame that succeeds on a candidate that is not its first"
    assert any(r["winner"] < 0 and len(r["code"]) > 0 for r in res), "a frame whose candidates all fail"
    traces = [tuple(t) for r in res for t in r["trace"]]
    has = lambda pred: any(pred(t) for t in traces)
    assert has(lambda t: "success" in t and "top_up_1" not in t), "success straight after the first solve"
    assert has(lambda t: "success" in t and "solve_2" in t and "top_up_2" not in t), "success through the first top-up only"
    assert has(lambda t: "bad" in t) and has(lambda t: "few_bow" in t) and has(lambda t: "few_solve" in t)
    assert has(lambda t: "few_pnp_leak" in t), "a candidate rejected with 0 < PnP inliers < 10"
    assert has(lambda t: "success" in t and "solve_3" in t), "success through both top-ups"
